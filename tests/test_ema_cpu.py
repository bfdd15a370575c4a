"""CPU: the decay schedule of ``optim.EMA`` restated on the host, its argument check, the script flags and the argument errors
of the two ABI entries of csrc/ema.hip (reported before any launch, so without a device)."""
import ctypes

import pytest
import torch

from adaptersis_amd import _lib, optim


@pytest.mark.parametrize("warmup", [True, False])
def test_decay_schedule_against_the_formula(warmup):
    for decay in (0.5, 0.9, 0.999, 0.9999):
        for t in range(1, 51):
            want = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
            assert optim.ema_decay_at(t, decay, warmup) == want
    # the warm-up is what rules early and the decay late
    assert optim.ema_decay_at(1, 0.999, True) == 2.0 / 11.0 and optim.ema_decay_at(50, 0.5, True) == 0.5
    with pytest.raises(ValueError):
        optim.ema_decay_at(0, 0.9, True)


class _Bucket:
    """what ``optim.EMA`` reads of a ``FlatBucket`` before it allocates anything"""
    momentum = torch.zeros(4)
    flat = torch.zeros(4)
    numel = 4


@pytest.mark.parametrize("decay", [0.0, 1.0, -0.1, 1.5, float("nan")])
def test_decay_outside_the_open_interval_raises(decay):
    with pytest.raises(ValueError, match="decay"):
        optim.EMA([_Bucket()], decay)


def test_gradient_only_buckets_are_not_averaged():
    class GradOnly(_Bucket):
        momentum = None
    with pytest.raises(ValueError, match="no bucket"):
        optim.EMA([GradOnly()], 0.9)


def test_parsers_accept_the_flags_and_default_to_off():
    from adaptersis_amd import predict, train, train_mla, train_multi_class
    for mod in (train, train_mla, train_multi_class):
        p = mod.get_args_parser()
        a = p.parse_args([])
        assert a.ema_decay is None and a.ema_no_warmup is False and a.ema_validate_live is False
        assert train._ema_args(a) == {}
        a = p.parse_args(["--ema_decay", "0.999", "--ema_no_warmup", "--ema_validate_live"])
        assert a.ema_decay == 0.999 and a.ema_no_warmup is True and a.ema_validate_live is True
        assert train._ema_args(a) == {"ema_decay": 0.999, "ema_warmup": False}
        assert train._ema_args(p.parse_args(["--ema_decay", "0.9"])) == {"ema_decay": 0.9, "ema_warmup": True}
        for bad in (["--ema_decay", "1.0"], ["--ema_decay", "0"], ["--ema_no_warmup"], ["--ema_validate_live"]):
            with pytest.raises(SystemExit):
                p.parse_args(bad)
    p = predict.get_args_parser()
    assert p.parse_args(["--input", "x"]).ema is False and p.parse_args(["--input", "x", "--ema"]).ema is True


def test_abi_argument_errors_are_reported_without_a_gpu():
    lib = _lib.lib()
    state = (ctypes.c_int32 * 1)()
    rec = (ctypes.c_float * 2)()
    buf = (ctypes.c_float * 8)()
    st, rc_, b = ctypes.addressof(state), ctypes.addressof(rec), ctypes.addressof(buf)
    for args in ((None, None, rc_, 0.9, 1), (None, st, None, 0.9, 1)):
        rc = lib.asis_ema_prepare(None, *args)
        assert rc == -1 and b"asis_ema_prepare: null pointer" in lib.asis_last_error()
    for decay in (0.0, 1.0, float("nan")):
        rc = lib.asis_ema_prepare(None, None, st, rc_, decay, 1)
        assert rc == -1 and b"decay" in lib.asis_last_error()
    for args in ((None, b, 8, rc_), (b, None, 8, rc_), (b, b, 8, None)):
        rc = lib.asis_ema_update(None, *args)
        assert rc == -1 and b"asis_ema_update: null pointer" in lib.asis_last_error()
    rc = lib.asis_ema_update(None, b, b, -1, rc_)
    assert rc == -1 and b"n=-1" in lib.asis_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc, "asis_ema_update")
    assert state[0] == 0 and rec[0] == 0.0 and rec[1] == 0.0      # nothing ran
