"""CPU: test-time augmentation of ``adaptersis_amd.predict`` — the view plan (``plan_views``), the new arguments, argument errors
raised before any file is read or any model is built, and the argument errors of ``asis_predict_mask_views`` that need no GPU."""
import ctypes

import pytest

from adaptersis_amd import _lib
from adaptersis_amd import predict as P


def test_plan_views_order_duplicates_and_default():
    assert P.plan_views(588, None, False) == [(588, False)]
    assert P.plan_views(588, None, True) == [(588, False), (588, True)]
    assert P.plan_views(224, [448, 224], True) == [(224, False), (224, True), (448, False), (448, True)]
    assert P.plan_views(224, [448, 224, 448, 224, 336], False) == [(224, False), (336, False), (448, False)]
    assert P.plan_views(224, [518], False) == [(518, False)]                      # --imsize is not added to --tta_sizes
    assert len(P.plan_views(14, [14 * k for k in range(1, 5)], True)) == 8        # 8 views are allowed
    assert len(P.plan_views(14, [14 * k for k in range(1, 9)], False)) == 8


def test_plan_views_errors():
    with pytest.raises(ValueError, match="9 views"):
        P.plan_views(14, [14 * k for k in range(1, 10)], False)
    with pytest.raises(ValueError, match="10 views"):
        P.plan_views(14, [14 * k for k in range(1, 6)], True)
    for bad in ([0], [224, -14], [224, 0, 448]):
        with pytest.raises(ValueError, match="positive input size"):
            P.plan_views(224, bad, False)
    with pytest.raises(ValueError, match="positive input size"):
        P.plan_views(0, None, True)


def _args(tmp_path, *extra):
    return P.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", "224", "--output_dir", str(tmp_path / "nowhere"),
                                           "--input", str(tmp_path), "--pred_dir", str(tmp_path / "pred"), *extra])


def test_parser_accepts_the_new_flags(tmp_path):
    a = _args(tmp_path)
    assert a.tta_flip is False and a.tta_sizes is None and a.confidence is False
    assert P.views_of(a) is None                                                  # no flag: SegEngine.predict, as before
    a = _args(tmp_path, "--tta_flip", "--tta_sizes", "448", "224", "--confidence")
    assert a.tta_flip is True and a.tta_sizes == [448, 224] and a.confidence is True
    assert P.views_of(a) == [(224, False), (224, True), (448, False), (448, True)]
    assert P.views_of(_args(tmp_path, "--confidence")) == [(224, False)]          # the confidence comes from the new op
    assert P.views_of(_args(tmp_path, "--tta_flip")) == [(224, False), (224, True)]
    assert P.views_of(_args(tmp_path, "--tta_sizes", "224")) == [(224, False)]


def test_argument_errors_come_before_files_and_model(tmp_path):
    """--input is an empty directory and there is no checkpoint: the error must be the one of the sizes."""
    with pytest.raises(ValueError, match="positive input size"):
        P.predict_seg(_args(tmp_path, "--tta_sizes", "224", "0"))
    with pytest.raises(ValueError, match="16 views"):
        P.predict_seg(_args(tmp_path, "--tta_flip", "--tta_sizes", *[str(14 * k) for k in range(1, 9)]))
    assert not (tmp_path / "pred").exists()
    with pytest.raises(ValueError, match="no frames"):                            # valid views: the empty input is what is wrong
        P.predict_seg(_args(tmp_path, "--tta_flip", "--tta_sizes", "224", "448"))


def _call(K=2, null_view=None, B=1, C=3, H=8, W=8, hs=(4, 5), ws=(4, 5), frames=False, overlay=False, target=False, counts=None):
    """asis_predict_mask_views with made-up non-null addresses: every case here is refused before anything is launched."""
    lib = _lib.lib()
    a = 4096
    n = max(K, 1)
    ptrs = (ctypes.c_void_p * n)(*[None if k == null_view else a for k in range(n)])
    h = (ctypes.c_int * n)(*[hs[k % len(hs)] for k in range(n)])
    w = (ctypes.c_int * n)(*[ws[k % len(ws)] for k in range(n)])
    f = (ctypes.c_int * n)(*[k & 1 for k in range(n)])
    return lib.asis_predict_mask_views(None, ptrs, h, w, f, K, B, C, H, W, a, a, None, a if frames else None, a if frames else None,
                                       a if frames else None, a if overlay else None, a if target else None,
                                       a if target else None, counts)


@pytest.mark.parametrize("kw,msg", [
    (dict(K=0), "K=0"), (dict(K=9), "K=9"), (dict(null_view=1), r"logits\[1\]"), (dict(C=17), "C=17"), (dict(C=0), "C=0"),
    (dict(B=65536), "65535"), (dict(H=16385), "16384"), (dict(W=0), "non-positive"), (dict(hs=(4, 16385)), "hs=16385"),
    (dict(ws=(0, 4)), "ws=0"), (dict(overlay=True), "overlay requested without frames"),
    (dict(counts=4096), "counts requested without"), (dict(counts=4100, target=True), "8-byte aligned")])
def test_abi_argument_errors_without_a_gpu(kw, msg):
    rc = _call(**kw)
    assert rc == _lib.ASIS_EINVAL
    with pytest.raises(ValueError, match=msg):
        _lib.check(rc, "asis_predict_mask_views")
