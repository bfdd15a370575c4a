"""CPU: ``python bench.py --gpus N`` (the driver's command shape) starts N ranks by itself — rendezvous on 127.0.0.1, one
JSON line from rank 0, exit code relayed — and refuses a --gpus / WORLD_SIZE mismatch.  (The ranks' GPU work is replaced by
a gloo all-reduce through ASIS_BENCH_RANKCHECK: there is no GPU in the build container.)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True,
                          timeout=600)


def test_bench_self_launches_n_ranks():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"ASIS_BENCH_RANKCHECK": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j == {"rankcheck": True, "n_gpus": 2, "n_ranks_seen": 2, "sum": 2.0}


def test_bench_refuses_world_size_mismatch():
    r = _run(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_bench_refuses_zero_steps():
    r = _run(["--gpus", "1", "--steps", "0"], {})
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dump_outputs_files_budget_and_fixed_sample(tmp_path):
    """``bench.dump_outputs`` on CPU stand-ins of the engine's flat buckets: one float32 .npy per output, small arrays whole,
    a large one as the same seeded sample on every call, all within the 64 MB budget."""
    import types

    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench

    def bucket(n, seed):
        g = torch.Generator().manual_seed(seed)
        return types.SimpleNamespace(flat=torch.rand(n, generator=g), grad=torch.rand(n, generator=g))

    dec, vit = bucket(1000, 1), bucket(8_000_000, 2)
    eng = types.SimpleNamespace(bucket=dec, vit_bucket=vit, optimizer=types.SimpleNamespace(buckets=[dec]))
    for d in ("a", "b"):
        bench.dump_outputs(eng, torch.tensor(0.25), str(tmp_path / d))
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["backbone_grad.npy", "decoder_grad.npy", "decoder_weights.npy", "loss.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64_000_000
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float32 and np.array_equal(x, y), n
    assert np.array_equal(np.load(tmp_path / "a" / "decoder_grad.npy"), dec.grad.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "decoder_weights.npy"), dec.flat.numpy())
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [0.25]
    sample = np.load(tmp_path / "a" / "backbone_grad.npy")
    assert 0 < sample.size < vit.grad.numel()


def _main_with_unwritable_build_dir(monkeypatch, lib_path):
    """bench.main() up to its GPU check, with build_library() failing as it does in a tree this user may not write."""
    import pytest
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from adaptersis_amd import build

    def refuse(*_a, **_k):
        raise PermissionError(13, "Permission denied", os.path.join(build.OBJ, ".lock"))

    monkeypatch.setattr(build, "build_library", refuse)
    monkeypatch.setattr(build, "LIB", lib_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "ASIS_BENCH_RANKCHECK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0"])
    return pytest, bench


def test_bench_runs_the_built_library_when_the_build_dir_is_not_writable(monkeypatch, tmp_path, capsys):
    lib = tmp_path / "libasis_hip.so"
    lib.write_bytes(b"")
    pytest, bench = _main_with_unwritable_build_dir(monkeypatch, str(lib))
    with pytest.raises(SystemExit, match="needs an MI355X"):   # got past the build step to the device check
        bench.main()
    assert "not writable" in capsys.readouterr().err


def test_bench_without_a_built_library_still_fails(monkeypatch, tmp_path):
    pytest, bench = _main_with_unwritable_build_dir(monkeypatch, str(tmp_path / "missing.so"))
    with pytest.raises(PermissionError):
        bench.main()
