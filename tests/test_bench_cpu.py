"""bench.py's launch contract (CPU): --gpus N > 1 starts N ranks itself."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_gpus_n_launches_n_ranks(monkeypatch):
    b = _bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--grid", "512"])
    with pytest.raises(SystemExit) as e:
        b.main()
    assert e.value.code == 7  # the launcher's exit code
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--master-addr=127.0.0.1" in cmd
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--grid", "512"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_world_size_must_match_gpus(monkeypatch):
    b = _bench()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8"])
    with pytest.raises(SystemExit) as e:
        b.main()
    assert "WORLD_SIZE=2" in str(e.value.code)


class _Vec:
    def __init__(self, a):
        self.a = a

    def download(self, n=None):
        return self.a[:n].copy()


class _Res:
    residual = 0.125


def test_dump_outputs_small_vector_whole(tmp_path):
    b = _bench()
    a = np.arange(12, dtype=np.float64)
    b.dump_outputs(str(tmp_path / "d"), _Vec(a), 10, _Res(), 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == ["residual.npy", "x.npy"]
    x = np.load(tmp_path / "d" / "x.npy")
    assert x.dtype == np.float64 and np.array_equal(x, a[:10])  # the rank's rows, not the halo
    assert np.array_equal(np.load(tmp_path / "d" / "residual.npy"), [0.125])


def test_dump_outputs_large_vector_fixed_sample(tmp_path, monkeypatch):
    """a vector above the cap is written as the same sorted sample every time,
    and the ranks share the cap: one run stays under 64 MB"""
    b = _bench()
    assert 8 * b.DUMP_MAX_ELEMS + 8 <= 64e6
    monkeypatch.setattr(b, "DUMP_MAX_ELEMS", 100)
    a = np.random.default_rng(1).uniform(-1, 1, 1000)
    for d in ("d1", "d2"):
        b.dump_outputs(str(tmp_path / d), _Vec(a), 1000, _Res(), 1, 2)
    x1, x2 = np.load(tmp_path / "d1" / "x_rank1.npy"), np.load(tmp_path / "d2" / "x_rank1.npy")
    assert x1.shape == (50,) and np.array_equal(x1, x2)
    idx = np.flatnonzero(np.isin(a, x1))
    assert idx.size == 50 and np.array_equal(a[idx], x1)  # distinct entries, in row order
    assert os.listdir(tmp_path / "d1") == ["x_rank1.npy"]  # the residual is rank 0's to write
