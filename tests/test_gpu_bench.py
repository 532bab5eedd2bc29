"""bench.py's plain run on the GPU: `--steps` sets the number of timed
iterations, run as solves of at most --solve-iters iterations each from
x0 = 0; the result line carries the headline fields and none of the --full
legs, and --dump-outputs writes what the last timed solve handed back --
bitwise what the same solve gives through the binding in this process, on an
x that an earlier solve used and that was zeroed on the device again.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_timed_solve(tmp_path):
    import lssp_amd
    N, steps, warmup, chunk = 24, 8, 2, 3  # timed solves of 3, 3 and 2 iterations
    out = tmp_path / "dump"
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--grid", str(N),
                        "--steps", str(steps), "--warmup", str(warmup), "--solve-iters", str(chunk),
                        "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["n_gpus"] == 1
    assert line["unit"] == "iters/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-3)
    for key in ("spmv", "roofline", "roofline_spmv", "config4", "cpu_baseline"):
        assert key not in line  # the --full legs

    assert sorted(os.listdir(out)) == ["residual.npy", "x.npy"]
    x = np.load(out / "x.npy")
    res = np.load(out / "residual.npy")
    assert x.dtype == np.float64 and x.shape == (N ** 3,) and res.dtype == np.float64 and res.shape == (1,)

    Ap, Aj, Ax = lssp_amd.poisson(3, N)
    n = Ap.size - 1
    dev = lssp_amd.Device(0)
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0)
    xd, bd = dev.vec(n, np.zeros(n)), dev.vec(n, np.ones(n))
    for iters in (chunk, steps % chunk):
        assert dev.L.lssp_amd_vec_set_value(dev.h, xd.ptr, n, 0.0) == 0
        want = lssp_amd.solve(dev, A, M, xd, bd, solver=lssp_amd.BICGSTAB, tol_rel=0.0, tol_abs=0.0, tol_rb=0.0,
                              maxit=iters)
    assert want.nits == steps % chunk
    assert np.array_equal(x, xd.download()) and res[0] == want.residual
    dev.close()
