"""The message lines of GMRES, RGMRES and LGMRES: text, count and order.

The golden runs (tests/test_gpu_parity.py) pin every number of these drivers;
the lines they print are pinned here, as tests/test_gpu_rlgmres.py does for
RLGMRES.  One set-up for all three: 7-pt Poisson 8^3, no preconditioner, b = 1,
x0 = 0, restart 4, at most 9 iterations.  That gives more than one cycle, a
stop at maxit in mid-cycle for the driver that tests it there, and LGMRES's
first augmented cycle (5 columns).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


def _lines(dev, solver):
    import lssp_amd
    lines = []
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p)
    cb = CB(lambda user, msg: lines.append(msg.decode()) or 0)
    L = lssp_amd._lib.load()
    Ap, Aj, Ax = lssp_amd.poisson(3, 8)
    n = Ap.size - 1
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    x, b = dev.vec(n, np.zeros(n)), dev.vec(n, np.ones(n))
    L.lssp_amd_set_print(ctypes.cast(cb, ctypes.c_void_p), None)
    try:
        r = lssp_amd.solve(dev, A, None, x, b, solver=solver, restart=4, maxit=9, verb=2)
    finally:
        L.lssp_amd_set_print(None, None)
    A.close()
    print("".join(lines), r.nits, repr(r.residual))
    return r, lines


def _check_frame(lines, r, head, nits):
    """the header lines first, the two footer lines last, the last residual printed is the one returned"""
    k = len(head)
    assert lines[:k] == head
    pre = head[0].split(":")[0]
    assert lines[k:k + 4] == [f"{pre}: maximal iteration: 9\n", f"{pre}: tolerance abs: 1e-07\n",
                              f"{pre}: tolerance rel: 1e-07\n", f"{pre}: tolerance rbn: 1e-07\n"]
    assert lines[-2] == f"{pre}: total iteration: {nits}\n"
    assert lines[-1].startswith(f"{pre}: total time: ")
    float(lines[-1].split("total time:")[1])
    its = lines[k + 4:-2]
    assert r.nits == nits
    res = float(its[-1].split("abs res:")[1].split(",")[0])
    assert res == float(f"{r.residual:.6e}")
    return its


def test_gmres_verbose_lines(dev):
    """one line per cycle, both counters the inner count; maxit is not tested inside a cycle: 3 full cycles"""
    import lssp_amd
    r, lines = _lines(dev, lssp_amd.GMRES)
    its = _check_frame(lines, r, ["gmres: restart parameter m: 4\n"], 12)
    assert all(ln.startswith("gmres: itr: ") and ", rel res: " in ln and ", rbn: " in ln for ln in its)
    assert [ln.split(", abs res:")[0] for ln in its] == ["gmres: itr: %4d / %5d" % (k, k) for k in (4, 8, 12)]


def test_rgmres_verbose_lines(dev):
    """gmres: header and footer, one rgmres: line per step with a single counter; stops at maxit in mid-cycle"""
    import lssp_amd
    r, lines = _lines(dev, lssp_amd.RGMRES)
    its = _check_frame(lines, r, ["gmres: restart parameter m: 4\n"], 9)
    assert all(ln.startswith("rgmres: itr: ") and ", rel res: " in ln and ", rbn: " in ln for ln in its)
    assert [ln.split(", abs res:")[0] for ln in its] == ["rgmres: itr: %4d" % k for k in range(1, 10)]


def test_lgmres_verbose_lines(dev):
    """one line per cycle with (outer, inner): a cycle of 4, then the first augmented cycle of 5 columns"""
    import lssp_amd
    r, lines = _lines(dev, lssp_amd.LGMRES)
    its = _check_frame(lines, r, ["lgmres: restart parameter m: 4\n", "lgmres: aug k: 3\n"], 9)
    assert all(ln.startswith("lgmres: itr: ") and ", rel res: " in ln and ", rbn: " in ln for ln in its)
    assert [ln.split(", abs res:")[0] for ln in its] == ["lgmres: itr: %4d / %5d" % p for p in ((0, 4), (1, 9))]
