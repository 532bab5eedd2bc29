"""RLGMRES (right-preconditioned LGMRES, lssp_solver_lgmres_r) on the GPU against
the reference's own runs (tests/golden/rlgmres_manifest.json, written by
make_golden_rlgmres.py from oracle/_ref/libref.so).

SERIAL reduction mode: nits, residual, every dot / norm of the trace and x are
bitwise the reference's, as tests/test_gpu_parity.py checks the other drivers.
TREE mode (the fast path): bitwise the oracle's restatement of the driver in the
same canonical reduction order (oracle/lssp_oracle.c lgmres_r, pinned to these
fixtures by tests/test_solver_params_cpu.py), and it stops where the reference's
run stops, within max(1, 5 %) iterations -- the bound of tests/test_gpu_refconv.py.
"""
import json
import math
import os

import numpy as np
import pytest

import oracle as O
from golden_util import build_matrix, case_id, fx, matches, vec

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rlgmres_manifest.json")) as _f:
    CASES = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


def _ilu_kw(pc, n):
    if pc["kind"] == "iluk":
        return dict(kind=1, level=pc["level"])
    if pc["kind"] == "ilut":
        return dict(kind=2, tol=pc["tol"], p=pc["p"])
    return dict(kind=1, level=0, blk=(n + pc["nblk"] - 1) // pc["nblk"])


def _run(dev, c, mode):
    import lssp_amd
    A = build_matrix(c["mat"])
    Ap, Aj, Ax = lssp_amd.sort_columns(A.Ap, A.Aj, A.Ax)  # lssp.cxx:173
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    M = None
    if c["pc"]["kind"] != "none":
        M = lssp_amd.DILU.create(dev, A.Ap, A.Aj, A.Ax, **_ilu_kw(c["pc"], A.n))
    b = dev.vec(A.n, vec(c["b"], A.n))
    x = dev.vec(A.n, np.zeros(A.n) if c["x0"] is None else vec(c["x0"], A.n))
    dev.set_reduction(mode)
    try:
        r = lssp_amd.solve(dev, D, M, x, b, solver=lssp_amd.RLGMRES, tol_rel=fx(c["rtol"]), tol_abs=fx(c["atol"]),
                           tol_rb=fx(c["rbtol"]), maxit=c["maxit"], restart=c["restart"], trace_cap=100000)
    finally:
        dev.set_reduction(lssp_amd.TREE)
    xh = x.download()
    if M is not None:
        M.close()
    D.close()
    return r, xh


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_rlgmres_serial_mode_trace_bitwise_vs_reference(dev, c):
    import lssp_amd
    assert c["solver"] == lssp_amd.RLGMRES
    r, xh = _run(dev, c, lssp_amd.SERIAL)
    assert r.nits == c["nits"]
    assert r.residual == fx(c["residual"])
    assert matches(c["trace"], r.trace)
    assert matches(c["x"], xh)


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_rlgmres_tree_mode_stops_with_the_reference(dev, c):
    import lssp_amd
    r, xh = _run(dev, c, lssp_amd.TREE)
    ref = c["nits"]
    assert abs(r.nits - ref) <= max(1, math.ceil(0.05 * ref))
    assert np.all(np.isfinite(xh))
    if ref < c["maxit"]:  # the reference's run converged: so must this one
        assert r.nits < c["maxit"]
        # the stop scale max(rtol ||r0||, atol, rb ||b||) (solver-lgmres.cxx:406-410); the trace
        # opens with norm(rhs), norm(r0)
        tol = max(fx(c["rtol"]) * r.trace[1], fx(c["atol"]), fx(c["rbtol"]) * r.trace[0])
        assert r.residual <= tol


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_rlgmres_tree_mode_bitwise_vs_oracle(dev, c):
    import lssp_amd
    r, xh = _run(dev, c, lssp_amd.TREE)
    A = build_matrix(c["mat"])
    pc = c["pc"]
    L = U = None
    if pc["kind"] == "iluk":
        L, U = O.ilu(A, "iluk", level=pc["level"])
    elif pc["kind"] == "ilut":
        L, U = O.ilu(A, "ilut", tol=pc["tol"], p=pc["p"])
    elif pc["kind"] == "bj":
        L, U = O.ilu(A, "iluk", level=0, blk=(A.n + pc["nblk"] - 1) // pc["nblk"])
    x0 = None if c["x0"] is None else vec(c["x0"], A.n)
    o = O.solve(O.RLGMRES, A, vec(c["b"], A.n), x0=x0, L=L, U=U, rtol=fx(c["rtol"]), atol=fx(c["atol"]),
                rbtol=fx(c["rbtol"]), maxit=c["maxit"], restart=c["restart"], mode=O.TREE)
    assert r.nits == o.nits
    assert r.residual == o.residual
    assert np.array_equal(r.trace, o.trace)
    assert np.array_equal(xh, o.x, equal_nan=True)


def test_rlgmres_verbose_lines(dev):
    """the reference's message lines: one counter, and the extra line after a cycle that did not converge"""
    import ctypes
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
        r = lssp_amd.solve(dev, A, None, x, b, solver=lssp_amd.RLGMRES, restart=4, maxit=9, verb=2)
    finally:
        L.lssp_amd_set_print(None, None)
    its = [ln for ln in lines if ln.startswith("lgmres: itr:")]
    assert r.nits == 9
    # cycles of 4, 5 (one augmentation column) steps: 9 step lines + a line after each unconverged cycle
    assert [int(ln.split("itr:")[1].split(",")[0]) for ln in its] == [1, 2, 3, 4, 4, 5, 6, 7, 8, 9, 9]
    assert all("/" not in ln.split("abs res")[0] for ln in its)
    assert lines[0] == "lgmres: restart parameter m: 4\n" and lines[1] == "lgmres: aug k: 3\n"
    assert any(ln.startswith("lgmres: total iteration: 9") for ln in lines)
    A.close()
