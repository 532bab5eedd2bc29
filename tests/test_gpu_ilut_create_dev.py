"""lssp_amd_ilut_create_dev: ILUT(tol, p) factored on the device from a matrix
handle, one wavefront per row (GPU box only).

Every observable of the handle -- counts, levels, factors, applies (one
enqueued), both single sweeps, the sweep layout, a whole GMRES(30) solve -- is
compared bit for bit (np.array_equal) with the CPU oracle AND with the handle
lssp_amd_ilu_create(kind ILUT) makes from the same arrays on the host.
Everything outside the scope answers "unsupported" (a non-square handle "invalid
argument") and leaves the matrix and the context usable.  A distributed matrix
is refused as well (several processes: not exercised here).
"""
import numpy as np
import pytest

import oracle as O
from golden_util import cases, fx, matches
from ilut_inputs import (CASES, arrow, box_random, csr, pivot_cancels, poisson7, random_sorted, tiny_a00, tridiag)
from inputs import uniform

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = 1, 6
NOLINES = (0, 0, 0)  # lssp_amd_ilu_sweep_layout of a handle on the packet / sync-free sweeps


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


def _identity(n):
    return O.CSR(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))


def _expected(Ap, Aj, Ax, tol, p):
    """the oracle's results for one matrix: factors, four applies, both sweeps"""
    n = Ap.size - 1
    A = O.CSR(n, Ap, Aj, Ax)
    L, U = O.ilu(A, "ilut", tol=tol, p=p)
    one = _identity(n)
    return dict(A=A, L=L, U=U,
                applies=[O.ilu_apply(L, U, uniform(200 + rep, n)) for rep in range(4)],
                lower=O.ilu_apply(L, one, uniform(300, n)),
                upper=O.ilu_apply(one, U, uniform(300, n)))


def _info(M):
    return M.n, M.nnzL, M.nnzU, M.levelsL, M.levelsU


def _check_pair(dev, Md, Mh, e):
    """the device-made handle == the oracle == the host-made handle, in everything the C-ABI shows"""
    n = e["A"].n
    assert Md.sweep_layout() == NOLINES and Mh.sweep_layout() == NOLINES
    assert _info(Md) == _info(Mh)
    assert (Md.nnzL, Md.nnzU) == (e["L"].Aj.size, e["U"].Aj.size)
    want = (e["L"].Ap, e["L"].Aj, e["L"].Ax, e["U"].Ap, e["U"].Aj, e["U"].Ax)
    for M in (Md, Mh):
        (Lp, Lj, Lx), (Up, Uj, Ux) = M.factors()
        for name, got, w in zip(("Lp", "Lj", "Lx", "Up", "Uj", "Ux"), (Lp, Lj, Lx, Up, Uj, Ux), want):
            assert np.array_equal(got, w), name
    x, z = dev.vec(n), dev.vec(n)
    for rep in range(4):
        r = dev.vec(n, uniform(200 + rep, n))
        if rep == 3:  # the enqueued form
            x.upload(np.zeros(n))
            Md.apply_async(x, r)
            Md.check()
        else:
            Md.apply(x, r)
        got = x.download()
        assert np.array_equal(got, e["applies"][rep]), rep
        Mh.apply(z, r)
        assert np.array_equal(got, z.download()), rep
    r = dev.vec(n, uniform(300, n))
    for which, key in ((0, "lower"), (1, "upper")):
        Md.trisolve(which, x, r)
        assert np.array_equal(x.download(), e[key]), key
        Mh.trisolve(which, z, r)
        assert np.array_equal(x.download(), z.download()), key


def _both(dev, Ap, Aj, Ax, tol, p):
    import lssp_amd
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Md = lssp_amd.DILU.ilut_create_dev(dev, D, tol=tol, p=p)
    D.close()  # the handle owns what it needs
    Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUT, tol=tol, p=p)
    _check_pair(dev, Md, Mh, _expected(Ap, Aj, Ax, tol, p))
    for h in (Md, Mh):
        h.close()


# 1 parameters and the cut (fill, dropping, both qsplit cuts); 2 selection swaps
# (p = 100 >= n: nothing cut); 3 long rows (row 0 of 200 entries read from A, U
# rows in chunks of 64, working rows of 199: the retry at the large capacity);
# 4 the hand-off (every row waits for the row before it, across workgroups and
# XCDs); 5 many rows in flight (chain depth 704, working rows 69 / 63); 6 a
# general pattern; 7 the pivot guards; 8 the smallest sizes
GPU_CASES = CASES + [
    ("box543-p100", lambda: box_random(5, 4, 3, 12), 0.0, 100),
    ("tridiag5000", lambda: tridiag(5000), 1e-3, 5),
    ("p7-16-fill", lambda: poisson7(16), 1e-4, 20),
    ("pivot-cancels", pivot_cancels, 1e-3, -1),
    ("tiny-a00", tiny_a00, 1e-3, -1),
    ("n1", lambda: csr([{0: 2.5}]), 1e-3, -1),
    ("n2", lambda: csr([{0: 2.0, 1: -1.0}, {0: -1.0, 1: 2.0}]), 1e-3, -1),
]


@pytest.mark.parametrize("name,make,tol,p", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_ilut_create_dev_equals_host_create(dev, name, make, tol, p):
    Ap, Aj, Ax = make()
    if name == "pivot-cancels":
        assert O.ilu(O.CSR(4, Ap, Aj, Ax), "ilut", tol=tol, p=p)[1].Ax[3] == -1e-3  # 0.0 replaced by the guard
    if name == "tiny-a00":
        assert O.ilu(O.CSR(4, Ap, Aj, Ax), "ilut", tol=tol, p=p)[1].Ax[0] == -1e-12  # the stored pivot stays
    _both(dev, Ap, Aj, Ax, tol, p)


def test_coo_to_ilut_preconditioned_gmres_without_a_host_matrix(dev):
    """COO in HBM -> coo_to_csr -> sort_columns -> from_device -> ilut_create_dev -> GMRES(30), 7-pt N = 32, b = 1,
    SERIAL reductions: the host-made handle's solve and the reference's recorded run (17 iterations)"""
    import lssp_amd
    from lssp_amd import convert as C
    gold = [c for c in cases("solve") if c["solver"] == lssp_amd.GMRES and c["pc"]["kind"] == "ilut"
            and c["mat"] == {"type": "poisson", "dim": 3, "N": 32} and c["b"] == "ones" and c["restart"] == 30]
    assert len(gold) == 1 and gold[0]["nits"] == 17
    g = gold[0]
    tol, p = g["pc"]["tol"], g["pc"]["p"]
    Ap, Aj, Ax = poisson7(32)
    n, nnz = Ap.size - 1, Aj.size
    perm = np.random.default_rng(8).permutation(nnz)
    Ci = np.repeat(np.arange(n, dtype=np.int32), np.diff(Ap))[perm]
    coo = dev.idx(nnz, Ci), dev.idx(nnz, Aj[perm]), dev.vec(nnz, Ax[perm])
    csr_d = C.coo_to_csr(dev, n, nnz, *coo)
    C.sort_columns(dev, n, n, nnz, *csr_d)
    D = lssp_amd.DMat.from_device(dev, n, n, nnz, *csr_d)
    Md = lssp_amd.DILU.ilut_create_dev(dev, D, tol=tol, p=p)
    for a in (*coo, *csr_d):
        a.free()
    Dh = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUT, tol=tol, p=p)
    kw = dict(solver=lssp_amd.GMRES, tol_rel=fx(g["rtol"]), tol_abs=fx(g["atol"]), tol_rb=fx(g["rbtol"]),
              maxit=g["maxit"], restart=30, trace_cap=100000)
    dev.set_reduction(lssp_amd.SERIAL)
    try:
        x, xh, b = dev.vec(n, np.zeros(n)), dev.vec(n, np.zeros(n)), dev.vec(n, np.ones(n))
        r = lssp_amd.solve(dev, D, Md, x, b, **kw)
        rh = lssp_amd.solve(dev, Dh, Mh, xh, b, **kw)
    finally:
        dev.set_reduction(lssp_amd.TREE)
    assert r.nits == rh.nits == 17
    assert r.residual == rh.residual == fx(g["residual"])
    assert np.array_equal(r.trace, rh.trace) and matches(g["trace"], r.trace)
    assert np.array_equal(x.download(), xh.download()) and matches(g["x"], x.download())
    for h in (Dh, Mh, D, Md):
        h.close()


def _refusal_input(case):
    import lssp_amd
    Ap, Aj, Ax = box_random(5, 4, 3, 12)
    n = Ap.size - 1
    mid = n // 2
    kw = dict(tol=0.0, p=3)
    if case == "block-jacobi":
        kw["blk"] = n // 2
    elif case == "unsorted":
        Aj, Ax = Aj.copy(), Ax.copy()
        a = Ap[mid] + 1
        Aj[[a, a + 1]] = Aj[[a + 1, a]]
        Ax[[a, a + 1]] = Ax[[a + 1, a]]
    elif case == "repeated-column":
        Aj = Aj.copy()
        Aj[Ap[mid] + 1] = Aj[Ap[mid]]
    elif case == "diagonal-deleted":
        e = Ap[mid] + int(np.flatnonzero(Aj[Ap[mid]:Ap[mid + 1]] == mid)[0])
        Bp = Ap.copy()
        Bp[mid + 1:] -= 1
        Ap, Aj, Ax = Bp, np.delete(Aj, e), np.delete(Ax, e)
    elif case == "capacity":
        cap = lssp_amd.DILU.ilut_capacity()
        assert cap >= 1024
        Ap, Aj, Ax = arrow(cap + 100)  # row 1 fills to cap + 98 entries past its diagonal
        kw = dict(tol=0.0, p=5)
    else:
        assert case == "non-square"
    return Ap, Aj, Ax, kw


REFUSED = ["block-jacobi", "unsorted", "repeated-column", "diagonal-deleted", "non-square", "capacity"]


@pytest.mark.parametrize("case", REFUSED)
def test_ilut_create_dev_refusals_leave_everything_usable(dev, case):
    import lssp_amd
    Ap, Aj, Ax, kw = _refusal_input(case)
    n = Ap.size - 1
    ncols = n + 1 if case == "non-square" else n
    D = lssp_amd.DMat(dev, Ap, Aj, Ax, ncols=ncols)
    with pytest.raises(lssp_amd.LsspError) as err:  # (no handle comes back: *out stays NULL)
        lssp_amd.DILU.ilut_create_dev(dev, D, **kw)
    assert err.value.status == (EINVAL if case == "non-square" else EUNSUPPORTED)
    # the matrix still multiplies ...
    xh = uniform(0x5EED, ncols)
    z = dev.vec(n)
    D.mv_mxy(dev.vec(ncols, xh), z)
    assert np.array_equal(z.download(), O.spmv(0, O.CSR(n, Ap, Aj, Ax), xh))
    D.close()
    # ... and the context still makes and applies a good handle
    Bp, Bj, Bx = box_random(5, 4, 3, 12)
    _both(dev, Bp, Bj, Bx, 0.0, 2)


def test_out_pointer_is_cleared_on_refusal(dev):
    import ctypes
    import lssp_amd
    Ap, Aj, Ax, kw = _refusal_input("unsorted")
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    h = ctypes.c_void_p(1)
    assert dev.L.lssp_amd_ilut_create_dev(dev.h, D.h, 0.0, 3, 0, ctypes.byref(h)) == EUNSUPPORTED
    assert h.value is None
    D.close()


def test_refactor_calls_refuse_the_ilut_handle(dev):
    import lssp_amd
    Ap, Aj, Ax = poisson7(8)
    n = Ap.size - 1
    e = _expected(Ap, Aj, Ax, 1e-4, 20)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    M = lssp_amd.DILU.ilut_create_dev(dev, D, tol=1e-4, p=20)
    for call in (M.iluk_refactor, M.refactor):
        with pytest.raises(lssp_amd.LsspError) as err:
            call(D)
        assert err.value.status == EUNSUPPORTED
    x = dev.vec(n)
    M.apply(x, dev.vec(n, uniform(200, n)))
    assert np.array_equal(x.download(), e["applies"][0])
    for h in (M, D):
        h.close()
