"""lssp_amd_iluk_create_dev: the skewed line-sweep ILU(1) of a 5-/7-point box made
from a matrix handle on the device (GPU box only).

Every observable of the handle -- counts, factors, applies, single sweeps, a
whole BiCGSTAB solve, the state after lssp_amd_iluk_refactor -- is compared bit
for bit (np.array_equal) with the CPU oracle AND with the handle
lssp_amd_ilu_create(level 1) makes from the same matrix on the host.  Level 0
goes to lssp_amd_ilu_create_dev unchanged.  Everything outside the scope answers
"unsupported" (a non-square handle "invalid argument") and leaves the matrix and
the context usable.
"""
import numpy as np
import pytest

import oracle as O
from inputs import rand_csr, uniform

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = 1, 6
TILES0 = (1, 16, 8)  # lssp_amd_ilu_sweep_layout of the tiled ILU(0) line sweeps
TILES1 = (2, 16, 8)  # ... of the skewed ILU(1) line sweeps


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


_BOX = {}


def _box7(nx, ny, nz, seed):
    """7-pt stencil on an nx x ny x nz box (natural order, i fastest; nz = 1: 5-pt), random
    nonsymmetric diagonally dominant values (tests/test_gpu_create_dev.py _box7)."""
    key = (nx, ny, nz, seed)
    if key not in _BOX:
        rng = np.random.default_rng(seed)
        n = nx * ny * nz
        Ap, Aj, Ax = [0], [], []
        for r in range(n):
            i, j, k = r % nx, r // nx % ny, r // (nx * ny)
            cols = [c for c, ok in ((r - nx * ny, k > 0), (r - nx, j > 0), (r - 1, i > 0), (r, True),
                                    (r + 1, i < nx - 1), (r + nx, j < ny - 1), (r + nx * ny, k < nz - 1)) if ok]
            vals = rng.uniform(-1, -0.1, len(cols))
            vals[cols.index(r)] = 7.0 + rng.uniform(0, 1)
            Aj += cols
            Ax += list(vals)
            Ap.append(len(Aj))
        _BOX[key] = (np.array(Ap, np.int32), np.array(Aj, np.int32), np.array(Ax))
    Ap, Aj, Ax = _BOX[key]
    return Ap, Aj, Ax.copy()


def _identity(n):
    return O.CSR(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))


_ORACLE = {}


def _expected(tag, Ap, Aj, Ax, level=1):
    """the oracle's results for one matrix, computed once: factors, four applies, both sweeps, a product"""
    if tag not in _ORACLE:
        n = Ap.size - 1
        A = O.CSR(n, Ap, Aj, Ax)
        L, U = O.ilu(A, "iluk", level=level)
        one = _identity(n)
        _ORACLE[tag] = dict(
            A=A, L=L, U=U,
            applies=[O.ilu_apply(L, U, uniform(200 + rep, n)) for rep in range(4)],
            lower=O.ilu_apply(L, one, uniform(300, n)),
            upper=O.ilu_apply(one, U, uniform(300, n)),
            mxy=O.spmv(0, A, uniform(0x5EED, n)))
    return _ORACLE[tag]


def _info(M):
    return M.n, M.nnzL, M.nnzU, M.levelsL, M.levelsU


def _check_pair(dev, Md, Mh, e, layout=TILES1, factors=True):
    """the device-made handle == the oracle == the host-made handle, in everything the C-ABI shows"""
    n = e["A"].n
    assert Md.sweep_layout()[0] == layout[0] and Mh.sweep_layout()[0] == layout[0]  # "unsupported" cannot pass unnoticed
    assert Md.sweep_layout() == layout and Mh.sweep_layout() == layout
    assert _info(Md) == _info(Mh)
    if factors:
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


def _multiplies(dev, D, want):
    n = want.size
    z = dev.vec(n)
    D.mv_mxy(dev.vec(n, uniform(0x5EED, n)), z)
    return np.array_equal(z.download(), want)


BOXES = [(4, 3, 2),      # the smallest accepted box: one tile
         (9, 21, 13),    # 33 skewed columns, planes 8 + 5, off-grid tiles skipped
         (13, 37, 35),   # five tile rows, 3 planes in the last
         (5, 300, 1)]    # a 2-D grid too tall for the one-workgroup route: tiles
CASES = ([(b, "upload") for b in BOXES]
         + [((9, 21, 13), "from_device"), ((9, 21, 13), "closed"), ((9, 21, 13), "level-1")])


@pytest.mark.parametrize("box,how", CASES, ids=[f"{b[0]}x{b[1]}x{b[2]}-{h}" for b, h in CASES])
def test_iluk_create_dev_equals_host_create(dev, box, how):
    import lssp_amd
    nx, ny, nz = box
    s = nx + ny + nz
    Ap, Aj, Ax = _box7(nx, ny, nz, s)
    n, nnz = Ap.size - 1, Aj.size
    e = _expected((nx, ny, nz, s), Ap, Aj, Ax)
    if how == "from_device":
        arrays = dev.idx(n + 1, Ap), dev.idx(nnz, Aj), dev.vec(nnz, Ax)
        D = lssp_amd.DMat.from_device(dev, n, n, nnz, *arrays)
        for a in arrays:
            a.free()
    else:
        D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Md = lssp_amd.DILU.iluk_create_dev(dev, D, kind=lssp_amd.ILUK, level=-1 if how == "level-1" else 1)
    if how == "closed":
        D.close()  # the handle owns what it needs
    else:
        assert _multiplies(dev, D, e["mxy"])
    Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=-1 if how == "level-1" else 1)
    assert Md.levelsL == Md.levelsU == nx + 2 * ny + 3 * nz - 5
    _check_pair(dev, Md, Mh, e)
    for h in (Md, Mh, D):
        h.close()


def test_iluk_create_dev_special_values(dev):
    """the row-0 tiny-pivot rule (A[0,0] = 1e-12) and exact +0.0 / -0.0 off-diagonals (the
    elimination skips an update whose multiplier row holds an exact zero)"""
    import lssp_amd
    nx, ny, nz = 9, 21, 13
    Ap, Aj, Ax = _box7(nx, ny, nz, 44)
    n = Ap.size - 1
    rng = np.random.default_rng(5)
    offd = np.flatnonzero(Aj != np.repeat(np.arange(n), np.diff(Ap)))
    pick = rng.choice(offd, offd.size // 50 + 8, replace=False)
    Ax[pick[8:]] = 0.0
    Ax[pick[:8]] = -0.0
    assert Aj[0] == 0
    Ax[0] = 1e-12
    e = _expected("special", Ap, Aj, Ax)
    assert e["U"].Ax[0] == 1e-12  # the stored pivot stays; only its reciprocal uses the replacement
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Md = lssp_amd.DILU.iluk_create_dev(dev, D)
    Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=1)
    assert Md.factors()[1][2][0] == 1e-12
    _check_pair(dev, Md, Mh, e)
    for h in (Md, Mh, D):
        h.close()


@pytest.mark.parametrize("read_factors", [True, False], ids=["factors-read", "factors-unread"])
def test_iluk_create_dev_is_born_refactorable(dev, read_factors):
    import lssp_amd
    nx, ny, nz = 9, 21, 13
    s = nx + ny + nz
    Ap, Aj, Ax0 = _box7(nx, ny, nz, s)
    vals = {0: Ax0, 1: _box7(nx, ny, nz, s + 1)[2], 2: _box7(nx, ny, nz, s + 2)[2]}
    D = lssp_amd.DMat(dev, Ap, Aj, Ax0)
    Md = lssp_amd.DILU.iluk_create_dev(dev, D)
    assert Md.sweep_layout() == TILES1
    for k in (1, 2, 0):  # two new sets of values, then the creation values again
        D.update_values(dev.vec(vals[k].size, vals[k]))
        Md.iluk_refactor(D)
        fresh = lssp_amd.DILU.create(dev, Ap, Aj, vals[k], kind=lssp_amd.ILUK, level=1)
        e = _expected((nx, ny, nz, s + k), Ap, Aj, vals[k])
        # (without the factors read in between, the host copies are first made after the last refactor)
        _check_pair(dev, Md, fresh, e, factors=read_factors or k == 0)
        assert _multiplies(dev, D, e["mxy"])
        fresh.close()
    Md.close()
    D.close()


def test_level_0_goes_to_create_dev(dev):
    import lssp_amd
    nx, ny, nz = 9, 21, 13
    s = nx + ny + nz
    Ap, Aj, Ax = _box7(nx, ny, nz, s)
    e = _expected((nx, ny, nz, s, "level0"), Ap, Aj, Ax, level=0)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Md = lssp_amd.DILU.iluk_create_dev(dev, D, level=0)
    Mc = lssp_amd.DILU.create_dev(dev, D, level=0)
    assert Md.sweep_layout() == TILES0
    _check_pair(dev, Md, Mc, e, layout=TILES0)
    Ax1 = _box7(nx, ny, nz, s + 1)[2]
    D.update_values(dev.vec(Ax1.size, Ax1))
    Md.refactor(D)
    Mc.refactor(D)
    _check_pair(dev, Md, Mc, _expected((nx, ny, nz, s + 1, "level0"), Ap, Aj, Ax1, level=0), layout=TILES0)
    for h in (Md, Mc, D):
        h.close()


def test_coo_to_ilu1_preconditioned_solve_without_a_host_matrix(dev):
    """shuffled COO in HBM -> coo_to_csr -> sort_columns -> from_device -> iluk_create_dev(-1) -> BiCGSTAB"""
    import lssp_amd
    from lssp_amd import convert as C
    nx, ny, nz = 9, 21, 13
    s = nx + ny + nz
    Ap, Aj, Ax = _box7(nx, ny, nz, s)
    n, nnz = Ap.size - 1, Aj.size
    e = _expected((nx, ny, nz, s), Ap, Aj, Ax)
    perm = np.random.default_rng(8).permutation(nnz)
    Ci = np.repeat(np.arange(n, dtype=np.int32), np.diff(Ap))[perm]
    coo = dev.idx(nnz, Ci), dev.idx(nnz, Aj[perm]), dev.vec(nnz, Ax[perm])
    csr = C.coo_to_csr(dev, n, nnz, *coo)
    C.sort_columns(dev, n, n, nnz, *csr)
    D = lssp_amd.DMat.from_device(dev, n, n, nnz, *csr)
    Md = lssp_amd.DILU.iluk_create_dev(dev, D, level=-1)
    for a in (*coo, *csr):
        a.free()
    assert Md.sweep_layout() == TILES1
    bh = uniform(77, n)
    kw = dict(solver=lssp_amd.BICGSTAB, tol_rel=1e-7, tol_abs=1e-7, tol_rb=1e-7, maxit=40, restart=30,
              trace_cap=100000)
    assert dev.reduction == lssp_amd.TREE
    x, b = dev.vec(n, np.zeros(n)), dev.vec(n, bh)
    r = lssp_amd.solve(dev, D, Md, x, b, **kw)
    o = O.solve(O.BICGSTAB, e["A"], bh, L=e["L"], U=e["U"], rtol=1e-7, atol=1e-7, rbtol=1e-7, maxit=40, restart=30,
                mode=O.TREE)
    assert r.nits == o.nits
    assert r.residual == o.residual
    assert np.array_equal(r.trace, o.trace)
    assert np.array_equal(x.download(), o.x)
    Dh = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=-1)
    assert Mh.sweep_layout() == TILES1
    xh = dev.vec(n, np.zeros(n))
    rh = lssp_amd.solve(dev, Dh, Mh, xh, b, **kw)
    assert (r.nits, r.residual) == (rh.nits, rh.residual)
    assert np.array_equal(r.trace, rh.trace) and np.array_equal(x.download(), xh.download())
    for h in (Dh, Mh, D, Md):
        h.close()


def _drop(Ap, Aj, Ax, e):
    """the CSR without entry e"""
    row = np.searchsorted(Ap, e, side="right") - 1
    Bp = Ap.copy()
    Bp[row + 1:] -= 1
    return Bp, np.delete(Aj, e), np.delete(Ax, e)


def _refusal_input(case):
    """(Ap, Aj, Ax, iluk_create_dev keywords) of one refused call"""
    import lssp_amd
    nx, ny, nz = 9, 21, 13
    Ap, Aj, Ax = _box7(nx, ny, nz, 43)
    n = Ap.size - 1
    mid = n // 2  # a mid-grid row: all six neighbours
    assert Ap[mid + 1] - Ap[mid] == 7
    kw = {}
    if case == "ilut":
        kw = dict(kind=lssp_amd.ILUT, tol=1e-4, p=20)
    elif case == "level2":
        kw = dict(level=2)
    elif case == "block-jacobi":
        kw = dict(blk=n // 2)
    elif case == "nx==2":
        Ap, Aj, Ax = _box7(2, 9, 9, 20)
    elif case == "one-workgroup":
        Ap, Aj, Ax = _box7(30, 27, 1, 57)
        kw = dict(level=1)
    elif case == "general":
        Ap, Aj, Ax = rand_csr(3000, 6, 11, unsorted=False)
    elif case == "entry-deleted":
        Ap, Aj, Ax = _drop(Ap, Aj, Ax, Ap[mid] + 1)
    elif case == "diagonal-deleted":
        assert Aj[Ap[mid] + 3] == mid
        Ap, Aj, Ax = _drop(Ap, Aj, Ax, Ap[mid] + 3)
    elif case == "unsorted":
        Aj, Ax = Aj.copy(), Ax.copy()
        a = Ap[mid] + 4
        Aj[[a, a + 1]] = Aj[[a + 1, a]]
        Ax[[a, a + 1]] = Ax[[a + 1, a]]
    elif case == "row0-moved":
        Aj = Aj.copy()
        assert Aj[Ap[1] - 1] == nx * ny  # row 0's last entry, (0, 0, 1): moved one column on
        Aj[Ap[1] - 1] += 1
    else:
        assert case in ("line-off", "non-square")
    return Ap, Aj, Ax, kw


REFUSED = ["ilut", "level2", "block-jacobi", "nx==2", "one-workgroup", "general", "entry-deleted",
           "diagonal-deleted", "unsorted", "row0-moved", "line-off", "non-square"]


@pytest.mark.parametrize("case", REFUSED)
def test_iluk_create_dev_refusals_leave_everything_usable(dev, case, monkeypatch):
    import lssp_amd
    Ap, Aj, Ax, kw = _refusal_input(case)
    n = Ap.size - 1
    if case == "one-workgroup":  # the host create does take that route there
        Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=1)
        assert Mh.sweep_layout() == (2, 27, 1)
        Mh.close()
    ncols = n + 1 if case == "non-square" else n
    D = lssp_amd.DMat(dev, Ap, Aj, Ax, ncols=ncols)
    with monkeypatch.context() as mp:
        if case == "line-off":
            mp.setenv("LSSP_AMD_LINE", "0")
        with pytest.raises(lssp_amd.LsspError) as err:
            lssp_amd.DILU.iluk_create_dev(dev, D, **kw)
    assert err.value.status == (EINVAL if case == "non-square" else EUNSUPPORTED)
    # the matrix still multiplies ...
    xh = uniform(0x5EED, ncols)
    z = dev.vec(n)
    D.mv_mxy(dev.vec(ncols, xh), z)
    assert np.array_equal(z.download(), O.spmv(0, O.CSR(n, Ap, Aj, Ax), xh))
    # ... and the context still makes the handle of an eligible box
    Bp, Bj, Bx = _box7(4, 3, 2, 9)
    B = lssp_amd.DMat(dev, Bp, Bj, Bx)
    M = lssp_amd.DILU.iluk_create_dev(dev, B)
    assert M.sweep_layout() == TILES1
    e = _expected((4, 3, 2, 9), Bp, Bj, Bx)
    x = dev.vec(e["A"].n)
    M.apply(x, dev.vec(e["A"].n, uniform(200, e["A"].n)))
    assert np.array_equal(x.download(), e["applies"][0])
    for h in (M, B, D):
        h.close()
