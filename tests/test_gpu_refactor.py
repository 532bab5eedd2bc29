"""New values on an unchanged pattern (lssp_amd_mat_update_values,
lssp_amd_ilu_refactor; GPU box only).

A matrix handle and the tiled line-sweep ILU(0) of a 7-point box take new
values without being assembled again.  Every result afterwards -- factors,
applies, single sweeps, products, a whole BiCGSTAB solve -- is compared bit for
bit (np.array_equal) with the CPU oracle on the new values AND with fresh
handles made from them.  Handle kinds outside the scope answer "unsupported"
and stay usable; a different pattern answers "invalid argument".
"""
import numpy as np
import pytest

import oracle as O
from bilu_util import bilu_apply
from inputs import rand_csr, uniform

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = 1, 6
TILES = (True, 16, 8)  # lssp_amd_ilu_sweep_layout of the tiled ILU(0) line sweeps


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


_BOX = {}


def _box7(nx, ny, nz, seed):
    """7-pt stencil on an nx x ny x nz box (natural order, i fastest), random
    nonsymmetric diagonally dominant values (tests/test_gpu_parity.py _box7)."""
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


def _expected(tag, Ap, Aj, Ax):
    """the oracle's results for one matrix, computed once: factors, four applies, both sweeps, a product"""
    if tag not in _ORACLE:
        n = Ap.size - 1
        A = O.CSR(n, Ap, Aj, Ax)
        L, U = O.ilu(A, "iluk", level=0)
        one = _identity(n)
        _ORACLE[tag] = dict(
            A=A, L=L, U=U,
            applies=[O.ilu_apply(L, U, uniform(200 + rep, n)) for rep in range(4)],
            lower=O.ilu_apply(L, one, uniform(300, n)),
            upper=O.ilu_apply(one, U, uniform(300, n)),
            mxy=O.spmv(0, A, uniform(0x5EED, n)))
    return _ORACLE[tag]


def _same_factors(M, L, U):
    (Lp, Lj, Lx), (Up, Uj, Ux) = M.factors()
    return (np.array_equal(Lp, L.Ap) and np.array_equal(Lj, L.Aj) and np.array_equal(Lx, L.Ax)
            and np.array_equal(Up, U.Ap) and np.array_equal(Uj, U.Aj) and np.array_equal(Ux, U.Ax))


def _check_state(dev, D, M, e, fresh=None):
    """handle state == the oracle's (and a fresh handle's) for the matrix e was computed from"""
    n = e["A"].n
    assert _same_factors(M, e["L"], e["U"])
    x, z = dev.vec(n), dev.vec(n)
    for rep in range(4):
        r = dev.vec(n, uniform(200 + rep, n))
        M.apply(x, r)
        got = x.download()
        assert np.array_equal(got, e["applies"][rep]), rep
        if fresh is not None:
            fresh[1].apply(z, r)
            assert np.array_equal(got, z.download()), rep
    r = dev.vec(n, uniform(300, n))
    M.trisolve(0, z, r)
    assert np.array_equal(z.download(), e["lower"])
    M.trisolve(1, z, r)
    assert np.array_equal(z.download(), e["upper"])
    xv = dev.vec(n, uniform(0x5EED, n))
    D.mv_mxy(xv, z)
    assert np.array_equal(z.download(), e["mxy"])
    if fresh is not None:
        assert _same_factors(fresh[1], e["L"], e["U"])
        fresh[0].mv_mxy(xv, x)
        assert np.array_equal(x.download(), e["mxy"])


def _refresh(dev, D, M, Ax):
    D.update_values(dev.vec(Ax.size, Ax))
    M.refactor(D)


BOXES = [(11, 16, 4),    # one tile
         (9, 21, 13),    # two ragged j tiles, 8 + 5 planes
         (13, 37, 35),   # 3 x 5 tiles, 3 planes in the last
         (5, 300, 1)]    # a 2-D grid too tall for the one-workgroup route: tiles


@pytest.mark.parametrize("nx,ny,nz", BOXES)
def test_refactor_against_fresh_create(dev, nx, ny, nz):
    import lssp_amd
    s = nx + ny + nz
    Ap, Aj, Ax0 = _box7(nx, ny, nz, s)
    _, _, Ax1 = _box7(nx, ny, nz, s + 1)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax0)
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax0, kind=lssp_amd.ILUK, level=0)
    assert M.sweep_layout() == TILES  # an "unsupported" answer cannot pass unnoticed
    _refresh(dev, D, M, Ax1)
    fresh = (lssp_amd.DMat(dev, Ap, Aj, Ax1), lssp_amd.DILU.create(dev, Ap, Aj, Ax1, kind=lssp_amd.ILUK, level=0))
    _check_state(dev, D, M, _expected((nx, ny, nz, s + 1), Ap, Aj, Ax1), fresh)
    assert M.sweep_layout() == TILES
    for h in (*fresh, M, D):
        h.close()


def test_refactor_special_values(dev):
    """the row-0 tiny-pivot rule (A[0,0] = 1e-12) and exact +0.0 / -0.0 off-diagonals (the
    elimination skips an update whose multiplier row holds an exact zero)"""
    import lssp_amd
    nx, ny, nz = 9, 21, 13
    Ap, Aj, Ax0 = _box7(nx, ny, nz, 43)
    _, _, Ax1 = _box7(nx, ny, nz, 44)
    n = Ap.size - 1
    rng = np.random.default_rng(5)
    offd = np.flatnonzero(Aj != np.repeat(np.arange(n), np.diff(Ap)))
    pick = rng.choice(offd, offd.size // 50 + 8, replace=False)
    Ax1[pick[8:]] = 0.0
    Ax1[pick[:8]] = -0.0
    assert Aj[0] == 0
    Ax1[0] = 1e-12
    D = lssp_amd.DMat(dev, Ap, Aj, Ax0)
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax0, kind=lssp_amd.ILUK, level=0)
    assert M.sweep_layout() == TILES
    _refresh(dev, D, M, Ax1)
    fresh = (lssp_amd.DMat(dev, Ap, Aj, Ax1), lssp_amd.DILU.create(dev, Ap, Aj, Ax1, kind=lssp_amd.ILUK, level=0))
    e = _expected("special", Ap, Aj, Ax1)
    assert e["U"].Ax[0] == 1e-12  # the stored pivot stays; only its reciprocal uses the replacement
    _check_state(dev, D, M, e, fresh)
    for h in (*fresh, M, D):
        h.close()


def test_refactor_leaves_no_stale_state(dev):
    import lssp_amd
    nx, ny, nz = 9, 21, 13
    s = nx + ny + nz
    Ap, Aj, Ax0 = _box7(nx, ny, nz, s)
    vals = {k: _box7(nx, ny, nz, s + k)[2] for k in (1, 2)}
    D = lssp_amd.DMat(dev, Ap, Aj, Ax0)
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax0, kind=lssp_amd.ILUK, level=0)
    assert M.sweep_layout() == TILES
    e0 = _expected((nx, ny, nz, s), Ap, Aj, Ax0)
    _check_state(dev, D, M, e0)
    for k in (1, 2, 1):
        _refresh(dev, D, M, vals[k])
        _check_state(dev, D, M, _expected((nx, ny, nz, s + k), Ap, Aj, vals[k]))
    _refresh(dev, D, M, Ax0)  # the creation values reproduce the created handle
    _check_state(dev, D, M, e0)
    M.close()
    D.close()


def test_solve_after_refresh(dev):
    import lssp_amd
    nx, ny, nz = 13, 37, 35
    s = nx + ny + nz
    Ap, Aj, Ax0 = _box7(nx, ny, nz, s)
    _, _, Ax1 = _box7(nx, ny, nz, s + 1)
    n = Ap.size - 1
    D = lssp_amd.DMat(dev, Ap, Aj, Ax0)
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax0, kind=lssp_amd.ILUK, level=0)
    assert M.sweep_layout() == TILES
    _refresh(dev, D, M, Ax1)
    e = _expected((nx, ny, nz, s + 1), Ap, Aj, Ax1)
    bh = uniform(77, n)
    kw = dict(solver=lssp_amd.BICGSTAB, tol_rel=1e-7, tol_abs=1e-7, tol_rb=1e-7, maxit=40, restart=30,
              trace_cap=100000)
    assert dev.reduction == lssp_amd.TREE
    x, b = dev.vec(n, np.zeros(n)), dev.vec(n, bh)
    r = lssp_amd.solve(dev, D, M, x, b, **kw)
    o = O.solve(O.BICGSTAB, e["A"], bh, L=e["L"], U=e["U"], rtol=1e-7, atol=1e-7, rbtol=1e-7, maxit=40, restart=30,
                mode=O.TREE)
    assert r.nits == o.nits
    assert r.residual == o.residual
    assert np.array_equal(r.trace, o.trace)
    assert np.array_equal(x.download(), o.x)
    Df = lssp_amd.DMat(dev, Ap, Aj, Ax1)
    Mf = lssp_amd.DILU.create(dev, Ap, Aj, Ax1, kind=lssp_amd.ILUK, level=0)
    xf = dev.vec(n, np.zeros(n))
    rf = lssp_amd.solve(dev, Df, Mf, xf, b, **kw)
    assert (r.nits, r.residual) == (rf.nits, rf.residual)
    assert np.array_equal(r.trace, rf.trace) and np.array_equal(x.download(), xf.download())
    for h in (Df, Mf, D, M):
        h.close()


def _scattered(n, seed, maxlen=20, reach=3000):
    """random CSR whose columns scatter within +-reach of the row: rows of 0..maxlen entries, empty
    rows and rows longer than 12 entries included (tests/test_gpu_parity.py _scattered)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxlen + 1, n)
    lens[::97] = 0
    Ap = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=Ap[1:])
    Aj = np.empty(Ap[-1], np.int64)
    for r in range(n):
        lo, hi = max(0, r - reach), min(n, r + reach + 1)
        Aj[Ap[r]:Ap[r + 1]] = np.sort(rng.choice(np.arange(lo, hi), lens[r], replace=False))
    Ax = uniform(seed + 7, int(Ap[-1]))
    return Ap.astype(np.int32), Aj.astype(np.int32), Ax


def _layout_input(which):
    if which == "coded":
        return _box7(9, 21, 13, 43)
    if which == "windowed":
        return _scattered(5000, 11)
    return _scattered(40000, 12, maxlen=12, reach=40000)


@pytest.mark.parametrize("which", ["coded", "windowed", "csr"])
def test_update_values_in_every_matrix_layout(dev, which):
    import lssp_amd
    Ap, Aj, Ax0 = _layout_input(which)
    n, nnz = Ap.size - 1, Ax0.size
    Ax1 = uniform(991, nnz)
    A1 = O.CSR(n, Ap, Aj, Ax1)
    xh, yh = uniform(0x5EED, n), uniform(3, n)
    want = [O.spmv(0, A1, xh), O.spmv(1, A1, xh, alpha=-0.75), O.spmv(3, A1, xh, alpha=-1.0, beta=1.0, y=yh),
            O.spmv(2, A1, xh, alpha=1.5, beta=0.25, z=yh.copy())]
    up = lssp_amd.DMat(dev, Ap, Aj, Ax0)
    fd = lssp_amd.DMat.from_device(dev, n, n, nnz, dev.idx(n + 1, Ap), dev.idx(max(nnz, 1), Aj), dev.vec(nnz, Ax0))
    for M in (up, fd):
        layout, nbytes = (M.ndiag, M.windowed), M.device_bytes
        assert (layout[0] > 0, layout[1]) == (which == "coded", which == "windowed")
        M.update_values(dev.vec(nnz, Ax1))
        assert (M.ndiag, M.windowed) == layout and M.device_bytes == nbytes
        x, y, z = dev.vec(n, xh), dev.vec(n, yh), dev.vec(n, yh)
        M.mv_mxy(x, z)
        assert np.array_equal(z.download(), want[0])
        M.mv_amxy(-0.75, x, z)
        assert np.array_equal(z.download(), want[1])
        M.mv_amxpbyz(-1.0, x, 1.0, y, z)
        assert np.array_equal(z.download(), want[2])
        M.mv_amxpby(1.5, x, 0.25, y)
        assert np.array_equal(y.download(), want[3])
    if which == "windowed":
        # CG in tree mode (the fused q.p of the product's epilogue); NaN compared as NaN, as
        # test_spmv_scattered_bitwise_vs_oracle does: the matrix is not SPD
        b, xs = dev.vec(n, np.ones(n)), dev.vec(n, np.zeros(n))
        r = lssp_amd.solve(dev, up, None, xs, b, solver=lssp_amd.CG, maxit=20, trace_cap=100000)
        o = O.solve(lssp_amd.CG, A1, np.ones(n), maxit=20, mode=O.TREE)
        assert r.nits == o.nits and np.array_equal(r.trace, o.trace, equal_nan=True)
        assert np.array_equal(xs.download(), o.x, equal_nan=True)
    with pytest.raises(lssp_amd.LsspError) as err:
        up.update_values(dev.vec(nnz + 1, np.zeros(nnz + 1)))
    assert err.value.status == EINVAL
    z = dev.vec(n)
    up.mv_mxy(dev.vec(n, xh), z)
    assert np.array_equal(z.download(), want[0])  # the handle is as it was
    up.close()
    fd.close()


def _refused(dev, M, D, status, want):
    """refactor answers status; one apply afterwards is still the expected one"""
    import lssp_amd
    with pytest.raises(lssp_amd.LsspError) as err:
        M.refactor(D)
    assert err.value.status == status
    n = want.size
    x = dev.vec(n)
    M.apply(x, dev.vec(n, uniform(200, n)))
    assert np.array_equal(x.download(), want)


UNSUPPORTED = ["one-workgroup", "level1", "ilut", "block-jacobi", "from_factors", "bilu", "general"]


@pytest.mark.parametrize("kind", UNSUPPORTED)
def test_refactor_unsupported_handles_stay_usable(dev, kind):
    import lssp_amd
    if kind == "one-workgroup":
        Ap, Aj, Ax = _box7(30, 27, 1, 57)
    elif kind == "general":
        Ap, Aj, Ax = rand_csr(3000, 6, 11, unsorted=False)
    else:
        Ap, Aj, Ax = _box7(9, 21, 13, 43)
    n = Ap.size - 1
    A = O.CSR(n, Ap, Aj, Ax)
    rhs = uniform(200, n)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    if kind in ("one-workgroup", "general"):
        M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0)
        assert M.sweep_layout() == ((1, 27, 1) if kind == "one-workgroup" else (0, 0, 0))
        want = O.ilu_apply(*O.ilu(A, "iluk", level=0), rhs)
    elif kind == "level1":
        M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=1)
        want = O.ilu_apply(*O.ilu(A, "iluk", level=1), rhs)
    elif kind == "ilut":
        M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUT, tol=1e-4, p=20)
        want = O.ilu_apply(*O.ilu(A, "ilut", tol=1e-4, p=20), rhs)
    elif kind == "block-jacobi":
        M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0, blk=n // 2)
        want = O.ilu_apply(*O.ilu(A, "iluk", level=0, blk=n // 2), rhs)
    elif kind == "from_factors":
        L, U = O.ilu(A, "iluk", level=0)
        M = lssp_amd.DILU.from_factors(dev, (L.Ap, L.Aj, L.Ax), (U.Ap, U.Aj, U.Ax))
        assert M.sweep_layout() == TILES  # the same sweeps, but not made by ilu_create
        want = O.ilu_apply(L, U, rhs)
    else:
        M = lssp_amd.DILU.bilu(dev, Ap, Aj, Ax, bs=1, level=0)
        Lf, Uf = M.factors()
        want = bilu_apply(n, 1, Lf, M.diag()[1], Uf, rhs)
    _refused(dev, M, D, EUNSUPPORTED, want)
    M.close()
    D.close()


def test_refactor_rejects_another_pattern(dev):
    import lssp_amd
    nx, ny, nz = 9, 21, 13
    Ap, Aj, Ax = _box7(nx, ny, nz, 43)
    n = Ap.size - 1
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0)
    assert M.sweep_layout() == TILES
    want = O.ilu_apply(*O.ilu(O.CSR(n, Ap, Aj, Ax), "iluk", level=0), uniform(200, n))
    Aj2 = Aj.copy()
    assert Aj2[Ap[1] - 1] == nx * ny  # row 0's last entry, (0, 0, 1): moved one column on
    Aj2[Ap[1] - 1] += 1
    other = lssp_amd.DMat(dev, Ap, Aj2, Ax)
    _refused(dev, M, other, EINVAL, want)
    Bp, Bj, Bx = _box7(nx, ny, nz - 1, 43)
    smaller = lssp_amd.DMat(dev, Bp, Bj, Bx)
    _refused(dev, M, smaller, EINVAL, want)
    # and the handle still refactors
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    _, _, Ax1 = _box7(nx, ny, nz, 44)
    _refresh(dev, D, M, Ax1)
    assert _same_factors(M, *O.ilu(O.CSR(n, Ap, Aj, Ax1), "iluk", level=0))
    for h in (other, smaller, D, M):
        h.close()
