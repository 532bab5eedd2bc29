"""lssp_amd_bilu_create_dev: a BILUK handle made on the device from a matrix that
lives in HBM (GPU box only).

Every observable of the handle -- counts, factors, inverted diagonal blocks, the
apply, both single sweeps, a short GMRES solve, both packet schedules, the state
after lssp_amd_bilu_refactor -- is compared bit for bit (np.array_equal) with the
handle lssp_amd_bilu_create makes from the same arrays on the host, with the
independent host path (lssp_amd.bilu_factor_host) and with the oracle's sweeps on
those factors (bilu_util.bilu_apply).  What is outside the scope answers
"unsupported" or "invalid argument" and leaves the matrix and the context usable.
"""
import numpy as np
import pytest

import oracle as O
from bilu_util import bilu_apply, block_grid
from inputs import uniform

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = 1, 6
# (dim, N, bs, level, variant), rows unshuffled: 8^3 x 3 (n = 1536), 6^3 x 4 (864; at level 1 strict rows of
# exactly 24 entries, the packet limit), 16^2 x 2 (512), 8^3 x 1 (512: must not take a line route), 4^3 x 8
# (512: the largest device block, 24-entry rows), 16^2 x 2 with holes inside the blocks
SHAPES = [(3, 8, 3, 0, None), (3, 8, 3, 1, None), (3, 6, 4, 0, None), (3, 6, 4, 1, None), (2, 16, 2, 0, None),
          (3, 8, 1, 0, None), (3, 4, 8, 0, None), (2, 16, 2, 0, "holes")]


def _name(c):
    dim, N, bs, level, variant = c
    return f"{N}^{dim}-bs{bs}-l{level}" + (f"-{variant}" if variant else "")


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    d.set_reduction(lssp_amd.TREE)
    yield d
    d.close()


_HOST = {}


def _host(key, A, bs, level):
    """the independent host path's factors and the oracle's apply and single sweeps on them, computed once"""
    import lssp_amd
    if key not in _HOST:
        n = A[0].size - 1
        L, Dinv, U = lssp_amd.bilu_factor_host(*A, bs, level)
        rhs = uniform(0xB12 + n, n)
        one = O.CSR(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))
        _HOST[key] = dict(L=L, Dinv=Dinv, U=U, rhs=rhs, apply=bilu_apply(n, bs, L, Dinv, U, rhs),
                          lower=O.ilu_apply(O.CSR(n, *L), one, rhs), upper=O.ilu_apply(one, O.CSR(n, *U), rhs))
    return _HOST[key]


def _factors_equal(got, want):
    """((Lp, Lj, Lx), Dinv, (Up, Uj, Ux)) bitwise"""
    return all(np.array_equal(a, b) for a, b in zip((*got[0], got[1], *got[2]), (*want[0], want[1], *want[2])))


def _factors_of(M):
    L, U = M.factors()
    return L, M.diag()[1], U


def _info(M):
    return M.n, M.nnzL, M.nnzU, M.levelsL, M.levelsU


def _apply(dev, M, rhs):
    x, r = dev.vec(rhs.size), dev.vec(rhs.size, rhs)
    M.apply(x, r)
    return x.download()


def _check_pair(dev, Md, Mh, D, e, solve=True, schedules=True):
    """the device-made handle == the host-made one == the independent host path + the oracle's sweeps"""
    import lssp_amd
    n = e["rhs"].size
    assert Md.sweep_layout() == (0, 0, 0) and Mh.sweep_layout() == (0, 0, 0)
    assert _info(Md) == _info(Mh)
    x, z, r = dev.vec(n), dev.vec(n), dev.vec(n, e["rhs"])
    # the apply first: the device state alone, before anything makes the host copies
    Md.apply(x, r)
    Mh.apply(z, r)
    assert np.array_equal(x.download(), e["apply"]) and np.array_equal(z.download(), e["apply"])
    Md.apply(x, r)  # the other pair of shadows
    assert np.array_equal(x.download(), e["apply"])
    x.upload(np.zeros(n))
    Md.apply_async(x, r)
    Md.check()
    assert np.array_equal(x.download(), e["apply"])
    if schedules:
        for which in (0, 1):
            sd, sh = Md.schedule(which), Mh.schedule(which)
            assert sd["origin"] == 1 and sh["origin"] == 0
            assert sd["unit"] == 1
            for key in sd:
                if key != "origin":
                    assert np.array_equal(sd[key], sh[key]), (which, key)
    host = (e["L"], e["Dinv"], e["U"])
    assert _factors_equal(_factors_of(Md), host) and _factors_equal(_factors_of(Mh), host)
    assert _info(Md) == _info(Mh)
    for which, key in ((0, "lower"), (1, "upper")):
        Md.trisolve(which, x, r)
        Mh.trisolve(which, z, r)
        assert np.array_equal(x.download(), e[key]) and np.array_equal(z.download(), e[key]), key
    if solve:
        b = dev.vec(n, uniform(78, n))
        out = []
        for H in (Md, Mh):
            xs = dev.vec(n, np.zeros(n))
            res = lssp_amd.solve(dev, D, H, xs, b, solver=lssp_amd.GMRES, tol_rel=1e-30, tol_abs=1e-30, tol_rb=1e-30,
                                 maxit=10, restart=10, trace_cap=64)
            out.append((res.nits, res.residual, res.trace, xs.download()))
        assert out[0][0] == out[1][0] and out[0][0] > 0 and out[0][1] == out[1][1]
        assert out[0][2].size > 0
        assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


@pytest.mark.parametrize("c", SHAPES, ids=[_name(c) for c in SHAPES])
def test_handle_is_bitwise_the_host_made_one(dev, c):
    import lssp_amd
    dim, N, bs, level, variant = c
    A = block_grid(dim, N, bs, seed=900 + SHAPES.index(c), variant=variant)
    e = _host(("grid", c), A, bs, level)
    if c == (3, 6, 4, 1, None) or c == (3, 4, 8, 0, None):  # exactly the packet limit
        assert max(np.diff(e["L"][0]).max(), np.diff(e["U"][0]).max()) - 1 == 24
    D = lssp_amd.DMat(dev, *A)
    Md = lssp_amd.DILU.bilu_create_dev(dev, D, bs, level=level)
    Mh = lssp_amd.DILU.bilu(dev, *A, bs, level=level)
    _check_pair(dev, Md, Mh, D, e)
    for h in (Md, Mh, D):
        h.close()


def test_default_level_is_one(dev):
    import lssp_amd
    A = block_grid(2, 16, 2, seed=931)
    e = _host(("default", 1), A, 2, 1)
    D = lssp_amd.DMat(dev, *A)
    Md = lssp_amd.DILU.bilu_create_dev(dev, D, 2, level=-1)
    assert np.array_equal(_apply(dev, Md, e["rhs"]), e["apply"])
    assert _factors_equal(_factors_of(Md), (e["L"], e["Dinv"], e["U"]))
    Md.close()
    D.close()


def _random_block_matrix(nb, bs, seed, w=12):
    """A block graph that is no grid: per block row the diagonal block, two blocks drawn left of it and two right
    of it, each side for itself (so the pattern is structurally unsymmetric), inside a window of w block
    columns -- fill stays inside the band, so at bs = 2 a strict row holds at most 2 w = 24 entries at any
    level.  Diagonal blocks 10 I + U(-0.3, 0.3), the others U(-0.3, 0.3).  Returns the CSR and the block rows."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(nb):
        cols = {i}
        if i:
            cols |= {int(c) for c in rng.integers(max(i - w, 0), i, 2)}
        if i < nb - 1:
            cols |= {int(c) for c in rng.integers(i + 1, min(i + w, nb - 1) + 1, 2)}
        rows.append(sorted(cols))
    Ap, Aj, Ax = [0], [], []
    for i in range(nb):
        for r in range(bs):
            for j in rows[i]:
                B = rng.uniform(-0.3, 0.3, bs)
                if j == i:
                    B[r] += 10.0
                Aj += range(j * bs, (j + 1) * bs)
                Ax += B.tolist()
            Ap.append(len(Aj))
    return (np.array(Ap, np.int32), np.array(Aj, np.int32), np.array(Ax)), rows


@pytest.mark.parametrize("level", [1, 2])
def test_a_block_graph_that_is_no_grid(dev, level):
    """Seed 1 was checked on the CPU with lssp_amd.bilu_factor_host (levels 0 / 1 / 2: 5776 / 8588 / 11092
    factor entries, longest strict row 4 / 12 / 20 entries, 966 blocks without their transpose); the
    assertions below repeat that check before anything runs on the GPU."""
    import lssp_amd
    nb, bs = 300, 2
    A, rows = _random_block_matrix(nb, bs, seed=1)
    assert 3.5 < sum(len(r) - 1 for r in rows) / nb < 4.5
    assert any(i not in rows[j] for i, r in enumerate(rows) for j in r)  # structurally unsymmetric
    size = {}
    for lvl in (0, 1, 2):
        e = _host(("rand", lvl), A, bs, lvl)
        size[lvl] = e["L"][1].size + e["U"][1].size
        assert max(np.diff(e["L"][0]).max(), np.diff(e["U"][0]).max()) - 1 <= 24  # the packet sweeps
    assert size[0] < size[1] < size[2]  # level 2 fills beyond level 1
    D = lssp_amd.DMat(dev, *A)
    Md = lssp_amd.DILU.bilu_create_dev(dev, D, bs, level=level)
    Mh = lssp_amd.DILU.bilu(dev, *A, bs, level=level)
    _check_pair(dev, Md, Mh, D, _host(("rand", level), A, bs, level), solve=False)
    for h in (Md, Mh, D):
        h.close()


@pytest.mark.parametrize("level", [0, 1])
def test_born_refactor_eligible(dev, level):
    import lssp_amd
    dim, N, bs = 3, 6, 4
    A0, A1 = block_grid(dim, N, bs, seed=941), block_grid(dim, N, bs, seed=942)
    e0, e1 = _host(("rf0", level), A0, bs, level), _host(("rf1", level), A1, bs, level)
    D = lssp_amd.DMat(dev, *A0)
    M = lssp_amd.DILU.bilu_create_dev(dev, D, bs, level=level)
    assert _factors_equal(_factors_of(M), (e0["L"], e0["Dinv"], e0["U"]))  # the host copies made from the plan
    D.update_values(dev.vec(A1[2].size, A1[2]))
    M.bilu_refactor(D)
    F = lssp_amd.DILU.bilu(dev, *A1, bs, level=level)
    assert np.array_equal(_apply(dev, M, e1["rhs"]), e1["apply"])
    assert np.array_equal(_apply(dev, F, e1["rhs"]), e1["apply"])
    assert _factors_equal(_factors_of(M), (e1["L"], e1["Dinv"], e1["U"]))  # ... and refreshed after the refactor
    assert _factors_equal(_factors_of(F), (e1["L"], e1["Dinv"], e1["U"]))
    _check_pair(dev, M, F, D, e1, solve=False, schedules=False)
    # a handle nobody read the host copies of refactors as well, and reads them afterwards
    D0 = lssp_amd.DMat(dev, *A0)
    M2 = lssp_amd.DILU.bilu_create_dev(dev, D0, bs, level=level)
    M2.bilu_refactor(D)
    assert np.array_equal(_apply(dev, M2, e1["rhs"]), e1["apply"])
    assert _factors_equal(_factors_of(M2), (e1["L"], e1["Dinv"], e1["U"]))
    for h in (M, M2, F, D, D0):
        h.close()


def test_matrix_may_be_closed_before_the_first_apply(dev):
    import lssp_amd
    bs, level = 3, 1
    A = block_grid(3, 8, bs, seed=951)
    e = _host(("life", level), A, bs, level)
    D = lssp_amd.DMat(dev, *A)
    M = lssp_amd.DILU.bilu_create_dev(dev, D, bs, level=level)
    D.close()
    other = lssp_amd.DMat(dev, *block_grid(3, 8, bs, seed=952))  # may reuse the freed arrays
    assert np.array_equal(_apply(dev, M, e["rhs"]), e["apply"])
    assert _factors_equal(_factors_of(M), (e["L"], e["Dinv"], e["U"]))
    x, r = dev.vec(e["rhs"].size), dev.vec(e["rhs"].size, e["rhs"])
    M.trisolve(0, x, r)
    assert np.array_equal(x.download(), e["lower"])
    M.close()
    other.close()


def test_long_rows_fall_back_to_the_host_schedules(dev):
    """4^3 x 8 at level 1: strict rows beyond 24 entries have no packet record, so the handle runs on host-built
    schedules (the sync-free fallback); bitwise the host create's all the same, and as little refactor-eligible"""
    import lssp_amd
    dim, N, bs, level = 3, 4, 8, 1
    A = block_grid(dim, N, bs, seed=961)
    e = _host(("long", level), A, bs, level)
    assert max(np.diff(e["L"][0]).max(), np.diff(e["U"][0]).max()) - 1 > 24
    D = lssp_amd.DMat(dev, *A)
    Md = lssp_amd.DILU.bilu_create_dev(dev, D, bs, level=level)
    Mh = lssp_amd.DILU.bilu(dev, *A, bs, level=level)
    _check_pair(dev, Md, Mh, D, e, schedules=False)
    for M in (Md, Mh):
        with pytest.raises(lssp_amd.LsspError) as err:
            M.bilu_refactor(D)
        assert err.value.status == EUNSUPPORTED
        with pytest.raises(lssp_amd.LsspError) as err:
            M.schedule(0)
        assert err.value.status == EUNSUPPORTED
        assert np.array_equal(_apply(dev, M, e["rhs"]), e["apply"])
    for h in (Md, Mh, D):
        h.close()


def _refused(dev, A, bs, level, status):
    import lssp_amd
    D = lssp_amd.DMat(dev, *A)
    n = A[0].size - 1
    xd, z = dev.vec(n, uniform(0x5EED, n)), dev.vec(n)
    D.mv_mxy(xd, z)
    before = z.download()
    with pytest.raises(lssp_amd.LsspError) as err:
        lssp_amd.DILU.bilu_create_dev(dev, D, bs, level=level)
    assert err.value.status == status
    # the matrix still multiplies as before, and the context still creates
    z.upload(np.zeros(n))
    D.mv_mxy(xd, z)
    assert np.array_equal(z.download(), before) and np.any(before != 0)
    D.close()
    good = block_grid(2, 16, 2, seed=971)
    e = _host(("good", 0), good, 2, 0)
    G = lssp_amd.DMat(dev, *good)
    M = lssp_amd.DILU.bilu_create_dev(dev, G, 2, level=0)
    assert np.array_equal(_apply(dev, M, e["rhs"]), e["apply"])
    M.close()
    G.close()


REFUSALS = {
    "shuffled": (lambda: block_grid(3, 6, 4, seed=981, shuffle=True), 4, 0, EUNSUPPORTED),
    "nodiag": (lambda: block_grid(2, 16, 2, seed=982, variant="nodiag"), 2, 0, EUNSUPPORTED),
    "nodiag-l1": (lambda: block_grid(2, 16, 2, seed=982, variant="nodiag"), 2, 1, EUNSUPPORTED),
    "bs9": (lambda: block_grid(3, 3, 9, seed=983), 9, 0, EUNSUPPORTED),
    "level255": (lambda: block_grid(2, 16, 2, seed=984), 2, 255, EUNSUPPORTED),
    "zerodiag": (lambda: block_grid(2, 16, 2, seed=985, variant="zerodiag"), 2, 0, EINVAL),
    "n-not-a-multiple": (lambda: block_grid(2, 16, 2, seed=986), 3, 0, EINVAL),
    "bs33": (lambda: block_grid(2, 16, 2, seed=986), 33, 0, EINVAL),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_leave_matrix_and_context_usable(dev, name):
    make, bs, level, status = REFUSALS[name]
    _refused(dev, make(), bs, level, status)


def test_repeated_column_and_null_arguments(dev):
    import ctypes

    import lssp_amd
    Ap, Aj, Ax = (a.copy() for a in block_grid(2, 16, 2, seed=987))
    Aj = np.insert(Aj, Ap[6], Aj[Ap[6] - 1])  # row 5's last column again
    Ax = np.insert(Ax, Ap[6], 0.625)
    Ap[6:] += 1
    _refused(dev, (Ap, Aj, Ax), 2, 0, EUNSUPPORTED)
    A = block_grid(2, 16, 2, seed=988)
    D = lssp_amd.DMat(dev, *A)
    h = ctypes.c_void_p(7)
    assert dev.L.lssp_amd_bilu_create_dev(None, D.h, 0, 2, ctypes.byref(h)) == EINVAL and h.value is None
    h = ctypes.c_void_p(7)
    assert dev.L.lssp_amd_bilu_create_dev(dev.h, None, 0, 2, ctypes.byref(h)) == EINVAL and h.value is None
    assert dev.L.lssp_amd_bilu_create_dev(dev.h, D.h, 0, 2, None) == EINVAL
    D.close()


def test_no_host_copy_of_the_matrix(dev):
    """the matrix handle made from arrays in HBM (DIdx / DVec), the arrays freed before the create"""
    import lssp_amd
    bs, level = 4, 1
    A = block_grid(3, 6, bs, seed=991)
    e = _host(("fromdev", level), A, bs, level)
    Ap, Aj, Ax = A
    n = Ap.size - 1
    dAp, dAj, dAx = dev.idx(Ap.size, Ap), dev.idx(Aj.size, Aj), dev.vec(Ax.size, Ax)
    D = lssp_amd.DMat.from_device(dev, n, n, Aj.size, dAp, dAj, dAx)
    for a in (dAp, dAj, dAx):
        a.free()
    M = lssp_amd.DILU.bilu_create_dev(dev, D, bs, level=level)
    Mh = lssp_amd.DILU.bilu(dev, *A, bs, level=level)
    _check_pair(dev, M, Mh, D, e, solve=False)
    for h in (M, Mh, D):
        h.close()
