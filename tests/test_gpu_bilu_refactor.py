"""New values on an unchanged block pattern for BILUK handles
(lssp_amd_bilu_refactor; GPU box only).

A handle made by lssp_amd_bilu_create (bs <= 8, packet sweeps) is factored again
from a device matrix with the same block graph.  Expected values come from the
host path (lssp_amd.bilu_factor_host, bitwise the device path) and the oracle's
sweeps on those factors (bilu_util.bilu_apply); every refreshed handle is also
compared with a fresh DILU.bilu on the new values.  All comparisons are bitwise
(np.array_equal).  Handles outside the scope answer "unsupported", a matrix with
another block graph or a singular diagonal block "invalid argument", and the
handle stays as it was.
"""
import numpy as np
import pytest

import oracle as O
from bilu_util import CASES, bilu_apply, block_grid, case_name
from inputs import uniform

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = 1, 6
SHAPES = [c for c in CASES if c[2] <= 8] + [(3, 6, 2, 0, False, None)]  # the last one: EP 8 records


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    d.set_reduction(lssp_amd.TREE)
    yield d
    d.close()


def _identity(n):
    return O.CSR(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))


def _factors_equal(got, want):
    """((Lp, Lj, Lx), Dinv, (Up, Uj, Ux)) bitwise"""
    return all(np.array_equal(a, b) for a, b in zip((*got[0], got[1], *got[2]), (*want[0], want[1], *want[2])))


def _factors_of(M):
    L, U = M.factors()
    return L, M.diag()[1], U


def _apply(dev, M, rhs):
    x, r = dev.vec(rhs.size), dev.vec(rhs.size, rhs)
    M.apply(x, r)
    return x.download()


def _matrix_for(dev, D, old, new):
    """D holding `new`: values updated in place where the scalar pattern is old's, else a new handle"""
    import lssp_amd
    if D is not None and np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1]):
        D.update_values(dev.vec(new[2].size, new[2]))
        return D
    if D is not None:
        D.close()
    return lssp_amd.DMat(dev, *new)


def _check_against_fresh(dev, M, D, A, bs, level, full=True):
    """M (refreshed to A's values; D holds A) == the host path, the oracle's apply and a fresh handle"""
    import lssp_amd
    n = A[0].size - 1
    host = lssp_amd.bilu_factor_host(*A, bs, level)
    F = lssp_amd.DILU.bilu(dev, *A, bs, level=level)
    assert (M.nnzL, M.nnzU, M.levelsL, M.levelsU) == (F.nnzL, F.nnzU, F.levelsL, F.levelsU)
    assert M.sweep_layout() == (0, 0, 0)
    rhs = uniform(0xB12 + n, n)
    want = bilu_apply(n, bs, host[0], host[1], host[2], rhs)
    x, z, r = dev.vec(n), dev.vec(n), dev.vec(n, rhs)
    # the apply first: the device state alone, before anything refreshes the host copies
    M.apply(x, r)
    F.apply(z, r)
    assert np.array_equal(x.download(), want) and np.array_equal(z.download(), want)
    M.apply(x, r)  # the other pair of shadows
    assert np.array_equal(x.download(), want)
    if full:
        x.upload(np.zeros(n))
        M.apply_async(x, r)
        M.check()
        assert np.array_equal(x.download(), want)
        # both single sweeps (their arrays are rebuilt from the refreshed host copies)
        one = _identity(n)
        for which, ref in ((0, O.ilu_apply(O.CSR(n, *host[0]), one, rhs)), (1, O.ilu_apply(one, O.CSR(n, *host[2]), rhs))):
            M.trisolve(which, x, r)
            F.trisolve(which, z, r)
            assert np.array_equal(x.download(), ref) and np.array_equal(z.download(), ref), which
        # a short solve: same iterates, same count, same residual
        b = dev.vec(n, uniform(78, n))
        out = []
        for H in (M, F):
            xs = dev.vec(n, np.zeros(n))
            res = lssp_amd.solve(dev, D, H, xs, b, solver=lssp_amd.GMRES, tol_rel=1e-12, maxit=20, restart=10,
                                 trace_cap=64)
            out.append((res.nits, res.residual, res.trace, xs.download()))
        assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
        assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])
    got = _factors_of(M)
    assert _factors_equal(got, host) and _factors_equal(_factors_of(F), host)
    F.close()


@pytest.mark.parametrize("c", SHAPES, ids=[case_name(c) for c in SHAPES])
def test_refresh_is_bitwise_a_fresh_create(dev, c):
    import lssp_amd
    dim, N, bs, level, shuffle, variant = c
    s = 500 + 3 * SHAPES.index(c)
    A = [block_grid(dim, N, bs, seed=s + k, shuffle=shuffle, variant=variant) for k in range(3)]
    n = A[0][0].size - 1
    M = lssp_amd.DILU.bilu(dev, *A[0], bs, level=level)
    rhs = uniform(0xB12 + n, n)
    want0 = _apply(dev, M, rhs)
    orig = _factors_of(M)
    x, r = dev.vec(n), dev.vec(n, rhs)
    M.trisolve(0, x, r)  # builds the single sweeps' arrays from the old values: the refactor must drop them
    D = _matrix_for(dev, None, None, A[0])
    D = _matrix_for(dev, D, A[0], A[1])
    M.bilu_refactor(D)
    _check_against_fresh(dev, M, D, A[1], bs, level)
    D = _matrix_for(dev, D, A[1], A[2])
    M.bilu_refactor(D)  # the kept plan
    _check_against_fresh(dev, M, D, A[2], bs, level, full=False)
    D = _matrix_for(dev, D, A[2], A[0])
    M.bilu_refactor(D)
    assert np.array_equal(_apply(dev, M, rhs), want0)
    assert _factors_equal(_factors_of(M), orig)
    M.close()
    D.close()


def _random_blocks(nb, per, bs, seed):
    """a random block pattern (about per + 1 blocks a row, the diagonal block present and
    dominant), vectorised; rows column-sorted"""
    rng = np.random.default_rng(seed)
    cols = np.concatenate([np.arange(nb)[:, None], rng.integers(0, nb, (nb, per))], axis=1)
    cols.sort(axis=1)
    keep = np.ones_like(cols, bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    bi = np.repeat(np.arange(nb), per + 1)[keep.reshape(-1)]
    bj = cols.reshape(-1)[keep.reshape(-1)]
    cnt = np.bincount(bi, minlength=nb)
    # scalar rows: row i*bs + r holds, per block of cell i, the bs columns j*bs ..
    Bp = np.concatenate([[0], np.cumsum(cnt)])
    Ap = np.zeros(nb * bs + 1, np.int64)
    Ap[1:] = np.cumsum(np.repeat(cnt * bs, bs))
    Aj = np.concatenate([(bj[Bp[i]:Bp[i + 1], None] * bs + np.arange(bs)[None, :]).reshape(-1)
                         for i in range(nb) for _ in range(bs)])
    return Ap.astype(np.int32), Aj.astype(np.int32), Bp


def _random_values(Ap, Aj, bs, seed):
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(Ap.size - 1), np.diff(Ap))
    Ax = rng.uniform(-0.3, 0.3, Aj.size)
    Ax[rows == Aj] += 10.0  # 5 off-diagonal blocks of bs entries below 0.3 each against 10
    return Ax


def test_steps_split_into_several_packets(dev):
    import lssp_amd
    nb, per, bs = 1500, 5, 2
    Ap, Aj, _ = _random_blocks(nb, per, bs, seed=42)
    A0, A1 = (Ap, Aj, _random_values(Ap, Aj, bs, 1)), (Ap, Aj, _random_values(Ap, Aj, bs, 2))
    n = nb * bs
    # on the CPU first: some level of L holds more than 256 rows inside one schedule block
    # (blocks of max(64, bandwidth) rows, build_bp_schedule), so that step is several packets
    (Lp, Lj, _), _, _ = lssp_amd.bilu_factor_host(*A0, bs, 0)
    rows = np.repeat(np.arange(n), np.diff(Lp))
    strict = Lj != rows
    B = min(n, max(64, int(np.max(rows[strict] - Lj[strict]))))
    lev = np.zeros(n, np.int64)
    for i in range(n):
        k = Lj[Lp[i]:Lp[i + 1] - 1]
        if k.size:
            lev[i] = lev[k].max() + 1
    widest = max(np.bincount(lev[q:q + B]).max() for q in range(0, n, B))
    assert widest > 256, widest
    assert np.diff(Lp).max() - 1 <= 24  # and the rows fit a packet record
    M = lssp_amd.DILU.bilu(dev, *A0, bs, level=0)
    D = lssp_amd.DMat(dev, *A0)
    D.update_values(dev.vec(A1[2].size, A1[2]))
    M.bilu_refactor(D)
    _check_against_fresh(dev, M, D, A1, bs, 0, full=False)
    M.close()
    D.close()


def test_same_block_graph_other_scalar_pattern(dev):
    import lssp_amd
    bs = 2
    full = block_grid(2, 16, bs, seed=31)
    holes = block_grid(2, 16, bs, seed=32, variant="holes")
    assert holes[1].size < full[1].size
    M = lssp_amd.DILU.bilu(dev, *full, bs, level=0)
    D = lssp_amd.DMat(dev, *holes)
    M.bilu_refactor(D)
    _check_against_fresh(dev, M, D, holes, bs, 0, full=False)
    # and duplicated columns: the last occurrence in storage order counts, as on the host path
    Ap, Aj, Ax = (a.copy() for a in full)
    n = Ap.size - 1
    k = np.arange(Ap[5], Ap[6])
    Aj = np.insert(Aj, Ap[6], Aj[k[0]])
    Ax = np.insert(Ax, Ap[6], 0.625)
    Ap[6:] += 1
    D2 = lssp_amd.DMat(dev, Ap, Aj, Ax)
    M.bilu_refactor(D2)
    host = lssp_amd.bilu_factor_host(Ap, Aj, Ax, bs, 0)
    assert _factors_equal(_factors_of(M), host)
    rhs = uniform(0xB12 + n, n)
    assert np.array_equal(_apply(dev, M, rhs), bilu_apply(n, bs, host[0], host[1], host[2], rhs))
    for h in (M, D, D2):
        h.close()


def _refused(dev, M, D, status, rhs, want):
    import lssp_amd
    with pytest.raises(lssp_amd.LsspError) as e:
        M.bilu_refactor(D)
    assert e.value.status == status
    assert np.array_equal(_apply(dev, M, rhs), want)


def test_einval_leaves_the_handle_as_it_was_and_refactorable(dev):
    import lssp_amd
    dim, N, bs = 2, 16, 2
    A0 = block_grid(dim, N, bs, seed=61)
    A1 = block_grid(dim, N, bs, seed=62)
    Ap, Aj, Ax = A0
    n = Ap.size - 1
    nb = n // bs
    rhs = uniform(0xB12 + n, n)
    M = lssp_amd.DILU.bilu(dev, *A0, bs, level=0)
    want = _apply(dev, M, rhs)
    orig = _factors_of(M)

    moved = Aj.copy()  # row 0's last entry into the block of the far corner cell, which row 0 lacks
    moved[Ap[1] - 1] = (nb - 1) * bs
    emptied = np.ones(Aj.size, bool)  # cell 0's block of its +1 neighbour removed from both of its rows
    for r in range(bs):
        seg = slice(Ap[r], Ap[r + 1])
        emptied[seg] = Aj[seg] // bs != 1
    Ep = np.concatenate([[0], np.cumsum([emptied[Ap[r]:Ap[r + 1]].sum() for r in range(n)])]).astype(np.int32)
    cases = {
        "moved": (Ap, moved, Ax),
        "emptied": (Ep, Aj[emptied], Ax[emptied]),
        "other n": block_grid(dim, N - 1, bs, seed=61),
        "singular": block_grid(dim, N, bs, seed=61, variant="zerodiag"),
    }
    good = lssp_amd.DMat(dev, *A1)
    host1 = lssp_amd.bilu_factor_host(*A1, bs, 0)
    want1 = bilu_apply(n, bs, host1[0], host1[1], host1[2], rhs)
    for name, Abad in cases.items():
        D = lssp_amd.DMat(dev, *Abad)
        _refused(dev, M, D, EINVAL, rhs, want)
        assert _factors_equal(_factors_of(M), orig), name
        D.close()
        # the handle still refactors: to A1, and back, so that the next case starts from A0 again
        M.bilu_refactor(good)
        assert np.array_equal(_apply(dev, M, rhs), want1), name
        # a refusal after a refactor nobody read the host copies of: they must still become A1's
        D = lssp_amd.DMat(dev, *Abad)
        _refused(dev, M, D, EINVAL, rhs, want1)
        assert _factors_equal(_factors_of(M), host1), name
        D.close()
        back = lssp_amd.DMat(dev, *A0)
        M.bilu_refactor(back)
        assert np.array_equal(_apply(dev, M, rhs), want), name
        back.close()
    good.close()
    M.close()


def test_handles_outside_the_scope_are_unsupported(dev):
    import lssp_amd
    from bilu_util import diag_csr
    # an ILUK handle
    Ap, Aj, Ax = lssp_amd.poisson(3, 6)
    n = Ap.size - 1
    rhs = uniform(9, n)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0)
    _refused(dev, M, D, EUNSUPPORTED, rhs, _apply(dev, M, rhs))
    M.close()
    D.close()
    # caller-made factors
    A = block_grid(2, 16, 2, seed=71)
    n = A[0].size - 1
    rhs = uniform(9, n)
    L, Dinv, U = lssp_amd.bilu_factor_host(*A, 2, 0)
    Dc = diag_csr(n, 2, Dinv)
    M = lssp_amd.DILU.from_ldu(dev, L, (Dc.Ap, Dc.Aj, Dc.Ax), U)
    D = lssp_amd.DMat(dev, *A)
    _refused(dev, M, D, EUNSUPPORTED, rhs, bilu_apply(n, 2, L, Dinv, U, rhs))
    M.close()
    D.close()
    # bs 9: the host numeric path; and bs 8 at level 1 in 3-D: rows past the longest packet record
    for dim, N, bs, level in ((3, 3, 9, 0), (3, 4, 8, 1)):
        A = block_grid(dim, N, bs, seed=72)
        n = A[0].size - 1
        rhs = uniform(9, n)
        M = lssp_amd.DILU.bilu(dev, *A, bs, level=level)
        L, U = M.factors()
        assert M.sweep_layout() == (0, 0, 0)
        # a strict row of more than 24 entries has no packet record (build_packets6): such a factor
        # runs the sync-free sweeps
        assert max(np.diff(L[0]).max(), np.diff(U[0]).max()) - 1 > 24
        D = lssp_amd.DMat(dev, *A)
        _refused(dev, M, D, EUNSUPPORTED, rhs, bilu_apply(n, bs, L, M.diag()[1], U, rhs))
        M.close()
        D.close()
