"""lssp_amd_pc_create_dev: one call for every preconditioner handle made from a
matrix that lives in HBM, and its general ILUK route -- the symbolic ILU(k)
factorization on the device, a wavefront per row (GPU box only).

Every observable of a general-route handle -- counts, level counts, factors,
applies (one enqueued), both single sweeps, a whole BiCGSTAB solve -- is
compared bit for bit (np.array_equal) with the CPU oracle AND with the handle
lssp_amd_ilu_create(kind ILUK, level) makes from the same arrays on the host;
its sweep layout is (0, 0, 0).  The handle is born refactorable.  Everything
outside the scope answers "unsupported" (a non-square handle "invalid
argument") and leaves the matrix and the context usable.  No test provokes a
timeout or a fault.
"""
import numpy as np
import pytest

import oracle as O
from ilut_inputs import arrow, csr, tridiag
from inputs import uniform
from pc_create_inputs import box, five, oracle_rows, pattern, symbolic, values

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


_ORACLE = {}


def _expected(key, Ap, Aj, Ax, level):
    """the oracle's results for one matrix, computed once: factors, four applies, both sweeps"""
    if key not in _ORACLE:
        n = Ap.size - 1
        A = O.CSR(n, Ap, Aj, Ax)
        L, U = O.ilu(A, "iluk", level=level)
        one = _identity(n)
        _ORACLE[key] = dict(A=A, L=L, U=U,
                            applies=[O.ilu_apply(L, U, uniform(200 + rep, n)) for rep in range(4)],
                            lower=O.ilu_apply(L, one, uniform(300, n)),
                            upper=O.ilu_apply(one, U, uniform(300, n)))
    return _ORACLE[key]


def _info(M):
    return M.n, M.nnzL, M.nnzU, M.levelsL, M.levelsU


def _same_factors(M, L, U):
    (Lp, Lj, Lx), (Up, Uj, Ux) = M.factors()
    return (np.array_equal(Lp, L.Ap) and np.array_equal(Lj, L.Aj) and np.array_equal(Lx, L.Ax)
            and np.array_equal(Up, U.Ap) and np.array_equal(Uj, U.Aj) and np.array_equal(Ux, U.Ax))


def _check_pair(dev, Md, Mh, e, factors=True):
    """the device-made handle == the oracle == the host-made handle, in everything the C-ABI shows"""
    n = e["A"].n
    assert Md.sweep_layout() == NOLINES
    assert _info(Md) == _info(Mh)
    assert (Md.nnzL, Md.nnzU) == (e["L"].Aj.size, e["U"].Aj.size)
    if factors:
        assert _same_factors(Md, e["L"], e["U"])
        assert _same_factors(Mh, e["L"], e["U"])
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


def _matrix(name):
    """(Ap, Aj, Ax) of a named create case"""
    if name == "tridiag5000":
        return tridiag(5000)
    if name == "five":
        return five()
    if name == "n1":
        return csr([{0: 2.5}])
    if name == "n2":
        return csr([{0: 2.0, 1: -1.0}, {0: -1.0, 1: 2.0}])
    Ap, Aj = pattern(name)
    return Ap, Aj, values(Ap, Aj, 0)


def _both(dev, name, level):
    import lssp_amd
    Ap, Aj, Ax = _matrix(name)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Md = lssp_amd.DILU.pc_create_dev(dev, D, level=level)
    D.close()  # the handle owns what it needs
    host_level = 1 if level < 0 else level
    Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=host_level)
    _check_pair(dev, Md, Mh, _expected((name, host_level, 0), Ap, Aj, Ax, host_level))
    return Md, Mh


# strict rows of 21 at box786 level 4 (EP 24); an nx == 2 box, which the box
# create refuses, at the default level; tridiag5000: every row waits for the row
# before it, across workgroups and XCDs; rand6: an irregular pattern on which
# the reference's level rule bites at level 1
CREATE_CASES = [("holed", 0), ("holed", 1), ("holed", 2), ("rand6", 0), ("rand6", 1), ("grid5", 2), ("box786", 4),
                ((9, 21, 13), 2), ((2, 9, 9), -1), ("tridiag5000", 1), ("five", 1), ("n1", 1), ("n2", 1)]


def _id(c):
    name, level = c
    return "%s-l%s" % (name if isinstance(name, str) else "x".join(map(str, name)), "default" if level < 0 else level)


@pytest.mark.parametrize("name,level", CREATE_CASES, ids=[_id(c) for c in CREATE_CASES])
def test_general_route_equals_host_create(dev, name, level):
    if (name, level) == ("rand6", 1):  # the case discriminates between the reference's level rule and the textbook's
        Ap, Aj = pattern("rand6")
        assert symbolic(Ap, Aj, 1, rule="min") != symbolic(Ap, Aj, 1)
    if name == "five":
        Ap, Aj = pattern("five")
        assert symbolic(Ap, Aj, 1)[3] == [0, 1, 3] and symbolic(Ap, Aj, 1, rule="min")[3] == [0, 1, 3, 4]
    for h in _both(dev, name, level):
        h.close()


def test_restatement_is_the_oracles_pattern_on_rand6():
    """what the min-rule assertions rest on: the max-rule restatement is the oracle's pattern"""
    Ap, Aj, Ax = _matrix("rand6")
    e = _expected(("rand6", 1, 0), Ap, Aj, Ax, 1)
    assert oracle_rows(e["L"], e["U"]) == symbolic(Ap, Aj, 1)


def test_schedules_are_built_on_the_device_and_equal_the_hosts(dev):
    Md, Mh = _both(dev, "holed", 1)
    for which in (0, 1):
        sd, sh = Md.schedule(which), Mh.schedule(which)
        assert sd["origin"] == 1 and sh["origin"] == 0
        for key in sd:
            if key != "origin":
                assert np.array_equal(sd[key], sh[key]), (which, key)
    for h in (Md, Mh):
        h.close()


def test_long_rows_fall_back_to_the_host_schedules(dev):
    """arrow(400) at level 0: row 0 holds 399 strict entries, beyond the 24 of the device schedule builder, so
    the handle runs on host-built schedules (the sync-free fallback); bitwise the host create's all the same,
    and as little refactor-eligible"""
    import lssp_amd
    Ap, Aj, Ax = arrow(400)
    assert np.diff(Ap).max() - 1 > 24
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Md = lssp_amd.DILU.pc_create_dev(dev, D, level=0)
    Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0)
    _check_pair(dev, Md, Mh, _expected(("arrow400", 0, 0), Ap, Aj, Ax, 0))
    for M in (Md, Mh):
        with pytest.raises(lssp_amd.LsspError) as err:
            M.iluk_refactor(D)
        assert err.value.status == EUNSUPPORTED
        with pytest.raises(lssp_amd.LsspError) as err:
            M.schedule(0)
        assert err.value.status == EUNSUPPORTED
    for h in (Md, Mh, D):
        h.close()


def test_routing_keeps_the_line_sweeps_of_a_box_and_serves_ilut(dev):
    import lssp_amd
    Ap, Aj = box(9, 21, 13)
    Ax = values(Ap, Aj, 0)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    M1 = lssp_amd.DILU.pc_create_dev(dev, D, level=1)
    assert M1.sweep_layout() == (2, 16, 8)
    M0 = lssp_amd.DILU.pc_create_dev(dev, D, level=0)
    assert M0.sweep_layout() == (1, 16, 8)
    Mt = lssp_amd.DILU.pc_create_dev(dev, D, kind=lssp_amd.ILUT, tol=1e-3, p=5)
    Mi = lssp_amd.DILU.ilut_create_dev(dev, D, tol=1e-3, p=5)
    for a, b in zip(sum(Mt.factors(), ()), sum(Mi.factors(), ())):
        assert np.array_equal(a, b)
    with pytest.raises(lssp_amd.LsspError) as err:
        Mt.iluk_refactor(D)
    assert err.value.status == EUNSUPPORTED
    for h in (M1, M0, Mt, Mi, D):
        h.close()


def _state(dev, M, e, fresh, factors=True):
    """handle state == the oracle's and a fresh host-made handle's"""
    n = e["A"].n
    if factors:
        assert _same_factors(M, e["L"], e["U"])
    x, z = dev.vec(n), dev.vec(n)
    for rep in range(4):
        r = dev.vec(n, uniform(200 + rep, n))
        M.apply(x, r)
        assert np.array_equal(x.download(), e["applies"][rep]), rep
        fresh.apply(z, r)
        assert np.array_equal(x.download(), z.download()), rep
    r = dev.vec(n, uniform(300, n))
    for which, key in ((0, "lower"), (1, "upper")):
        M.trisolve(which, z, r)
        assert np.array_equal(z.download(), e[key]), key


@pytest.mark.parametrize("read", [True, False], ids=["factors-read", "factors-unread"])
@pytest.mark.parametrize("name,level", [("holed", 1), ("rand6", 0)], ids=["holed-l1", "rand6-l0"])
def test_born_refactorable(dev, name, level, read):
    """iluk_refactor on the device-made handle, nothing built first: values 1, 2, then the creation values again,
    with factors() read between the steps or not (the lazy host refresh)"""
    import lssp_amd
    Ap, Aj = pattern(name)
    D = lssp_amd.DMat(dev, Ap, Aj, values(Ap, Aj, 0))
    M = lssp_amd.DILU.pc_create_dev(dev, D, level=level)
    assert M.sweep_layout() == NOLINES
    info = _info(M)
    for k in (1, 2, 0):
        Ax = values(Ap, Aj, k)
        D.update_values(dev.vec(Ax.size, Ax))
        M.iluk_refactor(D)
        fresh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=level)
        _state(dev, M, _expected((name, level, k), Ap, Aj, Ax, level), fresh, factors=read or k == 0)
        assert _info(M) == info == _info(fresh)
        fresh.close()
    for h in (M, D):
        h.close()


def test_an_entry_on_a_fill_position_is_refused(dev):
    import lssp_amd
    Ap, Aj = pattern("holed")
    Ax = values(Ap, Aj, 0)
    n = Ap.size - 1
    e = _expected(("holed", 1, 0), Ap, Aj, Ax, 1)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    M = lssp_amd.DILU.pc_create_dev(dev, D, level=1)
    L = e["L"]
    fill = None
    for row in range(n // 2, n):
        have = set(Aj[Ap[row]:Ap[row + 1]].tolist())
        extra = [c for c in L.Aj[L.Ap[row]:L.Ap[row + 1]].tolist() if c not in have]
        if extra:
            fill = (row, extra[0])
            break
    assert fill is not None
    row, col = fill
    at = Ap[row] + int(np.searchsorted(Aj[Ap[row]:Ap[row + 1]], col))
    Ap2 = Ap.copy()
    Ap2[row + 1:] += 1
    other = lssp_amd.DMat(dev, Ap2, np.insert(Aj, at, col).astype(np.int32), np.insert(Ax, at, 0.25))
    with pytest.raises(lssp_amd.LsspError) as err:
        M.iluk_refactor(other)
    assert err.value.status == EINVAL
    x = dev.vec(n)
    M.apply(x, dev.vec(n, uniform(200, n)))
    assert np.array_equal(x.download(), e["applies"][0])
    assert _same_factors(M, e["L"], e["U"])
    for h in (other, M, D):
        h.close()


def test_coo_to_iluk_preconditioned_bicgstab_without_a_host_matrix(dev):
    """permuted COO in HBM -> coo_to_csr -> sort_columns -> from_device -> pc_create_dev(level 1) -> BiCGSTAB on
    the holed box, b = 1, SERIAL reductions: the solve with the host-made handle, bit for bit"""
    import lssp_amd
    from lssp_amd import convert as C
    Ap, Aj = pattern("holed")
    Ax = values(Ap, Aj, 0)
    n, nnz = Ap.size - 1, Aj.size
    perm = np.random.default_rng(8).permutation(nnz)
    Ci = np.repeat(np.arange(n, dtype=np.int32), np.diff(Ap))[perm]
    coo = dev.idx(nnz, Ci), dev.idx(nnz, Aj[perm]), dev.vec(nnz, Ax[perm])
    csr_d = C.coo_to_csr(dev, n, nnz, *coo)
    C.sort_columns(dev, n, n, nnz, *csr_d)
    D = lssp_amd.DMat.from_device(dev, n, n, nnz, *csr_d)
    Md = lssp_amd.DILU.pc_create_dev(dev, D, level=1)
    assert Md.sweep_layout() == NOLINES
    for a in (*coo, *csr_d):
        a.free()
    Dh = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=1)
    kw = dict(solver=lssp_amd.BICGSTAB, tol_rel=1e-9, tol_abs=1e-9, tol_rb=1e-9, maxit=200, trace_cap=100000)
    dev.set_reduction(lssp_amd.SERIAL)
    try:
        x, xh, b = dev.vec(n, np.zeros(n)), dev.vec(n, np.zeros(n)), dev.vec(n, np.ones(n))
        r = lssp_amd.solve(dev, D, Md, x, b, **kw)
        rh = lssp_amd.solve(dev, Dh, Mh, xh, b, **kw)
    finally:
        dev.set_reduction(lssp_amd.TREE)
    assert r.nits == rh.nits and 0 < r.nits < 200
    assert r.residual == rh.residual
    assert np.array_equal(r.trace, rh.trace)
    assert np.array_equal(x.download(), xh.download())
    for h in (Dh, Mh, D, Md):
        h.close()


def _refusal_input(case):
    import lssp_amd
    Ap, Aj = pattern("box786")
    Ax = values(Ap, Aj, 0)
    n = Ap.size - 1
    mid = n // 2
    kw = dict(level=1)
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
        Ap, Aj, Ax = arrow(cap + 2)  # row 0 holds cap + 1 entries right of its diagonal
    elif case == "level255":
        kw = dict(level=255)
    else:
        assert case == "non-square"
    return Ap, Aj, Ax, kw


REFUSED = ["unsorted", "repeated-column", "diagonal-deleted", "block-jacobi", "capacity", "level255", "non-square"]


@pytest.mark.parametrize("case", REFUSED)
def test_refusals_leave_everything_usable(dev, case):
    import ctypes
    import lssp_amd
    Ap, Aj, Ax, kw = _refusal_input(case)
    n = Ap.size - 1
    ncols = n + 1 if case == "non-square" else n
    D = lssp_amd.DMat(dev, Ap, Aj, Ax, ncols=ncols)
    with pytest.raises(lssp_amd.LsspError) as err:
        lssp_amd.DILU.pc_create_dev(dev, D, **kw)
    assert err.value.status == (EINVAL if case == "non-square" else EUNSUPPORTED)
    h = ctypes.c_void_p(1)  # no handle comes back: *out is cleared
    st = dev.L.lssp_amd_pc_create_dev(dev.h, D.h, lssp_amd.ILUK, kw["level"], 1e-3, -1, kw.get("blk", 0),
                                      ctypes.byref(h))
    assert st == (EINVAL if case == "non-square" else EUNSUPPORTED) and h.value is None
    # the matrix still multiplies ...
    xh = uniform(0x5EED, ncols)
    z = dev.vec(n)
    D.mv_mxy(dev.vec(ncols, xh), z)
    assert np.array_equal(z.download(), O.spmv(0, O.CSR(n, Ap, Aj, Ax), xh))
    D.close()
    # ... and the context still makes an eligible handle
    Md, Mh = _both(dev, "five", 1)
    with pytest.raises(lssp_amd.LsspError) as err:  # (eligible: the pattern rule answers, not "unsupported")
        Md.iluk_refactor(lssp_amd.DMat(dev, *_matrix("n2")))
    assert err.value.status == EINVAL
    for hh in (Md, Mh):
        hh.close()
