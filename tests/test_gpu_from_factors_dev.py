"""lssp_amd_ilu_from_factors_dev and lssp_amd_ilu_get_schedule: a handle made from factors that
live in HBM, both packet schedules built on the device (GPU box only).

For every case of sched_inputs.CASES the device-made handle Md is compared with the handle Mh that
lssp_amd_ilu_from_factors makes from the same arrays on the host: the schedules (every header field
and every stream, np.array_equal; origin 1 against 0), the counts and levels, the factors read back,
four applies (one enqueued) and both single sweeps -- bitwise the CPU oracle's and Mh's -- and one
GMRES(30) solve, trace for trace.  Each case first asserts, on the HOST-made schedule, that it
exercises what it is named for (sched_inputs.check_case).  A grid's ILU(0), which the host puts
on line sweeps, is compared with the oracle alone.  Refusals leave the context usable.
"""
import numpy as np
import pytest

import oracle as O
import sched_inputs as S
from inputs import uniform

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = 1, 6
NOLINES = (0, 0, 0)
ARRAYS = ("blk", "desc", "rec", "idx", "perm", "pos")


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


def _identity(n):
    return O.CSR(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))


def _expected(L, U):
    """the oracle's results for one factor pair: four applies, both sweeps"""
    n = L[0].size - 1
    Lo, Uo, one = O.CSR(n, *L), O.CSR(n, *U), _identity(n)
    return dict(applies=[O.ilu_apply(Lo, Uo, uniform(200 + rep, n)) for rep in range(4)],
                lower=O.ilu_apply(Lo, one, uniform(300, n)), upper=O.ilu_apply(one, Uo, uniform(300, n)))


def _from_dev(dev, L, U):
    import lssp_amd
    d = [dev.idx(L[0].size, L[0]), dev.idx(L[1].size, L[1]), dev.vec(L[2].size, L[2]),
         dev.idx(U[0].size, U[0]), dev.idx(U[1].size, U[1]), dev.vec(U[2].size, U[2])]
    try:
        return lssp_amd.DILU.from_factors_dev(dev, d[:3], d[3:])
    finally:
        for a in d:  # the handle owns what it needs
            a.free()


def _info(M):
    return M.n, M.nnzL, M.nnzU, M.levelsL, M.levelsU


def _sweeps_equal_oracle(dev, Md, e, Mh=None):
    n = Md.n
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
        if Mh is not None:
            Mh.apply(z, r)
            assert np.array_equal(got, z.download()), rep
    r = dev.vec(n, uniform(300, n))
    for which, key in ((0, "lower"), (1, "upper")):
        Md.trisolve(which, x, r)
        assert np.array_equal(x.download(), e[key]), key
        if Mh is not None:
            Mh.trisolve(which, z, r)
            assert np.array_equal(x.download(), z.download()), key


def _tridiag(n):
    """the matrix of the GMRES run: 4 on the diagonal, -1 beside it"""
    rows = np.repeat(np.arange(n), 3)
    cols = rows + np.tile([-1, 0, 1], n)
    keep = (cols >= 0) & (cols < n)
    Ap = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return Ap, cols[keep].astype(np.int32), np.where(cols[keep] == rows[keep], 4.0, -1.0)


def _schedules_equal(Md, Mh):
    for w in (0, 1):
        sd, sh = Md.schedule(w), Mh.schedule(w)
        assert sd["origin"] == 1 and sh["origin"] == 0
        for k in S.HDR[:-1]:
            assert sd[k] == sh[k], (w, k)
        for k in ARRAYS:
            assert np.array_equal(sd[k], sh[k]), (w, k)


@pytest.mark.parametrize("name,make", S.CASES, ids=[c[0] for c in S.CASES])
def test_from_factors_dev_equals_from_factors(dev, name, make):
    import lssp_amd
    L, U = make()
    n = L[0].size - 1
    Mh = lssp_amd.DILU.from_factors(dev, L, U)
    assert Mh.sweep_layout() == NOLINES
    S.check_case(name, L, U, Mh.schedule(0), Mh.schedule(1))
    Md = _from_dev(dev, L, U)
    assert Md.sweep_layout() == NOLINES
    _schedules_equal(Md, Mh)
    assert _info(Md) == _info(Mh) and (Md.nnzL, Md.nnzU) == (L[1].size, U[1].size)
    _sweeps_equal_oracle(dev, Md, _expected(L, U), Mh)
    for M in (Md, Mh):  # (read after the applies: the device-made handle's host copies are made here)
        got = M.factors()
        for g, w in zip(got[0] + got[1], L + U):
            assert np.array_equal(g, w)
    for call in (Md.refactor, Md.iluk_refactor):
        A = lssp_amd.DMat(dev, *_tridiag(n))
        with pytest.raises(lssp_amd.LsspError) as err:
            call(A)
        assert err.value.status == EUNSUPPORTED
        A.close()
    # one GMRES(30) solve, trace for trace
    A = lssp_amd.DMat(dev, *_tridiag(n))
    kw = dict(solver=lssp_amd.GMRES, maxit=30, restart=30, trace_cap=4096)
    xd, xh, b = dev.vec(n, np.zeros(n)), dev.vec(n, np.zeros(n)), dev.vec(n, np.ones(n))
    rd = lssp_amd.solve(dev, A, Md, xd, b, **kw)
    rh = lssp_amd.solve(dev, A, Mh, xh, b, **kw)
    assert rd.nits == rh.nits and rd.residual == rh.residual
    assert np.array_equal(rd.trace, rh.trace) and np.array_equal(xd.download(), xh.download())
    for h in (A, Md, Mh):
        h.close()


def test_grid_ilu0_runs_the_packet_sweeps(dev):
    """poisson7(8)'s ILU(0): the host-made handle is on line sweeps, the device-made one on packets"""
    import lssp_amd
    L, U = S.ilu0_p7_8()
    Mh = lssp_amd.DILU.from_factors(dev, L, U)
    assert Mh.sweep_layout()[0] == 1
    with pytest.raises(lssp_amd.LsspError) as err:
        Mh.schedule(0)
    assert err.value.status == EUNSUPPORTED
    Md = _from_dev(dev, L, U)
    assert Md.sweep_layout() == NOLINES and Md.schedule(0)["origin"] == 1 and Md.schedule(1)["origin"] == 1
    _sweeps_equal_oracle(dev, Md, _expected(L, U))
    for h in (Md, Mh):
        h.close()


@pytest.mark.parametrize("name,make,status", S.REFUSALS, ids=[c[0] for c in S.REFUSALS])
def test_refusals_leave_the_context_usable(dev, name, make, status):
    import lssp_amd
    L, U = make()
    with pytest.raises(lssp_amd.LsspError) as err:
        _from_dev(dev, L, U)
    assert err.value.status == status
    L, U = S.chain(200)
    Md = _from_dev(dev, L, U)
    _sweeps_equal_oracle(dev, Md, _expected(L, U))
    Md.close()


def test_null_arguments_and_the_out_pointer(dev):
    import ctypes
    L, U = S.chain(50)
    d = [dev.idx(L[0].size, L[0]), dev.idx(L[1].size, L[1]), dev.vec(L[2].size, L[2]),
         dev.idx(U[0].size, U[0]), dev.idx(U[1].size, U[1]), dev.vec(U[2].size, U[2])]
    p = [a.ptr for a in d]
    f = dev.L.lssp_amd_ilu_from_factors_dev
    h = ctypes.c_void_p(1)
    assert f(dev.h, 50, p[0], None, p[2], p[3], p[4], p[5], ctypes.byref(h)) == EINVAL and h.value is None
    h = ctypes.c_void_p(1)
    assert f(dev.h, 0, *p, ctypes.byref(h)) == EINVAL and h.value is None
    assert f(dev.h, 50, *p, None) == EINVAL
    assert dev.L.lssp_amd_ilu_get_schedule(None, 0, None, None, None, None, None, None, None) == EINVAL
    for a in d:
        a.free()


@pytest.mark.parametrize("name", ["p7-8-fill", "rand300"])
def test_ilut_create_dev_builds_its_schedules_on_the_device(dev, name):
    """lssp_amd_ilut_create_dev: the finished factors stay in HBM and go through the device builder"""
    import lssp_amd
    from ilut_inputs import CASES
    make, tol, p = [c[1:] for c in CASES if c[0] == name][0]
    Ap, Aj, Ax = make()
    n = Ap.size - 1
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Md = lssp_amd.DILU.ilut_create_dev(dev, D, tol=tol, p=p)
    D.close()
    Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUT, tol=tol, p=p)
    _schedules_equal(Md, Mh)
    assert _info(Md) == _info(Mh)
    L, U = O.ilu(O.CSR(n, Ap, Aj, Ax), "ilut", tol=tol, p=p)
    x, r = dev.vec(n), uniform(200, n)
    Md.apply(x, dev.vec(n, r))
    assert np.array_equal(x.download(), O.ilu_apply(L, U, r))
    got = Md.factors()  # (read after an apply: the host copies are made here)
    for g, w in zip(got[0] + got[1], (L.Ap, L.Aj, L.Ax, U.Ap, U.Aj, U.Ax)):
        assert np.array_equal(g, w)
    for h in (Md, Mh):
        h.close()
