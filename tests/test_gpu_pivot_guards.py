"""The pivot guards of the ILUK numeric factorization and the unit-pivot state of
the sweeps, on every route that ends in k_ilu0_level (ilu_factor.hip) or in its
host restatement (GPU box only).  The value sets are those of
tests/pivot_inputs.py, each of which asserts through the oracle that its branch
is taken: interior pivots that cancel (stored as exactly +1e-3), a negative tiny
first pivot (stored as it is, reciprocal 1 / -1e-3), the same per block-Jacobi
block, pivots exactly at and one ulp inside the tolerance, and factors whose
pivots are all exactly 1.0.

Every comparison is bitwise (np.array_equal) against the CPU oracle and, where a
second handle exists, against that handle: factors, three applies, one enqueued
apply, both single sweeps and an apply in place.  Every case asserts the sweep
layout (and, on the packet sweeps, the record class) it is meant to exercise
first, so a route cannot be missed unnoticed.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
import pivot_inputs as P
from inputs import uniform

pytestmark = pytest.mark.gpu

R = P.R  # test_gpu_iluk_refactor: _pattern, _values, _check_state, _expected, _refresh, _refused
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUNSUPPORTED = R.EUNSUPPORTED
BOX, WG2D = (9, 21, 13), (30, 27, 1)


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


# ---- routes -----------------------------------------------------------------------------------
def _ep(strict_max):
    return 4 if strict_max <= 4 else 8 if strict_max <= 8 else 16 if strict_max <= 16 else 24


def _assert_route(M, route, e):
    """the sweeps M runs on are `route`'s: the layout, and what tells packets from the fallback"""
    import lssp_amd
    lay = M.sweep_layout()
    if route == "tiled0":
        assert lay == (1, 16, 8)
    elif route == "linef":
        assert lay == (2, 16, 8)
    elif route in ("wg2d0", "wg2d1"):  # the one-workgroup sweeps of a small 2-D grid: all ny lines in one tile
        assert lay == (1 + int(route[4:]), 27, 1)
    elif route == "syncfree":
        assert lay == (0, 0, 0)
        with pytest.raises(lssp_amd.LsspError) as err:
            M.schedule(0)
        assert err.value.status == EUNSUPPORTED
    else:
        want = int(route[2:])  # "ep4", "ep8", "ep16", "ep24"
        assert lay == (0, 0, 0)
        L, U = e["L"], e["U"]
        assert _ep(int(np.diff(L.Ap).max()) - 1) == want and _ep(int(np.diff(U.Ap).max()) - 1) == want
        assert M.schedule(0)["EP"] == want and M.schedule(1)["EP"] == want


def _make(dev, maker, Ap, Aj, Ax, level, blk=0):
    import lssp_amd
    if maker == "create":
        return lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=level, blk=blk)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    try:
        return getattr(lssp_amd.DILU, maker)(dev, D, kind=lssp_amd.ILUK, level=level)
    finally:
        D.close()  # the handle owns what it needs


def _check(dev, M, e, fresh=None, factors=True, sweeps=True):
    """_check_state plus the apply in place"""
    R._check_state(dev, M, e, fresh, factors=factors, sweeps=sweeps)
    n = e["A"].n
    y = dev.vec(n, uniform(200, n))
    M.apply(y, y)
    assert np.array_equal(y.download(), e["applies"][0])


_OWN = {}


def _expect(key, Ap, Aj, Ax, level, blk=0):
    """R._expected for a matrix that is no named pattern (or has blocks)"""
    if key not in _OWN:
        n = Ap.size - 1
        A = O.CSR(n, Ap, Aj, np.array(Ax))
        L, U = O.ilu(A, "iluk", level=level, blk=blk)
        one = R._identity(n)
        _OWN[key] = dict(A=A, L=L, U=U,
                         applies=[O.ilu_apply(L, U, uniform(200 + rep, n)) for rep in range(4)],
                         lower=O.ilu_apply(L, one, uniform(300, n)),
                         upper=O.ilu_apply(one, U, uniform(300, n)))
    return _OWN[key]


# ---- creates ------------------------------------------------------------------------------------
# (maker, route, pattern, level)
CREATES = [("create", "tiled0", BOX, 0),
           ("create", "linef", BOX, 1),
           ("create", "wg2d0", WG2D, 0),
           ("create", "wg2d1", WG2D, 1),
           ("create", "ep4", "grid5", 2),
           ("create", "ep8", "holed", 1),
           ("create", "ep16", "holed", 2),
           ("create", "ep24", "box786", 4),
           ("create", "syncfree", "rand6", 1),
           ("create_dev", "tiled0", BOX, 0),
           ("iluk_create_dev", "linef", BOX, 1),
           ("pc_create_dev", "ep8", "holed", 1),
           ("pc_create_dev", "ep8", "rand6", 0)]
SET_NAMES = ["benign", "cancel3", "row0_neg", "unit"]


def _cid(c):
    return f"{c[0]}-{c[1]}-{P.case_id(c[2], c[3])}"


@pytest.mark.parametrize("which", SET_NAMES)
@pytest.mark.parametrize("case", CREATES, ids=[_cid(c) for c in CREATES])
def test_create(dev, case, which):
    maker, route, name, level = case
    Ap, Aj = R._pattern(name)
    Ax = P.SETS[which](name, level)  # (asserts its branch through the oracle)
    e = P.expected(which, name, level)
    M = _make(dev, maker, Ap, Aj, Ax, level)
    _assert_route(M, route, e)
    # a device create is also compared with the host create of the same values
    other = _make(dev, "create", Ap, Aj, Ax, level) if maker != "create" else None
    _check(dev, M, e, other)
    for h in (other, M):
        if h is not None:
            h.close()


def test_create_block_rows(dev):
    """block-Jacobi, blocks of 945 rows = 5 planes: the first rows of the second and third block
    hold -1e-12 and +1e-12 (i % blk == 0 in the kernel)"""
    Ap, Aj, Ax = P.block_rows(945)
    e = _expect("block945", Ap, Aj, Ax, 0, blk=945)
    assert P.pivots(e["U"])[945] == -1e-12 and P.pivots(e["U"])[1890] == 1e-12
    M = _make(dev, "create", Ap, Aj, Ax, 0, blk=945)
    # the tiled line sweeps take a box whose plane couplings are cut at the block borders (a
    # missing neighbour is a +0.0 coefficient): the block rule's values go through their streams
    assert M.sweep_layout() == (1, 16, 8)
    _check(dev, M, e)
    M.close()


@pytest.mark.parametrize("maker", ["create", "pc_create_dev"])
def test_create_thresholds(dev, maker):
    Ap, Aj, Ax = P.thresholds()
    e = _expect("thresholds", Ap, Aj, Ax, 0)
    assert np.array_equal(P.pivots(e["U"])[:8], P.THRESHOLD_PIVOTS)
    M = _make(dev, maker, Ap, Aj, Ax, 0)
    assert M.sweep_layout() == (0, 0, 0)
    assert M.schedule(0)["EP"] == 4 and M.schedule(1)["EP"] == 4  # the packet sweeps, not the fallback
    _check(dev, M, e)
    x = dev.vec(300)
    M.apply(x, dev.vec(300, np.ones(300)))
    assert x.download()[0] == -1e12
    M.close()


# ---- the host numeric path (LSSP_AMD_ILU_HOST=1 is read once: a child process) -----------------
HOST_CASES = [c + (w,) for c in CREATES if c[0] == "create" for w in SET_NAMES] + ["block945", "thresholds"]


def _host_case(c):
    """(Ap, Aj, Ax, level, blk, route, expected) of a host case"""
    if c == "block945":
        Ap, Aj, Ax = P.block_rows(945)
        return Ap, Aj, Ax, 0, 945, None, _expect("block945", Ap, Aj, Ax, 0, blk=945)
    if c == "thresholds":
        Ap, Aj, Ax = P.thresholds()
        return Ap, Aj, Ax, 0, 0, None, _expect("thresholds", Ap, Aj, Ax, 0)
    _, route, name, level, which = c
    Ap, Aj = R._pattern(name)
    return Ap, Aj, P.SETS[which](name, level), level, 0, route, P.expected(which, name, level)


def _results(dev, M, n):
    """what a handle shows: factor values, one apply, both single sweeps"""
    (_, _, Lx), (_, _, Ux) = M.factors()
    x = dev.vec(n)
    out = [Lx, Ux]
    M.apply(x, dev.vec(n, uniform(200, n)))
    out.append(x.download())
    r = dev.vec(n, uniform(300, n))
    for w in (0, 1):
        M.trisolve(w, x, r)
        out.append(x.download())
    return out


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import lssp_amd
import test_gpu_pivot_guards as T
dev = lssp_amd.Device(0)
out = {}
for i, c in enumerate(T.HOST_CASES):
    Ap, Aj, Ax, level, blk, route, e = T._host_case(c)
    M = T._make(dev, "create", Ap, Aj, Ax, level, blk)
    if route is not None:
        T._assert_route(M, route, e)
    for q, a in enumerate(T._results(dev, M, Ap.size - 1)):
        out["%d_%d" % (i, q)] = a
    M.close()
np.savez(sys.argv[1], **out)
print("ok")
'''.replace("ROOT", ROOT)


def test_host_numeric_path(tmp_path):
    """every host create above with ilu0_factor (ilu_setup.cpp) in place of k_ilu0_level"""
    assert "LSSP_AMD_ILU_HOST" not in os.environ
    path = str(tmp_path / "host.npz")
    res = subprocess.run([sys.executable, "-c", CHILD, path], env=dict(os.environ, LSSP_AMD_ILU_HOST="1"),
                         capture_output=True, text=True, timeout=170)
    assert res.returncode == 0 and "ok" in res.stdout, (res.stdout[-2000:], res.stderr[-2000:])
    with np.load(path) as z:
        assert len(z.files) == 5 * len(HOST_CASES)
        for i, c in enumerate(HOST_CASES):
            e = _host_case(c)[-1]
            want = (e["L"].Ax, e["U"].Ax, e["applies"][0], e["lower"], e["upper"])
            for q, w in enumerate(want):
                assert np.array_equal(z["%d_%d" % (i, q)], w), (c, q)


# ---- refactors ----------------------------------------------------------------------------------
# (entry point, route, pattern, level)
REFACTORS = [("refactor", "tiled0", BOX, 0),
             ("iluk_refactor", "ep8", "holed", 1),
             ("iluk_refactor", "ep24", "box786", 4),
             ("iluk_refactor", "linef", BOX, 1)]


def _pair(dev, name, level, which):
    """a matrix handle and a host-created ILUK handle, both holding set `which`"""
    import lssp_amd
    Ap, Aj = R._pattern(name)
    Ax = P.SETS[which](name, level)
    return Ap, Aj, lssp_amd.DMat(dev, Ap, Aj, Ax), _make(dev, "create", Ap, Aj, Ax, level)


def _to(dev, D, M, how, name, level, which):
    """M factored again from set `which` through entry point `how`"""
    Ax = P.SETS[which](name, level)
    D.update_values(dev.vec(Ax.size, Ax))
    getattr(M, how)(D)


@pytest.mark.parametrize("read", [True, False], ids=["factors-read", "factors-unread"])
@pytest.mark.parametrize("case", REFACTORS, ids=[_cid(c) for c in REFACTORS])
def test_refactor_walk_leaves_nothing_stale(dev, case, read):
    """benign -> cancel3 -> benign -> row0_neg -> benign: a 1e-3 or a reciprocal of -1e-3 that
    stayed behind in a coefficient stream, a packet record or a sync-free array shows in the
    step after it; with factors() read between the steps or not (the lazy host refresh)"""
    how, route, name, level = case
    Ap, Aj, D, M = _pair(dev, name, level, "benign")
    _assert_route(M, route, P.expected("benign", name, level))
    _check(dev, M, P.expected("benign", name, level))
    for which in ("cancel3", "benign", "row0_neg", "benign"):
        _to(dev, D, M, how, name, level, which)
        fresh = _make(dev, "create", Ap, Aj, P.SETS[which](name, level), level)
        _check(dev, M, P.expected(which, name, level), fresh, factors=read)
        fresh.close()
    assert R._same_factors(M, *[P.expected("benign", name, level)[k] for k in ("L", "U")])
    M.close()
    D.close()


# ---- the unit state -------------------------------------------------------------------------------
def _same_schedules(M, fresh):
    """everything lssp_amd_ilu_get_schedule shows but who built it: the header (unit included),
    and blk, desc, rec, idx, perm, pos"""
    for w in (0, 1):
        a, b = M.schedule(w), fresh.schedule(w)
        assert a.keys() == b.keys()
        for key in a:
            if key != "origin":
                assert np.array_equal(a[key], b[key]), (w, key)


def _solve20(dev, D, M, e):
    """BiCGSTAB capped at 20 iterations, bitwise the oracle's (tolerances of 1e-15: it runs 4 or 5
    iterations on these diagonally dominant values, more than the 2 or 3 that 1e-7 would take)"""
    import lssp_amd
    n = e["A"].n
    bh = uniform(77, n)
    assert dev.reduction == lssp_amd.TREE
    x, b = dev.vec(n, np.zeros(n)), dev.vec(n, bh)
    r = lssp_amd.solve(dev, D, M, x, b, solver=lssp_amd.BICGSTAB, tol_rel=1e-15, tol_abs=1e-15, tol_rb=1e-15,
                       maxit=20, restart=30, trace_cap=1000)
    o = O.solve(O.BICGSTAB, e["A"], bh, L=e["L"], U=e["U"], rtol=1e-15, atol=1e-15, rbtol=1e-15, maxit=20,
                restart=30, mode=O.TREE)
    assert 4 <= o.nits <= 20 and r.nits == o.nits and r.residual == o.residual
    assert np.array_equal(r.trace, o.trace) and np.array_equal(x.download(), o.x)


UNIT = [c for c in REFACTORS if c[2] != "box786"]  # tiled ILU(0), packets (holed, level 1), skewed ILU(1)


@pytest.mark.parametrize("case", UNIT, ids=[_cid(c) for c in UNIT])
def test_unit_created_handle_takes_general_values(dev, case):
    """(a) created while every pivot was 1.0, refactored to general pivots before any single sweep:
    bitwise a fresh create, its schedules (header word unit included) too"""
    how, route, name, level = case
    Ap, Aj, D, M = _pair(dev, name, level, "unit")
    eu, eb = P.expected("unit", name, level), P.expected("benign", name, level)
    _assert_route(M, route, eu)
    if route == "ep8":
        assert M.schedule(0)["unit"] == 1 and M.schedule(1)["unit"] == 1
    _check(dev, M, eu, sweeps=False)
    _to(dev, D, M, how, name, level, "benign")
    fresh = _make(dev, "create", Ap, Aj, P.SETS["benign"](name, level), level)
    if route == "ep8":
        assert fresh.schedule(0)["unit"] == 1 and fresh.schedule(1)["unit"] == 0
        _same_schedules(M, fresh)
    _check(dev, M, eb, fresh)
    _solve20(dev, D, M, eb)
    for h in (fresh, M, D):
        h.close()


@pytest.mark.parametrize("case", UNIT, ids=[_cid(c) for c in UNIT])
def test_general_handle_takes_unit_values(dev, case):
    """(b) the reverse; then (c) a single U sweep builds its arrays while every pivot is 1.0: the
    apply stays right, and on the packet sweeps the next iluk_refactor is refused (the header's
    rule) with the handle unchanged.  The line sweeps build no such arrays and go on refactoring."""
    how, route, name, level = case
    Ap, Aj, D, M = _pair(dev, name, level, "benign")
    eu, eb = P.expected("unit", name, level), P.expected("benign", name, level)
    _assert_route(M, route, eb)
    _to(dev, D, M, how, name, level, "unit")
    fresh = _make(dev, "create", Ap, Aj, P.SETS["unit"](name, level), level)
    if route == "ep8":
        _same_schedules(M, fresh)
        assert M.schedule(1)["unit"] == 1
    _check(dev, M, eu, fresh, sweeps=False)
    _check(dev, M, eu, fresh)  # with trisolve(1): the U sweep's unit state is set now
    _check(dev, M, eu, fresh)
    Ab = P.SETS["benign"](name, level)
    D.update_values(dev.vec(Ab.size, Ab))
    if route == "ep8":
        R._refused(dev, M, D, EUNSUPPORTED, eu)
        _check(dev, M, eu, fresh)
    else:
        getattr(M, how)(D)
        _check(dev, M, eb)
    for h in (fresh, M, D):
        h.close()


@pytest.mark.parametrize("case", UNIT, ids=[_cid(c) for c in UNIT])
def test_unit_created_handle_after_a_single_sweep(dev, case):
    """(d) created from unit pivots, one single U sweep, then iluk_refactor: refused on the
    packet sweeps, handle unchanged and usable; served on the line sweeps"""
    how, route, name, level = case
    Ap, Aj, D, M = _pair(dev, name, level, "unit")
    eu, eb = P.expected("unit", name, level), P.expected("benign", name, level)
    _assert_route(M, route, eu)
    n = Ap.size - 1
    z = dev.vec(n)
    M.trisolve(1, z, dev.vec(n, uniform(300, n)))
    assert np.array_equal(z.download(), eu["upper"])
    Ab = P.SETS["benign"](name, level)
    D.update_values(dev.vec(Ab.size, Ab))
    if route == "ep8":
        R._refused(dev, M, D, EUNSUPPORTED, eu)
        _check(dev, M, eu)
    else:
        getattr(M, how)(D)
        _check(dev, M, eb)
    M.close()
    D.close()


# ---- non-finite and subnormal right-hand sides -----------------------------------------------------
FAMILIES = [("tiled0", BOX, 0), ("linef", BOX, 1), ("wg2d0", WG2D, 0), ("ep8", "holed", 1), ("ep24", "box786", 4),
            ("syncfree", "rand6", 1)]


def _odd_rhs(n, nonfinite):
    """uniform(200, n) with about 1 % of its entries -0.0 or the smallest subnormal and, with
    nonfinite, NaN, +Inf or -Inf too.  The non-finite ones lie in the middle third of the rows:
    a triangular sweep carries them to every row that follows, so the L sweep keeps finite
    values in the first third and the U sweep in the last, while the apply is NaN throughout."""
    r = uniform(200, n)
    rng = np.random.default_rng(n)
    at = rng.choice(n, max(n // 100, 6), replace=False)
    r[at] = np.resize(np.array([-0.0, 5e-324]), at.size)
    if nonfinite:
        mid = n // 3 + rng.choice(n // 3, max(n // 200, 3), replace=False)
        r[mid] = np.resize(np.array([np.nan, np.inf, -np.inf]), mid.size)
    assert not np.any(r.view(np.uint64) == np.uint64(0xFFF7DEADBEEFCAFE))  # the sweeps' hand-off pattern is no input
    return r


def _same_nonfinite(got, want):
    """NaNs by position (x86 and the GPU differ in the sign of a generated NaN), the rest by bits"""
    ok = ~np.isnan(want)
    return bool(np.array_equal(got, want, equal_nan=True)
                and np.array_equal(got.view(np.uint64)[ok], want.view(np.uint64)[ok]))


@pytest.mark.parametrize("case", FAMILIES, ids=[f"{c[0]}-{P.case_id(c[1], c[2])}" for c in FAMILIES])
def test_nonfinite_and_subnormal_rhs(dev, case):
    route, name, level = case
    Ap, Aj = R._pattern(name)
    e = P.expected("benign", name, level)
    M = _make(dev, "create", Ap, Aj, P.SETS["benign"](name, level), level)
    _assert_route(M, route, e)
    n = Ap.size - 1
    one = R._identity(n)
    x = dev.vec(n)
    for nonfinite in (False, True):
        rhs = _odd_rhs(n, nonfinite)
        want = (O.ilu_apply(e["L"], e["U"], rhs), O.ilu_apply(e["L"], one, rhs), O.ilu_apply(one, e["U"], rhs))
        if nonfinite:
            assert np.isnan(want[0]).any()
            assert all(np.isnan(w).any() and np.isfinite(w).sum() >= n // 4 for w in want[1:])
        else:
            assert all(np.isfinite(w).all() for w in want)
        r = dev.vec(n, rhs)
        M.apply(x, r)
        assert _same_nonfinite(x.download(), want[0]), nonfinite
        for w in (0, 1):
            M.trisolve(w, x, r)
            assert _same_nonfinite(x.download(), want[1 + w]), (nonfinite, w)
    # the handle is none the worse for it
    M.apply(x, dev.vec(n, uniform(200, n)))
    assert np.array_equal(x.download(), e["applies"][0])
    M.close()
