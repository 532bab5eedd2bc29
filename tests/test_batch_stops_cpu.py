"""The stop plan of tests/test_gpu_batch_stops.py, checked against the oracle alone.

The plan (tests/stop_util.py) must put a stop on every position of a batch
that the batched BiCGSTAB and CG drivers treat differently; these tests assert
those positions as conditions on the plan, that the oracle really leaves where
each stop says, and that the batch sizes the positions were laid out for are
still the ones solvers.cpp compiles.
"""
import numpy as np
import pytest

import oracle as O
import stop_util as SU


def test_batch_sizes_are_the_ones_the_positions_were_laid_out_for():
    """a retune of BATCH / CG_BATCH moves the boundaries: move the m lists of stop_util.py with it"""
    assert SU.batch_sizes() == (SU.BATCH, SU.CG_BATCH) == (8, 32)
    B, C = SU.BATCH, SU.CG_BATCH
    # last / first iteration of the first and second batch, the short third batch
    assert {B, B + 1, 2 * B, 2 * B + 1, 2 * B + 2} <= set(SU.BICG_MAXIT_M)
    assert {B, B + 1, 2 * B, 2 * B + 1} <= set(SU.BICG_TOL_M)
    assert {B - 1, B, B + 1, 2 * B, 2 * B + 1} == set(SU.BICG_SERIAL_M)
    assert {1, 2, C - 1, C, C + 1, C + 2, 2 * C - 1, 2 * C, 2 * C + 1, 2 * C + 2} == set(SU.CG_EDGE_M)
    assert {B - 1, B, B + 1, B + 2, 2 * B, 2 * B + 1} == set(SU.DIST_BICG_TOL_M)
    assert {B, B + 1} == set(SU.DIST_BICG_MAXIT_M)
    assert {C - 1, C, C + 1, C + 2} == set(SU.DIST_CG_TOL_M)


def _check_stops(solver, A, L, U, mode, stops, nranks=1):
    """the oracle leaves where each stop says, by the exit its kind names"""
    for st in stops:
        o = SU.expect(solver, A, L, U, mode, st, nranks)
        assert o.nits == st.m, (st, o.nits)
        if st.kind == "maxit":
            assert st.maxit == st.m and st.atol == st.rtol == 0.0 and st.bexp == 0
        elif st.kind == "tol":
            assert st.m < st.maxit and st.bexp == 0 and (st.atol > 0.0) != (st.rtol > 0.0)
            prev = SU.expect(solver, A, L, U, mode, SU.Stop("maxit", st.m, st.m), nranks)
            assert o.residual == prev.residual and np.array_equal(o.x, prev.x)  # the same m iterations
        else:
            assert st.kind == "brk" and st.atol == st.rtol == 0.0 and SU.is_breakdown(o, st.maxit)


@pytest.mark.parametrize("route", sorted(SU.BICG_ROUTES))
def test_bicgstab_tree_plan_reaches_every_position(route):
    A, L, U = SU.route_inputs(route)
    plan = SU.bicg_plan(route, O.TREE)
    assert [s.m for s in plan["maxit"]] == list(range(1, 19))
    assert [s.m for s in plan["tol"]] == list(range(1, 18))
    assert all(s.atol > 0.0 for s in plan["tol"])  # BiCGSTAB's residuals fall below h[0] at once
    brk = {s.m for s in plan["brk"]}
    assert {8, 9} <= brk and brk & {16, 17}
    for kind in ("maxit", "tol", "brk"):
        assert all(s.kind == kind for s in plan[kind])
        _check_stops(O.BICGSTAB, A, L, U, O.TREE, plan[kind])


@pytest.mark.parametrize("route", SU.BICG_SERIAL_ROUTES)
def test_bicgstab_serial_plan(route):
    A, L, U = SU.route_inputs(route)
    plan = SU.bicg_plan(route, O.SERIAL)
    assert [s.m for s in plan["maxit"]] == [7, 8, 9, 16, 17]
    assert [s.m for s in plan["tol"]] == [7, 8, 9, 16, 17]
    _check_stops(O.BICGSTAB, A, L, U, O.SERIAL, plan["maxit"] + plan["tol"])


def test_history_is_the_residual_of_the_run_stopped_at_maxit():
    """h[m], read from one run's trace, is O.solve(maxit=m)'s residual"""
    for solver, A, L, U, upto in ((O.BICGSTAB, *SU.route_inputs("line2"), 17), (O.CG, SU.matrix(3, 16), None, None, 66)):
        for mode in (O.TREE, O.SERIAL):
            h, _ = SU.history(solver, A, L, U, mode, upto)
            assert h[0] == np.sqrt(O.dot(np.ones(A.n), np.ones(A.n), mode))
            for m in (1, 2, 7, 8, 9, upto):
                o = O.solve(solver, A, np.ones(A.n), L=L, U=U, rtol=0.0, atol=0.0, rbtol=0.0, maxit=m, mode=mode)
                assert o.nits == m and o.residual == h[m]


@pytest.mark.parametrize("mode", [O.TREE, O.SERIAL], ids=["tree", "serial"])
def test_cg_plan_reaches_every_position(mode):
    reach = set()
    for mat in SU.CG_MATS:
        A = SU.matrix(*SU.CG_MATS[mat])
        plan = SU.cg_plan(mat, mode)
        assert [s.m for s in plan["maxit"]] == [1, 2, 31, 32, 33, 34, 63, 64, 65, 66]
        _check_stops(O.CG, A, None, None, mode, plan["maxit"] + plan["tol"])
        reach |= {s.m for s in plan["tol"]}
    assert set(SU.CG_EDGE_M) <= reach
    assert reach == set(range(1, 67))  # every position of the first two batches, on one matrix or the other


def test_cg_record_lows_are_the_ones_the_shapes_were_chosen_for():
    """the iterations no tolerance can stop at (no new low of the residual after the first iteration)"""
    def miss(mat, mode):
        return [m for m in range(1, 67) if m not in {s.m for s in SU.cg_plan(mat, mode)["tol"]}]
    assert miss("p3_16", O.TREE) == [62, 63, 64, 65]
    assert miss("p3_16", O.SERIAL) == [55, 56, 57, 58, 66]
    assert miss("p2_48", O.TREE) == miss("p2_48", O.SERIAL) == [3, 4, 6, 35, 36, 37, 40]


def test_two_rank_plan():
    A, L, U = SU.dist_inputs(O.BICGSTAB)
    stops = SU.dist_plan(O.BICGSTAB)
    assert [s.id for s in stops] == ["tol7", "tol8", "tol9", "tol10", "tol16", "tol17", "maxit8", "maxit9"]
    _check_stops(O.BICGSTAB, A, L, U, O.TREE, stops, nranks=SU.DIST_RANKS)
    A, L, U = SU.dist_inputs(O.CG)
    stops = SU.dist_plan(O.CG)
    assert [s.id for s in stops] == ["tol31", "tol32", "tol33", "tol34"]
    _check_stops(O.CG, A, L, U, O.TREE, stops, nranks=SU.DIST_RANKS)


def test_rho_exit_inputs_leave_after_a_batchs_last_and_first_iteration():
    assert sorted(SU.RHO_CASES) == [SU.BATCH + 1, SU.BATCH + 2]
    for m in SU.RHO_CASES:
        o = SU.rho_expect(m)
        assert o.nits == m and SU.is_rho_exit(o, SU.RHO_MAXIT)
        assert o.residual > 1e-3  # r != 0: neither converged nor the ||s|| exit
