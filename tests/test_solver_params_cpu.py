"""The oracle against the reference's runs with k != 3 and with a single term of
the stop scale deciding (tests/golden/solver_params_manifest.json), its RLGMRES
against the reference's RLGMRES runs, and -- on the oracle alone -- the
conditions without which the GPU comparisons of tests/test_gpu_solver_params.py
would pass vacuously.  Every assertion is equality of bits or of an integer,
or one of the stated inequalities between integers / against 1e-8 ||r0||.
"""
import json
import os

import numpy as np
import pytest

import oracle as O
import golden_util as G
import solver_params_util as SP

CASES = SP.cases()
MODES = {"serial": O.SERIAL, "tree": O.TREE}
with open(os.path.join(SP.HERE, "rlgmres_manifest.json")) as _f:
    RLGMRES_CASES = json.load(_f)["cases"]


def test_the_fixtures_are_the_cases_of_the_plan():
    keys = ("group", "solver", "pc", "mat", "b", "x0", "maxit", "restart", "rtol", "atol", "rbtol", "aug_k")
    assert [{k: c[k] for k in keys} for c in CASES] == [{k: c[k] for k in keys} for c in SP.case_specs()]
    assert len(SP.cases("mk")) == 24 and len(SP.cases("stop")) == 4 * 19 and len(SP.cases("exact")) == 5


def test_recorded_box_is_the_recipe():
    a, b = SP.build_matrix(SP.BOX, recorded=True), SP.build_matrix(SP.BOX, recorded=False)
    assert a.n == b.n == 630
    assert np.array_equal(a.Ap, b.Ap) and np.array_equal(a.Aj, b.Aj) and np.array_equal(a.Ax, b.Ax)


@pytest.mark.parametrize("c", CASES, ids=[SP.case_id(c) for c in CASES])
def test_oracle_serial_mode_reproduces_the_reference(c):
    r = SP.oracle_run(c, O.SERIAL)
    assert r.nits == c["nits"]
    assert r.residual == SP.fx(c["residual"])
    assert SP.matches(c["trace"], r.trace)  # every dot / norm, bit for bit
    assert np.array_equal(SP.stored(c["trace"])[0], r.trace, equal_nan=True)
    assert SP.matches(c["x"], r.x)


def _old_factors(c, A):
    pc = c["pc"]
    if pc["kind"] == "none":
        return None, None
    if pc["kind"] == "iluk":
        return O.ilu(A, "iluk", level=pc["level"])
    if pc["kind"] == "ilut":
        return O.ilu(A, "ilut", tol=pc["tol"], p=pc["p"])
    return O.ilu(A, "iluk", level=0, blk=(A.n + pc["nblk"] - 1) // pc["nblk"])


@pytest.mark.parametrize("c", RLGMRES_CASES, ids=[G.case_id(c) for c in RLGMRES_CASES])
def test_oracle_rlgmres_reproduces_the_reference(c):
    assert c["solver"] == O.RLGMRES
    A = G.build_matrix(c["mat"])
    L, U = _old_factors(c, A)
    x0 = None if c["x0"] is None else G.vec(c["x0"], A.n)
    r = O.solve(O.RLGMRES, A, G.vec(c["b"], A.n), x0=x0, L=L, U=U, rtol=G.fx(c["rtol"]), atol=G.fx(c["atol"]),
                rbtol=G.fx(c["rbtol"]), maxit=c["maxit"], restart=c["restart"], mode=O.SERIAL)
    assert r.nits == c["nits"]
    assert r.residual == G.fx(c["residual"])
    assert G.matches(c["trace"], r.trace)
    assert G.matches(c["x"], r.x)


@pytest.mark.parametrize("k", [0, -1])
@pytest.mark.parametrize("solver", SP.MK_SOLVERS)
def test_oracle_k_not_positive_means_three(solver, k):
    c = SP.zero_case(solver, SP.MK_PCS[0], 2, 3)
    a, b = SP.oracle_run(c, O.TREE), SP.oracle_run(c, O.TREE, aug_k=k)
    assert a.nits == b.nits and a.residual == b.residual
    assert np.array_equal(a.trace, b.trace) and np.array_equal(a.x, b.x)
    other = SP.oracle_run(c, O.TREE, aug_k=2)  # and k is not ignored
    assert not np.array_equal(a.x, other.x)


# ---- the stop rule: each term of max(rtol ||r0||, atol, rbtol ||b||) decides a stop of its own ----

def test_stop_inputs_separate_the_three_terms():
    c = SP.cases("stop")[0]
    t = SP.stored(c["trace"])[0]  # opens with ||b||, ||r0||
    assert 13.0 < t[0] < 13.6 and 89.0 < t[1] < 91.0
    scale = [SP.LADDER["rtol"][0] * t[1], SP.LADDER["atol"][1], SP.LADDER["rbtol"][2] * t[0]]
    assert len(set(scale)) == 3 and max(scale) == scale[1]


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("solver", sorted(SP.SOLVERS, key=SP.SOLVERS.get))
def test_single_tolerance_runs_stop_at_different_iterations(solver, mode):
    """a driver that drops a term, forgets ||b|| or takes the wrong maximum moves at least one of these"""
    runs = {c["rung"]: c for c in SP.cases("stop") if c["solver"] == SP.SOLVERS[solver]}
    assert sorted(runs) == sorted(SP.LADDER)
    nits = {rung: SP.oracle_run(c, MODES[mode]).nits for rung, c in runs.items()}
    single = [nits["rtol"], nits["atol"], nits["rbtol"]]
    print(solver, mode, single, nits["all"])
    assert len(set(single)) == 3
    assert all(1 < v < SP.STOP_MAXIT for v in single)
    assert nits["all"] == min(single)
    if mode == "serial":  # the reference's own counts
        assert [runs[r]["nits"] for r in ("rtol", "atol", "rbtol", "all")] == single + [nits["all"]]


# ---- the zero-tolerance (m, k) runs --------------------------------------------------------------

ZERO = SP.zero_cases()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("c", ZERO, ids=[SP.case_id(c) for c in ZERO])
def test_zero_tolerance_runs_wrap_the_ring_above_roundoff(c, mode):
    m, k = c["restart"], c["aug_k"]
    o = SP.oracle_run(c, MODES[mode])
    A = SP.build_matrix(c["mat"])
    assert A.n <= 630
    ws = SP.widths(m, k, 2 * k + 1)
    assert len(ws) >= 2 * k + 1 and max(ws) > m and sum(ws) == c["maxit"]
    # stopped by maxit, and the dots and norms evaluated are those of 2k + 1 full-width cycles: no
    # cycle was cut short by a breakdown or a gstol exit, so z[outer % k] was written 2k + 1 times
    assert o.nits == c["maxit"]
    assert o.trace.size == SP.full_cycles_trace_len(ws)
    r = SP.vec(c["b"], A) - O.spmv(0, A, o.x)
    true_res = float(np.sqrt(np.dot(r, r)))
    print(SP.case_id(c), mode, "true residual / ||r0|| =", true_res / o.trace[1])
    assert true_res > 1e-8 * o.trace[1]


@pytest.mark.parametrize("solver", SP.MK_SOLVERS)
def test_k1_m1_run_is_not_trivial(solver):
    c = SP.zero_case(solver, SP.MK_PCS[0], 1, 1)
    o = SP.oracle_run(c, O.TREE)
    assert c["maxit"] == 5 and o.nits == 5 and o.trace.size == SP.full_cycles_trace_len([1, 2, 2])
    assert np.all(np.isfinite(o.x)) and np.any(o.x != 0)


# ---- x0 exact ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("solver", sorted(SP.SOLVERS, key=SP.SOLVERS.get))
def test_exact_x0_leaves_x_alone(solver, mode):
    c = SP.exact_case(solver)
    A = SP.build_matrix(c["mat"])
    assert np.array_equal(SP.vec("A1", A) - O.spmv(0, A, np.ones(A.n)), np.zeros(A.n))
    o = SP.oracle_run(c, MODES[mode])
    assert o.nits == (1 if solver in SP.EXACT_ITERATING else 0)
    assert o.residual == 0.0
    assert np.array_equal(o.x, np.ones(A.n))
