"""The inputs of tests/test_gpu_dist_drivers.py, checked with the oracle alone (no GPU).

The GPU legs compare the library's P-rank runs with the oracle's P-rank mode and, in SERIAL
mode, with the reference's own block-Jacobi runs (tests/golden/).  That means something only
while (1) the oracle's SERIAL mode with nranks = nblk IS the reference's block-Jacobi run,
(2) the runs of the general legs are finite and (3) they end by their stop rule, not by maxit.
This file keeps those three under test for the case tables as they stand, together with the
tables' shape and the runner's timeout path (a stub worker that sleeps)."""
import os

import numpy as np
import pytest

import oracle as O
import dist_drivers_util as U
from dist_dev_util import rank_rows
from golden_util import case_id, fx, matches


@pytest.mark.parametrize("g", U.BJ_GOLDEN, ids=[case_id(g) for g in U.BJ_GOLDEN])
def test_oracle_serial_prank_mode_is_the_reference_block_jacobi_run(g):
    """nranks = nblk: the oracle's blocks of ceil(n / nblk) rows are the reference's, and the ranks'
    running sums its one sequential sum -- count, residual, every dot and x bit for bit.  In TREE
    mode the same run stops within max(1, 5 %) iterations of it (the bound the GPU leg asserts)."""
    n = U.matrix(g["mat"]).n
    nblk = g["pc"]["nblk"]
    kw = dict(b=g["b"], x0=g["x0"], tol=(fx(g["rtol"]), fx(g["atol"]), fx(g["rbtol"])), maxit=g["maxit"],
              restart=g["restart"])
    o = U.oracle_run(g["mat"], g["solver"], O.SERIAL, nblk, (n + nblk - 1) // nblk, **kw)
    assert o.nits == g["nits"]
    assert o.residual == fx(g["residual"])
    assert matches(g["trace"], o.trace)
    assert matches(g["x"], o.x)
    t = U.oracle_run(g["mat"], g["solver"], O.TREE, nblk, (n + nblk - 1) // nblk, **kw)
    assert abs(t.nits - g["nits"]) <= U.nits_bound(g["nits"])


GENERAL = U.LEGS["B"] + U.LEGS["C"] + U.LEGS["D"]
# RLGMRES without a preconditioner on the 10^3 box: the one run that ends by maxit (lowered to 200 for it)
BY_MAXIT = {f"C-p10-rlgmres-none-{m}" for _, m in U.MODES}


@pytest.mark.parametrize("c", GENERAL, ids=[c["key"] for c in GENERAL])
def test_general_legs_are_finite_and_end_by_their_stop_rule(c):
    o = U.expected(c)
    assert np.isfinite(o.residual) and np.all(np.isfinite(o.trace)) and np.all(np.isfinite(o.x))
    assert len(o.trace) < U.TRACE_CAP
    if c["leg"] == "D":  # zero tolerances: no early stop (each driver counts its last step its own way)
        assert c["maxit"] <= o.nits <= c["maxit"] + 2
    elif c["key"] in BY_MAXIT:
        assert o.nits == c["maxit"] == 200
    else:
        assert 0 < o.nits < c["maxit"]
        if c["solver"] in U.ARNOLDI:  # at least two restarts: the augmented Z basis is read
            assert o.nits > 2 * c["restart"]


@pytest.mark.parametrize("c", U.LEGS["E"], ids=[c["key"] for c in U.LEGS["E"]])
def test_global_factor_cases_repeat_the_reference(c):
    """leg E in SERIAL mode is the single-process reference order: the oracle gives the golden run"""
    if c["mode"] != O.SERIAL:
        o = U.expected(c)
        assert np.isfinite(o.residual)
        return
    o = U.expected(c)
    U.check_against_golden(c, o.nits, o.residual, o.trace, o.x)


def test_case_tables():
    keys = [c["key"] for c in U.ALL_CASES]
    assert len(set(keys)) == len(keys)
    count = {leg: len(cs) for leg, cs in U.LEGS.items()}
    # A: 19 drivers x 2 modes.  B: 18 drivers x {bj, none} x 2 modes.  C: (18 + 19) x 2 x 2.  D: 19 x 2.
    # E: (19 b = 1 runs + the b = 0 runs the reference has + 1 nblk = 2 run) x 2 modes.
    zeros = sum(1 for c in U.LEGS["E"] if c["b"] == "zeros" and c["mode"] == O.TREE)
    assert count == {"A": 38, "B": 72, "C": 148, "D": 38, "E": 2 * (19 + zeros + 1)}, count
    assert zeros >= 18
    for leg in "ABDE":
        assert {c["solver"] for c in U.LEGS[leg]} == set(U.DRIVERS) - ({O.CG} if leg == "B" else set())
    assert {c["solver"] for c in U.LEGS["C"] if c["group"] == "p10"} == set(U.DRIVERS)
    assert all(c["pc"] == "none" for c in U.LEGS["D"]) and all(c["golden"] for c in U.LEGS["A"] + U.LEGS["E"])
    assert max(U.WORLD.values()) <= 4  # rank processes alive at a time
    # the row splits the legs are named for
    assert [rank_rows(777, 2, r)[1] for r in range(2)] == [389, 388]
    assert [rank_rows(1000, 3, r)[1] for r in range(3)] == [334, 334, 332]
    assert [rank_rows(9, 4, r)[1] for r in range(4)] == [3, 3, 3, 0]
    # halo owners are arbitrary: far more distinct col - row than a stencil has, rows unsorted
    A = U.matrix(U.RAND777)
    rows = np.repeat(np.arange(A.n), np.diff(A.Ap))
    assert np.unique(A.Aj - rows).size == 1292
    assert any(np.any(np.diff(A.Aj[A.Ap[i]:A.Ap[i + 1]]) < 0) for i in range(A.n))


def _alive(pid):
    try:
        os.kill(pid, 0)
        return True
    except ProcessLookupError:
        return False


def test_runner_leaves_no_rank_alive_after_a_timeout():
    """ranks that never answer: the wait ends at its limit, every rank is terminated and reaped,
    and the outcome fails leg_ok / case_record instead of passing for a result"""
    run = U.spawn_leg("D", world=2, target=U._sleeping_worker, timeout=1.0, join_timeout=0.2)
    assert run["results"] is None and run["timed_out"]
    assert run["ended"] == [0, 1]
    assert all(e is not None and e != 0 for e in run["exitcodes"])
    assert not any(_alive(pid) for pid in run["pids"])
    with pytest.raises(AssertionError, match="no answer from the ranks"):
        U.case_record(run, U.LEGS["D"][0])


def test_unreached_case_fails_with_the_first_failing_case():
    first, second = U.LEGS["D"][0], U.LEGS["D"][1]
    run = {"results": {first["key"]: {"status": 3, "error": ["boom"] * 4}}, "wall": 0.0, "timed_out": False,
           "exitcodes": [0] * 4, "ended": [], "pids": []}
    with pytest.raises(AssertionError, match=first["key"]):
        U.case_record(run, second)
    with pytest.raises(AssertionError):
        U.check_result(first, U.case_record(run, first))
