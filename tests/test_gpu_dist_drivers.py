"""All 19 Krylov drivers on P ranks, against the oracle's P-rank mode and the reference's runs.

lssp_amd_solve takes a distributed matrix for every driver; tests/test_gpu_dist.py and
tests/test_gpu_dist_dev.py run five of them on more than one rank, on Poisson boxes with b = 1
and x0 = 0.  Here every driver runs with nx != n (work vectors and Arnoldi bases strided by
nrows + nhalo), through the rank combine of its reductions (TREE: rank sums added in rank
order; SERIAL: the ranks continue each other's running sums), with the block-Jacobi and the
global preconditioner, on nonsymmetric rows with arbitrary halo owners (generated unsorted:
the rank's ILU sorts its block, the rank sorts its rows for the upload), and with a rank that
owns no row.  The legs and their case tables are in tests/dist_drivers_util.py;
tests/test_dist_drivers_cpu.py pins their inputs without a GPU.

One spawn per leg (ranks on ONE device over the host-staged transport, at most 4 alive); the
cases below only assert on the leg's cached results.  All comparisons are bitwise, NaN as NaN:
  TREE    count, residual, every traced dot / norm and x == the oracle's P-rank mode
  SERIAL  the same against the oracle, and where the case repeats a run of the reference
          (legs A and E) against that run itself (tests/golden/)
and every rank -- the empty one included -- returns the same count, residual and trace."""
import pytest

import dist_drivers_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def legs():
    """leg name -> its run (spawned on first use, then cached for the module)"""
    cache = {}

    def get(leg):
        if leg not in cache:
            cache[leg] = U.spawn_leg(leg)
            r = cache[leg]
            done = 0 if r["results"] is None else len(r["results"])
            print(f"\nleg {leg}: {U.WORLD[leg]} ranks, {done} of {len(U.LEGS[leg])} cases in {r['wall']:.1f} s "
                  f"(exit codes {r['exitcodes']})")
        return cache[leg]

    return get


@pytest.mark.parametrize("leg", list(U.LEGS))
def test_leg_ran_to_its_end(legs, leg):
    """the ranks answered within the queue wait, left by themselves with status 0, and no case was left out"""
    run = legs(leg)
    U.leg_ok(run)
    assert set(run["results"]) == {c["key"] for c in U.LEGS[leg]}


@pytest.mark.parametrize("c", U.ALL_CASES, ids=[c["key"] for c in U.ALL_CASES])
def test_driver_on_p_ranks(legs, c):
    U.check_result(c, U.case_record(legs(c["leg"]), c))
