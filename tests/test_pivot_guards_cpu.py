"""The oracle on the value sets of tests/pivot_inputs.py -- interior pivots that
cancel, a negative tiny first pivot, unit pivots, pivots exactly at and one ulp
inside the tolerance -- pinned against the reference itself
(oracle/_ref/libref.so; skipped where it is absent, e.g. on the GPU box).
tests/test_gpu_pivot_guards.py compares every numeric route of the library with
the oracle on the same sets; the per-block set (block_rows) has no counterpart in
the reference checker and is asserted by the oracle alone.
"""
import numpy as np
import pytest

import oracle as O
import pivot_inputs as P
from inputs import uniform

pytestmark = pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref/libref.so not built")


def _same_as_reference(Ap, Aj, Ax, level):
    A = O.CSR(Ap.size - 1, Ap, Aj, np.array(Ax))
    L, U = O.ilu(A, "iluk", level=level)
    Lr, Ur = O.ref_ilu(A, "iluk", level=level)
    for mine, ref in ((L, Lr), (U, Ur)):
        assert np.array_equal(mine.Ap, ref.Ap) and np.array_equal(mine.Aj, ref.Aj)
        assert np.isfinite(ref.Ax).all() and np.array_equal(mine.Ax, ref.Ax)
    for seed in (200, 0x1234):
        rhs = uniform(seed, A.n)
        want = O.ref_ilu_apply(A, rhs, "iluk", level=level)
        assert np.isfinite(want).all() and np.array_equal(O.ilu_apply(L, U, rhs), want)
    return U


@pytest.mark.parametrize("which", sorted(P.SETS))
@pytest.mark.parametrize("name,level", P.CASES, ids=[P.case_id(*c) for c in P.CASES])
def test_oracle_equals_reference(name, level, which):
    Ap, Aj = P.R._pattern(name)
    U = _same_as_reference(Ap, Aj, P.SETS[which](name, level), level)
    piv = P.pivots(U)
    if which == "cancel3":
        assert np.count_nonzero(piv == P.REPL) == 3
    elif which == "row0_neg":
        assert piv[0] == -1e-12
    elif which == "unit":
        assert np.all(piv == 1.0)
    else:
        assert np.all(piv > 1.0)  # benign: no pivot anywhere near the tolerance


def test_oracle_equals_reference_at_the_thresholds():
    U = _same_as_reference(*P.thresholds(), 0)
    assert np.array_equal(P.pivots(U)[:8], P.THRESHOLD_PIVOTS)


def test_block_rows_take_the_rule_per_block():
    """the construction's own assertions (the oracle alone: the reference checker has no blk)"""
    Ap, Aj, Ax = P.block_rows(945)
    assert Ap.size - 1 == 2457 and Ax[P._diag_pos(Ap, Aj)[945]] == -1e-12
