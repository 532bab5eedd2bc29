"""LGMRES / RLGMRES's k, every driver's stop rule, exact starts and the restart
limits on the GPU, bit for bit.

SERIAL reduction mode against the reference's own runs (tests/golden/
solver_params_manifest.json), TREE mode against the oracle restating the same
canonical reduction order -- nits, residual, every dot / norm of the trace and
x.  tests/test_solver_params_cpu.py pins the oracle to those runs and asserts,
on the oracle alone, what makes these comparisons mean something: the three
single-tolerance runs of a driver stop at three different iterations, and the
zero-tolerance runs take 2k + 1 full-width cycles and end above roundoff.
All systems have at most 630 rows.
"""
import os
import re

import numpy as np
import pytest

import oracle as O
import solver_params_util as SP
from inputs import uniform

pytestmark = pytest.mark.gpu

CASES = SP.cases()
ZERO = SP.zero_cases()
K1M1 = [SP.zero_case(s, pc, 1, 1) for s in SP.MK_SOLVERS for pc in SP.MK_PCS]
ALL = sorted(SP.SOLVERS, key=SP.SOLVERS.get)


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def systems(dev):
    """(A, device matrix, device ILU(0) or None) per matrix and preconditioner, made once; the
    device factors are the oracle's, bit for bit"""
    import lssp_amd
    made = {}

    def get(c):
        key = (repr(sorted(c["mat"].items())), c["pc"]["kind"])
        if key not in made:
            A = SP.build_matrix(c["mat"])
            Ap, Aj, Ax = lssp_amd.sort_columns(A.Ap, A.Aj, A.Ax)  # lssp.cxx:173
            D = lssp_amd.DMat(dev, Ap, Aj, Ax)
            M = None
            if c["pc"]["kind"] != "none":
                M = lssp_amd.DILU.create(dev, A.Ap, A.Aj, A.Ax, kind=1, level=c["pc"]["level"])
                (Lp, Lj, Lx), (Up, Uj, Ux) = M.factors()
                L, U = SP.factors(c)
                assert np.array_equal(Lj, L.Aj) and np.array_equal(Lx, L.Ax)
                assert np.array_equal(Uj, U.Aj) and np.array_equal(Ux, U.Ax)
            made[key] = (A, D, M)
        return made[key]

    yield get
    for _, D, M in made.values():
        if M is not None:
            M.close()
        D.close()


def _gpu(dev, systems, c, mode, **over):
    import lssp_amd
    c = dict(c, **over)
    A, D, M = systems(c)
    b = dev.vec(A.n, SP.vec(c["b"], A))
    x = dev.vec(A.n, SP.vec(c["x0"], A))
    dev.set_reduction(mode)
    try:
        r = lssp_amd.solve(dev, D, M, x, b, solver=c["solver"], tol_rel=SP.fx(c["rtol"]), tol_abs=SP.fx(c["atol"]),
                           tol_rb=SP.fx(c["rbtol"]), maxit=c["maxit"], restart=c["restart"], bgsl=c["restart"],
                           idrs=c["restart"], aug_k=c["aug_k"], trace_cap=100000)
    finally:
        dev.set_reduction(lssp_amd.TREE)
    return r, x.download()


def _same_run(r, xh, o):
    assert r.nits == o.nits
    assert np.array_equal([r.residual], [o.residual], equal_nan=True)
    assert np.array_equal(r.trace, o.trace, equal_nan=True)
    assert np.array_equal(xh, o.x, equal_nan=True)


@pytest.mark.parametrize("c", CASES, ids=[SP.case_id(c) for c in CASES])
def test_serial_mode_bitwise_vs_reference(dev, systems, c):
    import lssp_amd
    r, xh = _gpu(dev, systems, c, lssp_amd.SERIAL)
    assert r.nits == c["nits"]
    assert r.residual == SP.fx(c["residual"])
    assert SP.matches(c["trace"], r.trace)
    assert SP.matches(c["x"], xh)


TREE = CASES + ZERO + K1M1


@pytest.mark.parametrize("c", TREE, ids=[SP.case_id(c) for c in TREE])
def test_tree_mode_bitwise_vs_oracle(dev, systems, c):
    """the fast path: the fixtures' cases, the zero-tolerance (m, k) runs that push the ring
    z[outer % k] round twice with full-width cycles, and k = 1 with m = 1"""
    import lssp_amd
    r, xh = _gpu(dev, systems, c, lssp_amd.TREE)
    _same_run(r, xh, SP.oracle_run(c, O.TREE))


@pytest.mark.parametrize("k", [0, -1])
@pytest.mark.parametrize("solver", SP.MK_SOLVERS)
def test_k_not_positive_is_k_three(dev, systems, solver, k):
    import lssp_amd
    c = SP.zero_case(solver, SP.MK_PCS[1], 2, 3)
    r3, x3 = _gpu(dev, systems, c, lssp_amd.TREE)
    r, xh = _gpu(dev, systems, c, lssp_amd.TREE, aug_k=k)
    _same_run(r, xh, SP.oracle_run(c, O.TREE))
    assert r.nits == r3.nits and r.residual == r3.residual
    assert np.array_equal(r.trace, r3.trace) and np.array_equal(xh, x3)


@pytest.mark.parametrize("mode", ["tree", "serial"])
@pytest.mark.parametrize("solver", ALL)
def test_exact_x0_bitwise_vs_oracle_and_x_stays(dev, systems, solver, mode):
    """x0 = 1 exact, b = A 1, atol = 0: r0 == 0.  Five drivers iterate once on it, the others
    return at 0; x stays 1 exactly either way"""
    import lssp_amd
    c = SP.exact_case(solver)
    r, xh = _gpu(dev, systems, c, lssp_amd.TREE if mode == "tree" else lssp_amd.SERIAL)
    _same_run(r, xh, SP.oracle_run(c, O.TREE if mode == "tree" else O.SERIAL))
    assert r.nits == (1 if solver in SP.EXACT_ITERATING else 0)
    assert np.array_equal(xh, np.ones(xh.size))


# ---- the restart limits of the GMRES family's setup -----------------------------------------------

def _scalar_slots():
    """(NSCAL, S_H) as internal.h defines them"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "lssp_amd", "csrc", "internal.h")) as f:
        src = f.read()
    nscal = re.findall(r"constexpr\s+int\s+NSCAL\s*=\s*(\d+)\s*;", src)
    s_h = re.findall(r"\bS_H\s*=\s*(\d+)\s*,", src)
    assert len(nscal) == 1 and len(s_h) == 1, (nscal, s_h)
    return int(nscal[0]), int(s_h[0])


@pytest.mark.parametrize("solver,k", [("GMRES", 0), ("LGMRES", 3), ("LGMRES", 5)])
def test_restart_limits(dev, solver, k):
    """restart = 0 is refused; the largest m + k with S_H + 2 (m + k) + 2 <= NSCAL runs and is the
    oracle's run bit for bit; one more is unsupported and leaves x as it was"""
    import lssp_amd
    nscal, s_h = _scalar_slots()
    top = (nscal - s_h - 2) // 2  # the largest m + k
    assert s_h + 2 * top + 2 <= nscal < s_h + 2 * (top + 1) + 2
    A = O.poisson(3, 4)
    assert A.n == 64
    D = lssp_amd.DMat(dev, A.Ap, A.Aj, A.Ax)
    bh, x0 = uniform(9, A.n), uniform(10, A.n)
    b = dev.vec(A.n, bh)
    sv = SP.SOLVERS[solver]
    run = lambda x, m: lssp_amd.solve(dev, D, None, x, b, solver=sv, maxit=6, restart=m, aug_k=k, trace_cap=100000)

    x = dev.vec(A.n, x0)
    with pytest.raises(lssp_amd.LsspError) as e:
        run(x, 0)
    assert e.value.status == 1  # LSSP_AMD_EINVAL
    assert np.array_equal(x.download(), x0)

    r = run(x, top - k)
    o = O.solve(sv, A, bh, x0=x0, maxit=6, restart=top - k, aug_k=k, mode=O.TREE)
    assert o.nits >= 6  # the left-preconditioned drivers test maxit between cycles only
    _same_run(r, x.download(), o)

    x = dev.vec(A.n, x0)
    with pytest.raises(lssp_amd.LsspError) as e:
        run(x, top - k + 1)
    assert e.value.status == 6  # LSSP_AMD_EUNSUPPORTED
    assert np.array_equal(x.download(), x0)
    D.close()
