"""BILUK's host path and the new interface, without a GPU.

The reference's block values depend on the BLAS / LAPACK it is linked with, so
lssp_amd_bilu_factor_host is compared with a numpy restatement of pc-biluk.cxx
(bilu_util.bilu_numpy) whose inverse is LAPACK's dgetrf + dgetri and whose
product follows netlib dgemm.  Patterns must be equal; the bound on the values
is measured here, not chosen: the restatement is evaluated a second time with
numpy.linalg.inv and @, the spread between the two evaluations (max |delta| /
max |value| over L, Dinv and U, the largest over the shapes) is what two
correct implementations differ by, and the library must lie within 8 x that of
the first evaluation -- the constant between two backward-stable eliminations
of well-conditioned blocks -- floored at 64 eps so a zero spread cannot make
the bound vacuous.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import oracle as O
from bilu_util import (CASES, bilu_numpy, block_grid, case_name, gemm_numpy, inv_numpy, rel_distance)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssp_amd.h")
EINVAL = 1
EPS = float(np.finfo(np.float64).eps)


def _case_matrix(c):
    dim, N, bs, level, shuffle, variant = c
    return block_grid(dim, N, bs, seed=100 + CASES.index(c), shuffle=shuffle, variant=variant)


@pytest.fixture(scope="module")
def evaluations():
    """per case: the library's host factors and the restatement's two evaluations (computed once)"""
    pytest.importorskip("scipy")
    import lssp_amd
    out = {}
    for c in CASES:
        Ap, Aj, Ax = _case_matrix(c)
        bs, level = c[2], c[3]
        sp, sj, sx = lssp_amd.sort_columns(Ap, Aj, Ax)
        out[c] = (lssp_amd.bilu_factor_host(Ap, Aj, Ax, bs, level), bilu_numpy(sp, sj, sx, bs, level),
                  bilu_numpy(sp, sj, sx, bs, level, inv=inv_numpy, gemm=gemm_numpy))
    return out


def test_host_factors_against_lapack(evaluations):
    spread = max(rel_distance(lap, alt) for _, lap, alt in evaluations.values())
    bound = max(8 * spread, 64 * EPS)
    print(f"\nreference spread (LAPACK + netlib order vs numpy inv + @): {spread:.3e}; bound {bound:.3e}")
    worst = 0.0
    for c, (lib, lap, alt) in evaluations.items():
        for f in (0, 2):  # patterns of L and U
            assert np.array_equal(lib[f][0], lap[f][0]) and np.array_equal(lib[f][1], lap[f][1]), case_name(c)
        d = rel_distance(lap, lib)
        worst = max(worst, d)
        print(f"  {case_name(c):24s} spread {rel_distance(lap, alt):.3e}  library distance {d:.3e}")
        assert d <= bound, (case_name(c), d, bound)
    print(f"largest library distance {worst:.3e}")


@pytest.mark.parametrize("c", CASES, ids=[case_name(c) for c in CASES])
def test_structure_and_size_query(c):
    import lssp_amd
    L_ = lssp_amd._lib.load()
    Ap, Aj, Ax = _case_matrix(c)
    bs, level = c[2], c[3]
    n = Ap.size - 1
    (Lp, Lj, Lx), Dinv, (Up, Uj, Ux) = lssp_amd.bilu_factor_host(Ap, Aj, Ax, bs, level)
    # L's last and U's first entry of every row: the diagonal, exactly 1
    assert np.array_equal(Lj[Lp[1:] - 1], np.arange(n)) and np.all(Lx[Lp[1:] - 1] == 1.0)
    assert np.array_equal(Uj[Up[:-1]], np.arange(n)) and np.all(Ux[Up[:-1]] == 1.0)
    for p, j in ((Lp, Lj), (Up, Uj)):  # columns ascending
        inner = np.ones(j.size - 1, bool)
        inner[p[1:-1] - 1] = False
        assert np.all(np.diff(j)[inner] > 0)
    # sizes: bs^2 per strict block + n; every entry of a block is kept
    nb = n // bs
    assert (Lj.size - n) % (bs * bs) == 0 and (Uj.size - n) % (bs * bs) == 0
    if level == 0:
        blocks = {(r // bs, int(col) // bs) for r in range(n) for col in Aj[Ap[r]:Ap[r + 1]]}
        assert Lj.size == bs * bs * sum(1 for i, j in blocks if j < i) + n
        assert Uj.size == bs * bs * sum(1 for i, j in blocks if j > i) + n
    assert Dinv.size == nb * bs * bs
    # the two-call size query agrees with the filled call
    nl, nu = ctypes.c_int(), ctypes.c_int()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert L_.lssp_amd_bilu_factor_host(n, p(Ap), p(Aj), p(Ax), level, bs, ctypes.byref(nl), ctypes.byref(nu),
                                        None, None, None, None, None, None, None) == 0
    assert (nl.value, nu.value) == (Lj.size, Uj.size)


def _raw(Ap, Aj, Ax, bs, level=0):
    import lssp_amd
    L_ = lssp_amd._lib.load()
    nl, nu = ctypes.c_int(), ctypes.c_int()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    n = Ap.size - 1
    cap = 64 * Aj.size + 64 * n  # room for any block size tried here
    dbl = [np.zeros(cap) for _ in range(3)]
    idx = [np.zeros(cap, np.int32) for _ in range(4)]
    return L_.lssp_amd_bilu_factor_host(n, p(Ap), p(Aj), p(Ax), level, bs, ctypes.byref(nl), ctypes.byref(nu),
                                        p(idx[0]), p(idx[1]), p(dbl[0]), p(dbl[1]), p(idx[2]), p(idx[3]),
                                        p(dbl[2]))


def test_errors_and_edge_cases():
    import lssp_amd
    Ap, Aj, Ax = block_grid(2, 6, 2, seed=5)
    assert _raw(Ap, Aj, Ax, 5) == EINVAL    # n % bs != 0 (72 % 5)
    Ap3, Aj3, Ax3 = block_grid(2, 3, 11, seed=6)
    assert _raw(Ap3, Aj3, Ax3, 33) == EINVAL  # n = 99 = 3 * 33: bs above the largest supported block
    assert _raw(Ap3, Aj3, Ax3, 11) == 0
    # an exactly singular (all-zero) diagonal block: EINVAL where the reference exits
    Az = block_grid(2, 6, 2, seed=5, variant="zerodiag")
    assert _raw(*Az, 2) == EINVAL
    with pytest.raises(lssp_amd.LsspError):
        lssp_amd.bilu_factor_host(*Az, 2)
    # a missing diagonal block: the identity as its inverse (pc-biluk.cxx:265-270 as intended)
    An = block_grid(2, 6, 2, seed=5, variant="nodiag")
    _, Dinv, _ = lssp_amd.bilu_factor_host(*An, 2)
    mid = 36 // 2
    assert np.array_equal(Dinv[4 * mid:4 * mid + 4], np.array([1.0, 0.0, 0.0, 1.0]))
    assert not np.array_equal(Dinv[4 * (mid - 1):4 * mid], np.array([1.0, 0.0, 0.0, 1.0]))


def test_interface_names_and_constants():
    import lssp_amd
    from lssp_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("lssp_amd_bilu_create", "lssp_amd_ilu_from_ldu", "lssp_amd_ilu_get_diag",
                 "lssp_amd_bilu_factor_host"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    enums = re.findall(r"enum\s*\{([^}]*)\}", src)
    solver = next(e for e in enums if "LSSP_AMD_GMRES" in e)
    pc = next(e for e in enums if "LSSP_AMD_ILUK" in e)
    assert re.search(r"LSSP_AMD_RLGMRES\s*=\s*3\b", solver)
    assert re.search(r"LSSP_AMD_BILUK\s*=\s*3\b", pc)
    assert lssp_amd.RLGMRES == 3 and lssp_amd.BILUK == 3
    assert callable(lssp_amd.DILU.bilu) and callable(lssp_amd.DILU.from_ldu) and callable(lssp_amd.DILU.diag)
    assert lssp_amd._lib.load().lssp_amd_version() >= 10100


# ---- the RLGMRES fixtures reproduce from the reference ----------------------------------
with open(os.path.join(ROOT, "tests", "golden", "rlgmres_manifest.json")) as _f:
    RL = json.load(_f)["cases"]


def test_rlgmres_fixture_cases():
    """the eight LGMRES shapes of make_golden.py, the unpreconditioned one capped at 300"""
    assert len(RL) == 8 and all(c["solver"] == 3 and c["kind"] == "solve" for c in RL)
    nopc = [c for c in RL if c["pc"]["kind"] == "none"]
    assert len(nopc) == 1 and nopc[0]["maxit"] == 300 and nopc[0]["nits"] == 300
    by = {(c["pc"]["kind"], c["mat"].get("N"), c["restart"]): c["nits"] for c in RL}
    assert by[("iluk", 100, 20)] == 60  # 5-pt 100^2 ILU(1), m 20


@pytest.mark.skipif(not O.ref_available(), reason="reference checker not built (make -C oracle ref)")
@pytest.mark.parametrize("k", range(8))
def test_rlgmres_fixtures_reproduce_from_reference(k):
    import sys
    from golden_util import fx, matches
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_rlgmres as G
    c = RL[k]
    pc, mat, bspec, x0spec, kw = G.SOLVES[k]
    case, R = G.run_case(pc, mat, bspec, x0spec, kw)
    for key in ("solver", "pc", "mat", "b", "x0", "maxit", "restart", "rtol", "atol", "rbtol", "nits"):
        assert case[key] == c[key], key
    assert R.residual == fx(c["residual"])
    assert matches(c["trace"], R.trace) and matches(c["x"], R.x)
