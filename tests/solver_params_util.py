"""The cases that pin LGMRES / RLGMRES's k and every driver's stop rule.  No GPU.

Shared by tests/golden/make_golden_solver_params.py (which runs the reference on
them), tests/test_solver_params_cpu.py (the oracle against those runs, and the
conditions that keep the GPU comparisons from passing vacuously) and
tests/test_gpu_solver_params.py.

  mk     LGMRES(m, k) and RLGMRES(m, k), k in {1, 2, 5} x m in {2, 5} (k > m
         included), without a preconditioner and with ILU(0), on a random-valued
         nonsymmetric 7-point 10 x 9 x 7 box; b = uniform(seed), x0 = 0, the
         default tolerances, maxit = 80.
  stop   all 19 drivers on the 7-point Poisson 8^3 with ILU(0), b = uniform(3),
         x0 = uniform(4) (so ||r0|| ~ 89.9 and ||b|| ~ 13.3 differ), restart 6,
         maxit 60: one run per term of the stop scale max(rtol ||r0||, atol,
         rbtol ||b||) with the other two tolerances 0, and one with all three.
  exact  x0 = 1, b = A 1 (exact on the integer Poisson matrix), atol = 0: the
         drivers whose start test is not "res <= atol" iterate once on a zero
         residual.
  zero   (oracle only, no fixture) the mk grid with every tolerance 0, stopped
         by maxit after exactly 2k + 1 full-width cycles.  On the mk box LGMRES
         is at roundoff (1e-16 ||r0||) long before that, so these runs take a
         harder system of the same kind: a 25 x 25 box whose diagonal is only
         (1 + 1e-3) times its row's off-diagonal sum; there every run ends
         above 1e-6 ||r0||.
"""
from __future__ import annotations

import json
import os
from functools import lru_cache

import numpy as np

import oracle as O
from inputs import digest, uniform

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SOLVERS = {"GMRES": 0, "LGMRES": 1, "RGMRES": 2, "RLGMRES": 3, "BICGSTAB": 4, "BICGSTABL": 5, "BICGSAFE": 6,
           "CG": 7, "CGS": 8, "GPBICG": 9, "CR": 10, "CRS": 11, "BICRSTAB": 12, "BICRSAFE": 13, "GPBICR": 14,
           "QMRCGSTAB": 15, "TFQMR": 16, "ORTHOMIN": 17, "IDRS": 18}
NAMES = {v: k for k, v in SOLVERS.items()}

BOX = {"type": "box7", "nx": 10, "ny": 9, "nz": 7, "seed": 26}
BOX_B = 1097
MK_SOLVERS = ("LGMRES", "RLGMRES")
MK_GRID = [(m, k) for k in (1, 2, 5) for m in (2, 5)]
MK_PCS = ({"kind": "none"}, {"kind": "iluk", "level": 0})
MK_MAXIT = 80
ZERO_BOX = {"type": "box7", "nx": 25, "ny": 25, "nz": 1, "seed": 5, "weak": 1e-3}

P8 = {"type": "poisson", "dim": 3, "N": 8}
ILU0 = {"kind": "iluk", "level": 0}
STOP_B, STOP_X0, STOP_MAXIT, STOP_RESTART = 3, 4, 60, 6
# the ladder: one rung per term of the stop scale, then all three together
LADDER = {"rtol": (1e-9, 0.0, 0.0), "atol": (0.0, 1e-2, 0.0), "rbtol": (0.0, 0.0, 1e-6), "all": (1e-9, 1e-2, 1e-6)}
# BiCGSTAB(l = 4) stops the rtol and rbtol runs at the same count (8 / 4 / 8): l = 2 there; s = 4 for IDR(s)
STOP_PARAM = {"BICGSTABL": 2, "IDRS": 4}

# x0 exact: the drivers that run one iteration on the zero residual
EXACT_ITERATING = ("BICGSAFE", "CR", "CRS", "BICRSTAB", "BICRSAFE")
EXACT_MAXIT = 20


def box7(nx, ny, nz, seed):
    """7-pt stencil on an nx x ny x nz box (natural order, i fastest), random
    nonsymmetric diagonally dominant values"""
    rng = np.random.default_rng(seed)
    n = nx * ny * nz
    Ap, Aj, Ax = [0], [], []
    for r in range(n):
        i, j, k = r % nx, r // nx % ny, r // (nx * ny)
        cols = [c for c, ok in ((r - nx * ny, k > 0), (r - nx, j > 0), (r - 1, i > 0), (r, True),
                                (r + 1, i < nx - 1), (r + nx, j < ny - 1), (r + nx * ny, k < nz - 1)) if ok]
        vals = rng.uniform(-1, -0.1, len(cols))
        vals[cols.index(r)] = 7.0 + rng.uniform(0, 1)
        Aj += cols
        Ax += list(vals)
        Ap.append(len(Aj))
    return np.array(Ap, np.int32), np.array(Aj, np.int32), np.array(Ax)


def weaken(Ap, Aj, Ax, eps):
    """every diagonal entry replaced by (1 + eps) times its row's off-diagonal absolute sum"""
    Ax = Ax.copy()
    for r in range(Ap.size - 1):
        q = np.arange(Ap[r], Ap[r + 1])
        d = q[Aj[q] == r]
        assert d.size == 1
        Ax[d[0]] = (np.abs(Ax[q]).sum() - abs(Ax[d[0]])) * (1 + eps)
    return Ap, Aj, Ax


def param(name: str) -> int:
    """what rides in `restart` in the stop and exact cases: m, ORTHOMIN's k, l or s"""
    return STOP_PARAM.get(name, STOP_RESTART)


def _case(solver, pc, mat, b, x0, maxit, restart, tols, aug_k, group, rung=None):
    c = {"kind": "solve", "group": group, "solver": SOLVERS[solver], "pc": pc, "mat": mat, "b": b, "x0": x0,
         "maxit": maxit, "restart": restart, "rtol": float(tols[0]).hex(), "atol": float(tols[1]).hex(),
         "rbtol": float(tols[2]).hex(), "aug_k": aug_k}
    if rung is not None:
        c["rung"] = rung
    return c


def exact_case(solver):
    return _case(solver, ILU0, P8, "A1", "ones", EXACT_MAXIT, param(solver), (1e-7, 0.0, 1e-7), 3, "exact")


def case_specs():
    """every fixture's parameters, in the manifest's order (no results)"""
    out = []
    for s in MK_SOLVERS:
        for pc in MK_PCS:
            for m, k in MK_GRID:
                out.append(_case(s, pc, BOX, BOX_B, None, MK_MAXIT, m, (1e-7, 1e-7, 1e-7), k, "mk"))
    for s in SOLVERS:
        for rung, tols in LADDER.items():
            out.append(_case(s, ILU0, P8, STOP_B, STOP_X0, STOP_MAXIT, param(s), tols, 3, "stop", rung))
    for s in EXACT_ITERATING:
        out.append(exact_case(s))
    return out


@lru_cache(maxsize=None)
def _loaded():
    with open(os.path.join(HERE, "solver_params_manifest.json")) as f:
        m = json.load(f)
    return m, dict(np.load(os.path.join(HERE, "solver_params.npz"), allow_pickle=False))


def cases(group=None):
    """the fixtures (tests/golden/solver_params_manifest.json)"""
    return [c for c in _loaded()[0]["cases"] if group is None or c["group"] == group]


def stored(entry):
    return [_loaded()[1][f"{entry['npz']}__{i}"] for i in range(entry["count"])]


@lru_cache(maxsize=None)
def _box(nx, ny, nz, seed, weak, recorded):
    if recorded:  # the arrays the fixtures were made with
        z = _loaded()[1]
        return O.CSR(nx * ny * nz, z["box7__0"], z["box7__1"], z["box7__2"])
    M = box7(nx, ny, nz, seed)
    return O.CSR(nx * ny * nz, *(weaken(*M, weak) if weak else M))


@lru_cache(maxsize=None)
def _poisson(dim, N):
    return O.poisson(dim, N)


def build_matrix(spec, recorded=True) -> O.CSR:
    if spec["type"] == "poisson":
        return _poisson(spec["dim"], spec["N"])
    weak = spec.get("weak", 0.0)  # only the mk box is recorded
    return _box(spec["nx"], spec["ny"], spec["nz"], spec["seed"], weak, recorded and not weak)


def vec(spec, A: O.CSR):
    if spec is None or spec == "zeros":
        return np.zeros(A.n)
    if spec == "ones":
        return np.ones(A.n)
    if spec == "A1":  # A 1: small integers on the Poisson matrix, exact in any order
        return O.spmv(0, A, np.ones(A.n))
    return uniform(int(spec), A.n)


_factors = {}


def factors(c, recorded=True):
    """(L, U) of a case by the oracle; (None, None) without a preconditioner"""
    if c["pc"]["kind"] == "none":
        return None, None
    key = (json.dumps(c["mat"], sort_keys=True), c["pc"]["level"], recorded)
    if key not in _factors:
        _factors[key] = O.ilu(build_matrix(c["mat"], recorded), "iluk", level=c["pc"]["level"])
    return _factors[key]


def fx(h: str) -> float:
    return float.fromhex(h)


def oracle_run(c, mode, recorded=True, **over) -> O.SolveResult:
    """the oracle's run of a case (or of a case with some parameters replaced)"""
    c = dict(c, **over)
    A = build_matrix(c["mat"], recorded)
    L, U = factors(c, recorded)
    return O.solve(c["solver"], A, vec(c["b"], A), x0=vec(c["x0"], A), L=L, U=U, rtol=fx(c["rtol"]),
                   atol=fx(c["atol"]), rbtol=fx(c["rbtol"]), maxit=c["maxit"], restart=c["restart"], mode=mode,
                   aug_k=c["aug_k"])


def case_id(c) -> str:
    pc = "nopc" if c["pc"]["kind"] == "none" else f"ilu{c['pc']['level']}"
    if c["group"] in ("mk", "zero"):
        return f"{NAMES[c['solver']]}-{pc}-m{c['restart']}-k{c['aug_k']}" + ("-tol0" if c["group"] == "zero" else "")
    if c["group"] == "stop":
        return f"{NAMES[c['solver']]}-{c['rung']}"
    return f"{NAMES[c['solver']]}-{c['group']}"


def matches(entry, *arrays) -> bool:
    return digest(*arrays) == entry["sha256"]


# ---- the zero-tolerance (m, k) runs -----------------------------------------

def widths(m, k, ncycles):
    """the cycles' widths: one more column per cycle up to m + k"""
    return [m + min(j, k) for j in range(ncycles)]


def zero_case(solver, pc, m, k):
    """every tolerance 0, maxit = the columns of exactly 2k + 1 full cycles: the ring z[outer % k]
    goes round twice and is written a third time"""
    return _case(solver, pc, ZERO_BOX, BOX_B, None, sum(widths(m, k, 2 * k + 1)), m, (0.0, 0.0, 0.0), k, "zero")


def zero_cases():
    return [zero_case(s, pc, m, k) for s in MK_SOLVERS for pc in MK_PCS for m, k in MK_GRID]


def full_cycles_trace_len(ws):
    """the dots and norms of a run of full cycles of these widths: ||b||, ||r0||, then per cycle
    the norm that opens it, column i's i + 1 dots and one norm, and the residual norm that closes it"""
    return 2 + sum(2 + sum(i + 2 for i in range(w)) for w in ws)
