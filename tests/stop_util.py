"""Where a batched driver stops: the plan of stops and its inputs.  No GPU.

BiCGSTAB (no preconditioner or line sweeps) and CG (no preconditioner) queue
their iterations in batches (solvers.cpp: BATCH = 8, CG_BATCH = 32), two in
flight, and test for the stop on the device.  tests/test_gpu_batch_stops.py
puts a stop on every position of a batch; this module chooses the parameters
that put it there, from the CPU oracle alone:

  maxit  maxit = m, every tolerance 0.
  tol    h[m] is the oracle's residual after m iterations (h[0] the initial
         one).  Where h[m] < min(h[0..m-1]), atol = sqrt(h[m] * min(h[0..m-1]))
         lies strictly between the two, so the run stops with nits = m.
         CG's residual on these grids first rises above h[0] (h[1] > h[0]), and
         an atol >= h[0] ends the run before its first iteration (solver-cg.cxx
         :235, res <= tol_abs).  Where h[m] < min(h[1..m-1]) only, the same
         threshold t = sqrt(h[m] * min(h[1..m-1])) is therefore given as
         rtol = t / h[0] (atol = 0): the drivers test res <= max(rtol * h[0],
         atol, rbtol * ||b||) on the device either way.  For m = 1 the bound
         above h[1] is taken as 4 h[1].
  brk    BiCGSTAB's ||s|| <= 1e-40 exit (solver-bicgstab.cxx:117): b = 2^e * 1
         scales every vector and norm by 2^e exactly and leaves alpha, omega
         and beta bit-identical, so lowering e moves the first iteration with
         ||s|| <= 1e-40 towards the start.  The e of a wanted m comes from the
         ||s|| history of the b = 1 run and is kept only if the oracle then
         leaves with nits = m.

  rho    BiCGSTAB's "next iteration's rho1 == 0" exit (:89-92) needs r exactly
         orthogonal to r^ with r != 0: RHO_CASES are small integer systems,
         found by a random search with the oracle, on which its tree-order run
         leaves that way after iteration 7 (a batch's last) and 8 (the next
         batch's first).

"Stop at nits = m": the driver leaves in its iteration of index m - 1.
All runs: x0 = 0, rbtol = 0.
"""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, CG_BATCH = 8, 32   # what the positions below are laid out for; batch_sizes() reads the source
BIG_MAXIT = 1000          # "no maxit" for the tolerance stops
BRK_MAXIT = 60            # the breakdown runs: nits < BRK_MAXIT marks the exit
BREAKDOWN = 1e-40         # solver-bicgstab.cxx:117

# BiCGSTAB routes: (dim, N, ILUK level or None, sweep_layout() the handle must report)
BICG_ROUTES = {
    "nopc": (3, 16, None, None),
    "line2": (3, 20, 0, (1, 16, 8)),    # k_line2: 20 lines = 16 + 4, 20 planes = 8 + 8 + 4
    "linef": (3, 20, 1, (2, 16, 8)),    # k_linef: skewed ILU(1) tiles
    "lineg0": (2, 40, 0, (1, 40, 1)),   # k_lineg: one workgroup, a line per lane (lines == ny)
    "lineg1": (2, 40, 1, (2, 40, 1)),
}
BICG_SERIAL_ROUTES = ("nopc", "line2")
CG_MATS = {"p3_16": (3, 16), "p2_48": (2, 48)}

BICG_MAXIT_M = tuple(range(1, 19))
BICG_TOL_M = tuple(range(1, 18))
BICG_BRK_M = (8, 9, 16, 17)             # 8, 9 and one of 16, 17 are required
BICG_SERIAL_M = (7, 8, 9, 16, 17)
CG_EDGE_M = (1, 2, 31, 32, 33, 34, 63, 64, 65, 66)
CG_TOL_M = tuple(range(1, 67))

# two ranks, 7-pt 16^3, block-Jacobi ILU(0) per rank (BiCGSTAB) / no preconditioner (CG)
DIST_N, DIST_RANKS = 16, 2
DIST_BICG_TOL_M, DIST_BICG_MAXIT_M = (7, 8, 9, 10, 16, 17), (8, 9)
DIST_CG_TOL_M = (31, 32, 33, 34)


@dataclass(frozen=True)
class Stop:
    kind: str        # "maxit", "tol" or "brk"
    m: int           # the nits the run must report
    maxit: int
    atol: float = 0.0
    bexp: int = 0    # b = 2^bexp * 1
    rtol: float = 0.0

    @property
    def id(self) -> str:
        return f"{self.kind}{self.m}"


def batch_sizes():
    """(BATCH of BiCGSTAB, CG_BATCH) as solvers.cpp defines them"""
    with open(os.path.join(ROOT, "lssp_amd", "csrc", "solvers.cpp")) as f:
        src = f.read()
    bicg = re.findall(r"constexpr\s+int\s+BATCH\s*=\s*(\d+)\s*;", src)
    cg = re.findall(r"^#define\s+CG_BATCH\s+(\d+)", src, re.M)
    assert len(bicg) == 1 and len(cg) == 1, (bicg, cg)
    return int(bicg[0]), int(cg[0])


@lru_cache(maxsize=None)
def matrix(dim: int, N: int) -> O.CSR:
    return O.poisson(dim, N)


@lru_cache(maxsize=None)
def oracle_factors(dim: int, N: int, level: int, blk: int = 0):
    return O.ilu(matrix(dim, N), "iluk", level=level, blk=blk)


def rhs(n: int, bexp: int = 0) -> np.ndarray:
    return np.full(n, math.ldexp(1.0, bexp))


def _per_it(solver):
    # scalars traced per iteration after ||b|| and ||r0||: BiCGSTAB rho1, rh.v, ||s||, t.s, t.t,
    # ||r|| (:87-141); CG rho1, q.p, ||r|| (solver-cg.cxx:80-106)
    return 6 if solver == O.BICGSTAB else 3


def history(solver, A, L, U, mode, upto, nranks=1):
    """(h, s): h[0..upto] the residual after that many iterations, s[k] BiCGSTAB's ||s|| in
    iteration k (None for CG), read from the trace of one run of `upto` iterations"""
    o = O.solve(solver, A, rhs(A.n), L=L, U=U, rtol=0.0, atol=0.0, rbtol=0.0, maxit=upto, mode=mode,
                nranks=nranks)
    w = _per_it(solver)
    assert o.nits == upto and o.trace.size == 2 + w * upto, (o.nits, o.trace.size)
    h = [float(o.trace[1])] + [float(o.trace[1 + w * m]) for m in range(1, upto + 1)]
    assert h[-1] == o.residual
    s = [float(o.trace[2 + w * k + 2]) for k in range(upto)] if solver == O.BICGSTAB else None
    return h, s


def maxit_stops(ms):
    return [Stop("maxit", m, m) for m in ms]


def tol_stops(h, ms):
    """a tolerance stop for every m of ms at which the residual reaches a new low: below
    h[0..m-1] through atol, below h[1..m-1] only (h[0] is lower) through rtol"""
    out = []
    for m in ms:
        low = min(h[:m])
        if 0.0 < h[m] < low:
            atol = math.sqrt(h[m] * low)
            if h[m] < atol < low:
                out.append(Stop("tol", m, BIG_MAXIT, atol=atol))
            continue
        low = min(h[1:m]) if m > 1 else 4.0 * h[m]
        if 0.0 < h[m] < low:
            rtol = math.sqrt(h[m] * low) / h[0]
            if h[m] < rtol * h[0] < low:  # the product as the drivers round it
                out.append(Stop("tol", m, BIG_MAXIT, rtol=rtol))
    return out


def expect(solver, A, L, U, mode, stop: Stop, nranks=1) -> O.SolveResult:
    """the oracle's run of a stop"""
    return O.solve(solver, A, rhs(A.n, stop.bexp), L=L, U=U, rtol=stop.rtol, atol=stop.atol, rbtol=0.0,
                   maxit=stop.maxit, mode=mode, nranks=nranks)


def is_breakdown(o: O.SolveResult, maxit: int) -> bool:
    """the run left through :117: ||s|| <= 1e-40 traced twice (:117, :118), then the true residual"""
    t = o.trace
    return o.nits < maxit and t.size >= 3 and t[-3] == t[-2] and 0.0 <= t[-2] <= BREAKDOWN


def brk_stops(A, L, U, mode, ms):
    """a :117 exit for every m of ms whose ||s|| is a new low; e from the b = 1 history, kept
    only if the oracle leaves there"""
    _, s = history(O.BICGSTAB, A, L, U, mode, max(ms))
    out = []
    for m in ms:
        if not (0.0 < s[m - 1] and (m == 1 or s[m - 1] < min(s[:m - 1]))):
            continue
        e0 = math.floor(math.log2(BREAKDOWN / s[m - 1]))
        for e in (e0, e0 - 1, e0 + 1):
            st = Stop("brk", m, BRK_MAXIT, bexp=e)
            o = expect(O.BICGSTAB, A, L, U, mode, st)
            if o.nits == m and is_breakdown(o, BRK_MAXIT):
                out.append(st)
                break
    return out


def route_inputs(route: str):
    """(A, L, U) of a BiCGSTAB route, the factors by the oracle"""
    dim, N, level, _ = BICG_ROUTES[route]
    A = matrix(dim, N)
    L, U = (None, None) if level is None else oracle_factors(dim, N, level)
    return A, L, U


@lru_cache(maxsize=None)
def bicg_plan(route: str, mode: int):
    """{"maxit": [...], "tol": [...], "brk": [...]} of a BiCGSTAB route in a reduction mode"""
    A, L, U = route_inputs(route)
    if mode == O.TREE:
        h, _ = history(O.BICGSTAB, A, L, U, mode, max(BICG_TOL_M))
        return {"maxit": maxit_stops(BICG_MAXIT_M), "tol": tol_stops(h, BICG_TOL_M),
                "brk": brk_stops(A, L, U, mode, BICG_BRK_M)}
    h, _ = history(O.BICGSTAB, A, L, U, mode, max(BICG_SERIAL_M))
    return {"maxit": maxit_stops(BICG_SERIAL_M), "tol": tol_stops(h, BICG_SERIAL_M), "brk": []}


@lru_cache(maxsize=None)
def cg_plan(mat: str, mode: int):
    A = matrix(*CG_MATS[mat])
    h, _ = history(O.CG, A, None, None, mode, max(CG_TOL_M))
    return {"maxit": maxit_stops(CG_EDGE_M), "tol": tol_stops(h, CG_TOL_M)}


def dist_inputs(solver):
    A = matrix(3, DIST_N)
    if solver == O.CG:
        return A, None, None
    L, U = oracle_factors(3, DIST_N, 0, (A.n + DIST_RANKS - 1) // DIST_RANKS)
    return A, L, U


@lru_cache(maxsize=None)
def dist_plan(solver: int):
    """the two-rank stops, placed by the histories of the oracle's own 2-rank mode"""
    A, L, U = dist_inputs(solver)
    if solver == O.CG:
        h, _ = history(solver, A, L, U, O.TREE, max(DIST_CG_TOL_M), nranks=DIST_RANKS)
        return tol_stops(h, DIST_CG_TOL_M)
    h, _ = history(solver, A, L, U, O.TREE, max(DIST_BICG_TOL_M), nranks=DIST_RANKS)
    return tol_stops(h, DIST_BICG_TOL_M) + maxit_stops(DIST_BICG_MAXIT_M)


# m -> (dense rows, b): the oracle (TREE order, tolerances 0) computes rho1 == 0 exactly in the
# last reduction of iteration m - 2 and reports nits = m
RHO_CASES = {
    9: ([[3, 0, 0, -1, -3, 0, 0, 0, 0, 0, 0, 1], [0, 2, 0, 0, -1, 0, -2, 0, 0, 0, 0, 0],
         [-2, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0],
         [-3, 0, 0, 0, 4, 0, 0, -1, 0, 0, 0, 0], [0, 0, -1, -2, 0, 1, 0, 0, 3, 0, 0, 0],
         [0, -3, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0],
         [0, -3, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0],
         [0, 0, 0, 0, 0, 0, 0, 0, 0, -1, 4, 0], [0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]],
        [0, 0, 0, 1, 0, 0, 1, 2, 0, 0, -1, 1]),
    10: ([[2, 0, 0, 0, 0, 0, -3, 0], [0, 3, 1, 0, 2, 0, 3, 0], [0, 0, 2, 2, 0, 0, -2, 0], [0, 0, 3, 2, 0, 0, 0, 0],
          [0, -3, -3, -2, 2, 0, -1, -1], [-2, 0, 0, 0, 0, 1, 0, 0], [-3, 0, 0, 0, 0, 0, 2, 0],
          [0, 0, 0, 0, 0, 0, 0, 2]],
         [-2, 0, 2, 2, 0, 2, 0, -2]),
}
RHO_MAXIT = 40


def rho_case(m: int):
    """(A, b) of RHO_CASES[m]"""
    rows, b = RHO_CASES[m]
    M = np.array(rows, np.float64)
    n = M.shape[0]
    nz = M != 0
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum(nz.sum(axis=1), out=Ap[1:])
    Aj = np.nonzero(nz)[1].astype(np.int32)
    return O.CSR(n, Ap, Aj, M[nz]), np.array(b, np.float64)


def rho_expect(m: int) -> O.SolveResult:
    A, b = rho_case(m)
    return O.solve(O.BICGSTAB, A, b, rtol=0.0, atol=0.0, rbtol=0.0, maxit=RHO_MAXIT, mode=O.TREE)


def is_rho_exit(o: O.SolveResult, maxit: int) -> bool:
    """the run left through :89-92: a whole number of iterations traced, then rho1 == 0"""
    return 1 < o.nits < maxit and o.trace.size == 2 + 6 * (o.nits - 1) + 1 and o.trace[-1] == 0.0
