#!/usr/bin/env python3
"""Generate the RLGMRES fixtures from the REFERENCE ITSELF (oracle/_ref/libref.so).

Run where the reference checker is built:
    make -C oracle all ref && python tests/golden/make_golden_rlgmres.py

Right-preconditioned LGMRES(m, k = 3) is LSSP_SOLVER_RLGMRES = 3
(lssp_solver_lgmres_r, solver-lgmres.cxx:313-604).  O.ref_solve passes the
solver value straight to lssp_solver_solve and records every dot / norm the
driver evaluates.  The cases are the eight LGMRES shapes of make_golden.py, the
unpreconditioned one capped at 300 iterations (RLGMRES never uses its
augmentation vectors in the update, so small restarts converge slowly: 2914
iterations uncapped).  Written in make_golden.py's case schema to
rlgmres_manifest.json and rlgmres.npz; only data is written.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import oracle as O  # noqa: E402
from make_golden import Store, build_matrix, vec  # noqa: E402

RLGMRES = 3  # LSSP_SOLVER_RLGMRES (type-defs.h)

P7 = lambda N: {"type": "poisson", "dim": 3, "N": N}  # noqa: E731
P5 = lambda N: {"type": "poisson", "dim": 2, "N": N}  # noqa: E731
RND2 = {"type": "rand", "n": 2000, "per_row": 5, "seed": 4242, "unsorted": True, "missing_diag_every": 0,
        "diag": 3.0}

SOLVES = [
    ({"kind": "ilut", "tol": 1e-4, "p": 20}, P7(32), "ones", None, {"restart": 30}),
    ({"kind": "iluk", "level": 0}, P7(32), "ones", None, {"restart": 10}),
    ({"kind": "iluk", "level": 1}, P5(100), "ones", None, {"restart": 20}),
    ({"kind": "none"}, P7(16), "ones", None, {"restart": 8, "maxit": 300}),
    ({"kind": "iluk", "level": 0}, P7(16), "ones", None, {"maxit": 13, "restart": 5}),
    ({"kind": "ilut", "tol": 1e-3, "p": 5}, RND2, 0x5EED, 0xB0B, {"restart": 6}),
    ({"kind": "bj", "nblk": 4}, P7(32), "ones", None, {"restart": 12}),
    ({"kind": "iluk", "level": 0}, P7(16), "zeros", None, {}),
]
PCMAP = {"none": O.PC_NON, "iluk": O.PC_ILUK, "ilut": O.PC_ILUT}


def run_case(pc, mat, bspec, x0spec, kw):
    """one reference run -> (case parameters, SolveResult)"""
    A = build_matrix(mat)
    b = vec(bspec, A.n)
    x0 = None if x0spec is None else vec(x0spec, A.n)
    maxit = kw.get("maxit", 5000)
    restart = kw.get("restart", 30)
    if pc["kind"] == "bj":
        R = O.ref_solve_bj(RLGMRES, A, b, pc["nblk"], x0=x0, maxit=maxit, restart=restart)
    else:
        R = O.ref_solve(RLGMRES, A, b, pc=PCMAP[pc["kind"]], level=pc.get("level", 0),
                        ilut_tol=pc.get("tol", 1e-3), ilut_p=pc.get("p", -1), x0=x0, maxit=maxit, restart=restart)
    case = {"kind": "solve", "solver": RLGMRES, "pc": pc, "mat": mat, "b": bspec, "x0": x0spec,
            "maxit": maxit, "restart": restart, "rtol": (1e-7).hex(), "atol": (1e-7).hex(),
            "rbtol": (1e-7).hex(), "nits": R.nits, "residual": R.residual.hex()}
    return case, R


def main():
    S = Store()
    for pc, mat, bspec, x0spec, kw in SOLVES:
        case, R = run_case(pc, mat, bspec, x0spec, kw)
        case.update({"trace": S.put(f"trace_{len(S.cases)}", R.trace),
                     "x": S.put(f"x_{len(S.cases)}", R.x), "x_norm": float(np.linalg.norm(R.x)).hex()})
        S.cases.append(case)
        print(f"rlgmres {pc} {mat.get('N', mat.get('n'))}: nits {R.nits} residual {R.residual:.8e}", flush=True)
    np.savez_compressed(os.path.join(HERE, "rlgmres.npz"), **S.arrays)
    with open(os.path.join(HERE, "rlgmres_manifest.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_rlgmres.py", "source": "oracle/_ref/libref.so "
                   "(reference compiled in place, g++ -O2)", "cases": S.cases}, f, indent=1)
    print(f"{len(S.cases)} cases, {len(S.arrays)} arrays")


if __name__ == "__main__":
    main()
