#!/usr/bin/env python3
"""Generate the solver-parameter fixtures from the REFERENCE ITSELF (oracle/_ref/libref.so).

Run where the reference checker is built:
    make -C oracle all ref && python tests/golden/make_golden_solver_params.py

The cases are those of tests/solver_params_util.py (case_specs):
  mk     LGMRES / RLGMRES with k in {1, 2, 5} (lssp_solver_set_augk, lssp.cxx:485)
         and m in {2, 5}, no preconditioner and ILU(0), on the 10 x 9 x 7 box;
  stop   every driver with one term of the stop scale max(rtol ||r0||, atol,
         rbtol ||b||) deciding, and with all three;
  exact  x0 = 1 exact, b = A 1, atol = 0, for the five drivers that iterate once
         on the zero residual.
O.ref_solve passes the parameters to the reference's setters and records every
dot / norm the driver evaluates.  Each case stores its trace in full, sha256 and
norm of x, nits and the residual, in make_golden.py's case schema plus `aug_k`,
`group` and `rung`; the box matrix's arrays are stored once.  Written to
solver_params_manifest.json and solver_params.npz; only data is written.
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
import solver_params_util as SP  # noqa: E402
from inputs import digest  # noqa: E402


def main():
    arrays, out = {}, []
    box = SP.build_matrix(SP.BOX, recorded=False)
    for i, a in enumerate((box.Ap, box.Aj, box.Ax)):
        arrays[f"box7__{i}"] = a
    for c in SP.case_specs():
        A = SP.build_matrix(c["mat"], recorded=False)
        pc = O.PC_NON if c["pc"]["kind"] == "none" else O.PC_ILUK
        R = O.ref_solve(c["solver"], A, SP.vec(c["b"], A), pc=pc, level=c["pc"].get("level", 0),
                        x0=SP.vec(c["x0"], A), rtol=SP.fx(c["rtol"]), atol=SP.fx(c["atol"]), rbtol=SP.fx(c["rbtol"]),
                        maxit=c["maxit"], restart=c["restart"], aug_k=c["aug_k"])
        key = f"trace_{len(out)}"
        arrays[f"{key}__0"] = R.trace
        c.update({"nits": R.nits, "residual": R.residual.hex(),
                  "trace": {"npz": key, "count": 1, "sha256": digest(R.trace)},
                  "x": {"sha256": digest(R.x)}, "x_norm": float(np.linalg.norm(R.x)).hex()})
        out.append(c)
        print(f"{SP.case_id(c)}: nits {R.nits} residual {R.residual:.8e}", flush=True)
    np.savez_compressed(os.path.join(HERE, "solver_params.npz"), **arrays)
    with open(os.path.join(HERE, "solver_params_manifest.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_solver_params.py", "source": "oracle/_ref/libref.so "
                   "(reference compiled in place, g++ -O2)", "box7": SP.BOX, "cases": out}, f, indent=1)
    print(f"{len(out)} cases, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
