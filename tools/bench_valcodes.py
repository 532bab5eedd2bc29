"""Value codes of the SpMV (lssp_amd_mat::Av): what building them costs.

    python tools/bench_valcodes.py [--grid 216] [--reps 6]
    python tools/bench_valcodes.py --thermal

One JSON line per item.  The 7-pt grid's upload (value-coded), then
lssp_amd_mat_update_values alternating between two constant-coefficient value
sets (the codes are rebuilt: collect, sort, code and verify every row) and
between two random ones (the collection stops at the 257th distinct row and
the codes are dropped).  The call returns after the device is idle, so the
wall time is the cost.  --thermal: config 5's matrix, which cannot be coded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def wall(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=216)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--thermal", action="store_true")
    args = ap.parse_args()
    import lssp_amd
    dev = lssp_amd.Device(0)
    if args.thermal:
        from lssp_amd.synthetic import thermal_like
        Ap, Aj, Ax = thermal_like()
        name = "thermal-like"
    else:
        Ap, Aj, Ax = lssp_amd.poisson(3, args.grid)
        name = f"poisson {args.grid}^3"
    n, nnz = Ap.size - 1, Ax.size
    A = None

    def up():
        nonlocal A
        A = lssp_amd.DMat(dev, Ap, Aj, Ax)

    t_up = wall(up)
    print(json.dumps({"item": "mat_upload", "matrix": name, "rows": n, "nnz": nnz, "ms": round(t_up, 2),
                      "ndiag": A.ndiag, "rowcodes": A.rowcodes, "valcodes": A.valcodes,
                      "device_bytes": list(A.device_bytes)}), flush=True)
    if args.thermal:
        return
    rng = np.random.default_rng(5)
    sets = {"constant": [dev.vec(nnz, Ax), dev.vec(nnz, 2.0 * Ax)],
            "random": [dev.vec(nnz, rng.uniform(-1, 1, nnz)), dev.vec(nnz, rng.uniform(-1, 1, nnz))]}
    for kind, v in sets.items():
        A.update_values(v[1])
        t = [wall(lambda k=k: A.update_values(v[k % 2])) for k in range(args.reps)]
        print(json.dumps({"item": "mat_update_values", "values": kind, "valcodes": A.valcodes,
                          "ms_median": round(float(np.median(t)), 3), "ms_min": round(min(t), 3), "reps": len(t),
                          "copy_bytes": 16 * nnz}), flush=True)


if __name__ == "__main__":
    main()
