"""CG without a preconditioner on the thermal-like mesh (the windowed product with one fused dot,
k_spmv_sell<*, 1>): ms per iteration, and the bare product"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lssp_amd
from lssp_amd.synthetic import thermal_like

Ap, Aj, Ax = thermal_like()
n = Ap.size - 1
dev = lssp_amd.Device(0)
A = lssp_amd.DMat(dev, Ap, Aj, Ax)
out = {"rows": n, "windowed": bool(A.windowed), "ndiag": A.ndiag}


def run(iters):
    x, b = dev.vec(n, np.zeros(n)), dev.vec(n, np.ones(n))
    dev.sync()
    t0 = time.perf_counter()
    r = lssp_amd.solve(dev, A, None, x, b, solver=lssp_amd.CG, tol_rel=0.0, tol_abs=0.0, tol_rb=0.0, maxit=iters)
    dev.sync()
    return r, time.perf_counter() - t0


run(50)
ms = []
for _ in range(3):
    r, t = run(2000)
    ms.append(round(t / r.nits * 1e3, 5))
out["cg_ms_per_iter"] = ms
out["residual"] = r.residual
print(json.dumps(out), flush=True)
dev.close()
