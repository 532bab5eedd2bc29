"""Wall time of DMat(...): the 7-pt 216^3 grid (all three layers coded) and a matrix the offset
layer refuses (2 M rows, 5 random columns each: more than 255 offsets, not windowed)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lssp_amd

dev = lssp_amd.Device(0)
warm = lssp_amd.DMat(dev, *lssp_amd.poisson(3, 16))
warm.close()


def timed(Ap, Aj, Ax, **kw):
    ts = []
    for _ in range(3):
        dev.sync()
        t0 = time.perf_counter()
        A = lssp_amd.DMat(dev, Ap, Aj, Ax, **kw)
        dev.sync()
        ts.append(round(time.perf_counter() - t0, 4))
        info = (A.ndiag, A.rowcodes, A.valcodes, bool(A.windowed), A.device_bytes)
        A.close()
    return {"seconds": ts, "ndiag,rowcodes,valcodes,windowed,bytes": info}


out = {"poisson216": timed(*lssp_amd.poisson(3, 216))}
nr, k = 2_000_000, 5
rng = np.random.default_rng(4)
Ap = np.arange(0, (nr + 1) * k, k, dtype=np.int32)
Aj = np.sort(rng.integers(0, nr, (nr, k)).astype(np.int32), axis=1).reshape(-1)
out["refused_2M_x5"] = timed(Ap, Aj, rng.uniform(-1, 1, nr * k))
print(json.dumps(out), flush=True)
dev.close()
