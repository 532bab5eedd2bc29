#!/usr/bin/env python3
"""Time the device format conversions (lssp_amd.convert) on 7-pt Poisson N^3
(default 216, BASELINE's matrix) with HIP events on the library's stream.

    python tools/bench_convert.py [N] [bs] [conv|assemble|all]

Prints one JSON line per conversion: milliseconds per call (mean of reps, the
host-side size query and output allocation included in the call as a user
sees it) and the algorithmic bytes (each input read once, each output written
once) divided by that time.  The assemble leg times the assembly calls
(is_sorted, the device column sort, adjust_zero_diag, get_block_diag) the same
way, and DMat.from_device against DMat(...) (lssp_amd_mat_upload of the same
arrays) by the wall clock in the same process.
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 216
    bs = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    leg = sys.argv[3] if len(sys.argv) > 3 else "all"
    import torch
    import lssp_amd
    from lssp_amd import convert as C
    dev = lssp_amd.Device(0)
    Ap, Aj, Ax = lssp_amd.poisson(3, N)
    n, nnz = Ap.size - 1, Aj.size
    dAp, dAj, dAx = dev.idx(n + 1, Ap), dev.idx(nnz, Aj), dev.vec(nnz, Ax)
    s = torch.cuda.ExternalStream(dev.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timeit(fn, reps=5):
        out = fn()
        for a in out if isinstance(out, tuple) else ():
            if hasattr(a, "free"):
                a.free()
        total = 0.0
        for _ in range(reps):
            e0.record(s)
            out = fn()
            e1.record(s)
            e1.synchronize()
            total += e0.elapsed_time(e1)
            for a in out:
                if hasattr(a, "free"):
                    a.free()
        return total / reps

    Ci, Cj, Cx = C.csr_to_coo(dev, n, nnz, dAp, dAj, dAx)
    m, Bp, Bj, Bx = C.csr_to_bcsr(dev, n, nnz, bs, dAp, dAj, dAx)
    nb = n // bs
    rows = [
        ("csr_to_coo", lambda: C.csr_to_coo(dev, n, nnz, dAp, dAj, dAx), 4 * (n + 1) + 4 * nnz + 24 * nnz),
        ("coo_to_csr", lambda: C.coo_to_csr(dev, n, nnz, Ci, Cj, Cx), 16 * nnz + 4 * (n + 1) + 12 * nnz),
        ("transpose", lambda: C.transpose(dev, n, n, nnz, dAp, dAj, dAx), 2 * (4 * (n + 1) + 12 * nnz)),
        ("csr_to_bcsr", lambda: C.csr_to_bcsr(dev, n, nnz, bs, dAp, dAj, dAx),
         4 * (n + 1) + 12 * nnz + 4 * (nb + 1) + 4 * m + 8 * m * bs * bs),
        ("bcsr_to_csr", lambda: C.bcsr_to_csr(dev, nb, nb, bs, m, Bp, Bj, Bx),
         4 * (nb + 1) + 4 * m + 8 * m * bs * bs + 4 * (n + 1) + 12 * nnz),
    ]
    if leg in ("conv", "all"):
        for name, fn, byts in rows:
            ms = timeit(fn)
            print(json.dumps({"op": name, "N": N, "n": n, "nnz": nnz, "bs": bs if "bcsr" in name else None,
                              "ms": round(ms, 3), "alg_bytes": byts, "alg_GBps": round(byts / ms / 1e6, 1)}),
                  flush=True)
    for a in (Ci, Cj, Cx, Bp, Bj, Bx):
        a.free()
    if leg in ("assemble", "all"):
        assemble_leg(dev, lssp_amd, C, timeit, N, Ap, Aj, Ax, dAp, dAj, dAx)
    dev.close()


def assemble_leg(dev, lssp_amd, C, timeit, N, Ap, Aj, Ax, dAp, dAj, dAx):
    """the assembly calls (is_sorted, sort_columns, adjust_zero_diag, get_block_diag,
    DMat.from_device) on the same matrix; from_device against DMat(...) = mat_upload of the
    same arrays, both wall-timed in this process"""
    import time
    import numpy as np
    n, nnz = Ap.size - 1, Aj.size
    csr = 4 * (n + 1) + 12 * nnz

    def emit(op, ms, byts=None, **kw):
        rec = {"op": op, "N": N, "n": n, "nnz": nnz, "ms": round(ms, 3)}
        if byts:
            rec.update(alg_bytes=byts, alg_GBps=round(byts / ms / 1e6, 1))
        rec.update(kw)
        print(json.dumps(rec), flush=True)

    emit("csr_is_sorted", timeit(lambda: (C.csr_is_sorted(dev, n, nnz, dAp, dAj),)), 4 * (n + 1) + 4 * nnz)
    # every row reversed: each one is out of order and gets sorted (a sorted input is only checked)
    rows = np.repeat(np.arange(n), np.diff(Ap))
    rev = (Ap[rows] + Ap[rows + 1] - 1 - np.arange(nnz)).astype(np.int64)
    rj, rx = Aj[rev], Ax[rev]
    wj, wx = dev.idx(nnz), dev.vec(nnz)
    import torch
    s = torch.cuda.ExternalStream(dev.stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def sort_reversed():
        wj.upload(rj)               # the sort is in place: a fresh input, outside the timed call
        wx.upload(rx)
        e0.record(s)
        C.sort_columns(dev, n, n, nnz, dAp, wj, wx)
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    sort_reversed()
    emit("sort_columns_dev(all rows reversed)", sum(sort_reversed() for _ in range(3)) / 3, 2 * csr)
    assert np.array_equal(wj.download(), Aj) and np.array_equal(wx.download(), Ax)
    emit("sort_columns_dev(sorted input)", timeit(lambda: (C.sort_columns(dev, n, n, nnz, dAp, dAj, dAx),)), csr)
    for a in (wj, wx):
        a.free()
    emit("adjust_zero_diag", timeit(lambda: C.adjust_zero_diag(dev, n, nnz, dAp, dAj, dAx, 1e-8)), 2 * csr)
    emit("get_block_diag(blk 6)", timeit(lambda: C.get_block_diag(dev, n, nnz, dAp, dAj, dAx, 6)), 2 * csr)

    def wall(make, reps=3):
        make().close()
        t = []
        for _ in range(reps):
            dev.sync()
            t0 = time.perf_counter()
            A = make()
            dev.sync()
            t.append((time.perf_counter() - t0) * 1e3)
            layout = (A.ndiag, A.windowed, A.device_bytes)
            A.close()
        return min(t), sum(t) / reps, layout

    fd_min, fd_mean, fd_layout = wall(lambda: lssp_amd.DMat.from_device(dev, n, n, nnz, dAp, dAj, dAx))
    up_min, up_mean, up_layout = wall(lambda: lssp_amd.DMat(dev, Ap, Aj, Ax))
    assert fd_layout == up_layout, (fd_layout, up_layout)
    emit("mat_from_device", fd_mean, ms_min=round(fd_min, 3), ndiag=fd_layout[0], timer="wall")
    emit("mat_upload", up_mean, ms_min=round(up_min, 3), ndiag=up_layout[0], timer="wall")
    emit("mat_from_device vs mat_upload", fd_mean, speedup=round(up_mean / fd_mean, 2),
         from_device_not_slower=bool(fd_mean <= up_mean and fd_min <= up_min))


if __name__ == "__main__":
    main()
