#!/usr/bin/env python3
"""Time the device route to a rank's distributed matrix and block-Jacobi ILU(0) --
lssp_amd_mat_from_device_dist + lssp_amd_mat_local_block + lssp_amd_pc_create_dev(level 0)
from arrays in HBM -- against the host route of the same build (lssp_amd_mat_upload_dist +
the block cut out with numpy + lssp_amd_ilu_create), a time step on each route (update_values +
local_block_refresh + refactor against the host rebuild), and lssp_amd_mat_upload_dist alone
against a library built from another commit's sources.

    python tools/dist_create_dev_bench.py [OUT.jsonl] [--grid N] [--ranks P] [--reps R]
                                          [--other-lib PATH/liblssp_amd.so]

The P ranks are spawned processes that share device 0 over the host-staged transport (as
bench.py --share-gpu): a rehearsal of the per-rank work, not a scaling measurement.  The
routes alternate inside one session; every timing starts at a barrier, is wall-clock around
the synchronous calls on each rank, and is reported per rank as median, minimum and maximum of
R repetitions (default 5) after one untimed pass.  With --other-lib, upload_dist alone is timed
in 2 R fresh sessions that alternate between the two libraries, one untimed and one timed call
each.  One JSON line per item is printed and appended to OUT.jsonl when given."""
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT_S = 420  # per session


def take(argv, flag, conv, default):
    if flag in argv:
        k = argv.index(flag)
        v = conv(argv[k + 1])
        del argv[k:k + 2]
        return v
    return default


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def rank_main(rank, world, port, what, N, reps, lib, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import ctypes
    import numpy as np
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        if lib:  # another build: the ctypes table is cut down to the calls it exports before the package loads it
            import importlib.util
            spec = importlib.util.spec_from_file_location("lssp_amd._lib", os.path.join(ROOT, "lssp_amd", "_lib.py"))
            tab = sys.modules["lssp_amd._lib"] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(tab)
            tab.LIB_PATH = lib
            probe = ctypes.CDLL(lib, mode=ctypes.RTLD_LOCAL)
            tab.SIGNATURES = {k: v for k, v in tab.SIGNATURES.items() if hasattr(probe, k)}
        import lssp_amd
        from bench import local_block
        from lssp_amd.dist import GlooTransport
        dev = lssp_amd.Device(0)
        dev.comm_init_host(world, rank, GlooTransport())
        n = N ** 3
        blk = (n + world - 1) // world
        r0 = min(rank * blk, n)
        nl = min(blk, n - r0)
        Ap, Aj, Ax = lssp_amd.poisson(3, N, r0, nl)
        nnz = int(Ap[-1])

        def wall(fn):
            dev.barrier()
            t0 = time.perf_counter()
            r = fn()
            dev.sync()
            return (time.perf_counter() - t0) * 1e3, r

        def host_route(ax):
            A = lssp_amd.DMat(dev, Ap, Aj, ax, dist=(n, r0))
            bp, bj, bx = local_block(Ap, Aj, ax, r0, nl)
            return A, None, lssp_amd.DILU.create(dev, bp, bj, bx, kind=lssp_amd.ILUK, level=0)

        ts = {}
        if what == "upload":
            lssp_amd.DMat(dev, Ap, Aj, Ax, dist=(n, r0)).close()
            t, A = wall(lambda: lssp_amd.DMat(dev, Ap, Aj, Ax, dist=(n, r0)))
            ts["upload_dist"] = [t]
            A.close()
        else:
            dAp, dAj, dAx = dev.idx(nl + 1, Ap), dev.idx(nnz, Aj), dev.vec(nnz, Ax)
            Ax2 = Ax * (1.0 + 0.125 * np.cos(np.arange(nnz)))
            dAx2 = dev.vec(nnz, Ax2)

            def dev_route():
                A = lssp_amd.DMat.from_device_dist(dev, n, r0, nl, nnz, dAp, dAj, dAx)
                B = A.local_block()
                return A, B, lssp_amd.DILU.pc_create_dev(dev, B, kind=lssp_amd.ILUK, level=0)

            def dev_step(A, B, M, vals):
                A.update_values(vals)
                B.refresh_block(A)
                M.refactor(B) if M.sweep_layout()[0] == 1 else M.iluk_refactor(B)

            for rep in range(reps + 1):  # the first pass is not kept
                for op, make in (("host create", lambda: host_route(Ax)), ("device create", dev_route)):
                    t, (A, B, M) = wall(make)
                    if op == "device create":
                        t2, _ = wall(lambda: dev_step(A, B, M, dAx2))
                    else:
                        t2, H = wall(lambda: host_route(Ax2))
                        for h in H:
                            if h is not None:
                                h.close()
                    if rep:
                        ts.setdefault(op, []).append(t)
                        ts.setdefault(op.split()[0] + " step", []).append(t2)
                    layout = M.sweep_layout()
                    for h in (M, B, A):
                        if h is not None:
                            h.close()
            ts["layout"] = list(layout)
        parts = [None] * world
        dist.all_gather_object(parts, ts)
        if rank == 0:
            out.put({"nlocal": nl, "nnz_local": nnz, "ranks": parts})
        dev.close()
    finally:
        dist.destroy_process_group()


def session(what, world, N, reps, lib=None):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=rank_main, args=(r, world, port, what, N, reps, lib, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = q.get(timeout=LIMIT_S)
    finally:
        for p in procs:
            p.join(timeout=60)
    if any(p.exitcode != 0 for p in procs):
        raise SystemExit("a rank failed: exit codes %s" % [p.exitcode for p in procs])
    return got


def main():
    argv = list(sys.argv)
    N = take(argv, "--grid", int, 216)
    world = take(argv, "--ranks", int, 2)
    reps = take(argv, "--reps", int, 5)
    other = take(argv, "--other-lib", str, None)
    out = open(argv[1], "a") if len(argv) > 1 else None

    def emit(op, ms, **kw):
        rec = {"grid": N, "ranks": world, "op": op, "timer": "wall, from a barrier", "reps": len(ms),
               "ms": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
        rec.update(kw)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    got = session("routes", world, N, reps)
    for r, ts in enumerate(got["ranks"]):
        for op in ("host create", "device create", "host step", "device step"):
            emit(op, ts[op], rank=r, nlocal=got["nlocal"], sweep_layout=ts["layout"])
    if other:
        runs = {"this build": [[] for _ in range(world)], "other build": [[] for _ in range(world)]}
        for _ in range(reps):
            for name, lib in (("this build", None), ("other build", os.path.abspath(other))):
                g = session("upload", world, N, 1, lib)
                for r, ts in enumerate(g["ranks"]):
                    runs[name][r] += ts["upload_dist"]
        for name, per_rank in runs.items():
            for r, ms in enumerate(per_rank):
                emit("upload_dist alone, " + name, ms, rank=r, runs_ms=[round(v, 3) for v in ms])


if __name__ == "__main__":
    main()
