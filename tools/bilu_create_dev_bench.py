#!/usr/bin/env python3
"""Time lssp_amd_bilu_create_dev -- block graph, symbolic block ILU(k), numeric
factorization, expansion and both packet schedules on the device -- against
lssp_amd_bilu_create of the same build on the same matrix (the host route: the
baseline), on one GPU: the 7-point block grid of tools/bench_bilu_refactor.py,
N^3 cells (default 64) with bs unknowns per cell (default 4), levels 0 and 1.

    python tools/bilu_create_dev_bench.py [OUT.jsonl] [--N 64] [--bs 4] [--reps R]

Two child processes, each under its own time limit; the run stops at the first
failure:
  1. the timings, both levels in ONE process: per level and create one untimed
     warm-up, then R repetitions (default 5), the handle destroyed in between;
     wall-clock around the synchronous call; median, minimum, maximum; one apply,
     lssp_amd_ilu_get_diag and the lssp_amd_ilu_info counts of both handles
     compared bit for bit at that size;
  2. the device create's phases, with LSSP_AMD_SETUP_TIMES=1, where the library
     drains the stream after each phase (the last of two creates per level).
One JSON line per item is printed and appended to OUT.jsonl when given.  A device
create slower than the host create is reported as it is, with its dominant phase.
"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEVELS = (0, 1)
LIMIT_S = 540  # per child process


def take(argv, flag, conv, default):
    if flag in argv:
        k = argv.index(flag)
        v = conv(argv[k + 1])
        del argv[k:k + 2]
        return v
    return default


def child_times(N, bs, reps):
    import numpy as np
    import lssp_amd
    from bench_bilu_refactor import block_grid7
    Ap, Aj, Ax = block_grid7(N, bs, 64)
    n, nnz = Ap.size - 1, Aj.size
    dev = lssp_amd.Device(0)
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    ok = True

    def wall(fn):
        dev.sync()
        t0 = time.perf_counter()
        r = fn()
        dev.sync()
        return (time.perf_counter() - t0) * 1e3, r

    for level in LEVELS:
        def emit(op, ms, **kw):
            rec = {"config": "grid%d^3 x %d" % (N, bs), "op": op, "n": n, "nnz": nnz, "bs": bs, "level": level,
                   "ms": round(ms, 3), "timer": "wall"}
            rec.update(kw)
            print(json.dumps(rec), flush=True)

        makers = {"bilu_create": lambda: lssp_amd.DILU.bilu(dev, Ap, Aj, Ax, bs, level=level),
                  "bilu_create_dev": lambda: lssp_amd.DILU.bilu_create_dev(dev, A, bs, level=level)}
        med, lo, hi = {}, {}, {}
        for op, make in makers.items():
            make().close()  # first-use costs (module load, allocator) outside the timings
            ts = []
            for _ in range(reps):
                t, M = wall(make)
                ts.append(t)
                M.close()
            med[op], lo[op], hi[op] = statistics.median(ts), min(ts), max(ts)
            emit(op, med[op], ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), reps=reps)
        emit("device create vs host create", med["bilu_create_dev"],
             host_over_dev=round(med["bilu_create"] / med["bilu_create_dev"], 2),
             slowest_dev_below_fastest_host=bool(hi["bilu_create_dev"] < lo["bilu_create"]))
        Mh, Md = makers["bilu_create"](), makers["bilu_create_dev"]()
        rhs = dev.vec(n, np.random.default_rng(1).uniform(-1, 1, n))
        x, y = dev.vec(n), dev.vec(n)
        Mh.apply(x, rhs)
        Md.apply(y, rhs)
        same = bool(np.array_equal(x.download(), y.download()))
        diag = bool(np.array_equal(Mh.diag()[1], Md.diag()[1]))
        info = bool((Mh.n, Mh.nnzL, Mh.nnzU, Mh.levelsL, Mh.levelsU)
                    == (Md.n, Md.nnzL, Md.nnzU, Md.levelsL, Md.levelsU))
        emit("bilu_create_dev == bilu_create", 0.0, bitwise=same and diag and info, apply=same, get_diag=diag,
             info=info, nnzL=Md.nnzL, nnzU=Md.nnzU, levelsL=Md.levelsL, levelsU=Md.levelsU,
             origin=[Md.schedule(0)["origin"], Md.schedule(1)["origin"]])
        ok = ok and same and diag and info
        Mh.close()
        Md.close()
    dev.close()
    if not ok:
        raise SystemExit("the device-made handle differs from the host-made one")


def child_phases(N, bs):
    """LSSP_AMD_SETUP_TIMES=1: two device creates per level; the library prints each phase to stderr"""
    import lssp_amd
    from bench_bilu_refactor import block_grid7
    Ap, Aj, Ax = block_grid7(N, bs, 64)
    dev = lssp_amd.Device(0)
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    for level in LEVELS:
        for _ in range(2):
            print("lssp_amd bilu_create_dev: -- create level %d --" % level, file=sys.stderr, flush=True)
            lssp_amd.DILU.bilu_create_dev(dev, A, bs, level=level).close()
    dev.close()


def main():
    argv = list(sys.argv)
    reps = take(argv, "--reps", int, 5)
    N = take(argv, "--N", int, 64)
    bs = take(argv, "--bs", int, 4)
    child = take(argv, "--child", str, None)
    if child == "times":
        return child_times(N, bs, reps)
    if child == "phases":
        return child_phases(N, bs)
    out = open(argv[1], "a") if len(argv) > 1 else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    if not os.path.exists(os.path.join(ROOT, "lssp_amd", "lib", "liblssp_amd.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lssp_amd", "csrc"), "-j16"], check=True, timeout=3000)
    me = os.path.abspath(__file__)
    shape = ["--N", str(N), "--bs", str(bs)]
    q = subprocess.run([sys.executable, me, "--child", "times", "--reps", str(reps)] + shape, stdout=subprocess.PIPE,
                       text=True, timeout=LIMIT_S)
    for line in q.stdout.splitlines():
        emit(line)
    if q.returncode != 0:
        raise SystemExit("the timing run failed (status %d)" % q.returncode)
    env = dict(os.environ, LSSP_AMD_SETUP_TIMES="1")
    q = subprocess.run([sys.executable, me, "--child", "phases"] + shape, env=env, stderr=subprocess.PIPE,
                       stdout=subprocess.DEVNULL, text=True, timeout=LIMIT_S)
    if q.returncode != 0:
        print(q.stderr[-2000:], file=sys.stderr)
        raise SystemExit("the phase run failed (status %d)" % q.returncode)
    for level in LEVELS:
        last = q.stderr.rsplit("-- create level %d --" % level, 1)[-1].split("-- create level", 1)[0]
        ph = {}
        for phase, sec in re.findall(r"^lssp_amd bilu_create_dev: (.*?)[ \t]+([0-9.]+) s$", last, re.M):
            ph[phase] = round(ph.get(phase, 0.0) + float(sec) * 1e3, 3)
        top = max(ph, key=ph.get) if ph else None
        emit(json.dumps({"config": "grid%d^3 x %d" % (N, bs), "op": "bilu_create_dev phases (second of 2)",
                         "level": level, "ms": round(sum(ph.values()), 3), "phases_ms": ph, "dominant": top}))


if __name__ == "__main__":
    main()
