#!/usr/bin/env python3
"""Time lssp_amd_pc_create_dev's general ILUK route -- the symbolic ILU(k) on the
device, a wavefront per row, the values through lssp_amd_iluk_refactor's kernels,
the schedules from the device builder -- against lssp_amd_ilu_create(kind ILUK)
of the same build on the same matrix (the host route: the baseline), on one GPU.

    python tools/pc_create_dev_bench.py [OUT.jsonl] [--reps R] [--only NAME]

Configurations: thermal-like ILU(0); the 7-pt stencil 128^3 at level 2; a 64^3
7-pt box with holes (every 17th row lacks its r + 1 and r - nx entries) at level
1.  Each configuration runs in two child processes of its own, each under its
own time limit, and the run stops at the first failure:
  1. the timings: one untimed warm-up, then R repetitions (default 5) of each
     create, the handle destroyed in between; wall-clock around the synchronous
     call; median, minimum, maximum; one apply of each handle and the
     lssp_amd_ilu_info counts compared bit for bit;
  2. the device create's phases, with LSSP_AMD_SETUP_TIMES=1, where the library
     drains the stream after each phase (the last of two creates).
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

CONFIGS = {"thermal-l0": 0, "poisson128-l2": 2, "holed64-l1": 1}
LIMIT_S = 420  # per child process


def take(argv, flag, conv, default):
    if flag in argv:
        k = argv.index(flag)
        v = conv(argv[k + 1])
        del argv[k:k + 2]
        return v
    return default


def matrix(name):
    """(Ap, Aj, Ax), rows column-sorted, each with its diagonal"""
    import numpy as np
    import lssp_amd
    if name == "thermal-l0":
        from lssp_amd.synthetic import thermal_like
        Ap, Aj, Ax = thermal_like()
    elif name == "poisson128-l2":
        Ap, Aj, Ax = lssp_amd.poisson(3, 128)
    else:
        N = 64
        Ap, Aj, Ax = lssp_amd.poisson(3, N)
        row = np.repeat(np.arange(Ap.size - 1), np.diff(Ap))
        drop = (row % 17 == 16) & ((Aj == row + 1) | (Aj == row - N))
        keep = ~drop
        Ap = np.concatenate(([0], np.cumsum(np.bincount(row[keep], minlength=Ap.size - 1)))).astype(np.int32)
        Aj, Ax = Aj[keep], Ax[keep]
    Ap, Aj, Ax = np.asarray(Ap, np.int32), np.asarray(Aj, np.int32), np.asarray(Ax, np.float64)
    row = np.repeat(np.arange(Ap.size - 1), np.diff(Ap))
    order = np.lexsort((Aj, row))  # both creates get the sorted rows
    return Ap, np.ascontiguousarray(Aj[order]), np.ascontiguousarray(Ax[order])


def child_times(name, reps):
    import numpy as np
    import lssp_amd
    level = CONFIGS[name]
    Ap, Aj, Ax = matrix(name)
    n, nnz = Ap.size - 1, Aj.size
    dev = lssp_amd.Device(0)

    def emit(op, ms, **kw):
        rec = {"config": name, "op": op, "n": n, "nnz": nnz, "level": level, "ms": round(ms, 3), "timer": "wall"}
        rec.update(kw)
        print(json.dumps(rec), flush=True)

    def wall(fn):
        dev.sync()
        t0 = time.perf_counter()
        r = fn()
        dev.sync()
        return (time.perf_counter() - t0) * 1e3, r

    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    makers = {"ilu_create(ILUK)": lambda: lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=level),
              "pc_create_dev": lambda: lssp_amd.DILU.pc_create_dev(dev, A, level=level)}
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
    emit("device create vs host create", med["pc_create_dev"],
         host_over_dev=round(med["ilu_create(ILUK)"] / med["pc_create_dev"], 2),
         slowest_dev_below_fastest_host=bool(hi["pc_create_dev"] < lo["ilu_create(ILUK)"]))
    Mh, Md = makers["ilu_create(ILUK)"](), makers["pc_create_dev"]()
    rhs = dev.vec(n, np.random.default_rng(1).uniform(-1, 1, n))
    x, y = dev.vec(n), dev.vec(n)
    Mh.apply(x, rhs)
    Md.apply(y, rhs)
    same = bool(np.array_equal(x.download(), y.download(), equal_nan=True))
    info = bool((Mh.n, Mh.nnzL, Mh.nnzU, Mh.levelsL, Mh.levelsU) == (Md.n, Md.nnzL, Md.nnzU, Md.levelsL, Md.levelsU))
    emit("pc_create_dev == ilu_create", 0.0, bitwise=same and info, apply=same, info=info, nnzL=Md.nnzL, nnzU=Md.nnzU,
         levelsL=Md.levelsL, levelsU=Md.levelsU, layout_dev=list(Md.sweep_layout()), layout_host=list(Mh.sweep_layout()))
    dev.close()
    if not (same and info):
        raise SystemExit("the device-made handle differs from the host-made one")


def child_phases(name):
    """LSSP_AMD_SETUP_TIMES=1: two device creates; the library prints each phase to stderr"""
    import lssp_amd
    Ap, Aj, Ax = matrix(name)
    dev = lssp_amd.Device(0)
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    for _ in range(2):
        print("lssp_amd pc_create_dev: -- create --", file=sys.stderr, flush=True)
        lssp_amd.DILU.pc_create_dev(dev, A, level=CONFIGS[name]).close()
    dev.close()


def main():
    argv = list(sys.argv)
    reps = take(argv, "--reps", int, 5)
    only = take(argv, "--only", str, None)
    child = take(argv, "--child", str, None)
    if child == "times":
        return child_times(argv[1], reps)
    if child == "phases":
        return child_phases(argv[1])
    out = open(argv[1], "a") if len(argv) > 1 else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    if not os.path.exists(os.path.join(ROOT, "lssp_amd", "lib", "liblssp_amd.so")):
        subprocess.run(["make", "-C", os.path.join(ROOT, "lssp_amd", "csrc"), "-j16"], check=True, timeout=3000)
    me = os.path.abspath(__file__)
    for name in CONFIGS:
        if only and name != only:
            continue
        q = subprocess.run([sys.executable, me, name, "--child", "times", "--reps", str(reps)], stdout=subprocess.PIPE,
                           text=True, timeout=LIMIT_S)
        for line in q.stdout.splitlines():
            emit(line)
        if q.returncode != 0:
            raise SystemExit("%s: the timing run failed (status %d)" % (name, q.returncode))
        env = dict(os.environ, LSSP_AMD_SETUP_TIMES="1")
        q = subprocess.run([sys.executable, me, name, "--child", "phases"], env=env, stderr=subprocess.PIPE,
                           stdout=subprocess.DEVNULL, text=True, timeout=LIMIT_S)
        if q.returncode != 0:
            print(q.stderr[-2000:], file=sys.stderr)
            raise SystemExit("%s: the phase run failed (status %d)" % (name, q.returncode))
        last = q.stderr.rsplit("-- create --", 1)[-1]  # the second create's lines
        ph = {}
        for phase, sec in re.findall(r"^lssp_amd (?:pc_create_dev|create_dev|iluk_create_dev): (.*?)[ \t]+([0-9.]+) s$",
                                     last, re.M):
            ph[phase] = round(ph.get(phase, 0.0) + float(sec) * 1e3, 3)
        top = max(ph, key=ph.get) if ph else None
        emit(json.dumps({"config": name, "op": "pc_create_dev phases (second of 2)", "ms": round(sum(ph.values()), 3),
                         "phases_ms": ph, "dominant": top}))


if __name__ == "__main__":
    main()
