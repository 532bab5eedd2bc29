#!/usr/bin/env python3
"""Time lssp_amd_ilut_create_dev -- ILUT(tol, p) factored on the device from a
matrix handle, a wavefront per row -- against lssp_amd_ilu_create(kind ILUT), the
same handle made from host arrays by the reference's row-sequential loop, on the
7-pt stencil N^3 (default 128), in one process.

    python tools/bench_ilut_create_dev.py [N] [OUT.jsonl] [--random SEED] [--tol T] [--p P] [--reps R]

Default: the constant-coefficient Poisson matrix at ILUT(1e-4, 20), BASELINE's
config 3.  --random SEED keeps the pattern and draws the off-diagonal values from
[-1, 1) and the diagonal from [1, 2): no dominance, long working rows and a long
chain of dependent rows, where a per-row latency shows.

All calls are synchronous (they return when the stream has finished), so all
times are wall-clock around the call.  Each is run five times after one untimed
warm-up, the handle destroyed between repetitions; the median and the range are
reported.  Prints (and writes to OUT.jsonl, when given) one JSON line per item:
the host create, the device create, whether the device create's slowest
repetition is below the host create's fastest, one apply of each handle and the
lssp_amd_ilu_info counts compared bit for bit, and -- from a second process run
with LSSP_AMD_SETUP_TIMES=1, where the library drains the stream after each phase
-- the device create's phases (check, numeric, compaction, download, schedules).
"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = ("check", "numeric", "compaction", "download", "schedules")


def take(argv, flag, conv, default):
    if flag in argv:
        k = argv.index(flag)
        v = conv(argv[k + 1])
        del argv[k:k + 2]
        return v
    return default


def matrix(N, seed):
    import numpy as np
    import lssp_amd
    Ap, Aj, Ax = lssp_amd.poisson(3, N)
    if seed is not None:
        rng = np.random.default_rng(seed)
        diag = Aj == np.repeat(np.arange(Ap.size - 1, dtype=Aj.dtype), np.diff(Ap))
        Ax = np.where(diag, rng.uniform(1, 2, Aj.size), rng.uniform(-1, 1, Aj.size))
    return Ap, Aj, Ax


def phases(N, seed, tol, p):
    """child process (LSSP_AMD_SETUP_TIMES=1): two device creates; the library prints each phase to stderr"""
    import lssp_amd
    Ap, Aj, Ax = matrix(N, seed)
    dev = lssp_amd.Device(0)
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    for _ in range(2):
        lssp_amd.DILU.ilut_create_dev(dev, A, tol=tol, p=p).close()
    dev.close()


def main():
    argv = list(sys.argv)
    seed = take(argv, "--random", int, None)
    tol = take(argv, "--tol", float, 1e-4)
    p = take(argv, "--p", int, 20)
    reps = take(argv, "--reps", int, 5)
    N = int(argv[1]) if len(argv) > 1 else 128
    if len(argv) > 2 and argv[2] == "--phases":
        return phases(N, seed, tol, p)
    out = open(argv[2], "w") if len(argv) > 2 else None
    import numpy as np
    import lssp_amd
    Ap, Aj, Ax = matrix(N, seed)
    n, nnz = Ap.size - 1, Aj.size
    dev = lssp_amd.Device(0)

    def emit(op, ms, **kw):
        rec = {"op": op, "N": N, "n": n, "nnz": nnz, "tol": tol, "p": p, "values": "poisson" if seed is None else
               "random seed %d" % seed, "ms": round(ms, 3), "timer": "wall"}
        rec.update(kw)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def wall(fn):
        dev.sync()
        t0 = time.perf_counter()
        r = fn()
        dev.sync()
        return (time.perf_counter() - t0) * 1e3, r

    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    makers = {"ilu_create(ILUT)": lambda: lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUT, tol=tol, p=p),
              "ilut_create_dev": lambda: lssp_amd.DILU.ilut_create_dev(dev, A, tol=tol, p=p)}
    med, lo, hi = {}, {}, {}
    for name, make in makers.items():
        make().close()  # first-use costs (module load, allocator) outside the timings
        ts = []
        for _ in range(reps):
            t, M = wall(make)
            ts.append(t)
            M.close()
        med[name], lo[name], hi[name] = statistics.median(ts), min(ts), max(ts)
        emit(name, med[name], ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), reps=reps)
    emit("device create vs host create", med["ilut_create_dev"],
         host_over_dev=round(med["ilu_create(ILUT)"] / med["ilut_create_dev"], 2),
         slowest_dev_below_fastest_host=bool(hi["ilut_create_dev"] < lo["ilu_create(ILUT)"]))

    # one apply of each handle, bit for bit (and the counts lssp_amd_ilu_info reports)
    Mh, Md = makers["ilu_create(ILUT)"](), makers["ilut_create_dev"]()
    rhs = dev.vec(n, np.random.default_rng(1).uniform(-1, 1, n))
    x, y = dev.vec(n), dev.vec(n)
    Mh.apply(x, rhs)
    Md.apply(y, rhs)
    same = bool(np.array_equal(x.download(), y.download(), equal_nan=True))
    info = bool((Mh.n, Mh.nnzL, Mh.nnzU, Mh.levelsL, Mh.levelsU) == (Md.n, Md.nnzL, Md.nnzU, Md.levelsL, Md.levelsU))
    emit("ilut_create_dev == ilu_create", 0.0, bitwise=same and info, apply=same, info=info, nnzL=Md.nnzL,
         nnzU=Md.nnzU, levelsL=Md.levelsL, levelsU=Md.levelsU)
    dev.close()

    # the device create's phases, from a process of their own
    env = dict(os.environ, LSSP_AMD_SETUP_TIMES="1")
    cmd = [sys.executable, os.path.abspath(__file__), str(N), "--phases", "--tol", repr(tol), "--p", str(p)]
    if seed is not None:
        cmd += ["--random", str(seed)]
    q = subprocess.run(cmd, env=env, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, timeout=900)
    seen = {}
    for name, sec in re.findall(r"^lssp_amd ilut_create_dev: (.*?)[ \t]+([0-9.]+) s$", q.stderr, re.M):
        seen.setdefault(name, []).append(float(sec) * 1e3)
    if q.returncode == 0 and all(k in seen for k in PHASES):
        last = {k: round(seen[k][-1], 3) for k in PHASES}
        emit("ilut_create_dev phases (last of 2)", sum(last.values()), phases_ms=last)
        emit("ilut_create_dev numeric phase", last["numeric"])
    else:
        print(q.stderr[-2000:], file=sys.stderr)
        raise SystemExit("the phase run failed")
    if not (same and info):
        raise SystemExit("the device-made handle differs from the host-made one")


if __name__ == "__main__":
    main()
