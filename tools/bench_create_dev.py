#!/usr/bin/env python3
"""Time lssp_amd_ilu_create_dev (the tiled line-sweep ILU(0) made from a matrix
handle on the device) against lssp_amd_ilu_create (the same handle made from
host arrays) on 7-pt Poisson N^3 (default 216, BASELINE's matrix), in one
process.

    python tools/bench_create_dev.py [N] [OUT.jsonl]

Both calls are synchronous (they return when the stream has finished), so all
times are wall-clock around the call.  Each is run five times, the handle
destroyed between repetitions; the median is reported.  Prints (and writes to
OUT.jsonl, when given) one JSON line per item: ilu_create, ilu_create_dev, the
ratio, the comparison with the recorded baselines (profiles/refactor_bench_216.jsonl:
ilu_create and the first ilu_refactor with its host plan build), one apply of
each handle compared bit for bit, and -- from a second process run with
LSSP_AMD_SETUP_TIMES=1, where the library drains the stream after each phase --
the device create's phases.
"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 5
PHASES = ("pattern check", "plan / levels", "numeric ILU(0)", "allocation + zeroing", "coefficient streams")
# the parent commit's records at 216^3 (profiles/refactor_bench_216.jsonl)
BASE_216 = {"ilu_create": 1272.0, "ilu_refactor(first: plan build included)": 188.23}


def phases(N):
    """child process (LSSP_AMD_SETUP_TIMES=1): three device creates; the library prints each
    phase to stderr"""
    import lssp_amd
    Ap, Aj, Ax = lssp_amd.poisson(3, N)
    dev = lssp_amd.Device(0)
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    for _ in range(3):
        lssp_amd.DILU.create_dev(dev, A).close()
    dev.close()


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 216
    if len(sys.argv) > 2 and sys.argv[2] == "--phases":
        return phases(N)
    out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
    import numpy as np
    import lssp_amd
    Ap, Aj, Ax = lssp_amd.poisson(3, N)
    n, nnz = Ap.size - 1, Aj.size
    dev = lssp_amd.Device(0)

    def emit(op, ms, **kw):
        rec = {"op": op, "N": N, "n": n, "nnz": nnz, "ms": round(ms, 3), "timer": "wall"}
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
    makers = {"ilu_create": lambda: lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0),
              "ilu_create_dev": lambda: lssp_amd.DILU.create_dev(dev, A, kind=lssp_amd.ILUK, level=0)}
    med = {}
    for name, make in makers.items():
        make().close()  # first-use costs (module load, allocator) outside the timings
        ts = []
        for _ in range(REPS):
            t, M = wall(make)
            assert M.sweep_layout() == (1, 16, 8), M.sweep_layout()
            ts.append(t)
            M.close()
        med[name] = statistics.median(ts)
        emit(name, med[name], ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), reps=REPS)
    rec = {"ilu_create_over_create_dev": round(med["ilu_create"] / med["ilu_create_dev"], 1),
           "create_dev_faster": bool(med["ilu_create_dev"] < med["ilu_create"])}
    if N == 216:
        first = BASE_216["ilu_refactor(first: plan build included)"]
        rec.update(recorded_ilu_create_ms=BASE_216["ilu_create"], recorded_first_refactor_ms=first,
                   below_recorded_first_refactor=bool(med["ilu_create_dev"] < first))
    emit("device create vs host create", med["ilu_create_dev"], **rec)

    # one apply of each handle, bit for bit (and the counts lssp_amd_ilu_info reports)
    Mh, Md = makers["ilu_create"](), makers["ilu_create_dev"]()
    rhs = dev.vec(n, np.random.default_rng(1).uniform(-1, 1, n))
    x, y = dev.vec(n), dev.vec(n)
    Mh.apply(x, rhs)
    Md.apply(y, rhs)
    same = bool(np.array_equal(x.download(), y.download()))
    info = bool((Mh.n, Mh.nnzL, Mh.nnzU, Mh.levelsL, Mh.levelsU) == (Md.n, Md.nnzL, Md.nnzU, Md.levelsL, Md.levelsU))
    emit("create_dev == create", 0.0, bitwise=same and info, apply=same, info=info)
    dev.close()

    # the device create's phases, from a process of their own
    env = dict(os.environ, LSSP_AMD_SETUP_TIMES="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(N), "--phases"], env=env,
                       stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, timeout=600)
    seen = {}
    for name, sec in re.findall(r"^lssp_amd create_dev: (.*?)[ \t]+([0-9.]+) s$", p.stderr, re.M):
        seen.setdefault(name, []).append(float(sec) * 1e3)
    if p.returncode == 0 and all(k in seen for k in PHASES):
        last = {k: round(seen[k][-1], 3) for k in PHASES}
        emit("ilu_create_dev phases (last of 3)", sum(last.values()), phases_ms=last)
    else:
        print(p.stderr[-2000:], file=sys.stderr)
        raise SystemExit("the phase run failed")
    if not (same and info):
        raise SystemExit("the device-made handle differs from the host-made one")


if __name__ == "__main__":
    main()
