#!/usr/bin/env python3
"""Time the device creates (lssp_amd_ilu_create_dev: the tiled line-sweep ILU(0);
lssp_amd_iluk_create_dev at level 1: the skewed line-sweep ILU(1)), which make the
handle from a matrix handle on the device, against lssp_amd_ilu_create (the same
handle made from host arrays) on 7-pt Poisson N^3 (default 216, BASELINE's
matrix), in one process.

    python tools/bench_create_dev.py [N] [OUT.jsonl] [--level 1]

All calls are synchronous (they return when the stream has finished), so all
times are wall-clock around the call.  Each is run five times after one untimed
warm-up, the handle destroyed between repetitions; the median and the range are
reported.  Prints (and writes to OUT.jsonl, when given) one JSON line per item:
the host create, the device create, the ratio (level 0: the comparison with the
recorded baselines, profiles/refactor_bench_216.jsonl; level 1: whether the
device create's slowest repetition is below the host create's fastest, and
lssp_amd_iluk_refactor on the device-made handle), one apply of each handle and
the lssp_amd_ilu_info counts compared bit for bit, and -- from a second process
run with LSSP_AMD_SETUP_TIMES=1, where the library drains the stream after each
phase -- the device create's phases.
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
PHASES = {0: ("pattern check", "plan / levels", "numeric ILU(0)", "allocation + zeroing", "coefficient streams"),
          1: ("pattern check", "F pattern", "levels", "scatter", "numeric", "allocation", "refill")}
PHASE_TAG = {0: "create_dev", 1: "iluk_create_dev"}
LAYOUT = {0: (1, 16, 8), 1: (2, 16, 8)}
# the parent commit's records at 216^3 (profiles/refactor_bench_216.jsonl)
BASE_216 = {"ilu_create": 1272.0, "ilu_refactor(first: plan build included)": 188.23}
# ... at level 1 (profiles/iluk_refactor_bench.jsonl)
BASE_216_L1 = {"ilu_create": 4314.0, "iluk_refactor": 96.0}


def phases(N, level):
    """child process (LSSP_AMD_SETUP_TIMES=1): three device creates; the library prints each
    phase to stderr"""
    import lssp_amd
    Ap, Aj, Ax = lssp_amd.poisson(3, N)
    dev = lssp_amd.Device(0)
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    for _ in range(3):
        (lssp_amd.DILU.iluk_create_dev(dev, A, level=1) if level else lssp_amd.DILU.create_dev(dev, A)).close()
    dev.close()


def main():
    argv = list(sys.argv)
    level = 0
    if "--level" in argv:
        k = argv.index("--level")
        level = int(argv[k + 1])
        del argv[k:k + 2]
    assert level in (0, 1)
    N = int(argv[1]) if len(argv) > 1 else 216
    if len(argv) > 2 and argv[2] == "--phases":
        return phases(N, level)
    out = open(argv[2], "w") if len(argv) > 2 else None
    import numpy as np
    import lssp_amd
    Ap, Aj, Ax = lssp_amd.poisson(3, N)
    n, nnz = Ap.size - 1, Aj.size
    dev = lssp_amd.Device(0)

    def emit(op, ms, **kw):
        rec = {"op": op, "N": N, "n": n, "nnz": nnz, "level": level, "ms": round(ms, 3), "timer": "wall"}
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
    dev_name = "iluk_create_dev" if level else "ilu_create_dev"
    makers = {"ilu_create": lambda: lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=level),
              dev_name: (lambda: lssp_amd.DILU.iluk_create_dev(dev, A, kind=lssp_amd.ILUK, level=1)) if level else
                        (lambda: lssp_amd.DILU.create_dev(dev, A, kind=lssp_amd.ILUK, level=0))}
    med, lo, hi = {}, {}, {}
    for name, make in makers.items():
        make().close()  # first-use costs (module load, allocator) outside the timings
        ts = []
        for _ in range(REPS):
            t, M = wall(make)
            assert M.sweep_layout() == LAYOUT[level], M.sweep_layout()
            ts.append(t)
            M.close()
        med[name], lo[name], hi[name] = statistics.median(ts), min(ts), max(ts)
        emit(name, med[name], ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), reps=REPS)
    rec = {"ilu_create_over_create_dev": round(med["ilu_create"] / med[dev_name], 1),
           "create_dev_faster": bool(med[dev_name] < med["ilu_create"]),
           "slowest_dev_below_fastest_host": bool(hi[dev_name] < lo["ilu_create"])}
    if N == 216 and level == 0:
        first = BASE_216["ilu_refactor(first: plan build included)"]
        rec.update(recorded_ilu_create_ms=BASE_216["ilu_create"], recorded_first_refactor_ms=first,
                   below_recorded_first_refactor=bool(med[dev_name] < first))
    if N == 216 and level == 1:
        rec.update(recorded_ilu_create_ms=BASE_216_L1["ilu_create"], recorded_refactor_ms=BASE_216_L1["iluk_refactor"])
    emit("device create vs host create", med[dev_name], **rec)
    if level:  # lssp_amd_iluk_refactor on the device-made handle (its plan was born with it)
        M = makers[dev_name]()
        ts = []
        for _ in range(REPS):
            t, _ = wall(lambda: M.iluk_refactor(A))
            ts.append(t)
        emit("iluk_refactor on the device-made handle", statistics.median(ts), ms_min=round(min(ts), 3),
             ms_max=round(max(ts), 3), reps=REPS)
        M.close()

    # one apply of each handle, bit for bit (and the counts lssp_amd_ilu_info reports)
    Mh, Md = makers["ilu_create"](), makers[dev_name]()
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
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(N), "--phases", "--level", str(level)], env=env,
                       stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, timeout=600)
    seen = {}
    for name, sec in re.findall(r"^lssp_amd %s: (.*?)[ \t]+([0-9.]+) s$" % PHASE_TAG[level], p.stderr, re.M):
        seen.setdefault(name, []).append(float(sec) * 1e3)
    if p.returncode == 0 and all(k in seen for k in PHASES[level]):
        last = {k: round(seen[k][-1], 3) for k in PHASES[level]}
        emit(dev_name + " phases (last of 3)", sum(last.values()), phases_ms=last)
    else:
        print(p.stderr[-2000:], file=sys.stderr)
        raise SystemExit("the phase run failed")
    if not (same and info):
        raise SystemExit("the device-made handle differs from the host-made one")


if __name__ == "__main__":
    main()
