#!/usr/bin/env python3
"""Time the device schedule builder (lssp_amd/csrc/tri_sched.hip) against the host
builder it reproduces, in one process:

    python tools/bench_from_factors_dev.py [N] [OUT.jsonl] [--tol T] [--p P] [--reps R] [--no-thermal]

1. lssp_amd_ilut_create_dev of the 7-pt Poisson matrix N^3 (default 128) at ILUT(tol, p) (default 1e-4,
   20): the device schedule route against the host schedule route of the same library
   (LSSP_AMD_SCHED_HOST=1: the factors downloaded, the schedules built by tri_bp.cpp -- the call as it was
   before the device builder), and whether the device route's slowest repetition is below the host route's
   fastest.
2. lssp_amd_ilu_from_factors_dev against lssp_amd_ilu_from_factors on those factors (the host call's
   time includes the upload of its schedules, the device call's the device-to-device copies).
3. The same pair on the ILU(0) factors of the thermal-like mesh matrix (lssp_amd.synthetic), an irregular
   pattern.

All calls are synchronous, so all times are wall-clock around the call; each is run R (5) times after one
untimed warm-up, the handle destroyed between repetitions; the median and the range are reported.  Each
pair's schedule headers and one apply are compared bit for bit.  The phases (check, levels, order,
entries, packets, fill per side) come from a second process run with LSSP_AMD_SETUP_TIMES=1, where the
library drains the stream after each phase.  One JSON line per item, also written to OUT.jsonl.
"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def take(argv, flag, conv, default):
    if flag in argv:
        k = argv.index(flag)
        v = conv(argv[k + 1])
        del argv[k:k + 2]
        return v
    return default


def upload(dev, L, U):
    return [dev.idx(L[0].size, L[0]), dev.idx(L[1].size, L[1]), dev.vec(L[2].size, L[2]),
            dev.idx(U[0].size, U[0]), dev.idx(U[1].size, U[1]), dev.vec(U[2].size, U[2])]


def phases(N, tol, p, thermal):
    """child process (LSSP_AMD_SETUP_TIMES=1): two creates of each kind; the library prints each phase to stderr"""
    import lssp_amd
    dev = lssp_amd.Device(0)
    Ap, Aj, Ax = lssp_amd.poisson(3, N)
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    for _ in range(2):
        M = lssp_amd.DILU.ilut_create_dev(dev, A, tol=tol, p=p)
        M.close()
    if thermal:
        from lssp_amd.synthetic import thermal_like
        Ap, Aj, Ax = thermal_like()
        L, U = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0).factors()
        d = upload(dev, L, U)
        for _ in range(2):
            lssp_amd.DILU.from_factors_dev(dev, d[:3], d[3:]).close()
    dev.close()


def main():
    argv = list(sys.argv)
    tol = take(argv, "--tol", float, 1e-4)
    p = take(argv, "--p", int, 20)
    reps = take(argv, "--reps", int, 5)
    thermal = "--no-thermal" not in argv
    argv = [a for a in argv if a != "--no-thermal"]
    N = int(argv[1]) if len(argv) > 1 else 128
    if len(argv) > 2 and argv[2] == "--phases":
        return phases(N, tol, p, thermal)
    out = open(argv[2], "w") if len(argv) > 2 else None
    import numpy as np
    import lssp_amd
    dev = lssp_amd.Device(0)

    def emit(op, case, ms, **kw):
        rec = {"op": op, "case": case, "ms": round(ms, 3), "timer": "wall"}
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

    def pair(case, makers, base, new):
        stat = {}
        for name, make in makers.items():
            make().close()  # first-use costs outside the timings
            ts = []
            for _ in range(reps):
                t, M = wall(make)
                ts.append(t)
                M.close()
            stat[name] = (statistics.median(ts), min(ts), max(ts))
            emit(name, case, stat[name][0], ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), reps=reps)
        emit("%s vs %s" % (new, base), case, stat[new][0], speedup=round(stat[base][0] / stat[new][0], 2),
             slowest_new_below_fastest_base=bool(stat[new][2] < stat[base][1]))
        Mb, Mn = makers[base](), makers[new]()
        n = Mb.n
        rhs = dev.vec(n, np.random.default_rng(1).uniform(-1, 1, n))
        x, y = dev.vec(n), dev.vec(n)
        Mb.apply(x, rhs)
        Mn.apply(y, rhs)
        same = bool(np.array_equal(x.download(), y.download(), equal_nan=True))
        hdr = []
        for M in (Mb, Mn):
            h = np.zeros((2, 12), np.int32)
            for w in (0, 1):
                dev.L.lssp_amd_ilu_get_schedule(M.h, w, h[w].ctypes.data, None, None, None, None, None, None)
            hdr.append(h)
        heads = bool(np.array_equal(hdr[0][:, :11], hdr[1][:, :11]))
        emit("%s == %s" % (new, base), case, 0.0, apply=same, headers=heads, origin=[int(hdr[0][0, 11]), int(hdr[1][0, 11])],
             L=[int(v) for v in hdr[1][0]], U=[int(v) for v in hdr[1][1]])
        if not (same and heads):
            raise SystemExit("the two handles differ")
        return Mb, Mn

    # 1: ilut_create_dev, host schedule route against device schedule route
    Ap, Aj, Ax = lssp_amd.poisson(3, N)
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    case = "7-pt %d^3 ILUT(%g, %d)" % (N, tol, p)

    def host_route():
        os.environ["LSSP_AMD_SCHED_HOST"] = "1"
        try:
            return lssp_amd.DILU.ilut_create_dev(dev, A, tol=tol, p=p)
        finally:
            del os.environ["LSSP_AMD_SCHED_HOST"]

    Mb, Mn = pair(case, {"ilut_create_dev (host schedules)": host_route,
                         "ilut_create_dev": lambda: lssp_amd.DILU.ilut_create_dev(dev, A, tol=tol, p=p)},
                  "ilut_create_dev (host schedules)", "ilut_create_dev")
    L, U = Mb.factors()
    for M in (Mb, Mn, A):
        M.close()

    # 2, 3: from_factors_dev against from_factors
    def factors_pair(case, L, U):
        d = upload(dev, L, U)
        Mb, Mn = pair(case, {"ilu_from_factors": lambda: lssp_amd.DILU.from_factors(dev, L, U),
                             "ilu_from_factors_dev": lambda: lssp_amd.DILU.from_factors_dev(dev, d[:3], d[3:])},
                      "ilu_from_factors", "ilu_from_factors_dev")
        for h in (Mb, Mn, *d):
            h.close()

    factors_pair(case, L, U)
    if thermal:
        from lssp_amd.synthetic import thermal_like
        Ap, Aj, Ax = thermal_like()
        L, U = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0).factors()
        factors_pair("thermal-like ILU(0), %d rows" % (Ap.size - 1), L, U)
    dev.close()

    env = dict(os.environ, LSSP_AMD_SETUP_TIMES="1")
    cmd = [sys.executable, os.path.abspath(__file__), str(N), "--phases", "--tol", repr(tol), "--p", str(p)]
    if not thermal:
        cmd.append("--no-thermal")
    q = subprocess.run(cmd, env=env, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, timeout=900)
    if q.returncode != 0:
        print(q.stderr[-2000:], file=sys.stderr)
        raise SystemExit("the phase run failed")
    for tag, case_ in (("ilut_create_dev", case), ("from_factors_dev", "thermal-like ILU(0)")):
        seen = {}
        for name, sec in re.findall(r"^lssp_amd %s: (.*?)[ \t]+([0-9.]+) s$" % tag, q.stderr, re.M):
            seen.setdefault(name, []).append(round(float(sec) * 1e3, 3))
        if seen:
            last = {k: v[-1] for k, v in seen.items()}
            emit("%s phases (last of 2)" % tag, case_, sum(last.values()), phases_ms=last)


if __name__ == "__main__":
    main()
