#!/usr/bin/env python3
"""Time the value refresh (lssp_amd_mat_update_values, lssp_amd_ilu_refactor)
against the assembly it replaces (lssp_amd_mat_upload, lssp_amd_ilu_create) on
7-pt Poisson N^3 (default 216, BASELINE's matrix), in one process.

    python tools/bench_refactor.py [N] [OUT.jsonl]

Every call is synchronous (it returns when the stream has finished), so all
times are wall-clock around the call.  Prints (and appends to OUT.jsonl, when
given) one JSON line per item: mat_upload, ilu_create, mat_update_values, the
first ilu_refactor (its plan build included), the median of five later ones,
the two ratios, and -- from a second process run with LSSP_AMD_SETUP_TIMES=1,
where the library drains the stream after each phase -- the refactor's phases
with the coefficient refill's bytes and rate.  After the timings the refreshed
handles are checked bit for bit against fresh ones.
"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(N):
    import numpy as np
    import lssp_amd
    Ap, Aj, Ax = lssp_amd.poisson(3, N)
    rng = np.random.default_rng(216)
    Ax1 = Ax * rng.uniform(0.9, 1.1, Ax.size)  # new values, same pattern, still diagonally dominant
    return Ap, Aj, Ax, Ax1


def phases(N):
    """child process (LSSP_AMD_SETUP_TIMES=1): create, then three refactors; the library prints
    each phase to stderr"""
    import lssp_amd
    Ap, Aj, Ax, Ax1 = inputs(N)
    dev = lssp_amd.Device(0)
    A = lssp_amd.DMat(dev, Ap, Aj, Ax)
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0)
    A.update_values(dev.vec(Ax1.size, Ax1))
    for _ in range(3):
        M.refactor(A)
    dev.close()


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 216
    if len(sys.argv) > 2 and sys.argv[2] == "--phases":
        return phases(N)
    out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
    import numpy as np
    import lssp_amd
    Ap, Aj, Ax, Ax1 = inputs(N)
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

    lssp_amd.DMat(dev, Ap, Aj, Ax).close()  # first-use costs (module load, allocator) outside the timings
    ups = []
    for _ in range(3):
        t, A = wall(lambda: lssp_amd.DMat(dev, Ap, Aj, Ax))
        ups.append(t)
        A.close()
    t_up, A = wall(lambda: lssp_amd.DMat(dev, Ap, Aj, Ax))
    ups.append(t_up)
    t_up = statistics.median(ups)
    emit("mat_upload", t_up, ms_min=round(min(ups), 3), reps=len(ups))
    t_cr, M = wall(lambda: lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0))
    assert M.sweep_layout() == (1, 16, 8), M.sweep_layout()
    emit("ilu_create", t_cr, setup_seconds=round(M.setup_seconds, 4))

    v = [dev.vec(nnz, Ax1), dev.vec(nnz, Ax)]
    A.update_values(v[0])
    tv = [wall(lambda k=k: A.update_values(v[k % 2]))[0] for k in range(1, 7)]  # ends on Ax1
    t_uv = statistics.median(tv)
    emit("mat_update_values", t_uv, ms_min=round(min(tv), 3), reps=len(tv), alg_bytes=16 * nnz,
         alg_GBps=round(16 * nnz / t_uv / 1e6, 1))
    t_first, _ = wall(lambda: M.refactor(A))
    emit("ilu_refactor(first: plan build included)", t_first)
    tr = []
    for k in range(5):  # alternate the two value sets
        A.update_values(v[(k + 1) % 2])
        tr.append(wall(lambda: M.refactor(A))[0])
    A.update_values(v[0])  # leave both handles on Ax1 for the comparison below
    M.refactor(A)
    t_rf = statistics.median(tr)
    emit("ilu_refactor(median of 5)", t_rf, ms_min=round(min(tr), 3), ms_max=round(max(tr), 3))
    emit("refresh vs assemble", t_rf + t_uv, ilu_create_over_refactor=round(t_cr / t_rf, 1),
         mat_upload_over_update_values=round(t_up / t_uv, 1),
         refactor_faster=bool(t_rf < t_cr), update_values_faster=bool(t_uv < t_up))

    # the refreshed handles against fresh ones, bit for bit
    Af = lssp_amd.DMat(dev, Ap, Aj, Ax1)
    Mf = lssp_amd.DILU.create(dev, Ap, Aj, Ax1, kind=lssp_amd.ILUK, level=0)
    (_, _, Lx), (_, _, Ux) = M.factors()
    (_, _, Lf), (_, _, Uf) = Mf.factors()
    rhs = dev.vec(n, np.random.default_rng(1).uniform(-1, 1, n))
    x, y = dev.vec(n), dev.vec(n)
    M.apply(x, rhs)
    Mf.apply(y, rhs)
    eq = {"factors": bool(np.array_equal(Lx, Lf) and np.array_equal(Ux, Uf)),
          "apply": bool(np.array_equal(x.download(), y.download()))}
    A.mv_mxy(rhs, x)
    Af.mv_mxy(rhs, y)
    eq["product"] = bool(np.array_equal(x.download(), y.download()))
    same = all(eq.values())
    emit("refreshed == fresh", 0.0, bitwise=same, **eq)
    dev.close()

    # the refactor's phases, from a process of their own
    env = dict(os.environ, LSSP_AMD_SETUP_TIMES="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), str(N), "--phases"], env=env,
                       stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, timeout=600)
    seen = {}
    for name, sec in re.findall(r"^lssp_amd refactor: (.*?)[ \t]+([0-9.]+) s$", p.stderr, re.M):
        seen.setdefault(name, []).append(float(sec) * 1e3)
    if p.returncode == 0 and "coefficient streams" in seen:
        last = {k: round(t[-1], 3) for k, t in seen.items() if k != "plan"}
        # the refill reads the factor once (Fp, Fj, Fx) per sweep and writes every stream slot
        m = re.search(r"refill bytes (\d+)", p.stderr)
        rec = {"phases_ms": last}
        if m:
            byts = int(m.group(1))
            rec.update(refill_bytes=byts, refill_GBps=round(byts / last["coefficient streams"] / 1e6, 1))
        emit("ilu_refactor phases (last of 3)", sum(last.values()), **rec)
    else:
        print(p.stderr[-2000:], file=sys.stderr)
        raise SystemExit("the phase run failed")
    if not same:
        raise SystemExit("refreshed handles differ from fresh ones")


if __name__ == "__main__":
    main()
