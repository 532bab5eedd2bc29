#!/usr/bin/env python3
"""Time lssp_amd_iluk_refactor against the lssp_amd_ilu_create it replaces, in one
process, on three workloads:

    box216-l1   7-point box of 216^3, ILU(1): the skewed line sweeps (the reference's default)
    thermal-l0  lssp_amd.thermal_like(), ILU(0): packet sweeps of an irregular matrix
    box128-l2   7-point box of 128^3, ILU(2): packet sweeps

    python tools/bench_iluk_refactor.py [OUT.jsonl] [reps] [--create-only LABEL] [--only NAME] [--scale S]

Every call is synchronous (it returns when the stream has finished), so all
times are wall-clock around the call.  Per workload it prints (and appends to
OUT.jsonl, when given) one JSON line per item: ilu_create on the new values
(median of reps, default 5), the first iluk_refactor (its plan build included),
the median of reps later ones with the library's own phase times (match,
scatter, numeric, refill: LSSP_AMD_SETUP_TIMES=1, which this tool sets; the
stream is drained after each phase, so the median includes four extra
synchronisations), the ratio, and whether one apply of the refreshed handle is
bitwise a fresh handle's.  --create-only LABEL times the creates alone and tags
them LABEL: run from a checkout of the parent commit it shows that create, which
now also keeps one flag byte per factor entry, is unchanged within its spread.
--scale S shrinks every grid edge by S (a quick functional run).
"""
import json
import os
import re
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("LSSP_AMD_SETUP_TIMES", "1")


def box7(N):
    """pattern of the 7-point stencil on an N^3 box, natural order, rows sorted"""
    import numpy as np
    n = N ** 3
    cell = np.arange(n)
    x, y, z = cell % N, cell // N % N, cell // (N * N)
    offs = [(-N * N, z > 0), (-N, y > 0), (-1, x > 0), (0, np.ones(n, bool)), (1, x < N - 1), (N, y < N - 1),
            (N * N, z < N - 1)]
    ok = np.stack([m for _, m in offs], axis=1)
    Aj = (cell[:, None] + np.array([o for o, _ in offs])[None, :])[ok]
    Ap = np.concatenate([[0], np.cumsum(ok.sum(axis=1))])
    return Ap.astype(np.int32), Aj.astype(np.int32)


def box_values(Ap, Aj, seed):
    """off-diagonals in [-1, -0.1), diagonals in [7, 8): nonsymmetric, diagonally dominant"""
    import numpy as np
    rng = np.random.default_rng(seed)
    Ax = rng.uniform(-1, -0.1, Aj.size)
    d = Aj == np.repeat(np.arange(Ap.size - 1, dtype=np.int32), np.diff(Ap))
    Ax[d] = rng.uniform(7, 8, int(d.sum()))
    return Ax


def thermal_values(Ap, Aj, Ax, seed):
    """the same Laplacian with every entry scaled by 1 +- 5 % (off-diagonals) or 1.1 +- 5 % (diagonal)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.95, 1.05, Ax.size)
    d = Aj == np.repeat(np.arange(Ap.size - 1, dtype=np.int32), np.diff(Ap))
    s[d] += 0.1
    return Ax * s


def capture_stderr(fn):
    """fn() with the process's stderr (the library's phase lines) collected"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            r = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return r, tmp.read().decode(errors="replace")


PHASE = re.compile(r"lssp_amd iluk_refactor:\s+(\S.*?)\s+([0-9.]+) s")


def main():
    args = sys.argv[1:]
    label, only, scale = None, None, 1
    for flag in ("--create-only", "--only", "--scale"):
        if flag in args:
            i = args.index(flag)
            v = args[i + 1]
            del args[i:i + 2]
            if flag == "--create-only":
                label = v
            elif flag == "--only":
                only = v
            else:
                scale = int(v)
    out = open(args[0], "a") if len(args) > 0 else None
    reps = int(args[1]) if len(args) > 1 else 5
    import numpy as np
    import lssp_amd
    dev = lssp_amd.Device(0)

    def workloads():
        if only in (None, "box216-l1"):
            Ap, Aj = box7(216 // scale)
            yield "box216-l1", 1, 2, Ap, Aj, [box_values(Ap, Aj, 70 + k) for k in range(3)]
        if only in (None, "thermal-l0"):
            from lssp_amd.synthetic import thermal_like
            Ap, Aj, Ax = thermal_like(m=1108 // scale)
            yield "thermal-l0", 0, 0, Ap, Aj, [Ax] + [thermal_values(Ap, Aj, Ax, 80 + k) for k in range(2)]
        if only in (None, "box128-l2"):
            Ap, Aj = box7(128 // scale)
            yield "box128-l2", 2, 0, Ap, Aj, [box_values(Ap, Aj, 90 + k) for k in range(3)]

    def wall(fn):
        dev.sync()
        t0 = time.perf_counter()
        r = fn()
        dev.sync()
        return (time.perf_counter() - t0) * 1e3, r

    ok = True
    for name, level, line, Ap, Aj, (Ax0, *vals) in workloads():
        n, nnz = Ap.size - 1, Aj.size

        def emit(op, ms, **kw):
            rec = {"op": op, "workload": name, "level": level, "n": n, "nnz": nnz, "ms": round(ms, 3), "timer": "wall"}
            if label:
                rec["commit"] = label
            rec.update(kw)
            text = json.dumps(rec)
            print(text, flush=True)
            if out:
                out.write(text + "\n")
                out.flush()

        def create(ax):
            return lssp_amd.DILU.create(dev, Ap, Aj, ax, kind=lssp_amd.ILUK, level=level)

        M = create(Ax0)  # also takes the first-use costs
        assert M.sweep_layout()[0] == line, (name, M.sweep_layout())
        tc = []
        for k in range(reps):  # the create a time step pays today, on the new values
            t, F = wall(lambda k=k: create(vals[k % 2]))
            tc.append(t)
            F.close()
        t_cr = statistics.median(tc)
        emit("ilu_create", t_cr, ms_min=round(min(tc), 3), ms_max=round(max(tc), 3), reps=reps, nnzL=M.nnzL,
             nnzU=M.nnzU, sweep_layout=list(M.sweep_layout()))
        if label:
            M.close()
            continue
        A = lssp_amd.DMat(dev, Ap, Aj, Ax0)
        v = [dev.vec(nnz, vals[0]), dev.vec(nnz, vals[1])]
        A.update_values(v[0])
        (t_first, _), _ = capture_stderr(lambda: wall(lambda: M.iluk_refactor(A)))
        emit("iluk_refactor(first: plan build included)", t_first)
        tr, phases = [], {}
        for k in range(reps):  # alternate the two value sets
            A.update_values(v[(k + 1) % 2])
            (t, _), err = capture_stderr(lambda: wall(lambda: M.iluk_refactor(A)))
            tr.append(t)
            for ph, sec in PHASE.findall(err):
                phases.setdefault(ph, []).append(float(sec) * 1e3)
        t_rf = statistics.median(tr)
        emit("iluk_refactor(median)", t_rf, ms_min=round(min(tr), 3), ms_max=round(max(tr), 3), reps=reps,
             phases_ms={ph: round(statistics.median(ts), 3) for ph, ts in phases.items()})
        emit("refactor vs create", t_rf, create_over_refactor=round(t_cr / t_rf, 1),
             create_over_first_refactor=round(t_cr / t_first, 1), refactor_faster=bool(t_rf < t_cr))
        # the refreshed handle against a fresh one on the values it holds now, bit for bit
        F = create(vals[reps % 2])
        rhs = dev.vec(n, np.random.default_rng(1).uniform(-1, 1, n))
        x, y = dev.vec(n), dev.vec(n)
        M.apply(x, rhs)
        F.apply(y, rhs)
        same = bool(np.array_equal(x.download(), y.download()))
        emit("refreshed == fresh", 0.0, bitwise=same)
        ok = ok and same and t_rf < t_cr
        for h in (F, M, A):
            h.close()
    dev.close()
    if not ok:
        raise SystemExit("the refreshed handle differs from a fresh one, or a refactor was not faster than create")


if __name__ == "__main__":
    main()
