#!/usr/bin/env python3
"""Time lssp_amd_bilu_refactor against the lssp_amd_bilu_create it replaces, on a
7-point block grid of N^3 cells (default 64) with bs unknowns per cell (default
4), at levels 0 and 1, in one process.

    python tools/bench_bilu_refactor.py [N] [bs] [OUT.jsonl] [reps]

Every call is synchronous (it returns when the stream has finished), so all
times are wall-clock around the call.  Per level it prints (and appends to
OUT.jsonl, when given) one JSON line per item: bilu_create on the new values
(median of reps, default 5), the first bilu_refactor (its plan build included),
the median of reps later ones, the ratio, and whether one apply and get_diag of
the refreshed handle are bitwise a fresh handle's.  With LSSP_AMD_SETUP_TIMES=1
the library prints the phases of every create and refactor to stderr.
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def block_grid7(N, bs, seed):
    """tests/bilu_util.block_grid's matrix family (3-D, columns sorted) without its Python loops:
    diagonal blocks 4.6 J + U(-1, 1), J the anti-identity; off-diagonal blocks -w I + U(-0.2, 0.2),
    w ~ U(0.5, 1)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    nb = N ** 3
    cell = np.arange(nb)
    x, y, z = cell % N, cell // N % N, cell // (N * N)
    offs = [(-N * N, z > 0), (-N, y > 0), (-1, x > 0), (0, np.ones(nb, bool)), (1, x < N - 1), (N, y < N - 1),
            (N * N, z < N - 1)]
    ok = np.stack([m for _, m in offs], axis=1)                      # [cell, 7]
    bj = (cell[:, None] + np.array([o for o, _ in offs])[None, :])[ok]  # blocks in (cell, ascending column) order
    bi = np.repeat(cell, ok.sum(axis=1))
    cnt = ok.sum(axis=1)
    Bp = np.concatenate([[0], np.cumsum(cnt)])
    nblk = bj.size
    V = rng.uniform(-0.2, 0.2, (nblk, bs, bs))                        # [block, r, c]
    V -= rng.uniform(0.5, 1, nblk)[:, None, None] * np.eye(bs)[None]
    d = bi == bj
    V[d] = 4.6 * np.eye(bs)[::-1][None] + rng.uniform(-1, 1, (int(d.sum()), bs, bs))
    # entry (block k of cell i at place q, r, c) sits at Bp[i] bs^2 + r cnt[i] bs + q bs + c
    q = np.arange(nblk) - Bp[bi]
    base = (Bp[bi] * bs * bs + q * bs)[:, None, None] + (np.arange(bs)[None, :, None] * (cnt[bi] * bs)[:, None, None]) \
        + np.arange(bs)[None, None, :]
    Ax = np.empty(nblk * bs * bs)
    Aj = np.empty(nblk * bs * bs, np.int32)
    Ax[base.reshape(-1)] = V.reshape(-1)
    Aj[base.reshape(-1)] = np.broadcast_to((bj * bs)[:, None, None] + np.arange(bs)[None, None, :], base.shape).reshape(-1)
    Ap = np.zeros(nb * bs + 1, np.int64)
    Ap[1:] = np.cumsum(np.repeat(cnt * bs, bs))
    return Ap.astype(np.int32), Aj, Ax


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    bs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    out = open(sys.argv[3], "a") if len(sys.argv) > 3 else None
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    import numpy as np
    import lssp_amd
    Ap, Aj, Ax0 = block_grid7(N, bs, 64)
    vals = [block_grid7(N, bs, 65)[2], block_grid7(N, bs, 66)[2]]  # same pattern, new values
    n, nnz = Ap.size - 1, Aj.size
    dev = lssp_amd.Device(0)

    def emit(op, ms, **kw):
        rec = {"op": op, "N": N, "bs": bs, "n": n, "nnz": nnz, "ms": round(ms, 3), "timer": "wall"}
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

    A = lssp_amd.DMat(dev, Ap, Aj, Ax0)
    v = [dev.vec(nnz, vals[0]), dev.vec(nnz, vals[1])]
    rhs = dev.vec(n, np.random.default_rng(1).uniform(-1, 1, n))
    x, y = dev.vec(n), dev.vec(n)
    ok = True
    for level in (0, 1):
        M = lssp_amd.DILU.bilu(dev, Ap, Aj, Ax0, bs, level=level)  # also takes the first-use costs
        tc = []
        for k in range(reps):  # the create a time step pays today, on the new values
            t, F = wall(lambda k=k: lssp_amd.DILU.bilu(dev, Ap, Aj, vals[k % 2], bs, level=level))
            tc.append(t)
            F.close()
        t_cr = statistics.median(tc)
        emit("bilu_create", t_cr, level=level, ms_min=round(min(tc), 3), ms_max=round(max(tc), 3), reps=reps,
             nnzL=M.nnzL, nnzU=M.nnzU)
        A.update_values(v[0])
        t_first, _ = wall(lambda: M.bilu_refactor(A))
        emit("bilu_refactor(first: plan build included)", t_first, level=level)
        tr = []
        for k in range(reps):  # alternate the two value sets
            A.update_values(v[(k + 1) % 2])
            tr.append(wall(lambda: M.bilu_refactor(A))[0])
        t_rf = statistics.median(tr)
        emit("bilu_refactor(median)", t_rf, level=level, ms_min=round(min(tr), 3), ms_max=round(max(tr), 3), reps=reps)
        emit("refactor vs create", t_rf, level=level, create_over_refactor=round(t_cr / t_rf, 1),
             create_over_first_refactor=round(t_cr / t_first, 1), refactor_faster=bool(t_rf < t_cr))
        # the refreshed handle against a fresh one on the values it holds now, bit for bit
        last = vals[reps % 2]
        F = lssp_amd.DILU.bilu(dev, Ap, Aj, last, bs, level=level)
        M.apply(x, rhs)
        F.apply(y, rhs)
        eq = {"apply": bool(np.array_equal(x.download(), y.download())),
              "diag": bool(np.array_equal(M.diag()[1], F.diag()[1]))}
        emit("refreshed == fresh", 0.0, level=level, bitwise=all(eq.values()), **eq)
        ok = ok and all(eq.values())
        F.close()
        M.close()
    dev.close()
    if not ok:
        raise SystemExit("the refreshed handle differs from a fresh one")


if __name__ == "__main__":
    main()
