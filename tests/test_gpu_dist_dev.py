"""Distributed matrices from device arrays, and the rank's block-Jacobi ILU made on the device.

lssp_amd_mat_from_device_dist against lssp_amd_mat_upload_dist of the same arrays,
lssp_amd_mat_local_block against the block cut out with numpy (bench.local_block),
lssp_amd_mat_update_values on a distributed handle and lssp_amd_mat_local_block_refresh for a
time step: handles, products, factors and BiCGSTAB solves bit for bit between the two routes
and against the oracle's P-rank mode.  Ranks are spawned processes on ONE device over the
host-staged transport (GlooTransport), as in tests/test_gpu_dist.py; one spawn per world
carries every check of that world.  The halo part of x is NaN before every product, so a row
that reads a halo column but was counted into the halo-free run shows up in y."""
import os
import socket

import numpy as np
import pytest

import oracle as O
from dist_dev_util import halo_plan, local_rows, random_rows, rank_rows, step_values, tridiag

pytestmark = pytest.mark.gpu

SEED = 0xD157
EINVAL, EUNSUPPORTED = 1, 6


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _global(kind):
    """(the global CSR, is it a Poisson box, its N)"""
    if kind.startswith("poisson"):
        N = int(kind[7:])
        A = O.poisson(3, N)
        return (A.Ap, A.Aj, A.Ax), True, N
    if kind == "random600":
        return random_rows(600, SEED), False, 0
    return tridiag(5), False, 0


def _observables(A):
    return (A.nhalo, A.ndiag, A.rowcodes, A.valcodes, A.windowed, A.device_bytes, A.nrows, A.nx)


def _status(call):
    import lssp_amd
    try:
        call()
        return 0
    except lssp_amd.LsspError as e:
        return e.status


def _product(dev, A, xown, amx=False):
    """y = A x (or z = 0.5 A x - 2 y0), the halo part of x NaN on entry"""
    x = dev.vec(A.nx, np.concatenate([xown, np.full(A.nhalo, np.nan)]))
    y = dev.vec(A.nx, np.zeros(A.nx))
    if not amx:
        A.mv_mxy(x, y)
        return y.download(A.nrows)
    y0 = dev.vec(A.nx, np.concatenate([xown[::-1], np.zeros(A.nhalo)]))
    A.mv_amxpbyz(0.5, x, -2.0, y0, y)
    return y.download(A.nrows)


def _solve(dev, A, M):
    import lssp_amd
    x = dev.vec(A.nx, np.zeros(A.nx))
    b = dev.vec(A.nx, np.ones(A.nx))
    r = lssp_amd.solve(dev, A, M, x, b, solver=lssp_amd.BICGSTAB, maxit=500, restart=30, trace_cap=100000)
    return r.nits, r.residual, r.trace, x.download(A.nrows)


def _same_solve(a, b):
    return a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def _same_factors(Ma, Mb):
    fa, fb = Ma.factors(), Mb.factors()
    return all(np.array_equal(u, v) for s, t in zip(fa, fb) for u, v in zip(s, t)) and \
        Ma.sweep_layout() == Mb.sweep_layout()


def _worker(rank, world, port, kind, steps, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import lssp_amd
        from bench import local_block
        from inputs import uniform
        from lssp_amd.dist import GlooTransport
        dev = lssp_amd.Device(0, reduction=lssp_amd.TREE)
        dev.comm_init_host(world, rank, GlooTransport())
        (gp, gj, gx), box, N = _global(kind)
        n = gp.size - 1
        r0, nl = rank_rows(n, world, rank)
        Ap, Aj, Ax = local_rows(gp, gj, gx, r0, nl)
        nnz = int(Ap[-1])
        res = {"rank": rank, "ok": {}}
        ok = res["ok"]

        def device_handle(ap, aj, ax):
            return lssp_amd.DMat.from_device_dist(dev, n, r0, nl, int(ap[-1]), dev.idx(nl + 1, ap),
                                                  dev.idx(int(ap[-1]), aj), dev.vec(int(ap[-1]), ax))

        # ---- handle parity -----------------------------------------------------
        Ah = lssp_amd.DMat(dev, Ap, Aj, Ax, dist=(n, r0))
        Ad = device_handle(Ap, Aj, Ax)
        hcols, _, _, _, _ = halo_plan(Ap, Aj, r0, nl)
        xg = uniform(SEED, n)
        res["y"] = np.zeros(0)
        if nl > 0:
            ok["nhalo is the numpy plan's"] = Ad.nhalo == hcols.size
            if kind != "tridiag5":
                ok["observables"] = _observables(Ad) == _observables(Ah)
                ok["valcodes 0"] = Ad.valcodes == 0
            yh, yd = _product(dev, Ah, xg[r0:r0 + nl]), _product(dev, Ad, xg[r0:r0 + nl])
            ok["mv_mxy"] = np.array_equal(yh, yd) and not np.isnan(yd).any()
            zh, zd = _product(dev, Ah, xg[r0:r0 + nl], True), _product(dev, Ad, xg[r0:r0 + nl], True)
            ok["mv_amxpbyz"] = np.array_equal(zh, zd) and not np.isnan(zd).any()
            res["y"] = yd
        sols = {}
        if kind != "tridiag5":
            # ---- block parity ----------------------------------------------------
            bp, bj, bx = local_block(Ap, Aj, Ax, r0, nl)
            Bh = lssp_amd.DMat(dev, bp, bj, bx)
            Bd = Ad.local_block()
            ok["block observables"] = _observables(Bd) == _observables(Bh) and Bd.nnz == int(bp[-1])
            ok["block not distributed"] = Bd.nhalo == 0 and Bd.nx == nl
            if box:
                ok["block value-coded"] = Bd.valcodes > 0
            xb = uniform(SEED + 1 + rank, nl)
            yb = _product(dev, Bd, xb)
            ok["block product"] = np.array_equal(yb, _product(dev, Bh, xb)) and \
                np.array_equal(yb, O.spmv(0, O.CSR(nl, bp, bj, bx), xb))
        if box:
            # ---- the rank's ILU from B, and the solve --------------------------------
            Md, Mh = {}, {}
            for level in (0, 1):
                Md[level] = lssp_amd.DILU.pc_create_dev(dev, Bd, kind=lssp_amd.ILUK, level=level)
                Mh[level] = lssp_amd.DILU.create(dev, bp, bj, bx, kind=lssp_amd.ILUK, level=level)
                ok[f"factors level {level}"] = _same_factors(Md[level], Mh[level])
                # a whole-plane slab keeps its line sweeps, a ragged one takes the general packet route
                ok[f"sweeps level {level}"] = Md[level].sweep_layout()[0] == (level + 1 if nl % (N * N) == 0 else 0)
                res.setdefault("layout", []).append(Md[level].sweep_layout())
                sd, sh = _solve(dev, Ad, Md[level]), _solve(dev, Ah, Mh[level])
                ok[f"solve level {level}"] = _same_solve(sd, sh)
                sols[("first", level)] = sd
            # ---- time steps: new values on the same pattern -----------------------------
            rhs, app = dev.vec(nl, uniform(SEED + 9, nl)), dev.vec(nl)
            for step in range(steps):
                Ax2 = step_values(Ap, Aj, Ax, r0, SEED + 100 * (step + 1) + rank)
                Ad.update_values(dev.vec(nnz, Ax2))
                Bd.refresh_block(Ad)
                Af = lssp_amd.DMat(dev, Ap, Aj, Ax2, dist=(n, r0))
                fp, fj, fx = local_block(Ap, Aj, Ax2, r0, nl)
                for level in (0, 1):
                    if Md[level].sweep_layout()[0] == 1:
                        Md[level].refactor(Bd)
                    else:
                        Md[level].iluk_refactor(Bd)
                    Mf = lssp_amd.DILU.create(dev, fp, fj, fx, kind=lssp_amd.ILUK, level=level)
                    ok[f"step {step} factors level {level}"] = _same_factors(Md[level], Mf)
                    Md[level].apply(app, rhs)  # a bare apply between the steps
                    Lf, Uf = Mf.factors()
                    ok[f"step {step} apply level {level}"] = np.array_equal(
                        app.download(), O.ilu_apply(O.CSR(nl, *Lf), O.CSR(nl, *Uf), uniform(SEED + 9, nl)))
                    sd, sf = _solve(dev, Ad, Md[level]), _solve(dev, Af, Mf)
                    ok[f"step {step} solve level {level}"] = _same_solve(sd, sf)
                    sols[(step, level)] = sd
                ok[f"step {step} product"] = np.array_equal(_product(dev, Ad, xg[r0:r0 + nl]),
                                                            _product(dev, Af, xg[r0:r0 + nl]))
                ok[f"step {step} valcodes 0"] = Ad.valcodes == 0
            if steps:
                # ---- refusals; every handle is used again afterwards -------------------
                rows = np.repeat(np.arange(nl), np.diff(Ap))
                keep = np.ones(nnz, bool)
                keep[np.flatnonzero((Aj >= r0) & (Aj < r0 + nl) & (Aj != r0 + rows))[0]] = False
                cut = np.zeros(nl + 1, np.int32)
                np.cumsum(np.bincount(rows[keep], minlength=nl), out=cut[1:])
                Ac = lssp_amd.DMat(dev, cut, Aj[keep], Ax[keep], dist=(n, r0))  # one owned entry fewer
                before = _product(dev, Bd, xb)
                ok["refresh with another pattern: EINVAL"] = _status(lambda: Bd.refresh_block(Ac)) == EINVAL
                ok["refresh of a distributed B: EINVAL"] = _status(lambda: Ad.refresh_block(Ad)) == EINVAL
                ok["B unchanged"] = np.array_equal(before, _product(dev, Bd, xb))
                ok["pc_create_dev on a distributed A: EUNSUPPORTED"] = _status(
                    lambda: lssp_amd.DILU.pc_create_dev(dev, Ad, kind=lssp_amd.ILUK, level=0)) == EUNSUPPORTED
                Bd.refresh_block(Ad)
                ok["B refreshed again"] = np.array_equal(before, _product(dev, Bd, xb))
        dev.barrier()
        res["sols"] = {k: v[:3] for k, v in sols.items()}
        res["x"] = {k: v[3] for k, v in sols.items()}
        parts = [None] * world
        dist.all_gather_object(parts, res)
        if rank == 0:
            out.put(parts)
        dev.close()
    finally:
        dist.destroy_process_group()


def _spawn(target, world, *args, timeout=150):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = q.get(timeout=timeout)
    finally:
        for p in procs:
            p.join(timeout=30)
    assert all(p.exitcode == 0 for p in procs)
    return got


def _oracle_solve(A, world, level):
    L, U = O.ilu(A, "iluk", level=level, blk=(A.n + world - 1) // world)
    return O.solve(O.BICGSTAB, A, np.ones(A.n), L=L, U=U, mode=O.TREE, nranks=world, maxit=500, restart=30)


@pytest.mark.parametrize("world,kind,steps", [(2, "poisson12", 2), (3, "poisson10", 2), (4, "poisson16", 0),
                                              (3, "random600", 0), (4, "tridiag5", 0)],
                         ids=["2x12^3", "3x10^3", "4x16^3", "3xrandom600", "4xtridiag5"])
def test_device_made_distributed_handles_equal_the_host_route_and_the_oracle(world, kind, steps):
    """from_device_dist == DMat(dist=...), local_block == DMat(local_block(...)), the ILU(0) and
    ILU(1) of B == DILU.create of the host block, BiCGSTAB (TREE) with the device-made pair bitwise
    the host-made pair's and the oracle's P-rank mode; two time steps (update_values,
    refresh_block, refactor) bitwise a fresh host build and the oracle; the refusals."""
    from inputs import uniform
    parts = _spawn(_worker, world, kind, steps)
    print(kind, "sweep layouts (level 0, level 1) per rank:", [p.get("layout") for p in parts])
    for p in parts:
        bad = [k for k, v in p["ok"].items() if not v]
        assert not bad, (p["rank"], bad)
    (gp, gj, gx), box, _ = _global(kind)
    A = O.CSR(gp.size - 1, gp, gj, gx)
    assert np.array_equal(np.concatenate([p["y"] for p in parts]), O.spmv(0, A, uniform(SEED, A.n)))
    if not box:
        return
    assert all(("solve level 0" in p["ok"] and "solve level 1" in p["ok"]) for p in parts)
    for key in parts[0]["sols"]:
        when, level = key
        Ao = A
        if when != "first":  # the step's values, rank by rank, as the workers made them
            vals = []
            for r in range(world):
                r0, nl = rank_rows(A.n, world, r)
                lp, lj, lx = local_rows(gp, gj, gx, r0, nl)
                vals.append(step_values(lp, lj, lx, r0, SEED + 100 * (when + 1) + r))
            Ao = O.CSR(A.n, gp, gj, np.concatenate(vals))
        o = _oracle_solve(Ao, world, level)
        nits, res, trace = parts[0]["sols"][key]
        assert nits == o.nits and res == o.residual, (key, nits, o.nits)
        assert np.array_equal(trace, o.trace), key
        assert np.array_equal(np.concatenate([p["x"][key] for p in parts]), o.x), key
    assert len(parts[0]["sols"]) == 2 + 2 * steps


def _bad_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import lssp_amd
        from inputs import uniform
        from lssp_amd.dist import GlooTransport
        dev = lssp_amd.Device(0)
        dev.comm_init_host(world, rank, GlooTransport())
        N = 8
        n = N ** 3
        r0, nl = rank_rows(n, world, rank)
        Ap, Aj, Ax = lssp_amd.poisson(3, N, r0, nl)
        nnz = int(Ap[-1])

        def make(ap, aj):
            return lssp_amd.DMat.from_device_dist(dev, n, r0, nl, nnz, dev.idx(nl + 1, ap), dev.idx(nnz, aj),
                                                  dev.vec(nnz, Ax))
        got = []
        for bad_rank in (0, 1):
            bj = Aj.copy()
            if rank == bad_rank:
                bj[3] = n + 7  # a column outside the global matrix
            got.append(_status(lambda: make(Ap, bj)))
            bp = Ap.copy()
            if rank == bad_rank:
                bp[5], bp[6] = Ap[6], Ap[5]  # the row pointers step back
            got.append(_status(lambda: make(bp, Aj)))
        A = make(Ap, Aj)  # and the ranks still build a handle together
        y = _product(dev, A, uniform(SEED, n)[r0:r0 + nl])
        dev.barrier()
        parts = [None] * world
        dist.all_gather_object(parts, (got, y))
        if rank == 0:
            out.put(parts)
        dev.close()
    finally:
        dist.destroy_process_group()


def test_from_device_dist_bad_input_fails_on_every_rank():
    """a column n + 7, or row pointers that step back, on ONE rank of two: the flag raised on
    the device is agreed on before any collective step, so BOTH ranks return EINVAL, none waits
    in the exchange, both go on to build a good handle and exit with status 0"""
    from inputs import uniform
    parts = _spawn(_bad_worker, 2)
    for got, _ in parts:
        assert got == [EINVAL] * 4
    A = O.poisson(3, 8)
    assert np.array_equal(np.concatenate([y for _, y in parts]), O.spmv(0, A, uniform(SEED, A.n)))


def test_one_rank_without_a_communicator():
    """one rank, no comm_init: no halo, no exchange; the distributed handle's product is the
    oracle's, and its local block is a copy -- the single-rank handle of the same arrays"""
    import lssp_amd
    from inputs import uniform
    Ap, Aj, Ax = lssp_amd.poisson(3, 7)
    n, nnz = Ap.size - 1, int(Ap[-1])
    dev = lssp_amd.Device(0)
    Ad = lssp_amd.DMat.from_device_dist(dev, n, 0, n, nnz, dev.idx(n + 1, Ap), dev.idx(nnz, Aj), dev.vec(nnz, Ax))
    Ah = lssp_amd.DMat(dev, Ap, Aj, Ax, dist=(n, 0))
    assert Ad.nhalo == 0 and _observables(Ad) == _observables(Ah) and Ad.valcodes == 0
    x = uniform(SEED, n)
    want = O.spmv(0, O.CSR(n, Ap, Aj, Ax), x)
    assert np.array_equal(_product(dev, Ad, x), want) and np.array_equal(_product(dev, Ah, x), want)
    B, S = Ad.local_block(), lssp_amd.DMat(dev, Ap, Aj, Ax)
    assert _observables(B) == _observables(S) and B.valcodes > 0 and B.nnz == nnz
    assert np.array_equal(_product(dev, B, x), want)
    M = lssp_amd.DILU.pc_create_dev(dev, B, kind=lssp_amd.ILUK, level=0)
    assert _same_factors(M, lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0))
    dev.close()
