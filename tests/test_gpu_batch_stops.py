"""The batched drivers' stop, on every position of a batch.

BiCGSTAB (no preconditioner or line sweeps) and CG (no preconditioner) queue 8
and 32 iterations per batch (solvers.cpp), two batches in flight, test for the
stop on the device and rebuild nits, the residual, the trace and the printed
lines from a snapshot of the residual ring.  What that machinery does depends
on where in a batch the stop lands: the batch's last CG iteration launches its
own x update (CGF_X), a stop in batch j leaves batch j + 1 queued behind the
guard (its skipped line sweeps must leave the next apply's hand-off buffers
armed), iteration k's residual sits in ring slot k % S_HB, and the ||s|| exit
reports one iteration line fewer.  tests/stop_util.py places a stop on each of
these positions from the oracle alone (tests/test_batch_stops_cpu.py checks
the plan); here every planned stop runs on the GPU.

Per stop: nits, residual, the whole trace and x are bitwise the oracle's, with
the handle's own factors; the handles of a route serve all its stops, so right
after each stopped solve a bare apply is bitwise the oracle's and the same
solve run again is bitwise the first.
"""
import ctypes
import os
import socket

import numpy as np
import pytest

import oracle as O
import stop_util as SU
from inputs import uniform

pytestmark = pytest.mark.gpu

MODES = {"tree": O.TREE, "serial": O.SERIAL}


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


class Route:
    """the handles of one matrix (and preconditioner), made once and reused by every stop"""

    def __init__(self, dev, A, level=None, layout=None):
        import lssp_amd
        self.dev, self.A, self.n = dev, A, A.n
        self.D = lssp_amd.DMat(dev, A.Ap, A.Aj, A.Ax)
        self.M = self.L = self.U = None
        if level is not None:
            self.M = lssp_amd.DILU.create(dev, A.Ap, A.Aj, A.Ax, kind=lssp_amd.ILUK, level=level)
            # a route that silently fell back to another sweep fails here
            assert self.M.sweep_layout() == layout
            (Lp, Lj, Lx), (Up, Uj, Ux) = self.M.factors()
            self.L, self.U = O.CSR(A.n, Lp, Lj, Lx), O.CSR(A.n, Up, Uj, Ux)
            self.rhs = uniform(0xA991, A.n)
            self.rhs_d = dev.vec(A.n, self.rhs)
            self.y = dev.vec(A.n)
            self.applied = O.ilu_apply(self.L, self.U, self.rhs)
        self.x, self.b = dev.vec(A.n), dev.vec(A.n)

    def solve(self, solver, stop, b=None, verb=0, maxit=None):
        import lssp_amd
        self.x.upload(np.zeros(self.n))
        self.b.upload(SU.rhs(self.n, stop.bexp) if b is None else b)
        r = lssp_amd.solve(self.dev, self.D, self.M, self.x, self.b, solver=solver, tol_rel=stop.rtol,
                           tol_abs=stop.atol, tol_rb=0.0, maxit=stop.maxit if maxit is None else maxit, verb=verb,
                           trace_cap=4096)
        return r, self.x.download()


_routes = {}


def _route(dev, key):
    """key: a BiCGSTAB route of stop_util.BICG_ROUTES or a CG matrix of stop_util.CG_MATS"""
    if key not in _routes:
        if key in SU.BICG_ROUTES:
            dim, N, level, layout = SU.BICG_ROUTES[key]
            _routes[key] = Route(dev, SU.matrix(dim, N), level, layout)
        else:
            _routes[key] = Route(dev, SU.matrix(*SU.CG_MATS[key]))
    return _routes[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_routes():
    yield
    _routes.clear()


def _same(r, x, o):
    assert r.nits == o.nits
    assert r.residual == o.residual
    assert np.array_equal(r.trace, o.trace)
    assert np.array_equal(x, o.x)


def _run_stops(dev, R, solver, mode, stops):
    import lssp_amd
    assert stops
    dev.set_reduction(mode)
    try:
        for st in stops:
            o = SU.expect(solver, R.A, R.L, R.U, mode, st)
            assert o.nits == st.m, st  # the plan holds with the handle's own factors
            r1, x1 = R.solve(solver, st)
            print(f"{st.id}: nits {r1.nits} residual {r1.residual!r} trace {r1.trace.size} (oracle {o.nits} "
                  f"{o.residual!r} {o.trace.size})")
            if R.M is not None:  # the state the stopped batches left behind: a bare apply
                R.M.apply(R.y, R.rhs_d)
                assert np.array_equal(R.y.download(), R.applied), st
            r2, x2 = R.solve(solver, st)  # and the same solve again
            _same(r1, x1, o)
            assert r2.nits == r1.nits and r2.residual == r1.residual, st
            assert np.array_equal(r2.trace, r1.trace) and np.array_equal(x2, x1), st
    finally:
        dev.set_reduction(lssp_amd.TREE)


# ---- BiCGSTAB ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["maxit", "tol", "brk"])
@pytest.mark.parametrize("route", sorted(SU.BICG_ROUTES))
def test_bicgstab_tree_stops_at_every_batch_position(dev, route, kind):
    """maxit 1..18 (the short last batch), tolerance 1..17 (the stop flag, the guard, the batch
    still queued) and the ||s|| <= 1e-40 exit at 8, 9 and 16 or 17"""
    _run_stops(dev, _route(dev, route), O.BICGSTAB, O.TREE, SU.bicg_plan(route, O.TREE)[kind])


@pytest.mark.parametrize("kind", ["maxit", "tol"])
@pytest.mark.parametrize("route", SU.BICG_SERIAL_ROUTES)
def test_bicgstab_serial_stops_around_the_batch_boundaries(dev, route, kind):
    """the reference's reduction order (||s|| in a round of its own): 7, 8, 9, 16, 17"""
    _run_stops(dev, _route(dev, route), O.BICGSTAB, O.SERIAL, SU.bicg_plan(route, O.SERIAL)[kind])


@pytest.mark.parametrize("m", sorted(SU.RHO_CASES))
def test_bicgstab_rho_exit_after_a_batchs_last_and_first_iteration(dev, m):
    """"the next iteration's rho1 == 0" (:89-92, the device's stop code 3): small integer systems
    on which r becomes exactly orthogonal to r^ in iteration 7 (a batch's last) and 8 (the next
    batch's first).  No preconditioner; bitwise the oracle's run, twice."""
    A, b = SU.rho_case(m)
    o = SU.rho_expect(m)
    assert o.nits == m and SU.is_rho_exit(o, SU.RHO_MAXIT)
    R = Route(dev, A)
    st = SU.Stop("rho", m, SU.RHO_MAXIT)
    r1, x1 = R.solve(O.BICGSTAB, st, b=b)
    r2, x2 = R.solve(O.BICGSTAB, st, b=b)
    _same(r1, x1, o)
    _same(r2, x2, o)


# ---- CG ---------------------------------------------------------------------------------------

def _cg_stops(mat, mode, kind, part):
    stops = SU.cg_plan(mat, mode)[kind]
    if kind == "tol":  # one test per batch the stop lands in (and the third batch's first two)
        lo, hi = ((1, SU.CG_BATCH), (SU.CG_BATCH + 1, 2 * SU.CG_BATCH + 2))[part]
        stops = [s for s in stops if lo <= s.m <= hi]
    return stops


@pytest.mark.parametrize("kind,part", [("maxit", 0), ("tol", 0), ("tol", 1)], ids=["maxit", "tol-batch1", "tol-batch2"])
@pytest.mark.parametrize("mat", sorted(SU.CG_MATS))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_cg_stops_at_every_batch_position(dev, mode, mat, kind, part):
    """tree: k_cg_fused, whose x update rides with the next p pass except in the batch's last
    iteration (CGF_X, stamped with the global iteration count); serial: the unfused K_CG_XR path.
    maxit at 1, 2, 31..34, 63..66; a tolerance stop at every iteration 1..66 at which the
    residual reaches a new low on this matrix (on one of the two matrices: every iteration)"""
    _run_stops(dev, _route(dev, mat), O.CG, MODES[mode], _cg_stops(mat, MODES[mode], kind, part))


# ---- the printed lines --------------------------------------------------------------------------

def _lines(R, solver, st):
    import lssp_amd
    lines = []
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p)
    cb = CB(lambda user, msg: lines.append(msg.decode()) or 0)
    L = lssp_amd._lib.load()
    L.lssp_amd_set_print(ctypes.cast(cb, ctypes.c_void_p), None)
    try:
        r, x = R.solve(solver, st, verb=1)
    finally:
        L.lssp_amd_set_print(None, None)
    print("".join(lines), r.nits, repr(r.residual))
    return r, x, lines


def _check_lines(R, solver, mode, st):
    name = "bicgstab" if solver == O.BICGSTAB else "cg"
    o = SU.expect(solver, R.A, R.L, R.U, mode, st)
    r, x, lines = _lines(R, solver, st)
    _same(r, x, o)
    its = [ln for ln in lines if ln.startswith(f"{name}: itr: ")]
    rest = [ln for ln in lines if not ln.startswith(f"{name}: itr: ")]
    printed = st.m - 1 if st.kind == "brk" else st.m
    assert [int(ln.split("itr:")[1].split(",")[0]) for ln in its] == list(range(printed))
    last = float(its[-1].split("abs res:")[1].split(",")[0])
    if st.kind == "brk":
        # the iteration that broke down prints no line (:117 comes before :143): the last line is
        # the iteration before it, then the driver's message and nothing more
        assert len(rest) == 1 and rest[0].startswith("bicgstab: ||s|| is too small: ") and lines[-1] is rest[0]
        before = O.solve(solver, R.A, SU.rhs(R.n, st.bexp), L=R.L, U=R.U, rtol=0.0, atol=0.0, rbtol=0.0,
                         maxit=st.m - 1, mode=mode)
        assert last == float(f"{before.residual:.6e}")
    else:
        assert rest == []
        assert last == float(f"{r.residual:.6e}")


@pytest.mark.parametrize("route", sorted(SU.BICG_ROUTES))
def test_bicgstab_iteration_lines_at_the_batch_boundary(dev, route):
    """verb = 1: one line per iteration 0..m-1 without a gap for a tolerance and a maxit stop at
    m = 8 and 9, 0..m-2 and the driver's message for the ||s|| exit; the last residual printed
    is the one returned (the ||s|| exit: the one of the iteration before)"""
    R = _route(dev, route)
    plan = SU.bicg_plan(route, O.TREE)
    for kind in ("tol", "maxit", "brk"):
        for m in (SU.BATCH, SU.BATCH + 1):
            (st,) = [s for s in plan[kind] if s.m == m]
            _check_lines(R, O.BICGSTAB, O.TREE, st)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_cg_iteration_lines_at_the_batch_boundary(dev, mode):
    import lssp_amd
    R = _route(dev, "p3_16")
    plan = SU.cg_plan("p3_16", MODES[mode])
    dev.set_reduction(MODES[mode])
    try:
        for kind in ("tol", "maxit"):
            for m in (SU.CG_BATCH, SU.CG_BATCH + 1):
                (st,) = [s for s in plan[kind] if s.m == m]
                _check_lines(R, O.CG, MODES[mode], st)
    finally:
        dev.set_reduction(lssp_amd.TREE)


# ---- two ranks ------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, N, solver, stops, out):
    """one rank: the handles made once, the stops run in sequence on them"""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import lssp_amd
        from bench import local_block
        from lssp_amd.dist import GlooTransport
        dev = lssp_amd.Device(0, reduction=lssp_amd.TREE)
        dev.comm_init_host(world, rank, GlooTransport())
        n = N ** 3
        blk = (n + world - 1) // world
        r0 = min(rank * blk, n)
        nl = min(blk, n - r0)
        Ap, Aj, Ax = lssp_amd.poisson(3, N, r0, nl)
        A = lssp_amd.DMat(dev, Ap, Aj, Ax, dist=(n, r0))
        M = None
        if solver == lssp_amd.BICGSTAB:  # block-Jacobi ILU(0): this rank's slab on the line sweeps
            bp, bj, bx = local_block(Ap, Aj, Ax, r0, nl)
            M = lssp_amd.DILU.create(dev, bp, bj, bx, kind=lssp_amd.ILUK, level=0)
            assert M.sweep_layout()[0] == 1
            (Lp, Lj, Lx), (Up, Uj, Ux) = M.factors()
            rhs = uniform(0xA991 + rank, nl)
            rhs_d, y = dev.vec(nl, rhs), dev.vec(nl)
            applied = O.ilu_apply(O.CSR(nl, Lp, Lj, Lx), O.CSR(nl, Up, Uj, Ux), rhs)
        x, b = dev.vec(A.nx), dev.vec(A.nx, np.ones(A.nx))
        res = []
        for st in stops:
            x.upload(np.zeros(A.nx))
            r = lssp_amd.solve(dev, A, M, x, b, solver=solver, tol_rel=st.rtol, tol_abs=st.atol, tol_rb=0.0,
                               maxit=st.maxit, trace_cap=4096)
            ok = True
            if M is not None:
                M.apply(y, rhs_d)
                ok = bool(np.array_equal(y.download(), applied))
            res.append((r.nits, r.residual, r.trace, x.download(nl), ok))
        dev.barrier()
        parts = [None] * world
        dist.all_gather_object(parts, res)
        if rank == 0:
            out.put([(p0[0], p0[1], p0[2], np.concatenate([p[i][3] for p in parts]), all(p[i][4] for p in parts))
                     for i, p0 in enumerate(parts[0])])
        dev.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("solver", [O.BICGSTAB, O.CG], ids=["bicgstab", "cg"])
def test_two_rank_stops_around_the_batch_boundaries(solver):
    """two ranks on one device over the host transport, 7-pt 16^3: the rank-combined reductions
    decide the stop (CG: the unfused path, tree order).  BiCGSTAB with block-Jacobi ILU(0) per
    rank on the line sweeps: tolerance 7, 8, 9, 10, 16, 17 and maxit 8, 9; CG: tolerance 31..34.
    One spawn per driver; the stops run in sequence on the same handles, each bitwise the
    oracle's 2-rank mode, and each rank's bare apply after every stop bitwise the oracle's."""
    import torch.multiprocessing as mp
    stops = SU.dist_plan(solver)
    A, L, U = SU.dist_inputs(solver)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, SU.DIST_RANKS, port, SU.DIST_N, solver, stops, q))
             for r in range(SU.DIST_RANKS)]
    for p in procs:
        p.start()
    try:
        want = [SU.expect(solver, A, L, U, O.TREE, st, nranks=SU.DIST_RANKS) for st in stops]
        got = q.get(timeout=150)
    finally:
        for p in procs:
            p.join(timeout=30)
    assert all(p.exitcode == 0 for p in procs)
    assert len(got) == len(stops)
    for st, o, (nits, res, trace, x, applied_ok) in zip(stops, want, got):
        print(f"{st.id}: nits {nits} residual {res!r} (oracle {o.nits} {o.residual!r})")
        assert o.nits == st.m
        assert nits == o.nits, st
        assert res == o.residual, st
        assert np.array_equal(trace, o.trace), st
        assert np.array_equal(x, o.x), st
        assert applied_ok, st
