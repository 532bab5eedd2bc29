"""Case tables, the oracle's expected values and the one spawn runner of the P-rank driver
tests (tests/test_gpu_dist_drivers.py on the GPU, tests/test_dist_drivers_cpu.py without one).

A LEG is one world of rank processes on one device over the host-staged transport
(lssp_amd.dist.GlooTransport).  Its worker builds each matrix handle and preconditioner of
the leg once and runs every (driver, mode, pc) case in the table's order, the same on every
rank; the results come back once, as a dict keyed by case.  The pytest cases only assert on
that dict, so a wrong driver fails under its own id and a leg costs one process start-up.

  A  4 ranks: the reference's block-Jacobi (nblk = 4) runs of all 19 drivers (tests/golden/)
  B  2 ranks: nonsymmetric random rows, unsorted, 389 + 388 rows, x0 != 0, b not constant
  C  3 ranks: 334 + 334 + 332 rows of a random matrix and of the 7-point 10^3 box
  D  4 ranks, the last one without rows: a 9-row tridiagonal matrix
  E  2 ranks: every rank holds the ILU(0) of the whole matrix (the reference's own run)

The random matrices go to the oracle and to the preconditioners as generated (unsorted rows);
each rank column-sorts its rows before the upload, as lssp_solver_assemble does (lssp.cxx:173)
and as the oracle's solve does with its copy -- the library's products sum in entry order.

In every case the halo part of x and the tail of b beyond the rank's rows are NaN on entry:
the solve's products overwrite the first and nothing may read the second (include/lssp_amd.h),
so a read of stale halo data turns up as NaN in the bitwise comparisons.
"""
from __future__ import annotations

import functools
import json
import os
import queue
import socket
import time

import numpy as np

import oracle as O
from dist_dev_util import local_rows, rank_rows, tridiag
from golden_util import build_matrix, cases as golden_cases, fx, matches, vec

QUEUE_WAIT = 150.0  # seconds a leg may take before its ranks are reaped
TRACE_CAP = 100000
DEF_TOL = 1e-7      # lssp.cxx:11-13

NAMES = {O.GMRES: "gmres", O.LGMRES: "lgmres", O.RGMRES: "rgmres", O.RLGMRES: "rlgmres", O.BICGSTAB: "bicgstab",
         O.BICGSTABL: "bicgstabl", O.BICGSAFE: "bicgsafe", O.CG: "cg", O.CGS: "cgs", O.GPBICG: "gpbicg", O.CR: "cr",
         O.CRS: "crs", O.BICRSTAB: "bicrstab", O.BICRSAFE: "bicrsafe", O.GPBICR: "gpbicr",
         O.QMRCGSTAB: "qmrcgstab", O.TFQMR: "tfqmr", O.ORTHOMIN: "orthomin", O.IDRS: "idrs"}
DRIVERS = sorted(NAMES)                                   # all 19
ARNOLDI = (O.GMRES, O.LGMRES, O.RGMRES, O.RLGMRES)        # the GMRES family (restart = m)
SL = (O.BICGSTABL, O.IDRS)                                # restart = l / s
MODES = ((O.TREE, "tree"), (O.SERIAL, "serial"))

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rlgmres_manifest.json")) as _f:
    GOLDEN = golden_cases("solve") + json.load(_f)["cases"]  # the reference's runs of all 19 drivers

POISSON = {"type": "poisson", "dim": 3}
RAND777 = {"type": "rand", "n": 777, "per_row": 6, "seed": 0x51, "unsorted": True}
RAND1000 = {"type": "rand", "n": 1000, "per_row": 6, "seed": 0x52, "unsorted": True}
TRIDIAG9 = {"type": "tridiag", "n": 9}


def _matkey(mat) -> str:
    return json.dumps(mat, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _matrix(matkey: str) -> O.CSR:
    mat = json.loads(matkey)
    if mat["type"] == "tridiag":
        Ap, Aj, Ax = tridiag(mat["n"])
        return O.CSR(mat["n"], Ap, Aj, Ax)
    return build_matrix(mat)


def matrix(mat) -> O.CSR:
    """the global matrix of a case, as generated (random rows stay unsorted)"""
    return _matrix(_matkey(mat))


# ---- the case tables -----------------------------------------------------------------------
def _case(leg, group, mat, world, solver, mode, pc, *, b, x0, tol, maxit, restart, golden=None, bound=False):
    """pc: "bj" the rank's block-Jacobi ILU(0), "none", "global" the ILU(0) of the whole matrix.
    tol: (rel, abs, rb).  golden: the reference's run this case repeats (SERIAL: bit for bit).
    bound: TREE mode stops within max(1, 5 %) iterations of the reference's count."""
    mname = dict(MODES)[mode]
    return {"key": f"{leg}-{group}-{NAMES[solver]}-{pc}-{mname}", "leg": leg, "group": group, "mat": mat,
            "world": world, "solver": solver, "mode": mode, "pc": pc, "b": b, "x0": x0, "tol": tol, "maxit": maxit,
            "restart": restart, "golden": golden, "bound": bound}


def _from_golden(leg, group, world, g, pc, bound):
    tol = (fx(g["rtol"]), fx(g["atol"]), fx(g["rbtol"]))
    return [_case(leg, group, g["mat"], world, g["solver"], mode, pc, b=g["b"], x0=g["x0"], tol=tol,
                  maxit=g["maxit"], restart=g["restart"], golden=g, bound=bound) for mode, _ in MODES]


def _restart(solver, arnoldi, sl):
    return arnoldi if solver in ARNOLDI else sl if solver in SL else 30  # the others take none


def _leg_a():
    """the reference's own block-Jacobi runs, nblk = 4 = the rank count: 16^3 and 32^3"""
    out = []
    for g in GOLDEN:
        if g["pc"] == {"kind": "bj", "nblk": 4}:
            out += _from_golden("A", f"p{g['mat']['N']}", 4, g, "bj", True)
    return out


def _general(leg, group, mat, world, drivers):
    """legs B and C: default tolerances, x0 and b seeded, short restarts so that every GMRES
    driver restarts at least twice and LGMRES / RLGMRES read their Z basis"""
    out = []
    for s in drivers:
        for pc in ("bj", "none"):
            for mode, _ in MODES:
                # RLGMRES without M on the 10^3 box stops at maxit; a run that ends there is still a trace
                maxit = 200 if (mat["type"], s, pc) == ("poisson", O.RLGMRES, "none") else 300
                out.append(_case(leg, group, mat, world, s, mode, pc, b="11", x0="12", tol=(DEF_TOL,) * 3,
                                 maxit=maxit, restart=_restart(s, 5, 4)))
    return out


NOT_CG = [s for s in DRIVERS if s != O.CG]  # CG runs 300 iterations on the nonsymmetric matrices without converging


def _leg_d():
    """an empty rank: zero tolerances, no preconditioner (an ILU handle has n > 0, and every rank
    takes the same preconditioner path); the GMRES drivers run two whole cycles -- RGMRES stopped
    mid-cycle by maxit yields a NaN x by the reference's own arithmetic (solver-gmres.cxx:414-418)"""
    out = []
    for s in DRIVERS:
        for mode, _ in MODES:
            out.append(_case("D", "tri9", TRIDIAG9, 4, s, mode, "none", b="21", x0="22", tol=(0.0, 0.0, 0.0),
                             maxit=6 if s in ARNOLDI else 4, restart=_restart(s, 3, 2)))
    return out


def _leg_e():
    """the global preconditioner: each driver's first ILU(0) run on the 16^3 box with b = 1 (CG: its
    24^3 run) and its b = 0 run, where the reference has one; and, on the same two ranks, the
    reference's nblk = 2 block-Jacobi BiCGSTAB run"""
    out = []
    ilu0 = {"kind": "iluk", "level": 0}
    for s in DRIVERS:
        mine = [g for g in GOLDEN if g["solver"] == s and g["pc"] == ilu0 and g["mat"]["type"] == "poisson"
                and g["mat"]["dim"] == 3]
        ones = [g for g in mine if g["b"] == "ones" and g["mat"]["N"] == (24 if s == O.CG else 16)]
        zeros = [g for g in mine if g["b"] == "zeros"]
        out += _from_golden("E", f"p{ones[0]['mat']['N']}", 2, ones[0], "global", False)
        if zeros:
            out += _from_golden("E", f"p{zeros[0]['mat']['N']}-b0", 2, zeros[0], "global", False)
    for g in GOLDEN:
        if g["pc"] == {"kind": "bj", "nblk": 2}:
            out += _from_golden("E", f"p{g['mat']['N']}-nblk2", 2, g, "bj", True)
    return out


LEGS = {
    "A": _leg_a(),
    "B": _general("B", "rand777", RAND777, 2, NOT_CG),
    "C": _general("C", "rand1000", RAND1000, 3, NOT_CG) + _general("C", "p10", dict(POISSON, N=10), 3, DRIVERS),
    "D": _leg_d(),
    "E": _leg_e(),
}
WORLD = {leg: cs[0]["world"] for leg, cs in LEGS.items()}
ALL_CASES = [c for leg in LEGS for c in LEGS[leg]]
BJ_GOLDEN = [g for g in GOLDEN if g["pc"]["kind"] == "bj"]  # every block-Jacobi run the reference left


def groups(leg):
    """the leg's cases by (matrix, group), in table order: one handle and one preconditioner set each"""
    out = {}
    for c in LEGS[leg]:
        out.setdefault((_matkey(c["mat"]), c["group"]), []).append(c)
    return list(out.values())


# ---- what the oracle gives -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _factors(matkey: str, blk: int):
    return O.ilu(_matrix(matkey), "iluk", level=0, blk=blk)


def oracle_run(mat, solver, mode, nranks, blk, *, b, x0, tol, maxit, restart):
    """blk: None no preconditioner, 0 the ILU(0) of the whole matrix, else block-Jacobi blocks of blk rows"""
    A = matrix(mat)
    L, U = (None, None) if blk is None else _factors(_matkey(mat), blk)
    return O.solve(solver, A, vec(b, A.n), x0=None if x0 is None else vec(x0, A.n), L=L, U=U, rtol=tol[0],
                   atol=tol[1], rbtol=tol[2], maxit=maxit, restart=restart, mode=mode, nranks=nranks,
                   trace_cap=TRACE_CAP)


@functools.lru_cache(maxsize=None)
def _expected(key: str):
    c = next(c for c in ALL_CASES if c["key"] == key)
    n, P = matrix(c["mat"]).n, c["world"]
    blk = {"none": None, "global": 0, "bj": (n + P - 1) // P}[c["pc"]]
    # the global factors in SERIAL mode: the ranks continue one sequential sum, the single-process order
    nranks = 1 if (c["pc"], c["mode"]) == ("global", O.SERIAL) else P
    return oracle_run(c["mat"], c["solver"], c["mode"], nranks, blk, b=c["b"], x0=c["x0"], tol=c["tol"],
                      maxit=c["maxit"], restart=c["restart"])


def expected(c) -> O.SolveResult:
    """the oracle's P-rank run of a case; computed once and shared -- do not modify"""
    return _expected(c["key"])


def same_bits(a, b) -> bool:
    """bitwise, NaN compared as NaN"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    if a.shape != b.shape:
        return False
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


def nits_bound(ref: int) -> int:
    return max(1, ref // 20)


def check_against_golden(c, nits, residual, trace, x):
    """SERIAL: the reference's run bit for bit; TREE (where the case says so): its count within 5 %"""
    g = c["golden"]
    if g is None:
        return
    if c["mode"] == O.SERIAL:
        assert nits == g["nits"], (nits, g["nits"])
        assert same_bits(residual, fx(g["residual"])), (residual, fx(g["residual"]))
        assert matches(g["trace"], np.asarray(trace)), "trace differs from the reference's"
        assert matches(g["x"], np.asarray(x)), "x differs from the reference's"
    elif c["bound"]:
        assert abs(nits - g["nits"]) <= nits_bound(g["nits"]), (nits, g["nits"])


def check_result(c, rec):
    """one case of a leg's results against the oracle and, where there is one, the reference's run"""
    assert rec["status"] == 0, rec
    o = expected(c)
    first = rec["ranks"][0]
    for q, other in enumerate(rec["ranks"]):  # an empty rank included: the same count, residual and trace
        assert other[0] == first[0] and same_bits(other[1], first[1]) and same_bits(other[2], first[2]), \
            f"rank {q} returned another run than rank 0: {other[:2]} vs {first[:2]}"
    nits, residual, trace = first
    x = rec["x"]
    print(f"{c['key']}: nits {nits} (oracle {o.nits}), residual {residual!r} (oracle {o.residual!r}), "
          f"trace {len(trace)} (oracle {len(o.trace)})")
    assert nits == o.nits, (nits, o.nits)
    assert same_bits(residual, o.residual), (residual, o.residual)
    assert same_bits(trace, o.trace), _first_diff(trace, o.trace)
    assert same_bits(x, o.x), _first_diff(x, o.x)
    check_against_golden(c, nits, residual, trace, x)


def _first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return f"lengths {a.shape} vs {b.shape}"
    bad = np.flatnonzero(~((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))
    i = int(bad[0])
    return f"{bad.size} of {a.size} entries differ, the first at {i}: {a[i]!r} vs {b[i]!r}"


# ---- the ranks ---------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _agree(dist, bad: bool) -> bool:
    """does any rank report a failure?  Agreed on, so that the ranks stop at the same case."""
    import torch
    t = torch.tensor([1 if bad else 0])
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return bool(t.item())


def _run_cases(dev, dist, leg, rank, world):
    """this rank's part of every case of the leg, in table order: {key: record}.  An LsspError
    becomes the record of the step that raised it and ends the leg on every rank."""
    import lssp_amd
    from bench import local_block
    res = {}
    for cases in groups(leg):
        A = matrix(cases[0]["mat"])
        n = A.n
        r0, nl = rank_rows(n, world, rank)
        Ap, Aj, Ax = local_rows(A.Ap, A.Aj, A.Ax, r0, nl)
        pcs = {c["pc"] for c in cases}
        M = {"none": None}
        try:
            # the solvers take the assembled matrix, whose columns lssp_solver_assemble sorts
            # (lssp.cxx:173, include/lssp_amd.h), as the oracle's solve sorts its copy; the
            # preconditioners get the rows as generated and sort for themselves
            sp, sj, sx = lssp_amd.sort_columns(Ap, Aj, Ax, ncols=n) if nl else (Ap, Aj, Ax)
            D = lssp_amd.DMat(dev, sp, sj, sx, dist=(n, r0))
            if "bj" in pcs:  # the rank's diagonal block (pc-iluk.cxx:441-535, blk = ceil(n / P))
                M["bj"] = lssp_amd.DILU.create(dev, *local_block(Ap, Aj, Ax, r0, nl), kind=lssp_amd.ILUK, level=0)
            if "global" in pcs:  # the factors of the whole matrix on every rank (pc-iluk.cxx:574)
                M["global"] = lssp_amd.DILU.create(dev, A.Ap, A.Aj, A.Ax, kind=lssp_amd.ILUK, level=0)
            err = None
        except lssp_amd.LsspError as e:
            err = {"status": e.status, "error": f"setup of {cases[0]['group']}: {e}"}
        if _agree(dist, err is not None):
            res[cases[0]["key"]] = err or {"status": -1, "error": "another rank failed in the setup"}
            return res
        nx = D.nx
        for c in cases:
            bg, xg = vec(c["b"], n), np.zeros(n) if c["x0"] is None else vec(c["x0"], n)
            xh, bh = np.full(max(nx, 1), np.nan), np.full(max(nx, 1), np.nan)
            xh[:nl], bh[:nl] = xg[r0:r0 + nl], bg[r0:r0 + nl]
            x, b = dev.vec(max(nx, 1), xh), dev.vec(max(nx, 1), bh)
            dev.set_reduction(c["mode"])
            try:
                r = lssp_amd.solve(dev, D, M[c["pc"]], x, b, solver=c["solver"], tol_rel=c["tol"][0],
                                   tol_abs=c["tol"][1], tol_rb=c["tol"][2], maxit=c["maxit"], restart=c["restart"],
                                   bgsl=c["restart"], idrs=c["restart"], trace_cap=TRACE_CAP)
                rec = {"status": 0, "nits": r.nits, "residual": r.residual, "trace": r.trace, "x": x.download(nl)}
            except lssp_amd.LsspError as e:
                rec = {"status": e.status, "error": str(e)}
            x.free()
            b.free()
            bad = _agree(dist, rec["status"] != 0)
            if bad and rec["status"] == 0:
                rec = {"status": -1, "error": "another rank failed in this case"}
            res[c["key"]] = rec
            if bad:
                return res
        for m in M.values():
            if m is not None:
                m.close()
        D.close()
    return res


def _merge(parts):
    """the ranks' records of a case as one: x in row order, (nits, residual, trace) per rank"""
    out = {}
    for key in parts[0]:
        recs = [p[key] for p in parts]
        bad = [r for r in recs if r["status"] != 0]
        if bad:
            real = [r for r in bad if r["status"] > 0] or bad
            out[key] = {"status": real[0]["status"], "error": [r.get("error") for r in recs]}
        else:
            out[key] = {"status": 0, "x": np.concatenate([r["x"] for r in recs]),
                        "ranks": [(r["nits"], r["residual"], r["trace"]) for r in recs]}
    return out


def _worker(rank, world, port, leg, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import lssp_amd
        from lssp_amd.dist import GlooTransport
        dev = lssp_amd.Device(0)
        dev.comm_init_host(world, rank, GlooTransport())
        res = _run_cases(dev, dist, leg, rank, world)
        dev.set_reduction(lssp_amd.TREE)
        dev.barrier()
        parts = [None] * world
        dist.all_gather_object(parts, res)
        if rank == 0:
            out.put(_merge(parts))
        dev.close()
    finally:
        dist.destroy_process_group()


def _sleeping_worker(rank, world, port, leg, out):
    """a rank that never answers: what the runner's timeout path is tested with (no GPU)"""
    time.sleep(600)


def _reap(procs, join_timeout):
    """join every rank, then end whatever is still alive; the ranks that had to be ended"""
    for p in procs:
        p.join(timeout=join_timeout)
    ended = []
    for q, p in enumerate(procs):
        if p.is_alive():
            ended.append(q)
            p.terminate()
    for p in procs:
        p.join(timeout=5)
        if p.is_alive():
            p.kill()
            p.join(timeout=5)
    return ended


def spawn_leg(leg, world=None, target=_worker, timeout=QUEUE_WAIT, join_timeout=30.0):
    """Run a leg's ranks as spawned processes and wait for rank 0's dict.  Always returns, and with
    no rank process left alive: {"results": the dict or None, "wall": seconds from the first
    start to the answer, "timed_out", "exitcodes", "ended": the ranks that had to be terminated}.
    A rank that dies before the answer ends the wait early (its peers would wait in a collective)."""
    import multiprocessing as mp
    world = WORLD[leg] if world is None else world
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, leg, q)) for r in range(world)]
    t0 = time.perf_counter()
    for p in procs:
        p.start()
    got, died = None, False
    try:
        while got is None and time.perf_counter() - t0 < timeout:
            try:
                got = q.get(timeout=min(0.5, timeout))
            except queue.Empty:
                if died:  # one more look at the queue after a rank died, then give up
                    break
                died = any(p.exitcode not in (None, 0) for p in procs)
    finally:
        wall = time.perf_counter() - t0
        ended = _reap(procs, join_timeout if got is not None else min(join_timeout, 2.0))
    return {"results": got, "wall": wall, "timed_out": got is None and not died, "exitcodes": [p.exitcode for p in procs],
            "ended": ended, "pids": [p.pid for p in procs]}


def leg_ok(run):
    """the runner's own outcome: an answer, every rank gone by itself with status 0"""
    assert run["results"] is not None, f"no answer from the ranks (timed out: {run['timed_out']}, " \
        f"exit codes {run['exitcodes']}, ended by the runner: {run['ended']})"
    assert not run["ended"] and all(e == 0 for e in run["exitcodes"]), (run["exitcodes"], run["ended"])


def case_record(run, c):
    """a case's record from a leg's run; a case the leg never reached fails, naming the one that stopped it"""
    leg_ok(run)
    res = run["results"]
    if c["key"] not in res:
        stopped = [(k, r) for k, r in res.items() if r["status"] != 0]
        raise AssertionError(f"{c['key']} did not run: the leg stopped at {stopped[0][0] if stopped else '?'}: "
                             f"{stopped[0][1] if stopped else res.keys()}")
    return res[c["key"]]
