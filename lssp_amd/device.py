"""Thin Python handles over the C-ABI (device context, vectors, CSR, ILU, solve).

Everything computes in lssp_amd/lib/liblssp_amd.so on the GPU; this module
only moves numpy arrays across the boundary and turns status codes into
exceptions (the reference would lssp_error() -> exit(1), utils.cxx:114-135).
"""
from __future__ import annotations

import ctypes
import weakref
from dataclasses import dataclass

import numpy as np

from . import _lib

GMRES, LGMRES, RGMRES, BICGSTAB, CG = 0, 1, 2, 4, 7
BICGSAFE, CGS, GPBICG, CR, CRS, BICRSTAB, BICRSAFE, GPBICR, QMRCGSTAB, TFQMR, ORTHOMIN = (
    6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17)  # LSSP_SOLVER_TYPE (type-defs.h:157-178)
BICGSTABL, IDRS = 5, 18
RLGMRES = 3                        # right-preconditioned LGMRES (lssp_solver_lgmres_r)
ILUK, ILUT, BILUK = 1, 2, 3        # LSSP_PC_TYPE (type-defs.h:63-101)
SERIAL, TREE = 0, 1                # reduction order


class LsspError(RuntimeError):
    def __init__(self, status: int, what: str):
        msg = _lib.load().lssp_amd_strerror(status).decode()
        super().__init__(f"{what}: {msg} (status {status})")
        self.status = status


def _ck(status: int, what: str):
    if status != 0:
        raise LsspError(status, what)


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Device:
    """One GPU context (device + HIP stream + reduction scratch)."""

    def __init__(self, device: int = 0, reduction: int = TREE):
        self.L = _lib.load()
        h = ctypes.c_void_p()
        _ck(self.L.lssp_amd_ctx_create(device, ctypes.byref(h)), "ctx_create")
        self.h = h
        self._children = weakref.WeakSet()  # closed before the context goes away
        self.set_reduction(reduction)

    def _adopt(self, obj):
        self._children.add(obj)
        return obj

    def set_reduction(self, mode: int):
        _ck(self.L.lssp_amd_ctx_set_reduction(self.h, mode), "set_reduction")
        self.reduction = mode

    def sync(self):
        _ck(self.L.lssp_amd_ctx_sync(self.h), "sync")

    @property
    def stream(self) -> int:
        return self.L.lssp_amd_ctx_stream(self.h) or 0

    def close(self):
        if self.h:
            for child in list(self._children):
                child.close()
            self.L.lssp_amd_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- vectors ----------------------------------------------------------
    def vec(self, n: int, data=None) -> "DVec":
        v = DVec(self, n)
        if data is not None:
            v.upload(data)
        return v

    def idx(self, n: int, data=None) -> "DIdx":
        v = DIdx(self, n)
        if data is not None:
            v.upload(data)
        return v

    # ---- comm ------------------------------------------------------------------
    def comm_init(self, nranks: int, rank: int, uid: bytes):
        buf = ctypes.create_string_buffer(uid, len(uid))
        _ck(self.L.lssp_amd_comm_init(self.h, nranks, rank, buf), "comm_init")

    def comm_init_host(self, nranks: int, rank: int, transport):
        """multi-rank protocol over a host-staged transport (e.g. lssp_amd.dist.GlooTransport)"""
        self._transport = transport  # keeps the ctypes callbacks alive
        _ck(self.L.lssp_amd_comm_init_host(self.h, nranks, rank, ctypes.byref(transport.struct)),
            "comm_init_host")

    def barrier(self):
        _ck(self.L.lssp_amd_comm_barrier(self.h), "barrier")

    def comm_nranks(self) -> int:
        """the communicator's rank count (ncclCommCount on RCCL; the host transport's count)"""
        v = ctypes.c_int()
        _ck(self.L.lssp_amd_comm_nranks(self.h, ctypes.byref(v)), "comm_nranks")
        return v.value

    def comm_selftest(self):
        """all-gather + grouped send/recv ring through the configured transport, checked"""
        _ck(self.L.lssp_amd_comm_selftest(self.h), "comm_selftest")


def comm_unique_id() -> bytes:
    L = _lib.load()
    n = L.lssp_amd_comm_unique_id_size()
    buf = ctypes.create_string_buffer(n)
    _ck(L.lssp_amd_comm_get_unique_id(buf), "get_unique_id")
    return buf.raw


class DVec:
    """A device fp64 vector (lssp_vec with d in HBM)."""

    def __init__(self, dev: Device, n: int):
        self.dev, self.n = dev, int(n)
        p = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_vec_alloc(dev.h, self.n, ctypes.byref(p)), "vec_alloc")
        self.ptr = p
        dev._adopt(self)

    def upload(self, a):
        a = _f64(a)
        assert a.size <= self.n
        _ck(self.dev.L.lssp_amd_vec_upload(self.dev.h, self.ptr, _p(a), a.size), "vec_upload")
        return self

    def download(self, n: int | None = None) -> np.ndarray:
        out = np.empty(self.n if n is None else n)
        _ck(self.dev.L.lssp_amd_vec_download(self.dev.h, _p(out), self.ptr, out.size), "vec_download")
        return out

    def free(self):
        if self.ptr:
            self.dev.L.lssp_amd_vec_free(self.dev.h, self.ptr)
            self.ptr = None

    close = free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DIdx(DVec):
    """A device int32 array (the Ap / Aj / Ai members of a matrix in HBM)."""

    def __init__(self, dev: Device, n: int):
        self.dev, self.n = dev, int(n)
        p = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_idx_alloc(dev.h, self.n, ctypes.byref(p)), "idx_alloc")
        self.ptr = p
        dev._adopt(self)

    def upload(self, a):
        a = _i32(a)
        assert a.size <= self.n
        _ck(self.dev.L.lssp_amd_idx_upload(self.dev.h, self.ptr, _p(a), a.size), "idx_upload")
        return self

    def download(self, n: int | None = None) -> np.ndarray:
        out = np.empty(self.n if n is None else n, np.int32)
        _ck(self.dev.L.lssp_amd_idx_download(self.dev.h, _p(out), self.ptr, out.size), "idx_download")
        return out

    def free(self):
        if self.ptr:
            self.dev.L.lssp_amd_idx_free(self.dev.h, self.ptr)
            self.ptr = None

    close = free


class DMat:
    """A device CSR matrix (lssp_mat_csr in HBM), entry order as given."""

    def __init__(self, dev: Device, Ap, Aj, Ax, ncols: int | None = None, dist=None):
        self.dev = dev
        Ap, Aj, Ax = _i32(Ap), _i32(Aj), _f64(Ax)
        h = ctypes.c_void_p()
        if dist is None:
            n = Ap.size - 1
            ncols = n if ncols is None else ncols
            _ck(dev.L.lssp_amd_mat_upload(dev.h, n, ncols, int(Ap[-1]), _p(Ap), _p(Aj), _p(Ax),
                                          ctypes.byref(h)), "mat_upload")
        else:
            n_global, row0 = dist
            _ck(dev.L.lssp_amd_mat_upload_dist(dev.h, n_global, row0, Ap.size - 1, _p(Ap), _p(Aj), _p(Ax),
                                               ctypes.byref(h)), "mat_upload_dist")
        self._adopt_handle(dev, h, int(Ap[-1]))

    def _adopt_handle(self, dev: Device, h, nnz: int):
        self.dev, self.h = dev, h
        dev._adopt(self)
        r0, nl, nh = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        dev.L.lssp_amd_mat_local_rows(h, ctypes.byref(r0), ctypes.byref(nl), ctypes.byref(nh))
        self.row0, self.nrows, self.nhalo = r0.value, nl.value, nh.value
        self.nnz = nnz

    @classmethod
    def from_device(cls, dev: Device, nrows: int, ncols: int, nnz: int, Ap: "DIdx", Aj: "DIdx", Ax: "DVec"):
        """The handle of a CSR that already lives in HBM (lssp_amd_mat_from_device): equal to
        DMat(dev, Ap, Aj, Ax) of the same arrays; it owns copies, so Ap / Aj / Ax may be freed."""
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_mat_from_device(dev.h, nrows, ncols, nnz, Ap.ptr, Aj.ptr, Ax.ptr, ctypes.byref(h)),
            "mat_from_device")
        self = cls.__new__(cls)
        self._adopt_handle(dev, h, int(nnz))
        return self

    @classmethod
    def from_device_dist(cls, dev: Device, n_global: int, row0: int, nlocal: int, nnz: int, Ap: "DIdx", Aj: "DIdx",
                         Ax: "DVec"):
        """The distributed handle of local rows [row0, row0 + nlocal) that already live in HBM with
        GLOBAL columns (lssp_amd_mat_from_device_dist): equal to DMat(dev, Ap, Aj, Ax, dist=(n_global,
        row0)) of the same arrays; collective, canonical partition only.  It owns copies, so Ap / Aj /
        Ax may be freed."""
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_mat_from_device_dist(dev.h, n_global, row0, nlocal, nnz, Ap.ptr, Aj.ptr, Ax.ptr,
                                                ctypes.byref(h)), "mat_from_device_dist")
        self = cls.__new__(cls)
        self._adopt_handle(dev, h, int(nnz))
        return self

    def local_block(self) -> "DMat":
        """The rank's diagonal block as a single-rank handle (lssp_amd_mat_local_block): the entries
        whose column this rank owns, in this handle's entry order; equal to DMat(dev, bp, bj, bx) of the
        block cut out on the host.  What DILU.pc_create_dev / bilu_create_dev take for the rank's
        block-Jacobi factor."""
        h = ctypes.c_void_p()
        _ck(self.dev.L.lssp_amd_mat_local_block(self.dev.h, self.h, ctypes.byref(h)), "mat_local_block")
        n = ctypes.c_int()
        _ck(self.dev.L.lssp_amd_mat_info(h, None, None, ctypes.byref(n)), "mat_info")
        B = type(self).__new__(type(self))
        B._adopt_handle(self.dev, h, n.value)
        return B

    def refresh_block(self, A: "DMat"):
        """On a handle from A.local_block(): its values again from the values A holds now
        (lssp_amd_mat_local_block_refresh), finished as update_values() finishes.  An A whose owned
        entries per row differ, or a distributed self, raises LsspError with status 1 and leaves self
        as it was."""
        _ck(self.dev.L.lssp_amd_mat_local_block_refresh(self.dev.h, self.h, A.h), "mat_local_block_refresh")

    @property
    def nx(self) -> int:
        """length a vector multiplied by this matrix must have (owned + halo)"""
        return self.nrows + self.nhalo

    @property
    def ndiag(self) -> int:
        """> 0: the SpMV reads 1-byte diagonal ids (that many offsets) instead of columns"""
        v, w = ctypes.c_int(), ctypes.c_int()
        _ck(self.dev.L.lssp_amd_mat_layout(self.h, ctypes.byref(v), ctypes.byref(w)), "mat_layout")
        return v.value

    @property
    def rowcodes(self) -> int:
        """> 0: the SpMV reads one pattern byte per row (that many patterns) instead of the
        row pointers and the ids"""
        v = ctypes.c_int()
        _ck(self.dev.L.lssp_amd_mat_rowcodes(self.h, ctypes.byref(v)), "mat_rowcodes")
        return v.value

    @property
    def valcodes(self) -> int:
        """> 0: the SpMV reads one value-row byte per row (that many distinct rows: pattern and
        values, bit for bit) and no matrix values"""
        v = ctypes.c_int()
        _ck(self.dev.L.lssp_amd_mat_valcodes(self.h, ctypes.byref(v)), "mat_valcodes")
        return v.value

    @property
    def windowed(self) -> bool:
        """the SpMV stages each 1024-row block's x span in LDS (k_spmv_win)"""
        v, w = ctypes.c_int(), ctypes.c_int()
        _ck(self.dev.L.lssp_amd_mat_layout(self.h, ctypes.byref(v), ctypes.byref(w)), "mat_layout")
        return bool(w.value)

    @property
    def device_bytes(self) -> tuple[int, int]:
        """(resident CSR bytes, bytes of the SpMV layouts beside it)"""
        c, a = ctypes.c_longlong(), ctypes.c_longlong()
        _ck(self.dev.L.lssp_amd_mat_bytes(self.h, ctypes.byref(c), ctypes.byref(a)), "mat_bytes")
        return c.value, a.value

    def update_values(self, ax: DVec):
        """New values (a device vector of nnz entries, in the handle's entry order) on the
        same pattern: lssp_amd_mat_update_values.  Every layout is kept; the value codes
        (valcodes) are rebuilt for the new values, or dropped.  On a distributed handle the call is
        local to the rank (no collective) and there are no value codes to rebuild."""
        _ck(self.dev.L.lssp_amd_mat_update_values(self.dev.h, self.h, ax.ptr, ax.n), "mat_update_values")

    def close(self):
        if self.h:
            self.dev.L.lssp_amd_mat_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # mvops.h:9-19
    def mv_amxpby(self, alpha, x: DVec, beta, y: DVec):
        _ck(self.dev.L.lssp_amd_mv_amxpby(self.dev.h, alpha, self.h, x.ptr, beta, y.ptr), "mv_amxpby")

    def mv_amxpbyz(self, alpha, x: DVec, beta, y: DVec, z: DVec):
        _ck(self.dev.L.lssp_amd_mv_amxpbyz(self.dev.h, alpha, self.h, x.ptr, beta, y.ptr, z.ptr), "mv_amxpbyz")

    def mv_amxy(self, a, x: DVec, y: DVec):
        _ck(self.dev.L.lssp_amd_mv_amxy(self.dev.h, a, self.h, x.ptr, y.ptr), "mv_amxy")

    def mv_mxy(self, x: DVec, y: DVec):
        _ck(self.dev.L.lssp_amd_mv_mxy(self.dev.h, self.h, x.ptr, y.ptr), "mv_mxy")


class DILU:
    """Device ILU factors + their sync-free trisolve schedules (LSSP_PC.L/.U)."""

    def __init__(self, dev: Device, handle):
        self.dev, self.h = dev, handle
        dev._adopt(self)
        n, nl, nu, ll, lu, ts = (ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(),
                                 ctypes.c_int(), ctypes.c_double())
        dev.L.lssp_amd_ilu_info(handle, ctypes.byref(n), ctypes.byref(nl), ctypes.byref(nu),
                                ctypes.byref(ll), ctypes.byref(lu), ctypes.byref(ts))
        self.n, self.nnzL, self.nnzU = n.value, nl.value, nu.value
        self.levelsL, self.levelsU, self.setup_seconds = ll.value, lu.value, ts.value

    def sweep_layout(self):
        """(line sweeps: 0 none, 1 ILU(0) grid, 2 ILU(1) grid; tile lines, tile planes)
        -- lssp_amd_ilu_sweep_layout."""
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _ck(self.dev.L.lssp_amd_ilu_sweep_layout(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
            "ilu_sweep_layout")
        return a.value, b.value, c.value

    @classmethod
    def create(cls, dev: Device, Ap, Aj, Ax, kind=ILUK, level=0, tol=1e-3, p=-1, blk=0):
        Ap, Aj, Ax = _i32(Ap), _i32(Aj), _f64(Ax)
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_ilu_create(dev.h, kind, Ap.size - 1, _p(Ap), _p(Aj), _p(Ax), level, tol, p, blk,
                                      ctypes.byref(h)), "ilu_create")
        return cls(dev, h)

    @classmethod
    def create_dev(cls, dev: Device, A: DMat, kind=ILUK, level=0, tol=1e-3, p=-1, blk=0):
        """create() for a matrix that lives in HBM (lssp_amd_ilu_create_dev): the tiled
        line-sweep ILU(0) of a natural-order 5-/7-point box, built on the device from A's
        arrays and bitwise create()'s handle; refactor() is eligible on it at once.  Rows must
        be column-sorted.  Anything else raises LsspError with status 6 (unsupported) and
        leaves A as it was: use create() there."""
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_ilu_create_dev(dev.h, A.h, kind, level, tol, p, blk, ctypes.byref(h)), "ilu_create_dev")
        return cls(dev, h)

    @classmethod
    def iluk_create_dev(cls, dev: Device, A: DMat, kind=ILUK, level=-1, tol=1e-3, p=-1, blk=0):
        """create() for a matrix that lives in HBM, at the reference's default level too
        (lssp_amd_iluk_create_dev): what create_dev() serves goes there unchanged; level 1 (or
        < 0, the default) makes the ILU(1) of a complete natural-order 7-point box (nx, ny >= 3,
        nz >= 2) or 5-point grid (nx, ny >= 3) on the skewed line sweeps, sweep_layout() ==
        (2, 16, 8), on the device and bitwise create(level=1)'s handle; iluk_refactor() is
        eligible on it at once.  Rows must be column-sorted.  ILUT, level >= 2, block-Jacobi,
        nx == 2, a small 2-D grid on the one-workgroup sweeps, LSSP_AMD_LINE=0 and any matrix
        that is no such box raise LsspError with status 6 (unsupported) and leave A as it was:
        use create() there."""
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_iluk_create_dev(dev.h, A.h, kind, level, tol, p, blk, ctypes.byref(h)), "iluk_create_dev")
        return cls(dev, h)

    @classmethod
    def ilut_create_dev(cls, dev: Device, A: DMat, tol=1e-3, p=-1, blk=0):
        """create(kind=ILUT) for a matrix that lives in HBM (lssp_amd_ilut_create_dev): ILUT(tol,
        p) factored on the device, a wavefront per row, bitwise create()'s handle.  A's arrays
        stay in HBM, and so do the finished factors: the sweeps' schedules are built on the device
        (schedule(w)["origin"] == 1) and factors() downloads them on first use.  Rows
        must be column-sorted and hold their diagonal.  Block-Jacobi, an unsorted row, a repeated
        column, a missing diagonal and a working row beyond ilut_capacity() entries on a side
        raise LsspError with status 6 (unsupported) and leave A as it was: use create() there."""
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_ilut_create_dev(dev.h, A.h, tol, p, blk, ctypes.byref(h)), "ilut_create_dev")
        return cls(dev, h)

    @staticmethod
    def ilut_capacity() -> int:
        """entries a working row of ilut_create_dev() may hold on each side of the diagonal"""
        from . import _lib
        return _lib.load().lssp_amd_ilut_capacity()

    @classmethod
    def pc_create_dev(cls, dev: Device, A: DMat, kind=ILUK, level=-1, tol=1e-3, p=-1, blk=0):
        """One call for every handle made from a matrix that lives in HBM (lssp_amd_pc_create_dev).
        kind=ILUT is ilut_create_dev().  kind=ILUK first tries iluk_create_dev(): a complete box
        keeps its line sweeps.  Anything that refuses -- a thermal-like matrix, an irregular mesh, a
        box with holes, level >= 2, nx == 2 -- takes the general route: the symbolic ILU(level)
        runs on the device, a wavefront per row, the values go through iluk_refactor()'s kernels,
        and the packet schedules are built on the device (schedule(w)["origin"] == 1;
        sweep_layout() == (0, 0, 0)); bitwise create(level=level)'s handle, and iluk_refactor()
        is eligible on it at once.  Rows must be column-sorted and hold their diagonal.
        Block-Jacobi, an unsorted row, a repeated column, a missing diagonal, a working row beyond
        ilut_capacity() entries on a side and level > 254 raise LsspError with status 6
        (unsupported) and leave A as it was: use create() there."""
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_pc_create_dev(dev.h, A.h, kind, level, tol, p, blk, ctypes.byref(h)), "pc_create_dev")
        return cls(dev, h)

    @classmethod
    def from_factors(cls, dev: Device, L, U):
        Lp, Lj, Lx = _i32(L[0]), _i32(L[1]), _f64(L[2])
        Up, Uj, Ux = _i32(U[0]), _i32(U[1]), _f64(U[2])
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_ilu_from_factors(dev.h, Lp.size - 1, _p(Lp), _p(Lj), _p(Lx), _p(Up), _p(Uj), _p(Ux),
                                            ctypes.byref(h)), "ilu_from_factors")
        return cls(dev, h)

    @classmethod
    def from_factors_dev(cls, dev: Device, L, U):
        """from_factors() for factors that live in HBM (lssp_amd_ilu_from_factors_dev): L and U are
        (DIdx, DIdx, DVec) triples, L with its diagonal last in each row, U with its pivot first.
        Both packet schedules are built on the device; no factor array crosses to the host, and
        the handle owns copies, so the arrays may be freed.  Always on the packet sweeps
        (sweep_layout() == (0, 0, 0)); bitwise from_factors() otherwise.  A strict row beyond 24
        entries or a schedule beyond the packet limits raises LsspError with status 6
        (unsupported): use from_factors() there; malformed factors raise status 1."""
        n = L[0].n - 1
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_ilu_from_factors_dev(dev.h, n, L[0].ptr, L[1].ptr, L[2].ptr, U[0].ptr, U[1].ptr, U[2].ptr,
                                                ctypes.byref(h)), "ilu_from_factors_dev")
        return cls(dev, h)

    _SCHED_HDR = ("B", "nb", "nsteps", "npackets", "EP", "EXT", "rows", "rec_words", "idx_words", "unit", "nlevels",
                  "origin")

    def schedule(self, which: int):
        """The packet schedule of the L (which = 0) or U (1) sweep (lssp_amd_ilu_get_schedule): a
        dict of the header fields (B, nb, nsteps, npackets, EP, EXT, rows, rec_words, idx_words,
        unit, nlevels, origin -- 0 built on the host, 1 on the device) and the arrays blk, desc,
        rec, idx, perm, pos.  A handle on line sweeps or on the sync-free fallback raises
        LsspError with status 6 (unsupported)."""
        hdr = np.zeros(12, np.int32)
        _ck(self.dev.L.lssp_amd_ilu_get_schedule(self.h, which, _p(hdr), None, None, None, None, None, None),
            "ilu_get_schedule")
        s = dict(zip(self._SCHED_HDR, (int(v) for v in hdr)))
        s["blk"] = np.zeros(s["nb"] + 1, np.int32)
        s["desc"] = np.zeros(max(4 * s["npackets"], 1), np.int32)
        s["rec"] = np.zeros(s["rec_words"], np.uint32)
        s["idx"] = np.zeros(s["idx_words"], np.int32)
        s["perm"], s["pos"] = np.zeros(self.n, np.int32), np.zeros(self.n, np.int32)
        _ck(self.dev.L.lssp_amd_ilu_get_schedule(self.h, which, _p(hdr), _p(s["blk"]), _p(s["desc"]), _p(s["rec"]),
                                                 _p(s["idx"]), _p(s["perm"]), _p(s["pos"])), "ilu_get_schedule")
        return s

    @classmethod
    def bilu(cls, dev: Device, Ap, Aj, Ax, bs: int, level: int = 0):
        """BILUK: block ILU(level) on bs x bs blocks (lssp_amd_bilu_create); the numeric
        factorization runs on the GPU for bs <= 8"""
        Ap, Aj, Ax = _i32(Ap), _i32(Aj), _f64(Ax)
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_bilu_create(dev.h, Ap.size - 1, _p(Ap), _p(Aj), _p(Ax), level, bs, ctypes.byref(h)),
            "bilu_create")
        return cls(dev, h)

    @classmethod
    def bilu_create_dev(cls, dev: Device, A: DMat, bs: int, level: int = 0):
        """bilu() for a matrix that lives in HBM (lssp_amd_bilu_create_dev), bs <= 8: block graph,
        symbolic block ILU(level), numeric factorization, expansion to L and U and both packet
        schedules (schedule(w)["origin"] == 1) are made on the device, bitwise bilu()'s handle.
        A's arrays stay in HBM and A may be closed on return; factors() / diag() download on first
        use; bilu_refactor() is eligible at once and builds nothing.  Rows must be column-sorted
        and every block row must hold its diagonal block.  bs 9..32, a distributed A, an unsorted
        row, a repeated column, a block row without its diagonal block, a working block row
        beyond ilut_capacity() blocks on a side and level > 254 raise LsspError with status 6
        (unsupported) and leave A as it was: use bilu() there.  A singular diagonal block, n not
        a multiple of bs and a non-square A raise status 1."""
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_bilu_create_dev(dev.h, A.h, level, bs, ctypes.byref(h)), "bilu_create_dev")
        return cls(dev, h)

    @classmethod
    def from_ldu(cls, dev: Device, L, D, U):
        """BILUK factors as the reference leaves them in pc.L / pc.D / pc.U (D: block diagonal CSR)"""
        Lp, Lj, Lx = _i32(L[0]), _i32(L[1]), _f64(L[2])
        Dp, Dj, Dx = _i32(D[0]), _i32(D[1]), _f64(D[2])
        Up, Uj, Ux = _i32(U[0]), _i32(U[1]), _f64(U[2])
        h = ctypes.c_void_p()
        _ck(dev.L.lssp_amd_ilu_from_ldu(dev.h, Lp.size - 1, _p(Lp), _p(Lj), _p(Lx), _p(Dp), _p(Dj), _p(Dx),
                                        _p(Up), _p(Uj), _p(Ux), ctypes.byref(h)), "ilu_from_ldu")
        return cls(dev, h)

    def diag(self):
        """(bs, Dinv): the block size and the inverted diagonal blocks, block i column-major at
        Dinv[i*bs*bs:]; (0, None) for an ILUK / ILUT handle"""
        bs = ctypes.c_int()
        _ck(self.dev.L.lssp_amd_ilu_get_diag(self.h, ctypes.byref(bs), None), "ilu_get_diag")
        if bs.value == 0:
            return 0, None
        Dinv = np.zeros(self.n * bs.value)
        _ck(self.dev.L.lssp_amd_ilu_get_diag(self.h, ctypes.byref(bs), _p(Dinv)), "ilu_get_diag")
        return bs.value, Dinv

    def factors(self):
        n = self.n
        Lp, Lj, Lx = np.zeros(n + 1, np.int32), np.zeros(self.nnzL, np.int32), np.zeros(self.nnzL)
        Up, Uj, Ux = np.zeros(n + 1, np.int32), np.zeros(self.nnzU, np.int32), np.zeros(self.nnzU)
        _ck(self.dev.L.lssp_amd_ilu_get_factors(self.h, _p(Lp), _p(Lj), _p(Lx), _p(Up), _p(Uj), _p(Ux)),
            "ilu_get_factors")
        return (Lp, Lj, Lx), (Up, Uj, Ux)

    def refactor(self, A: DMat):
        """Factor again from the values A holds now, keeping the sweep schedules
        (lssp_amd_ilu_refactor): the tiled line-sweep ILU(0) of a 5-/7-point grid only; any
        other handle raises LsspError with status 6 (unsupported) and stays as it was."""
        _ck(self.dev.L.lssp_amd_ilu_refactor(self.dev.h, self.h, A.h), "ilu_refactor")

    def bilu_refactor(self, A: DMat):
        """Factor a BILUK handle again from the values A holds now, on the block pattern it
        was created with (lssp_amd_bilu_refactor): bs <= 8 handles on the packet sweeps; A
        must have the creating matrix's block graph (status 1 otherwise, or for a singular
        diagonal block); any other handle raises LsspError with status 6 (unsupported).  The
        handle stays as it was in every such case."""
        _ck(self.dev.L.lssp_amd_bilu_refactor(self.dev.h, self.h, A.h), "bilu_refactor")

    def iluk_refactor(self, A: DMat):
        """Factor any one-block ILUK handle again from the values A holds now, keeping every
        schedule (lssp_amd_iluk_refactor): what refactor() serves, plus handles on the packet
        sweeps and on the skewed ILU(1) line sweeps, at any level.  A must have the creating
        matrix's (column-sorted) pattern exactly (status 1 otherwise); any other handle raises
        LsspError with status 6 (unsupported).  The handle stays as it was in every such case."""
        _ck(self.dev.L.lssp_amd_iluk_refactor(self.dev.h, self.h, A.h), "iluk_refactor")

    def apply(self, x: DVec, rhs: DVec):
        """x = U^-1 L^-1 rhs (lssp_pc_ilu_solve, solver-tri.cxx:57-60)"""
        _ck(self.dev.L.lssp_amd_ilu_apply(self.dev.h, self.h, x.ptr, rhs.ptr), "ilu_apply")

    def apply_async(self, x: DVec, rhs: DVec):
        """the apply enqueued without waiting (lssp_amd_ilu_apply_async); check() reports timeouts"""
        _ck(self.dev.L.lssp_amd_ilu_apply_async(self.dev.h, self.h, x.ptr, rhs.ptr), "ilu_apply_async")

    def check(self):
        _ck(self.dev.L.lssp_amd_ilu_check(self.dev.h, self.h), "ilu_check")

    def trisolve(self, which: int, x: DVec, rhs: DVec):
        _ck(self.dev.L.lssp_amd_ilu_trisolve(self.dev.h, self.h, which, x.ptr, rhs.ptr), "ilu_trisolve")

    def close(self):
        if self.h:
            self.dev.L.lssp_amd_ilu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class Result:
    nits: int
    residual: float
    trace: np.ndarray


def solve(dev: Device, A: DMat, M: DILU | None, x: DVec, b: DVec, solver=BICGSTAB, tol_rel=1e-7,
          tol_abs=1e-7, tol_rb=1e-7, maxit=1000, restart=-1, verb=0, trace_cap=0, aug_k=3, bgsl=4,
          idrs=4) -> Result:
    prm = _lib.SolveParams(solver, tol_rel, tol_abs, tol_rb, maxit, restart, verb, aug_k, bgsl, idrs)
    it, res, tl = ctypes.c_int(), ctypes.c_double(), ctypes.c_int()
    tr = np.zeros(max(trace_cap, 1))
    _ck(dev.L.lssp_amd_solve(dev.h, A.h, M.h if M is not None else None, ctypes.byref(prm), x.ptr, b.ptr,
                             ctypes.byref(it), ctypes.byref(res), _p(tr) if trace_cap else None, trace_cap,
                             ctypes.byref(tl)), "solve")
    return Result(it.value, res.value, tr[: min(tl.value, trace_cap)].copy() if trace_cap else np.zeros(0))


def poisson(dim: int, N: int, row0: int = 0, nrows: int | None = None):
    """Rows [row0, row0+nrows) of the 5-pt (dim 2, exam.cxx:4-59) / 7-pt Laplacian."""
    L = _lib.load()
    n = N ** dim
    nrows = n - row0 if nrows is None else nrows
    cap = min(7 if dim == 3 else 5, 7) * nrows
    Ap = np.zeros(nrows + 1, np.int32)
    Aj = np.zeros(cap, np.int32)
    Ax = np.zeros(cap)
    _ck(L.lssp_amd_poisson_rows(dim, N, row0, nrows, _p(Ap), _p(Aj), _p(Ax)), "poisson_rows")
    nnz = int(Ap[-1])
    return Ap, Aj[:nnz].copy(), Ax[:nnz].copy()


def bilu_factor_host(Ap, Aj, Ax, bs: int, level: int = 0):
    """BILUK's factors by the host path, without a GPU (lssp_amd_bilu_factor_host):
    ((Lp, Lj, Lx), Dinv, (Up, Uj, Ux))."""
    L = _lib.load()
    Ap, Aj, Ax = _i32(Ap), _i32(Aj), _f64(Ax)
    n = Ap.size - 1
    nl, nu = ctypes.c_int(), ctypes.c_int()
    _ck(L.lssp_amd_bilu_factor_host(n, _p(Ap), _p(Aj), _p(Ax), level, bs, ctypes.byref(nl), ctypes.byref(nu),
                                    None, None, None, None, None, None, None), "bilu_factor_host")
    Lp, Lj, Lx = np.zeros(n + 1, np.int32), np.zeros(nl.value, np.int32), np.zeros(nl.value)
    Up, Uj, Ux = np.zeros(n + 1, np.int32), np.zeros(nu.value, np.int32), np.zeros(nu.value)
    Dinv = np.zeros(n * bs)
    _ck(L.lssp_amd_bilu_factor_host(n, _p(Ap), _p(Aj), _p(Ax), level, bs, ctypes.byref(nl), ctypes.byref(nu),
                                    _p(Lp), _p(Lj), _p(Lx), _p(Dinv), _p(Up), _p(Uj), _p(Ux)), "bilu_factor_host")
    return (Lp, Lj, Lx), Dinv, (Up, Uj, Ux)


def sort_columns(Ap, Aj, Ax, ncols=None):
    """lssp_mat_sort_column (matrix-utils.cxx:387-481) on host arrays, in place on copies."""
    Ap, Aj, Ax = _i32(Ap).copy(), _i32(Aj).copy(), _f64(Ax).copy()
    n = Ap.size - 1
    _ck(_lib.load().lssp_amd_csr_sort_columns(n, n if ncols is None else ncols, _p(Ap), _p(Aj), _p(Ax)),
        "sort_columns")
    return Ap, Aj, Ax
