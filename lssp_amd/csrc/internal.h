// internal.h -- shared state of the lssp_amd library (not part of the C-ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lssp_amd.h"
#include "sched_dev.h"  // BP_RING, PK3_*, pk6_xs_off: shared with the device schedule builder

namespace lssp_amd {

// ---- canonical reduction layout ------------------------------
constexpr int CHUNK = 256;       // level 1: one aligned chunk of 256 elements per partial
constexpr int L2_LANES = 1024;   // level 2: one workgroup, lane t sums partials t, t+1024, ...
constexpr int MAX_SLOTS = 4;     // partial sums one pass can produce
constexpr int NSCAL = 4096;      // device scalar slots per context

// sync-free trisolve: the value-as-flag "not yet computed" pattern (a NaN payload
// no arithmetic produces)
constexpr uint64_t TRI_SENTINEL = 0xFFF7DEADBEEFCAFEull;

// scalar slots of the Krylov drivers (device memory, ctx->d_scal)
enum Scal {
    S_RHO0 = 0, S_RHO1, S_ALPHA, S_BETA, S_OMEGA, S_RES, S_SNORM, S_BREAK, S_BNORM, S_TMP,
    S_DONE, S_TOL, S_NIT,  // batched iterations (solvers.cpp Run::batches: bicgstab, cg): stop flag, tolerance, iterations run
    S_SUM0 = 16,   // raw reduced sums of the last reduction
    S_H = 32,      // GMRES Hessenberg column (up to NSCAL - 32 entries); batched residual history ring
    S_HB = 64,     // ... of S_HB entries: iteration k's residual at S_H + k % S_HB (two batches in flight)
};

// finalize programs run by one lane after a reduction (same code for every
// reduction mode, so the scalar recurrences are bit-identical across modes)
enum FinOp {
    FIN_STORE = 0,       // scal[dst[k]] = sum[k]
    FIN_NORM,            // scal[dst[0]] = sqrt(sum[0])
    FIN_BICG_RHO,        // rho1 = s0; beta = (rho1*alpha)/(rho0*omega); rho0 = rho1
    FIN_BICG_ALPHA,      // alpha = rho1 / s0
    FIN_BICG_S,          // snorm = sqrt(s0); break = snorm <= 1e-40
    FIN_BICG_OMEGA,      // omega = s0 / s1
    FIN_BICG_RES_RHO,    // res = sqrt(s0); then FIN_BICG_RHO on s1
    FIN_BICG_RES_RHO_B,  // FIN_BICG_RES_RHO, then res -> history S_H + nit % S_HB, nit += 1, done = 2 breakdown
                         // (S_BREAK), 1 res <= tol, 3 the next iteration's rho1 == 0
    FIN_CG_RHO,          // rho1 = s0; beta = rho1 / rho0
    FIN_CG_ALPHA,        // alpha = rho1 / s0; rho0 = rho1
    FIN_CG_RES,          // res = sqrt(s0)
    FIN_CG_RES_RHO,      // res = sqrt(s0); rho1 = s0; beta = rho1/rho0  (PC_NON: z == r)
    FIN_CG_RES_RHO_B,    // FIN_CG_RES_RHO, then res -> history S_H + nit % S_HB, nit += 1, done = res <= tol
    FIN_BICG_S_OMEGA,    // sums (t.s, t.t, s.s): FIN_BICG_S on s2 (traced at tpos[2]), then FIN_BICG_OMEGA
};

struct Fin {
    int op = FIN_STORE;
    int nsum = 1;
    int dst[MAX_SLOTS] = {S_SUM0, S_SUM0 + 1, S_SUM0 + 2, S_SUM0 + 3};
    int tpos[3] = {-1, -1, -1};  // trace positions of the (up to three) traced values
};

}  // namespace lssp_amd

struct lssp_amd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int reduce_mode = LSSP_AMD_REDUCE_TREE;
    int num_cus = 256;
    // reduction scratch
    double *d_part = nullptr;  // [MAX_SLOTS][part_cap] level-1 partials
    long part_cap = 0;
    double *d_sums = nullptr;  // [MAX_SLOTS] rank-local sums
    double *d_wsum = nullptr;  // [MAX_SLOTS][16] level-2 wave sums (k_reduce2m)
    unsigned *d_rcnt = nullptr;  // level-2 arrival counter (k_reduce2m), 0 between launches
    double *d_scal = nullptr;  // [NSCAL] scalar slots
    double *h_scal = nullptr;  // pinned mirror
    double *d_trace = nullptr; // device trace buffer
    long trace_cap = 0;
    int *d_err = nullptr;      // error word (trisolve timeouts)
    // batched iterations: the stream copies each batch's scalars and error word
    // into snapshot k (pinned) and records ev_snap[k], so the host reads batch
    // j while batch j + 1 runs (solvers.cpp Run::batches)
    double *h_snap = nullptr;  // [2][S_H + S_HB]
    int *h_snap_err = nullptr; // [2]
    hipEvent_t ev_snap[2] = {nullptr, nullptr};
    // while set: every k_ew / k_spmv3 / reduction launch returns at once when
    // *guard != 0 (batched iterations past the one that converged)
    const double *guard = nullptr;
    // multi-GPU (RCCL)
    int nranks = 1, rank = 0;
    void *comm = nullptr;      // ncclComm_t
    lssp_amd_host_transport host{};  // host-staged transport (comm == nullptr, nranks > 1)
    double *d_gather = nullptr;  // [nranks][MAX_SLOTS]
    double *d_carry = nullptr;   // [MAX_SLOTS] serial mode: running sums of the ranks before this one
    int *d_igather = nullptr;    // [1 + nranks] comm_gather_int scratch (allocated with the communicator)
    // RCCL mode: the halo round runs on comm_stream while the interior rows'
    // product runs on stream (ev_pack: send buffer packed; ev_halo: halo landed)
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_pack = nullptr, ev_halo = nullptr;
    int tri_blocks_per_cu = 1;  // the sync-free sweep's grid (k_trisolve)
    // Krylov work vectors, kept across solves (no hipMalloc on the solve path)
    struct WsBuf {
        double *p;
        long n;
        bool used;
    };
    std::vector<WsBuf> pool;
};

struct lssp_amd_mat {
    lssp_amd_ctx *ctx = nullptr;
    int nrows = 0, ncols = 0, nnz = 0;  // local rows; ncols = local column space (owned + halo)
    int *Ap = nullptr, *Aj = nullptr;
    double *Ax = nullptr;
    // diagonal-id column coding (SpMV): when the rows use at most 255 distinct
    // offsets col - row (stencil matrices), Ad[k] indexes d_off and the SpMV
    // reads one byte per entry instead of Aj's four; ndiag == 0: not coded
    uint8_t *Ad = nullptr;
    int *d_off = nullptr;
    int ndiag = 0;
    int max_off = 0;  // max |col - row| of the coded offsets
    // row coding (SpMV): when an offset-coded matrix has rows of at most 8
    // entries in at most ROWPAT_MAX distinct patterns (a row's ids in CSR
    // order; a 7-pt grid has 27), Ac[i] indexes d_pat and the SpMV reads one
    // byte per row instead of Ap's four and Ad's byte per entry.  Pattern key:
    // byte k = id of entry k, plus 1 (0: no entry k); d_pat is ascending, so
    // the patterns' lengths ascend with the code and pat_thr[l] = number of
    // patterns shorter than l + 1 entries gives a code's length without the
    // table (build_row_codes, convert.hip); npat == 0: not row-coded
    uint8_t *Ac = nullptr;
    unsigned long long *d_pat = nullptr;
    int npat = 0;
    unsigned short pat_thr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // value coding (SpMV): when a row-coded matrix has at most ROWVAL_MAX
    // distinct rows -- pattern code plus the bit patterns of the row's values
    // in CSR order (a constant-coefficient 7-pt grid has 27) -- Av[i] indexes
    // the table d_val and the SpMV reads one byte per row and no Ax.  d_val
    // holds 9 rows of nval 64-bit words: word c of row 0 = the pattern key of
    // value row c (as in d_pat), of row 1 + k = the bits of its value k (+0.0
    // past its length).  The value rows are numbered by ascending (pattern
    // code, value bits in order), so lengths still ascend with the code and
    // val_thr is pat_thr's counterpart (build_val_codes, convert.hip, which
    // compares every row bit for bit with the table row it assigns).  d_voff
    // is the table's patterns decoded for the kernel, 9 rows of nval ints:
    // word c of row k = the column offset of value row c's entry k (past its
    // length: of its last entry again; an empty row's: 0), of row 8 = its
    // length.  nval == 0: not value-coded
    uint8_t *Av = nullptr;
    unsigned long long *d_val = nullptr;
    int *d_voff = nullptr;
    int nval = 0;
    unsigned short val_thr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // max |col - row| over the rows of the halo-free chunks [ich0, ich1) of a
    // distributed matrix (its whole row range on one rank: max_off)
    int max_off_int = 0;
    // windowed x (k_spmv_sell): when every 1024-row block's columns fall in a
    // span of at most WIN_CAP entries, d_win[2b], d_win[2b+1] = that span
    // [lo, hi) and the product stages x[lo, hi) in LDS; nullptr: not windowed
    int *d_win = nullptr;
    // the sliced copy of a windowed matrix that k_spmv_sell reads (build_windows):
    // each 1024-row block's rows sorted by length (stable, descending) into 16
    // slices of 64 rows; slice s keeps entry k of lane l's row at
    // s_meta[2s] + 64 k + l (s_ax) and its column, as a 16-bit offset from the
    // block's staging base (lo rounded down to even), in half (k & 1) of the
    // 32-bit word s_meta[2s] / 2 + 64 (k >> 1) + l (s_col); s_meta[2s + 1] is
    // the slice's longest row; s_row[64 w + l] = local row | length << 10 of
    // thread 64 w + l of its block
    double *s_ax = nullptr;
    uint32_t *s_col = nullptr, *s_row = nullptr;
    int *s_meta = nullptr;
    // device bytes held beside the CSR arrays (offset ids + table, row codes + table, value codes + table, window spans,
    // the sliced copy): lssp_amd_mat_bytes
    long long aux_bytes = 0;
    // k_spmv3's block streams, timed at upload (tune_spmv_streams); 0: the default 8
    int streams = 0;
    // distributed layout
    int n_global = 0, row0 = 0, nhalo = 0;
    bool dist = false;  // made by lssp_amd_mat_upload_dist (any rank count)
    // halo exchange plan: for each peer, indices (local) to send and the count to receive
    std::vector<int> send_peer, send_off, send_cnt;  // host plan
    std::vector<int> recv_peer, recv_off, recv_cnt;  // recv_off relative to the halo region
    int *d_send_idx = nullptr;
    double *d_send_buf = nullptr;
    int nsend = 0;
    // the longest run of 256-row chunks [ich0, ich1) none of whose rows reads a
    // halo column: their product does not wait for the halo round (spmv_halo)
    long ich0 = 0, ich1 = 0;
};

namespace lssp_amd {

struct TriSched {
    int n = 0, nnz = 0, nlevels = 0, unit = 0, upper = 0;
    int *perm = nullptr;   // position -> row, rows ordered by level
    int *rp = nullptr;     // [n+1] entry ranges in schedule order
    int *cols = nullptr;   // strict entries, in the reference's summation order
    double *vals = nullptr;
    double *diag = nullptr;  // per position (nullptr when unit)
    std::vector<int> level_ptr;  // host: schedule positions of each level
    int max_level_rows = 0;
    // block-pipelined schedule (tri_bp.cpp): contiguous row blocks of B >=
    // bandwidth rows in sweep order, each walked level by level by one workgroup
    int bp_B = 0, bp_nb = 0, bp_nsteps = 0;
    int *bp_perm = nullptr;  // schedule position -> row
    int *bp_pos = nullptr;   // row -> schedule position (the inverse of bp_perm)
    // packets v6 (k_tri_pk6: schedule-ordered shadow vectors between sweeps)
    int pk6_n = 0, pk6_ep = 4, pk6_rows = 256;
    int pk6_ext = 2;  // HBM operand loads per loader lane per packet (2, 3 or 4; build_packets6)
    int *pk6_blk = nullptr, *pk6_desc = nullptr, *pk6_idx = nullptr;
    uint32_t *pk6_rec = nullptr;
    mutable unsigned long long pk6_base = 0;
    unsigned long long *pk6_claim = nullptr;
    std::vector<int> h_pos;  // L factor: row -> schedule position (for the U factor's build)
    // lssp_amd_ilu_get_schedule: the streams' lengths in 4-byte words (trailing words included), whether every
    // diagonal is exactly 1.0 (unit above is set with the sync-free arrays only), and who built the schedule
    // (0: tri_bp.cpp on the host, 1: tri_sched.hip on the device)
    long pk6_nrec = 0, pk6_nidx = 0;
    int bp_unit = 0, bp_origin = 0;
};

// ---- line sweeps of structured factors (linesweep.hip, linefill.hip) ---------
// The 5-/7-point ILU(0) (kind 0, k_line2) and the 7-point ILU(1) pattern (kind
// 1, k_linef) run on tiles of NJ = 16 lines x P = 8 planes, LV = 2 levels per
// workgroup step: two compute waves, wave w owns planes 4w .. 4w+3 and runs
// one level later per w, a lane one row per level.  Kind 1's lines are the
// skewed j' = j + k.  Tile (J, K) of the W x S tiles takes its inputs from
// tiles (J-1, K) and (J, K-1) through hand-off buffers in HBM; a small 2-D
// grid of either kind runs on one workgroup instead (k_lineg, g2).
enum { LT_KIN = 1, LT_JIN = 2, LT_KOUT = 4, LT_JOUT = 8, LT_SKIP = 16 };  // LT_SKIP: k_linef tile wholly off the grid
struct LineGeom {
    int nx = 0, ny = 0, nz = 0;
    std::vector<char> kin;  // plane k has its (k-1) neighbour
    bool unitL = true;
};
struct LineTile {  // one workgroup's unit of work, in its sweep's coordinates
    int j0, nj, k0, np;
    int flags;        // LT_*
    int T;            // levels (padded to a whole number of LV-level steps)
    int tk, tj;      // producer tiles of the k / j inputs (-1: none)
    int ut;           // L sweep: the mirror U tile (its rhs stream)
    long long cbase;  // first row of the tile in its sweep's streams
    long long ubase;  // L sweep: cbase of the mirror U tile
};
struct LineSweep {
    int nx = 0, ny = 0, nz = 0, ntiles = 0, tmax = 0;
    int NA = 3;   // coefficients per row (kind 0: 3, + the diagonal 4; kind 1: 6, 7)
    int P = 8;    // planes per tile
    int NJ = 16;  // lines per tile
    int LV = 2;   // levels per workgroup step
    long rows_total = 0;  // stream rows: per tile T levels x P planes x nj lines
    LineTile *d_tiles = nullptr;
    double *d_coef = nullptr;
    unsigned long long *d_claim = nullptr;
    int *d_order = nullptr;  // the tile of each claim: producers before consumers (line_layout)
    mutable unsigned long long base = 0;
    std::vector<LineTile> h_tiles;
};
struct LineILU {
    LineGeom g;
    int P = 8, NJ = 16, LV = 2;  // the tiles' (k_lineg: 1 plane, ny lines, 1 level)
    int W = 0, S = 0, tmax = 0, ntiles = 0;  // W x S tiles (ntiles > 0: line sweeps active)
    int kind = 0;  // 0: 5-/7-point ILU(0) (linesweep.hip); 1: 7-point ILU(1) pattern (linefill.hip)
    LineSweep L, U;
    double *d_ustream = nullptr;  // the U sweep's rhs, written by the L sweep
    double *d_lstream = nullptr;  // the L sweep's rhs in its stream layout (k_line_rhs)
    // the natural-order vector d_lstream already holds (written with it by a
    // solver pass, launch_line_gather_ew): the next apply of exactly that rhs
    // skips its gather; every apply / sweep clears it
    mutable const double *lstream_of = nullptr;
    double *d_hk = nullptr, *d_hj = nullptr;  // hand-off buffers (armed with TRI_SENTINEL)
    long hk_stride = 0, hj_stride = 0, hk_n = 0, hj_n = 0;
    // the U sweep's tail product (launch_line_apply_spmv): U tiles finished per
    // tile row (monotonic), natural plane -> L tile row, chunk claims
    unsigned *d_kdone = nullptr;
    int *d_kof = nullptr;
    unsigned long long *d_tclaim = nullptr;
    mutable unsigned long long tbase = 0;
    mutable unsigned kepoch = 0;
    // kind 1 on a small 2-D grid (linefill.hip k_lineg): ONE workgroup, lines on
    // lanes; level-major streams [level][S, SE, W(, diag), rhs][lane] per sweep
    int g2 = 0, g2fill = 0, g2V = 0, g2NYP = 0, g2NCL = 0, g2NCU = 0;
    double *d_g2L = nullptr, *d_g2U = nullptr;
};

// lssp_amd_ilu_refactor's and lssp_amd_iluk_refactor's state (ilu_factor.hip):
// the factor pattern F (row i = L's strict part, the diagonal, U's strict part:
// at level 0 the matrix's own pattern) and the buffers k_ilu0_level works in,
// kept between refactors.  4 + 8 B per entry, 4 + 8 + 4 B per row; a plan of
// lssp_amd_iluk_refactor's own routes adds the flag bytes and the diagonal
// positions: 4 + 8 + 1 B per entry, 4 + 8 + 4 + 4 B per row.
struct RefactorPlan {
    long nnz = 0;
    int *d_Fp = nullptr, *d_Fj = nullptr;
    double *d_Fx = nullptr, *d_dinv = nullptr;
    int *d_rows = nullptr;     // rows ordered by level of the strict-lower DAG
    std::vector<int> lev_off;  // host: d_rows[lev_off[l] .. lev_off[l + 1]) is level l
    int *d_flag = nullptr;     // the pattern compare's answer
    // lssp_amd_iluk_refactor (nullptr in a plan lssp_amd_ilu_refactor built):
    unsigned char *d_fin = nullptr;  // per entry of F: lssp_amd_ilu::fIn
    int *d_dpos = nullptr;           // per row: the position of its diagonal in F
};

// lssp_amd_bilu_refactor's state (bilu_factor.hip), kept between refactors: the
// block factor pattern (Bp, Bj: what bilu_pattern made, fill blocks included),
// per block its block row and whether the creating matrix's block graph held
// it, and the buffers the numeric block ILU(0) works in.  d_Bx / d_inv are
// scratch: a refused call (pattern, singular block) dirties only them.  d_Fx is
// the committed copy -- strict-lower blocks as factored, blocks right of the
// diagonal already scaled by the row's inverse (bilu_expand's U values) -- which
// the packet refill and the lazy host refresh read; it changes together with
// the record streams and the handle's d_Dinv, after both flags are read.
// Device bytes: 16 bs^2 + 10 per block, 8 bs^2 + 12 per block row.
struct BiluPlan {
    int nb = 0, bs = 0;
    long nblk = 0;
    int *d_Bp = nullptr, *d_Bj = nullptr, *d_Brow = nullptr;
    unsigned char *d_in = nullptr;   // 1: a block of the creating matrix's graph (not fill)
    unsigned char *d_hit = nullptr;  // the scatter's marks, compared with d_in
    double *d_Bx = nullptr, *d_inv = nullptr, *d_Fx = nullptr;
    int *d_first = nullptr;    // each block row's first non-lower block (Bp[i + 1] when none)
    int *d_rows = nullptr;     // block rows ordered by level of the strict-lower block DAG
    std::vector<int> lev_off;  // host: d_rows[lev_off[l] .. lev_off[l + 1]) is level l
    int *d_flag = nullptr;     // [0] pattern rule broken, [1] singular diagonal block
};

}  // namespace lssp_amd

struct lssp_amd_ilu {
    lssp_amd_ctx *ctx = nullptr;
    int n = 0;
    std::vector<int> Lp, Lj, Up, Uj;  // host copies (for get_factors / tests)
    std::vector<double> Lx, Ux;
    lssp_amd::TriSched lower, upper;
    double *d_cache = nullptr;  // L sweep output, kept all-sentinel between applies
    // packet sweeps: schedule-ordered shadows {L out, L out', U out, U out'} and the
    // apply counter selecting the buffer pair (trisolve.hip launch_ilu_apply)
    mutable double *d_sh[4] = {nullptr, nullptr, nullptr, nullptr};
    mutable double *d_rperm = nullptr;  // the apply's rhs in L order
    mutable unsigned epoch = 0;
    lssp_amd::LineILU line;  // structured factors: line sweeps (ntiles > 0)
    std::mutex sync_free_mu;  // the sync-free arrays, built on first use (ensure_sync_free)
    // BILUK (bs > 0): the inverted diagonal blocks, block i column-major at
    // Dinv + i*bs*bs; the apply runs L^-1, then z = D y (k_bdiag), then U^-1
    int bs = 0;
    std::vector<double> Dinv;
    double *d_Dinv = nullptr;
    double *d_mid = nullptr;  // z: in the L sweep's schedule order (packets) or natural order (sync-free)
    double setup_seconds = 0;
    // how the handle was made (lssp_amd_ilu_refactor's eligibility test):
    // c_kind 0 = caller-made factors (from_factors / from_ldu / BILUK)
    int c_kind = 0, c_level = 0, c_blk = 0;
    lssp_amd::RefactorPlan *rf = nullptr;  // built by the first lssp_amd_ilu_refactor
    bool host_stale = false;  // Lx / Ux (BILUK: and Dinv) are older than the device factors (refreshed by their readers)
    // lssp_amd_bilu_create, bs <= 8 (lssp_amd_bilu_refactor's eligibility test and
    // plan): the block factor pattern -- L / U cannot give it back, a block row
    // without its diagonal block looks the same there -- and per block whether
    // the creating matrix's block graph held it; the level is c_level
    std::vector<int> bBp, bBj;
    std::vector<unsigned char> bIn;
    // built by the first lssp_amd_bilu_refactor; a handle lssp_amd_bilu_create_dev made is born with it, and its
    // bBp / bBj / bIn are downloaded from it with the other host copies (host_missing below)
    lssp_amd::BiluPlan *brf = nullptr;
    // lssp_amd_ilu_create, ILUK with one block (lssp_amd_iluk_refactor's pattern
    // rule): per entry of the factor pattern F, 1 = an entry of the sorted
    // creating matrix, 0 = fill, 2 = an inserted diagonal (ilu_factor); empty:
    // not such a handle, or the creating matrix repeated a column in a row
    std::vector<unsigned char> fIn;
    // made by lssp_amd_ilu_create_dev / lssp_amd_iluk_create_dev: the host copies Lp .. Ux do not exist until
    // something reads them (refactor_host_factors splits them from the device F);
    // until then the entry counts are these
    bool host_missing = false;
    int dev_nnzL = 0, dev_nnzU = 0;
    // made by lssp_amd_ilu_from_factors_dev (and by lssp_amd_ilut_create_dev on the device schedule
    // route): the handle's own device copies of the factors, from which refactor_host_factors makes the
    // host copies on first use (and frees these); nullptr otherwise
    int *fd_Lp = nullptr, *fd_Lj = nullptr, *fd_Up = nullptr, *fd_Uj = nullptr;
    double *fd_Lx = nullptr, *fd_Ux = nullptr;
};

namespace lssp_amd {

// ---- error handling --------------------------------------------------------
#define LSSP_HIP(call)                                                                    \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            fprintf(stderr, "lssp_amd: HIP error %s at %s:%d\n", hipGetErrorString(e_), \
                    __FILE__, __LINE__);                                                  \
            return LSSP_AMD_EHIP;                                                         \
        }                                                                                 \
    } while (0)

#define LSSP_TRY(call)               \
    do {                             \
        int s_ = (call);             \
        if (s_ != LSSP_AMD_OK) return s_; \
    } while (0)

// ---- kernel launchers (kernels.hip) ------------------------------------------
enum Epi { EPI_MXY = 0, EPI_AMXY, EPI_AXPBY, EPI_AMX };  // see spmv kernel
int build_windows(lssp_amd_mat *M, const int *Ap, const int *Aj, const double *Ax);
int tune_spmv_streams(lssp_amd_ctx *c, lssp_amd_mat *M);
constexpr int WIN_ROWS = 1024, WIN_CAP = 16384;
// The SpMV's codings of a matrix whose Ap / Aj / Ax are in HBM (convert.hip),
// each layer on the one below: diagonal ids (at most DIAG_MAX distinct offsets
// col - row, else ndiag stays 0), row codes (at most ROWPAT_MAX patterns of at
// most ROWPAT_LEN entries, else npat stays 0), value codes (at most ROWVAL_MAX
// distinct rows, else nval stays 0; not for a distributed matrix).  step:
// what becomes of each layer's status (lssp_amd_mat_upload_dist's agreement)
constexpr int DIAG_MAX = 255;
constexpr int ROWPAT_MAX = 256, ROWPAT_LEN = 8;
constexpr int ROWVAL_MAX = 256;
int build_codings(lssp_amd_ctx *c, lssp_amd_mat *M, int (*step)(lssp_amd_ctx *, int) = nullptr);
// the value-code layer alone, from the resident Ap / Ac / Ax.  It first drops
// the codes the matrix has (lssp_amd_mat_update_values calls it again)
int build_val_codes(lssp_amd_ctx *c, lssp_amd_mat *M);
// a distributed matrix whose local rows are resident with GLOBAL columns
// (convert.hip): the structure checks, then the local numbering in place with
// the halo list, the halo-free chunk run and max_off_int.  Both are local to
// the rank; the caller (comm.cpp) agrees on each status
int dist_check_dev(lssp_amd_ctx *c, const lssp_amd_mat *M);
int dist_localize_dev(lssp_amd_ctx *c, lssp_amd_mat *M, std::vector<int> &hcols);
int launch_spmv(lssp_amd_ctx *c, const lssp_amd_mat *A, int epi, double alpha, const double *x,
                double beta, const double *y, double *z, int nred, const double *w0,
                const double *w1, long cb = 0, long ce = -1);  // chunks [cb, ce); ce < 0: all
// elementwise + optional partials; kinds in kernels.hip (EwKind)
struct Ew {
    int kind = 0;
    long n = 0;
    double a = 0, b = 0;
    const double *x = nullptr, *y = nullptr, *u = nullptr, *v = nullptr;
    double *out0 = nullptr, *out1 = nullptr;
    const double *scal = nullptr;   // device scalars
    int nred = 0;
    const double *r0a = nullptr, *r0b = nullptr, *r1a = nullptr, *r1b = nullptr;
    const double *r2a = nullptr, *r2b = nullptr, *r3a = nullptr, *r3b = nullptr;  // nred 3, 4
    const double *vbase = nullptr;  // GMRES basis [k][n]
    int k = 0;
    int sidx = 0;                   // scalar index for device-scalar kinds
    int pslot = 0;                  // first partial row the pass's reductions write
};
int launch_ew(lssp_amd_ctx *c, const Ew &e);
// x = y (vector.cxx:73-83): 16-byte vector copy when both are 16-byte aligned
int launch_copy(lssp_amd_ctx *c, double *x, const double *y, long n);
int launch_stream_read(lssp_amd_ctx *c, const double *x, long n, double *sink);

// finish a reduction whose level-1 partials (tree) or operands (serial) are set:
// tree: level-2 over nslot partial rows of C entries; then the finalize program
int launch_reduce_tree(lssp_amd_ctx *c, long C, int nslot, const Fin &f, int slot0 = 0);  // partial rows slot0 ..
// CG's vector updates with the preceding reduction's level 2 folded in (k_cg_fused)
// CGF_R / CGF_PX / CGF_X: the x update x += alpha p is deferred from the x/r
// pass into the next p pass (which reads p anyway), or a batch's last pass
// CGF_X; stamp = the S_DONE value (FIN_CG_RES_RHO_B) that the stop test of
// this pass's own reduction writes -- a guard equal to it still runs the
// pass's x update, any other nonzero guard skips the pass
enum { CGF_P = 0, CGF_XR = 1, CGF_R = 2, CGF_PX = 3, CGF_X = 4 };
int launch_cg_fused(lssp_amd_ctx *c, int kind, long n, double *x, double *p, double *r, const double *z,
                    const double *q, int pin_slot, int pout_slot, const Fin &f, int stamp = 0);
// serial: sums of products a_k[i]*b_k[i] in index order (== vector.cxx:123-133)
int launch_reduce_serial(lssp_amd_ctx *c, long n, int nslot, const double *const *a,
                         const double *const *b, const Fin &f, const double *carry = nullptr);
int launch_finalize(lssp_amd_ctx *c, const double *sums, int nslot, const Fin &f);
int launch_fill(lssp_amd_ctx *c, double *x, long n, uint64_t bits);
int launch_trisolve(lssp_amd_ctx *c, const TriSched &t, const double *rhs, double *x,
                    double *reset);
// BP_RING, pk6_xs_off: sched_dev.h
int build_bp_schedule(lssp_amd_ctx *c, int n, const std::vector<int> &Tp, const std::vector<int> &Tj,
                      const std::vector<double> &Tx, bool upper, const std::vector<int> &lev,
                      TriSched &t, const TriSched *prod = nullptr);
// tri_sched.hip: the same schedule from a factor in HBM (device CSR Tp / Tj / Tx of nnz
// entries), byte for byte; rhs_pos: the L sweep's bp_pos for the U factor (nullptr: the factor's own).
// EINVAL: malformed (tri_levels' rules); EUNSUPPORTED: a strict row beyond 24 entries, more than PK3_CAP
// packets in a block, a stream beyond INT_MAX words (the host builder falls back to the sync-free sweep
// there; this one does not); ETIMEOUT: a bounded wait of the level pass expired.  t is left for
// free_trisched on every failure.  mark(phase) is called after each stage.
int build_trisched_dev(lssp_amd_ctx *c, int n, int nnz, const int *dTp, const int *dTj, const double *dTx, bool upper,
                       const int *rhs_pos, TriSched &t, const std::function<int(const char *)> &mark);
int launch_ilu_apply(lssp_amd_ctx *c, const lssp_amd_ilu *M, double *x, const double *rhs);
int launch_pack(lssp_amd_ctx *c, const int *idx, const double *x, double *buf, int n);
int launch_sum_ranks(lssp_amd_ctx *c, int nslot, const Fin &f);

long num_chunks(long n);
int ensure_part(lssp_amd_ctx *c, long C);

// ---- host pieces ---------------------------------------------------------------
// the drivers' messages (the reference's lssp_printf lines): to the hook set
// with lssp_amd_set_print, else to stdout (flushed, as lssp_printf does)
int lprint(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
double wall_time();  // seconds, lssp_get_time() (utils.cxx:40-46)
// LSSP_AMD_SETUP_TIMES=1 (tuning aid): the setup phases' times go to stderr.  The
// variable's one reader; read at the first call and kept
bool setup_times_on();
// the host setup's phases: "lssp_amd setup: <phase> <seconds> s" (setup_times_on())
void setup_mark(const char *phase);
// The clock of one create or refactor.  mark(phase) prints "lssp_amd <tag>: <phase>
// <seconds> s", the time since the last mark, when setup_times_on() -- after
// draining c's stream when drain is set, so that a phase's time is its own;
// without the variable it does nothing.  total(): the call's setup_seconds.
// Converts to the mark callback the device builders take.
struct PhaseClock {
    lssp_amd_ctx *c;
    const char *tag;
    bool drain;
    double t_start, t0;
    PhaseClock(lssp_amd_ctx *c, const char *tag, bool drain = true);
    int mark(const char *phase);
    double total() const;
    operator std::function<int(const char *)>()
    {
        return [this](const char *phase) { return mark(phase); };
    }
};
// a sub-phase's own duration (LSSP_AMD_SETUP_TIMES; thread-safe: no shared clock)
struct SetupTimer {
    double t0;
    SetupTimer();
    void mark(const char *phase);
};
// host setup loops: f(lo, hi) over [0, n) in contiguous chunks on up to 16
// threads (OMP_NUM_THREADS / the hardware concurrency, whichever is smaller)
int host_threads();  // worker threads for host setup: <= 16, <= OMP_NUM_THREADS
// [0, n) cut into at most 16 contiguous ranges of >= grain items, one thread each
void parallel_for(long n, const std::function<void(long, long)> &f, long grain = 4096);
// a host CSR's shape: Ap from 0 to nnz and never descending, columns inside [0, ncols); else EINVAL
int check_csr(int nrows, int ncols, int nnz, const int *Ap, const int *Aj);

// the hipMallocs of one call (the device builders' temporaries): freed on every path out of it
struct DevBufs {
    std::vector<void *> all;
    template <typename T>
    hipError_t get(T **p, size_t count)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, sizeof(T) * std::max<size_t>(count, 1));
        if (e == hipSuccess) all.push_back(q);
        *p = (T *)q;
        return e;
    }
    void drop(void *q)
    {
        all.erase(std::remove(all.begin(), all.end(), q), all.end());
        (void)hipFree(q);
    }
    ~DevBufs()
    {
        for (void *q : all) (void)hipFree(q);
    }
};

// ILU setup (ilu_setup.cpp), exact restatement of pc-iluk.cxx / pc-ilut.cxx
struct HostCSR {
    int n = 0, ncols = 0;
    std::vector<int> Ap, Aj;
    std::vector<double> Ax;
};
void sort_columns(HostCSR &A);
// c != nullptr: ILUK's numeric ILU(0) runs on c's GPU (ilu_factor.hip), bitwise
// the host restatement (LSSP_AMD_ILU_HOST=1 selects the host one); ILUT stays
// on the host (pc-ilut.cxx:51-286 is sequential by row)
// fin != nullptr, ILUK with one block: one byte per entry of the factor pattern
// F (row i = L's strict part, the diagonal, U's strict part): 1 = an entry of the
// sorted matrix, 0 = fill of level >= 1, 2 = a diagonal adjust_zero_diag
// inserted; left empty otherwise, and when a row of A repeats a column
void ilu_factor(lssp_amd_ctx *c, int kind, HostCSR &&A, int level, double tol, int p, int blk, HostCSR &L,
                HostCSR &U, int *status, std::vector<unsigned char> *fin = nullptr);
int ilu0_factor_gpu(lssp_amd_ctx *c, int n, int blk, const std::vector<int> &Ap, const std::vector<int> &Aj,
                    std::vector<double> &Ax);
// BILUK setup (ilu_setup.cpp, bilu_factor.hip): pc-biluk.cxx on the arithmetic of bilu_dev.h
struct HostBCSR {
    int nb = 0, bs = 1;
    std::vector<int> Bp, Bj;  // block rows; block columns ascending
    std::vector<double> Bx;   // bs x bs blocks, column-major
    std::vector<unsigned char> in_graph;  // per block: A holds an entry of it (0: a fill block of level > 0)
};
// A (columns sorted) to BCSR on the level-k block pattern; EINVAL when n % bs != 0
int bilu_pattern(const HostCSR &A, int level, int bs, HostBCSR &T);
// numeric block ILU(0) in place, inv = the inverted diagonal blocks; EINVAL on a
// singular diagonal block.  The GPU one (bs <= 8) is bitwise the host one.
int bilu0_factor_host(HostBCSR &T, std::vector<double> &inv);
int bilu0_factor_gpu(lssp_amd_ctx *c, HostBCSR &T, std::vector<double> &inv);
// scaled: the blocks right of the diagonal already hold inv_i * a_ij (BiluPlan::d_Fx)
void bilu_expand(const HostBCSR &T, const std::vector<double> &inv, HostCSR &L, HostCSR &U, bool scaled = false);
// block rows ordered by level of the strict-lower block DAG (k_bilu0_level's
// launches): rows[off[l] .. off[l + 1]) is level l, ascending inside a level
void bilu_levels(int nb, const std::vector<int> &Bp, const std::vector<int> &Bj, std::vector<int> &off,
                 std::vector<int> &rows);
// lssp_amd_bilu_refactor (ilu_handle.cpp).  bilu_factor.hip: the plan from the kept
// block pattern; the device steps (scatter, graph compare, k_bilu0_level, U
// scaling, packet refill, d_Dinv), EINVAL with the handle's live state untouched
// when A breaks the pattern rule or a diagonal block is singular; Lx / Ux / Dinv
// from the committed device values.
int bilu_plan_build(lssp_amd_ctx *c, lssp_amd_ilu *M);
void bilu_plan_free(BiluPlan *p);
int bilu_refactor_device(lssp_amd_ctx *c, lssp_amd_ilu *M, const lssp_amd_mat *A);
int bilu_refactor_host_factors(lssp_amd_ilu *M);
// lssp_amd_bilu_create_dev (ilu_handle.cpp; bilu_factor.hip, bilu_create_dev.h), for a
// single-rank square A with n % bs == 0, bs <= 8: M->brf = the plan lssp_amd_bilu_refactor works on, made
// on the device -- rows check, block graph, iluk_symbolic_dev on the graph, its level lists,
// k_bilu_scatter / k_bilu0_level / k_bilu_commit -- and *F = the point factors L and U expanded from the
// committed blocks, in HBM, for the device schedule builder (the caller frees them: iluk_split_free, also
// after a failure).  EUNSUPPORTED: a row whose columns do not ascend strictly inside [0, n), a block row
// without its diagonal block, iluk_symbolic_dev's refusals, bs^2 * blocks + n beyond INT_MAX; EINVAL: a
// singular diagonal block; ETIMEOUT: a bounded wait expired.  mark(phase) is called after each stage.
struct IlutDevFactors;
int bilu_create_device(lssp_amd_ctx *c, lssp_amd_ilu *M, const lssp_amd_mat *A, int level, int bs, IlutDevFactors *F,
                       const std::function<int(const char *)> &mark);
// trisolve.hip: the V array of every packet record of t rewritten from the
// committed block values Fx (k_pk6_refill); C, D, ROW and everything else stay
int launch_pk6_refill(lssp_amd_ctx *c, const TriSched &t, bool upper, int bs, int nb, const int *Bp, const int *Bj,
                      const int *first, const double *Fx);
// z = D y of a BILUK apply.  pos != nullptr: y and z are indexed by schedule
// position, row r at pos[r] (the packet sweeps' shadows); else natural order
int launch_bdiag(lssp_amd_ctx *c, int n, int bs, const double *Dinv, const int *pos, const double *y, double *z);
int build_trisched(lssp_amd_ctx *c, int n, const std::vector<int> &Tp, const std::vector<int> &Tj,
                   const std::vector<double> &Tx, bool upper, TriSched &t, const TriSched *prod = nullptr,
                   bool packets = true, bool arrays = true, std::vector<int> *lev_in = nullptr);
// the rows' dependency levels alone (build_trisched's first pass; lev_in above
// takes them precomputed, e.g. on another thread)
int tri_levels(int n, const std::vector<int> &Tp, const std::vector<int> &Tj, bool upper, std::vector<int> &lev);
// line sweeps (linesweep.hip): LSSP_AMD_EUNSUPPORTED when the factors are not
// the structured ILU(0) of a 5-/7-point grid
int build_line_sweep(lssp_amd_ctx *c, int n, const std::vector<int> &Lp, const std::vector<int> &Lj,
                     const std::vector<double> &Lx, const std::vector<int> &Up, const std::vector<int> &Uj,
                     const std::vector<double> &Ux, LineILU &li);
int line_rearm(lssp_amd_ctx *c, LineILU &li);
// lssp_amd_ilu_create_dev: the tiled sweeps of the ILU(0) of a complete nx x ny
// x nz box from the grid alone -- build_line_sweep's tiles, layouts and buffers,
// the coefficient streams zeroed for launch_line_refill, which every create
// (build_line_sweep included) takes its values from.  line_box_tiled:
// build_line_sweep would put that factor on the 16 x 8 tiles (not on the
// one-workgroup route, not switched off); else EUNSUPPORTED.
bool line_box_tiled(int nx, int ny, int nz);
int build_line_sweep_box(lssp_amd_ctx *c, int nx, int ny, int nz, LineILU &li);
// linefill.hip: the 7-point ILU(1) pattern (EUNSUPPORTED when the factor is not it)
int build_linefill(lssp_amd_ctx *c, int n, const std::vector<int> &Lp, const std::vector<int> &Lj,
                   const std::vector<double> &Lx, const std::vector<int> &Up, const std::vector<int> &Uj,
                   const std::vector<double> &Ux, LineILU &li);
// lssp_amd_iluk_create_dev: the skewed k_linef sweeps of the ILU(1) of a
// complete nx x ny x nz box from the grid alone -- build_linefill's tiles,
// layouts and buffers, the coefficient streams zeroed for
// launch_linefill_refill.  linefill_box_tiled: build_linefill would put that
// factor on the skewed 16 x 8 tiles (line_enabled, detect_fill1's sizes, not
// the one-workgroup route); else EUNSUPPORTED.
bool line_enabled();  // linesweep.hip: LSSP_AMD_LINE=0 turns every line sweep off
bool linefill_box_tiled(int nx, int ny, int nz);
int build_linefill_box(lssp_amd_ctx *c, int nx, int ny, int nz, LineILU &li);
// What the two tiled builds share (linesweep.hip).  line_layout, from a sweep's
// tiles (ls.P / NJ / LV set; W tiles per tile row): every tile's place in the
// streams, the tile table, the claim counter, the coefficient stream's
// allocation (line_coef_len doubles; its values are the refill kernels') and the claim order
// -- tile (J, K) by ascending wj J + wk K, its earliest start, so both producers
// of a tile are claimed before it.  finish_line_tiles, after both layouts: the
// L tiles' links to their mirror U tiles, both rhs streams (zeroed), the
// hand-off buffers (hk_stride / hj_stride doubles per tile, armed), and the
// final synchronise.
size_t line_coef_len(const LineSweep &ls);
int line_layout(lssp_amd_ctx *c, const LineGeom &g, const std::vector<LineTile> &tiles, int NA, int W, int wj, int wk,
                LineSweep &ls);
int finish_line_tiles(lssp_amd_ctx *c, LineILU &li, long hk_stride, long hj_stride);
// line_args: the kernel arguments (linesweep_dev.h) of one sweep of li (which: 0
// L, 1 U) from its rhs stream; outk 2: out = the U rhs stream, 1: natural order
// (tail: the product run by the sweep's workgroups after its tiles, outk 1
// only).  line_launch: that sweep on one of a call site's two kernels -- kern
// (lds0 bytes of LDS), or, with a.tail, the tail instantiation kernt (ldst) --
// with min(tiles, CUs) workgroups of block threads; sets a kernel's dynamic LDS
// limit at its first launch and advances the sweep's claim base by the claims
// the launch consumes.
struct LineArgs;
struct LineTail;
struct LineKernels {  // one static object per call site
    void (*kern)(LineArgs), (*kernt)(LineArgs);
    int lds0, ldst, block;
    std::atomic<bool> sized[2] = {};  // kern's / kernt's LDS limit is set
};
LineArgs line_args(lssp_amd_ctx *c, const LineILU &li, int which, const double *stream, double *out, int outk,
                   const LineTail *tail);
int line_launch(lssp_amd_ctx *c, const LineSweep &ls, const LineArgs &a, LineKernels &k);
// k_linef's rhs gather and sweep launch (linefill.hip; launch_line_apply / _sweep /
// _apply_spmv run them for kind 1): arguments as linesweep.hip's launch_line_gather / launch_line2
int launch_linef_gather(lssp_amd_ctx *c, const LineSweep &ls, int mirror, const double *rhs, double *stream);
int launch_linef(lssp_amd_ctx *c, const LineILU &li, int which, const double *stream, double *out, int outk,
                 const LineTail *tail = nullptr);
// small 2-D grids on one workgroup (linefill.hip): L / U are views of the host
// factors, each row's ncl (U: 3, fill 4) components S, (SE,) W (, diag) taken
// by the shared row rules (iluk_refactor_dev.h); mode 0 apply, 1 L, 2 U
struct FactorView;
int build_lineg(lssp_amd_ctx *c, const LineGeom &g, int fill, int ncl, const FactorView &L, const FactorView &U,
                LineILU &li);
int launch_lineg(lssp_amd_ctx *c, const LineILU &li, int mode, double *x, const double *rhs);
constexpr int G2_MAXNY = 256;  // k_lineg: lines (lanes) of one workgroup
// k_lineg addresses its streams and output through buffer resources: every
// byte offset (and the dropped-store offset 2^30) within 32 bits
inline bool lineg_fits(const LineGeom &g, int fill)
{
    const long nyp = (g.ny + 63) / 64 * 64, V = g.nx + (fill ? 2L : 1L) * (g.ny - 1);
    return (long)g.nx * g.ny * 8 < (1L << 30) && V * 5 * nyp * 8 + 1024 < (1L << 30);
}
void free_line_sweep(LineILU &li);
// lssp_amd_ilu_refactor (ilu_handle.cpp).  ilu_factor.hip: the plan from the host
// copies of the factor pattern; *same = A's device pattern equals it; the
// numeric ILU(0) of Ax (device, plan order) into d_Fx; Lx / Ux from d_Fx.
int refactor_plan_build(lssp_amd_ctx *c, lssp_amd_ilu *M, bool with_flags = false);
void refactor_plan_free(RefactorPlan *p);
int refactor_same_pattern(lssp_amd_ctx *c, const RefactorPlan &p, int n, const int *dAp, const int *dAj, int *same);
int refactor_numeric(lssp_amd_ctx *c, RefactorPlan &p, int n, const double *dAx);
int refactor_host_factors(lssp_amd_ilu *M);
// lssp_amd_iluk_refactor's own routes (ilu_handle.cpp; ilu_factor.hip, DESIGN.md
// 3.3c), on a plan built with the flag bytes.  iluk_match: *ok = A's device
// pattern obeys the pattern rule (nothing written).  iluk_scatter_numeric: A's
// values onto F (fill +0.0, inserted diagonals ZERO_DIAG_TOL), then
// refactor_numeric's launches.
int iluk_match(lssp_amd_ctx *c, const RefactorPlan &p, int n, int nnz, const int *dAp, const int *dAj, int *ok);
int iluk_scatter(lssp_amd_ctx *c, RefactorPlan &p, int n, const int *dAp, const double *dAx);
int refactor_levels(lssp_amd_ctx *c, RefactorPlan &p, int n);
// trisolve.hip: launch_pk6_refill for a scalar factor F (dpos: each row's
// diagonal position); the U sweep's records also get D = the stored pivot, and
// *nonunit (device, zeroed by the caller; may be null) is ORed with 1 when one
// of those pivots is not exactly 1.0
int launch_pk6_refill_scalar(lssp_amd_ctx *c, const TriSched &t, bool upper, int n, const int *Fp, const int *Fj,
                             const int *dpos, const double *Fx, int *nonunit = nullptr);
// linefill.hip: both coefficient streams of a k_linef factor written from one
// factor view per sweep (iluk_refactor_dev.h); every slot is written
int launch_linefill_refill(lssp_amd_ctx *c, LineILU &li, long n, const FactorView &fl, const FactorView &fu);
// lssp_amd_ilu_create_dev (ilu_factor.hip), for a device CSR (n rows, nnz
// entries) and a box nx x ny x nz = n.  box_pattern_check: *ok = the pattern is
// exactly the complete natural-order 5-/7-point stencil of that box, rows
// column-sorted (one flag word read back).  refactor_plan_from_box: the plan of
// such a matrix without a host pass over it -- F's pattern copied device to
// device, the level lists in closed form (row (i, j, k) has level i + j + k;
// rows ascending inside a level, as level_lists orders them).
int box_pattern_check(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, int nx, int ny, int nz,
                      int *ok);
int refactor_plan_from_box(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, int nx, int ny, int nz,
                           RefactorPlan **out);
// lssp_amd_iluk_create_dev (ilu_factor.hip, iluk_create_dev.h):
// the plan of the ILU(1) of such a box, flag bytes and diagonal positions
// included, in closed form.  fill1_nnz: F's entry count (each of L and U holds
// (that + n) / 2).  fill1_plan_pattern: the buffers, and F's pattern written by
// one pass (no wait).  fill1_plan_levels: row (i, j, k) has level i + 2 j + 3 k;
// the level lists from two small host tables, then both passes' flag word read
// back: EINVAL when a position fell outside its array.
long fill1_nnz(int nx, int ny, int nz);
int fill1_plan_pattern(lssp_amd_ctx *c, int n, int nx, int ny, int nz, RefactorPlan **out);
int fill1_plan_levels(lssp_amd_ctx *c, RefactorPlan &p, int n, int nx, int ny, int nz);
// lssp_amd_ilut_create_dev (ilut_factor.hip, ilut_dev.h): ILUT(tol,
// p) of the one-block device CSR factored on the device, a wavefront per row,
// and the finished factors downloaded into L* / U* (ilut_factor_lu's result bit
// for bit).  EUNSUPPORTED: a row unsorted, with a repeated column or without
// its diagonal, or a working row beyond ilut_capacity() entries on a side;
// ETIMEOUT: a bounded wait expired.  mark(phase) is called after the check, the
// numeric phase, the compaction and the download.  keep != nullptr: no download
// -- the finished factors stay in HBM, the six arrays handed to the caller
// (hipFree), L* / U* left empty.
struct IlutDevFactors {
    int *Lp = nullptr, *Lj = nullptr, *Up = nullptr, *Uj = nullptr;
    double *Lx = nullptr, *Ux = nullptr;
    int nnzL = 0, nnzU = 0;
};
int ilut_capacity();
int ilut_factor_dev(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, const double *dAx, double tol,
                    int p, std::vector<int> &Lp, std::vector<int> &Lj, std::vector<double> &Lx,
                    std::vector<int> &Up, std::vector<int> &Uj, std::vector<double> &Ux,
                    const std::function<int(const char *)> &mark, IlutDevFactors *keep = nullptr);
// k_ilut_check's rule on its own (ilut_factor.hip): *ok = Ap starts at 0, ends at nnz and never descends,
// every row's columns ascend strictly inside [0, n) and hold the diagonal (one flag word read back)
int csr_rows_check_dev(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, int *ok);
// tri_sched.hip's level pass on its own, for a factor the caller split itself: lev[i] (device) and the count
int tri_levels_dev(lssp_amd_ctx *c, int n, const int *dTp, const int *dTj, bool upper, int *lev, int *nlevels);
// lssp_amd_pc_create_dev's general ILUK route (iluk_symbolic.hip, iluk_symbolic_dev.h).
// iluk_symbolic_dev: the check, then the plan of the level-k pattern of the one-block device CSR -- d_Fp,
// d_Fj, the flag bytes and the diagonal positions written, d_Fx / d_dinv / d_rows allocated -- made on the
// device, a wavefront per row (level 0: A's pattern copied).  EUNSUPPORTED: k_ilut_check's rule broken,
// level > 254, a working row beyond ilut_capacity() entries on a side, Fp[n] beyond INT_MAX; ETIMEOUT: a
// bounded wait expired.  iluk_split_pattern_dev: Lp / Lj / Up / Uj of F's split (L = strict part + unit
// diagonal last, U = stored pivot first + strict part) and both entry counts, Lx / Ux allocated;
// iluk_split_values_dev: Lx / Ux from the factored d_Fx; iluk_split_free: the six arrays.
// iluk_plan_levels_dev: d_rows and lev_off, the level lists of the numeric DAG (= the L sweep's levels),
// from the split L by tri_sched.hip's level pass and one stable sort.
int iluk_symbolic_dev(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, int level, RefactorPlan **out,
                      const std::function<int(const char *)> &mark);
int iluk_split_pattern_dev(lssp_amd_ctx *c, int n, const RefactorPlan &p, IlutDevFactors *S);
int iluk_split_values_dev(lssp_amd_ctx *c, int n, const RefactorPlan &p, const IlutDevFactors &S);
void iluk_split_free(IlutDevFactors *S);
int iluk_plan_levels_dev(lssp_amd_ctx *c, int n, RefactorPlan &p, const IlutDevFactors &S);
// linesweep.hip: both coefficient streams of a k_line2 factor written from one
// factor view per sweep (iluk_refactor_dev.h: the combined F for both, or a
// lone L and a lone U); every slot is written.  line_refill_host: the same for
// a host create of either kind -- L, then U, each through temporary device
// buffers and refill, its kind's one-sweep launch (which: 0 L, 1 U).
int launch_line_refill(lssp_amd_ctx *c, LineILU &li, long n, const FactorView &fl, const FactorView &fu);
using LineSweepRefill = int (*)(lssp_amd_ctx *, LineILU &, int which, long n, const FactorView &);
int line_refill_host(lssp_amd_ctx *c, LineILU &li, long n, const std::vector<int> &Lp, const std::vector<int> &Lj,
                     const std::vector<double> &Lx, const std::vector<int> &Up, const std::vector<int> &Uj,
                     const std::vector<double> &Ux, LineSweepRefill refill);
int launch_line_apply(lssp_amd_ctx *c, const LineILU &li, double *x, const double *rhs);
// the apply followed by z = op(A x) (+ fused dots), the product run by the U
// sweep's workgroups as planes of x become final (k_line2 tail); results are
// bitwise launch_line_apply + launch_spmv.  EUNSUPPORTED when A is not a coded
// single-rank stencil of the factor's grid (the caller then runs the two)
int launch_line_apply_spmv(lssp_amd_ctx *c, const LineILU &li, double *x, const double *rhs, const lssp_amd_mat *A,
                           int epi, double alpha, double beta, const double *y, double *z, int nred,
                           const double *w0, const double *w1);
// the same on P ranks: the tail computes the halo-free chunks [ich0, ich1)
// only; the halo round and the boundary chunks follow it (spmv_boundary)
int spmv_boundary(lssp_amd_ctx *c, const lssp_amd_mat *A, int epi, double alpha, double *x, double beta,
                  const double *y, double *z, int nred, const double *w0, const double *w1);
int launch_line_sweep(lssp_amd_ctx *c, const LineILU &li, int which, double *x, const double *rhs);
// A BiCGSTAB vector pass fused with the next apply's rhs gather: out (natural
// order, n rows) = op(x, y, out) and the same values into the L sweep's
// stream, which the next launch_line_apply of rhs == out then reads as is.
// op: GEW_BICG_P out = x + beta*(out - omega*y), GEW_BICG_S out = x - alpha*y
// (scalars from scal; k_ew's EW_BICG_P / EW_BICG_S arithmetic).  Eligible
// (line_gather_ew_ok) for the k_line2 sweeps of an n-row grid factor.
enum { GEW_BICG_P = 1, GEW_BICG_S = 2 };
bool line_gather_ew_ok(const LineILU &li, long n);
int launch_line_gather_ew(lssp_amd_ctx *c, const LineILU &li, int op, const double *x, const double *y, double *out,
                          const double *scal);
void free_trisched(TriSched &t);
// the sync-free sweep's arrays of t alone (perm, rp, cols, vals, diag), the pointers cleared: a refactor drops
// them, the next single sweep builds them again (ensure_sync_free)
void free_sync_free_arrays(TriSched &t);

// reductions with the context's mode; result left in d_sums / scal per Fin
int finish_reduce(lssp_amd_ctx *c, long n, int nslot, const double *const *a,
                  const double *const *b, const Fin &f);
int reduce_dots(lssp_amd_ctx *c, long n, int nslot, const double *const *a,
                const double *const *b, const Fin &f);
// multi-rank: all-gather rank sums and sum in rank order, then the finalize
int comm_allgather_sums(lssp_amd_ctx *c, int nslot);
// recv (nranks * bytes, rank order) = every rank's send (bytes), through the
// context's transport (RCCL or the host hooks)
int comm_allgather(lssp_amd_ctx *c, const void *send, void *recv, long bytes);
int comm_gather_int(lssp_amd_ctx *c, int v, std::vector<int> &all);  // collective, rank order
// serial mode, P ranks: receive the running sums of rank-1 (zeros on rank 0)
// into c->d_carry / pass this rank's on to rank+1
int comm_carry_in(lssp_amd_ctx *c);
int comm_carry_out(lssp_amd_ctx *c);
int halo_exchange(const lssp_amd_mat *A, double *x);
// halo round + product, the halo-free chunks overlapped with the round
int spmv_halo(lssp_amd_ctx *c, const lssp_amd_mat *A, int epi, double alpha, double *x, double beta,
              const double *y, double *z, int nred, const double *w0, const double *w1);
int comm_destroy(lssp_amd_ctx *c);

// The canonical level-1 halving tree of one wave: lane 0 gets
// (((v0 + v32) + (v16 + v48)) + ...), the pairs of an xor butterfly over 32,
// 16, 8, 4, 2, 1 -- evaluated for lane 0 only: the 32- and 16-lane steps by
// v_permlane32_swap / v_permlane16_swap, the 8, 4, 2, 1 steps by DPP row
// shifts (row_shl:k), instead of six dependent ds_bpermute round trips per
// half.  Lane 0 adds the same operands in the same pairs, so its value is
// bitwise the butterfly's; the other lanes hold partial sums (every caller
// reads lane 0).  -DWAVE_SUM_BPERM restores the butterfly (A/B).
__device__ __forceinline__ double wave_sum_l0(double v)
{
#ifdef WAVE_SUM_BPERM
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
#else
    auto split = [](double x, unsigned &lo, unsigned &hi) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(x);
        lo = (unsigned)b;
        hi = (unsigned)(b >> 32);
    };
    auto join = [](unsigned lo, unsigned hi) {
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    };
    unsigned lo, hi;
    split(v, lo, hi);
    {  // lanes 0..31 <- lanes 32..63
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v = v + join(a[1], b[1]);
    }
    split(v, lo, hi);
    {  // lanes 0..15 <- lanes 16..31
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = v + join(a[1], b[1]);
    }
    // lanes l <- l + k inside each 16-lane row (row_shl:k = 0x100 + k)
    split(v, lo, hi);
    v = v + join((unsigned)__builtin_amdgcn_update_dpp((int)lo, (int)lo, 0x108, 0xf, 0xf, false),
                 (unsigned)__builtin_amdgcn_update_dpp((int)hi, (int)hi, 0x108, 0xf, 0xf, false));
    split(v, lo, hi);
    v = v + join((unsigned)__builtin_amdgcn_update_dpp((int)lo, (int)lo, 0x104, 0xf, 0xf, false),
                 (unsigned)__builtin_amdgcn_update_dpp((int)hi, (int)hi, 0x104, 0xf, 0xf, false));
    split(v, lo, hi);
    v = v + join((unsigned)__builtin_amdgcn_update_dpp((int)lo, (int)lo, 0x102, 0xf, 0xf, false),
                 (unsigned)__builtin_amdgcn_update_dpp((int)hi, (int)hi, 0x102, 0xf, 0xf, false));
    split(v, lo, hi);
    v = v + join((unsigned)__builtin_amdgcn_update_dpp((int)lo, (int)lo, 0x101, 0xf, 0xf, false),
                 (unsigned)__builtin_amdgcn_update_dpp((int)hi, (int)hi, 0x101, 0xf, 0xf, false));
    return v;
#endif
}

}  // namespace lssp_amd
