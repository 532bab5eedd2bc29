/*
 * lssp_amd.h -- C-ABI of the MI355X-native LSSP Krylov hot path.
 *
 * Plain pointers and sizes only (no torch, no C++ types).  Device vectors are
 * raw `double *` obtained from lssp_amd_vec_alloc; host arrays are the
 * caller's.  Every entry point returns an int status (LSSP_AMD_OK == 0) and
 * never exits the process; the reference-side binding
 * (integration/amd_backend.cxx) maps a non-zero status to lssp_error(1, ...),
 * which reproduces the reference's exit-on-fatal (utils.cxx:114-135).
 *
 * Each group cites the reference interface it replaces (paths relative to the
 * huiscliu/lssp tree).  The binding a maintainer would add on the reference
 * side is shown in INTEGRATION.md.
 */
#ifndef LSSP_AMD_H
#define LSSP_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status ------------------------------------------------------------ */
enum {
    LSSP_AMD_OK = 0,
    LSSP_AMD_EINVAL = 1,      /* bad argument (the reference asserts / lssp_error) */
    LSSP_AMD_EHIP = 2,        /* HIP runtime error */
    LSSP_AMD_ENOMEM = 3,      /* device or host allocation failed (utils.h:41-57) */
    LSSP_AMD_ETIMEOUT = 4,    /* a sync-free trisolve wait exceeded its bound */
    LSSP_AMD_ECOMM = 5,       /* RCCL error */
    LSSP_AMD_EUNSUPPORTED = 6 /* solver/PC combination not on the hot path */
};

/* reduction order of every dot / norm (vector.cxx:123-139) */
enum {
    LSSP_AMD_REDUCE_SERIAL = 0, /* sequential sum from 0, bitwise == the reference */
    LSSP_AMD_REDUCE_TREE = 1    /* canonical 256-chunk tree, the fast path */
};

/* LSSP_SOLVER_TYPE values of the reference (type-defs.h:157-178) */
enum {
    LSSP_AMD_GMRES = 0, LSSP_AMD_LGMRES = 1, LSSP_AMD_RGMRES = 2, LSSP_AMD_RLGMRES = 3, LSSP_AMD_BICGSTAB = 4,
    LSSP_AMD_BICGSAFE = 6, LSSP_AMD_CG = 7, LSSP_AMD_CGS = 8, LSSP_AMD_GPBICG = 9, LSSP_AMD_CR = 10,
    LSSP_AMD_CRS = 11, LSSP_AMD_BICRSTAB = 12, LSSP_AMD_BICRSAFE = 13, LSSP_AMD_GPBICR = 14,
    LSSP_AMD_QMRCGSTAB = 15, LSSP_AMD_TFQMR = 16, LSSP_AMD_ORTHOMIN = 17,
    LSSP_AMD_BICGSTABL = 5, LSSP_AMD_IDRS = 18
};
/* ILU kinds (LSSP_PC_TYPE, type-defs.h:63-101) */
enum { LSSP_AMD_ILUK = 1, LSSP_AMD_ILUT = 2, LSSP_AMD_BILUK = 3 };

typedef struct lssp_amd_ctx lssp_amd_ctx; /* one device + stream + scratch */
typedef struct lssp_amd_mat lssp_amd_mat; /* device CSR (lssp_mat_csr, type-defs.h:15-24) */
typedef struct lssp_amd_ilu lssp_amd_ilu; /* device L/U + trisolve schedules (LSSP_PC.L/.U) */

const char *lssp_amd_strerror(int status);
int lssp_amd_version(void);

/* Where the drivers' messages go (the lines the reference prints with
 * lssp_printf, utils.cxx:93-112: parameters at verb >= 2, the per-iteration
 * line at verb >= 1, "total iteration" / "total time" at verb >= 2).  fn ==
 * NULL (the default): stdout, flushed after every line.  The reference-side
 * binding routes them through lssp_printf, so a log file set with
 * lssp_set_log receives them too.  Process-wide; fn returns < 0 on error. */
void lssp_amd_set_print(int (*fn)(void *user, const char *msg), void *user);

/* ---- context: replaces the implicit single host thread ------------------ */
int lssp_amd_ctx_create(int device, lssp_amd_ctx **ctx);
int lssp_amd_ctx_destroy(lssp_amd_ctx *ctx);
int lssp_amd_ctx_set_reduction(lssp_amd_ctx *ctx, int mode);
int lssp_amd_ctx_sync(lssp_amd_ctx *ctx);
/* HIP stream the context enqueues on (a hipStream_t), for timing with events */
void *lssp_amd_ctx_stream(lssp_amd_ctx *ctx);

/* ---- device vectors: lssp_vec_create/destroy/set_value_by_array/get_value
 *      (vector.cxx:4-70) ----------------------------------------------- */
int lssp_amd_vec_alloc(lssp_amd_ctx *ctx, long n, double **d);
int lssp_amd_vec_free(lssp_amd_ctx *ctx, double *d);
int lssp_amd_vec_upload(lssp_amd_ctx *ctx, double *d, const double *h, long n);
int lssp_amd_vec_download(lssp_amd_ctx *ctx, double *h, const double *d, long n);

/* ---- CSR matrix: a device copy of an lssp_mat_csr, kept in the given entry
 *      order (SpMV sums in that order, mvops.cxx:55-58).  The solvers expect
 *      the assembled matrix, whose columns lssp_solver_assemble sorts
 *      (lssp.cxx:173): call lssp_amd_csr_sort_columns first, as that does. */
int lssp_amd_csr_sort_columns(int nrows, int ncols, int *Ap, int *Aj, double *Ax); /* matrix-utils.cxx:387-481 */
int lssp_amd_mat_upload(lssp_amd_ctx *ctx, int nrows, int ncols, int nnz, const int *Ap,
                        const int *Aj, const double *Ax, lssp_amd_mat **A);
int lssp_amd_mat_destroy(lssp_amd_mat *A);
int lssp_amd_mat_info(const lssp_amd_mat *A, int *nrows, int *ncols, int *nnz);
/* Device layout of the SpMV's column stream: *ndiag > 0 when every entry's
 * offset col - row is one of ndiag (<= 255) distinct values (stencil
 * matrices); the SpMV then reads a 1-byte offset id per entry instead of the
 * 4-byte column (same entries, same summation order).  0: plain CSR columns.
 * *windowed (may be NULL) = 1 when the columns of every 1024-row block span
 * at most 16384 entries and the product stages that span of x in LDS instead
 * of gathering it from memory (locally numbered meshes); 0 otherwise. */
int lssp_amd_mat_layout(const lssp_amd_mat *A, int *ndiag, int *windowed);
/* Row coding of an offset-coded matrix: *npatterns > 0 when every row has at
 * most 8 entries and the rows' offset-id sequences take at most 256 distinct
 * values (a 7-pt grid has 27); the SpMV then reads one byte per row -- the
 * index of the row's pattern -- instead of the row pointer and the ids (same
 * entries, same summation order).  0: not row-coded. */
int lssp_amd_mat_rowcodes(const lssp_amd_mat *A, int *npatterns);
/* Value coding of a row-coded matrix: *nvalues > 0 when its rows -- pattern
 * and values, compared bit for bit -- take at most 256 distinct values (a
 * constant-coefficient 7-pt grid has 27); the SpMV then reads one byte per
 * row -- the index of the row in a table of those rows -- and none of the
 * matrix values (same entries, same summation order).  The codes follow the
 * values: lssp_amd_mat_update_values rebuilds or drops them.  0: not
 * value-coded (always for a distributed matrix). */
int lssp_amd_mat_valcodes(const lssp_amd_mat *A, int *nvalues);
/* Device memory of a matrix: *csr_bytes = the resident CSR (Ap, Aj, Ax: every
 * operation but the two SpMV layouts above reads it), *aux_bytes = what the
 * SpMV layouts add beside it (offset ids + table; row codes + pattern table;
 * value codes + value table; window spans and the sliced copy, about as large as Aj + Ax again).  A
 * windowed matrix whose padded
 * sliced copy would exceed 2^30 entries is not windowed (32-bit slice
 * offsets) and runs on the CSR product.  Either pointer may be NULL. */
int lssp_amd_mat_bytes(const lssp_amd_mat *A, long long *csr_bytes, long long *aux_bytes);

/* ---- SpMV: mvops.h:9-19 (mvops.cxx:5-150), bitwise per row --------------
 * x: for a matrix from lssp_amd_mat_upload the first ncols entries are read.
 * For a distributed matrix (lssp_amd_mat_upload_dist) x MUST hold
 * nrows + nhalo entries (lssp_amd_mat_local_rows): the rank's own entries,
 * then room for the halo, which every product OVERWRITES with the peers'
 * values before computing -- hence x is not const. */
/* y = y*beta + alpha*A*x            (lssp_mv_amxpby,  mvops.cxx:33-39)  */
int lssp_amd_mv_amxpby(lssp_amd_ctx *ctx, double alpha, const lssp_amd_mat *A, double *x,
                       double beta, double *y);
/* z = y*beta + alpha*A*x            (lssp_mv_amxpbyz, mvops.cxx:71-78)  */
int lssp_amd_mv_amxpbyz(lssp_amd_ctx *ctx, double alpha, const lssp_amd_mat *A, double *x,
                        double beta, const double *y, double *z);
/* y = a*A*x                         (lssp_mv_amxy,    mvops.cxx:109-115) */
int lssp_amd_mv_amxy(lssp_amd_ctx *ctx, double a, const lssp_amd_mat *A, double *x, double *y);
/* y = A*x                           (lssp_mv_mxy,     mvops.cxx:144-150) */
int lssp_amd_mv_mxy(lssp_amd_ctx *ctx, const lssp_amd_mat *A, double *x, double *y);

/* ---- BLAS-1: vector.h:8-39 (vector.cxx:31-146) -------------------------- */
int lssp_amd_vec_set_value(lssp_amd_ctx *ctx, double *x, long n, double val);
int lssp_amd_vec_copy(lssp_amd_ctx *ctx, double *x, const double *y, long n);
/* Measurement aid (no reference counterpart): read x[0..n) once with 16-byte
 * non-temporal loads and store the XOR of all its 64-bit words (as bits) in
 * the device double *sink -- the HBM streaming-read rate quoted beside the
 * 8 TB/s spec.  n even, x 16-byte aligned (else LSSP_AMD_EINVAL). */
int lssp_amd_stream_read(lssp_amd_ctx *ctx, const double *x, long n, double *sink);
int lssp_amd_vec_axy(lssp_amd_ctx *ctx, double alpha, const double *x, double *y, long n);
int lssp_amd_vec_axpby(lssp_amd_ctx *ctx, double alpha, const double *x, double beta, double *y,
                       long n);
int lssp_amd_vec_axpbyz(lssp_amd_ctx *ctx, double alpha, const double *x, double beta,
                        const double *y, double *z, long n);
int lssp_amd_vec_scale(lssp_amd_ctx *ctx, double *x, long n, double a);
int lssp_amd_vec_dot(lssp_amd_ctx *ctx, const double *x, const double *y, long n, double *result);
int lssp_amd_vec_norm(lssp_amd_ctx *ctx, const double *x, long n, double *result);

/* ---- ILU preconditioner ---------------------------------------------------
 * Setup on the host, exactly the reference algorithm: ILUK
 * (lssp_pc_iluk_assemble, pc-iluk.cxx:566-581) or ILUT (lssp_pc_ilut_assemble,
 * pc-ilut.cxx:429-456); blk > 0 and < n selects block-Jacobi blocks of that
 * size (the blk_size path of pc-iluk.cxx:411-552), used per rank on multi-GPU.
 * Then the factors are uploaded with their sync-free trisolve schedules.
 * Apply: x = U^-1 L^-1 rhs on the device (lssp_pc_ilu_solve,
 * solver-tri.cxx:57-60), bitwise; x may alias rhs. */
int lssp_amd_ilu_create(lssp_amd_ctx *ctx, int kind, int n, const int *Ap, const int *Aj,
                        const double *Ax, int level, double tol, int p, int blk,
                        lssp_amd_ilu **M);
/* upload caller-made factors (L: unit diagonal LAST per row; U: pivot FIRST) */
int lssp_amd_ilu_from_factors(lssp_amd_ctx *ctx, int n, const int *Lp, const int *Lj,
                              const double *Lx, const int *Up, const int *Uj, const double *Ux,
                              lssp_amd_ilu **M);
int lssp_amd_ilu_destroy(lssp_amd_ilu *M);
int lssp_amd_ilu_apply(lssp_amd_ctx *ctx, const lssp_amd_ilu *M, double *x, const double *rhs);
/* The apply enqueued on the context's stream without waiting for it (the
 * synchronous lssp_amd_ilu_apply returns when x is written, like the
 * reference's pc.solve); lssp_amd_ilu_check then waits for the stream and
 * reports a hand-off timeout (LSSP_AMD_ETIMEOUT) of any apply since the last
 * check, re-arming the factor's hand-off buffers.  After an ETIMEOUT, the x of
 * EVERY apply enqueued since the last successful check is invalid (an apply
 * queued behind the one that timed out reads its un-armed hand-off buffers):
 * re-run them. */
int lssp_amd_ilu_apply_async(lssp_amd_ctx *ctx, const lssp_amd_ilu *M, double *x, const double *rhs);
int lssp_amd_ilu_check(lssp_amd_ctx *ctx, const lssp_amd_ilu *M);
/* one triangular sweep: which = 0 lower (solver-tri.cxx:4-24), 1 upper (:26-46) */
int lssp_amd_ilu_trisolve(lssp_amd_ctx *ctx, const lssp_amd_ilu *M, int which, double *x,
                          const double *rhs);
int lssp_amd_ilu_info(const lssp_amd_ilu *M, int *n, int *nnzL, int *nnzU, int *levelsL,
                      int *levelsU, double *setup_seconds);
int lssp_amd_ilu_get_factors(const lssp_amd_ilu *M, int *Lp, int *Lj, double *Lx, int *Up,
                             int *Uj, double *Ux);
/* How an apply sweeps M's factors (no reference counterpart: a query like
 * lssp_amd_mat_layout).  *line = 1 when the factors are a natural-ordered 5-/7-
 * point grid's ILU(0) and run as line sweeps, with tiles of *lines lines x
 * *planes planes (chosen per factor); 2 when they are a 7-point grid's ILU(1)
 * (fill offsets nx-1, nx*ny-nx, nx*ny-1) and run as skewed line sweeps
 * (*lines = 16 lines of j + k, *planes = 8); 0 (and 0 x 0) for the general
 * packet sweeps.  Any pointer may be NULL. */
int lssp_amd_ilu_sweep_layout(const lssp_amd_ilu *M, int *line, int *lines, int *planes);
/* lssp_amd_ilu_from_factors for factors that already live in HBM (no reference
 * counterpart): dLp .. dUx are DEVICE arrays in the same layout (L: diagonal
 * LAST per row; U: pivot FIRST).  No factor array crosses to the host: both
 * packet schedules are built on the device, and only a few
 * words come back (Lp[n], Up[n], flags and counts).  The handle owns device-
 * to-device copies, so the caller may free or reuse its arrays on return; its
 * host copies are made by the first call that reads them
 * (lssp_amd_ilu_get_factors, lssp_amd_ilu_trisolve).  The handle always runs
 * the packet sweeps -- lssp_amd_ilu_sweep_layout answers (0, 0, 0) even for a
 * grid's ILU(0) -- and every sweep is bitwise the reference's, so results do
 * not depend on that: lssp_amd_ilu_apply / _apply_async + _check / _trisolve /
 * lssp_amd_solve / _info / _get_factors are bitwise those of
 * lssp_amd_ilu_from_factors on the same arrays, and both refactor calls
 * answer LSSP_AMD_EUNSUPPORTED, as there.  LSSP_AMD_EUNSUPPORTED, with *out
 * NULL and nothing left allocated: a strict row beyond 24 entries, more than
 * 4096 packets in one block of the schedule, a record or index stream beyond
 * INT_MAX words (the sync-free fallback is not built on the device: use
 * lssp_amd_ilu_from_factors there).  LSSP_AMD_EINVAL: a NULL argument,
 * n <= 0, a row without a diagonal slot, a strict column on the wrong side of
 * its row or outside [0, n).  LSSP_AMD_ETIMEOUT: a bounded wait of the level
 * pass expired.  LSSP_AMD_EHIP: a HIP error, everything freed. */
int lssp_amd_ilu_from_factors_dev(lssp_amd_ctx *ctx, int n, const int *dLp, const int *dLj, const double *dLx,
                                  const int *dUp, const int *dUj, const double *dUx, lssp_amd_ilu **out);
/* The packet schedule an apply of M walks (no reference counterpart: a query
 * like lssp_amd_ilu_sweep_layout).  which = 0: the L sweep's, 1: the U
 * sweep's.  hdr = {B (rows per block), nb (blocks), nsteps, npackets, EP
 * (operand slots per row: 4, 8, 16, 24), EXT (HBM operand loads per loader
 * lane), rows per packet, rec words, idx words, unit (every diagonal is 1.0),
 * nlevels, origin}; origin = 0: built on the host, 1: on the device.  With
 * every array pointer NULL only hdr is filled (the two-call form of
 * lssp_amd_csr_to_bcsr); otherwise each non-NULL array is downloaded: blk
 * (nb + 1), desc (4 * npackets), rec (rec words), idx (idx words), perm and
 * pos (n).  A handle without a packet schedule (line sweeps, the sync-free
 * fallback), or a record stream beyond INT_MAX words: LSSP_AMD_EUNSUPPORTED. */
int lssp_amd_ilu_get_schedule(const lssp_amd_ilu *M, int which, int hdr[12], int *blk, int *desc,
                              unsigned *rec, int *idx, int *perm, int *pos);

/* ---- BILUK: block ILU(level) on bs x bs blocks (lssp_pc_biluk_assemble,
 *      pc-biluk.cxx:388-431; the reference passes num_blks = n / bs).  The apply
 *      is y = L^-1 rhs, z = D y, x = U^-1 z (lssp_pc_bilu_solve, :22-60), D the
 *      inverted diagonal blocks.  The reference's block values depend on its
 *      BLAS / LAPACK; this library fixes one arithmetic of its own (DESIGN.md
 *      3.7), the same bits on the host and the device path.  A handle works with
 *      lssp_amd_ilu_apply / _apply_async / _check / _trisolve / _info /
 *      _get_factors / _destroy and lssp_amd_solve like any other.  Single rank
 *      only (no block-Jacobi blk argument).
 * n % bs == 0 and 1 <= bs <= 32, else EINVAL.  level < 0: default 1.  bs <= 8
 * runs the numeric factorization on the GPU, larger blocks on the host.  A
 * block row without a diagonal block gets the identity as its inverse; an
 * exactly singular diagonal block returns LSSP_AMD_EINVAL (the reference
 * exits). */
int lssp_amd_bilu_create(lssp_amd_ctx *ctx, int n, const int *Ap, const int *Aj, const double *Ax,
                         int level, int bs, lssp_amd_ilu **M);
/* caller-made factors (what the reference's host setup leaves in pc.L / pc.D / pc.U):
 * L unit diagonal LAST, U unit diagonal FIRST, D block diagonal CSR */
int lssp_amd_ilu_from_ldu(lssp_amd_ctx *ctx, int n, const int *Lp, const int *Lj, const double *Lx,
                          const int *Dp, const int *Dj, const double *Dx,
                          const int *Up, const int *Uj, const double *Ux, lssp_amd_ilu **M);
/* *bs = 0 for an ILUK/ILUT handle; else Dinv (may be NULL) receives n*bs doubles,
 * block i column-major at Dinv + i*bs*bs */
int lssp_amd_ilu_get_diag(const lssp_amd_ilu *M, int *bs, double *Dinv);
/* HOST ONLY (no context, runs without a GPU): the same factors by the host path.
 * Two calls like lssp_amd_csr_to_bcsr: with Lj == NULL only *nnzL / *nnzU are set. */
int lssp_amd_bilu_factor_host(int n, const int *Ap, const int *Aj, const double *Ax, int level, int bs,
                              int *nnzL, int *nnzU, int *Lp, int *Lj, double *Lx, double *Dinv,
                              int *Up, int *Uj, double *Ux);

/* ---- Krylov solve: lssp_solver_solve (lssp.cxx:250-414) for BiCGSTAB
 *      (solver-bicgstab.cxx:10-175), GMRES(m) (solver-gmres.cxx:12-255),
 *      right-preconditioned GMRES(m) (solver-gmres.cxx:257-479), LGMRES(m, k)
 *      (solver-lgmres.cxx:12-312), CG (solver-cg.cxx:8-136), and the other internal
 *      drivers (solver-{bicgstabl,bicgsafe,cgs,gpbicg,cr,crs,bicrstab,bicrsafe,
 *      gpbicr,qmrcgstab,tfqmr,orthomin,idrs}.cxx).  Same recurrences, guards, defaults and
 *      iteration counting; vectors stay in HBM. ------------------------- */
typedef struct {
    int solver;     /* LSSP_AMD_* above (LSSP_SOLVER_TYPE) */
    double tol_rel; /* < 0: default 1e-7 (lssp.cxx:11-13) */
    double tol_abs;
    double tol_rb;
    int maxit;      /* <= 0: default 1000 */
    int restart;    /* GMRES m; < 0: default 50 */
    int verb;       /* >= 1 prints the reference's per-iteration line */
    int aug_k;      /* LGMRES augmentation vectors k; <= 0: default 3 (lssp.cxx:6) */
    int bgsl;       /* BiCGSTAB(l) l; <= 0: default 4 (LSSP_SOLVER.bgsl, lssp.cxx:7, :495-503) */
    int idrs;       /* IDR(s) s; <= 0: default 4 (LSSP_SOLVER.idrs, lssp.cxx:8, :505-513) */
} lssp_amd_solve_params;

/* x: device, x0 on entry, solution on exit; b: device.  M == NULL is PC_NON
 * (pc.cxx:67-70).  trace (host, optional) receives every dot/norm the driver
 * evaluates, in the reference's call order.  On a distributed matrix x and
 * every work vector hold nrows + nhalo entries (the halo part of x is
 * overwritten by the solve's products); b holds nrows. */
int lssp_amd_solve(lssp_amd_ctx *ctx, const lssp_amd_mat *A, const lssp_amd_ilu *M,
                   const lssp_amd_solve_params *prm, double *x, const double *b, int *nits,
                   double *residual, double *trace, int trace_cap, int *trace_len);

/* ---- multi-GPU: one process per GPU, row-block partition, RCCL over xGMI --
 * The reference is serial (README.md:3); this is the SURVEY 8(e) extension.
 * Rank r owns rows [r*ceil(n/P), min((r+1)*ceil(n/P), n)).  A distributed
 * matrix holds the rank's rows with columns renumbered [owned | halo]; SpMV
 * fetches the halo with grouped ncclSend/ncclRecv; dots all-gather the P rank
 * partials and sum them in rank order (deterministic, identical on every
 * rank). */
int lssp_amd_comm_unique_id_size(void);
int lssp_amd_comm_get_unique_id(void *id_out);
/* Collective over the nranks processes (ncclCommInitRank).  Every nranks >= 1
 * creates a real RCCL communicator, nranks == 1 included: the caller must pass
 * an id from lssp_amd_comm_get_unique_id (a placeholder id blocks or fails in
 * RCCL).  A context that never calls it runs single-rank with no communicator;
 * lssp_amd_comm_nranks reports the communicator's rank count (ncclCommCount). */
int lssp_amd_comm_init(lssp_amd_ctx *ctx, int nranks, int rank, const void *id);
int lssp_amd_comm_nranks(lssp_amd_ctx *ctx, int *nranks);
int lssp_amd_comm_barrier(lssp_amd_ctx *ctx);
/* Transport check (collective): an all-gather of every rank's id and a ring
 * round of grouped send/recv (rank r -> r+1, r-1 -> r; a 1-rank communicator
 * sends to itself) driven exactly as the SpMV's halo round is -- packed on the
 * compute stream, the round on the communication stream between two events,
 * the compute stream waiting for it -- then every received word checked.
 * LSSP_AMD_OK, or LSSP_AMD_ECOMM when a value did not arrive.  With nranks = 1
 * lssp_amd_comm_init still creates the (1-rank) RCCL communicator, so a single
 * GPU can run this before a multi-GPU job. */
int lssp_amd_comm_selftest(lssp_amd_ctx *ctx);

/* Host-staged transport: the same protocol with the collective carried by the
 * caller (an MPI library, a torch.distributed gloo group, ...) instead of
 * RCCL.  The library copies the bytes to host memory, calls the hook and
 * copies the result back; used where RCCL is unavailable and to exercise the
 * multi-rank path with several ranks on ONE device (RCCL refuses that).
 * Every hook returns 0 on success; buffers are host memory. */
typedef struct {
    void *user;
    /* recv[q*bytes .. (q+1)*bytes) = rank q's send, for q = 0 .. nranks-1 */
    int (*allgather)(void *user, const void *send, void *recv, long bytes);
    /* one grouped round: nsend messages to peers send_peer[i], nrecv from
     * recv_peer[i]; a rank sends at most one message to each peer per round */
    int (*sendrecv)(void *user, int nsend, const int *send_peer, const void *const *send_buf,
                    const long *send_bytes, int nrecv, const int *recv_peer, void *const *recv_buf,
                    const long *recv_bytes);
} lssp_amd_host_transport;
int lssp_amd_comm_init_host(lssp_amd_ctx *ctx, int nranks, int rank, const lssp_amd_host_transport *t);

/* rows [row0, row0 + nlocal) of a global n x n CSR given by its local rows.
 * Collective: every rank calls it; the input checks are agreed on across the
 * ranks first, so a bad argument on one rank makes EVERY rank return
 * LSSP_AMD_EINVAL (no rank is left waiting in a collective). */
int lssp_amd_mat_upload_dist(lssp_amd_ctx *ctx, int n_global, int row0, int nlocal,
                             const int *Ap, const int *Aj, const double *Ax, lssp_amd_mat **A);
int lssp_amd_mat_local_rows(const lssp_amd_mat *A, int *row0, int *nlocal, int *nhalo);
/* The same handle from DEVICE arrays: local rows [row0, row0 + nlocal) with
 * GLOBAL column indices, dAp (nlocal + 1), dAj and dAx (nnz) in HBM.  Equal to
 * lssp_amd_mat_upload_dist of the same arrays in every observable way
 * (lssp_amd_mat_local_rows, _layout, _rowcodes, _valcodes (0), _bytes, _info,
 * every product, every solve bitwise, the status for the same input); that call
 * copies its arrays to HBM and runs this builder.  The handle owns copies: the
 * caller may free its arrays on return.
 * Collective, canonical partition only (rank r holds rows [r blk, r blk + blk),
 * blk = ceil(n_global / P)).  dAp[0] == 0, dAp non-decreasing, dAp[nlocal] ==
 * nnz and every column in [0, n_global) are checked on the device; the ranks
 * agree on the outcome before anything indexes with a column and before every
 * collective step, so one rank's bad input makes EVERY rank return
 * LSSP_AMD_EINVAL (an allocation that fails on one: LSSP_AMD_ENOMEM on all),
 * with nothing left allocated.  A NULL ctx or A returns LSSP_AMD_EINVAL at once.
 * The halo list (flag, compact, sort, de-duplicate), the renumbering [owned |
 * halo] and the halo-free chunk run are made on the device; the halo list, P
 * counts, the send indices and two words per 256-row chunk cross to the host,
 * never O(nnz) data.  Peak device memory above the finished handle: 8 B per row
 * and 16 B per halo-column ENTRY (duplicates included) plus the radix sort's
 * scratch of about as much again, freed on return.  On one rank (no
 * communicator needed) there is no halo and no exchange. */
int lssp_amd_mat_from_device_dist(lssp_amd_ctx *ctx, int n_global, int row0, int nlocal, int nnz,
                                  const int *dAp, const int *dAj, const double *dAx, lssp_amd_mat **A);
/* The rank's diagonal block of A as a single-rank nlocal x nlocal handle B: the
 * entries of A whose column the rank owns, in A's entry order, made from A's
 * resident arrays (per-row counts, a scan, a fill).  B is equal in every
 * observable way to lssp_amd_mat_upload of the block cut out on the host, value
 * codes included; for an A without halo columns it is a copy of A.  A row left
 * without an entry stays empty (the create calls then refuse the missing
 * diagonal).  B is what lssp_amd_pc_create_dev / _ilut_create_dev /
 * _bilu_create_dev and, after a refresh, the refactor calls take for the rank's
 * block-Jacobi ILU; lssp_amd_solve(A, M) takes the block-Jacobi path.  Local, no
 * collective.  A NULL argument or a rank without rows: LSSP_AMD_EINVAL.  Peak
 * device memory above B: one more copy of the block (12 B per entry + 8 B per
 * row), freed on return. */
int lssp_amd_mat_local_block(lssp_amd_ctx *ctx, const lssp_amd_mat *A, lssp_amd_mat **B);
/* B's values again from the values A holds now (after
 * lssp_amd_mat_update_values on A), finished as lssp_amd_mat_update_values
 * finishes: the value codes rebuilt or dropped.  The device checks that A's
 * owned entries per row are B's row lengths; a mismatch, a distributed B or
 * another number of rows returns LSSP_AMD_EINVAL with B unchanged.  Local, no
 * collective; 8 B per entry of B are held until it returns. */
int lssp_amd_mat_local_block_refresh(lssp_amd_ctx *ctx, lssp_amd_mat *B, const lssp_amd_mat *A);

/* ---- device index arrays: the int members of lssp_mat_csr / lssp_mat_coo /
 *      lssp_mat_bcsr (type-defs.h:15-55) in HBM, as lssp_amd_vec_* for doubles */
int lssp_amd_idx_alloc(lssp_amd_ctx *ctx, long n, int **d);
int lssp_amd_idx_free(lssp_amd_ctx *ctx, int *d);
int lssp_amd_idx_upload(lssp_amd_ctx *ctx, int *d, const int *h, long n);
int lssp_amd_idx_download(lssp_amd_ctx *ctx, int *h, const int *d, long n);

/* ---- format conversions on the device (matrix-utils.h:22-49) --------------
 * Every array is DEVICE memory (idx_alloc / vec_alloc); outputs are caller
 * allocated and must not overlap the inputs.  Results are bitwise those of
 * the reference functions, entry order included.  Input structure is checked
 * on the device first (row pointers non-decreasing from 0 to nnz, indices
 * that address memory in range); a violation returns LSSP_AMD_EINVAL where the
 * reference would assert or read out of bounds.  With nnz == 0 the output row
 * pointers are all 0 (the reference leaves them unallocated). */
/* lssp_mat_csr_to_coo (matrix-utils.cxx:281-322): Ci[k] = row of entry k,
 * Cj/Cx copies.  Cj/Cx may be NULL (the caller keeps using Aj/Ax). */
int lssp_amd_csr_to_coo(lssp_amd_ctx *ctx, int nrows, int nnz, const int *Ap, const int *Aj,
                        const double *Ax, int *Ci, int *Cj, double *Cx);
/* lssp_mat_coo_to_csr (matrix-utils.cxx:324-380): rows bucketed in order,
 * entries of one row kept in input order (a stable sort by row); Ci must lie
 * in [0, nrows), column indices are copied unchecked as in the reference.
 * Ap holds nrows + 1. */
int lssp_amd_coo_to_csr(lssp_amd_ctx *ctx, int nrows, int nnz, const int *Ci, const int *Cj,
                        const double *Cx, int *Ap, int *Aj, double *Ax);
/* lssp_mat_transpose (matrix-utils.cxx:700-765): T (ncols x nrows), row c of
 * T lists the rows of A holding column c in increasing row order (entry
 * order within a row of A for duplicates).  Tp holds ncols + 1. */
int lssp_amd_csr_transpose(lssp_amd_ctx *ctx, int nrows, int ncols, int nnz, const int *Ap,
                           const int *Aj, const double *Ax, int *Tp, int *Tj, double *Tx);
/* lssp_mat_csr_to_bcsr (matrix-utils.cxx:62-162): n x n CSR (n % bs == 0,
 * nnz > 0, else EINVAL as lssp_error/assert there) to (n/bs)^2 blocks of
 * bs x bs, block columns of a block row ascending, each block COLUMN-major
 * (entry (r, c) at Bx[blk*bs*bs + (c%bs)*bs + r%bs]), absent entries 0, and a
 * duplicate (r, c) keeps its last value.  Two calls: with Bj == NULL only
 * *bnnz (number of blocks) is computed; then Bp (n/bs + 1), Bj (*bnnz) and
 * Bx (*bnnz * bs * bs) are filled. */
int lssp_amd_csr_to_bcsr(lssp_amd_ctx *ctx, int n, int nnz, int bs, const int *Ap, const int *Aj,
                         const double *Ax, int *bnnz, int *Bp, int *Bj, double *Bx);
/* lssp_mat_bcsr_to_csr (matrix-utils.cxx:164-215): the entries with
 * fabs(v) > 0 (zeros and NaNs are dropped, as there), each row's columns
 * sorted (lssp_mat_sort_column, :387-481: a row that was out of order gives
 * every duplicate column the value of its last occurrence).  Two calls: with
 * Aj == NULL only *nnz is computed (Ap may be NULL); then Ap (nbrows*bs + 1),
 * Aj and Ax (*nnz) are filled. */
int lssp_amd_bcsr_to_csr(lssp_amd_ctx *ctx, int nbrows, int nbcols, int bs, int bnnz, const int *Bp,
                         const int *Bj, const double *Bx, int *nnz, int *Ap, int *Aj, double *Ax);

/* ---- assembly on the device: the rest of matrix-utils.h and the matrix
 *      handle, for a CSR that already lives in HBM (an assembly kernel's, a
 *      coo_to_csr or bcsr_to_csr result).  Same conventions as the conversions
 *      above: device arrays, caller-allocated outputs that do not overlap the
 *      inputs, structure checked on the device first (LSSP_AMD_EINVAL), results
 *      bitwise the reference's.  COO in HBM -> lssp_amd_coo_to_csr ->
 *      lssp_amd_csr_sort_columns_dev -> lssp_amd_mat_from_device ->
 *      lssp_amd_solve runs without a host copy of the matrix.
 *      The tiled line-sweep ILU(0) of a natural-order 5-/7-point box is made
 *      from the matrix handle without a host copy either
 *      (lssp_amd_ilu_create_dev, below), and so is the ILU(1) of such a box on
 *      the skewed line sweeps, the reference's default level
 *      (lssp_amd_iluk_create_dev).  ILUT of any one-block matrix with sorted
 *      rows is factored on the device from the handle too
 *      (lssp_amd_ilut_create_dev): the matrix and the finished factors stay
 *      in HBM, where the sweeps' schedules are built too; factors that
 *      already live in HBM make a handle the same way
 *      (lssp_amd_ilu_from_factors_dev).  ILUK of any other one-block matrix
 *      with sorted rows, at any level, is made on the device as well, symbolic
 *      factorization included; lssp_amd_pc_create_dev is the one call that
 *      routes to all of them.  BILUK with blocks up to 8 x 8 is made on the
 *      device from the handle too (lssp_amd_bilu_create_dev).
 *      What still goes through the host: every other ILU setup
 *      (lssp_amd_ilu_create / lssp_amd_bilu_create take host arrays, as the
 *      reference factors on the host; download the CSR for them:
 *      block-Jacobi, BILUK with blocks beyond 8 x 8 or a block row without
 *      its diagonal block, a row without its diagonal), and the
 *      sliced copy of a windowed matrix (see lssp_amd_mat_from_device).  Both
 *      only when the PATTERN is new: new values on the same pattern stay on the
 *      device (lssp_amd_mat_update_values, lssp_amd_ilu_refactor /
 *      lssp_amd_iluk_refactor for the ILUK handles they serve and
 *      lssp_amd_bilu_refactor for packet-swept BILUK handles, below). */
/* lssp_mat_csr_is_sorted (matrix-utils.cxx:249-279): *sorted = 0 iff some row
 * holds neighbours Aj[k-1] > Aj[k] (equal neighbours are sorted); nnz == 0: 1.
 * Column values are compared only, never used as indices. */
int lssp_amd_csr_is_sorted(lssp_amd_ctx *ctx, int nrows, int nnz, const int *Ap, const int *Aj, int *sorted);
/* lssp_mat_bcsr_is_sorted (:217-247): the same over block rows / block columns */
int lssp_amd_bcsr_is_sorted(lssp_amd_ctx *ctx, int nbrows, int bnnz, const int *Bp, const int *Bj, int *sorted);
/* lssp_mat_sort_column (:387-481) in place on Aj / Ax, the device form of
 * lssp_amd_csr_sort_columns: a row without a descending neighbour pair is
 * left as it is (duplicates included); any other row comes out with ascending
 * columns, every duplicate column carrying the value of its last occurrence. */
int lssp_amd_csr_sort_columns_dev(lssp_amd_ctx *ctx, int nrows, int ncols, int nnz, const int *Ap, int *Aj,
                                  double *Ax);
/* lssp_mat_adjust_zero_diag (:483-587), n x n: a row without an entry Aj == i
 * gains (i, 1 * tol), appended and then moved left past the trailing entries
 * whose column is greater than i (it stops at the first that is not: no sort);
 * all other entries keep their order.  Two calls: with Mj == NULL only *mnnz =
 * nnz + number of rows without a diagonal is computed (Mp may be NULL); then
 * Mp (n + 1), Mj and Mx (*mnnz) are filled. */
int lssp_amd_csr_adjust_zero_diag(lssp_amd_ctx *ctx, int n, int nnz, const int *Ap, const int *Aj,
                                  const double *Ax, double tol, int *mnnz, int *Mp, int *Mj, double *Mx);
/* lssp_mat_get_block_diag (:589-698), n x n, nnz > 0 and blk > 0 (else EINVAL,
 * asserts there): blk == n copies the matrix; any other blk (greater than n
 * included) keeps of row i the entries whose column lies in the row's diagonal
 * block [i/blk*blk, min(that + blk, n)), in order, and gives a row left with
 * none the single entry (i, 1.0).  Two calls as above. */
int lssp_amd_csr_get_block_diag(lssp_amd_ctx *ctx, int n, int nnz, const int *Ap, const int *Aj,
                                const double *Ax, int blk, int *mnnz, int *Mp, int *Mj, double *Mx);
/* A matrix handle from DEVICE arrays, equal in every observable way to
 * lssp_amd_mat_upload of the same arrays (layout, bytes, every product and
 * solve bitwise).  The handle owns device-to-device copies: the caller may
 * free or reuse its arrays on return.  The SpMV's offset-id coding is built
 * on the GPU; at most 255 offsets and a few status words cross to the host.
 * A matrix that is not offset-coded and passes the window test (run on the
 * GPU) is downloaded ONCE (12 B per entry) for the host routine that lays out
 * its sliced copy; a matrix that fails it never leaves HBM.  Single rank only:
 * a distributed matrix comes from lssp_amd_mat_upload_dist. */
int lssp_amd_mat_from_device(lssp_amd_ctx *ctx, int nrows, int ncols, int nnz, const int *dAp,
                             const int *dAj, const double *dAx, lssp_amd_mat **A);

/* ---- new values on an unchanged pattern (no reference counterpart: the
 *      reference assembles solver and preconditioner again).  For time-stepping
 *      and Newton loops: everything that depends on the sparsity pattern alone
 *      (column coding, window layout, level lists, tiles, stream layout,
 *      hand-off buffers) is kept, and nothing crosses the host. */
/* dAx: DEVICE memory, nnz values in the entry order of the arrays the handle
 * was made from (lssp_amd_mat_upload, lssp_amd_mat_from_device,
 * lssp_amd_mat_upload_dist or lssp_amd_mat_from_device_dist).  Afterwards
 * every product and solve on A is bitwise that of a fresh handle made from the
 * same pattern with these values; lssp_amd_mat_layout / _bytes / _info answer
 * as before.  nnz other than the handle's or a NULL argument: LSSP_AMD_EINVAL
 * with A unchanged.  On a distributed matrix the call is local to the rank (its
 * values are its own: no collective) and builds no value codes; its products
 * are split at the halo rows, so coding them would take one more agreement
 * round.  Returns when the stream has finished. */
int lssp_amd_mat_update_values(lssp_amd_ctx *ctx, lssp_amd_mat *A, const double *dAx, int nnz);
/* Factor M again from the values A holds now, keeping every schedule.
 * Afterwards lssp_amd_ilu_apply / _apply_async / _trisolve / lssp_amd_solve /
 * lssp_amd_ilu_get_factors are bitwise those of a fresh
 * lssp_amd_ilu_create(ILUK, level 0) on the new values (the host copies of the
 * factor values are refreshed by the next lssp_amd_ilu_get_factors).
 * Eligible: M from lssp_amd_ilu_create with kind ILUK, level 0 and one block
 * (blk <= 0 or >= n) that runs the tiled line sweeps
 * (lssp_amd_ilu_sweep_layout: *line == 1 with 16 x 8 tiles).  Every other handle
 * -- from_factors / from_ldu, ILUT, level >= 1, block-Jacobi, BILUK, the
 * one-workgroup sweeps of a small 2-D grid (*lines == ny), general packet-swept
 * factors -- and a distributed A return LSSP_AMD_EUNSUPPORTED with M unchanged
 * and usable.  For a rank's block-Jacobi factor take lssp_amd_mat_local_block
 * first (and lssp_amd_mat_local_block_refresh before each refactor).
 * A must be n x n with exactly the factor's pattern (per row: L's strict part,
 * the diagonal, U's strict part), i.e. column-sorted rows that hold their
 * diagonal, as the matrix M was created from; compared on the device, a
 * mismatch returns LSSP_AMD_EINVAL with M unchanged.
 * The first call builds a plan kept until lssp_amd_ilu_destroy: the factor
 * pattern, a factor value buffer, the reciprocal pivots and the level lists,
 * 12 B per entry + 16 B per row of device memory; a handle that is never
 * refactored allocates none of it.  Returns when the stream has finished.  A
 * HIP error part-way returns LSSP_AMD_EHIP, after which M may only be
 * destroyed. */
int lssp_amd_ilu_refactor(lssp_amd_ctx *ctx, lssp_amd_ilu *M, const lssp_amd_mat *A);
/* The same for a BILUK handle: factor M again from the values A holds now, on
 * the block pattern M was created with.  Every schedule is kept and no matrix
 * or factor array crosses the host (two flag words are read back).  Afterwards
 * lssp_amd_ilu_apply / _apply_async + _check / _trisolve / lssp_amd_solve with M,
 * lssp_amd_ilu_get_factors and lssp_amd_ilu_get_diag are bitwise those of a
 * fresh lssp_amd_bilu_create(A's arrays, M's level, M's bs) -- hence of
 * lssp_amd_bilu_factor_host on the new values; lssp_amd_ilu_info and
 * _sweep_layout answer as before.  The host copies of L, U and the inverses
 * are refreshed by the next call that reads them (one download), and the
 * arrays a single sweep (lssp_amd_ilu_trisolve) built are dropped and rebuilt
 * by the next one.  All work is enqueued on the context's stream, after any
 * earlier lssp_amd_ilu_apply_async; the call returns when the stream has
 * finished.
 * Eligible: M from lssp_amd_bilu_create with bs <= 8 (the device numeric path)
 * whose two sweeps run on packet schedules.  An ILUK / ILUT handle, a handle
 * from lssp_amd_ilu_from_ldu / _from_factors, bs 9..32, a handle on the
 * sync-free fallback (a factor row longer than 24 entries) and a distributed A
 * return LSSP_AMD_EUNSUPPORTED with M unchanged and usable.  For a rank's
 * diagonal block take lssp_amd_mat_local_block first.
 * Pattern rule: A is n x n with M's n and has the BLOCK graph M was created
 * from -- every entry of A lies in a block the creating matrix had, and every
 * block the creating matrix had holds at least one entry of A.  The symbolic
 * pattern at M's level is then M's.  Inside blocks the scalar pattern is free:
 * A's nnz may differ, absent entries are 0.0, columns need not be sorted, and
 * of a duplicated column the last occurrence in storage order counts.  Checked
 * on the device (columns outside [0, n) included); a violation or another n
 * returns LSSP_AMD_EINVAL, as does an exactly singular diagonal block, with M
 * unchanged in both cases: the handle's record streams and inverses are
 * written last, after both flags are read.  NULL arguments: LSSP_AMD_EINVAL.
 * The first call builds a plan kept until lssp_amd_ilu_destroy: the block
 * pattern with each block's row and graph flag, the hit marks, two block value
 * buffers (scratch, and the committed values the refill and the host refresh
 * read), the scratch inverses and the level lists of the block rows --
 * 16 bs^2 + 10 B per block and 8 bs^2 + 12 B per block row of device memory;
 * a handle that is never refactored allocates none of it.  A HIP error
 * part-way returns LSSP_AMD_EHIP, after which M may only be destroyed. */
int lssp_amd_bilu_refactor(lssp_amd_ctx *ctx, lssp_amd_ilu *M, const lssp_amd_mat *A);
/* The same for any one-block ILUK handle: factor M again from the values A
 * holds now, keeping every schedule; no matrix or factor array crosses the
 * host (one flag word is read back).  Afterwards lssp_amd_ilu_apply /
 * _apply_async + _check / _trisolve / lssp_amd_solve with M and
 * lssp_amd_ilu_get_factors are bitwise those of a fresh
 * lssp_amd_ilu_create(ILUK, M's level) on the new values; lssp_amd_ilu_info and
 * _sweep_layout answer as before.  The host copies of the factor values are
 * refreshed by the next call that reads them (one download), and the arrays a
 * single sweep (lssp_amd_ilu_trisolve) built are dropped and rebuilt by the
 * next one.  All work is enqueued on the context's stream, after any earlier
 * lssp_amd_ilu_apply_async; the call returns when the stream has finished.
 * A superset of lssp_amd_ilu_refactor: a handle eligible there (one made by
 * lssp_amd_ilu_create_dev included) takes that path unchanged, so one call
 * serves every ILUK handle.  A level-1 handle lssp_amd_iluk_create_dev made is
 * eligible from birth (it carries its plan).  Newly eligible: M from lssp_amd_ilu_create with
 * kind ILUK, any level (negative: the default 1), one block (blk <= 0 or >= n),
 * whose sweeps run either on packet schedules (lssp_amd_ilu_sweep_layout: *line
 * == 0; general patterns, ILU(k >= 2) of stencils, boxes with holes) or on the
 * skewed ILU(1) line sweeps of a 7-point box (*line == 2 with 16 x 8 tiles: the
 * reference's default configuration).  ILUT (its pattern depends on the
 * values), block-Jacobi, from_factors / from_ldu and BILUK handles, the
 * one-workgroup sweeps of a small 2-D grid (*lines == ny), a factor on the
 * sync-free fallback (a strict row longer than 24 entries), a handle whose
 * single-sweep arrays were built while every pivot was exactly 1.0 (its U
 * sweeps never read the pivots), a handle whose creating matrix repeated a
 * column in a row, and a distributed A return LSSP_AMD_EUNSUPPORTED with M
 * unchanged and usable.  For a rank's diagonal block take
 * lssp_amd_mat_local_block first.
 * Pattern rule, checked on the device with nothing of A trusted: A is n x n
 * with M's n, every row's columns are strictly ascending and inside [0, n), and
 * A's pattern is exactly that of the creating matrix after its column sort (a
 * diagonal create had to insert stays absent).  At level >= 1 an entry of A on
 * a fill position of the factor is therefore refused: a fresh create would
 * build another symbolic pattern.  A violation, another n or a row range
 * outside [0, nnz) returns LSSP_AMD_EINVAL, NULL arguments too, with everything
 * a caller can read unchanged: nothing is written before the check has passed,
 * and nothing can refuse after it (scalar ILU(0) replaces tiny pivots).
 * Afterwards lssp_amd_ilu_get_schedule answers what it answers for a fresh
 * lssp_amd_ilu_create of the new values, its header word "unit" included (one
 * flag word comes back from the U sweep's refill for it).
 * The first call builds a plan kept until lssp_amd_ilu_destroy: the factor
 * pattern with one flag byte per entry (matrix entry, fill, inserted
 * diagonal), a factor value buffer, the reciprocal pivots, each row's diagonal
 * position and the level lists -- 13 B per factor entry + 20 B per row of
 * device memory; a handle that is never refactored allocates none of it (create
 * keeps the flag bytes on the host, 1 B per factor entry).  A HIP error part-way
 * returns LSSP_AMD_EHIP, after which M may only be destroyed. */
int lssp_amd_iluk_refactor(lssp_amd_ctx *ctx, lssp_amd_ilu *M, const lssp_amd_mat *A);
/* lssp_amd_ilu_create for a matrix that lives in HBM: the arguments have its
 * meaning, the matrix is the handle's device CSR.  No matrix array is copied to
 * the host, neither pattern nor values; a few words come back (row 0's entries,
 * which give nx and nx * ny, and the pattern check's flag).  The handle is
 * bitwise lssp_amd_ilu_create's of the same matrix -- applies, sweeps, solves,
 * lssp_amd_ilu_info, lssp_amd_ilu_get_factors (the host copies of the factors
 * are made on the first call that reads them) -- it owns copies of what it
 * needs, so A may be destroyed, and it is made with its refactor plan:
 * lssp_amd_ilu_refactor is eligible on it and builds nothing.
 * Eligible: kind ILUK, level 0, one block (blk <= 0 or >= n), A single-rank and
 * square with exactly the pattern of a complete natural-order 5-/7-point box
 * nx x ny (x nz), nx >= 2, ny >= 8 -- column-sorted rows (run
 * lssp_amd_csr_sort_columns_dev first when they may not be) that hold their
 * diagonal and every grid neighbour r -+ 1, r -+ nx, r -+ nx*ny that exists --
 * which lssp_amd_ilu_create would run on the 16 x 8 tiled line sweeps.
 * Everything else returns LSSP_AMD_EUNSUPPORTED with *out == NULL, A and ctx
 * untouched: ILUT, level >= 1 or < 0 (the reference's default level), block-
 * Jacobi, an unsorted row, a missing diagonal or neighbour, a matrix that is
 * no such box, a small 2-D grid on the one-workgroup sweeps
 * (lssp_amd_ilu_sweep_layout *lines == ny there), LSSP_AMD_LINE=0, a distributed
 * A (take its lssp_amd_mat_local_block first); use lssp_amd_ilu_create for those -- or lssp_amd_iluk_create_dev (below),
 * which also makes the level-1 handle on the device.  NULL arguments, a kind
 * that is neither ILUK nor ILUT, or nrows != ncols: LSSP_AMD_EINVAL.  A HIP
 * error part-way: LSSP_AMD_EHIP, everything freed.  Returns when the stream has
 * finished. */
int lssp_amd_ilu_create_dev(lssp_amd_ctx *ctx, const lssp_amd_mat *A, int kind, int level, double tol, int p,
                            int blk, lssp_amd_ilu **out);
/* The same for every device-made ILUK handle, the reference's default level
 * included (a superset of lssp_amd_ilu_create_dev, as lssp_amd_iluk_refactor is
 * of lssp_amd_ilu_refactor; the arguments are the same).  Whatever
 * lssp_amd_ilu_create_dev accepts goes to it unchanged.  Newly eligible: kind
 * ILUK, level 1 or level < 0 (the default, 1), one block (blk <= 0 or >= n), A
 * single-rank and square with exactly the pattern of a complete natural-order
 * box -- column-sorted rows that hold their diagonal and every grid neighbour
 * that exists; a 7-point box with nx >= 3, ny >= 3, nz >= 2 or a 5-point grid
 * with nx >= 3, ny >= 3 -- whose ILU(1) lssp_amd_ilu_create would run on the
 * skewed line sweeps (lssp_amd_ilu_sweep_layout: 2, 16, 8).  The factor
 * pattern, its fill flags, the level lists (row (i, j, k) is on level i + 2 j +
 * 3 k) and the sweeps' tiles then follow from the grid alone; the values go
 * through lssp_amd_iluk_refactor's own kernels.  No matrix array is copied to
 * the host (row 0's entries and flag words come back).  The handle is bitwise
 * lssp_amd_ilu_create(ILUK, level 1)'s of the same matrix in lssp_amd_ilu_apply
 * / _apply_async + _check / _trisolve / lssp_amd_solve, lssp_amd_ilu_info,
 * _sweep_layout and _get_factors (the host copies of the factors are made on
 * the first call that reads them); it owns what it needs, so A may be
 * destroyed, and it is made with its refactor plan, flag bytes included (13 B
 * per factor entry + 20 B per row): lssp_amd_iluk_refactor is eligible on it at
 * once and builds nothing.
 * LSSP_AMD_EUNSUPPORTED with *out == NULL, nothing allocated, A and ctx
 * untouched: ILUT, level >= 2, block-Jacobi, nx == 2 (or ny == 2), a small 2-D
 * grid on the one-workgroup sweeps (*lines == ny; LSSP_AMD_LINEG=0 keeps the
 * tiles), LSSP_AMD_LINE=0, a distributed A (take its lssp_amd_mat_local_block
 * first), an unsorted row, a missing diagonal or neighbour, any matrix that is
 * no such box; use lssp_amd_ilu_create for those.  NULL arguments, a kind that is neither ILUK nor ILUT, or nrows !=
 * ncols: LSSP_AMD_EINVAL.  A HIP error part-way: LSSP_AMD_EHIP, everything
 * freed.  Returns when the stream has finished. */
int lssp_amd_iluk_create_dev(lssp_amd_ctx *ctx, const lssp_amd_mat *A, int kind, int level, double tol, int p,
                             int blk, lssp_amd_ilu **out);
/* lssp_amd_ilu_create(kind ILUT) for a matrix that lives in HBM: ILUT(tol, p)
 * (pc-ilut.cxx:51-286) is factored on the device, one wavefront per row, each
 * row waiting per pivot for the earlier row it needs -- the reference's
 * arithmetic in the reference's order, so the factors are its factors bit for
 * bit.  tol < 0 means 1e-3, p <= 0 means ceil(nnz / n) (pc-ilut.cxx:436-438), as
 * in lssp_amd_ilu_create.
 * Host traffic: no array of A crosses to the host (two words of Ap and flag
 * words come back), and no array of the factors: the finished L and U stay
 * in HBM and the sweeps' packet schedules are built on the device, byte for
 * byte as lssp_amd_ilu_create builds them (lssp_amd_ilu_from_factors_dev's
 * builder; lssp_amd_ilu_get_schedule answers origin 1); the handle's host
 * copies are made by the first call that reads them.  Factors beyond that
 * builder (p > 24 entries in a strict row, the packet limits) are downloaded
 * once, 12 B per entry, and scheduled on the host as before version 1.9;
 * LSSP_AMD_SCHED_HOST=1 forces that route.
 * The handle is bitwise lssp_amd_ilu_create(LSSP_AMD_ILUT, ...)'s of the same
 * matrix in lssp_amd_ilu_apply / _apply_async + _check / _trisolve /
 * lssp_amd_solve, lssp_amd_ilu_info, _sweep_layout (0, 0, 0) and _get_factors;
 * it owns what it needs, so A may be destroyed.  It is an ILUT handle: both
 * refactor calls answer LSSP_AMD_EUNSUPPORTED for it.
 * Eligible: A single-rank and square, one block (blk <= 0 or >= n), every row
 * with strictly ascending columns inside [0, n) and its diagonal (checked on
 * the device, nothing trusted; lssp_amd_csr_sort_columns_dev sorts), and no
 * working row -- a row's L part or U part before the cut to p -- beyond
 * lssp_amd_ilut_capacity() entries (1024).
 * LSSP_AMD_EUNSUPPORTED with *out == NULL, nothing left allocated, A and ctx
 * usable: a distributed A (take its lssp_amd_mat_local_block first),
 * block-Jacobi, an unsorted row or a repeated column,
 * a missing diagonal (the reference inserts one first; that path is not
 * reproduced here), a working row beyond the capacity; use lssp_amd_ilu_create
 * for those.  NULL arguments or nrows != ncols: LSSP_AMD_EINVAL.  A bounded
 * wait of the kernel expired: LSSP_AMD_ETIMEOUT.  A HIP error part-way:
 * LSSP_AMD_EHIP, everything freed.  LSSP_AMD_SETUP_TIMES=1 prints the phases
 * (check, numeric, compaction, then per side check, levels, order, entries,
 * packets, fill; on the host route download, schedules).  Returns when the
 * stream has finished. */
int lssp_amd_ilut_create_dev(lssp_amd_ctx *ctx, const lssp_amd_mat *A, double tol, int p, int blk,
                             lssp_amd_ilu **out);
/* entries a working row of lssp_amd_ilut_create_dev (and of lssp_amd_pc_create_dev's
 * general ILUK route) may hold on each side of the diagonal */
int lssp_amd_ilut_capacity(void);
/* One call for every preconditioner handle made from a matrix that lives in
 * HBM; the arguments mean what they mean in lssp_amd_ilu_create_dev.  Routing:
 * kind ILUT goes to lssp_amd_ilut_create_dev(ctx, A, tol, p, blk, out), result
 * returned unchanged.  Kind ILUK (a negative level means the default, 1) first
 * tries lssp_amd_iluk_create_dev: a complete box keeps its line sweeps, and any
 * status other than LSSP_AMD_EUNSUPPORTED is returned as is.  What that call
 * refuses takes the general route, for one block (blk <= 0 or >= n) of a
 * single-rank A: the ILU(level) of ANY matrix whose rows have strictly ascending
 * columns inside [0, n) and hold their diagonal -- a thermal-like matrix, an
 * irregular mesh, a box with holes, level >= 2 of a stencil, an nx == 2 box.
 * The symbolic factorization (pc-iluk.cxx:22-135, the reference's level rule: a
 * repeated hit raises a level) runs on the device, one wavefront per row; the
 * values go through lssp_amd_iluk_refactor's own kernels; the factors are split
 * and the sweeps' packet schedules built on the device
 * (lssp_amd_ilu_get_schedule answers origin 1).  No array of A and no factor
 * array crosses to the host (flag words, two entry counts, Fp[n] and the level
 * lists' offsets come back); the host copies of the factors are made by their
 * first reader; A may be destroyed on return.
 * The general route's handle is bitwise lssp_amd_ilu_create(LSSP_AMD_ILUK,
 * level)'s of the same matrix in lssp_amd_ilu_apply / _apply_async + _check /
 * _trisolve / lssp_amd_solve, lssp_amd_ilu_info and _get_factors.
 * lssp_amd_ilu_sweep_layout answers (0, 0, 0): the route always runs the packet
 * sweeps (or, for factors beyond the device schedule builder -- a strict row
 * beyond 24 entries, the packet limits -- the host-built schedules, sync-free
 * fallback included, from one download of the factors).  In a few shapes
 * lssp_amd_ilu_create would pick a line route that the box creates refuse (the
 * one-workgroup 2-D grids, nx == 2, ny < 8 at level 0): there only the layout
 * answer differs -- every sweep is bitwise the reference's, so no result does.
 * The handle is made with its refactor plan, flag bytes included (13 B per
 * entry of the factor pattern + 20 B per row): on the packet sweeps
 * lssp_amd_iluk_refactor is eligible on it at once and builds nothing.
 * LSSP_AMD_EUNSUPPORTED from the general route, with *out == NULL, nothing left
 * allocated, A and ctx usable: block-Jacobi, a distributed A (take its
 * lssp_amd_mat_local_block first: the rank's slab then gets its line sweeps or
 * the general route like any matrix), a row whose
 * columns are not strictly ascending inside [0, n), a row without its diagonal
 * (the inserted-diagonal path is not reproduced; lssp_amd_csr_adjust_zero_diag
 * on the device makes such a matrix eligible), a working row beyond
 * lssp_amd_ilut_capacity() entries on one side of the diagonal, level > 254
 * (levels travel as bytes), a factor pattern beyond INT_MAX entries.  NULL
 * arguments, nrows != ncols, a kind that is neither ILUK nor ILUT:
 * LSSP_AMD_EINVAL.  A bounded wait of a kernel expired: LSSP_AMD_ETIMEOUT.  A
 * HIP error part-way: LSSP_AMD_EHIP, everything freed.  LSSP_AMD_SETUP_TIMES=1
 * prints the phases (check, symbolic, pack, levels, scatter, numeric, split,
 * then per side the schedule builder's; on the host route download,
 * schedules).  Returns when the stream has finished. */
int lssp_amd_pc_create_dev(lssp_amd_ctx *ctx, const lssp_amd_mat *A, int kind, int level, double tol, int p, int blk,
                           lssp_amd_ilu **out);
/* lssp_amd_bilu_create for a matrix that lives in HBM: BILUK, the reference's
 * block ILU(level) on bs x bs blocks, made on the device from the handle A.
 * Eligible: a single-rank square A, n % bs == 0, 1 <= bs <= 8 (the device numeric
 * path), every row's columns strictly ascending inside [0, n), every block row
 * holding at least one entry in its diagonal block.  A negative level means the
 * default, 1; levels up to 254 are accepted.
 * The route: the rows are checked; the block graph -- each block row's sorted
 * distinct block columns, a bs-way merge of its bs rows -- is built by a count
 * pass, a scan and a fill pass, one block row per lane; at level >= 1 the
 * symbolic ILU(level) of that graph is lssp_amd_pc_create_dev's, one wavefront per
 * block row (the reference's level rule); the level lists of the block rows come
 * from the device level pass; the values go through lssp_amd_bilu_refactor's own
 * scatter, numeric and U-scaling kernels; the factored blocks are expanded to the
 * point factors L and U in HBM, and both packet schedules are built there
 * (lssp_amd_ilu_get_schedule answers origin 1).  No array of A and no factor
 * array crosses to the host: flag words, block and entry counts, Bp[nb] and the
 * level lists' offsets come back.  The handle owns what it needs: A may be
 * destroyed on return.
 * The handle is bitwise lssp_amd_bilu_create(A's arrays, level, bs)'s in
 * lssp_amd_ilu_apply / _apply_async + _check / _trisolve / lssp_amd_solve,
 * lssp_amd_ilu_info, _get_factors and _get_diag, and in lssp_amd_ilu_get_schedule
 * apart from origin.  It is born with lssp_amd_bilu_refactor's plan (16 bs^2 + 10 B
 * per block and 8 bs^2 + 12 B per block row of device memory): the refactor is
 * eligible at once and builds nothing.  The host copies of L, U, the inverses
 * and the block pattern are made by the first call that reads them, from the
 * plan.  Factors beyond the device schedule builder (a strict row beyond 24
 * entries, e.g. bs = 8 at level 1 on a 7-point block grid, or the packet limits)
 * take the host-built schedules, sync-free fallback included, from one download
 * of the factored blocks; such a handle keeps no plan and lssp_amd_bilu_refactor
 * refuses it, as it refuses the host-made one.
 * LSSP_AMD_EUNSUPPORTED, with *out == NULL, nothing left allocated, A and ctx
 * usable: bs 9..32 (lssp_amd_bilu_create factors those on the host), a
 * distributed A (take its lssp_amd_mat_local_block first), a row whose columns
 * are not strictly ascending inside [0, n)
 * (lssp_amd_csr_sort_columns_dev sorts one), a block row without its diagonal
 * block -- lssp_amd_bilu_create gives such a row the identity as its inverse;
 * that path is not reproduced here, at any level --, a working block row beyond
 * lssp_amd_ilut_capacity() blocks on one side of the diagonal, level > 254, a
 * block pattern beyond INT_MAX blocks or bs^2 * blocks + n beyond INT_MAX.
 * LSSP_AMD_EINVAL: NULL arguments, nrows != ncols, n % bs != 0, bs outside 1..32,
 * an exactly singular diagonal block (the device numeric path's flag).
 * LSSP_AMD_ETIMEOUT: a bounded wait of the symbolic or the level pass expired.
 * LSSP_AMD_EHIP: a HIP error part-way, everything freed.  LSSP_AMD_SETUP_TIMES=1
 * prints the phases (check, block graph, graph check, symbolic, pack, levels,
 * scatter, numeric BILU(0), U scaling, expansion, then per side the schedule
 * builder's; on the host route download, schedules).  Returns when the stream
 * has finished. */
int lssp_amd_bilu_create_dev(lssp_amd_ctx *ctx, const lssp_amd_mat *A, int level, int bs, lssp_amd_ilu **out);

/* ---- synthetic inputs (example/exam.cxx:4-59 and its 7-pt analogue) ------ */
long lssp_amd_poisson_nnz(int dim, int N);
/* rows [row0, row0+nrows) of the 5-pt (dim 2) or 7-pt (dim 3) Laplacian */
int lssp_amd_poisson_rows(int dim, int N, long row0, long nrows, int *Ap, int *Aj, double *Ax);

#ifdef __cplusplus
}
#endif
#endif
