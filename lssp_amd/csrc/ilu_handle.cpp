// ilu_handle.cpp -- the life of an lssp_amd_ilu handle: the host and device
// creates, the refactors, the readers, the applies and the destroy (extern "C"
// entry points of include/lssp_amd.h; the rest of the C API is capi.cpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>

#include "iluk_refactor_dev.h"
#include "internal.h"

using namespace lssp_amd;

// ---- what every create shares -------------------------------------------------------
// The birth and the end of a create.  The handle is made with what says how it
// was made (c_kind 0: caller-made factors), build(M) runs under one try; on any
// failure the HIP error is cleared and the handle destroyed -- lssp_amd_ilu_destroy
// drains the stream first, so nothing of the handle is in flight when it is freed
// -- and *out stays as the caller left it; on success setup_seconds is stamped
// from clk and *out set.
static int create_handle(lssp_amd_ctx *c, int n, int kind, int level, int blk, const PhaseClock &clk,
                         lssp_amd_ilu **out, const std::function<int(lssp_amd_ilu *)> &build)
{
    lssp_amd_ilu *M = new lssp_amd_ilu();
    M->ctx = c;
    M->n = n;
    M->c_kind = kind;
    M->c_level = level;
    M->c_blk = blk;
    int st;
    try {
        st = build(M);
    } catch (const std::exception &) {
        st = LSSP_AMD_ENOMEM;
    }
    if (st != LSSP_AMD_OK) {
        (void)hipGetLastError();
        lssp_amd_ilu_destroy(M);
        return st;
    }
    M->setup_seconds = clk.total();
    *out = M;
    return LSSP_AMD_OK;
}

static void adopt_factors(lssp_amd_ilu *M, HostCSR &&L, HostCSR &&U)
{
    M->Lp = std::move(L.Ap);
    M->Lj = std::move(L.Aj);
    M->Lx = std::move(L.Ax);
    M->Up = std::move(U.Ap);
    M->Uj = std::move(U.Aj);
    M->Ux = std::move(U.Ax);
}

// the host copies of caller-made factors (from_factors, from_ldu)
static void copy_factors(lssp_amd_ilu *M, int n, const int *Lp, const int *Lj, const double *Lx, const int *Up,
                         const int *Uj, const double *Ux)
{
    M->Lp.assign(Lp, Lp + n + 1);
    M->Lj.assign(Lj, Lj + Lp[n]);
    M->Lx.assign(Lx, Lx + Lp[n]);
    M->Up.assign(Up, Up + n + 1);
    M->Uj.assign(Uj, Uj + Up[n]);
    M->Ux.assign(Ux, Ux + Up[n]);
}

// a plan's factored F as the line refills read it: both sweeps' view, L's diagonal the unit
static FactorView plan_view(const RefactorPlan &p) { return FactorView{p.d_Fp, p.d_Fj, p.d_Fx, p.d_dpos, true}; }

// the device creates' public prologue: *out cleared, then the arguments; any_kind: ILUK or ILUT
static int check_create_dev_args(lssp_amd_ctx *c, const lssp_amd_mat *A, bool any_kind, int kind, lssp_amd_ilu **out)
{
    if (out) *out = nullptr;
    if (!c || !A || !out) return LSSP_AMD_EINVAL;
    // a distributed A is out of scope, not a bad argument: its column space
    // [owned | halo] is not square, so it is answered before the shape test
    // (lssp_amd_mat_local_block makes the rank's square block)
    if (A->dist || A->nhalo > 0) return LSSP_AMD_EUNSUPPORTED;
    if (A->nrows <= 0 || A->nrows != A->ncols) return LSSP_AMD_EINVAL;
    if (any_kind && kind != LSSP_AMD_ILUK && kind != LSSP_AMD_ILUT) return LSSP_AMD_EINVAL;
    return LSSP_AMD_OK;
}

// the device creates' scope: one block (no block-Jacobi), one rank
static bool one_block_local(const lssp_amd_mat *A, int blk)
{
    return (blk <= 0 || blk >= A->nrows) && !A->dist && !(A->nhalo > 0);
}

// ---- the sweeps' schedules ------------------------------------------------------------
// the sync-free sweeps' level-ordered arrays (k_trisolve) of a general factor,
// built on first use: the apply's fallback when a factor has no packet
// schedule, and the single sweeps of lssp_amd_ilu_trisolve
// (the first lssp_amd_ilu_trisolve on a general factor builds them: the handle
// is mutated then, under its own lock).  Each factor is built on its own, and a
// build that fails part-way frees what it allocated, so a retry never
// overwrites live buffers.
static int sync_free_one(lssp_amd_ctx *c, int n, const std::vector<int> &Tp, const std::vector<int> &Tj,
                         const std::vector<double> &Tx, bool upper, TriSched &t)
{
    if (t.rp) return LSSP_AMD_OK;
    int st;
    try {
        st = build_trisched(c, n, Tp, Tj, Tx, upper, t, nullptr, false, true);
    } catch (const std::exception &) {
        st = LSSP_AMD_ENOMEM;
    }
    if (st != LSSP_AMD_OK) free_sync_free_arrays(t);
    return st;
}
static int ensure_sync_free(lssp_amd_ctx *c, lssp_amd_ilu *M)
{
    std::lock_guard<std::mutex> lk(M->sync_free_mu);
    LSSP_TRY(refactor_host_factors(M));  // a handle made on the device has no host factors yet
    LSSP_TRY(sync_free_one(c, M->n, M->Lp, M->Lj, M->Lx, false, M->lower));
    return sync_free_one(c, M->n, M->Up, M->Uj, M->Ux, true, M->upper);
}

static int ilu_upload(lssp_amd_ctx *c, lssp_amd_ilu *M)
{
    // structured ILU(0) of a 5-/7-point grid: line sweeps (linesweep.hip); the
    // packet schedules of the general sweeps are then not needed
    setup_mark(nullptr);
    // a BILUK handle always takes the general route: the line apply fuses the L
    // and U sweeps and has no place for the D stage between them (a bs = 1
    // BILUK of a grid would otherwise pass for a structured ILU(0))
    const int ls = M->bs > 0 ? LSSP_AMD_EUNSUPPORTED
                             : build_line_sweep(c, M->n, M->Lp, M->Lj, M->Lx, M->Up, M->Uj, M->Ux, M->line);
    if (ls != LSSP_AMD_OK && ls != LSSP_AMD_EUNSUPPORTED) return ls;
    setup_mark("line sweeps");
    // line sweeps serve every sweep of a structured factor: the packet and
    // sync-free schedules are then not built (only the level counts)
    const bool general = ls != LSSP_AMD_OK;
    // U's level pass (a sequential walk of the whole factor) runs beside L's
    // schedule build; U's build needs L's finished schedule
    std::vector<int> levU;
    int stU = LSSP_AMD_OK, stL = LSSP_AMD_OK;
    std::thread tu([&] {
        try {
            SetupTimer tm;
            stU = tri_levels(M->n, M->Up, M->Uj, true, levU);
            tm.mark("U levels (thread)");
        } catch (const std::exception &) {
            stU = LSSP_AMD_ENOMEM;
        }
    });
    try {  // the thread is joined on every path
        stL = build_trisched(c, M->n, M->Lp, M->Lj, M->Lx, false, M->lower, nullptr, general, false);
    } catch (const std::exception &) {
        stL = LSSP_AMD_ENOMEM;
    }
    tu.join();
    LSSP_TRY(stL);
    LSSP_TRY(stU);
    LSSP_TRY(build_trisched(c, M->n, M->Up, M->Uj, M->Ux, true, M->upper, general ? &M->lower : nullptr, general,
                            false, &levU));
    // the sync-free sweeps' level-ordered arrays only when a factor has no
    // packet schedule (launch_ilu_apply falls back to them): at 256^3 ILUT they
    // are ~8 GB of host copies and uploads nothing else reads
    const bool fallback = general && !(M->lower.pk6_n > 0 && M->upper.pk6_n > 0);
    if (fallback) LSSP_TRY(ensure_sync_free(c, M));
    setup_mark("sweep schedules (L, U)");
    M->lower.h_pos.clear();
    M->lower.h_pos.shrink_to_fit();
    if (fallback) {  // the sync-free sweeps' intermediate vector
        LSSP_HIP(hipMalloc(&M->d_cache, sizeof(double) * std::max(M->n, 1)));
        LSSP_TRY(launch_fill(c, M->d_cache, M->n, TRI_SENTINEL));
    }
    if (M->bs > 0) {  // BILUK: the inverted diagonal blocks and the middle stage's output
        LSSP_HIP(hipMalloc(&M->d_Dinv, sizeof(double) * std::max<size_t>(M->Dinv.size(), 1)));
        LSSP_HIP(hipMemcpyAsync(M->d_Dinv, M->Dinv.data(), sizeof(double) * M->Dinv.size(), hipMemcpyHostToDevice,
                                c->stream));
        LSSP_HIP(hipMalloc(&M->d_mid, sizeof(double) * std::max(M->n, 1)));
    }
    LSSP_HIP(hipStreamSynchronize(c->stream));
    return LSSP_AMD_OK;
}

// Both packet schedules of factors F in HBM from the device builder (tri_sched.hip;
// DESIGN.md 3.5a), and the counts the handle reports while it has no host copies.
// EUNSUPPORTED: beyond the device builder (a strict row beyond 24 entries, the
// packet limits); what it had built is freed, the handle is host_schedules' to finish.
static int device_schedules(lssp_amd_ctx *c, lssp_amd_ilu *M, const IlutDevFactors &F, PhaseClock &clk)
{
    M->dev_nnzL = F.nnzL;
    M->dev_nnzU = F.nnzU;
    M->host_missing = M->host_stale = true;
    int st = build_trisched_dev(c, M->n, F.nnzL, F.Lp, F.Lj, F.Lx, false, nullptr, M->lower, clk);
    if (st == LSSP_AMD_OK)
        st = build_trisched_dev(c, M->n, F.nnzU, F.Up, F.Uj, F.Ux, true, M->lower.bp_pos, M->upper, clk);
    LSSP_HIP(hipStreamSynchronize(c->stream));  // the caller's matrix may be destroyed on return, a scratch F freed
    if (st == LSSP_AMD_EUNSUPPORTED) {
        free_trisched(M->lower);
        free_trisched(M->upper);
    }
    return st;
}

// The schedules built on the host, sync-free fallback included (ilu_upload), for a
// handle a device create is making: its host copies first, where they are missing.
static int host_schedules(lssp_amd_ctx *c, lssp_amd_ilu *M, PhaseClock &clk)
{
    if (M->host_missing) {
        LSSP_TRY(refactor_host_factors(M));
        LSSP_TRY(clk.mark("download"));
    }
    setup_mark(nullptr);
    LSSP_TRY(ilu_upload(c, M));
    return clk.mark("schedules");
}

// ---- the host creates -------------------------------------------------------------------
// (their phases are setup_mark's lines; the clock gives setup_seconds)
static int ilu_create(lssp_amd_ctx *c, int kind, int n, const int *Ap, const int *Aj, const double *Ax, int level,
                      double tol, int p, int blk, lssp_amd_ilu **out)
{
    if (!c || !out || n <= 0 || (kind != LSSP_AMD_ILUK && kind != LSSP_AMD_ILUT)) return LSSP_AMD_EINVAL;
    LSSP_TRY(check_csr(n, n, Ap[n], Ap, Aj));
    if (Ap[n] < 1) return LSSP_AMD_EINVAL;
    LSSP_HIP(hipSetDevice(c->device));
    const PhaseClock clk(c, "create");
    setup_mark(nullptr);
    HostCSR A;
    A.n = n;
    A.ncols = n;
    A.Ap.assign(Ap, Ap + n + 1);
    A.Aj.assign(Aj, Aj + Ap[n]);
    A.Ax.assign(Ax, Ax + Ap[n]);
    sort_columns(A);  // lssp.cxx:173
    setup_mark("copy + column sort");
    if (kind == LSSP_AMD_ILUK && level < 0) level = 1;  // pc-iluk.cxx:583-592
    HostCSR L, U;
    int fst = LSSP_AMD_OK;
    std::vector<unsigned char> fin;  // what lssp_amd_iluk_refactor needs of the pattern: 1 B per factor entry, host
    ilu_factor(c, kind, std::move(A), level, tol < 0 ? 1e-3 : tol, p, blk, L, U, &fst, &fin);
    if (fst != LSSP_AMD_OK) return fst;
    return create_handle(c, n, kind, level, blk, clk, out, [&](lssp_amd_ilu *M) {
        M->fIn = std::move(fin);
        adopt_factors(M, std::move(L), std::move(U));
        return ilu_upload(c, M);
    });
}

// host setup allocates multi-GB vectors: an allocation the host refuses
// becomes LSSP_AMD_ENOMEM at the C-ABI instead of an exception
int lssp_amd_ilu_create(lssp_amd_ctx *c, int kind, int n, const int *Ap, const int *Aj,
                        const double *Ax, int level, double tol, int p, int blk, lssp_amd_ilu **out)
{
    try {
        return ilu_create(c, kind, n, Ap, Aj, Ax, level, tol, p, blk, out);
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

static int ilu_from_factors(lssp_amd_ctx *c, int n, const int *Lp, const int *Lj, const double *Lx, const int *Up,
                            const int *Uj, const double *Ux, lssp_amd_ilu **out)
{
    if (!c || !out || n <= 0) return LSSP_AMD_EINVAL;
    LSSP_TRY(check_csr(n, n, Lp[n], Lp, Lj));
    LSSP_TRY(check_csr(n, n, Up[n], Up, Uj));
    LSSP_HIP(hipSetDevice(c->device));
    const PhaseClock clk(c, "from_factors");
    return create_handle(c, n, 0, 0, 0, clk, out, [&](lssp_amd_ilu *M) {
        copy_factors(M, n, Lp, Lj, Lx, Up, Uj, Ux);
        return ilu_upload(c, M);
    });
}

int lssp_amd_ilu_from_factors(lssp_amd_ctx *c, int n, const int *Lp, const int *Lj, const double *Lx,
                              const int *Up, const int *Uj, const double *Ux, lssp_amd_ilu **out)
{
    try {
        return ilu_from_factors(c, n, Lp, Lj, Lx, Up, Uj, Ux, out);
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

// ---- the refactors ------------------------------------------------------------------------
// New values on the same pattern: the numeric ILU(0) again (k_ilu0_level over
// the kept level lists) and both coefficient streams rewritten from it
// (k_coef_refill); tiles, stream layout, hand-off buffers and claim counters
// stay as ilu_create left them.
static bool ilu0_tiled_handle(const lssp_amd_ilu *M)
{
    const LineILU &li = M->line;
    return M->c_kind == LSSP_AMD_ILUK && M->c_level == 0 && (M->c_blk <= 0 || M->c_blk >= M->n) && M->bs == 0 &&
           li.ntiles > 0 && li.kind == 0 && li.g2 == 0 && li.P * li.NJ <= 256;
}

int lssp_amd_ilu_refactor(lssp_amd_ctx *c, lssp_amd_ilu *M, const lssp_amd_mat *A)
{
    if (!c || !M || !A) return LSSP_AMD_EINVAL;
    const LineILU &li = M->line;
    if (!ilu0_tiled_handle(M) || A->dist) return LSSP_AMD_EUNSUPPORTED;
    if (A->nrows != M->n || A->ncols != M->n) return LSSP_AMD_EINVAL;
    const long fnnz = M->host_missing ? (long)M->dev_nnzL + M->dev_nnzU - M->n : (long)M->Lp[M->n] + M->Up[M->n] - M->n;
    if ((long)A->nnz != fnnz) return LSSP_AMD_EINVAL;
    try {
        LSSP_HIP(hipSetDevice(c->device));
        PhaseClock clk(c, "refactor", false);  // no drain: the steps below wait where they have to
        LSSP_TRY(refactor_plan_build(c, M));
        clk.mark("plan");
        int same = 0;
        LSSP_TRY(refactor_same_pattern(c, *M->rf, M->n, A->Ap, A->Aj, &same));
        if (!same) return LSSP_AMD_EINVAL;
        clk.mark("pattern compare");
        LSSP_TRY(refactor_numeric(c, *M->rf, M->n, A->Ax));
        M->host_stale = true;
        if (setup_times_on()) LSSP_HIP(hipStreamSynchronize(c->stream));
        clk.mark("numeric ILU(0)");
        LSSP_TRY(launch_line_refill(c, M->line, M->n, plan_view(*M->rf), plan_view(*M->rf)));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        clk.mark("coefficient streams");
        if (setup_times_on())  // the refill's traffic: each sweep reads F once and writes every slot of its stream
            fprintf(stderr, "lssp_amd refactor: refill bytes %lld\n",
                    2 * (4LL * (M->n + 1) + 12LL * M->rf->nnz) +
                        8LL * (li.L.rows_total * li.L.NA + li.U.rows_total * li.U.NA));
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
    return LSSP_AMD_OK;
}

// Any one-block ILUK handle on the packet sweeps or the skewed ILU(1) line
// sweeps: A's pattern matched against the kept flag bytes,
// its values scattered onto the factor pattern (fill +0.0), k_ilu0_level over
// the kept level lists, the sweeps' value arrays rewritten from the result.
// Schedules, layouts, shadows, hand-off buffers and claim counters stay as
// ilu_create left them.  A handle lssp_amd_ilu_refactor serves goes there.
int lssp_amd_iluk_refactor(lssp_amd_ctx *c, lssp_amd_ilu *M, const lssp_amd_mat *A)
{
    if (!c || !M || !A) return LSSP_AMD_EINVAL;
    if (ilu0_tiled_handle(M)) return lssp_amd_ilu_refactor(c, M, A);
    const LineILU &li = M->line;
    const bool packets = li.ntiles == 0 && M->lower.pk6_n > 0 && M->upper.pk6_n > 0;
    const bool linef = li.ntiles > 0 && li.kind == 1 && li.g2 == 0;
    // a handle lssp_amd_iluk_create_dev made is born with its plan, flag bytes
    // included: it needs neither the host flags nor the host factor copies
    const bool planned = M->rf && M->rf->d_fin;
    // upper.unit: the single sweeps' arrays were built while every pivot was
    // exactly 1.0, and the U sweeps then never read D
    const bool eligible = M->c_kind == LSSP_AMD_ILUK && (M->c_blk <= 0 || M->c_blk >= M->n) && M->bs == 0 &&
                          (planned || (!M->fIn.empty() && !M->host_missing)) && !M->upper.unit && (packets || linef);
    if (!eligible || A->dist) return LSSP_AMD_EUNSUPPORTED;
    if (A->nrows != M->n || A->ncols != M->n) return LSSP_AMD_EINVAL;
    try {
        LSSP_HIP(hipSetDevice(c->device));
        PhaseClock clk(c, "iluk_refactor");
        LSSP_TRY(refactor_plan_build(c, M, true));
        RefactorPlan &p = *M->rf;
        if (!p.d_fin) return LSSP_AMD_EUNSUPPORTED;
        LSSP_TRY(clk.mark("plan"));
        int ok = 0;
        LSSP_TRY(iluk_match(c, p, M->n, A->nnz, A->Ap, A->Aj, &ok));
        if (!ok) return LSSP_AMD_EINVAL;  // nothing written
        LSSP_TRY(clk.mark("match"));
        LSSP_TRY(iluk_scatter(c, p, M->n, A->Ap, A->Ax));
        LSSP_TRY(clk.mark("scatter"));
        LSSP_TRY(refactor_levels(c, p, M->n));
        LSSP_TRY(clk.mark("numeric"));
        int nonunit = 1;
        if (packets) {
            // d_flag is 0 here (iluk_match accepted the pattern); the U refill ORs it
            // when a pivot is not 1.0, which lssp_amd_ilu_get_schedule reports as a
            // fresh create would
            LSSP_TRY(launch_pk6_refill_scalar(c, M->lower, false, M->n, p.d_Fp, p.d_Fj, p.d_dpos, p.d_Fx));
            LSSP_TRY(launch_pk6_refill_scalar(c, M->upper, true, M->n, p.d_Fp, p.d_Fj, p.d_dpos, p.d_Fx, p.d_flag));
            LSSP_HIP(hipMemcpyAsync(&nonunit, p.d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        } else {
            LSSP_TRY(launch_linefill_refill(c, M->line, M->n, plan_view(p), plan_view(p)));
        }
        LSSP_HIP(hipStreamSynchronize(c->stream));
        if (packets) M->upper.bp_unit = nonunit ? 0 : 1;
        LSSP_TRY(clk.mark("refill"));
        // the device factors are ahead of Lx / Ux now, and of the sync-free arrays a
        // single sweep built from those: the next reader refreshes the host
        // copies, the next lssp_amd_ilu_trisolve rebuilds the arrays
        std::lock_guard<std::mutex> lk(M->sync_free_mu);
        M->host_stale = true;
        free_sync_free_arrays(M->lower);
        free_sync_free_arrays(M->upper);
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
    return LSSP_AMD_OK;
}

// ---- the device creates -------------------------------------------------------------------
// The box a device matrix claims to be, from row 0's few words and the entry
// count (both device creates): row 0 of a complete natural-order box holds {0,
// 1, nx, nx * ny} (2-D: {0, 1, nx}); strict = the stencil's entries on each side
// of the diagonal.  EUNSUPPORTED when no box has that row 0 and that count; the
// pattern itself is box_pattern_check's to judge.
static int box_geometry_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, long &nx, long &ny, long &nz, long &strict)
{
    const int n = A->nrows, nnz = A->nnz;
    if (nnz < 3) return LSSP_AMD_EUNSUPPORTED;
    int h_p[2] = {0, 0}, h_j[4] = {0, 0, 0, 0};
    LSSP_HIP(hipMemcpyAsync(h_p, A->Ap, sizeof(int) * 2, hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(h_j, A->Aj, sizeof(int) * std::min(nnz, 4), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    const int len0 = h_p[1] - h_p[0];
    if (h_p[0] != 0 || (len0 != 3 && len0 != 4) || len0 > nnz || h_j[0] != 0 || h_j[1] != 1)
        return LSSP_AMD_EUNSUPPORTED;
    nx = h_j[2];
    const long plane = len0 == 4 ? (long)h_j[3] : (long)n;
    if (nx < 2 || plane < nx || plane % nx || n % plane) return LSSP_AMD_EUNSUPPORTED;
    ny = plane / nx;
    nz = n / plane;
    if ((len0 == 4) != (nz > 1)) return LSSP_AMD_EUNSUPPORTED;
    strict = (nx - 1) * ny * nz + nx * (ny - 1) * nz + nx * ny * (nz - 1);
    if (2 * strict + n != (long)nnz) return LSSP_AMD_EUNSUPPORTED;
    return LSSP_AMD_OK;
}

// lssp_amd_ilu_create for a box matrix in HBM: what ilu_create builds on the
// host from the factors is built here from the grid (tiles, layouts, buffers:
// build_line_sweep_box) and on the device from the matrix (pattern check, level
// lists in closed form, k_ilu0_level, k_coef_refill).  The handle is born with
// its refactor plan; its host factor copies wait for a reader.
static int ilu_create_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, int kind, int level, int blk, lssp_amd_ilu **out)
{
    const int n = A->nrows, nnz = A->nnz;
    if (kind != LSSP_AMD_ILUK || level != 0 || !one_block_local(A, blk)) return LSSP_AMD_EUNSUPPORTED;
    LSSP_HIP(hipSetDevice(c->device));
    PhaseClock clk(c, "create_dev");
    long nx, ny, nz, strict;
    LSSP_TRY(box_geometry_dev(c, A, nx, ny, nz, strict));
    if (!line_box_tiled((int)nx, (int)ny, (int)nz)) return LSSP_AMD_EUNSUPPORTED;
    int ok = 0;
    LSSP_TRY(box_pattern_check(c, n, nnz, A->Ap, A->Aj, (int)nx, (int)ny, (int)nz, &ok));
    if (!ok) return LSSP_AMD_EUNSUPPORTED;
    LSSP_TRY(clk.mark("pattern check"));
    return create_handle(c, n, kind, level, blk, clk, out, [&](lssp_amd_ilu *M) -> int {
        LSSP_TRY(refactor_plan_from_box(c, n, nnz, A->Ap, A->Aj, (int)nx, (int)ny, (int)nz, &M->rf));
        LSSP_TRY(clk.mark("plan / levels"));
        LSSP_TRY(refactor_numeric(c, *M->rf, n, A->Ax));
        LSSP_TRY(clk.mark("numeric ILU(0)"));
        LSSP_TRY(build_line_sweep_box(c, (int)nx, (int)ny, (int)nz, M->line));
        LSSP_TRY(clk.mark("allocation + zeroing"));
        LSSP_TRY(launch_line_refill(c, M->line, n, plan_view(*M->rf), plan_view(*M->rf)));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        LSSP_TRY(clk.mark("coefficient streams"));
        // what ilu_upload's level passes report: row (i, j, k) is on level i + j + k of
        // L's DAG and on the mirrored level of U's
        M->lower.n = M->upper.n = n;
        M->lower.nlevels = M->upper.nlevels = (int)(nx + ny + nz - 2);
        M->host_missing = M->host_stale = true;
        M->dev_nnzL = M->dev_nnzU = (int)(strict + n);
        return LSSP_AMD_OK;
    });
}

int lssp_amd_ilu_create_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, int kind, int level, double tol, int p, int blk,
                            lssp_amd_ilu **out)
{
    (void)tol;  // ILUT's arguments: accepted as lssp_amd_ilu_create takes them, ILUT itself is not made here
    (void)p;
    LSSP_TRY(check_create_dev_args(c, A, true, kind, out));
    try {
        return ilu_create_dev(c, A, kind, level, blk, out);
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

// The same for the reference's default level: the ILU(1) of a complete box on
// the skewed k_linef sweeps.  The pattern-dependent pieces
// follow from the grid (F, its flags, diagonal positions and level lists in
// closed form: iluk_create_dev.h; tiles, layouts and buffers:
// build_linefill_box); the value-dependent ones are lssp_amd_iluk_refactor's
// (iluk_scatter, k_ilu0_level, k_linef_refill).
static int iluk1_create_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, int kind, int blk, lssp_amd_ilu **out)
{
    const int n = A->nrows, nnz = A->nnz;
    LSSP_HIP(hipSetDevice(c->device));
    PhaseClock clk(c, "iluk_create_dev");
    long nx, ny, nz, strict;
    LSSP_TRY(box_geometry_dev(c, A, nx, ny, nz, strict));
    if (!linefill_box_tiled((int)nx, (int)ny, (int)nz)) return LSSP_AMD_EUNSUPPORTED;
    const long fnnz = fill1_nnz((int)nx, (int)ny, (int)nz);
    if (fnnz > 0x7fffffffL) return LSSP_AMD_EUNSUPPORTED;
    int ok = 0;
    LSSP_TRY(box_pattern_check(c, n, nnz, A->Ap, A->Aj, (int)nx, (int)ny, (int)nz, &ok));
    if (!ok) return LSSP_AMD_EUNSUPPORTED;
    LSSP_TRY(clk.mark("pattern check"));
    return create_handle(c, n, kind, 1, blk, clk, out, [&](lssp_amd_ilu *M) -> int {
        LSSP_TRY(fill1_plan_pattern(c, n, (int)nx, (int)ny, (int)nz, &M->rf));
        LSSP_TRY(clk.mark("F pattern"));
        LSSP_TRY(fill1_plan_levels(c, *M->rf, n, (int)nx, (int)ny, (int)nz));
        LSSP_TRY(clk.mark("levels"));
        LSSP_TRY(iluk_scatter(c, *M->rf, n, A->Ap, A->Ax));
        LSSP_TRY(clk.mark("scatter"));
        LSSP_TRY(refactor_levels(c, *M->rf, n));
        LSSP_TRY(clk.mark("numeric"));
        LSSP_TRY(build_linefill_box(c, (int)nx, (int)ny, (int)nz, M->line));
        LSSP_TRY(clk.mark("allocation"));
        LSSP_TRY(launch_linefill_refill(c, M->line, n, plan_view(*M->rf), plan_view(*M->rf)));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        LSSP_TRY(clk.mark("refill"));
        // what ilu_upload's level passes report: row (i, j, k) is on level i + 2 j + 3 k
        // of L's DAG and on the mirrored level of U's
        M->lower.n = M->upper.n = n;
        M->lower.nlevels = M->upper.nlevels = (int)(nx + 2 * ny + 3 * nz - 5);
        M->host_missing = M->host_stale = true;
        M->dev_nnzL = M->dev_nnzU = (int)((fnnz + n) / 2);
        return LSSP_AMD_OK;
    });
}

int lssp_amd_iluk_create_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, int kind, int level, double tol, int p, int blk,
                             lssp_amd_ilu **out)
{
    LSSP_TRY(check_create_dev_args(c, A, true, kind, out));
    // level 0 (and everything lssp_amd_ilu_create_dev refuses for other reasons than the level)
    if (kind != LSSP_AMD_ILUK || level == 0) return lssp_amd_ilu_create_dev(c, A, kind, level, tol, p, blk, out);
    if (level < 0) level = 1;  // the default (pc-iluk.cxx:583-592)
    if (level != 1 || !one_block_local(A, blk)) return LSSP_AMD_EUNSUPPORTED;
    try {
        return iluk1_create_dev(c, A, kind, blk, out);
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

// lssp_amd_ilu_create(kind ILUT) for a matrix in HBM: ilut_factor_lu's row loop
// runs on the device, a wavefront per row (ilut_factor.hip), and
// the finished L and U stay in HBM, where the device schedule builder
// (tri_sched.hip) makes the sweeps' schedules byte for byte as
// ilu_upload makes them from host copies -- the handle is the host-made one bit
// for bit, its host copies made by their first reader.  What the device builder
// refuses takes the download and ilu_upload.  No array of A crosses to the host.
static int ilut_create_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, double tol, int p, int blk, lssp_amd_ilu **out)
{
    const int n = A->nrows, nnz = A->nnz;
    if (!one_block_local(A, blk) || nnz < n) return LSSP_AMD_EUNSUPPORTED;
    if (tol < 0) tol = 1e-3;
    if (p <= 0) p = (int)(((long)nnz + n - 1) / n);  // pc-ilut.cxx:436-438
    LSSP_HIP(hipSetDevice(c->device));
    PhaseClock clk(c, "ilut_create_dev");
    return create_handle(c, n, LSSP_AMD_ILUT, 0, blk, clk, out, [&](lssp_amd_ilu *M) -> int {
        // LSSP_AMD_SCHED_HOST=1: the schedules built on the host from a download, as before 1.9 (A/B)
        const bool host_route = getenv("LSSP_AMD_SCHED_HOST") && atoi(getenv("LSSP_AMD_SCHED_HOST"));  // read per call
        IlutDevFactors F;
        LSSP_TRY(ilut_factor_dev(c, n, nnz, A->Ap, A->Aj, A->Ax, tol, p, M->Lp, M->Lj, M->Lx, M->Up, M->Uj, M->Ux, clk,
                                 host_route ? nullptr : &F));
        if (host_route) return host_schedules(c, M, clk);
        // the finished factors stay in HBM, the handle's own now, and go through the device
        // schedule builder; the host copies are made by their first reader
        M->fd_Lp = F.Lp, M->fd_Lj = F.Lj, M->fd_Lx = F.Lx, M->fd_Up = F.Up, M->fd_Uj = F.Uj, M->fd_Ux = F.Ux;
        const int st = device_schedules(c, M, F, clk);
        return st == LSSP_AMD_EUNSUPPORTED ? host_schedules(c, M, clk) : st;
    });
}

int lssp_amd_ilut_capacity(void) { return ilut_capacity(); }

int lssp_amd_ilut_create_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, double tol, int p, int blk, lssp_amd_ilu **out)
{
    LSSP_TRY(check_create_dev_args(c, A, false, 0, out));
    try {
        return ilut_create_dev(c, A, tol, p, blk, out);
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

namespace {
// the general route's split of F into L and U: scratch of the schedule builder,
// freed on every path out of the build, once nothing of it is in flight
struct SplitScratch {
    lssp_amd_ctx *c;
    IlutDevFactors F;
    ~SplitScratch()
    {
        (void)hipStreamSynchronize(c->stream);
        iluk_split_free(&F);
    }
};
}  // namespace

// lssp_amd_pc_create_dev's general route: lssp_amd_ilu_create(kind
// ILUK, level) of any one-block matrix in HBM.  The symbolic ILU(k) factorization
// runs on the device, a wavefront per row (iluk_symbolic.hip), and leaves the
// plan lssp_amd_iluk_refactor works on -- F, its flag bytes, diagonal positions
// and level lists; the values are the refactor's own kernels' (iluk_scatter,
// k_ilu0_level); F is split into L and U on the device for the device schedule
// builder (tri_sched.hip), and the split is freed once both schedules stand:
// a finished TriSched keeps no pointer into the factor arrays it was built from,
// and the host copies are split from the plan's F by their first reader, so a
// later refactor leaves no stale factor copy behind.  What the device builder
// refuses takes the download and ilu_upload, as in ilut_create_dev.
static int iluk_general_create_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, int level, int blk, lssp_amd_ilu **out)
{
    const int n = A->nrows, nnz = A->nnz;
    if (!one_block_local(A, blk)) return LSSP_AMD_EUNSUPPORTED;
    LSSP_HIP(hipSetDevice(c->device));
    PhaseClock clk(c, "pc_create_dev");
    return create_handle(c, n, LSSP_AMD_ILUK, level, blk, clk, out, [&](lssp_amd_ilu *M) -> int {
        SplitScratch S{c};
        LSSP_TRY(iluk_symbolic_dev(c, n, nnz, A->Ap, A->Aj, level, &M->rf, clk));
        RefactorPlan &p = *M->rf;
        LSSP_TRY(iluk_split_pattern_dev(c, n, p, &S.F));
        LSSP_TRY(iluk_plan_levels_dev(c, n, p, S.F));
        LSSP_TRY(clk.mark("levels"));
        LSSP_TRY(iluk_scatter(c, p, n, A->Ap, A->Ax));
        LSSP_TRY(clk.mark("scatter"));
        LSSP_TRY(refactor_levels(c, p, n));
        LSSP_TRY(clk.mark("numeric"));
        LSSP_TRY(iluk_split_values_dev(c, n, p, S.F));
        LSSP_TRY(clk.mark("split"));
        const int st = device_schedules(c, M, S.F, clk);
        if (st != LSSP_AMD_EUNSUPPORTED) return st;
        iluk_split_free(&S.F);  // the host copies come from the plan's F
        return host_schedules(c, M, clk);
    });
}

int lssp_amd_pc_create_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, int kind, int level, double tol, int p, int blk,
                           lssp_amd_ilu **out)
{
    LSSP_TRY(check_create_dev_args(c, A, true, kind, out));
    if (kind == LSSP_AMD_ILUT) return lssp_amd_ilut_create_dev(c, A, tol, p, blk, out);
    if (level < 0) level = 1;  // the default (pc-iluk.cxx:583-592)
    // a complete box keeps its line sweeps
    const int st = lssp_amd_iluk_create_dev(c, A, kind, level, tol, p, blk, out);
    if (st != LSSP_AMD_EUNSUPPORTED) return st;
    *out = nullptr;
    try {
        return iluk_general_create_dev(c, A, level, blk, out);
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

// lssp_amd_ilu_from_factors for factors that live in HBM: the
// handle copies the six arrays device to device, both packet schedules are built
// on the device from the copies (tri_sched.hip), and the host copies are made by
// the first call that reads them (refactor_host_factors).  The handle always
// runs the packet sweeps: no line-sweep detection, no sync-free fallback.
static int ilu_from_factors_dev(lssp_amd_ctx *c, int n, const int *dLp, const int *dLj, const double *dLx,
                                const int *dUp, const int *dUj, const double *dUx, lssp_amd_ilu **out)
{
    LSSP_HIP(hipSetDevice(c->device));
    PhaseClock clk(c, "from_factors_dev");
    int h_n[4] = {0, 0, 0, 0};  // Lp[0], Lp[n], Up[0], Up[n]
    LSSP_HIP(hipMemcpyAsync(h_n + 0, dLp, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(h_n + 1, dLp + n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(h_n + 2, dUp, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(h_n + 3, dUp + n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (h_n[0] != 0 || h_n[2] != 0 || h_n[1] < n || h_n[3] < n) return LSSP_AMD_EINVAL;  // (a diagonal slot per row)
    return create_handle(c, n, 0, 0, 0, clk, out, [&](lssp_amd_ilu *M) -> int {
        auto copy = [&](auto *&d, const auto *src, size_t cnt) -> int {
            using T = typename std::remove_const<typename std::remove_pointer<decltype(src)>::type>::type;
            LSSP_HIP(hipMalloc(&d, sizeof(T) * std::max<size_t>(cnt, 1)));
            LSSP_HIP(hipMemcpyAsync(d, src, sizeof(T) * cnt, hipMemcpyDeviceToDevice, c->stream));
            return LSSP_AMD_OK;
        };
        LSSP_TRY(copy(M->fd_Lp, dLp, (size_t)n + 1));
        LSSP_TRY(copy(M->fd_Lj, dLj, (size_t)h_n[1]));
        LSSP_TRY(copy(M->fd_Lx, dLx, (size_t)h_n[1]));
        LSSP_TRY(copy(M->fd_Up, dUp, (size_t)n + 1));
        LSSP_TRY(copy(M->fd_Uj, dUj, (size_t)h_n[3]));
        LSSP_TRY(copy(M->fd_Ux, dUx, (size_t)h_n[3]));
        LSSP_TRY(clk.mark("copies"));
        const IlutDevFactors F{M->fd_Lp, M->fd_Lj, M->fd_Up, M->fd_Uj, M->fd_Lx, M->fd_Ux, h_n[1], h_n[3]};
        return device_schedules(c, M, F, clk);  // no fallback: what the device builder refuses is refused
    });
}

int lssp_amd_ilu_from_factors_dev(lssp_amd_ctx *c, int n, const int *dLp, const int *dLj, const double *dLx,
                                  const int *dUp, const int *dUj, const double *dUx, lssp_amd_ilu **out)
{
    if (out) *out = nullptr;
    if (!c || !out || n <= 0 || !dLp || !dLj || !dLx || !dUp || !dUj || !dUx) return LSSP_AMD_EINVAL;
    try {
        return ilu_from_factors_dev(c, n, dLp, dLj, dLx, dUp, dUj, dUx, out);
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

int lssp_amd_ilu_get_schedule(const lssp_amd_ilu *M, int which, int hdr[12], int *blk, int *desc, unsigned *rec,
                              int *idx, int *perm, int *pos)
{
    if (!M || !hdr || (which != 0 && which != 1)) return LSSP_AMD_EINVAL;
    // line sweeps and the sync-free fallback have no packet schedule
    if (M->line.ntiles > 0 || !(M->lower.pk6_n > 0 && M->upper.pk6_n > 0)) return LSSP_AMD_EUNSUPPORTED;
    const lssp_amd::TriSched &t = which ? M->upper : M->lower;
    if (t.pk6_nrec > INT_MAX || t.pk6_nidx > INT_MAX) return LSSP_AMD_EUNSUPPORTED;  // hdr holds ints
    const int h[12] = {t.bp_B,     t.bp_nb,         t.bp_nsteps,     t.pk6_n,   t.pk6_ep,  t.pk6_ext,
                       t.pk6_rows, (int)t.pk6_nrec, (int)t.pk6_nidx, t.bp_unit, t.nlevels, t.bp_origin};
    memcpy(hdr, h, sizeof(h));
    if (!blk && !desc && !rec && !idx && !perm && !pos) return LSSP_AMD_OK;
    lssp_amd_ctx *c = M->ctx;
    LSSP_HIP(hipSetDevice(c->device));
    auto down = [&](auto *dst, const auto *src, size_t cnt) -> int {
        if (dst) LSSP_HIP(hipMemcpyAsync(dst, src, sizeof(*dst) * cnt, hipMemcpyDeviceToHost, c->stream));
        return LSSP_AMD_OK;
    };
    LSSP_TRY(down(blk, t.pk6_blk, (size_t)t.bp_nb + 1));
    LSSP_TRY(down(desc, t.pk6_desc, std::max<size_t>(4 * (size_t)t.pk6_n, 1)));
    LSSP_TRY(down(rec, t.pk6_rec, (size_t)t.pk6_nrec));
    LSSP_TRY(down(idx, t.pk6_idx, (size_t)t.pk6_nidx));
    LSSP_TRY(down(perm, t.bp_perm, (size_t)M->n));
    LSSP_TRY(down(pos, t.bp_pos, (size_t)M->n));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    return LSSP_AMD_OK;
}

// ---- BILUK (pc-biluk.cxx) --------------------------------------------------------
// steps 1-4 of the setup on the host copy A; c != nullptr and bs <= 8: the
// numeric block ILU(0) on c's GPU (bilu_factor.hip), else on the host
// T: the factored BCSR (its pattern is what lssp_amd_bilu_refactor keeps); *level_out: the level used
static int bilu_factor(lssp_amd_ctx *c, int n, const int *Ap, const int *Aj, const double *Ax, int level, int bs,
                       HostCSR &L, HostCSR &U, std::vector<double> &inv, HostBCSR &T, int *level_out = nullptr)
{
    if (n <= 0 || !Ap || !Aj || !Ax || bs < 1 || bs > BILU_MAX_BS || n % bs != 0) return LSSP_AMD_EINVAL;
    LSSP_TRY(check_csr(n, n, Ap[n], Ap, Aj));
    if (Ap[n] < 1) return LSSP_AMD_EINVAL;
    if (level < 0) level = 1;  // pc.cxx: the reference's default iluk_level
    if (level_out) *level_out = level;
    setup_mark(nullptr);
    {
        HostCSR A;
        A.n = A.ncols = n;
        A.Ap.assign(Ap, Ap + n + 1);
        A.Aj.assign(Aj, Aj + Ap[n]);
        A.Ax.assign(Ax, Ax + Ap[n]);
        sort_columns(A);  // lssp.cxx:173
        LSSP_TRY(bilu_pattern(A, level, bs, T));
    }
    setup_mark("BILUK copy, BCSR, symbolic");
    const double t0 = wall_time();
    const bool dev = c && bs <= BILU_MAX_BS_DEV;
    LSSP_TRY(dev ? bilu0_factor_gpu(c, T, inv) : bilu0_factor_host(T, inv));
    if (setup_times_on())
        fprintf(stderr, "lssp_amd setup:   BILU(0) numeric (%s path)      %10.6f s\n", dev ? "device" : "host",
                wall_time() - t0);
    setup_mark("BILUK numeric");
    bilu_expand(T, inv, L, U);
    setup_mark("BILUK expansion to L, U");
    return LSSP_AMD_OK;
}

int lssp_amd_bilu_create(lssp_amd_ctx *c, int n, const int *Ap, const int *Aj, const double *Ax, int level, int bs,
                         lssp_amd_ilu **out)
{
    if (!c || !out) return LSSP_AMD_EINVAL;
    try {
        LSSP_HIP(hipSetDevice(c->device));
        const PhaseClock clk(c, "bilu_create");
        HostCSR L, U;
        std::vector<double> inv;
        HostBCSR T;
        int lvl = level;
        LSSP_TRY(bilu_factor(c, n, Ap, Aj, Ax, level, bs, L, U, inv, T, &lvl));
        return create_handle(c, n, 0, lvl, 0, clk, out, [&](lssp_amd_ilu *M) {
            M->bs = bs;
            if (bs <= BILU_MAX_BS_DEV) {  // what lssp_amd_bilu_refactor needs of the pattern: 5 B per block, host
                M->bBp = std::move(T.Bp);
                M->bBj = std::move(T.Bj);
                M->bIn = std::move(T.in_graph);
            }
            M->Dinv = std::move(inv);
            adopt_factors(M, std::move(L), std::move(U));
            return ilu_upload(c, M);
        });
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

// lssp_amd_bilu_create for a matrix in HBM: bilu_create_device
// (bilu_factor.hip) leaves the plan lssp_amd_bilu_refactor works on and the point
// factors L and U in HBM; both packet schedules come from the device builder,
// and the factors are freed once the schedules stand -- the host copies, block
// pattern included, are made from the plan by their first reader
// (bilu_refactor_host_factors).  What the device builder refuses takes the host
// copies and ilu_upload, as in iluk_general_create_dev; such a handle keeps no
// plan: lssp_amd_bilu_refactor refuses it as it refuses the host-made one.
static int bilu_create_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, int level, int bs, lssp_amd_ilu **out)
{
    const int n = A->nrows;
    LSSP_HIP(hipSetDevice(c->device));
    PhaseClock clk(c, "bilu_create_dev");
    return create_handle(c, n, 0, level, 0, clk, out, [&](lssp_amd_ilu *M) -> int {
        SplitScratch S{c};
        M->bs = bs;
        LSSP_TRY(bilu_create_device(c, M, A, level, bs, &S.F, clk));
        const size_t ninv = (size_t)n * bs;  // nb blocks of bs^2
        LSSP_HIP(hipMalloc(&M->d_Dinv, sizeof(double) * ninv));
        LSSP_HIP(hipMemcpyAsync(M->d_Dinv, M->brf->d_inv, sizeof(double) * ninv, hipMemcpyDeviceToDevice, c->stream));
        const int st = device_schedules(c, M, S.F, clk);
        if (st == LSSP_AMD_OK) {  // the middle stage's output, as ilu_upload gives a BILUK handle
            LSSP_HIP(hipMalloc(&M->d_mid, sizeof(double) * std::max(n, 1)));
            return LSSP_AMD_OK;
        }
        if (st != LSSP_AMD_EUNSUPPORTED) return st;
        iluk_split_free(&S.F);  // the host copies come from the plan
        LSSP_TRY(refactor_host_factors(M));
        LSSP_TRY(clk.mark("download"));
        (void)hipFree(M->d_Dinv);  // ilu_upload uploads the host copy
        M->d_Dinv = nullptr;
        bilu_plan_free(M->brf);
        M->brf = nullptr;
        return host_schedules(c, M, clk);
    });
}

int lssp_amd_bilu_create_dev(lssp_amd_ctx *c, const lssp_amd_mat *A, int level, int bs, lssp_amd_ilu **out)
{
    LSSP_TRY(check_create_dev_args(c, A, false, 0, out));
    if (bs < 1 || bs > BILU_MAX_BS || A->nrows % bs != 0) return LSSP_AMD_EINVAL;
    if (level < 0) level = 1;  // pc.cxx: the reference's default iluk_level
    // the device numeric path, one rank, levels that travel as bytes (iluk_symbolic_dev)
    if (bs > BILU_MAX_BS_DEV || !one_block_local(A, 0) || level > 254) return LSSP_AMD_EUNSUPPORTED;
    try {
        return bilu_create_dev(c, A, level, bs, out);
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

// New values on the same block pattern: scatter, graph compare, k_bilu0_level
// over the kept level lists, U scaling, both record streams refilled
// (bilu_factor.hip bilu_refactor_device); packet schedules, shadows and claim
// counters stay as lssp_amd_bilu_create left them.
int lssp_amd_bilu_refactor(lssp_amd_ctx *c, lssp_amd_ilu *M, const lssp_amd_mat *A)
{
    if (!c || !M || !A) return LSSP_AMD_EINVAL;
    // (a handle lssp_amd_bilu_create_dev made has its plan, and its host pattern only once something read it)
    const bool eligible = M->bs >= 1 && M->bs <= BILU_MAX_BS_DEV && (M->brf || !M->bBp.empty()) &&
                          M->line.ntiles == 0 && M->lower.pk6_n > 0 && M->upper.pk6_n > 0 && M->d_Dinv;
    if (!eligible || A->dist) return LSSP_AMD_EUNSUPPORTED;
    if (A->nrows != M->n || A->ncols != M->n) return LSSP_AMD_EINVAL;
    try {
        LSSP_HIP(hipSetDevice(c->device));
        LSSP_TRY(bilu_refactor_device(c, M, A));
        // the device factors are ahead of Lx / Ux / Dinv now, and of the sync-free
        // arrays a single sweep built from those: the next reader refreshes the
        // host copies, the next lssp_amd_ilu_trisolve rebuilds the arrays
        std::lock_guard<std::mutex> lk(M->sync_free_mu);
        M->host_stale = true;
        free_sync_free_arrays(M->lower);
        free_sync_free_arrays(M->upper);
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
    return LSSP_AMD_OK;
}

int lssp_amd_bilu_factor_host(int n, const int *Ap, const int *Aj, const double *Ax, int level, int bs, int *nnzL,
                              int *nnzU, int *Lp, int *Lj, double *Lx, double *Dinv, int *Up, int *Uj, double *Ux)
{
    if (!nnzL || !nnzU) return LSSP_AMD_EINVAL;
    try {
        if (n <= 0 || !Ap || !Aj || !Ax || bs < 1 || bs > BILU_MAX_BS || n % bs != 0) return LSSP_AMD_EINVAL;
        if (!Lj) {  // size query: the pattern alone
            LSSP_TRY(check_csr(n, n, Ap[n], Ap, Aj));
            if (Ap[n] < 1) return LSSP_AMD_EINVAL;
            HostCSR A;
            A.n = A.ncols = n;
            A.Ap.assign(Ap, Ap + n + 1);
            A.Aj.assign(Aj, Aj + Ap[n]);
            A.Ax.assign(Ap[n], 0.0);
            sort_columns(A);
            HostBCSR T;
            LSSP_TRY(bilu_pattern(A, level < 0 ? 1 : level, bs, T));
            long nl = 0, nu = 0;
            for (int i = 0; i < T.nb; i++)
                for (int k = T.Bp[i]; k < T.Bp[i + 1]; k++) {
                    nl += T.Bj[k] < i;
                    nu += T.Bj[k] > i;
                }
            nl = nl * bs * bs + n;
            nu = nu * bs * bs + n;
            if (nl > INT_MAX || nu > INT_MAX) return LSSP_AMD_EINVAL;
            *nnzL = (int)nl;
            *nnzU = (int)nu;
            return LSSP_AMD_OK;
        }
        if (!Lp || !Lx || !Dinv || !Up || !Uj || !Ux) return LSSP_AMD_EINVAL;
        HostCSR L, U;
        std::vector<double> inv;
        HostBCSR T;
        LSSP_TRY(bilu_factor(nullptr, n, Ap, Aj, Ax, level, bs, L, U, inv, T));
        *nnzL = L.Ap[n];
        *nnzU = U.Ap[n];
        memcpy(Lp, L.Ap.data(), sizeof(int) * (n + 1));
        memcpy(Lj, L.Aj.data(), sizeof(int) * L.Aj.size());
        memcpy(Lx, L.Ax.data(), sizeof(double) * L.Ax.size());
        memcpy(Up, U.Ap.data(), sizeof(int) * (n + 1));
        memcpy(Uj, U.Aj.data(), sizeof(int) * U.Aj.size());
        memcpy(Ux, U.Ax.data(), sizeof(double) * U.Ax.size());
        memcpy(Dinv, inv.data(), sizeof(double) * inv.size());
        return LSSP_AMD_OK;
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

// L, D, U as the reference's host setup leaves them in pc.L / pc.D / pc.U: D is
// the block diagonal as CSR (lssp_pc_biluk_assemble_diag_mat, pc-biluk.cxx:279-314),
// every row of block i holding the bs columns i*bs .. i*bs + bs-1 in order
int lssp_amd_ilu_from_ldu(lssp_amd_ctx *c, int n, const int *Lp, const int *Lj, const double *Lx, const int *Dp,
                          const int *Dj, const double *Dx, const int *Up, const int *Uj, const double *Ux,
                          lssp_amd_ilu **out)
{
    if (!c || !out || n <= 0 || !Lp || !Lj || !Lx || !Dp || !Dj || !Dx || !Up || !Uj || !Ux) return LSSP_AMD_EINVAL;
    try {
        LSSP_TRY(check_csr(n, n, Lp[n], Lp, Lj));
        LSSP_TRY(check_csr(n, n, Up[n], Up, Uj));
        LSSP_TRY(check_csr(n, n, Dp[n], Dp, Dj));
        const int bs = Dp[1] - Dp[0];
        if (bs < 1 || bs > BILU_MAX_BS || n % bs != 0 || (long)Dp[n] != (long)n * bs) return LSSP_AMD_EINVAL;
        std::vector<double> inv((size_t)n * bs);
        for (int row = 0; row < n; row++) {
            const int b0 = row / bs * bs;
            if (Dp[row + 1] - Dp[row] != bs) return LSSP_AMD_EINVAL;
            for (int q = 0; q < bs; q++) {
                if (Dj[Dp[row] + q] != b0 + q) return LSSP_AMD_EINVAL;
                inv[(size_t)b0 * bs + (size_t)q * bs + (row - b0)] = Dx[Dp[row] + q];
            }
        }
        LSSP_HIP(hipSetDevice(c->device));
        const PhaseClock clk(c, "from_ldu");
        return create_handle(c, n, 0, 0, 0, clk, out, [&](lssp_amd_ilu *M) {
            M->bs = bs;
            M->Dinv = std::move(inv);
            copy_factors(M, n, Lp, Lj, Lx, Up, Uj, Ux);
            return ilu_upload(c, M);
        });
    } catch (const std::exception &) {
        return LSSP_AMD_ENOMEM;
    }
}

int lssp_amd_ilu_get_diag(const lssp_amd_ilu *M, int *bs, double *Dinv)
{
    if (!M || !bs) return LSSP_AMD_EINVAL;
    *bs = M->bs;
    // after lssp_amd_bilu_refactor the host copy is brought up to date here
    if (M->bs > 0 && Dinv) LSSP_TRY(refactor_host_factors(const_cast<lssp_amd_ilu *>(M)));
    if (M->bs > 0 && Dinv) memcpy(Dinv, M->Dinv.data(), sizeof(double) * M->Dinv.size());
    return LSSP_AMD_OK;
}

int lssp_amd_ilu_destroy(lssp_amd_ilu *M)
{
    if (!M) return LSSP_AMD_OK;
    if (M->ctx) (void)hipStreamSynchronize(M->ctx->stream);
    free_trisched(M->lower);
    free_trisched(M->upper);
    free_line_sweep(M->line);
    refactor_plan_free(M->rf);
    bilu_plan_free(M->brf);
    if (M->d_cache) (void)hipFree(M->d_cache);
    for (double *p : M->d_sh)
        if (p) (void)hipFree(p);
    if (M->d_rperm) (void)hipFree(M->d_rperm);
    for (void *q : {(void *)M->fd_Lp, (void *)M->fd_Lj, (void *)M->fd_Lx, (void *)M->fd_Up, (void *)M->fd_Uj,
                    (void *)M->fd_Ux})
        if (q) (void)hipFree(q);
    if (M->d_Dinv) (void)hipFree(M->d_Dinv);
    if (M->d_mid) (void)hipFree(M->d_mid);
    delete M;
    return LSSP_AMD_OK;
}

static int check_err(lssp_amd_ctx *c, const lssp_amd_ilu *M = nullptr)
{
    int e = 0;
    LSSP_HIP(hipMemcpyAsync(&e, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (e) {
        LSSP_HIP(hipMemset(c->d_err, 0, sizeof(int)));
        // a sweep that gave up mid-way leaves hand-off entries written: re-arm
        if (M && M->line.ntiles) {
            LSSP_TRY(line_rearm(c, const_cast<lssp_amd_ilu *>(M)->line));
            LSSP_HIP(hipStreamSynchronize(c->stream));
        }
        return LSSP_AMD_ETIMEOUT;
    }
    return LSSP_AMD_OK;
}

// solver-tri.cxx:48-60: cache = L^-1 rhs ; x = U^-1 cache.  The L sweep also
// arms x (sentinel) for the U sweep, the U sweep re-arms the cache.
int lssp_amd_ilu_apply(lssp_amd_ctx *c, const lssp_amd_ilu *M, double *x, const double *rhs)
{
    if (!c || !M || !x || !rhs) return LSSP_AMD_EINVAL;
    LSSP_TRY(launch_ilu_apply(c, M, x, rhs));
    return check_err(c, M);
}

// The same apply, only enqueued on the context's stream (no host round trip):
// for callers that pipeline applies with other work; a hand-off timeout of an
// enqueued apply is reported by lssp_amd_ilu_check.
int lssp_amd_ilu_apply_async(lssp_amd_ctx *c, const lssp_amd_ilu *M, double *x, const double *rhs)
{
    if (!c || !M || !x || !rhs) return LSSP_AMD_EINVAL;
    return launch_ilu_apply(c, M, x, rhs);
}

int lssp_amd_ilu_check(lssp_amd_ctx *c, const lssp_amd_ilu *M)
{
    if (!c || !M) return LSSP_AMD_EINVAL;
    return check_err(c, M);
}

int lssp_amd_ilu_trisolve(lssp_amd_ctx *c, const lssp_amd_ilu *M, int which, double *x, const double *rhs)
{
    if (!c || !M || !x || !rhs || x == rhs) return LSSP_AMD_EINVAL;
    if (M->line.ntiles) {
        LSSP_TRY(launch_line_sweep(c, M->line, which ? 1 : 0, x, rhs));
        return check_err(c, M);
    }
    LSSP_TRY(ensure_sync_free(c, const_cast<lssp_amd_ilu *>(M)));
    LSSP_TRY(launch_fill(c, x, M->n, TRI_SENTINEL));
    LSSP_TRY(launch_trisolve(c, which ? M->upper : M->lower, rhs, x, nullptr));
    return check_err(c);
}

int lssp_amd_ilu_info(const lssp_amd_ilu *M, int *n, int *nnzL, int *nnzU, int *levelsL, int *levelsU,
                      double *setup_seconds)
{
    if (!M) return LSSP_AMD_EINVAL;
    if (n) *n = M->n;
    if (nnzL) *nnzL = M->host_missing ? M->dev_nnzL : (int)M->Lj.size();
    if (nnzU) *nnzU = M->host_missing ? M->dev_nnzU : (int)M->Uj.size();
    if (levelsL) *levelsL = M->lower.nlevels;
    if (levelsU) *levelsU = M->upper.nlevels;
    if (setup_seconds) *setup_seconds = M->setup_seconds;
    return LSSP_AMD_OK;
}

int lssp_amd_ilu_sweep_layout(const lssp_amd_ilu *M, int *line, int *lines, int *planes)
{
    if (!M) return LSSP_AMD_EINVAL;
    const bool ls = M->line.ntiles > 0;
    if (line) *line = ls ? 1 + M->line.kind : 0;
    if (lines) *lines = ls ? M->line.NJ : 0;
    if (planes) *planes = ls ? M->line.P : 0;
    return LSSP_AMD_OK;
}

int lssp_amd_ilu_get_factors(const lssp_amd_ilu *M, int *Lp, int *Lj, double *Lx, int *Up, int *Uj,
                             double *Ux)
{
    if (!M) return LSSP_AMD_EINVAL;
    // after lssp_amd_ilu_refactor the host copies of the values are brought up to date here;
    // a handle made by lssp_amd_ilu_create_dev gets its host copies here
    if (Lx || Ux || M->host_missing) LSSP_TRY(refactor_host_factors(const_cast<lssp_amd_ilu *>(M)));
    if (Lp) memcpy(Lp, M->Lp.data(), sizeof(int) * M->Lp.size());
    if (Lj) memcpy(Lj, M->Lj.data(), sizeof(int) * M->Lj.size());
    if (Lx) memcpy(Lx, M->Lx.data(), sizeof(double) * M->Lx.size());
    if (Up) memcpy(Up, M->Up.data(), sizeof(int) * M->Up.size());
    if (Uj) memcpy(Uj, M->Uj.data(), sizeof(int) * M->Uj.size());
    if (Ux) memcpy(Ux, M->Ux.data(), sizeof(double) * M->Ux.size());
    return LSSP_AMD_OK;
}
