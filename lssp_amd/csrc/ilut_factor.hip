// ilut_factor.hip -- lssp_amd_ilut_create_dev: ILUT(tol, p) of one block factored
// on the device, a bitwise device form of ilut_factor_lu (ilu_setup.cpp;
// pc-ilut.cxx:51-286).  DESIGN.md 3.3e.
//
// The reference's row loop is sequential, but row i needs an earlier row
// finished only when it reaches that row as a pivot, and its arithmetic is
// order-sensitive only per working-row slot (updates accumulate in ascending
// pivot order) and in the storage order qsplit permutes.  So: one wavefront per
// row, waiting per pivot (k_ilut); the row body is ilut_dev.h's lane-level
// steps, which tools/ilut_dev_check.cpp runs on the host.
//
// Phases: eligibility check (k_ilut_check) -> numeric (k_ilut into per-row
// staging areas) -> compaction (counts, exclusive scan, k_ilut_pack).  The
// finished L and U then stay in HBM for the device schedule builder
// (tri_sched.hip), or -- on the host schedule route -- are
// downloaded once (12 B per factor entry) for ilu_upload / tri_bp.cpp.  No array
// of the matrix crosses to the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "ilut_dev.h"
#include "internal.h"

namespace lssp_amd {

namespace {

// ---------------------------------------------------------------------------
// Eligibility, nothing trusted: Ap starts at 0, ends at nnz and never
// descends; every row's columns ascend strictly inside [0, n) and hold the
// diagonal.  A row is read only when its range lies inside [0, nnz].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ilut_check(int n, int nnz, const int *__restrict__ Ap,
                                                    const int *__restrict__ Aj, int *__restrict__ flag)
{
    bool bad = false;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < n; r += (long)gridDim.x * 256) {
        const int a = Ap[r], b = Ap[r + 1];
        if (r == 0) bad |= a != 0;
        if (r == n - 1) bad |= b != nnz;
        if (a < 0 || b > nnz || b < a) {
            bad = true;
            continue;
        }
        int prev = -1;
        bool diag = false;
        for (int k = a; k < b; k++) {
            const int col = Aj[k];
            bad |= col <= prev || col >= n;
            diag |= (long)col == r;
            prev = col;
        }
        bad |= !diag;
    }
    if (bad) atomicOr(flag, 1);
}

// ---------------------------------------------------------------------------
// The numeric factorization.
//
// Row assignment: one wavefront (one 64-lane workgroup) per row at a time.  The
// rows are cut into chunks of a.chunk consecutive rows; a wave draws the next
// chunk, in ascending order, from an atomic ticket and works through its rows in
// order.  A chunk that has been drawn therefore belongs to a running wave, every
// chunk below it has been drawn too, and the smallest unfinished row -- the row
// its wave is at, as that wave's earlier rows are finished -- depends only on
// finished rows: it can always progress, whatever the grid and whatever is
// co-resident, so the kernel cannot deadlock (k_trisolve's argument,
// trisolve.hip, with the ticket in place of the static assignment, which would
// need every wave of the grid resident).  The chunk length sets how far the rows
// in flight reach: ILUT's independent rows of a stencil matrix lie many grid
// planes apart, so a chunk is n / (64 CUs) rows (16 .. 512), and at least 8
// waves per CU in flight then span an eighth of the matrix.
// Every wait is still bounded (4 s of s_memrealtime): a timeout raises
// ctx->d_err and ctl[1], the row publishes a poison pivot (NaN, no entries) so
// that no later row waits for it, every row reached from then on is abandoned
// the same way, and the call returns LSSP_AMD_ETIMEOUT.
//
// Hand-off (cdna_hip_programming Guideline 16, R1 with the pivot as the flag): a
// finished row stores its staged U part and its entry count write-through
// (agent-scope stores), drains them (s_waitcnt vmcnt(0), every lane), then one
// lane stores the guarded pivot into diag[i] -- TRI_SENTINEL until then -- with
// one 8-byte agent-scope store.  A consumer polls that one word, the whole wave
// together (no lane spins against a lane of its own wave), relaxed at agent
// scope with back-off; every load of the handed-off bytes is an agent-scope
// (L1-bypassing) load, so no L1 line can serve them stale.  Row 0's U part is
// A's row 0, read in place.  The L parts are read by the next kernel only.
//
// Capacity: the working row holds CAP entries on each side in LDS.  A row that
// needs more sets ctl[1]; from then on every row is abandoned as it is reached (it
// publishes the poison pivot), the kernel drains, and the host retries with the
// large capacity or returns LSSP_AMD_EUNSUPPORTED.
// ---------------------------------------------------------------------------
constexpr int ILUT_CHUNK_MIN = 16, ILUT_CHUNK_MAX = 512;  // rows per chunk: n / (64 CUs) within these
constexpr int ILUT_CTL_OVERFLOW = 1, ILUT_CTL_TIMEOUT = 2;  // bits of ctl[1]
constexpr int ILUT_ERR_TIMEOUT = 8;  // bit of ctx->d_err
constexpr uint64_t ILUT_WAIT_TICKS = 400000000ull;  // 4 s at 100 MHz

struct IlutArgs {
    int n, p, keep, chunk;
    double tol;
    const int *Ap, *Aj;
    const double *Ax;
    int *sLj, *sUj;      // staging: row i's kept entries at ilut_stage_off(i, keep)
    double *sLx, *sUx;
    int *lcnt, *ucnt;    // kept strict-L / U-part entries of a row
    double *diag;        // guarded pivots; TRI_SENTINEL = row not finished
    int *ctl;            // [0] the chunk ticket (before: the check's flag), [1] capacity exceeded / wait expired
    int *err;
};

__device__ __forceinline__ int ldi_agent(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sti_agent(int *p, int v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ldq_agent(const double *p)
{
    return __hip_atomic_load(reinterpret_cast<const uint64_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void stq_agent(double *p, uint64_t bits)
{
    __hip_atomic_store(reinterpret_cast<uint64_t *>(p), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// the pivot is the flag: a computed value with the sentinel's bits (a NaN payload
// no arithmetic here produces) is published as the default quiet NaN
__device__ __forceinline__ void publish_pivot(double *p, double v)
{
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if (b == TRI_SENTINEL) b = 0x7FF8000000000000ull;
    stq_agent(p, b);
}

// the whole wave polls one word; false: the bounded wait expired
__device__ __forceinline__ bool wait_pivot(const double *p, double &d)
{
    auto poll = [&]() -> uint64_t {
        const uint64_t b = ldq_agent(p);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32));
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(b & 0xffffffffull));
        return ((uint64_t)hi << 32) | (uint64_t)lo;  // (readfirstlane returns int: no sign extension)
    };
    uint64_t bits = poll();
    if (bits == TRI_SENTINEL) {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        int nap = 1;
        for (;;) {
            for (int q = 0; q < nap; q++) __builtin_amdgcn_s_sleep(2);
            if (nap < 64) nap <<= 1;  // a long wait polls every ~3.5 us: thousands of waves wait at once
            bits = poll();
            if (bits != TRI_SENTINEL) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 > ILUT_WAIT_TICKS) return false;
        }
    }
    asm volatile("" ::: "memory");  // the payload's loads stay below the poll
    d = __longlong_as_double((long long)bits);
    return true;
}

// a row that is not factored (capacity exceeded somewhere, or its wait expired):
// nobody may wait for it
__device__ __forceinline__ void abandon_row(const IlutArgs &a, int i, int lane)
{
    if (lane == 0) {
        a.lcnt[i] = 0;
        sti_agent(a.ucnt + i, 0);
    }
    drain_stores();
    if (lane == 0) stq_agent(a.diag + i, 0x7FF8000000000000ull);
}

template <int CAP>
__device__ __forceinline__ void ilut_row(const IlutArgs &a, const IlutRow &R, int i, int lane)
{
    const unsigned long long below = (1ull << lane) - 1;
    if (i == 0) {  // A's row as is (pc-ilut.cxx:89-96); its divisor is guarded, its stored pivot is not
        if (lane == 0) publish_pivot(a.diag, ilut_guard(a.Ax[a.Ap[0]]));
        return;
    }
    if (ldi_agent(a.ctl + 1) != 0) {
        abandon_row(a, i, lane);
        return;
    }
    const int b = a.Ap[i], e = a.Ap[i + 1];
    ilut_clear_lane(R, lane);
    __syncthreads();
    const double rel = a.tol * ilut_row_norm(a.Ax, b, e);
    int nl = 0, nu = 0;
    for (int c = b; c < e; c += ILUT_LANES) {
        const int k = c + lane;
        const bool valid = k < e;
        const int col = valid ? a.Aj[k] : 0;
        const double v = valid ? a.Ax[k] : 0.0;
        const bool isl = valid && col < i, isu = valid && col > i;
        const unsigned long long bl = __ballot(isl), bu = __ballot(isu);
        const int tl = __popcll(bl), tu = __popcll(bu);
        if (nl + tl > CAP || nu + tu > CAP) {
            if (lane == 0) atomicOr(a.ctl + 1, ILUT_CTL_OVERFLOW);
            abandon_row(a, i, lane);
            return;
        }
        const int at = isl ? nl + __popcll(bl & below) : ilut_upos(R, nu + __popcll(bu & below));
        if (valid) ilut_load_lane(R, i, col, v, at);
        nl += tl;
        nu += tu;
    }
    __syncthreads();

    const int a0 = a.Ap[0];
    const int len0 = a.Ap[1] - a0;
    for (int j = 0; j < nl; j++) {
        // the selection step: the smallest remaining column comes to position j
        long long best = ilut_min_lane(R, j, nl, lane);
        for (int o = 32; o; o >>= 1) {
            const long long x = __shfl_xor(best, o);
            best = x < best ? x : best;
        }
        const int jrow = (int)(best >> 32), at = (int)(best & 0xffffffffll);
        double d;
        if (!wait_pivot(a.diag + jrow, d)) {
            if (lane == 0) {
                atomicOr(a.err, ILUT_ERR_TIMEOUT);
                atomicOr(a.ctl + 1, ILUT_CTL_TIMEOUT);
            }
            abandon_row(a, i, lane);
            return;
        }
        if (lane == 0) {
            ilut_swap(R, j, at);
            R.w[j] = R.w[j] / d;
        }
        __syncthreads();
        const double aik = R.w[j];
        // pivot row jrow's U part in stored order, 64 entries at a time
        // (the entry loads are issued with the count's, over the staging area's whole
        // stride, and masked by the count when it arrives: one round trip, not two)
        const int cnt = jrow ? ldi_agent(a.ucnt + jrow) : len0;
        const int lim = jrow ? a.keep : len0;
        const long long off = jrow ? ilut_stage_off(jrow, a.keep) : (long long)a0;
        for (int c = 0;; c += ILUT_LANES) {
            const int k = c + lane;
            int col = 0;
            double u = 0.0;
            if (k < lim) {
                if (jrow) {
                    col = ldi_agent(a.sUj + off + k);
                    u = __longlong_as_double((long long)ldq_agent(a.sUx + off + k));
                } else {
                    col = a.Aj[off + k];
                    u = a.Ax[off + k];
                }
            }
            if (c >= cnt) break;
            bool valid = k < cnt;
            if (col <= jrow) valid = false;  // (row 0 of A: its diagonal)
            const double mx = ilut_mx(aik, u);
            const int q = valid ? ilut_lookup_lane(R, i, col) : -1;
            if (valid && !ilut_kept(q, mx, rel)) valid = false;
            const bool fresh = valid && q == -1;
            // new entries are appended in the pivot row's order, each side for itself
            const unsigned long long bl = __ballot(fresh && col < i), bu = __ballot(fresh && col > i);
            const int tl = __popcll(bl), tu = __popcll(bu);
            if (nl + tl > CAP || nu + tu > CAP) {
                if (lane == 0) atomicOr(a.ctl + 1, ILUT_CTL_OVERFLOW);
                abandon_row(a, i, lane);
                return;
            }
            const int pos = col < i ? nl + __popcll(bl & below) : ilut_upos(R, nu + __popcll(bu & below));
            __syncthreads();  // every lookup is done before the table changes
            if (valid) ilut_update_lane(R, col, mx, q, pos);
            __syncthreads();
            nl += tl;
            nu += tu;
        }
    }
    __syncthreads();

    // finish: the U part first, it is what other rows wait for
    const double d = ilut_guard(R.w[ilut_dpos(R)]);
    const int ku = nu < a.p ? nu : a.p, kl = nl < a.p ? nl : a.p;
    const long long off = ilut_stage_off(i, a.keep);
    if (lane == 0) ilut_qsplit(R.w + ilut_upos(R, 0), R.jw + ilut_upos(R, 0), nu, ku);
    __syncthreads();
    for (int k = lane; k < ku; k += ILUT_LANES) {
        sti_agent(a.sUj + off + k, R.jw[ilut_upos(R, k)]);
        stq_agent(a.sUx + off + k, (uint64_t)__double_as_longlong(R.w[ilut_upos(R, k)]));
    }
    if (lane == 0) sti_agent(a.ucnt + i, ku);
    drain_stores();
    if (lane == 0) publish_pivot(a.diag + i, d);
    if (lane == 0) ilut_qsplit(R.w, R.jw, nl, kl);
    __syncthreads();
    for (int k = lane; k < kl; k += ILUT_LANES) {
        a.sLj[off + k] = R.jw[k];
        a.sLx[off + k] = R.w[k];
    }
    if (lane == 0) a.lcnt[i] = kl;
    __syncthreads();  // the working row is read out before the next row clears it
}

template <int CAP>
__global__ __launch_bounds__(ILUT_LANES) void k_ilut(IlutArgs a)
{
    __shared__ int s_jw[2 * CAP + 1];
    __shared__ double s_w[2 * CAP + 1];
    __shared__ int s_hk[4 * CAP], s_hv[4 * CAP];
    const IlutRow R{s_jw, s_w, s_hk, s_hv, CAP};
    const int lane = threadIdx.x;
    const long nchunks = ((long)a.n + a.chunk - 1) / a.chunk;
    for (;;) {
        int c = 0;
        if (lane == 0) c = atomicAdd(a.ctl, 1);
        c = __builtin_amdgcn_readfirstlane(c);
        if (c >= nchunks || c < 0) break;
        const long end = std::min(((long)c + 1) * a.chunk, (long)a.n);
        for (long i = (long)c * a.chunk; i < end; i++) ilut_row<CAP>(a, R, (int)i, lane);
    }
}

// ---------------------------------------------------------------------------
// Compaction: the rows' entry counts (one slot more than n, so that the
// exclusive scan gives Lp[n] and Up[n]), then the pack -- one thread per slot of
// a row's staging area, grid-strided.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ilut_counts(int n, int len0, const int *__restrict__ lcnt,
                                                     const int *__restrict__ ucnt, int *__restrict__ cl,
                                                     int *__restrict__ cu)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i <= n; i += (long)gridDim.x * 256) {
        cl[i] = i < n ? ilut_count_l((int)i, lcnt[i]) : 0;
        cu[i] = i < n ? ilut_count_u((int)i, ucnt[i], len0) : 0;
    }
}

__global__ __launch_bounds__(256) void k_ilut_pack(IlutArgs a, int len0, const int *__restrict__ Lp,
                                                   const int *__restrict__ Up, int *__restrict__ Lj,
                                                   double *__restrict__ Lx, int *__restrict__ Uj,
                                                   double *__restrict__ Ux)
{
    const long long S = a.keep + 1, total = (long long)a.n * S;
    const long long g = blockIdx.x * 256LL + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long t = g; t < total; t += stride) {
        const int i = (int)(t / S), k = (int)(t % S);
        if (i == 0) continue;
        const int lc = a.lcnt[i], uc = a.ucnt[i];
        const long long off = ilut_stage_off(i, a.keep);
        if (k < lc) {
            Lj[Lp[i] + k] = a.sLj[off + k];
            Lx[Lp[i] + k] = a.sLx[off + k];
        } else if (k == lc) {
            Lj[Lp[i] + k] = i;
            Lx[Lp[i] + k] = 1.0;
        }
        if (k == 0) {
            Uj[Up[i]] = i;
            Ux[Up[i]] = a.diag[i];
        } else if (k <= uc) {
            Uj[Up[i] + k] = a.sUj[off + k - 1];
            Ux[Up[i] + k] = a.sUx[off + k - 1];
        }
    }
    const int a0 = a.Ap[0];
    for (long long t = g; t < len0; t += stride) {  // row 0: A's row in U, (0, 1.0) in L
        Uj[t] = a.Aj[a0 + t];
        Ux[t] = a.Ax[a0 + t];
    }
    if (g == 0) {
        Lj[0] = 0;
        Lx[0] = 1.0;
    }
}

unsigned blocks_for(long long items) { return (unsigned)std::min<long long>((items + 255) / 256, 65536); }

template <int CAP>
int run_numeric(lssp_amd_ctx *c, const IlutArgs &a0)
{
    // one workgroup per wave slot of the chip (32 per CU); the working row's LDS
    // decides how many the hardware keeps resident, and the ticket needs none of
    // them resident: a workgroup that starts late draws what is left, or nothing
    IlutArgs a = a0;
    const long cus = std::max(c->num_cus, 1);
    a.chunk = (int)std::min<long>(std::max<long>(a.n / (64 * cus), ILUT_CHUNK_MIN), ILUT_CHUNK_MAX);
    const long nchunks = ((long)a.n + a.chunk - 1) / a.chunk;
    const long grid = std::max(1L, std::min(nchunks, 32 * cus));
    if (setup_times_on())
        fprintf(stderr, "lssp_amd ilut_create_dev: capacity %d, grid %ld, chunks of %d rows\n", CAP, grid, a.chunk);
    LSSP_TRY(launch_fill(c, a.diag, a.n, TRI_SENTINEL));
    LSSP_HIP(hipMemsetAsync(a.ctl, 0, 16, c->stream));
    k_ilut<CAP><<<(unsigned)grid, ILUT_LANES, 0, c->stream>>>(a);
    LSSP_HIP(hipGetLastError());
    return LSSP_AMD_OK;
}

}  // namespace

int ilut_capacity() { return ILUT_CAP_LARGE; }

// k_ilut_check on its own (lssp_amd_pc_create_dev's general route shares the rule): one flag word read back
int csr_rows_check_dev(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, int *ok)
{
    *ok = 0;
    if (n < 1 || nnz < n) return LSSP_AMD_OK;
    DevBufs B;
    int *flag = nullptr;
    LSSP_HIP(B.get(&flag, 4));
    LSSP_HIP(hipMemsetAsync(flag, 0, 16, c->stream));
    k_ilut_check<<<blocks_for(n), 256, 0, c->stream>>>(n, nnz, dAp, dAj, flag);
    LSSP_HIP(hipGetLastError());
    int bad = 1;
    LSSP_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    *ok = !bad;
    return LSSP_AMD_OK;
}

int ilut_factor_dev(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, const double *dAx, double tol,
                    int p, std::vector<int> &Lp, std::vector<int> &Lj, std::vector<double> &Lx,
                    std::vector<int> &Up, std::vector<int> &Uj, std::vector<double> &Ux,
                    const std::function<int(const char *)> &mark, IlutDevFactors *keep)
{
    if (n < 1 || nnz < n) return LSSP_AMD_EUNSUPPORTED;
    DevBufs B;
    int *ctl = nullptr;
    LSSP_HIP(B.get(&ctl, 4));
    LSSP_HIP(hipMemsetAsync(ctl, 0, 16, c->stream));
    k_ilut_check<<<blocks_for(n), 256, 0, c->stream>>>(n, nnz, dAp, dAj, ctl);
    LSSP_HIP(hipGetLastError());
    int bad = 1, h_p[2] = {0, 0};
    LSSP_HIP(hipMemcpyAsync(&bad, ctl, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(h_p, dAp, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (bad) return LSSP_AMD_EUNSUPPORTED;
    const int len0 = h_p[1] - h_p[0];
    LSSP_TRY(mark("check"));

    IlutArgs a{};
    a.n = n;
    a.p = p;
    a.tol = tol;
    a.Ap = dAp;
    a.Aj = dAj;
    a.Ax = dAx;
    a.ctl = ctl;
    a.err = c->d_err;
    LSSP_HIP(B.get(&a.lcnt, n));
    LSSP_HIP(B.get(&a.ucnt, n));
    LSSP_HIP(B.get(&a.diag, n));
    int *sj = nullptr;
    double *sx = nullptr;
    bool done = false;
    for (int cap : {ILUT_CAP_SMALL, ILUT_CAP_LARGE}) {
        a.keep = ilut_keep(p, n, cap);
        if ((long long)n * (a.keep + 1) + len0 > (long long)INT_MAX) return LSSP_AMD_EUNSUPPORTED;
        const size_t st = (size_t)ilut_stage_off(n, a.keep);
        if (sj) {  // the retry's staging areas replace the first try's
            B.drop(sj);
            B.drop(sx);
        }
        LSSP_HIP(B.get(&sj, 2 * st));
        LSSP_HIP(B.get(&sx, 2 * st));
        a.sLj = sj;
        a.sUj = sj + st;
        a.sLx = sx;
        a.sUx = sx + st;
        LSSP_TRY(cap == ILUT_CAP_SMALL ? run_numeric<ILUT_CAP_SMALL>(c, a) : run_numeric<ILUT_CAP_LARGE>(c, a));
        int h_ctl[2] = {0, 0}, h_err = 0;
        LSSP_HIP(hipMemcpyAsync(h_ctl, ctl, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipMemcpyAsync(&h_err, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        if (h_err || (h_ctl[1] & ILUT_CTL_TIMEOUT)) {
            LSSP_HIP(hipMemset(c->d_err, 0, sizeof(int)));
            return LSSP_AMD_ETIMEOUT;
        }
        if (!h_ctl[1]) {
            done = true;
            break;
        }
    }
    if (!done) return LSSP_AMD_EUNSUPPORTED;  // a working row beyond the largest capacity
    LSSP_TRY(mark("numeric"));

    int *cl = nullptr, *cu = nullptr, *dLp = nullptr, *dUp = nullptr;
    LSSP_HIP(B.get(&cl, (size_t)n + 1));
    LSSP_HIP(B.get(&cu, (size_t)n + 1));
    LSSP_HIP(B.get(&dLp, (size_t)n + 1));
    LSSP_HIP(B.get(&dUp, (size_t)n + 1));
    k_ilut_counts<<<blocks_for((long long)n + 1), 256, 0, c->stream>>>(n, len0, a.lcnt, a.ucnt, cl, cu);
    LSSP_HIP(hipGetLastError());
    size_t bytes = 0;
    LSSP_HIP(rocprim::exclusive_scan(nullptr, bytes, cl, dLp, 0, (size_t)n + 1, rocprim::plus<int>(), c->stream));
    char *tmp = nullptr;
    LSSP_HIP(B.get(&tmp, bytes));
    LSSP_HIP(rocprim::exclusive_scan(tmp, bytes, cl, dLp, 0, (size_t)n + 1, rocprim::plus<int>(), c->stream));
    LSSP_HIP(rocprim::exclusive_scan(tmp, bytes, cu, dUp, 0, (size_t)n + 1, rocprim::plus<int>(), c->stream));
    int h_nnz[2] = {0, 0};
    LSSP_HIP(hipMemcpyAsync(h_nnz, dLp + n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(h_nnz + 1, dUp + n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    const size_t nnzL = (size_t)h_nnz[0], nnzU = (size_t)h_nnz[1];
    int *dLj = nullptr, *dUj = nullptr;
    double *dLx = nullptr, *dUx = nullptr;
    LSSP_HIP(B.get(&dLj, nnzL));
    LSSP_HIP(B.get(&dLx, nnzL));
    LSSP_HIP(B.get(&dUj, nnzU));
    LSSP_HIP(B.get(&dUx, nnzU));
    k_ilut_pack<<<blocks_for((long long)n * (a.keep + 1)), 256, 0, c->stream>>>(a, len0, dLp, dUp, dLj, dLx, dUj, dUx);
    LSSP_HIP(hipGetLastError());
    LSSP_TRY(mark("compaction"));

    if (keep) {  // the factors stay in HBM: the caller owns the six arrays from here on
        void *six[6] = {dLp, dLj, dLx, dUp, dUj, dUx};
        B.all.erase(std::remove_if(B.all.begin(), B.all.end(),
                                   [&](void *q) { return std::find(six, six + 6, q) != six + 6; }),
                    B.all.end());
        *keep = IlutDevFactors{dLp, dLj, dUp, dUj, dLx, dUx, (int)nnzL, (int)nnzU};
        return LSSP_AMD_OK;
    }
    Lp.resize((size_t)n + 1);
    Up.resize((size_t)n + 1);
    LSSP_HIP(hipMemcpyAsync(Lp.data(), dLp, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(Up.data(), dUp, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, c->stream));
    Lj.resize(nnzL);
    Lx.resize(nnzL);
    Uj.resize(nnzU);
    Ux.resize(nnzU);
    LSSP_HIP(hipMemcpyAsync(Lj.data(), dLj, sizeof(int) * nnzL, hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(Lx.data(), dLx, sizeof(double) * nnzL, hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(Uj.data(), dUj, sizeof(int) * nnzU, hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(Ux.data(), dUx, sizeof(double) * nnzU, hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    LSSP_TRY(mark("download"));
    return LSSP_AMD_OK;
}

}  // namespace lssp_amd
