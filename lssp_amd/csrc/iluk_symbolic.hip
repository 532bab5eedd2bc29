// iluk_symbolic.hip -- lssp_amd_pc_create_dev's general ILUK route: the
// symbolic ILU(k) factorization of one block on the device (pc-iluk.cxx:22-135,
// restated on the host in iluk_symbolic, ilu_setup.cpp), the plan of the
// resulting pattern (flag bytes, diagonal positions, level lists of the numeric
// DAG) and the split of the factored F into L and U, all without a host pass.
// DESIGN.md 3.3f.
//
// Why the lanes of a wave may merge a pivot row's entries in any order
// (k_iluk_symbolic below): every slot's final level is the maximum of its
// initial level and of every admitted it = ulev + lev[k] + 1 that hits it (the
// reference RAISES a level on a repeated hit, pc-iluk.cxx:100-102), so it does
// not depend on the order of the hits.  Pivots are taken in ascending column
// order, as the reference's selection step takes them.  A pivot's level is final
// when it is taken: hits on column k come only from pivots k' < k, and new
// L-side fill always lies right of the current pivot (a pivot row's U part holds
// columns beyond the pivot).  Whether a column is admitted depends only on
// final levels (ulev of a finished row, lev[k] of a taken pivot), never on the
// working row's order.  The reference sorts F's rows afterwards (:342), so its
// discovery order is not observable; k_iluk_pack sorts each row by column.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "iluk_symbolic_dev.h"
#include "internal.h"

namespace lssp_amd {

namespace {

// ---------------------------------------------------------------------------
// The symbolic factorization, level >= 1.
//
// Row assignment: k_ilut's (ilut_factor.hip).  One wavefront (one 64-lane
// workgroup) per row at a time; the rows are cut into chunks of a.chunk
// consecutive rows, a wave draws the next chunk, in ascending order, from an
// atomic ticket and works through its rows in order.  A drawn chunk belongs to
// a running wave and every chunk below it has been drawn, so the smallest
// unfinished row depends only on finished rows: it can always progress,
// whatever the grid and whatever is co-resident, and the kernel cannot
// deadlock.  Every wait is still bounded (4 s of s_memrealtime): on expiry the
// row raises ctl[1], publishes an empty U part so that nobody waits for it,
// every row reached from then on is abandoned the same way, and the call
// returns LSSP_AMD_ETIMEOUT.
//
// Hand-off (cdna_hip_programming Guideline 16, R1 with the row's U count as the
// flag; ilut_factor.hip:87-95 with the count in the pivot's place): a finished
// row stores its staged U part -- the column words and their levels, one byte
// per level -- write-through (agent-scope stores), drains them (s_waitcnt
// vmcnt(0), every lane), then one lane stores the U count into ucnt[i] -- -1
// until then -- with one agent-scope store.  A consumer polls that one word, the
// whole wave together (no lane spins against a lane of its own wave), relaxed at
// agent scope with back-off; every load of the handed-off bytes is an
// agent-scope (L1-bypassing) load.  The L parts are read by the pack only.
//
// Capacity: the working row holds CAP entries on each side in LDS.  A row that
// needs more sets ctl[1]; from then on every row is abandoned as it is reached,
// the kernel drains, and the host retries with the large capacity or returns
// LSSP_AMD_EUNSUPPORTED.
// ---------------------------------------------------------------------------
constexpr int ILUK_CHUNK_MIN = 16, ILUK_CHUNK_MAX = 512;  // rows per chunk: n / (64 CUs) within these
constexpr int ILUK_CTL_OVERFLOW = 1, ILUK_CTL_TIMEOUT = 2;  // bits of ctl[1]
constexpr uint64_t ILUK_WAIT_TICKS = 400000000ull;  // 4 s at 100 MHz

struct IlukArgs {
    int n, level, stride, chunk;
    const int *Ap, *Aj;
    unsigned *sLj, *sUj;  // staging: row i's column words at iluk_stage_off(i, stride)
    unsigned char *sUl;   // the U parts' levels
    int *lcnt, *ucnt;     // entries of a row's L / U part; ucnt is the flag: -1 = row not finished
    int *ctl;             // [0] the chunk ticket, [1] capacity exceeded / wait expired
};

__device__ __forceinline__ int ldi_agent(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sti_agent(int *p, int v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned ldu_agent(const unsigned *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void stu_agent(unsigned *p, unsigned v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned char ldb_agent(const unsigned char *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void stb_agent(unsigned char *p, unsigned char v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// the whole wave polls one word; false: the bounded wait expired
__device__ __forceinline__ bool wait_count(const int *p, int &cnt)
{
    int v = __builtin_amdgcn_readfirstlane(ldi_agent(p));
    if (v < 0) {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        int nap = 1;
        for (;;) {
            for (int q = 0; q < nap; q++) __builtin_amdgcn_s_sleep(2);
            if (nap < 64) nap <<= 1;  // a long wait polls every ~3.5 us: thousands of waves wait at once
            v = __builtin_amdgcn_readfirstlane(ldi_agent(p));
            if (v >= 0) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 > ILUK_WAIT_TICKS) return false;
        }
    }
    asm volatile("" ::: "memory");  // the payload's loads stay below the poll
    cnt = v;
    return true;
}

// a row that is not factored (capacity exceeded somewhere, or its wait expired):
// nobody may wait for it
__device__ __forceinline__ void abandon_row(const IlukArgs &a, int i, int lane)
{
    if (lane == 0) {
        a.lcnt[i] = 0;
        sti_agent(a.ucnt + i, 0);
    }
}

template <int CAP>
__device__ __forceinline__ void iluk_row(const IlukArgs &a, const IlukRow &R, int i, int lane)
{
    const unsigned long long below = (1ull << lane) - 1;
    if (ldi_agent(a.ctl + 1) != 0) {
        abandon_row(a, i, lane);
        return;
    }
    const int b = a.Ap[i], e = a.Ap[i + 1];
    iluk_clear_lane(R, lane);
    __syncthreads();
    int nl = 0, nu = 0;
    for (int c = b; c < e; c += ILUT_LANES) {
        const int k = c + lane;
        const int col = k < e ? a.Aj[k] : i;  // (the diagonal has no slot)
        const bool isl = col < i, isu = col > i;
        const unsigned long long bl = __ballot(isl), bu = __ballot(isu);
        const int tl = __popcll(bl), tu = __popcll(bu);
        if (nl + tl > CAP || nu + tu > CAP) {
            if (lane == 0) atomicOr(a.ctl + 1, ILUK_CTL_OVERFLOW);
            abandon_row(a, i, lane);
            return;
        }
        const int at = isl ? nl + __popcll(bl & below) : iluk_upos(R, nu + __popcll(bu & below));
        if (isl || isu) iluk_load_lane(R, col, at);
        nl += tl;
        nu += tu;
    }
    __syncthreads();

    for (int j = 0; j < nl; j++) {
        // the selection step: the smallest remaining column comes to position j
        long long best = iluk_min_lane(R, j, nl, lane);
        for (int o = 32; o; o >>= 1) {
            const long long x = __shfl_xor(best, o);
            best = x < best ? x : best;
        }
        const int k = (int)(best >> 32), at = (int)(best & 0xffffffffll);
        if (lane == 0) iluk_swap(R, j, at);
        int cnt;
        if (!wait_count(a.ucnt + k, cnt)) {
            if (lane == 0) atomicOr(a.ctl + 1, ILUK_CTL_TIMEOUT);
            abandon_row(a, i, lane);
            return;
        }
        __syncthreads();
        const int plev = R.lv[j];
        // pivot row k's U part, 64 entries at a time (cnt <= the stride: only this kernel writes it)
        const long long off = iluk_stage_off(k, a.stride);
        for (int c = 0; c < cnt; c += ILUT_LANES) {
            const int kk = c + lane;
            bool valid = kk < cnt;
            const int col = valid ? iluk_stage_col(ldu_agent(a.sUj + off + kk)) : 0;
            const int it = valid ? iluk_it(ldb_agent(a.sUl + off + kk), plev) : 0;
            if (it > a.level || col == i) valid = false;
            const int q = valid ? iluk_lookup_lane(R, col) : -1;
            const bool fresh = valid && q == -1;
            // new entries are appended each side for itself
            const unsigned long long bl = __ballot(fresh && col < i), bu = __ballot(fresh && col > i);
            const int tl = __popcll(bl), tu = __popcll(bu);
            if (nl + tl > CAP || nu + tu > CAP) {
                if (lane == 0) atomicOr(a.ctl + 1, ILUK_CTL_OVERFLOW);
                abandon_row(a, i, lane);
                return;
            }
            const int pos = col < i ? nl + __popcll(bl & below) : iluk_upos(R, nu + __popcll(bu & below));
            __syncthreads();  // every lookup is done before the table changes
            if (valid) iluk_merge_lane(R, col, it, q, pos);
            __syncthreads();
            nl += tl;
            nu += tu;
        }
    }
    __syncthreads();

    // finish: the U part first, it is what other rows wait for
    const long long off = iluk_stage_off(i, a.stride);
    for (int k = lane; k < nu; k += ILUT_LANES) {
        stu_agent(a.sUj + off + k, iluk_stage_word(R.jw[iluk_upos(R, k)], R.og[iluk_upos(R, k)]));
        stb_agent(a.sUl + off + k, R.lv[iluk_upos(R, k)]);
    }
    drain_stores();
    if (lane == 0) sti_agent(a.ucnt + i, nu);
    for (int k = lane; k < nl; k += ILUT_LANES) a.sLj[off + k] = iluk_stage_word(R.jw[k], R.og[k]);
    if (lane == 0) a.lcnt[i] = nl;
    __syncthreads();  // the working row is read out before the next row clears it
}

template <int CAP>
__global__ __launch_bounds__(ILUT_LANES) void k_iluk_symbolic(IlukArgs a)
{
    __shared__ int s_jw[2 * CAP];
    __shared__ unsigned char s_lv[2 * CAP], s_og[2 * CAP];
    __shared__ int s_hk[4 * CAP], s_hv[4 * CAP];
    const IlukRow R{s_jw, s_lv, s_og, s_hk, s_hv, CAP};
    const int lane = threadIdx.x;
    const long nchunks = ((long)a.n + a.chunk - 1) / a.chunk;
    for (;;) {
        int c = 0;
        if (lane == 0) c = atomicAdd(a.ctl, 1);
        c = __builtin_amdgcn_readfirstlane(c);
        if (c >= nchunks || c < 0) break;
        const long end = std::min(((long)c + 1) * a.chunk, (long)a.n);
        for (long i = (long)c * a.chunk; i < end; i++) iluk_row<CAP>(a, R, (int)i, lane);
    }
}

// ---------------------------------------------------------------------------
// Compaction: the rows' entry counts (one slot more than n, so that the
// exclusive scan gives Fp[n]) and their 64-bit sum, then the pack -- one wave per
// row: the L part as it is (the selection step left it sorted), the diagonal,
// the U part sorted by column in LDS (by rank: the columns are distinct), each
// entry with its flag byte; dpos[i] = the diagonal's position.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_iluk_counts(int n, const int *__restrict__ lcnt, const int *__restrict__ ucnt,
                                                     int *__restrict__ cnt, unsigned long long *__restrict__ total)
{
    unsigned long long s = 0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i <= n; i += (long)gridDim.x * 256) {
        const int v = i < n ? iluk_count(lcnt[i], ucnt[i]) : 0;
        cnt[i] = v;
        s += (unsigned long long)v;
    }
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

__global__ __launch_bounds__(ILUT_LANES) void k_iluk_pack(IlukArgs a, const int *__restrict__ Fp, int *__restrict__ Fj,
                                                          unsigned char *__restrict__ fin, int *__restrict__ dpos)
{
    __shared__ unsigned s_w[ILUT_CAP_LARGE];
    const int lane = threadIdx.x;
    for (long i = blockIdx.x; i < a.n; i += gridDim.x) {
        const int nl = a.lcnt[i], nu = min(a.ucnt[i], ILUT_CAP_LARGE), o = Fp[i];
        const long long off = iluk_stage_off((int)i, a.stride);
        for (int k = lane; k < nl; k += ILUT_LANES) {
            const unsigned w = a.sLj[off + k];
            Fj[o + k] = iluk_stage_col(w);
            fin[o + k] = iluk_stage_origin(w);
        }
        if (lane == 0) {
            Fj[o + nl] = (int)i;
            fin[o + nl] = 1;
            dpos[i] = o + nl;
        }
        for (int k = lane; k < nu; k += ILUT_LANES) s_w[k] = a.sUj[off + k];
        __syncthreads();
        for (int k = lane; k < nu; k += ILUT_LANES) {
            const int r = iluk_rank(s_w, nu, k);
            Fj[o + nl + 1 + r] = iluk_stage_col(s_w[k]);
            fin[o + nl + 1 + r] = iluk_stage_origin(s_w[k]);
        }
        __syncthreads();
    }
}

// level 0: F is A's pattern; the diagonal's position in each (checked) row
__global__ __launch_bounds__(256) void k_iluk_dpos0(int n, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                    int *__restrict__ dpos)
{
    for (long r = blockIdx.x * 256L + threadIdx.x; r < n; r += (long)gridDim.x * 256) {
        int k = Ap[r];
        const int e = Ap[r + 1];
        while (k < e - 1 && (long)Aj[k] < r) k++;
        dpos[r] = k;
    }
}

// ---------------------------------------------------------------------------
// The level lists of the numeric DAG in the layout refactor_levels consumes:
// rows ordered by level, ascending inside a level (one stable sort of the rows
// by their level), and where each level begins.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_iluk_iota(int n, int *__restrict__ v)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) v[i] = (int)i;
}
// slev: the sorted levels.  Every level below the deepest has a row (a row of level l > 0 reads one of level l - 1)
__global__ __launch_bounds__(256) void k_iluk_level_off(int n, int nlev, const int *__restrict__ slev,
                                                        int *__restrict__ off)
{
    for (long p = blockIdx.x * 256L + threadIdx.x; p < n; p += (long)gridDim.x * 256) {
        const int l = slev[p];
        if (l >= 0 && l < nlev && (p == 0 || slev[p - 1] != l)) off[l] = (int)p;
        if (p == 0) off[nlev] = n;
    }
}

// ---------------------------------------------------------------------------
// The split of F into the factors the schedule builder reads: L = the strict
// part, then the unit diagonal LAST; U = the stored pivot FIRST, then the strict
// part (refactor_host_factors' layout, ilu_factor.hip).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_iluk_split_counts(int n, const int *__restrict__ Fp,
                                                           const int *__restrict__ dpos, int *__restrict__ cl,
                                                           int *__restrict__ cu)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i <= n; i += (long)gridDim.x * 256) {
        cl[i] = i < n ? dpos[i] - Fp[i] + 1 : 0;
        cu[i] = i < n ? Fp[i + 1] - dpos[i] : 0;
    }
}
// Fx == nullptr: the patterns only
__global__ __launch_bounds__(256) void k_iluk_split(int n, const int *__restrict__ Fp, const int *__restrict__ Fj,
                                                    const double *__restrict__ Fx, const int *__restrict__ dpos,
                                                    const int *__restrict__ Lp, const int *__restrict__ Up,
                                                    int *__restrict__ Lj, double *__restrict__ Lx,
                                                    int *__restrict__ Uj, double *__restrict__ Ux)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int f = Fp[i], d = dpos[i], e = Fp[i + 1], l = Lp[i], u = Up[i];
        if (Fx) {
            for (int k = f; k < d; k++) Lx[l + k - f] = Fx[k];
            Lx[l + d - f] = 1.0;
            for (int k = d; k < e; k++) Ux[u + k - d] = Fx[k];
        } else {
            for (int k = f; k < d; k++) Lj[l + k - f] = Fj[k];
            Lj[l + d - f] = (int)i;
            for (int k = d; k < e; k++) Uj[u + k - d] = Fj[k];
        }
    }
}

unsigned blocks_for(long long items) { return (unsigned)std::max<long long>(1, std::min<long long>((items + 255) / 256, 16384)); }

int scan_excl(lssp_amd_ctx *c, DevBufs &B, const int *in, int *out, size_t cnt)
{
    size_t bytes = 0;
    char *tmp = nullptr;
    LSSP_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0, cnt, rocprim::plus<int>(), c->stream));
    LSSP_HIP(B.get(&tmp, bytes));
    LSSP_HIP(rocprim::exclusive_scan(tmp, bytes, in, out, 0, cnt, rocprim::plus<int>(), c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));  // the scratch is freed next
    B.drop(tmp);
    return LSSP_AMD_OK;
}

template <int CAP>
int run_symbolic(lssp_amd_ctx *c, const IlukArgs &a0)
{
    // one workgroup per wave slot of the chip, as run_numeric launches k_ilut (ilut_factor.hip)
    IlukArgs a = a0;
    const long cus = std::max(c->num_cus, 1);
    a.chunk = (int)std::min<long>(std::max<long>(a.n / (64 * cus), ILUK_CHUNK_MIN), ILUK_CHUNK_MAX);
    const long nchunks = ((long)a.n + a.chunk - 1) / a.chunk;
    const long grid = std::max(1L, std::min(nchunks, 32 * cus));
    if (setup_times_on())
        fprintf(stderr, "lssp_amd pc_create_dev: capacity %d, grid %ld, chunks of %d rows\n", CAP, grid, a.chunk);
    LSSP_HIP(hipMemsetAsync(a.ucnt, 0xFF, sizeof(int) * (size_t)a.n, c->stream));  // -1: not finished
    LSSP_HIP(hipMemsetAsync(a.ctl, 0, 16, c->stream));
    k_iluk_symbolic<CAP><<<(unsigned)grid, ILUT_LANES, 0, c->stream>>>(a);
    LSSP_HIP(hipGetLastError());
    return LSSP_AMD_OK;
}

// the plan's buffers for a pattern of fnnz entries (d_rows and lev_off: iluk_plan_levels_dev)
int plan_alloc(RefactorPlan *p, int n, long fnnz)
{
    p->nnz = fnnz;
    LSSP_HIP(hipMalloc(&p->d_Fp, sizeof(int) * ((size_t)n + 1)));
    LSSP_HIP(hipMalloc(&p->d_Fj, sizeof(int) * (size_t)std::max(fnnz, 1L)));
    LSSP_HIP(hipMalloc(&p->d_Fx, sizeof(double) * (size_t)std::max(fnnz, 1L)));
    LSSP_HIP(hipMalloc(&p->d_dinv, sizeof(double) * (size_t)n));
    LSSP_HIP(hipMalloc(&p->d_rows, sizeof(int) * (size_t)n));
    LSSP_HIP(hipMalloc(&p->d_flag, sizeof(int)));
    LSSP_HIP(hipMalloc(&p->d_fin, (size_t)std::max(fnnz, 1L)));
    LSSP_HIP(hipMalloc(&p->d_dpos, sizeof(int) * (size_t)n));
    return LSSP_AMD_OK;
}

int symbolic_body(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, int level, RefactorPlan *p,
                  const std::function<int(const char *)> &mark)
{
    if (level == 0) {  // F is A's pattern, every entry an entry of A
        LSSP_TRY(plan_alloc(p, n, nnz));
        LSSP_HIP(hipMemcpyAsync(p->d_Fp, dAp, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToDevice, c->stream));
        LSSP_HIP(hipMemcpyAsync(p->d_Fj, dAj, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToDevice, c->stream));
        LSSP_HIP(hipMemsetAsync(p->d_fin, 1, (size_t)nnz, c->stream));
        k_iluk_dpos0<<<blocks_for(n), 256, 0, c->stream>>>(n, dAp, dAj, p->d_dpos);
        LSSP_HIP(hipGetLastError());
        return mark("symbolic");
    }
    DevBufs B;
    IlukArgs a{};
    a.n = n;
    a.level = level;
    a.Ap = dAp;
    a.Aj = dAj;
    LSSP_HIP(B.get(&a.ctl, 4));
    LSSP_HIP(B.get(&a.lcnt, n));
    LSSP_HIP(B.get(&a.ucnt, n));
    unsigned *sj = nullptr;
    unsigned char *sl = nullptr;
    bool done = false;
    for (int cap : {ILUT_CAP_SMALL, ILUT_CAP_LARGE}) {
        a.stride = cap;
        const size_t st = (size_t)iluk_stage_off(n, a.stride);
        if (sj) {  // the retry's staging areas replace the first try's
            B.drop(sj);
            B.drop(sl);
        }
        LSSP_HIP(B.get(&sj, 2 * st));
        LSSP_HIP(B.get(&sl, st));
        a.sLj = sj;
        a.sUj = sj + st;
        a.sUl = sl;
        LSSP_TRY(cap == ILUT_CAP_SMALL ? run_symbolic<ILUT_CAP_SMALL>(c, a) : run_symbolic<ILUT_CAP_LARGE>(c, a));
        int h_ctl[2] = {0, 0};
        LSSP_HIP(hipMemcpyAsync(h_ctl, a.ctl, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        if (h_ctl[1] & ILUK_CTL_TIMEOUT) return LSSP_AMD_ETIMEOUT;
        if (!h_ctl[1]) {
            done = true;
            break;
        }
    }
    if (!done) return LSSP_AMD_EUNSUPPORTED;  // a working row beyond the largest capacity
    LSSP_TRY(mark("symbolic"));

    int *cnt = nullptr;
    unsigned long long *total = nullptr, h_total = 0;
    LSSP_HIP(B.get(&cnt, (size_t)n + 1));
    LSSP_HIP(B.get(&total, 2));
    LSSP_HIP(hipMemsetAsync(total, 0, 16, c->stream));
    k_iluk_counts<<<blocks_for((long long)n + 1), 256, 0, c->stream>>>(n, a.lcnt, a.ucnt, cnt, total);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipMemcpyAsync(&h_total, total, sizeof(h_total), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (h_total > (unsigned long long)INT_MAX) return LSSP_AMD_EUNSUPPORTED;  // Fp holds ints
    LSSP_TRY(plan_alloc(p, n, (long)h_total));
    LSSP_TRY(scan_excl(c, B, cnt, p->d_Fp, (size_t)n + 1));
    k_iluk_pack<<<(unsigned)std::min<long>(n, 1L << 20), ILUT_LANES, 0, c->stream>>>(a, p->d_Fp, p->d_Fj, p->d_fin,
                                                                                  p->d_dpos);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(c->stream));  // the staging areas are freed next
    return mark("pack");
}

}  // namespace

int iluk_symbolic_dev(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, int level, RefactorPlan **out,
                      const std::function<int(const char *)> &mark)
{
    *out = nullptr;
    if (n < 1 || nnz < n || level < 0 || level > ILUK_LEVEL_MAX) return LSSP_AMD_EUNSUPPORTED;
    int ok = 0;
    LSSP_TRY(csr_rows_check_dev(c, n, nnz, dAp, dAj, &ok));
    if (!ok) return LSSP_AMD_EUNSUPPORTED;
    LSSP_TRY(mark("check"));
    RefactorPlan *p = new RefactorPlan();
    const int st = symbolic_body(c, n, nnz, dAp, dAj, level, p, mark);
    if (st != LSSP_AMD_OK) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);
        refactor_plan_free(p);
        return st;
    }
    *out = p;
    return LSSP_AMD_OK;
}

int iluk_split_pattern_dev(lssp_amd_ctx *c, int n, const RefactorPlan &p, IlutDevFactors *S)
{
    *S = IlutDevFactors();
    DevBufs B;
    int *cl = nullptr, *cu = nullptr;
    LSSP_HIP(B.get(&cl, (size_t)n + 1));
    LSSP_HIP(B.get(&cu, (size_t)n + 1));
    auto fill = [&]() -> int {
        LSSP_HIP(hipMalloc(&S->Lp, sizeof(int) * ((size_t)n + 1)));
        LSSP_HIP(hipMalloc(&S->Up, sizeof(int) * ((size_t)n + 1)));
        k_iluk_split_counts<<<blocks_for((long long)n + 1), 256, 0, c->stream>>>(n, p.d_Fp, p.d_dpos, cl, cu);
        LSSP_HIP(hipGetLastError());
        LSSP_TRY(scan_excl(c, B, cl, S->Lp, (size_t)n + 1));
        LSSP_TRY(scan_excl(c, B, cu, S->Up, (size_t)n + 1));
        LSSP_HIP(hipMemcpyAsync(&S->nnzL, S->Lp + n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipMemcpyAsync(&S->nnzU, S->Up + n, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        if (S->nnzL < n || S->nnzU < n || (long)S->nnzL + S->nnzU != p.nnz + n) return LSSP_AMD_EHIP;
        LSSP_HIP(hipMalloc(&S->Lj, sizeof(int) * (size_t)S->nnzL));
        LSSP_HIP(hipMalloc(&S->Lx, sizeof(double) * (size_t)S->nnzL));
        LSSP_HIP(hipMalloc(&S->Uj, sizeof(int) * (size_t)S->nnzU));
        LSSP_HIP(hipMalloc(&S->Ux, sizeof(double) * (size_t)S->nnzU));
        k_iluk_split<<<blocks_for(n), 256, 0, c->stream>>>(n, p.d_Fp, p.d_Fj, nullptr, p.d_dpos, S->Lp, S->Up, S->Lj,
                                                          S->Lx, S->Uj, S->Ux);
        LSSP_HIP(hipGetLastError());
        return LSSP_AMD_OK;
    };
    const int st = fill();
    if (st != LSSP_AMD_OK) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);
        iluk_split_free(S);
    }
    return st;
}

int iluk_split_values_dev(lssp_amd_ctx *c, int n, const RefactorPlan &p, const IlutDevFactors &S)
{
    k_iluk_split<<<blocks_for(n), 256, 0, c->stream>>>(n, p.d_Fp, p.d_Fj, p.d_Fx, p.d_dpos, S.Lp, S.Up, S.Lj, S.Lx,
                                                      S.Uj, S.Ux);
    LSSP_HIP(hipGetLastError());
    return LSSP_AMD_OK;
}

void iluk_split_free(IlutDevFactors *S)
{
    for (void *q : {(void *)S->Lp, (void *)S->Lj, (void *)S->Lx, (void *)S->Up, (void *)S->Uj, (void *)S->Ux})
        if (q) (void)hipFree(q);
    *S = IlutDevFactors();
}

int iluk_plan_levels_dev(lssp_amd_ctx *c, int n, RefactorPlan &p, const IlutDevFactors &S)
{
    DevBufs B;
    int *lev = nullptr, *slev = nullptr, *iota = nullptr, *off = nullptr;
    LSSP_HIP(B.get(&lev, n));
    int nlev = 0;
    LSSP_TRY(tri_levels_dev(c, n, S.Lp, S.Lj, false, lev, &nlev));
    if (nlev < 1 || nlev > n) return LSSP_AMD_EHIP;
    LSSP_HIP(B.get(&slev, n));
    LSSP_HIP(B.get(&iota, n));
    LSSP_HIP(B.get(&off, (size_t)nlev + 1));
    k_iluk_iota<<<blocks_for(n), 256, 0, c->stream>>>(n, iota);
    LSSP_HIP(hipGetLastError());
    unsigned end_bit = 1;
    while (end_bit < 32 && ((unsigned)(nlev - 1) >> end_bit)) end_bit++;
    size_t bytes = 0;
    char *tmp = nullptr;
    // (the levels are not negative: sorted as unsigned words over the bits they use)
    const unsigned *key = reinterpret_cast<const unsigned *>(lev);
    unsigned *skey = reinterpret_cast<unsigned *>(slev);
    LSSP_HIP(rocprim::radix_sort_pairs(nullptr, bytes, key, skey, iota, p.d_rows, (size_t)n, 0u, end_bit, c->stream));
    LSSP_HIP(B.get(&tmp, bytes));
    LSSP_HIP(rocprim::radix_sort_pairs(tmp, bytes, key, skey, iota, p.d_rows, (size_t)n, 0u, end_bit, c->stream));
    LSSP_HIP(hipMemsetAsync(off, 0xFF, sizeof(int) * ((size_t)nlev + 1), c->stream));
    k_iluk_level_off<<<blocks_for(n), 256, 0, c->stream>>>(n, nlev, slev, off);
    LSSP_HIP(hipGetLastError());
    p.lev_off.assign((size_t)nlev + 1, 0);
    LSSP_HIP(hipMemcpyAsync(p.lev_off.data(), off, sizeof(int) * ((size_t)nlev + 1), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    // the launches of refactor_levels take their bounds from these words: nothing but a partition of [0, n) passes
    if (p.lev_off[0] != 0 || p.lev_off[nlev] != n) return LSSP_AMD_EHIP;
    for (int l = 0; l < nlev; l++)
        if (p.lev_off[l + 1] <= p.lev_off[l]) return LSSP_AMD_EHIP;
    return LSSP_AMD_OK;
}

}  // namespace lssp_amd
