// tri_sched.hip -- the packet schedule of k_tri_pk6 (trisolve.hip) built on the
// device from a triangular factor in HBM: byte for byte what build_bp_schedule
// and build_packets6 (tri_bp.cpp, sched_host.h) build on the host from a host
// copy.  DESIGN.md 3.5a.  The lane-level bodies are sched_dev.h's, which
// tools/sched_dev_check.cpp runs on the host against the host builder.
//
// Stages (each reproduces the host code named in sched_dev.h):
//   1 check + scalars   k_sched_check: tri_levels' rules, bandwidth, longest row, unit diagonal
//   2 levels            k_sched_levels: one lane per row, chunks of 64 sweep positions drawn in
//                       ascending order from a ticket; the level word is the flag (below)
//   3 block order       keys (block, level) over the sweep positions, one stable radix sort
//                       (rocprim), steps where the sorted key changes
//   4 entries           k_sched_codes: the operand codes in summation order
//   5 packet cutting    k_sched_walk: the greedy walk, one wave per block, a row's entries on
//                       the lanes; counted at EXT = 4, 2 (, 3) as the host does, then once more
//                       writing the descriptors and each operand's slot
//   6 layout + fill     exclusive scans over the blocks, streams at their exact sizes,
//                       k_sched_fill: one wave per packet
// Only a few words come back to the host: the check's flags and maxima, the
// level pass's flag and depth, the step count, the packet counts and the
// streams' lengths.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "internal.h"

namespace lssp_amd {

namespace {

// words of the control block (ints), zeroed by a hipMemsetAsync before every stage that uses them
enum { C_FLAGS = 0, C_BW, C_MAXLEN, C_TICKET, C_TIMEOUT, C_MAXLEV, C_WALKBAD, C_CAPX, C_WORDS = 16 };
constexpr uint64_t SCHED_WAIT_TICKS = 400000000ull;  // 4 s at 100 MHz (s_memrealtime)

__device__ __forceinline__ int ldi_agent(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sti_agent(int *p, int v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int wave_max(int v)
{
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_or(int v)
{
    for (int o = 32; o; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// ---- stage 1 ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sched_check(int n, int nnz, int upper, const int *__restrict__ Tp,
                                                     const int *__restrict__ Tj, const double *__restrict__ Tx,
                                                     int *__restrict__ ctl)
{
    int f = 0, bw = 0, len = 0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        int fi, bi, li;
        sched_check_row(n, nnz, upper != 0, Tp, Tj, Tx, (int)i, fi, bi, li);
        f |= fi;
        bw = max(bw, bi);
        len = max(len, li);
    }
    // one atomic of each kind per wave (Guideline 12)
    f = wave_or(f);
    bw = wave_max(bw);
    len = wave_max(len);
    if ((threadIdx.x & 63) == 0) {
        if (f) atomicOr(ctl + C_FLAGS, f);
        if (bw) atomicMax(ctl + C_BW, bw);
        if (len) atomicMax(ctl + C_MAXLEN, len);
    }
}

// ---- stage 2 ---------------------------------------------------------------------
// lev[i] = max(lev[j] + 1) over the strict entries, forward for L, backward for U.
// The rows in sweep order are cut into chunks of 64; a wave draws the next chunk,
// in ascending order, from an atomic ticket and takes one row per lane.  A drawn
// chunk therefore belongs to a running wave and every chunk below it has been
// drawn, so the smallest unfinished row belongs to a running wave and needs only
// finished rows: it always progresses, whatever the grid and whatever is resident
// (ilut_factor.hip's argument).  The level word is the flag (Guideline 16, R2): -1
// (the per-call hipMemsetAsync) until its row is finished, written and read by
// agent-scope relaxed atomic stores and loads, one aligned 4-byte word, no other
// payload.  The whole wave loops together until all its lanes are done, so a lane
// never spins against a lane of its own wave.  Every wait is bounded by
// s_memrealtime: an expired wait raises ctl[C_TIMEOUT], the wave's unfinished rows
// and every row reached from then on publish level 0 so that nobody waits for
// them, the kernel drains and the call answers LSSP_AMD_ETIMEOUT.
__global__ __launch_bounds__(256) void k_sched_levels(int n, int upper, const int *__restrict__ Tp,
                                                      const int *__restrict__ Tj, int *lev, int *ctl)
{
    const int lane = threadIdx.x & 63;
    const long nchunks = ((long)n + SCHED_LANES - 1) / SCHED_LANES;
    auto load = [](const int *p) { return ldi_agent(p); };
    int lmax = 0;
    for (;;) {
        int c = 0;
        if (lane == 0) c = atomicAdd(ctl + C_TICKET, 1);
        c = __builtin_amdgcn_readfirstlane(c);
        if (c >= nchunks || c < 0) break;
        const long q = (long)c * SCHED_LANES + lane;
        const bool valid = q < n;
        const int i = valid ? sched_q(n, upper != 0, (int)q) : 0;
        int k = 0, kend = 0, l = 0;
        if (valid) {
            k = sched_strict_begin(Tp, upper != 0, i);
            kend = sched_strict_end(Tp, upper != 0, i);
        }
        bool done = !valid;
        bool giveup = __builtin_amdgcn_readfirstlane(ldi_agent(ctl + C_TIMEOUT)) != 0;
        uint64_t t0 = 0;
        bool timing = false;
        int nap = 1;
        for (;;) {
            bool now = false;
            if (!done) {
                if (giveup) {
                    sti_agent(lev + i, 0);
                    done = true;
                } else if (sched_level_try(Tj, kend, lev, load, k, l)) {
                    sti_agent(lev + i, l);
                    lmax = max(lmax, l);
                    done = now = true;
                }
            }
            if (__all(done)) break;
            if (__any(now)) {  // progress: the rows of this wave that waited for those rows try again at once
                nap = 1;
                timing = false;
                continue;
            }
            if (!timing) {
                t0 = __builtin_amdgcn_s_memrealtime();
                timing = true;
            } else if (__builtin_amdgcn_s_memrealtime() - t0 > SCHED_WAIT_TICKS) {
                if (lane == 0) atomicOr(ctl + C_TIMEOUT, 1);
                giveup = true;
                continue;
            }
            for (int s = 0; s < nap; s++) __builtin_amdgcn_s_sleep(2);
            if (nap < 64) nap <<= 1;
            giveup = __builtin_amdgcn_readfirstlane(ldi_agent(ctl + C_TIMEOUT)) != 0;
        }
    }
    lmax = wave_max(lmax);
    if (lane == 0 && lmax) atomicMax(ctl + C_MAXLEV, lmax);
}

// ---- stage 3 ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sched_keys(int n, int upper, long B, const int *__restrict__ lev,
                                                    unsigned long long *__restrict__ keys, int *__restrict__ rows)
{
    for (long q = blockIdx.x * 256L + threadIdx.x; q < n; q += (long)gridDim.x * 256) {
        const int r = sched_q(n, upper != 0, (int)q);
        keys[q] = sched_key(q, B, lev[r]);
        rows[q] = r;
    }
}
__global__ __launch_bounds__(256) void k_sched_flags(int n, const unsigned long long *__restrict__ keys,
                                                     int *__restrict__ flag)
{
    for (long p = blockIdx.x * 256L + threadIdx.x; p < n; p += (long)gridDim.x * 256)
        flag[p] = p == 0 || keys[p] != keys[p - 1];
}
// sidx: the inclusive scan of the flags (step of position p = sidx[p] - 1)
__global__ __launch_bounds__(256) void k_sched_steps(int n, long B, int nb, int nsteps, const int *__restrict__ perm,
                                                     const int *__restrict__ sidx, int *__restrict__ pos,
                                                     int *__restrict__ step_pos, int *__restrict__ blk_step)
{
    for (long p = blockIdx.x * 256L + threadIdx.x; p < n; p += (long)gridDim.x * 256) {
        pos[perm[p]] = (int)p;
        const int s = sidx[p] - 1;
        if (p == 0 || sidx[p - 1] != sidx[p]) step_pos[s] = (int)p;
        if (p % B == 0) blk_step[p / B] = s;  // a block's first position opens a step
        if (p == 0) {
            step_pos[nsteps] = n;
            blk_step[nb] = nsteps;
        }
    }
}

// ---- stage 4 ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sched_lens(int n, int upper, const int *__restrict__ Tp,
                                                    const int *__restrict__ perm, int *__restrict__ lens)
{
    for (long p = blockIdx.x * 256L + threadIdx.x; p <= n; p += (long)gridDim.x * 256) {
        const int i = p < n ? perm[p] : 0;
        lens[p] = p < n ? sched_strict_end(Tp, upper != 0, i) - sched_strict_begin(Tp, upper != 0, i) : 0;
    }
}
__global__ __launch_bounds__(256) void k_sched_codes(int n, int upper, long B, const int *__restrict__ Tp,
                                                     const int *__restrict__ Tj, const int *__restrict__ perm,
                                                     const int *__restrict__ pos, const int *__restrict__ sidx,
                                                     const int *__restrict__ step_pos, const int *__restrict__ rp,
                                                     int *__restrict__ cols)
{
    for (long p = blockIdx.x * 256L + threadIdx.x; p < n; p += (long)gridDim.x * 256) {
        const int i = perm[p], b = (int)(p / B), send = step_pos[sidx[p]];
        const int k0 = rp[p], len = rp[p + 1] - k0;
        for (int e = 0; e < len; e++)
            cols[k0 + e] = sched_code(n, upper != 0, B, b, send, Tj[sched_entry(Tp, upper != 0, i, e)], pos);
    }
}

// ---- stage 5 ---------------------------------------------------------------------
struct WalkArgs {
    int n, upper, nb, EP, cap;
    long B;
    const int *rp, *step_pos, *blk_step;
    int *cols;          // the final walk replaces an HBM operand's code by its slot in its packet's list
    int *stamp, *slot;  // [nb][2 B] the walk's windows (sched_window)
    long *npk, *recw, *idxw;  // [nb + 1] counting walk: the block's packets, record words, index words;
                              // final walk: their exclusive scans
    unsigned long long *total;  // counting walk: the packets of all blocks
    int *ctl;
    int *desc, *pkxl, *xl, *blk;  // final walk: descriptors, each packet's place in xl, the operand lists, pk6_blk
};

// The greedy walk of build_packets6, sequential within a block: one wave per
// block, lane e holds entry e of the row under test.  FINAL: writes what the
// fill needs; else counts.  The window words of a block are written and read by
// this wave alone: a workgroup-scope fence orders a row's stores before the next
// row's loads.
template <bool FINAL>
__global__ __launch_bounds__(SCHED_LANES) void k_sched_walk(WalkArgs a)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1;
    const long sbase = 2 * a.B * b;
    int *stamp = a.stamp + sbase, *slot = a.slot + sbase;
    const long pk0 = FINAL ? a.npk[b] : 0, rec0 = FINAL ? a.recw[b] : 0, idx0 = FINAL ? a.idxw[b] : 0;
    const long pkend = FINAL ? a.npk[b + 1] : 0;
    const int xl0 = a.rp[min((long)b * a.B, (long)a.n)];
    int pid = 0;
    long npk = 0, recw = 0, idxw = 0, xo = 0;
    for (int s = a.blk_step[b]; s < a.blk_step[b + 1]; s++) {
        int p = a.step_pos[s];
        const int pend = a.step_pos[s + 1];
        while (p < pend) {
            int nr = 0, nx = 0, emax = 0;
            while (p + nr < pend && nr < PK3_ROWS) {
                const int r = p + nr;
                if (!sched_rec_fits(a.EP, nr)) break;  // LDS record slot
                const int k0 = a.rp[r], len = a.rp[r + 1] - k0;
                int g;
                long w;
                bool fresh, bad = len > PK6_MAXLEN;
                sched_walk_lane(a.n, a.upper != 0, a.B, b, a.cols, k0, len, lane, stamp, pid, g, w, fresh, bad);
                if (__any(bad)) {
                    if (lane == 0) atomicOr(a.ctl + C_WALKBAD, 1);
                    return;
                }
                const int newx = __popcll(__ballot(fresh));
                if (nx + newx > a.cap) break;
                // a column repeated inside the row: its first entry takes the slot
                int dup = -1;
                if (newx > 1)
                    for (int e = 0; e < len; e++) {
                        const int ge = __shfl(g, e), fe = __shfl((int)fresh, e);
                        if (lane > e && fresh && fe && ge == g && dup < 0) dup = e;
                    }
                const bool first = fresh && dup < 0;
                const unsigned long long bm = __ballot(first);
                int myslot = nx + __popcll(bm & below);
                if (!first && g >= 0 && !fresh) myslot = slot[w];  // taken by an earlier row of this packet
                const int ds = __shfl(myslot, dup < 0 ? lane : dup);
                if (dup >= 0) myslot = ds;
                if (first) {
                    stamp[w] = pid;
                    slot[w] = myslot;
                    if (FINAL) a.xl[xl0 + xo + myslot] = g;
                }
                if (FINAL && g >= 0) a.cols[k0 + lane] = myslot;
                __threadfence_block();
                nx += __popcll(bm);
                emax = max(emax, len);
                nr++;
            }
            if (nr == 0) {  // cannot happen (a row has at most 24 operands): never spin
                if (lane == 0) atomicOr(a.ctl + C_WALKBAD, 1);
                return;
            }
            if (FINAL && pk0 + npk >= pkend) {  // the counting walk saw fewer packets: cannot happen, never write past
                if (lane == 0) atomicOr(a.ctl + C_WALKBAD, 1);
                return;
            }
            if (FINAL && lane == 0) {
                reinterpret_cast<int4 *>(a.desc)[pk0 + npk] =
                    make_int4((int)((rec0 + recw) / 4), (int)(idx0 + idxw), nr | (nx << 10) | (emax << 21), p);
                a.pkxl[pk0 + npk] = (int)(xl0 + xo);
            }
            recw += sched_rec_words(a.EP, nr);
            idxw += nr + nx;
            xo += nx;
            npk++;
            p += nr;
            pid++;
        }
    }
    if (lane != 0) return;
    if (FINAL) {
        a.blk[b] = (int)pk0;
        if (b == a.nb - 1) a.blk[a.nb] = (int)(pk0 + npk);
    } else {
        a.npk[b] = npk;
        a.recw[b] = recw;
        a.idxw[b] = idxw;
        if (b == 0) a.npk[a.nb] = a.recw[a.nb] = a.idxw[a.nb] = 0;
        atomicAdd(a.total, (unsigned long long)npk);
        if (npk > PK3_CAP) atomicOr(a.ctl + C_CAPX, 1);
    }
}

// ---- stage 6 ---------------------------------------------------------------------
// one wave per packet: the records of its rows (16-byte stores: C for EP >= 8, the
// V pairs), the zero pads, the rows' rhs entries and the operand positions
__global__ __launch_bounds__(SCHED_LANES) void k_sched_fill(int npk, int upper, int EP, long B, int unit,
                                                            const int *__restrict__ Tp, const double *__restrict__ Tx,
                                                            const int *__restrict__ perm, const int *__restrict__ pos,
                                                            const int *__restrict__ rhs_pos, const int *__restrict__ rp,
                                                            const int *__restrict__ cols, const int *__restrict__ blk,
                                                            const int *__restrict__ desc, const int *__restrict__ pkxl,
                                                            const int *__restrict__ xl, uint32_t *__restrict__ rec,
                                                            int *__restrict__ idx)
{
    const int lane = threadIdx.x;
    for (long pk = blockIdx.x; pk < npk; pk += gridDim.x) {
        const int4 d = reinterpret_cast<const int4 *>(desc)[pk];
        const int nr = d.z & 1023, nx = (d.z >> 10) & 2047, p = d.w;
        const int par = (int)(pk - blk[p / B]) & 1;  // the packet's index in its block, mod 2
        uint32_t *w = rec + 4L * d.x;
        for (int r = lane; r < nr; r += SCHED_LANES) {
            const int i = perm[p + r], k0 = rp[p + r], len = rp[p + r + 1] - k0;
            sched_fill_row(w, EP, nr, r, par, cols, k0, len, Tp, Tx, upper != 0, i, unit != 0);
            idx[(long)d.y + r] = rhs_pos[i];
        }
        if (lane == 0) sched_fill_pads(w, EP, nr);
        const int xb = pkxl[pk];
        for (int x = lane; x < nx; x += SCHED_LANES) idx[(long)d.y + nr + x] = pos[xl[xb + x]];
    }
}

unsigned blocks_for(long long items) { return (unsigned)std::max<long long>(1, std::min<long long>((items + 255) / 256, 65536)); }

template <typename T>
int scan_excl(lssp_amd_ctx *c, DevBufs &bufs, const T *in, T *out, size_t cnt, bool inclusive = false)
{
    size_t bytes = 0;
    char *tmp = nullptr;
    if (inclusive) LSSP_HIP(rocprim::inclusive_scan(nullptr, bytes, in, out, cnt, rocprim::plus<T>(), c->stream));
    else LSSP_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, T(0), cnt, rocprim::plus<T>(), c->stream));
    LSSP_HIP(bufs.get(&tmp, bytes));
    if (inclusive) LSSP_HIP(rocprim::inclusive_scan(tmp, bytes, in, out, cnt, rocprim::plus<T>(), c->stream));
    else LSSP_HIP(rocprim::exclusive_scan(tmp, bytes, in, out, T(0), cnt, rocprim::plus<T>(), c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));  // the scratch is freed next
    bufs.drop(tmp);
    return LSSP_AMD_OK;
}

}  // namespace

int build_trisched_dev(lssp_amd_ctx *c, int n, int nnz, const int *dTp, const int *dTj, const double *dTx, bool upper,
                       const int *rhs_pos, TriSched &t, const std::function<int(const char *)> &mark0)
{
    if (n <= 0 || nnz < n || !dTp || !dTj || !dTx) return LSSP_AMD_EINVAL;
    const std::string side = upper ? "U " : "L ";
    auto mark = [&](const char *what) { return mark0((side + what).c_str()); };
    hipStream_t st = c->stream;
    DevBufs bufs;
    int *ctl = nullptr, h_ctl[C_WORDS];
    LSSP_HIP(bufs.get(&ctl, C_WORDS));
    auto read_ctl = [&]() -> int {
        LSSP_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, st));
        LSSP_HIP(hipStreamSynchronize(st));
        return LSSP_AMD_OK;
    };
    const int up = upper ? 1 : 0;

    // 1: check and scalars
    LSSP_HIP(hipMemsetAsync(ctl, 0, sizeof(h_ctl), st));
    k_sched_check<<<blocks_for(n), 256, 0, st>>>(n, nnz, up, dTp, dTj, dTx, ctl);
    LSSP_HIP(hipGetLastError());
    LSSP_TRY(read_ctl());
    if (h_ctl[C_FLAGS] & SCHED_BAD) return LSSP_AMD_EINVAL;
    if (h_ctl[C_MAXLEN] > PK6_MAXLEN) return LSSP_AMD_EUNSUPPORTED;  // ILUT(tol, p <= 24), ILU(k) of stencils
    const bool unit = !(h_ctl[C_FLAGS] & SCHED_NONUNIT);
    const int EP = sched_ep(h_ctl[C_MAXLEN]);
    long B = std::max(64L, (long)std::max(h_ctl[C_BW], 1));  // one bandwidth per block
    if (B > n) B = n;
    const int nb = (int)((n + B - 1) / B);
    const int nstrict = nnz - n;
    LSSP_TRY(mark("check"));

    // 2: levels
    int *lev = nullptr;
    LSSP_HIP(bufs.get(&lev, n));
    LSSP_HIP(hipMemsetAsync(lev, 0xFF, sizeof(int) * (size_t)n, st));  // -1: not written
    LSSP_HIP(hipMemsetAsync(ctl, 0, sizeof(h_ctl), st));
    {
        const long nchunks = ((long)n + SCHED_LANES - 1) / SCHED_LANES;
        const long grid = std::max(1L, std::min((nchunks + 3) / 4, 8L * std::max(c->num_cus, 1)));
        k_sched_levels<<<(unsigned)grid, 256, 0, st>>>(n, up, dTp, dTj, lev, ctl);
        LSSP_HIP(hipGetLastError());
    }
    LSSP_TRY(read_ctl());
    if (h_ctl[C_TIMEOUT]) return LSSP_AMD_ETIMEOUT;
    t.n = n;
    t.nlevels = h_ctl[C_MAXLEV] + 1;
    LSSP_TRY(mark("levels"));

    // 3: block order
    LSSP_HIP(hipMalloc(&t.bp_perm, sizeof(int) * (size_t)n));
    LSSP_HIP(hipMalloc(&t.bp_pos, sizeof(int) * (size_t)n));
    int *sidx = nullptr, *step_pos = nullptr, *blk_step = nullptr;
    LSSP_HIP(bufs.get(&sidx, (size_t)n + 1));
    int nsteps = 0;
    {
        unsigned long long *keys = nullptr, *skeys = nullptr;
        int *rows = nullptr, *flag = nullptr;
        char *tmp = nullptr;
        LSSP_HIP(bufs.get(&keys, n));
        LSSP_HIP(bufs.get(&skeys, n));
        LSSP_HIP(bufs.get(&rows, n));
        LSSP_HIP(bufs.get(&flag, n));
        k_sched_keys<<<blocks_for(n), 256, 0, st>>>(n, up, B, lev, keys, rows);
        LSSP_HIP(hipGetLastError());
        unsigned end_bit = 33;  // the level word and the bits of the block number
        while (end_bit < 64 && ((unsigned long long)(nb - 1) >> (end_bit - 32))) end_bit++;
        size_t bytes = 0;
        LSSP_HIP(rocprim::radix_sort_pairs(nullptr, bytes, keys, skeys, rows, t.bp_perm, (size_t)n, 0u, end_bit, st));
        LSSP_HIP(bufs.get(&tmp, bytes));
        LSSP_HIP(rocprim::radix_sort_pairs(tmp, bytes, keys, skeys, rows, t.bp_perm, (size_t)n, 0u, end_bit, st));
        k_sched_flags<<<blocks_for(n), 256, 0, st>>>(n, skeys, flag);
        LSSP_HIP(hipGetLastError());
        LSSP_TRY(scan_excl(c, bufs, flag, sidx, (size_t)n, true));
        LSSP_HIP(hipMemcpyAsync(&nsteps, sidx + n - 1, sizeof(int), hipMemcpyDeviceToHost, st));
        LSSP_HIP(hipStreamSynchronize(st));
        for (void *q : {(void *)keys, (void *)skeys, (void *)rows, (void *)flag, (void *)tmp}) bufs.drop(q);
    }
    bufs.drop(lev);
    if (nsteps < nb || nsteps > n) return LSSP_AMD_EHIP;  // (every block opens a step)
    LSSP_HIP(bufs.get(&step_pos, (size_t)nsteps + 1));
    LSSP_HIP(bufs.get(&blk_step, (size_t)nb + 1));
    k_sched_steps<<<blocks_for(n), 256, 0, st>>>(n, B, nb, nsteps, t.bp_perm, sidx, t.bp_pos, step_pos, blk_step);
    LSSP_HIP(hipGetLastError());
    LSSP_TRY(mark("order"));

    // 4: entries in summation order
    int *lens = nullptr, *rp = nullptr, *cols = nullptr;
    LSSP_HIP(bufs.get(&lens, (size_t)n + 1));
    LSSP_HIP(bufs.get(&rp, (size_t)n + 1));
    LSSP_HIP(bufs.get(&cols, nstrict));
    k_sched_lens<<<blocks_for((long long)n + 1), 256, 0, st>>>(n, up, dTp, t.bp_perm, lens);
    LSSP_HIP(hipGetLastError());
    LSSP_TRY(scan_excl(c, bufs, lens, rp, (size_t)n + 1));
    bufs.drop(lens);
    k_sched_codes<<<blocks_for(n), 256, 0, st>>>(n, up, B, dTp, dTj, t.bp_perm, t.bp_pos, sidx, step_pos, rp, cols);
    LSSP_HIP(hipGetLastError());
    LSSP_TRY(mark("entries"));

    // 5: packet cutting -- counted at EXT = 4, then 2 and 3: the smallest within 1 % of EXT = 4's count
    WalkArgs a{};
    a.n = n;
    a.upper = up;
    a.nb = nb;
    a.EP = EP;
    a.B = B;
    a.rp = rp;
    a.step_pos = step_pos;
    a.blk_step = blk_step;
    a.cols = cols;
    a.ctl = ctl;
    const size_t win = 2 * (size_t)B * (size_t)nb;
    LSSP_HIP(bufs.get(&a.stamp, win));
    LSSP_HIP(bufs.get(&a.slot, win));
    long *cntA = nullptr, *cntB = nullptr, *offs = nullptr;  // [3][nb + 1] each: packets, record words, index words
    unsigned long long *total = nullptr;
    const size_t nb1 = (size_t)nb + 1;
    LSSP_HIP(bufs.get(&cntA, 3 * nb1));
    LSSP_HIP(bufs.get(&cntB, 3 * nb1));
    LSSP_HIP(bufs.get(&offs, 3 * nb1));
    LSSP_HIP(bufs.get(&total, 2));
    auto count_at = [&](int cap, long *cnt, long &packets, bool &capx) -> int {
        a.cap = cap;
        a.npk = cnt;
        a.recw = cnt + nb1;
        a.idxw = cnt + 2 * nb1;
        a.total = total;
        LSSP_HIP(hipMemsetAsync(a.stamp, 0xFF, sizeof(int) * win, st));
        LSSP_HIP(hipMemsetAsync(total, 0, 16, st));
        LSSP_HIP(hipMemsetAsync(ctl, 0, sizeof(h_ctl), st));
        k_sched_walk<false><<<(unsigned)nb, SCHED_LANES, 0, st>>>(a);
        LSSP_HIP(hipGetLastError());
        unsigned long long h_total = 0;
        LSSP_HIP(hipMemcpyAsync(&h_total, total, sizeof(h_total), hipMemcpyDeviceToHost, st));
        LSSP_TRY(read_ctl());
        if (h_ctl[C_WALKBAD]) return LSSP_AMD_EINVAL;
        packets = (long)h_total;
        capx = h_ctl[C_CAPX] != 0;
        return LSSP_AMD_OK;
    };
    int ext = PK3_EXT;
    long *cnt = cntA;
    bool capx = false;
    {
        long c4 = 0, ce = 0;
        bool cx = false;
        LSSP_TRY(count_at(PK3_ROWS * PK3_EXT, cntA, c4, capx));
        for (int e = 2; e < PK3_EXT; e++) {
            LSSP_TRY(count_at(PK3_ROWS * e, cntB, ce, cx));
            if (ce <= c4 + c4 / 100) {
                ext = e;
                cnt = cntB;
                capx = cx;
                break;
            }
        }
    }
    if (capx) return LSSP_AMD_EUNSUPPORTED;  // more than PK3_CAP packets in a block
    LSSP_TRY(mark("packets"));

    // 6: layout and fill
    for (int k = 0; k < 3; k++) LSSP_TRY(scan_excl(c, bufs, cnt + k * nb1, offs + k * nb1, nb1));
    long h_tot[3];
    for (int k = 0; k < 3; k++)
        LSSP_HIP(hipMemcpyAsync(h_tot + k, offs + k * nb1 + nb, sizeof(long), hipMemcpyDeviceToHost, st));
    LSSP_HIP(hipStreamSynchronize(st));
    const long npk = h_tot[0], recw = h_tot[1], idxw = h_tot[2];
    if (npk > INT_MAX || recw / 4 > INT_MAX || idxw > INT_MAX) return LSSP_AMD_EUNSUPPORTED;
    const size_t ndesc = std::max<size_t>(4 * (size_t)npk, 1), nrec = (size_t)recw + 4, nidx = (size_t)idxw + 1;
    LSSP_HIP(hipMalloc(&t.pk6_blk, sizeof(int) * nb1));
    LSSP_HIP(hipMalloc(&t.pk6_desc, sizeof(int) * ndesc));
    LSSP_HIP(hipMalloc(&t.pk6_rec, sizeof(uint32_t) * nrec));
    LSSP_HIP(hipMalloc(&t.pk6_idx, sizeof(int) * nidx));
    LSSP_HIP(hipMalloc(&t.pk6_claim, sizeof(unsigned long long)));
    LSSP_HIP(hipMemsetAsync(t.pk6_claim, 0, sizeof(unsigned long long), st));
    LSSP_HIP(hipMemsetAsync(t.pk6_rec + recw, 0, 4 * sizeof(uint32_t), st));  // the kernels' whole-unit reads past the end
    LSSP_HIP(hipMemsetAsync(t.pk6_idx + idxw, 0, sizeof(int), st));
    LSSP_HIP(bufs.get(&a.pkxl, (size_t)npk));
    LSSP_HIP(bufs.get(&a.xl, nstrict));
    a.cap = PK3_ROWS * ext;
    a.npk = offs;
    a.recw = offs + nb1;
    a.idxw = offs + 2 * nb1;
    a.desc = t.pk6_desc;
    a.blk = t.pk6_blk;
    LSSP_HIP(hipMemsetAsync(a.stamp, 0xFF, sizeof(int) * win, st));
    LSSP_HIP(hipMemsetAsync(ctl, 0, sizeof(h_ctl), st));
    k_sched_walk<true><<<(unsigned)nb, SCHED_LANES, 0, st>>>(a);
    LSSP_HIP(hipGetLastError());
    k_sched_fill<<<(unsigned)std::max(1L, std::min(npk, 1L << 20)), SCHED_LANES, 0, st>>>(
        (int)npk, up, EP, B, unit ? 1 : 0, dTp, dTx, t.bp_perm, t.bp_pos, rhs_pos ? rhs_pos : t.bp_pos, rp, cols,
        t.pk6_blk, t.pk6_desc, a.pkxl, a.xl, t.pk6_rec, t.pk6_idx);
    LSSP_HIP(hipGetLastError());
    LSSP_TRY(read_ctl());
    if (h_ctl[C_WALKBAD]) return LSSP_AMD_EINVAL;
    t.upper = up;
    t.bp_B = (int)B;
    t.bp_nb = nb;
    t.bp_nsteps = nsteps;
    t.bp_unit = unit ? 1 : 0;
    t.bp_origin = 1;
    t.pk6_n = (int)npk;
    t.pk6_ep = EP;
    t.pk6_ext = ext;
    t.pk6_rows = PK3_ROWS;
    t.pk6_nrec = (long)nrec;
    t.pk6_nidx = (long)nidx;
    t.pk6_base = 0;
    LSSP_TRY(mark("fill"));
    return LSSP_AMD_OK;
}

// stage 2 on its own, for a factor whose rows the caller made itself (no check pass: every strict column
// must lie on its side of the diagonal inside [0, n)): lev[i] (device, n words) and the level count
int tri_levels_dev(lssp_amd_ctx *c, int n, const int *dTp, const int *dTj, bool upper, int *lev, int *nlevels)
{
    if (n <= 0 || !dTp || !dTj || !lev || !nlevels) return LSSP_AMD_EINVAL;
    hipStream_t st = c->stream;
    DevBufs bufs;
    int *ctl = nullptr, h_ctl[C_WORDS];
    LSSP_HIP(bufs.get(&ctl, C_WORDS));
    LSSP_HIP(hipMemsetAsync(lev, 0xFF, sizeof(int) * (size_t)n, st));  // -1: not written
    LSSP_HIP(hipMemsetAsync(ctl, 0, sizeof(h_ctl), st));
    const long nchunks = ((long)n + SCHED_LANES - 1) / SCHED_LANES;
    const long grid = std::max(1L, std::min((nchunks + 3) / 4, 8L * std::max(c->num_cus, 1)));
    k_sched_levels<<<(unsigned)grid, 256, 0, st>>>(n, upper ? 1 : 0, dTp, dTj, lev, ctl);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipMemcpyAsync(h_ctl, ctl, sizeof(h_ctl), hipMemcpyDeviceToHost, st));
    LSSP_HIP(hipStreamSynchronize(st));
    if (h_ctl[C_TIMEOUT]) return LSSP_AMD_ETIMEOUT;
    *nlevels = h_ctl[C_MAXLEV] + 1;
    return LSSP_AMD_OK;
}

}  // namespace lssp_amd
