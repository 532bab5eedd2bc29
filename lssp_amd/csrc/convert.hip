// convert.hip -- sparse format conversions on the device.
//
// lssp_mat_csr_to_coo / _coo_to_csr / _transpose / _csr_to_bcsr /
// _bcsr_to_csr (matrix-utils.cxx:62-380, :700-765) for matrices that already
// live in HBM.  All of it is integer / byte movement: no arithmetic on the
// values, so every result is bitwise the reference's, entry order included.
//
// The reference orders entries with counting sorts whose sequential loops
// make them STABLE (coo_to_csr keeps the input order inside a row, transpose
// the row order inside a column).  On the GPU the same orders come from
// stable LSD radix sorts (rocPRIM's device radix sort, keys limited to the bits
// the row / column range needs) of (key, entry index) pairs followed by a
// coalesced gather, and row pointers are lower bounds in the sorted keys.
// Block patterns (csr_to_bcsr) come from one radix sort of packed
// (block row, block column) 64-bit keys and a flag / scan / scatter unique.
// Work where ONE row's entries are written in the reference's sequential
// order (duplicate (r, c) in csr_to_bcsr: last value wins; bcsr_to_csr rows
// in block order) is done by one thread per row, so the order is the same
// by construction.  These kernels are HBM-bound streaming passes; none of
// them is on the solve path.
//
// Assembly (second half of the file): lssp_mat_csr_is_sorted /
// _bcsr_is_sorted / _sort_column / _adjust_zero_diag / _get_block_diag
// (matrix-utils.cxx:217-279, :387-698) on device arrays, and
// lssp_amd_mat_from_device, which builds the handle lssp_amd_mat_upload
// (capi.cpp) builds, offset-id coding included, from a CSR in HBM.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "internal.h"

namespace {

constexpr int CT = 256;  // threads per block (4 waves)

unsigned grid_for(long n)
{
    long b = (n + CT - 1) / CT;
    return (unsigned)std::max<long>(1, std::min<long>(b, 16384));
}

#define GRID_STRIDE(i, n) for (long i = blockIdx.x * (long)CT + threadIdx.x; i < (n); i += (long)gridDim.x * CT)

int bits_for(unsigned long v)  // bits needed to hold every value in [0, v]
{
    int b = 1;
    while (b < 64 && (v >> b) != 0) b++;
    return b;
}

// Ap[0] == 0, non-decreasing, Ap[nrows] == nnz: afterwards every per-row loop
// stays inside [0, nnz)
__global__ __launch_bounds__(CT) void k_check_ptr(long nrows, int nnz, const int *__restrict__ Ap,
                                                  int *__restrict__ err)
{
    GRID_STRIDE(i, nrows + 1)
    {
        int a = Ap[i];
        bool bad = (i == 0 && a != 0) || (i == nrows && a != nnz) || (i < nrows && Ap[i + 1] < a);
        if (bad) atomicOr(err, 1);
    }
}

__global__ __launch_bounds__(CT) void k_check_idx(long n, const int *__restrict__ v, int lim,
                                                  int *__restrict__ err)
{
    GRID_STRIDE(i, n)
    {
        if ((unsigned)v[i] >= (unsigned)lim) atomicOr(err, 1);
    }
}

// matrix-utils.cxx:287-294: the row of every entry
__global__ __launch_bounds__(CT) void k_expand_rows(long nrows, const int *__restrict__ Ap,
                                                    int *__restrict__ Ci)
{
    GRID_STRIDE(i, nrows)
    {
        int e = Ap[i + 1];
        for (int k = Ap[i]; k < e; k++) Ci[k] = (int)i;
    }
}

__global__ __launch_bounds__(CT) void k_iota(long n, int *__restrict__ v)
{
    GRID_STRIDE(i, n) v[i] = (int)i;
}

// P[r] = first position whose key is >= r, r = 0..nr: the row pointers of
// entries sorted by row (empty rows included)
__global__ __launch_bounds__(CT) void k_row_ptr(long nr, const unsigned *__restrict__ key, int nkeys,
                                                int *__restrict__ P)
{
    GRID_STRIDE(r, nr + 1)
    {
        int lo = 0, hi = nkeys;
        while (lo < hi) {
            int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            if (key[mid] < (unsigned long)r)
                lo = mid + 1;
            else
                hi = mid;
        }
        P[r] = lo;
    }
}

__global__ __launch_bounds__(CT) void k_gather(long n, const int *__restrict__ perm, const int *__restrict__ sj,
                                               const double *__restrict__ sx, int *__restrict__ dj,
                                               double *__restrict__ dx)
{
    GRID_STRIDE(i, n)
    {
        int k = perm[i];
        dj[i] = sj[k];
        dx[i] = sx[k];
    }
}

// csr_to_bcsr: (block row << cbits) | block column of every entry
__global__ __launch_bounds__(CT) void k_block_keys(long n, int bs, int cbits, const int *__restrict__ Ap,
                                                   const int *__restrict__ Aj, uint64_t *__restrict__ key)
{
    GRID_STRIDE(i, n)
    {
        uint64_t hi = (uint64_t)(i / bs) << cbits;
        int e = Ap[i + 1];
        for (int k = Ap[i]; k < e; k++) key[k] = hi | (uint64_t)(unsigned)(Aj[k] / bs);
    }
}

__global__ __launch_bounds__(CT) void k_unique_flag(long n, const uint64_t *__restrict__ key, int *__restrict__ flag)
{
    GRID_STRIDE(i, n) flag[i] = (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(CT) void k_unique_put(long n, const uint64_t *__restrict__ key,
                                                   const int *__restrict__ flag, const int *__restrict__ pos,
                                                   int cbits, int *__restrict__ Bj, unsigned *__restrict__ brow)
{
    GRID_STRIDE(i, n)
    {
        if (flag[i]) {
            uint64_t k = key[i];
            Bj[pos[i]] = (int)(k & ((1ull << cbits) - 1));
            brow[pos[i]] = (unsigned)(k >> cbits);
        }
    }
}

// matrix-utils.cxx:125-156: one thread per CSR row writes its entries in
// order into the zeroed column-major blocks, so a duplicate keeps its last value
__global__ __launch_bounds__(CT) void k_bcsr_fill(long n, int bs, const int *__restrict__ Ap,
                                                  const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                  const int *__restrict__ Bp, const int *__restrict__ Bj,
                                                  double *__restrict__ Bx)
{
    GRID_STRIDE(i, n)
    {
        int ib = (int)(i / bs), ro = (int)(i % bs);
        int b0 = Bp[ib], b1 = Bp[ib + 1];
        int e = Ap[i + 1];
        for (int k = Ap[i]; k < e; k++) {
            int c = Aj[k], bc = c / bs;
            int lo = b0, hi = b1 - 1;  // bc is in the block row's pattern by construction
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                if (Bj[mid] < bc)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            Bx[(long)lo * bs * bs + (long)(c % bs) * bs + ro] = Ax[k];
        }
    }
}

// bcsr_to_csr (matrix-utils.cxx:185-203): entries of output row i with
// fabs(v) > 0, in block order then block-column offset
__global__ __launch_bounds__(CT) void k_bcsr_count(long n, int bs, const int *__restrict__ Bp,
                                                   const double *__restrict__ Bx, int *__restrict__ cnt)
{
    GRID_STRIDE(i, n)
    {
        int ib = (int)(i / bs), ro = (int)(i % bs), c = 0;
        for (int t = Bp[ib]; t < Bp[ib + 1]; t++) {
            const double *b = Bx + (long)t * bs * bs + ro;
            for (int co = 0; co < bs; co++) c += fabs(b[(long)co * bs]) > 0. ? 1 : 0;
        }
        cnt[i] = c;
    }
}

// lssp_mat_sort_column's rule (matrix-utils.cxx:448-471) for ONE row [s, o)
// that has an inversion: sorted by column, and every occurrence of a column
// takes the value stored last for it (the dense row[] buffer there); a stable
// insertion sort keeps equal columns in their original order, so that value
// is the last of each run.  One thread; rows of up to SORT_THREAD_MAX entries
// in lssp_amd_csr_sort_columns_dev
__device__ __forceinline__ void sort_row_last_wins(int *__restrict__ Aj, double *__restrict__ Ax, int s, int o)
{
    for (int a = s + 1; a < o; a++) {
        int c = Aj[a];
        double v = Ax[a];
        int b = a - 1;
        while (b >= s && Aj[b] > c) {
            Aj[b + 1] = Aj[b];
            Ax[b + 1] = Ax[b];
            b--;
        }
        Aj[b + 1] = c;
        Ax[b + 1] = v;
    }
    for (int a = o - 1; a > s; a--)
        if (Aj[a - 1] == Aj[a]) Ax[a - 1] = Ax[a];
}

// fill row i, then lssp_mat_sort_column (matrix-utils.cxx:434-471) on it
__global__ __launch_bounds__(CT) void k_bcsr_rows(long n, int bs, const int *__restrict__ Bp,
                                                  const int *__restrict__ Bj, const double *__restrict__ Bx,
                                                  const int *__restrict__ Ap, int *__restrict__ Aj,
                                                  double *__restrict__ Ax)
{
    GRID_STRIDE(i, n)
    {
        int ib = (int)(i / bs), ro = (int)(i % bs);
        int o = Ap[i], s = o;
        bool sorted = true;
        for (int t = Bp[ib]; t < Bp[ib + 1]; t++) {
            const double *b = Bx + (long)t * bs * bs + ro;
            int c0 = Bj[t] * bs;
            for (int co = 0; co < bs; co++) {
                double v = b[(long)co * bs];
                if (fabs(v) > 0.) {
                    if (o > s && Aj[o - 1] > c0 + co) sorted = false;
                    Aj[o] = c0 + co;
                    Ax[o] = v;
                    o++;
                }
            }
        }
        if (!sorted) sort_row_last_wins(Aj, Ax, s, o);
    }
}

// ---- the rest of matrix-utils.h on device arrays (assembly) ------------------

// first index in v[0, n) whose value is > t (v non-decreasing)
__device__ __forceinline__ int upper_bound(const int *__restrict__ v, int n, int t)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (v[mid] <= t)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// matrix-utils.cxx:217-279: one thread per entry; a descending neighbour
// pair counts when both entries lie in one row, i.e. k is no row start (a
// binary search in Ap, run for descending pairs only, until one is found)
__global__ __launch_bounds__(CT) void k_is_sorted(long nnz, int nrows, const int *__restrict__ Ap,
                                                  const int *__restrict__ Aj, int *__restrict__ uns)
{
    GRID_STRIDE(k, nnz)
    {
        if (k == 0 || Aj[k - 1] <= Aj[k]) continue;
        if (*(volatile int *)uns) continue;
        int r = upper_bound(Ap, nrows + 1, (int)k - 1);  // first row pointer >= k
        if (r > nrows || Ap[r] != (int)k) atomicOr(uns, 1);
    }
}

constexpr int SORT_THREAD_MAX = 64;  // longest row one thread checks / sorts by insertion

// the same test, one thread per row of up to SORT_THREAD_MAX entries (a
// stencil matrix descends at every row boundary, which would send each row
// of k_is_sorted into its binary search); flag[0]: unsorted, flag[1]: a
// longer row exists, and k_is_sorted then runs over all entries
__global__ __launch_bounds__(CT) void k_is_sorted_rows(long nrows, const int *__restrict__ Ap,
                                                       const int *__restrict__ Aj, int *__restrict__ flag)
{
    GRID_STRIDE(i, nrows)
    {
        int s = Ap[i], e = Ap[i + 1];
        if (e - s > SORT_THREAD_MAX) {
            if (!*(volatile int *)(flag + 1)) atomicOr(flag + 1, 1);
            continue;
        }
        bool sorted = true;
        for (int a = s + 1; a < e && sorted; a++) sorted = Aj[a - 1] <= Aj[a];
        if (!sorted && !*(volatile int *)flag) atomicOr(flag, 1);
    }
}

// lssp_mat_sort_column, rows of up to SORT_THREAD_MAX entries: checked and
// sorted in place by their thread; longer rows are left as candidates
// (cand[i] = length, else 0) for the per-entry passes below
__global__ __launch_bounds__(CT) void k_sort_short(long nrows, const int *__restrict__ Ap, int *__restrict__ Aj,
                                                   double *__restrict__ Ax, int *__restrict__ cand)
{
    GRID_STRIDE(i, nrows)
    {
        int s = Ap[i], e = Ap[i + 1];
        if (e - s > SORT_THREAD_MAX) {
            cand[i] = e - s;
            continue;
        }
        cand[i] = 0;
        bool sorted = true;
        for (int a = s + 1; a < e && sorted; a++) sorted = Aj[a - 1] <= Aj[a];
        if (!sorted) sort_row_last_wins(Aj, Ax, s, e);
    }
}

// entry t of the candidate rows laid end to end (off = exclusive sum of their
// lengths, 0 for the other rows): its row, the last with off[row] <= t
__device__ __forceinline__ int packed_row(const int *__restrict__ off, int nrows, int t)
{
    return upper_bound(off, nrows + 1, t) - 1;
}

// which candidate rows hold a descending pair, one thread per entry
__global__ __launch_bounds__(CT) void k_long_check(long total, int nrows, const int *__restrict__ off,
                                                   const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                   int *__restrict__ uns)
{
    GRID_STRIDE(t, total)
    {
        int r = packed_row(off, nrows, (int)t);
        int k = Ap[r] + ((int)t - off[r]);
        if (k > Ap[r] && Aj[k - 1] > Aj[k]) uns[r] = 1;
    }
}

// ... and the lengths of those alone (in place; cand[nrows] stays 0)
__global__ __launch_bounds__(CT) void k_long_len(long nrows, const int *__restrict__ uns, int *__restrict__ cand)
{
    GRID_STRIDE(i, nrows)
    {
        if (!uns[i]) cand[i] = 0;
    }
}

// the unsorted long rows' entries as (row << cbits | column) keys with their
// values, laid end to end
__global__ __launch_bounds__(CT) void k_long_keys(long total, int nrows, int cbits, const int *__restrict__ off,
                                                  const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                  const double *__restrict__ Ax, uint64_t *__restrict__ key,
                                                  int *__restrict__ idx, double *__restrict__ vx)
{
    GRID_STRIDE(t, total)
    {
        int r = packed_row(off, nrows, (int)t);
        int k = Ap[r] + ((int)t - off[r]);
        key[t] = ((uint64_t)(unsigned)r << cbits) | (uint64_t)(unsigned)Aj[k];
        idx[t] = (int)t;
        vx[t] = Ax[k];
    }
}

// ... back into their rows after the stable sort: position t of the sorted
// keys is entry t - off[row] of its row; equal keys kept their input order,
// so the value stored last for a column is the last of its run
__global__ __launch_bounds__(CT) void k_long_put(long total, int cbits, const uint64_t *__restrict__ key,
                                                 const int *__restrict__ idx, const double *__restrict__ vx,
                                                 const int *__restrict__ off, const int *__restrict__ Ap,
                                                 int *__restrict__ Aj, double *__restrict__ Ax)
{
    GRID_STRIDE(t, total)
    {
        uint64_t k = key[t];
        long lo = t, hi = total;  // last position of k's run: the one before the first key > k
        while (hi - lo > 1) {
            long mid = (lo + hi) >> 1;
            if (key[mid] == k)
                lo = mid;
            else
                hi = mid;
        }
        int r = (int)(k >> cbits);
        int d = Ap[r] + ((int)t - off[r]);
        Aj[d] = (int)(k & ((1ull << cbits) - 1));
        Ax[d] = vx[idx[lo]];
    }
}

// matrix-utils.cxx:498-532: entries of output row i (one more without a diagonal)
__global__ __launch_bounds__(CT) void k_azd_count(long n, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                  int *__restrict__ cnt)
{
    GRID_STRIDE(i, n)
    {
        int s = Ap[i], e = Ap[i + 1];
        bool has = false;
        for (int k = s; k < e; k++) has |= Aj[k] == (int)i;
        cnt[i] = e - s + (has ? 0 : 1);
    }
}

// matrix-utils.cxx:542-582: the row copied in order; (i, 1 * tol), appended
// to a row without a diagonal, then moves left past the trailing entries whose
// column is greater and stops at the first that is not
__global__ __launch_bounds__(CT) void k_azd_fill(long n, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                 const double *__restrict__ Ax, double tol,
                                                 const int *__restrict__ Mp, int *__restrict__ Mj,
                                                 double *__restrict__ Mx)
{
    GRID_STRIDE(i, n)
    {
        int s = Ap[i], len = Ap[i + 1] - s, o = Mp[i];
        int p = len;  // where the new entry goes (len: all of the row stays before it)
        if (Mp[i + 1] - o == len)
            p = -1;  // has its diagonal
        else
            while (p > 0 && Aj[s + p - 1] > (int)i) p--;
        for (int k = 0; k < len; k++) {
            int d = o + k + ((p >= 0 && k >= p) ? 1 : 0);
            Mj[d] = Aj[s + k];
            Mx[d] = Ax[s + k];
        }
        if (p >= 0) {
            Mj[o + p] = (int)i;
            Mx[o + p] = 1 * tol;
        }
    }
}

// matrix-utils.cxx:615-647: row i keeps the columns of its own diagonal block
// [start, end); a row left with none gets one entry
__device__ __forceinline__ void block_range(long i, int n, int blk, int &start, int &end)
{
    long s = i / blk * (long)blk;
    start = (int)s;
    end = s + blk < n ? (int)(s + blk) : n;
}

__global__ __launch_bounds__(CT) void k_bd_count(long n, int blk, const int *__restrict__ Ap,
                                                 const int *__restrict__ Aj, int *__restrict__ cnt)
{
    GRID_STRIDE(i, n)
    {
        int start, end, c = 0;
        block_range(i, (int)n, blk, start, end);
        for (int k = Ap[i]; k < Ap[i + 1]; k++) c += (Aj[k] >= start && Aj[k] < end) ? 1 : 0;
        cnt[i] = c ? c : 1;
    }
}

// matrix-utils.cxx:659-687
__global__ __launch_bounds__(CT) void k_bd_fill(long n, int blk, const int *__restrict__ Ap,
                                                const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                const int *__restrict__ Mp, int *__restrict__ Mj,
                                                double *__restrict__ Mx)
{
    GRID_STRIDE(i, n)
    {
        int start, end, o = Mp[i];
        block_range(i, (int)n, blk, start, end);
        for (int k = Ap[i]; k < Ap[i + 1]; k++)
            if (Aj[k] >= start && Aj[k] < end) {
                Mj[o] = Aj[k];
                Mx[o] = Ax[k];
                o++;
            }
        if (o == Mp[i]) {
            Mj[o] = (int)i;
            Mx[o] = 1;
        }
    }
}

// ---- the SpMV's offset-id coding built on the device (build_diag_ids, capi.cpp) --
using lssp_amd::DIAG_HS;
using lssp_amd::DIAG_MAX;
constexpr int OFF_EMPTY = INT32_MIN;  // no col - row: columns are >= 0 and rows < INT32_MAX
// the device-wide set: DIAG_HS hash slots, the number of distinct offsets
// seen, the overflow flag (a 256th distinct offset), the offsets in arrival order
constexpr int G_COUNT = DIAG_HS, G_OVER = DIAG_HS + 1, G_LIST = DIAG_HS + 2, G_SIZE = G_LIST + DIAG_MAX;

__device__ __forceinline__ unsigned off_slot(int k) { return ((unsigned)k * 2654435761u) >> 22; }  // 10 bits

__global__ __launch_bounds__(CT) void k_off_init(int *__restrict__ g)
{
    for (int t = threadIdx.x; t < G_SIZE; t += CT) g[t] = t < DIAG_HS ? OFF_EMPTY : 0;
}

// k into the open-addressing set tab; true when this call claimed its slot.
// A slot is READ first, so a key already present costs no atomic (a stencil's
// 7 offsets are there after the first rows).  Slots only ever fill, and every
// inserter of k walks the same probe sequence, so k lands in one slot only.
// *full (more than DIAG_MAX claims) stops further claims: the set never fills up
__device__ __forceinline__ bool off_insert(int *tab, const int *full, int k)
{
    unsigned h = off_slot(k);
    for (int p = 0; p < DIAG_HS; p++, h = (h + 1) & (DIAG_HS - 1)) {
        int cur = *(volatile int *)(tab + h);
        if (cur == k) return false;
        if (cur != OFF_EMPTY) continue;
        if (*(volatile const int *)full > DIAG_MAX) return false;
        int old = atomicCAS(tab + h, OFF_EMPTY, k);
        if (old == OFF_EMPTY) return true;
        if (old == k) return false;
    }
    return false;
}

// distinct col - row of all entries: each block collects its own in an LDS
// set (70 M entries hit 7 keys: LDS reads, no global traffic), then merges
// that set into the device-wide one
__global__ __launch_bounds__(CT) void k_off_collect(long nrows, const int *__restrict__ Ap,
                                                    const int *__restrict__ Aj, int *__restrict__ g)
{
    __shared__ int tab[DIAG_HS];
    __shared__ int cnt;
    for (int t = threadIdx.x; t < DIAG_HS; t += CT) tab[t] = OFF_EMPTY;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    GRID_STRIDE(i, nrows)
    {
        if (*(volatile int *)&cnt > DIAG_MAX || *(volatile int *)(g + G_OVER)) break;
        int e = Ap[i + 1];
        for (int k = Ap[i]; k < e; k++)
            if (off_insert(tab, &cnt, Aj[k] - (int)i)) atomicAdd(&cnt, 1);
    }
    __syncthreads();
    if (cnt > DIAG_MAX) {
        if (threadIdx.x == 0) atomicOr(g + G_OVER, 1);
        return;
    }
    for (int t = threadIdx.x; t < DIAG_HS; t += CT) {
        int k = tab[t];
        if (k == OFF_EMPTY || !off_insert(g, g + G_COUNT, k)) continue;
        int at = atomicAdd(g + G_COUNT, 1);
        if (at < DIAG_MAX)
            g[G_LIST + at] = k;
        else
            atomicOr(g + G_OVER, 1);
    }
}

// Ad[k] = index of col - row in the ascending table off[0, nd)
__global__ __launch_bounds__(CT) void k_off_ids(long nrows, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                const int *__restrict__ off, int nd, uint8_t *__restrict__ Ad)
{
    __shared__ int tab[DIAG_MAX + 1];
    for (int t = threadIdx.x; t < nd; t += CT) tab[t] = off[t];
    __syncthreads();
    GRID_STRIDE(i, nrows)
    {
        int e = Ap[i + 1];
        for (int k = Ap[i]; k < e; k++) {
            int o = Aj[k] - (int)i, lo = 0, hi = nd - 1;  // o is in the table by construction
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                if (tab[mid] < o)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            Ad[k] = (uint8_t)lo;
        }
    }
}

// ---- the SpMV's row coding (lssp_amd_mat::Ac), from the resident Ap and Ad ----
using lssp_amd::ROWPAT_LEN;
using lssp_amd::ROWPAT_MAX;
typedef unsigned long long pat_t;
constexpr pat_t PAT_EMPTY = ~0ull;  // eight entries of id 254: such a row leaves the matrix uncoded
constexpr int PAT_HS = 1024;        // hash slots of the pattern sets
// the device-wide set's counters: distinct patterns seen, the flag of a matrix
// that cannot be coded; its keys: PAT_HS hash slots, then the patterns in arrival order
constexpr int P_COUNT = 0, P_OVER = 1;

__device__ __forceinline__ unsigned pat_slot(pat_t k) { return (unsigned)((k * 0x9E3779B97F4A7C15ull) >> 54); }  // 10 bits

__global__ __launch_bounds__(CT) void k_pat_init(pat_t *__restrict__ gk, int *__restrict__ gi)
{
    for (int t = threadIdx.x; t < PAT_HS + ROWPAT_MAX; t += CT) gk[t] = t < PAT_HS ? PAT_EMPTY : 0;
    if (threadIdx.x < 2) gi[threadIdx.x] = 0;
}

// off_insert for 64-bit pattern keys; *full counts the claims, more than
// ROWPAT_MAX of them stop further claims
__device__ __forceinline__ bool pat_insert(pat_t *tab, const int *full, pat_t k)
{
    unsigned h = pat_slot(k);
    for (int p = 0; p < PAT_HS; p++, h = (h + 1) & (PAT_HS - 1)) {
        pat_t cur = *(volatile pat_t *)(tab + h);
        if (cur == k) return false;
        if (cur != PAT_EMPTY) continue;
        if (*(volatile const int *)full > ROWPAT_MAX) return false;
        pat_t old = atomicCAS(tab + h, PAT_EMPTY, k);
        if (old == PAT_EMPTY) return true;
        if (old == k) return false;
    }
    return false;
}

// a row's pattern key: byte k = Ad of its entry k, plus 1
__device__ __forceinline__ pat_t pat_key(const uint8_t *__restrict__ Ad, int b, int e)
{
    pat_t key = 0;
    for (int k = b; k < e; k++) key |= (pat_t)(Ad[k] + 1u) << (8 * (k - b));
    return key;
}

// distinct row patterns, collected as k_off_collect collects offsets (10 M
// rows hit 27 keys); a row of more than ROWPAT_LEN entries raises P_OVER
__global__ __launch_bounds__(CT) void k_pat_collect(long nrows, const int *__restrict__ Ap,
                                                    const uint8_t *__restrict__ Ad, pat_t *__restrict__ gk,
                                                    int *__restrict__ gi)
{
    __shared__ pat_t tab[PAT_HS];
    __shared__ int cnt;
    for (int t = threadIdx.x; t < PAT_HS; t += CT) tab[t] = PAT_EMPTY;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    GRID_STRIDE(i, nrows)
    {
        if (*(volatile int *)&cnt > ROWPAT_MAX || *(volatile int *)(gi + P_OVER)) break;
        const int b = Ap[i], e = Ap[i + 1];
        const pat_t key = e - b <= ROWPAT_LEN ? pat_key(Ad, b, e) : PAT_EMPTY;
        if (key == PAT_EMPTY) {
            atomicOr(gi + P_OVER, 1);
            break;
        }
        if (pat_insert(tab, &cnt, key)) atomicAdd(&cnt, 1);
    }
    __syncthreads();
    if (cnt > ROWPAT_MAX) {
        if (threadIdx.x == 0) atomicOr(gi + P_OVER, 1);
        return;
    }
    for (int t = threadIdx.x; t < PAT_HS; t += CT) {
        pat_t k = tab[t];
        if (k == PAT_EMPTY || !pat_insert(gk, gi + P_COUNT, k)) continue;
        int at = atomicAdd(gi + P_COUNT, 1);
        if (at < ROWPAT_MAX)
            gk[PAT_HS + at] = k;
        else
            atomicOr(gi + P_OVER, 1);
    }
}

// Ac[i] = index of row i's key in the ascending table pat[0, np)
__global__ __launch_bounds__(CT) void k_pat_codes(long nrows, const int *__restrict__ Ap,
                                                  const uint8_t *__restrict__ Ad, const pat_t *__restrict__ pat,
                                                  int np, uint8_t *__restrict__ Ac)
{
    __shared__ pat_t tab[ROWPAT_MAX];
    for (int t = threadIdx.x; t < np; t += CT) tab[t] = pat[t];
    __syncthreads();
    GRID_STRIDE(i, nrows)
    {
        const pat_t key = pat_key(Ad, Ap[i], Ap[i + 1]);  // in the table by construction
        int lo = 0, hi = np - 1;
        while (lo < hi) {
            int mid = (lo + hi) >> 1;
            if (tab[mid] < key)
                lo = mid + 1;
            else
                hi = mid;
        }
        Ac[i] = (uint8_t)lo;
    }
}

// ---- the SpMV's value coding (lssp_amd_mat::Av), from the resident Ap, Ac and Ax ----
// A row's key is its pattern and the bit patterns of its values in CSR order:
// nine 64-bit words, the pattern key (d_pat[Ac[i]]: ascending with the code)
// and eight values (+0.0 past the row's length, which the pattern fixes).  The
// rows are collected by a 64-bit mix of the key in the pattern sets above, each
// distinct mix with one row that produced it; the table is then those rows'
// keys, and k_val_codes compares every row with the table in full, so two keys
// that share a mix leave the matrix uncoded instead of miscoded.
using lssp_amd::ROWVAL_MAX;
static_assert(ROWVAL_MAX == ROWPAT_MAX, "the value sets are the pattern sets (pat_insert's bound)");
constexpr int VAL_WORDS = 1 + ROWPAT_LEN;

__device__ __forceinline__ pat_t val_mix(pat_t h, pat_t v)
{
    h = (h ^ v) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 32);
}

__device__ __forceinline__ pat_t val_hash(unsigned code, const double *__restrict__ Ax, int b, int e)
{
    pat_t h = val_mix(0x243F6A8885A308D3ull, code);
    for (int k = b; k < e; k++) h = val_mix(h, (pat_t)__double_as_longlong(Ax[k]));
    return h == PAT_EMPTY ? h - 1 : h;
}

// pat_insert that reports the slot it claimed (-1: the key was there, or the set is full)
__device__ __forceinline__ int pat_claim(pat_t *tab, const int *full, pat_t k)
{
    unsigned h = pat_slot(k);
    for (int p = 0; p < PAT_HS; p++, h = (h + 1) & (PAT_HS - 1)) {
        pat_t cur = *(volatile pat_t *)(tab + h);
        if (cur == k) return -1;
        if (cur != PAT_EMPTY) continue;
        if (*(volatile const int *)full > ROWVAL_MAX) return -1;
        pat_t old = atomicCAS(tab + h, PAT_EMPTY, k);
        if (old == PAT_EMPTY) return (int)h;
        if (old == k) return -1;
    }
    return -1;
}

// distinct value rows, as k_pat_collect collects patterns: rep[at] = one row of
// the at-th distinct mix.  More than ROWVAL_MAX of them raise P_OVER, and every
// workgroup stops at its next row (a matrix of varying coefficients pays a
// fraction of one pass)
__global__ __launch_bounds__(CT) void k_val_collect(long nrows, const int *__restrict__ Ap,
                                                    const uint8_t *__restrict__ Ac, const double *__restrict__ Ax,
                                                    pat_t *__restrict__ gk, int *__restrict__ gi,
                                                    int *__restrict__ rep)
{
    __shared__ pat_t tab[PAT_HS];
    __shared__ int trow[PAT_HS];
    __shared__ int cnt;
    for (int t = threadIdx.x; t < PAT_HS; t += CT) tab[t] = PAT_EMPTY;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    GRID_STRIDE(i, nrows)
    {
        if (*(volatile int *)&cnt > ROWVAL_MAX || *(volatile int *)(gi + P_OVER)) break;
        const int at = pat_claim(tab, &cnt, val_hash(Ac[i], Ax, Ap[i], Ap[i + 1]));
        if (at >= 0) {
            trow[at] = (int)i;
            atomicAdd(&cnt, 1);
        }
    }
    __syncthreads();
    if (cnt > ROWVAL_MAX) {
        if (threadIdx.x == 0) atomicOr(gi + P_OVER, 1);
        return;
    }
    for (int t = threadIdx.x; t < PAT_HS; t += CT) {
        pat_t k = tab[t];
        if (k == PAT_EMPTY || !pat_insert(gk, gi + P_COUNT, k)) continue;
        int at = atomicAdd(gi + P_COUNT, 1);
        if (at < ROWVAL_MAX)
            rep[at] = trow[t];
        else
            atomicOr(gi + P_OVER, 1);
    }
}

// row i's key, word q
__device__ __forceinline__ pat_t val_word(int q, pat_t pt, const double *__restrict__ Ax, int b, int len)
{
    if (q == 0) return pt;
    return q - 1 < len ? (pat_t)__double_as_longlong(Ax[b + q - 1]) : 0;
}

// out[VAL_WORDS * t + q] = word q of row rep[t]'s key
__global__ __launch_bounds__(CT) void k_val_gather(int nrep, const int *__restrict__ rep, const int *__restrict__ Ap,
                                                   const uint8_t *__restrict__ Ac, const double *__restrict__ Ax,
                                                   const pat_t *__restrict__ pat, pat_t *__restrict__ out)
{
    const int t = threadIdx.x;
    if (t >= nrep) return;
    const int i = rep[t], b = Ap[i], len = Ap[i + 1] - b;
    for (int q = 0; q < VAL_WORDS; q++) out[VAL_WORDS * t + q] = val_word(q, pat[Ac[i]], Ax, b, len);
}

// Av[i] = index of row i's key in the ascending table val (word q of entry c
// at val[q * nv + c]), found by bisection and then compared word for word: a
// row that is not in the table raises *bad
__global__ __launch_bounds__(CT) void k_val_codes(long nrows, const int *__restrict__ Ap,
                                                  const uint8_t *__restrict__ Ac, const double *__restrict__ Ax,
                                                  const pat_t *__restrict__ pat, int np,
                                                  const pat_t *__restrict__ val, int nv, uint8_t *__restrict__ Av,
                                                  int *__restrict__ bad)
{
    __shared__ pat_t spat[ROWPAT_MAX];
    __shared__ pat_t sv[VAL_WORDS][ROWVAL_MAX];
    for (int t = threadIdx.x; t < np; t += CT) spat[t] = pat[t];
    for (int t = threadIdx.x; t < VAL_WORDS * nv; t += CT) sv[t / nv][t % nv] = val[t];
    __syncthreads();
    GRID_STRIDE(i, nrows)
    {
        const int b = Ap[i], len = Ap[i + 1] - b;
        pat_t key[VAL_WORDS];
#pragma unroll
        for (int q = 0; q < VAL_WORDS; q++) key[q] = val_word(q, spat[Ac[i]], Ax, b, len);
        // -1 / 0 / 1: entry c below / equal to / above the key
        auto cmp = [&](int c) {
            int r = 0;
#pragma unroll
            for (int q = VAL_WORDS - 1; q >= 0; q--) {
                const pat_t w = sv[q][c];
                if (w != key[q]) r = w < key[q] ? -1 : 1;
            }
            return r;
        };
        int lo = 0, hi = nv - 1;
        while (lo < hi) {
            int mid = (lo + hi) >> 1;
            if (cmp(mid) < 0)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (cmp(lo) != 0) atomicOr(bad, 1);
        Av[i] = (uint8_t)lo;
    }
}

// build_windows' first test (capi.cpp): does some WIN_ROWS-row block's column
// span exceed WIN_CAP?  One workgroup per block
__global__ __launch_bounds__(CT) void k_win_wide(long nb, int nrows, const int *__restrict__ Ap,
                                                 const int *__restrict__ Aj, int *__restrict__ wide)
{
    __shared__ int slo, shi;
    for (long b = blockIdx.x; b < nb; b += gridDim.x) {
        if (threadIdx.x == 0) slo = INT32_MAX, shi = INT32_MIN;
        __syncthreads();
        long r0 = b * lssp_amd::WIN_ROWS, r1 = r0 + lssp_amd::WIN_ROWS < nrows ? r0 + lssp_amd::WIN_ROWS : nrows;
        int lo = INT32_MAX, hi = INT32_MIN;
        for (int k = Ap[r0] + threadIdx.x; k < Ap[r1]; k += CT) {
            lo = min(lo, Aj[k]);
            hi = max(hi, Aj[k]);
        }
        if (lo <= hi) {
            atomicMin(&slo, lo);
            atomicMax(&shi, hi);
        }
        __syncthreads();
        if (threadIdx.x == 0 && slo <= shi && (long)shi + 1 - (slo & ~1) > lssp_amd::WIN_CAP) atomicOr(wide, 1);
        __syncthreads();
    }
}

// The values of a windowed matrix's sliced copy (build_windows, capi.cpp) from
// its CSR values.  Thread t of 1024-row block b is lane l = t % 64 of slice
// 16 b + t / 64; s_row[1024 b + t] = its row in the block | that row's length
// << 10; entry k of the row goes to s_ax[s_meta[2 slice] + 64 k + l], so a wave
// writes 64 consecutive doubles per k.  Slots past a row's length (padding to
// the slice's longest row) are not touched: they hold +0.0 from the build.
__global__ __launch_bounds__(CT) void k_sell_refill(long nb, int nrows, const int *__restrict__ Ap,
                                                    const uint32_t *__restrict__ s_row,
                                                    const int *__restrict__ s_meta, const double *__restrict__ Ax,
                                                    double *__restrict__ s_ax)
{
    GRID_STRIDE(g, nb * lssp_amd::WIN_ROWS)
    {
        const uint32_t rw = s_row[g];
        const long row = g / lssp_amd::WIN_ROWS * lssp_amd::WIN_ROWS + (rw & (lssp_amd::WIN_ROWS - 1));
        if (row >= nrows) continue;
        const long slice = g / 64;
        const int l = (int)(g % 64), e0 = Ap[row];
        // the row's length as the layout was built for it, never past the slice's padded length
        const int len = min(min((int)(rw >> 10), Ap[row + 1] - e0), s_meta[2 * slice + 1]);
        double *dst = s_ax + s_meta[2 * slice] + l;
        for (int k = 0; k < len; k++) dst[64L * k] = Ax[e0 + k];
    }
}

// temporary device memory of one call, released after the stream drains
struct Scratch {
    hipStream_t s;
    std::vector<void *> p;
    explicit Scratch(hipStream_t st) : s(st) {}
    template <class T>
    T *get(long count)
    {
        void *q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(sizeof(T) * (size_t)std::max<long>(count, 1), 16)) != hipSuccess)
            return nullptr;
        p.push_back(q);
        return (T *)q;
    }
    ~Scratch()
    {
        (void)hipStreamSynchronize(s);
        for (void *q : p) (void)hipFree(q);
    }
};

#define SCRATCH(var, T, count)                         \
    T *var = S.get<T>(count);                          \
    if (!var) return LSSP_AMD_ENOMEM

int fetch(hipStream_t s, const int *d, int *h)
{
    LSSP_HIP(hipMemcpyAsync(h, d, sizeof(int), hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipStreamSynchronize(s));
    return LSSP_AMD_OK;
}

// run the structure checks queued on err and report
int checked(hipStream_t s, const int *err)
{
    int h = 0;
    int st = fetch(s, err, &h);
    if (st) return st;
    return h ? LSSP_AMD_EINVAL : LSSP_AMD_OK;
}

// rocPRIM's device-wide primitives (the library's own API): the LSD radix
// sort is stable, which is what reproduces the reference's counting sorts
template <class K, class V>
int sort_pairs(Scratch &S, const K *kin, K *kout, const V *vin, V *vout, long n, int bits)
{
    size_t bytes = 0;
    LSSP_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)bits, S.s));
    SCRATCH(t, char, (long)bytes);
    LSSP_HIP(rocprim::radix_sort_pairs(t, bytes, kin, kout, vin, vout, (size_t)n, 0u, (unsigned)bits, S.s));
    return LSSP_AMD_OK;
}

template <class K>
int sort_keys(Scratch &S, const K *kin, K *kout, long n, int bits)
{
    size_t bytes = 0;
    LSSP_HIP(rocprim::radix_sort_keys(nullptr, bytes, kin, kout, (size_t)n, 0u, (unsigned)bits, S.s));
    SCRATCH(t, char, (long)bytes);
    LSSP_HIP(rocprim::radix_sort_keys(t, bytes, kin, kout, (size_t)n, 0u, (unsigned)bits, S.s));
    return LSSP_AMD_OK;
}

int exclusive_sum(Scratch &S, const int *in, int *out, long n)
{
    size_t bytes = 0;
    LSSP_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0, (size_t)n, rocprim::plus<int>(), S.s));
    SCRATCH(t, char, (long)bytes);
    LSSP_HIP(rocprim::exclusive_scan(t, bytes, in, out, 0, (size_t)n, rocprim::plus<int>(), S.s));
    return LSSP_AMD_OK;
}

#define TRY(x)                     \
    do {                           \
        int st_ = (x);             \
        if (st_) return st_;       \
    } while (0)

// entries (key[k], value k) stably sorted by key, then row pointers over
// [0, nr] and the gathered (sj, sx): the counting sorts of coo_to_csr and
// transpose
int bucket(Scratch &S, long nnz, const int *key, int nr, const int *sj, const double *sx, int *P, int *dj,
           double *dx)
{
    hipStream_t s = S.s;
    SCRATCH(idx, int, nnz);
    SCRATCH(perm, int, nnz);
    SCRATCH(skey, unsigned, nnz);
    k_iota<<<grid_for(nnz), CT, 0, s>>>(nnz, idx);
    TRY(sort_pairs(S, (const unsigned *)key, skey, (const int *)idx, perm, nnz, bits_for((unsigned)std::max(nr - 1, 0))));
    k_row_ptr<<<grid_for((long)nr + 1), CT, 0, s>>>(nr, skey, (int)nnz, P);
    k_gather<<<grid_for(nnz), CT, 0, s>>>(nnz, perm, sj, sx, dj, dx);
    LSSP_HIP(hipGetLastError());
    return LSSP_AMD_OK;
}

}  // namespace

// The row codes of an offset-coded matrix, from its resident Ap and Ad: one
// routine for every construction path (upload, distributed upload, device
// arrays), so the codes, the table and aux_bytes are the same on each.  The
// patterns are numbered by ascending key, whatever order the rows arrived in.
int lssp_amd::build_row_codes(lssp_amd_ctx *c, lssp_amd_mat *M)
{
    M->npat = 0;
    if (M->ndiag == 0 || !M->Ad || M->nnz == 0 || M->nrows == 0) return LSSP_AMD_OK;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(gk, pat_t, PAT_HS + ROWPAT_MAX);
    SCRATCH(gi, int, 2);
    k_pat_init<<<1, CT, 0, s>>>(gk, gi);
    k_pat_collect<<<grid_for(M->nrows), CT, 0, s>>>(M->nrows, M->Ap, M->Ad, gk, gi);
    LSSP_HIP(hipGetLastError());
    int head[2];  // count, flag
    std::vector<pat_t> pat(ROWPAT_MAX);
    LSSP_HIP(hipMemcpyAsync(head, gi, sizeof(head), hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipMemcpyAsync(pat.data(), gk + PAT_HS, sizeof(pat_t) * ROWPAT_MAX, hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipStreamSynchronize(s));
    if (head[P_OVER] || head[P_COUNT] > ROWPAT_MAX || head[P_COUNT] <= 0) return LSSP_AMD_OK;  // not row-coded
    pat.resize(head[P_COUNT]);
    std::sort(pat.begin(), pat.end());
    // +32: padded as Ad is
    const size_t ac_bytes = (size_t)M->nrows + 32;
    LSSP_HIP(hipMalloc(&M->Ac, ac_bytes));
    LSSP_HIP(hipMalloc(&M->d_pat, sizeof(pat_t) * pat.size()));
    LSSP_HIP(hipMemsetAsync(M->Ac + M->nrows, 0, 32, s));
    LSSP_HIP(hipMemcpyAsync(M->d_pat, pat.data(), sizeof(pat_t) * pat.size(), hipMemcpyHostToDevice, s));
    k_pat_codes<<<grid_for(M->nrows), CT, 0, s>>>(M->nrows, M->Ap, M->Ad, M->d_pat, (int)pat.size(), M->Ac);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(s));
    // a key's length is the place of its highest non-zero byte, so the sorted keys' lengths ascend
    for (int l = 0; l < ROWPAT_LEN; l++) {
        int shorter = 0;
        for (pat_t k : pat) shorter += (k >> (8 * l)) == 0;  // at most l entries
        M->pat_thr[l] = (unsigned short)shorter;
    }
    M->aux_bytes += (long long)ac_bytes + (long long)sizeof(pat_t) * (long long)pat.size();
    M->npat = (int)pat.size();
    return LSSP_AMD_OK;
}

// The value codes of a row-coded matrix, from its resident Ap, Ac and Ax: one
// routine for the upload, mat_from_device and every lssp_amd_mat_update_values,
// which first drops what an earlier call built.  The value rows are numbered
// by ascending key, whatever order the rows arrived in.
int lssp_amd::build_val_codes(lssp_amd_ctx *c, lssp_amd_mat *M)
{
    // per value row: its key, and its decoded pattern (d_voff)
    constexpr long long ROW_BYTES = sizeof(pat_t) * VAL_WORDS + sizeof(int) * (ROWPAT_LEN + 1);
    auto drop = [M]() {
        if (M->Av) (void)hipFree(M->Av);
        if (M->d_val) (void)hipFree(M->d_val);
        if (M->d_voff) (void)hipFree(M->d_voff);
        M->Av = nullptr;
        M->d_val = nullptr;
        M->d_voff = nullptr;
    };
    if (M->nval > 0) M->aux_bytes -= (long long)M->nrows + 32 + ROW_BYTES * M->nval;
    M->nval = 0;
    drop();
    if (M->npat == 0 || !M->Ac || M->nnz == 0 || M->nrows == 0) return LSSP_AMD_OK;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(gk, pat_t, PAT_HS + ROWPAT_MAX);
    SCRATCH(gi, int, 2);
    SCRATCH(rep, int, ROWVAL_MAX);
    SCRATCH(keys, pat_t, VAL_WORDS * ROWVAL_MAX);
    SCRATCH(bad, int, 1);
    k_pat_init<<<1, CT, 0, s>>>(gk, gi);
    k_val_collect<<<grid_for(M->nrows), CT, 0, s>>>(M->nrows, M->Ap, M->Ac, M->Ax, gk, gi, rep);
    LSSP_HIP(hipGetLastError());
    int head[2];  // count, flag
    LSSP_HIP(hipMemcpyAsync(head, gi, sizeof(head), hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipStreamSynchronize(s));
    if (head[P_OVER] || head[P_COUNT] > ROWVAL_MAX || head[P_COUNT] <= 0) return LSSP_AMD_OK;  // not value-coded
    const int nv = head[P_COUNT];
    k_val_gather<<<1, CT, 0, s>>>(nv, rep, M->Ap, M->Ac, M->Ax, M->d_pat, keys);
    LSSP_HIP(hipGetLastError());
    typedef std::array<pat_t, VAL_WORDS> key_t;
    std::vector<key_t> key(nv);
    LSSP_HIP(hipMemcpyAsync(key.data(), keys, sizeof(key_t) * nv, hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipStreamSynchronize(s));
    std::sort(key.begin(), key.end());  // by pattern key (= by pattern code), then by the value bits in order
    std::vector<pat_t> tab((size_t)VAL_WORDS * nv);
    for (int q = 0; q < VAL_WORDS; q++)
        for (int t = 0; t < nv; t++) tab[(size_t)q * nv + t] = key[t][q];
    // +32: padded as Ac is
    const size_t av_bytes = (size_t)M->nrows + 32;
    LSSP_HIP(hipMalloc(&M->Av, av_bytes));
    LSSP_HIP(hipMalloc(&M->d_val, sizeof(pat_t) * tab.size()));
    LSSP_HIP(hipMemsetAsync(M->Av + M->nrows, 0, 32, s));
    LSSP_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
    LSSP_HIP(hipMemcpyAsync(M->d_val, tab.data(), sizeof(pat_t) * tab.size(), hipMemcpyHostToDevice, s));
    k_val_codes<<<grid_for(M->nrows), CT, 0, s>>>(M->nrows, M->Ap, M->Ac, M->Ax, M->d_pat, M->npat, M->d_val, nv,
                                                  M->Av, bad);
    LSSP_HIP(hipGetLastError());
    int hbad = 0;
    TRY(fetch(s, bad, &hbad));
    if (hbad) {  // two distinct rows shared a mix: the table lacks one of them
        drop();
        return LSSP_AMD_OK;
    }
    // the patterns decoded for the kernel
    std::vector<int> off(M->ndiag), voff((size_t)(ROWPAT_LEN + 1) * nv);
    LSSP_HIP(hipMemcpy(off.data(), M->d_off, sizeof(int) * off.size(), hipMemcpyDeviceToHost));
    for (int t = 0; t < nv; t++) {
        const pat_t pt = key[t][0];
        int len = 0;
        while (len < ROWPAT_LEN && ((pt >> (8 * len)) & 255u) != 0) len++;
        for (int k = 0; k < ROWPAT_LEN; k++)
            voff[(size_t)k * nv + t] = len ? off[(int)((pt >> (8 * std::min(k, len - 1))) & 255u) - 1] : 0;
        voff[(size_t)ROWPAT_LEN * nv + t] = len;
    }
    LSSP_HIP(hipMalloc(&M->d_voff, sizeof(int) * voff.size()));
    LSSP_HIP(hipMemcpy(M->d_voff, voff.data(), sizeof(int) * voff.size(), hipMemcpyHostToDevice));
    // as pat_thr: the sorted keys' lengths ascend
    for (int l = 0; l < ROWPAT_LEN; l++) {
        int shorter = 0;
        for (const key_t &k : key) shorter += (k[0] >> (8 * l)) == 0;  // at most l entries
        M->val_thr[l] = (unsigned short)shorter;
    }
    M->aux_bytes += (long long)av_bytes + ROW_BYTES * nv;
    M->nval = nv;
    return LSSP_AMD_OK;
}

extern "C" {

int lssp_amd_idx_alloc(lssp_amd_ctx *c, long n, int **d)
{
    if (!c || !d || n < 0) return LSSP_AMD_EINVAL;
    if (hipMalloc(d, sizeof(int) * std::max<long>(n, 1)) != hipSuccess) return LSSP_AMD_ENOMEM;
    return LSSP_AMD_OK;
}

int lssp_amd_idx_free(lssp_amd_ctx *c, int *d)
{
    if (!c) return LSSP_AMD_EINVAL;
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (d) LSSP_HIP(hipFree(d));
    return LSSP_AMD_OK;
}

int lssp_amd_idx_upload(lssp_amd_ctx *c, int *d, const int *h, long n)
{
    if (!c || n < 0 || (n > 0 && (!d || !h))) return LSSP_AMD_EINVAL;
    if (n == 0) return LSSP_AMD_OK;
    LSSP_HIP(hipMemcpyAsync(d, h, sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    return LSSP_AMD_OK;
}

int lssp_amd_idx_download(lssp_amd_ctx *c, int *h, const int *d, long n)
{
    if (!c || n < 0 || (n > 0 && (!d || !h))) return LSSP_AMD_EINVAL;
    if (n == 0) return LSSP_AMD_OK;
    LSSP_HIP(hipMemcpyAsync(h, d, sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    return LSSP_AMD_OK;
}

// matrix-utils.cxx:281-322
int lssp_amd_csr_to_coo(lssp_amd_ctx *c, int nrows, int nnz, const int *Ap, const int *Aj, const double *Ax,
                        int *Ci, int *Cj, double *Cx)
{
    if (!c || nrows < 0 || nnz < 0 || !Ap || (nnz > 0 && (!Aj || !Ax || !Ci))) return LSSP_AMD_EINVAL;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    k_check_ptr<<<grid_for((long)nrows + 1), CT, 0, s>>>(nrows, nnz, Ap, err);
    TRY(checked(s, err));
    if (nnz == 0) return LSSP_AMD_OK;
    k_expand_rows<<<grid_for(nrows), CT, 0, s>>>(nrows, Ap, Ci);
    LSSP_HIP(hipGetLastError());
    if (Cj) LSSP_HIP(hipMemcpyAsync(Cj, Aj, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
    if (Cx) LSSP_HIP(hipMemcpyAsync(Cx, Ax, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
    LSSP_HIP(hipStreamSynchronize(s));
    return LSSP_AMD_OK;
}

// matrix-utils.cxx:324-380
int lssp_amd_coo_to_csr(lssp_amd_ctx *c, int nrows, int nnz, const int *Ci, const int *Cj, const double *Cx,
                        int *Ap, int *Aj, double *Ax)
{
    if (!c || nrows < 0 || nnz < 0 || !Ap || (nnz > 0 && (!Ci || !Cj || !Cx || !Aj || !Ax)))
        return LSSP_AMD_EINVAL;
    hipStream_t s = c->stream;
    Scratch S(s);
    if (nnz == 0) {
        LSSP_HIP(hipMemsetAsync(Ap, 0, sizeof(int) * ((size_t)nrows + 1), s));
        LSSP_HIP(hipStreamSynchronize(s));
        return LSSP_AMD_OK;
    }
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    k_check_idx<<<grid_for(nnz), CT, 0, s>>>(nnz, Ci, nrows, err);
    TRY(checked(s, err));
    TRY(bucket(S, nnz, Ci, nrows, Cj, Cx, Ap, Aj, Ax));
    LSSP_HIP(hipStreamSynchronize(s));
    return LSSP_AMD_OK;
}

// matrix-utils.cxx:700-765
int lssp_amd_csr_transpose(lssp_amd_ctx *c, int nrows, int ncols, int nnz, const int *Ap, const int *Aj,
                           const double *Ax, int *Tp, int *Tj, double *Tx)
{
    if (!c || nrows <= 0 || ncols <= 0 || nnz < 0 || !Ap || !Tp || (nnz > 0 && (!Aj || !Ax || !Tj || !Tx)))
        return LSSP_AMD_EINVAL;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    k_check_ptr<<<grid_for((long)nrows + 1), CT, 0, s>>>(nrows, nnz, Ap, err);
    if (nnz > 0) k_check_idx<<<grid_for(nnz), CT, 0, s>>>(nnz, Aj, ncols, err);
    TRY(checked(s, err));
    if (nnz == 0) {
        LSSP_HIP(hipMemsetAsync(Tp, 0, sizeof(int) * ((size_t)ncols + 1), s));
        LSSP_HIP(hipStreamSynchronize(s));
        return LSSP_AMD_OK;
    }
    SCRATCH(Ci, int, nnz);
    k_expand_rows<<<grid_for(nrows), CT, 0, s>>>(nrows, Ap, Ci);
    TRY(bucket(S, nnz, Aj, ncols, Ci, Ax, Tp, Tj, Tx));
    LSSP_HIP(hipStreamSynchronize(s));
    return LSSP_AMD_OK;
}

// matrix-utils.cxx:62-162
int lssp_amd_csr_to_bcsr(lssp_amd_ctx *c, int n, int nnz, int bs, const int *Ap, const int *Aj,
                         const double *Ax, int *bnnz, int *Bp, int *Bj, double *Bx)
{
    if (!c || n <= 0 || nnz <= 0 || bs <= 0 || n % bs != 0 || !Ap || !Aj || !bnnz) return LSSP_AMD_EINVAL;
    if (Bj && (!Bp || !Bx || !Ax)) return LSSP_AMD_EINVAL;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    k_check_ptr<<<grid_for((long)n + 1), CT, 0, s>>>(n, nnz, Ap, err);
    k_check_idx<<<grid_for(nnz), CT, 0, s>>>(nnz, Aj, n, err);
    TRY(checked(s, err));
    int nb = n / bs;
    int cbits = bits_for((unsigned)(nb - 1)), rbits = bits_for((unsigned)(nb - 1));
    SCRATCH(key, uint64_t, nnz);
    SCRATCH(skey, uint64_t, nnz);
    SCRATCH(flag, int, nnz);
    SCRATCH(pos, int, nnz);
    k_block_keys<<<grid_for(n), CT, 0, s>>>(n, bs, cbits, Ap, Aj, key);
    TRY(sort_keys(S, (const uint64_t *)key, skey, nnz, cbits + rbits));
    k_unique_flag<<<grid_for(nnz), CT, 0, s>>>(nnz, skey, flag);
    TRY(exclusive_sum(S, flag, pos, nnz));
    int last_pos = 0, last_flag = 0;
    TRY(fetch(s, pos + nnz - 1, &last_pos));
    TRY(fetch(s, flag + nnz - 1, &last_flag));
    *bnnz = last_pos + last_flag;
    if (!Bj) return LSSP_AMD_OK;
    SCRATCH(brow, unsigned, *bnnz);
    k_unique_put<<<grid_for(nnz), CT, 0, s>>>(nnz, skey, flag, pos, cbits, Bj, brow);
    k_row_ptr<<<grid_for((long)nb + 1), CT, 0, s>>>(nb, brow, *bnnz, Bp);
    LSSP_HIP(hipMemsetAsync(Bx, 0, sizeof(double) * (size_t)*bnnz * bs * bs, s));
    k_bcsr_fill<<<grid_for(n), CT, 0, s>>>(n, bs, Ap, Aj, Ax, Bp, Bj, Bx);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(s));
    return LSSP_AMD_OK;
}

// matrix-utils.cxx:164-215 (and :387-481 on its result)
int lssp_amd_bcsr_to_csr(lssp_amd_ctx *c, int nbrows, int nbcols, int bs, int bnnz, const int *Bp,
                         const int *Bj, const double *Bx, int *nnz, int *Ap, int *Aj, double *Ax)
{
    if (!c || nbrows < 0 || nbcols < 0 || bs <= 0 || bnnz < 0 || !Bp || !nnz || (bnnz > 0 && (!Bj || !Bx)))
        return LSSP_AMD_EINVAL;
    if ((long)nbrows * bs > INT32_MAX - 1 || (long)nbcols * bs > INT32_MAX) return LSSP_AMD_EINVAL;
    if (Aj && (!Ap || !Ax)) return LSSP_AMD_EINVAL;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    k_check_ptr<<<grid_for((long)nbrows + 1), CT, 0, s>>>(nbrows, bnnz, Bp, err);
    if (bnnz > 0) k_check_idx<<<grid_for(bnnz), CT, 0, s>>>(bnnz, Bj, nbcols, err);
    TRY(checked(s, err));
    long n = (long)nbrows * bs;
    SCRATCH(cnt, int, n + 1);
    int *P = Ap;
    if (!P) {
        SCRATCH(Pt, int, n + 1);
        P = Pt;
    }
    LSSP_HIP(hipMemsetAsync(cnt + n, 0, sizeof(int), s));
    k_bcsr_count<<<grid_for(n), CT, 0, s>>>(n, bs, Bp, Bx, cnt);
    TRY(exclusive_sum(S, cnt, P, n + 1));
    TRY(fetch(s, P + n, nnz));
    if (!Aj) return LSSP_AMD_OK;
    k_bcsr_rows<<<grid_for(n), CT, 0, s>>>(n, bs, Bp, Bj, Bx, P, Aj, Ax);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(s));
    return LSSP_AMD_OK;
}

// matrix-utils.cxx:249-279 (CSR) and :217-247 (block columns of a BCSR): the same test
static int is_sorted_dev(lssp_amd_ctx *c, int nrows, int nnz, const int *Ap, const int *Aj, int *sorted)
{
    if (!c || nrows < 0 || nnz < 0 || !Ap || !sorted || (nnz > 0 && !Aj)) return LSSP_AMD_EINVAL;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(err, int, 3);  // structure, unsorted, long rows
    LSSP_HIP(hipMemsetAsync(err, 0, 3 * sizeof(int), s));
    k_check_ptr<<<grid_for((long)nrows + 1), CT, 0, s>>>(nrows, nnz, Ap, err);
    TRY(checked(s, err));
    *sorted = 1;
    if (nnz == 0) return LSSP_AMD_OK;
    k_is_sorted_rows<<<grid_for(nrows), CT, 0, s>>>(nrows, Ap, Aj, err + 1);
    LSSP_HIP(hipGetLastError());
    int h[2] = {0, 0};
    LSSP_HIP(hipMemcpyAsync(h, err + 1, sizeof(h), hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipStreamSynchronize(s));
    if (!h[0] && h[1]) {  // rows too long for one thread: every entry by its own
        k_is_sorted<<<grid_for(nnz), CT, 0, s>>>(nnz, nrows, Ap, Aj, err + 1);
        LSSP_HIP(hipGetLastError());
        TRY(fetch(s, err + 1, &h[0]));
    }
    *sorted = h[0] ? 0 : 1;
    return LSSP_AMD_OK;
}

int lssp_amd_csr_is_sorted(lssp_amd_ctx *c, int nrows, int nnz, const int *Ap, const int *Aj, int *sorted)
{
    return is_sorted_dev(c, nrows, nnz, Ap, Aj, sorted);
}

int lssp_amd_bcsr_is_sorted(lssp_amd_ctx *c, int nbrows, int bnnz, const int *Bp, const int *Bj, int *sorted)
{
    return is_sorted_dev(c, nbrows, bnnz, Bp, Bj, sorted);
}

// matrix-utils.cxx:387-481, in place
int lssp_amd_csr_sort_columns_dev(lssp_amd_ctx *c, int nrows, int ncols, int nnz, const int *Ap, int *Aj,
                                  double *Ax)
{
    if (!c || nrows < 0 || nnz < 0 || !Ap || (nnz > 0 && (!Aj || !Ax || ncols <= 0))) return LSSP_AMD_EINVAL;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    k_check_ptr<<<grid_for((long)nrows + 1), CT, 0, s>>>(nrows, nnz, Ap, err);
    if (nnz > 0) k_check_idx<<<grid_for(nnz), CT, 0, s>>>(nnz, Aj, ncols, err);
    TRY(checked(s, err));
    if (nnz == 0 || nrows == 0) return LSSP_AMD_OK;
    // rows of up to SORT_THREAD_MAX entries: one thread each
    SCRATCH(cand, int, (long)nrows + 1);
    SCRATCH(off, int, (long)nrows + 1);
    LSSP_HIP(hipMemsetAsync(cand + nrows, 0, sizeof(int), s));
    k_sort_short<<<grid_for(nrows), CT, 0, s>>>(nrows, Ap, Aj, Ax, cand);
    TRY(exclusive_sum(S, cand, off, (long)nrows + 1));
    int total = 0;
    TRY(fetch(s, off + nrows, &total));
    if (total == 0) return LSSP_AMD_OK;
    // longer rows, one thread per entry: which of them are out of order ...
    SCRATCH(uns, int, nrows);
    LSSP_HIP(hipMemsetAsync(uns, 0, sizeof(int) * (size_t)nrows, s));
    k_long_check<<<grid_for(total), CT, 0, s>>>(total, nrows, off, Ap, Aj, uns);
    k_long_len<<<grid_for(nrows), CT, 0, s>>>(nrows, uns, cand);
    TRY(exclusive_sum(S, cand, off, (long)nrows + 1));
    TRY(fetch(s, off + nrows, &total));
    if (total == 0) return LSSP_AMD_OK;
    // ... and those through one stable radix sort of (row, column) keys
    int cbits = bits_for((unsigned)(ncols - 1)), rbits = bits_for((unsigned)(nrows - 1));
    SCRATCH(key, uint64_t, total);
    SCRATCH(skey, uint64_t, total);
    SCRATCH(idx, int, total);
    SCRATCH(sidx, int, total);
    SCRATCH(vx, double, total);
    k_long_keys<<<grid_for(total), CT, 0, s>>>(total, nrows, cbits, off, Ap, Aj, Ax, key, idx, vx);
    TRY(sort_pairs(S, (const uint64_t *)key, skey, (const int *)idx, sidx, total, cbits + rbits));
    k_long_put<<<grid_for(total), CT, 0, s>>>(total, cbits, skey, sidx, vx, off, Ap, Aj, Ax);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(s));
    return LSSP_AMD_OK;
}

// the two-call protocol shared by adjust_zero_diag and get_block_diag: cnt
// (n + 1, last 0) summed into the row pointers, *mnnz fetched
static int sized_rows(Scratch &S, long n, const int *cnt, int *P, int *mnnz)
{
    TRY(exclusive_sum(S, cnt, P, n + 1));
    return fetch(S.s, P + n, mnnz);
}

// matrix-utils.cxx:483-587
int lssp_amd_csr_adjust_zero_diag(lssp_amd_ctx *c, int n, int nnz, const int *Ap, const int *Aj, const double *Ax,
                                  double tol, int *mnnz, int *Mp, int *Mj, double *Mx)
{
    if (!c || n <= 0 || nnz < 0 || !Ap || !mnnz || (nnz > 0 && !Aj)) return LSSP_AMD_EINVAL;
    if (Mj && (!Mp || !Mx || (nnz > 0 && !Ax))) return LSSP_AMD_EINVAL;
    if ((long)nnz + n > INT32_MAX) return LSSP_AMD_EINVAL;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    k_check_ptr<<<grid_for((long)n + 1), CT, 0, s>>>(n, nnz, Ap, err);
    if (nnz > 0) k_check_idx<<<grid_for(nnz), CT, 0, s>>>(nnz, Aj, n, err);
    TRY(checked(s, err));
    SCRATCH(cnt, int, (long)n + 1);
    int *P = Mp;
    if (!P) {
        SCRATCH(Pt, int, (long)n + 1);
        P = Pt;
    }
    LSSP_HIP(hipMemsetAsync(cnt + n, 0, sizeof(int), s));
    k_azd_count<<<grid_for(n), CT, 0, s>>>(n, Ap, Aj, cnt);
    TRY(sized_rows(S, n, cnt, P, mnnz));
    if (!Mj) return LSSP_AMD_OK;
    k_azd_fill<<<grid_for(n), CT, 0, s>>>(n, Ap, Aj, Ax, tol, P, Mj, Mx);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(s));
    return LSSP_AMD_OK;
}

// matrix-utils.cxx:589-698
int lssp_amd_csr_get_block_diag(lssp_amd_ctx *c, int n, int nnz, const int *Ap, const int *Aj, const double *Ax,
                                int blk, int *mnnz, int *Mp, int *Mj, double *Mx)
{
    if (!c || n <= 0 || nnz <= 0 || blk <= 0 || !Ap || !Aj || !mnnz) return LSSP_AMD_EINVAL;
    if (Mj && (!Mp || !Mx || !Ax)) return LSSP_AMD_EINVAL;
    if ((long)nnz + n > INT32_MAX) return LSSP_AMD_EINVAL;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    k_check_ptr<<<grid_for((long)n + 1), CT, 0, s>>>(n, nnz, Ap, err);
    k_check_idx<<<grid_for(nnz), CT, 0, s>>>(nnz, Aj, n, err);
    TRY(checked(s, err));
    if (blk == n) {  // :606-613: the matrix itself
        *mnnz = nnz;
        if (!Mj) return LSSP_AMD_OK;
        LSSP_HIP(hipMemcpyAsync(Mp, Ap, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
        LSSP_HIP(hipMemcpyAsync(Mj, Aj, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
        LSSP_HIP(hipMemcpyAsync(Mx, Ax, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
        LSSP_HIP(hipStreamSynchronize(s));
        return LSSP_AMD_OK;
    }
    SCRATCH(cnt, int, (long)n + 1);
    int *P = Mp;
    if (!P) {
        SCRATCH(Pt, int, (long)n + 1);
        P = Pt;
    }
    LSSP_HIP(hipMemsetAsync(cnt + n, 0, sizeof(int), s));
    k_bd_count<<<grid_for(n), CT, 0, s>>>(n, blk, Ap, Aj, cnt);
    TRY(sized_rows(S, n, cnt, P, mnnz));
    if (!Mj) return LSSP_AMD_OK;
    k_bd_fill<<<grid_for(n), CT, 0, s>>>(n, blk, Ap, Aj, Ax, P, Mj, Mx);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(s));
    return LSSP_AMD_OK;
}

// build_diag_ids (capi.cpp) for a CSR in HBM: the same table and byte stream
static int diag_ids_dev(lssp_amd_ctx *c, lssp_amd_mat *M)
{
    M->ndiag = 0;
    if (M->nnz == 0 || M->nrows == 0) return LSSP_AMD_OK;
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(g, int, G_SIZE);
    k_off_init<<<1, CT, 0, s>>>(g);
    k_off_collect<<<grid_for(M->nrows), CT, 0, s>>>(M->nrows, M->Ap, M->Aj, g);
    LSSP_HIP(hipGetLastError());
    int head[2 + DIAG_MAX];  // count, overflow, the offsets
    LSSP_HIP(hipMemcpyAsync(head, g + G_COUNT, sizeof(head), hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipStreamSynchronize(s));
    if (head[1] || head[0] > DIAG_MAX) return LSSP_AMD_OK;  // a 256th distinct offset: not coded
    std::vector<int> off(head + 2, head + 2 + head[0]);
    std::sort(off.begin(), off.end());
    // +32: see build_diag_ids
    const size_t ad_bytes = (size_t)M->nnz + 32;
    LSSP_HIP(hipMalloc(&M->Ad, ad_bytes));
    LSSP_HIP(hipMalloc(&M->d_off, sizeof(int) * off.size()));
    LSSP_HIP(hipMemsetAsync(M->Ad + M->nnz, 0, 32, s));
    LSSP_HIP(hipMemcpyAsync(M->d_off, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, s));
    k_off_ids<<<grid_for(M->nrows), CT, 0, s>>>(M->nrows, M->Ap, M->Aj, M->d_off, (int)off.size(), M->Ad);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(s));
    M->aux_bytes += (long long)ad_bytes + (long long)sizeof(int) * (long long)off.size();
    M->ndiag = (int)off.size();
    M->max_off = 0;
    for (int o : off) M->max_off = std::max(M->max_off, std::abs(o));
    M->max_off_int = M->max_off;
    TRY(lssp_amd::build_row_codes(c, M));
    return lssp_amd::build_val_codes(c, M);
}

// build_windows (capi.cpp) for a CSR in HBM: the span test runs on the device;
// only a matrix that passes it is downloaded, once, for the host routine that
// lays out the sliced copy
static int windows_dev(lssp_amd_ctx *c, lssp_amd_mat *M)
{
    if (M->ndiag > 0 || M->nnz == 0 || M->nrows == 0) return LSSP_AMD_OK;
    hipStream_t s = c->stream;
    {
        Scratch S(s);
        SCRATCH(wide, int, 1);
        LSSP_HIP(hipMemsetAsync(wide, 0, sizeof(int), s));
        const long nb = ((long)M->nrows + lssp_amd::WIN_ROWS - 1) / lssp_amd::WIN_ROWS;
        k_win_wide<<<(unsigned)std::min<long>(nb, 16384), CT, 0, s>>>(nb, M->nrows, M->Ap, M->Aj, wide);
        LSSP_HIP(hipGetLastError());
        int h = 0;
        TRY(fetch(s, wide, &h));
        if (h) return LSSP_AMD_OK;
    }
    std::vector<int> Ap((size_t)M->nrows + 1), Aj((size_t)M->nnz);
    std::vector<double> Ax((size_t)M->nnz);
    LSSP_HIP(hipMemcpyAsync(Ap.data(), M->Ap, sizeof(int) * Ap.size(), hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipMemcpyAsync(Aj.data(), M->Aj, sizeof(int) * Aj.size(), hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipMemcpyAsync(Ax.data(), M->Ax, sizeof(double) * Ax.size(), hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipStreamSynchronize(s));
    return lssp_amd::build_windows(M, Ap.data(), Aj.data(), Ax.data());
}

// lssp_amd_mat_upload (capi.cpp) from arrays in HBM
int lssp_amd_mat_from_device(lssp_amd_ctx *c, int nrows, int ncols, int nnz, const int *dAp, const int *dAj,
                             const double *dAx, lssp_amd_mat **out)
{
    if (!c || !out || nrows < 0 || ncols <= 0 || nnz < 0 || !dAp || (nnz > 0 && (!dAj || !dAx)))
        return LSSP_AMD_EINVAL;
    LSSP_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    {
        Scratch S(s);
        SCRATCH(err, int, 1);
        LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
        k_check_ptr<<<grid_for((long)nrows + 1), CT, 0, s>>>(nrows, nnz, dAp, err);
        if (nnz > 0) k_check_idx<<<grid_for(nnz), CT, 0, s>>>(nnz, dAj, ncols, err);
        TRY(checked(s, err));
    }
    lssp_amd_mat *M = new lssp_amd_mat();
    M->ctx = c;
    M->nrows = nrows;
    M->ncols = ncols;
    M->nnz = nnz;
    M->n_global = nrows;
    auto fill = [&]() -> int {
        // the handle's own copies, padded as upload_csr (capi.cpp) pads them
        LSSP_HIP(hipMalloc(&M->Ap, sizeof(int) * ((size_t)nrows + 1)));
        LSSP_HIP(hipMalloc(&M->Aj, sizeof(int) * ((size_t)nnz + 4)));
        LSSP_HIP(hipMalloc(&M->Ax, sizeof(double) * ((size_t)nnz + 4)));
        LSSP_HIP(hipMemcpyAsync(M->Ap, dAp, sizeof(int) * ((size_t)nrows + 1), hipMemcpyDeviceToDevice, s));
        if (nnz) {
            LSSP_HIP(hipMemcpyAsync(M->Aj, dAj, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
            LSSP_HIP(hipMemcpyAsync(M->Ax, dAx, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
        }
        TRY(diag_ids_dev(c, M));
        TRY(windows_dev(c, M));
        LSSP_HIP(hipStreamSynchronize(s));
        return LSSP_AMD_OK;
    };
    int st = fill();
    if (st != LSSP_AMD_OK) {
        lssp_amd_mat_destroy(M);
        return st;
    }
    // as lssp_amd_mat_upload: a measurement only
    if (lssp_amd::tune_spmv_streams(c, M) != LSSP_AMD_OK) (void)hipGetLastError();
    *out = M;
    return LSSP_AMD_OK;
}

// New values on the same pattern.  The offset ids, the row codes, the window
// spans and the sliced copy's columns and row order depend on the pattern
// alone; the value codes do not and are built again (build_val_codes).  The values
// are copied into the resident Ax and, for a windowed matrix, into the sliced
// copy's value slots (k_sell_refill); its padding slots stay +0.0.
int lssp_amd_mat_update_values(lssp_amd_ctx *c, lssp_amd_mat *A, const double *dAx, int nnz)
{
    if (!c || !A || !dAx || nnz != A->nnz) return LSSP_AMD_EINVAL;
    if (A->dist) return LSSP_AMD_EUNSUPPORTED;
    if (nnz == 0) return LSSP_AMD_OK;
    LSSP_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    LSSP_HIP(hipMemcpyAsync(A->Ax, dAx, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
    if (A->d_win) {
        const long nb = ((long)A->nrows + lssp_amd::WIN_ROWS - 1) / lssp_amd::WIN_ROWS;
        k_sell_refill<<<grid_for(nb * lssp_amd::WIN_ROWS), CT, 0, s>>>(nb, A->nrows, A->Ap, A->s_row, A->s_meta, A->Ax,
                                                                      A->s_ax);
        LSSP_HIP(hipGetLastError());
    }
    LSSP_HIP(hipStreamSynchronize(s));
    // the value codes describe the old values: rebuilt for the new ones, or dropped
    return lssp_amd::build_val_codes(c, A);
}

}  // extern "C"
