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
// (capi.cpp) builds from a CSR in HBM; and the SpMV's codings of every
// handle (build_codings: offset ids, row codes, value codes).  Also the device
// half of the distributed builder (dist_check_dev, dist_localize_dev; the
// collective half is comm.cpp's) and the rank's diagonal block
// (lssp_amd_mat_local_block, lssp_amd_mat_local_block_refresh).
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

// ---- a distributed matrix's local numbering (lssp_amd::dist_localize_dev) -------
// halo entries of row i: the columns outside the rank's rows [row0, row0 + nl)
__global__ __launch_bounds__(CT) void k_halo_count(long nl, int row0, const int *__restrict__ Ap,
                                                   const int *__restrict__ Aj, int *__restrict__ cnt)
{
    GRID_STRIDE(i, nl)
    {
        int c = 0;
        for (int k = Ap[i]; k < Ap[i + 1]; k++) c += ((unsigned)(Aj[k] - row0) >= (unsigned)nl) ? 1 : 0;
        cnt[i] = c;
    }
}

__global__ __launch_bounds__(CT) void k_halo_fill(long nl, int row0, const int *__restrict__ Ap,
                                                  const int *__restrict__ Aj, const int *__restrict__ Hp,
                                                  int *__restrict__ raw)
{
    GRID_STRIDE(i, nl)
    {
        int o = Hp[i];
        for (int k = Ap[i]; k < Ap[i + 1]; k++)
            if ((unsigned)(Aj[k] - row0) >= (unsigned)nl) raw[o++] = Aj[k];
    }
}

// the first of every run of equal sorted keys; flag has n + 1 words, the last 0,
// so its exclusive sum ends with the number of distinct keys
__global__ __launch_bounds__(CT) void k_first_flag(long n, const unsigned *__restrict__ key, int *__restrict__ flag)
{
    GRID_STRIDE(i, n + 1) flag[i] = (i < n && (i == 0 || key[i] != key[i - 1])) ? 1 : 0;
}

__global__ __launch_bounds__(CT) void k_first_put(long n, const unsigned *__restrict__ key,
                                                  const int *__restrict__ pos, int *__restrict__ out)
{
    GRID_STRIDE(i, n)
    {
        if (i == 0 || key[i] != key[i - 1]) out[pos[i]] = (int)key[i];
    }
}

// global column -> local: an owned column g - row0, a halo column nl + its rank
// in the ascending halo list (bisection).  Four entries per thread, 16-byte
// accesses: Aj is padded to a multiple of four entries (nnz + 4 allocated)
__global__ __launch_bounds__(CT) void k_localize(long nnz, int row0, int nl, const int *__restrict__ hcols,
                                                 int nhalo, int *__restrict__ Aj)
{
    GRID_STRIDE(q, (nnz + 3) / 4)
    {
        int4 v = reinterpret_cast<const int4 *>(Aj)[q];
        int g[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (4 * q + t >= nnz) continue;  // the padding passes through
            if ((unsigned)(g[t] - row0) < (unsigned)nl) {
                g[t] -= row0;
                continue;
            }
            int lo = 0, hi = nhalo;
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                if (hcols[mid] < g[t])
                    lo = mid + 1;
                else
                    hi = mid;
            }
            g[t] = nl + lo;
        }
        reinterpret_cast<int4 *>(Aj)[q] = make_int4(g[0], g[1], g[2], g[3]);
    }
}

// per 256-row chunk of the localized matrix: does a row read a halo column, and
// the rows' widest |col - row| (a workgroup per chunk, a thread per row)
__global__ __launch_bounds__(CT) void k_chunk_halo(long nch, int nl, const int *__restrict__ Ap,
                                                   const int *__restrict__ Aj, int *__restrict__ ch_halo,
                                                   int *__restrict__ ch_off)
{
    __shared__ int s_halo, s_off;
    for (long ch = blockIdx.x; ch < nch; ch += gridDim.x) {
        if (threadIdx.x == 0) s_halo = 0, s_off = 0;
        __syncthreads();
        const long i = ch * CT + threadIdx.x;
        int halo = 0, mo = 0;
        if (i < nl)
            for (int k = Ap[i]; k < Ap[i + 1]; k++) {
                const int j = Aj[k];
                halo |= j >= nl ? 1 : 0;
                const int d = j - (int)i;
                mo = max(mo, d < 0 ? -d : d);
            }
        if (halo) atomicOr(&s_halo, 1);
        if (mo) atomicMax(&s_off, mo);
        __syncthreads();
        if (threadIdx.x == 0) {
            ch_halo[ch] = s_halo;
            ch_off[ch] = s_off;
        }
        __syncthreads();
    }
}

// ---- the rank's diagonal block (lssp_amd_mat_local_block) ----------------------
// entries of row i whose local column is owned (below nl); cnt has nl + 1 words
__global__ __launch_bounds__(CT) void k_lb_count(long nl, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                 int *__restrict__ cnt)
{
    GRID_STRIDE(i, nl)
    {
        int c = 0;
        for (int k = Ap[i]; k < Ap[i + 1]; k++) c += Aj[k] < (int)nl ? 1 : 0;
        cnt[i] = c;
    }
}

// the block's entries in A's order.  Bj == nullptr: the values alone, into a
// block whose row pointers are given (the refresh); a row whose owned entries are
// not exactly Bp's raises err and writes nothing past its slots
__global__ __launch_bounds__(CT) void k_lb_fill(long nl, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                const double *__restrict__ Ax, const int *__restrict__ Bp,
                                                int *__restrict__ Bj, double *__restrict__ Bx,
                                                int *__restrict__ err)
{
    GRID_STRIDE(i, nl)
    {
        int o = Bp[i];
        const int e = Bp[i + 1];
        for (int k = Ap[i]; k < Ap[i + 1]; k++)
            if (Aj[k] < (int)nl) {
                if (o < e) {
                    if (Bj) Bj[o] = Aj[k];
                    Bx[o] = Ax[k];
                }
                o++;
            }
        if (o != e) atomicOr(err, 1);
    }
}

// ---- the SpMV's codings: offset ids (Ad), row codes (Ac), value codes (Av) ----
// Each layer replaces something the product streams by a byte that indexes a
// table of at most 256 distinct keys: an entry's col - row, a row's pattern of
// offset ids, a row's pattern and values.  The three are built the same way: a
// kernel collects the distinct keys in an open-addressing set (k_collect), the
// host sorts them into the table (collect_keys), a second kernel bisects the
// table for every key and writes the byte.  A layer differs in its key type,
// in how a row yields its keys and in how many keys it admits: its policy
// (OffKeys, PatKeys, ValKeys).
using lssp_amd::DIAG_MAX;
using lssp_amd::ROWPAT_LEN;
using lssp_amd::ROWPAT_MAX;
using lssp_amd::ROWVAL_MAX;
typedef unsigned long long pat_t;
constexpr int SET_HS = 1024;       // hash slots of every key set
constexpr int SET_MAX = 256;       // the most keys a layer admits
constexpr int OFF_EMPTY = INT32_MIN;  // no col - row: columns are >= 0 and rows < INT32_MAX
constexpr pat_t PAT_EMPTY = ~0ull;    // eight entries of id 254: such a row leaves the matrix uncoded

__device__ __forceinline__ unsigned key_slot(int k) { return ((unsigned)k * 2654435761u) >> 22; }  // 10 bits
__device__ __forceinline__ unsigned key_slot(pat_t k) { return (unsigned)((k * 0x9E3779B97F4A7C15ull) >> 54); }  // 10 bits

// the device-wide set of a layer: the hash slots, then what the host fetches:
// the keys in arrival order, the row that brought each (layers with a payload),
// the number of distinct keys seen and the flag of a matrix the layer refuses
// (one key too many, or a row that cannot be coded)
template <class K>
struct KeySet {
    K slot[SET_HS];
    struct Found {
        K list[SET_MAX];
        int row[SET_MAX];
        int count, over;
    } found;
};

template <class K, K EMPTY>
__global__ __launch_bounds__(CT) void k_set_init(KeySet<K> *__restrict__ g)
{
    for (int t = threadIdx.x; t < SET_HS; t += CT) g->slot[t] = EMPTY;
    for (int t = threadIdx.x; t < SET_MAX; t += CT) g->found.list[t] = 0, g->found.row[t] = 0;
    if (threadIdx.x == 0) g->found.count = g->found.over = 0;
}

// k into the open-addressing set tab of HS slots; the slot this call claimed,
// or -1 (the key was there, or the set takes no more).
// A slot is READ first, so a key already present costs no atomic (a stencil's
// 7 offsets are there after the first rows).  Slots only ever fill, and every
// inserter of k walks the same probe sequence, so k lands in one slot only.
// *full (more than BOUND claims) stops further claims: the set never fills up
template <class K, int HS, K EMPTY, int BOUND>
__device__ __forceinline__ int set_insert(K *tab, const int *full, K k)
{
    unsigned h = key_slot(k);
    for (int p = 0; p < HS; p++, h = (h + 1) & (HS - 1)) {
        K cur = *(volatile K *)(tab + h);
        if (cur == k) return -1;
        if (cur != EMPTY) continue;
        if (*(volatile const int *)full > BOUND) return -1;
        K old = atomicCAS(tab + h, EMPTY, k);
        if (old == EMPTY) return (int)h;
        if (old == k) return -1;
    }
    return -1;
}

// a row's pattern key: byte k = Ad of its entry k, plus 1
__device__ __forceinline__ pat_t pat_key(const uint8_t *__restrict__ Ad, int b, int e)
{
    pat_t key = 0;
    for (int k = b; k < e; k++) key |= (pat_t)(Ad[k] + 1u) << (8 * (k - b));
    return key;
}

// A value row's key is its pattern and the bit patterns of its values in CSR
// order: nine 64-bit words, the pattern key (d_pat[Ac[i]]: ascending with the
// code) and eight values (+0.0 past the row's length, which the pattern fixes).
// The rows are collected by a 64-bit mix of the key, each distinct mix with one
// row that produced it; the table is then those rows' keys, and k_val_codes
// compares every row with the table in full, so two keys that share a mix
// leave the matrix uncoded instead of miscoded.
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

// The layers' policies.  row(i, put) hands row i's keys to put(key, at), at
// being the place of the byte that codes the key (k_codes), and returns false
// for a row the layer cannot code.  MAX: the keys admitted; ROWS: the set keeps
// the row that brought each key.
struct OffKeys {  // col - row of every entry (70 M entries hit 7 keys); coded at the entry
    typedef int key_t;
    static constexpr key_t EMPTY = OFF_EMPTY;
    static constexpr int MAX = DIAG_MAX;
    static constexpr bool ROWS = false;
    const int *__restrict__ Ap, *__restrict__ Aj;
    template <class F>
    __device__ __forceinline__ bool row(long i, F put) const
    {
        const int e = Ap[i + 1];
        for (int k = Ap[i]; k < e; k++) put(Aj[k] - (int)i, (long)k);
        return true;
    }
};
struct PatKeys {  // the row's pattern (10 M rows hit 27 keys); more than ROWPAT_LEN entries: not coded
    typedef pat_t key_t;
    static constexpr key_t EMPTY = PAT_EMPTY;
    static constexpr int MAX = ROWPAT_MAX;
    static constexpr bool ROWS = false;
    const int *__restrict__ Ap;
    const uint8_t *__restrict__ Ad;
    template <class F>
    __device__ __forceinline__ bool row(long i, F put) const
    {
        const int b = Ap[i], e = Ap[i + 1];
        const pat_t key = e - b <= ROWPAT_LEN ? pat_key(Ad, b, e) : PAT_EMPTY;
        if (key == PAT_EMPTY) return false;
        put(key, i);
        return true;
    }
};
struct ValKeys {  // the mix of the row's pattern code and values, and the row itself
    typedef pat_t key_t;
    static constexpr key_t EMPTY = PAT_EMPTY;
    static constexpr int MAX = ROWVAL_MAX;
    static constexpr bool ROWS = true;
    const int *__restrict__ Ap;
    const uint8_t *__restrict__ Ac;
    const double *__restrict__ Ax;
    template <class F>
    __device__ __forceinline__ bool row(long i, F put) const
    {
        put(val_hash(Ac[i], Ax, Ap[i], Ap[i + 1]), i);
        return true;
    }
};

// the distinct keys of all rows: each block collects its own in an LDS set
// (LDS reads, no global traffic, for the few keys of a stencil), then merges
// that set into the device-wide one, where a key new to it joins the list.
// One key more than P::MAX, or a row that cannot be coded, raises `over`, and
// every workgroup stops at its next row (a matrix of varying coefficients pays
// a fraction of one pass)
template <class P>
__global__ __launch_bounds__(CT) void k_collect(long nrows, const P p, KeySet<typename P::key_t> *__restrict__ g)
{
    typedef typename P::key_t K;
    __shared__ K tab[SET_HS];
    __shared__ int trow[P::ROWS ? SET_HS : 1];
    __shared__ int cnt;
    for (int t = threadIdx.x; t < SET_HS; t += CT) tab[t] = P::EMPTY;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    GRID_STRIDE(i, nrows)
    {
        if (*(volatile int *)&cnt > P::MAX || *(volatile int *)&g->found.over) break;
        const bool coded = p.row(i, [&](K k, long) {
            const int at = set_insert<K, SET_HS, P::EMPTY, P::MAX>(tab, &cnt, k);
            if (at < 0) return;
            if (P::ROWS) trow[at] = (int)i;
            atomicAdd(&cnt, 1);
        });
        if (!coded) {
            atomicOr(&g->found.over, 1);
            break;
        }
    }
    __syncthreads();
    if (cnt > P::MAX) {
        if (threadIdx.x == 0) atomicOr(&g->found.over, 1);
        return;
    }
    for (int t = threadIdx.x; t < SET_HS; t += CT) {
        const K k = tab[t];
        if (k == P::EMPTY || set_insert<K, SET_HS, P::EMPTY, P::MAX>(g->slot, &g->found.count, k) < 0) continue;
        const int at = atomicAdd(&g->found.count, 1);
        if (at < P::MAX) {
            g->found.list[at] = k;
            if (P::ROWS) g->found.row[at] = trow[t];
        } else {
            atomicOr(&g->found.over, 1);
        }
    }
}

// the first of n ascending table entries that is not below the key: below(m)
// tells whether entry m is
template <class F>
__device__ __forceinline__ int lower_bound(int n, F below)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (below(mid))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// out[at] = index of the key in the ascending table tabg[0, n), for every key
// of every row (Ad per entry, Ac per row); the keys are in the table by construction
template <class P>
__global__ __launch_bounds__(CT) void k_codes(long nrows, const P p, const typename P::key_t *__restrict__ tabg,
                                              int n, uint8_t *__restrict__ out)
{
    typedef typename P::key_t K;
    __shared__ K tab[SET_MAX];
    for (int t = threadIdx.x; t < n; t += CT) tab[t] = tabg[t];
    __syncthreads();
    GRID_STRIDE(i, nrows)
    {
        p.row(i, [&](K key, long at) { out[at] = (uint8_t)lower_bound(n, [&](int m) { return tab[m] < key; }); });
    }
}

// row i's value key, word q
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
        const int lo = lower_bound(nv, [&](int c) { return cmp(c) < 0; });
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

namespace {

// A layer's distinct keys over the matrix's rows: keys comes back ascending,
// or empty when the layer refuses the matrix (one key too many, a row that
// cannot be coded, no key at all).  *set is the device-wide set in S, whose
// found.row a layer with a payload reads next.  The table is sorted, so the
// codes do not depend on the order the keys arrived in.
template <class P>
int collect_keys(Scratch &S, long nrows, const P &p, std::vector<typename P::key_t> &keys,
                 KeySet<typename P::key_t> **set = nullptr)
{
    typedef KeySet<typename P::key_t> Set;
    keys.clear();
    SCRATCH(g, Set, 1);
    k_set_init<typename P::key_t, P::EMPTY><<<1, CT, 0, S.s>>>(g);
    k_collect<P><<<grid_for(nrows), CT, 0, S.s>>>(nrows, p, g);
    LSSP_HIP(hipGetLastError());
    typename Set::Found f;
    LSSP_HIP(hipMemcpyAsync(&f, &g->found, sizeof(f), hipMemcpyDeviceToHost, S.s));
    LSSP_HIP(hipStreamSynchronize(S.s));
    if (set) *set = g;
    if (f.over || f.count > P::MAX || f.count <= 0) return LSSP_AMD_OK;  // not coded
    keys.assign(f.list, f.list + f.count);
    std::sort(keys.begin(), keys.end());
    return LSSP_AMD_OK;
}

// a stream of n code bytes in HBM.  +32: the SpMV stages a byte stream with
// 16-byte loads that may touch one vector past the last code
int byte_stream(hipStream_t s, size_t n, uint8_t **d, size_t *bytes)
{
    *bytes = n + 32;
    LSSP_HIP(hipMalloc(d, *bytes));
    LSSP_HIP(hipMemsetAsync(*d + n, 0, 32, s));
    return LSSP_AMD_OK;
}

// thr[l] = how many of the n ascending pattern keys have at most l entries: a
// key's length is the place of its highest non-zero byte, so the sorted keys'
// lengths ascend and a code's length is the number of thresholds it reaches
void length_thresholds(const pat_t *key, int n, unsigned short *thr)
{
    for (int l = 0; l < ROWPAT_LEN; l++) {
        int shorter = 0;
        for (int t = 0; t < n; t++) shorter += (key[t] >> (8 * l)) == 0;
        thr[l] = (unsigned short)shorter;
    }
}

// a layer's table in HBM
template <class K>
int upload_table(hipStream_t s, const std::vector<K> &tab, K **d)
{
    LSSP_HIP(hipMalloc(d, sizeof(K) * tab.size()));
    LSSP_HIP(hipMemcpyAsync(*d, tab.data(), sizeof(K) * tab.size(), hipMemcpyHostToDevice, s));
    return LSSP_AMD_OK;
}

// The offset ids of a CSR in HBM: at most DIAG_MAX distinct col - row (5- / 7- /
// 27-point stencils, the z-slab halo columns of a distributed stencil), every
// entry the byte index of its offset in the ascending table.  Rows are summed
// exactly as before (same entries, same order): only the way the column is
// found changes.  set_max_off_int: the matrix's halo-free rows are all its rows
int build_off_ids(lssp_amd_ctx *c, lssp_amd_mat *M, bool set_max_off_int)
{
    M->ndiag = 0;
    if (M->nnz == 0 || M->nrows == 0) return LSSP_AMD_OK;
    hipStream_t s = c->stream;
    Scratch S(s);
    const OffKeys p{M->Ap, M->Aj};
    std::vector<int> off;
    TRY(collect_keys(S, M->nrows, p, off));
    if (off.empty()) return LSSP_AMD_OK;  // a 256th distinct offset: not coded
    size_t ad_bytes = 0;
    TRY(byte_stream(s, (size_t)M->nnz, &M->Ad, &ad_bytes));
    TRY(upload_table(s, off, &M->d_off));
    k_codes<OffKeys><<<grid_for(M->nrows), CT, 0, s>>>(M->nrows, p, M->d_off, (int)off.size(), M->Ad);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(s));
    M->aux_bytes += (long long)ad_bytes + (long long)sizeof(int) * (long long)off.size();
    M->ndiag = (int)off.size();
    M->max_off = 0;
    for (int o : off) M->max_off = std::max(M->max_off, std::abs(o));
    if (set_max_off_int) M->max_off_int = M->max_off;
    return LSSP_AMD_OK;
}

// The row codes of an offset-coded matrix, from its resident Ap and Ad: the
// patterns are numbered by ascending key
int build_row_codes(lssp_amd_ctx *c, lssp_amd_mat *M)
{
    M->npat = 0;
    if (M->ndiag == 0 || !M->Ad || M->nnz == 0 || M->nrows == 0) return LSSP_AMD_OK;
    hipStream_t s = c->stream;
    Scratch S(s);
    const PatKeys p{M->Ap, M->Ad};
    std::vector<pat_t> pat;
    TRY(collect_keys(S, M->nrows, p, pat));
    if (pat.empty()) return LSSP_AMD_OK;  // a 257th pattern, or a row of more than ROWPAT_LEN entries: not row-coded
    size_t ac_bytes = 0;
    TRY(byte_stream(s, (size_t)M->nrows, &M->Ac, &ac_bytes));
    TRY(upload_table(s, pat, &M->d_pat));
    k_codes<PatKeys><<<grid_for(M->nrows), CT, 0, s>>>(M->nrows, p, M->d_pat, (int)pat.size(), M->Ac);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(s));
    length_thresholds(pat.data(), (int)pat.size(), M->pat_thr);
    M->aux_bytes += (long long)ac_bytes + (long long)sizeof(pat_t) * (long long)pat.size();
    M->npat = (int)pat.size();
    return LSSP_AMD_OK;
}

}  // namespace

// The value codes of a row-coded matrix, from its resident Ap, Ac and Ax:
// build_codings' last step, and all of lssp_amd_mat_update_values' rebuild,
// so it first drops what an earlier call built.  The value rows are numbered
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
    SCRATCH(keys, pat_t, VAL_WORDS * ROWVAL_MAX);
    SCRATCH(bad, int, 1);
    std::vector<pat_t> mix;
    KeySet<pat_t> *set = nullptr;
    TRY(collect_keys(S, M->nrows, ValKeys{M->Ap, M->Ac, M->Ax}, mix, &set));
    if (mix.empty()) return LSSP_AMD_OK;  // a 257th distinct value row: not value-coded
    const int nv = (int)mix.size();
    k_val_gather<<<1, CT, 0, s>>>(nv, set->found.row, M->Ap, M->Ac, M->Ax, M->d_pat, keys);
    LSSP_HIP(hipGetLastError());
    typedef std::array<pat_t, VAL_WORDS> key_t;
    std::vector<key_t> key(nv);
    LSSP_HIP(hipMemcpyAsync(key.data(), keys, sizeof(key_t) * nv, hipMemcpyDeviceToHost, s));
    LSSP_HIP(hipStreamSynchronize(s));
    std::sort(key.begin(), key.end());  // by pattern key (= by pattern code), then by the value bits in order
    std::vector<pat_t> tab((size_t)VAL_WORDS * nv);
    for (int q = 0; q < VAL_WORDS; q++)
        for (int t = 0; t < nv; t++) tab[(size_t)q * nv + t] = key[t][q];
    size_t av_bytes = 0;
    TRY(byte_stream(s, (size_t)M->nrows, &M->Av, &av_bytes));
    TRY(upload_table(s, tab, &M->d_val));
    LSSP_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
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
    length_thresholds(tab.data(), nv, M->val_thr);  // (the table's first row: the pattern keys)
    M->aux_bytes += (long long)av_bytes + ROW_BYTES * nv;
    M->nval = nv;
    return LSSP_AMD_OK;
}

// The SpMV's codings of a matrix whose CSR is in HBM, layer on layer: offset
// ids, then row codes, then value codes.  One routine for every construction
// path (lssp_amd_mat_upload, lssp_amd_mat_upload_dist, lssp_amd_mat_from_device),
// so the codes, the tables and aux_bytes are the same on each.  step, when
// given, sees every layer's status and returns what to go on with
// (lssp_amd_mat_upload_dist: the status the ranks agree on).
int lssp_amd::build_codings(lssp_amd_ctx *c, lssp_amd_mat *M, int (*step)(lssp_amd_ctx *, int))
{
    auto done = [&](int st) { return step ? step(c, st) : st; };
    // a matrix with halo columns keeps the max_off_int that the distributed
    // upload computed over its halo-free chunks
    TRY(done(build_off_ids(c, M, M->nhalo == 0)));
    TRY(done(build_row_codes(c, M)));
    // A distributed matrix is not value-coded and stays on COL_ROW: its
    // products are split at the halo rows, so the eligibility test would need
    // one more agreement round (and lssp_amd_mat_update_values a collective)
    if (M->dist) return LSSP_AMD_OK;
    return done(build_val_codes(c, M));
}

// The structure checks of a distributed matrix whose local rows are resident
// with GLOBAL columns: Ap[0] == 0, Ap non-decreasing, Ap[nrows] == nnz, every
// column in [0, n_global).  Nothing indexes with a column before this passed.
int lssp_amd::dist_check_dev(lssp_amd_ctx *c, const lssp_amd_mat *M)
{
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    k_check_ptr<<<grid_for((long)M->nrows + 1), CT, 0, s>>>(M->nrows, M->nnz, M->Ap, err);
    if (M->nnz > 0) k_check_idx<<<grid_for(M->nnz), CT, 0, s>>>(M->nnz, M->Aj, M->n_global, err);
    LSSP_HIP(hipGetLastError());
    return checked(s, err);
}

// The local numbering of a checked distributed matrix, in place: hcols comes
// back as the halo columns, ascending (= grouped by owner, then ascending: the
// owners hold contiguous ranges); Aj becomes [owned | halo]; nhalo, ncols, the
// longest run [ich0, ich1) of halo-free 256-row chunks (the first of equals)
// and max_off_int over its rows are set.  Local to the rank: no collective.
// Only the halo list and two words per chunk cross to the host.
int lssp_amd::dist_localize_dev(lssp_amd_ctx *c, lssp_amd_mat *M, std::vector<int> &hcols)
{
    const int nl = M->nrows, nnz = M->nnz, row0 = M->row0;
    hipStream_t s = c->stream;
    Scratch S(s);
    hcols.clear();
    int nh = 0;
    if (nl > 0 && nnz > 0) {
        SCRATCH(cnt, int, (long)nl + 1);
        SCRATCH(Hp, int, (long)nl + 1);
        LSSP_HIP(hipMemsetAsync(cnt + nl, 0, sizeof(int), s));
        k_halo_count<<<grid_for(nl), CT, 0, s>>>(nl, row0, M->Ap, M->Aj, cnt);
        int nraw = 0;
        TRY(exclusive_sum(S, cnt, Hp, (long)nl + 1));
        TRY(fetch(s, Hp + nl, &nraw));
        if (nraw > 0) {
            SCRATCH(raw, unsigned, nraw);
            SCRATCH(srt, unsigned, nraw);
            SCRATCH(flag, int, (long)nraw + 1);
            SCRATCH(pos, int, (long)nraw + 1);
            k_halo_fill<<<grid_for(nl), CT, 0, s>>>(nl, row0, M->Ap, M->Aj, Hp, (int *)raw);
            TRY(sort_keys(S, (const unsigned *)raw, srt, nraw, bits_for((unsigned)(M->n_global - 1))));
            k_first_flag<<<grid_for((long)nraw + 1), CT, 0, s>>>(nraw, srt, flag);
            TRY(exclusive_sum(S, flag, pos, (long)nraw + 1));
            TRY(fetch(s, pos + nraw, &nh));
            int *uniq = (int *)raw;  // the unsorted list is done with
            k_first_put<<<grid_for(nraw), CT, 0, s>>>(nraw, srt, pos, uniq);
            LSSP_HIP(hipGetLastError());
            hcols.resize(nh);
            LSSP_HIP(hipMemcpyAsync(hcols.data(), uniq, sizeof(int) * (size_t)nh, hipMemcpyDeviceToHost, s));
            k_localize<<<grid_for(((long)nnz + 3) / 4), CT, 0, s>>>(nnz, row0, nl, uniq, nh, M->Aj);
        } else {
            k_localize<<<grid_for(((long)nnz + 3) / 4), CT, 0, s>>>(nnz, row0, nl, nullptr, 0, M->Aj);
        }
        LSSP_HIP(hipGetLastError());
    }
    M->nhalo = nh;
    M->ncols = nl + nh;
    // the longest run of chunks without a halo-reading row (spmv_halo), and the
    // widest reach of its rows (the U sweep's tail product, linesweep.hip)
    const long nch = num_chunks(nl);
    std::vector<int> ch_halo((size_t)nch), ch_off((size_t)nch);
    if (nch > 0) {
        SCRATCH(d_halo, int, nch);
        SCRATCH(d_off, int, nch);
        k_chunk_halo<<<(unsigned)std::min<long>(nch, 16384), CT, 0, s>>>(nch, nl, M->Ap, M->Aj, d_halo, d_off);
        LSSP_HIP(hipGetLastError());
        LSSP_HIP(hipMemcpyAsync(ch_halo.data(), d_halo, sizeof(int) * (size_t)nch, hipMemcpyDeviceToHost, s));
        LSSP_HIP(hipMemcpyAsync(ch_off.data(), d_off, sizeof(int) * (size_t)nch, hipMemcpyDeviceToHost, s));
    }
    LSSP_HIP(hipStreamSynchronize(s));
    long run0 = 0, best0 = 0, best1 = 0;
    for (long ch = 0; ch <= nch; ch++)
        if (ch == nch || ch_halo[ch]) {
            if (ch - run0 > best1 - best0) best0 = run0, best1 = ch;
            run0 = ch + 1;
        }
    M->ich0 = best0;
    M->ich1 = best1;
    int mo = 0;
    for (long ch = best0; ch < best1; ch++) mo = std::max(mo, ch_off[ch]);
    M->max_off_int = mo;
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
        TRY(lssp_amd::build_codings(c, M));
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
    // the value codes describe the old values: rebuilt for the new ones, or
    // dropped.  A distributed matrix has none (build_codings): local, no collective
    if (A->dist) return LSSP_AMD_OK;
    return lssp_amd::build_val_codes(c, A);
}

// The rank's diagonal block of a distributed matrix as a single-rank handle:
// the entries whose local column is owned, in A's order (per-row counts, a scan,
// a fill), handed to lssp_amd_mat_from_device, so B is the handle of the
// host-extracted block in every observable way.  A row left without an entry
// stays empty.
int lssp_amd_mat_local_block(lssp_amd_ctx *c, const lssp_amd_mat *A, lssp_amd_mat **B)
{
    if (!c || !A || !B || A->nrows <= 0) return LSSP_AMD_EINVAL;
    LSSP_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Scratch S(s);
    const int nl = A->nrows;
    SCRATCH(cnt, int, (long)nl + 1);
    SCRATCH(Bp, int, (long)nl + 1);
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(cnt + nl, 0, sizeof(int), s));
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    k_lb_count<<<grid_for(nl), CT, 0, s>>>(nl, A->Ap, A->Aj, cnt);
    int bnnz = 0;
    TRY(sized_rows(S, nl, cnt, Bp, &bnnz));
    SCRATCH(Bj, int, bnnz);
    SCRATCH(Bx, double, bnnz);
    k_lb_fill<<<grid_for(nl), CT, 0, s>>>(nl, A->Ap, A->Aj, A->Ax, Bp, Bj, Bx, err);
    LSSP_HIP(hipGetLastError());
    return lssp_amd_mat_from_device(c, nl, nl, bnnz, Bp, Bj, Bx, B);
}

// B's values again from the values A holds now.  The fill goes to a temporary
// and checks on the way that A's owned entries per row are B's row lengths, so a
// mismatch leaves B as it was; the rest is lssp_amd_mat_update_values.
int lssp_amd_mat_local_block_refresh(lssp_amd_ctx *c, lssp_amd_mat *B, const lssp_amd_mat *A)
{
    if (!c || !B || !A) return LSSP_AMD_EINVAL;
    if (B->dist || B->nhalo > 0 || B->nrows != A->nrows || B->ncols != A->nrows) return LSSP_AMD_EINVAL;
    LSSP_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Scratch S(s);
    SCRATCH(Bx, double, B->nnz);
    SCRATCH(err, int, 1);
    LSSP_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
    if (B->nrows > 0) {
        k_lb_fill<<<grid_for(B->nrows), CT, 0, s>>>(B->nrows, A->Ap, A->Aj, A->Ax, B->Ap, nullptr, Bx, err);
        LSSP_HIP(hipGetLastError());
    }
    TRY(checked(s, err));
    return lssp_amd_mat_update_values(c, B, Bx, B->nnz);
}

}  // extern "C"
