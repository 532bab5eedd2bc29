// bilu_refactor_dev.h -- the per-row bodies of lssp_amd_bilu_refactor's kernels
// (DESIGN.md 3.8): k_bilu_scatter (bilu_factor.hip) and k_pk6_refill
// (trisolve.hip) call them, one row per lane.  They are plain host + device
// functions so that their index arithmetic also runs on the host, under a
// sanitizer, against build_packets6's own placement (tools/bilu_refill_check.cpp).
#pragma once

#include <cstdint>

#include "bilu_dev.h"

namespace lssp_amd {

// The word offsets of a v6 packet record of nr rows and EP entry slots per row
// (tri_bp.cpp build_packets6): C at 0, V at v, D at d, ROW at row, end at end;
// each array padded to 4 words.
struct Pk6Layout {
    long v, d, row, end;
};
BILU_HD inline Pk6Layout pk6_layout(int EP, int nr)
{
    const long wc = ((long)(EP / 2) * nr + 3) & ~3L, wv = 2L * EP * nr;
    const long wd = (2L * nr + 3) & ~3L, wr = ((long)nr + 3) & ~3L;
    return Pk6Layout{wc, wc + wv, wc + wv + wd, wc + wv + wd + wr};
}

// the block of block column cb in the sorted block row Bj[s .. e); -1: absent
BILU_HD inline int bilu_find_block(const int *Bj, int s, int e, int cb)
{
    int lo = s, hi = e;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (Bj[mid] < cb) lo = mid + 1;
        else hi = mid;
    }
    return lo < e && Bj[lo] == cb ? lo : -1;
}

// Row r of the n x n CSR (Ap, Aj, Ax; nnz entries) into the zeroed block values
// Bx on the block pattern (Bp, Bj), as bilu_pattern places it: entry (r, c) at
// Bx[at(c / bs) * bs^2 + (c % bs) * bs + r % bs], the row's entries in storage
// order, so the last of a duplicated column wins.  hit[k] = 1 for every block
// that received an entry.  Nothing of the matrix is trusted: a row range outside
// [0, nnz), a column outside [0, n) or an entry whose block the pattern lacks
// is skipped and reported (return 1).
BILU_HD inline int bilu_scatter_row(int r, int n, int bs, int nnz, const int *Ap, const int *Aj, const double *Ax,
                                    const int *Bp, const int *Bj, double *Bx, unsigned char *hit)
{
    const int i = r / bs, rr = r - i * bs, bs2 = bs * bs;
    const int a = Ap[r], b = Ap[r + 1];
    if (a < 0 || b > nnz || b < a) return 1;
    const int s = Bp[i], e = Bp[i + 1];
    int bad = 0, last_cb = -1, at = -1;
    for (int k = a; k < b; k++) {
        const int col = Aj[k];
        if (col < 0 || col >= n) {
            bad = 1;
            continue;
        }
        const int cb = col / bs;
        if (cb != last_cb) {  // a row's entries mostly come block by block
            last_cb = cb;
            at = bilu_find_block(Bj, s, e, cb);
        }
        if (at < 0) {
            bad = 1;
            continue;
        }
        Bx[(size_t)at * bs2 + (size_t)(col - cb * bs) * bs + rr] = Ax[k];
        hit[at] = 1;
    }
    return bad;
}

// Row r (of nr) of a packet record: the values of its entry slots rewritten
// from the committed block values Fx.  rec = the record's first word, row = the
// natural row ROW[r] names: cell i = row / bs, row-in-cell rr.  Entry e sits at
// V[2 * ((e / 2) * nr + r) + (e & 1)] (build_packets6).
//   L sweep: L's strict entries ascending -- entry e is block Bp[i] + e / bs,
//            column e % bs, up to the row's first non-lower block first[i];
//   U sweep: U's strict entries in descending storage order -- entry e is block
//            Bp[i + 1] - 1 - e / bs, column bs - 1 - e % bs, down to the block
//            after the diagonal one.
// Whole pairs go out as one 16-byte store (consecutive lanes = consecutive
// pairs); the lone last entry of an odd row as 8 bytes, so slots past the row's
// length keep their build-time +0.0.  A row longer than EP cannot come from the
// pattern the record was built on; it is cut there rather than written past V.
BILU_HD inline void pk6_refill_row(uint32_t *rec, int EP, int nr, int r, int row, bool upper, int bs, int nb,
                                   const int *Bp, const int *Bj, const int *first, const double *Fx)
{
    const int i = row / bs, rr = row - i * bs, bs2 = bs * bs;
    if (i < 0 || i >= nb) return;
    const int f = first[i], end = Bp[i + 1];
    int nblk, k0;
    if (!upper) {
        k0 = Bp[i];
        nblk = f - k0;
    } else {
        k0 = end - 1;
        nblk = end - (f + (f < end && Bj[f] == i ? 1 : 0));
    }
    int len = nblk * bs;
    if (len > EP) len = EP;
    double *V = reinterpret_cast<double *>(rec + pk6_layout(EP, nr).v);
    auto val = [&](int e) {
        const int q = e / bs, m = e - q * bs;
        const size_t blk = upper ? (size_t)(k0 - q) : (size_t)(k0 + q);
        const int c = upper ? bs - 1 - m : m;
        return Fx[blk * bs2 + (size_t)c * bs + rr];
    };
    for (int e = 0; e < len; e += 2) {
        double *p = V + 2 * ((long)(e / 2) * nr + r);
        const double v0 = val(e);
        if (e + 1 < len) {
            const double v1 = val(e + 1);
#ifdef __HIP_DEVICE_COMPILE__
            typedef double v2d __attribute__((ext_vector_type(2)));
            *reinterpret_cast<v2d *>(p) = v2d{v0, v1};
#else
            p[0] = v0;
            p[1] = v1;
#endif
        } else {
            p[0] = v0;
        }
    }
}

}  // namespace lssp_amd
