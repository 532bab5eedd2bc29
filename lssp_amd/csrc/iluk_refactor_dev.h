// iluk_refactor_dev.h -- the per-row bodies of lssp_amd_iluk_refactor's kernels
// (DESIGN.md 3.3c): k_iluk_match / k_iluk_scatter (ilu_factor.hip),
// k_pk6_refill_scalar (trisolve.hip) and k_linef_refill (linefill.hip) call
// them, one row or slot per lane.  They are plain host + device functions so
// that their index arithmetic also runs on the host, under a sanitizer, against
// build_packets6's and fill_upload's own placement (tools/iluk_refill_check.cpp).
#pragma once

#include "bilu_refactor_dev.h"

namespace lssp_amd {

constexpr double ILUK_INSERTED_DIAG = 1e-10;  // what adjust_zero_diag(.., ZERO_DIAG_TOL) stores (pc.cxx:7)

// Row r of the CSR pattern (Ap, Aj; nnz entries) against row r of the factor
// pattern (Fp, Fj: columns strictly ascending, inside [0, n)) and its flag bytes
// fin (1 = an entry of the creating matrix, 0 = fill, 2 = an inserted diagonal).
// Returns 1 unless A's row is exactly F's flag-1 entries in F's order.  Because
// F's row is strictly ascending and in range, a row of A that walks it as a
// subsequence is so too: an unsorted row, a repeated or out-of-range column, a
// column F lacks and a column on a fill position all leave entries of A
// unmatched (or meet a flag other than 1).  Nothing of A is trusted: a row range
// outside [0, nnz) is reported without a read.
BILU_HD inline int iluk_match_row(int r, int nnz, const int *Ap, const int *Aj, const int *Fp, const int *Fj,
                                  const unsigned char *fin)
{
    const int a = Ap[r], b = Ap[r + 1];
    if (a < 0 || b > nnz || b < a) return 1;
    int k = a, bad = 0;
    for (int f = Fp[r]; f < Fp[r + 1]; f++) {
        if (k < b && Aj[k] == Fj[f]) {
            bad |= fin[f] != 1;
            k++;
        } else {
            bad |= fin[f] == 1;  // an entry of the creating matrix that A lacks
        }
    }
    return bad | (k != b);
}

// The same walk, after iluk_match_row accepted the row: F's values from A's.
// flag 1 takes A's value, flag 0 +0.0, flag 2 the inserted diagonal.
BILU_HD inline void iluk_scatter_row(int r, const int *Ap, const double *Ax, const int *Fp, const unsigned char *fin,
                                     double *Fx)
{
    int k = Ap[r];
    for (int f = Fp[r]; f < Fp[r + 1]; f++) Fx[f] = fin[f] == 1 ? Ax[k++] : fin[f] == 2 ? ILUK_INSERTED_DIAG : 0.0;
}

// Row r (of nr) of a packet record of a scalar factor: pk6_refill_row with
// bs = 1 on F (block row = row, first = the diagonal position), which places
// L's strict entries ascending and U's in descending storage order; the U
// sweep's record also gets D[r] = the stored pivot Fx[dpos[row]], the value
// build_bp_schedule takes from Ux (not its tiny-pivot replacement).  An L
// record's D stays the 1.0 of the unit diagonal.
BILU_HD inline void iluk_pk6_row(uint32_t *rec, int EP, int nr, int r, int row, bool upper, int n, const int *Fp,
                                 const int *Fj, const int *dpos, const double *Fx)
{
    if (row < 0 || row >= n) return;
    pk6_refill_row(rec, EP, nr, r, row, upper, 1, n, Fp, Fj, dpos, Fx);
    if (upper) reinterpret_cast<double *>(rec + pk6_layout(EP, nr).d)[r] = Fx[dpos[row]];
}

// k_linef's streams (linefill.hip fill_upload).  A tile (first line j0 of the
// skewed j' = j + k columns, nj lines, first plane k0, np planes, T levels)
// holds T * P * nj slots of NA doubles; local slot s = v * P * nj + p * nj + l
// is level v, plane p, line l, which is sweep row ((k0 + p) * ny + j) * nx + i
// with j = j0 + l - (k0 + p), i = v - 2 l - p - sig(p), sig = 1 on planes 4 ..
// 7.  Returns that sweep row, or -1 for a slot off the grid (p >= np, j or i
// outside the box), which holds +0.0.
constexpr int LINEF_P = 8;
BILU_HD inline long linef_slot_row(long s, int j0, int nj, int k0, int np, int nx, int ny)
{
    const long SB = (long)LINEF_P * nj;
    const long v = s / SB;
    const int q = (int)(s - v * SB), p = q / nj, l = q - p * nj;
    if (p >= np) return -1;
    const int j = j0 + l - (k0 + p);
    const long i = v - 2 * l - p - (p >> 2);
    if (j < 0 || j >= ny || i < 0 || i >= nx) return -1;
    return ((long)(k0 + p) * ny + j) * nx + i;
}

// The NA coefficients {B, BE, BN, S, SE, W(, diag)} of sweep row rs (FillCoef::
// build): natural row R = rs (L) or n - 1 - rs (U); the strict entries of F's
// row R on the sweep's side of the diagonal, each placed by its distance from
// the diagonal (pl, pl - 1, pl - nx, nx, nx - 1, anything else: 1), a missing
// neighbour +0.0; diag = U's stored pivot, L's unit 1.0.
BILU_HD inline void linef_coef_row(long rs, bool upper, long n, long nx, long pl, int NA, const int *Fp, const int *Fj,
                                   const int *dpos, const double *Fx, double *out)
{
    const long R = upper ? n - 1 - rs : rs;
    for (int a = 0; a < NA; a++) out[a] = 0.0;
    const int d = dpos[R];
    if (NA == 7) out[6] = upper ? Fx[d] : 1.0;
    const int b = upper ? d + 1 : Fp[R], e = upper ? Fp[R + 1] : d;
    for (int q = b; q < e; q++) {
        const long off = upper ? Fj[q] - R : R - Fj[q];
        const int a = off == pl ? 0 : off == pl - 1 ? 1 : off == pl - nx ? 2 : off == nx ? 3 : off == nx - 1 ? 4 : 5;
        out[a] = Fx[q];
    }
}

}  // namespace lssp_amd
