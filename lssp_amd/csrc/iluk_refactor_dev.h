// iluk_refactor_dev.h -- the per-row bodies of lssp_amd_iluk_refactor's kernels
//  and of the line sweeps' coefficient-stream builders (3.3a):
// k_iluk_match / k_iluk_scatter (ilu_factor.hip), k_pk6_refill_scalar
// (trisolve.hip), k_coef_refill (linesweep.hip), k_linef_refill and build_lineg
// (linefill.hip) call them, one row or slot per lane.  They are plain host +
// device functions so that their index arithmetic also runs on the host, under
// a sanitizer, against an independent restatement of build_packets6's placement
// and of the stream layouts (tools/iluk_refill_check.cpp).
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

// ---- the line sweeps' coefficient streams ----
// k_coef_refill (linesweep.hip), k_linef_refill and build_lineg (linefill.hip)
// are their only builders; which offset is which component, and which row a
// slot holds, is written below and nowhere else.
//
// What a sweep's coefficients are read from.  Either the combined factor F (row
// = L's strict part, the diagonal, U's strict part; dpos, where the plan has
// it, narrows the scan to the sweep's side), whose L has the unit diagonal, or
// one lone factor (L: strict part, diagonal last; U: pivot first, strict part;
// dpos == nullptr), whose L diagonal is the stored value.
struct FactorView {
    const int *p, *j;
    const double *x;
    const int *dpos;  // per row of F: the diagonal's position (may be nullptr)
    bool unit;        // the L sweep's diagonal is the unit 1.0, not the stored entry
};
// the entries [b, e) of row R that can lie on the sweep's side, diagonal included
BILU_HD inline void factor_row_range(const FactorView &f, long R, bool upper, int &b, int &e)
{
    b = f.p[R];
    e = f.p[R + 1];
    if (f.dpos) (upper ? b : e) = f.dpos[R] + (upper ? 0 : 1);
}

// k_line2's streams.  A tile (first line j0, first plane k0, np planes; T levels
// of P planes x nj lines) holds slot (level s, plane p, line l) at s * P * nj +
// p * nj + l: sweep row ((k0 + p) * ny + j0 + l) * nx + i with i = s - l - p -
// line_sigma(p) (compute wave w owns planes 4w .. 4w+3 and runs (LV-1) w levels
// later).  Returns that sweep row, or -1 for a slot that holds +0.0 (p >= np, i
// off the line).
BILU_HD inline int line_sigma(int LV, int p) { return (LV - 1) * (p / 4); }
BILU_HD inline long line_slot_row(int s, int p, int l, int j0, int k0, int np, int nx, int ny, int LV)
{
    const int i = s - l - p - line_sigma(LV, p);
    if (p >= np || i < 0 || i >= nx) return -1;
    return ((long)(k0 + p) * ny + (j0 + l)) * nx + i;
}

// The NA coefficients {c_k, c_j, c_i(, diag)} of sweep row rs of the 5-/7-point
// ILU(0): natural row R = rs (L) or n - 1 - rs (U); the entries on the sweep's
// side of the diagonal by their distance from it (plane, nx, anything else: 1),
// a missing neighbour +0.0; diag = the stored entry, or the unit 1.0 of F's L.
// A grid row holds at most 7 entries: all loads are issued before the first is
// used.
BILU_HD inline void line_coef_row(long rs, bool upper, long n, long nx, long plane, int NA, const FactorView &f,
                                  double *out)
{
    const long R = upper ? n - 1 - rs : rs;
    int b, e;
    factor_row_range(f, R, upper, b, e);
    int fj[7];
    double fx[7];
#pragma unroll
    for (int u = 0; u < 7; u++) {
        const bool in = b + u < e;
        fj[u] = in ? f.j[b + u] : (int)R;
        fx[u] = in ? f.x[b + u] : 0.;
    }
    for (int a = 0; a < NA; a++) out[a] = 0.0;
#pragma unroll
    for (int u = 0; u < 7; u++) {
        const long off = upper ? (long)fj[u] - R : R - (long)fj[u];
        if (b + u >= e) continue;
        if (off > 0) out[off == plane ? 0 : off == nx ? 1 : 2] = fx[u];
        else if (off == 0 && NA == 4) out[3] = upper || !f.unit ? fx[u] : 1.0;
    }
}

// k_linef's streams.  A tile (first line j0 of the
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

// The NA coefficients {B, BE, BN, S, SE, W(, diag)} of sweep row rs of the
// 7-point ILU(1) pattern: natural row R = rs (L) or n - 1 - rs (U); the entries
// on the sweep's side of the diagonal, each placed by its distance from it (pl,
// pl - 1, pl - nx, nx, nx - 1, anything else: 1), a missing neighbour +0.0;
// diag = the stored entry, or the unit 1.0 of F's L.
BILU_HD inline void linef_coef_row(long rs, bool upper, long n, long nx, long pl, int NA, const FactorView &f,
                                   double *out)
{
    const long R = upper ? n - 1 - rs : rs;
    for (int a = 0; a < NA; a++) out[a] = 0.0;
    int b, e;
    factor_row_range(f, R, upper, b, e);
    for (int q = b; q < e; q++) {
        const long off = upper ? f.j[q] - R : R - f.j[q];
        if (off > 0)
            out[off == pl ? 0 : off == pl - 1 ? 1 : off == pl - nx ? 2 : off == nx ? 3 : off == nx - 1 ? 4 : 5] = f.x[q];
        else if (off == 0 && NA == 7) out[6] = upper || !f.unit ? f.x[q] : 1.0;
    }
}

}  // namespace lssp_amd
