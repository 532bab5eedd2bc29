// ilut_dev.h -- the row body of lssp_amd_ilut_create_dev's kernel (k_ilut,
// ilut_factor.hip), written as lane-level steps over (lane, the
// wave's shared working row).  The kernel runs a step on its 64 lanes and joins
// them at its wave-level synchronisation points; a plain host loop over 64
// lanes between the same points runs the same code, under a sanitizer, against
// the oracle's ILUT (tools/ilut_dev_check.cpp).
//
// The working row of row i (ilut_factor_lu, ilu_setup.cpp; pc-ilut.cxx:51-286):
// positions [0, cap) hold the L part (columns < i) in the reference's order,
// [cap, 2 cap) the U part (columns > i), position 2 cap the diagonal.  The
// reference finds a column's position in an n-sized array (jr); here an
// open-addressing table of 4 cap slots maps column -> position.  A column that
// entered the row stays in the table: a processed pivot is never looked up again
// (every later column is larger), and at most 2 cap columns ever enter.
#pragma once

#include <cmath>
#include <cstdint>

#include "bilu_dev.h"

namespace lssp_amd {

constexpr int ILUT_LANES = 64;
// entries per part of the working row (the L part and the U part each): the
// first try, and the retry of a row set that overflowed it.  The constant-
// coefficient 7-point case needs 69 / 63 at (1e-4, 20), random non-dominant
// coefficients ~1000 / ~900
constexpr int ILUT_CAP_SMALL = 128, ILUT_CAP_LARGE = 1024;
constexpr double ILUT_ZERO_DIAG_TOL = 1e-10, ILUT_ZERO_DIAG_VALUE = 1e-3;  // pc-ilut.cxx:98, :249

struct IlutRow {
    int *jw;     // [2 cap + 1] columns
    double *w;   // [2 cap + 1] values
    int *hk;     // [4 cap] table keys (columns), -1 = empty
    int *hv;     // [4 cap] table values (positions)
    int cap;     // a power of two
};

BILU_HD inline int ilut_row_words(int cap) { return 2 * cap + 1; }
BILU_HD inline int ilut_table_slots(int cap) { return 4 * cap; }
BILU_HD inline int ilut_upos(const IlutRow &R, int u) { return R.cap + u; }
BILU_HD inline int ilut_dpos(const IlutRow &R) { return 2 * R.cap; }

BILU_HD inline unsigned ilut_hash(int col, int slots)
{
    unsigned x = (unsigned)col * 0x9E3779B1u;
    x ^= x >> 15;
    return x & (unsigned)(slots - 1);
}

// compare-and-swap of one table key: the lanes of a wave claim slots at the same time
BILU_HD inline int ilut_cas(int *p, int expect, int val)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, val);
#else
    const int old = *p;
    if (old == expect) *p = val;
    return old;
#endif
}

BILU_HD inline double ilut_guard(double d)  // pc-ilut.cxx:98-100, :249-251
{
    if (std::fabs(d) < ILUT_ZERO_DIAG_TOL) return d > 0 ? ILUT_ZERO_DIAG_VALUE : -ILUT_ZERO_DIAG_VALUE;
    return d;
}

// ---- the table ---------------------------------------------------------------
BILU_HD inline void ilut_clear_lane(const IlutRow &R, int lane)
{
    for (int s = lane; s < ilut_table_slots(R.cap); s += ILUT_LANES) R.hk[s] = -1;
}

// the lanes' columns are distinct and absent
BILU_HD inline void ilut_table_put(const IlutRow &R, int col, int pos)
{
    const int slots = ilut_table_slots(R.cap);
    unsigned s = ilut_hash(col, slots);
    for (;;) {
        if (ilut_cas(&R.hk[s], -1, col) == -1) {
            R.hv[s] = pos;
            return;
        }
        s = (s + 1) & (unsigned)(slots - 1);
    }
}

BILU_HD inline int ilut_table_slot(const IlutRow &R, int col)
{
    const int slots = ilut_table_slots(R.cap);
    unsigned s = ilut_hash(col, slots);
    for (;;) {
        const int k = R.hk[s];
        if (k == col) return (int)s;
        if (k == -1) return -1;
        s = (s + 1) & (unsigned)(slots - 1);
    }
}

// ---- row setup -----------------------------------------------------------------
// norm of A's row [b, e): the sequential sum in entry order over the entry count
// (pc-ilut.cxx:104-108); every lane computes the same value
BILU_HD inline double ilut_row_norm(const double *Ax, int b, int e)
{
    double norm = 0.0;
    for (int k = b; k < e; k++) norm += std::fabs(Ax[k]);
    return norm / (double)(e - b);
}

// the lane's entry (col, v) of A's row i goes to position at (the caller's
// ordered count of the entries of its part before it); the diagonal to its slot
BILU_HD inline void ilut_load_lane(const IlutRow &R, int i, int col, double v, int at)
{
    if (col == i) {
        R.jw[ilut_dpos(R)] = i;
        R.w[ilut_dpos(R)] = v;
        return;
    }
    R.jw[at] = col;
    R.w[at] = v;
    ilut_table_put(R, col, at);
}

// ---- the selection step (pc-ilut.cxx:127-150) -------------------------------------
// the lane's share of min jw[j .. nl): (column << 32) | position, the columns
// are distinct; INT64_MAX when the lane has none
BILU_HD inline long long ilut_min_lane(const IlutRow &R, int j, int nl, int lane)
{
    long long best = INT64_MAX;
    for (int k = j + lane; k < nl; k += ILUT_LANES) {
        const long long key = ((long long)R.jw[k] << 32) | (long long)k;
        if (key < best) best = key;
    }
    return best;
}

// one lane: the minimum (at position at) goes to position j, w with it
BILU_HD inline void ilut_swap(const IlutRow &R, int j, int at)
{
    if (at == j) return;
    const int col = R.jw[j];
    R.jw[j] = R.jw[at];
    R.jw[at] = col;
    const double t = R.w[j];
    R.w[j] = R.w[at];
    R.w[at] = t;
    R.hv[ilut_table_slot(R, col)] = at;  // (the minimum's own entry is never read again)
}

// ---- the update (pc-ilut.cxx:152-211) -----------------------------------------------
// where column col of a pivot row meets the working row of row i: its position,
// -1 = absent
BILU_HD inline int ilut_lookup_lane(const IlutRow &R, int i, int col)
{
    if (col == i) return ilut_dpos(R);
    const int s = ilut_table_slot(R, col);
    return s < 0 ? -1 : R.hv[s];
}

BILU_HD inline double ilut_mx(double aik, double u) { return -aik * u; }

// an absent column whose update is below the row's threshold is skipped
BILU_HD inline bool ilut_kept(int q, double mx, double rel) { return !(q == -1 && std::fabs(mx) < rel); }

// the lane's kept update: accumulated onto position q, or (q == -1) appended at
// position at -- the caller's ordered count by ballot and prefix, on its side
BILU_HD inline void ilut_update_lane(const IlutRow &R, int col, double mx, int q, int at)
{
    if (q >= 0) {
        R.w[q] += mx;
        return;
    }
    R.jw[at] = col;
    R.w[at] = mx;
    ilut_table_put(R, col, at);
}

// ---- the cut (pc-ilut.cxx:7-49) --------------------------------------------------
BILU_HD inline void ilut_qsplit(double *a, int *ind, int n, int ncut)
{
    int first = 0, last = n - 1;
    if (ncut < first || ncut >= last) return;
    for (;;) {
        int mid = first;
        const double key = std::fabs(a[mid]);
        for (int j = first + 1; j <= last; j++)
            if (std::fabs(a[j]) > key) {
                mid++;
                const double ta = a[mid];
                a[mid] = a[j];
                a[j] = ta;
                const int ti = ind[mid];
                ind[mid] = ind[j];
                ind[j] = ti;
            }
        const double ta = a[mid];
        a[mid] = a[first];
        a[first] = ta;
        const int ti = ind[mid];
        ind[mid] = ind[first];
        ind[first] = ti;
        if (mid == ncut) return;
        if (mid > ncut) last = mid - 1;
        else first = mid + 1;
    }
}

// ---- staging and pack offsets ---------------------------------------------------
// entries a row keeps per part, and the stride of its staging area: p, but no
// more than a row can hold (n - 1 columns on a side, cap positions)
BILU_HD inline int ilut_keep(int p, int n, int cap)
{
    int k = p < n - 1 ? p : n - 1;
    if (k > cap) k = cap;
    return k < 0 ? 0 : k;
}
BILU_HD inline long long ilut_stage_off(int i, int keep) { return (long long)i * keep; }
// rows of the packed factors: L = the strict entries, then (i, 1.0); U = the
// pivot, then the U part.  Row 0 is A's row 0 (len0 entries) in U and (0, 1.0) in L
BILU_HD inline int ilut_count_l(int i, int lcnt) { return i == 0 ? 1 : lcnt + 1; }
BILU_HD inline int ilut_count_u(int i, int ucnt, int len0) { return i == 0 ? len0 : ucnt + 1; }

}  // namespace lssp_amd
