// iluk_symbolic_dev.h -- the row body of lssp_amd_pc_create_dev's symbolic
// ILU(k) kernel (k_iluk_symbolic, iluk_symbolic.hip), written as
// lane-level steps over (lane, the wave's shared working row), as ilut_dev.h
// is.  The kernel runs a step on its 64 lanes and joins them at its wave-level
// synchronisation points; a plain host loop over 64 lanes between the same
// points runs the same code, under a sanitizer, against the oracle's ILUK
// pattern (tools/iluk_symbolic_check.cpp).
//
// The working row of row i (iluk_symbolic, ilu_setup.cpp; pc-iluk.cxx:22-135):
// positions [0, cap) hold the L part (columns < i), [cap, 2 cap) the U part
// (columns > i); the diagonal is known to be there and has no slot.  Each
// position carries its column, its level of fill (one byte: levels beyond 254
// are refused) and an origin bit (1 = an entry of A, which stays 1 when a hit
// raises the entry's level: the flag bytes of lssp_amd_iluk_refactor's pattern
// rule need it).  Columns are found through ilut_dev.h's open-addressing table
// of 4 cap slots.
//
// The level rule is the reference's: a hit on a column already present RAISES
// its level (pc-iluk.cxx:100-102, if (levls[ip] < it) levls[ip] = it) -- it does
// not lower it as textbook ILU(k) does, and that changes the pattern.
#pragma once

#include <cstdint>

#include "ilut_dev.h"

namespace lssp_amd {

constexpr int ILUK_LEVEL_MAX = 254;            // levels travel as bytes
constexpr unsigned ILUK_ORIGIN = 0x80000000u;  // staged column word: bit 31 = an entry of A

struct IlukRow {
    int *jw;            // [2 cap] columns
    unsigned char *lv;  // [2 cap] levels of fill
    unsigned char *og;  // [2 cap] origin bits
    int *hk;            // [4 cap] table keys (columns), -1 = empty
    int *hv;            // [4 cap] table values (positions)
    int cap;            // a power of two
};

BILU_HD inline int iluk_row_words(int cap) { return 2 * cap; }
// the columns and the table, as ilut_dev.h's steps take them (no values)
BILU_HD inline IlutRow iluk_table(const IlukRow &R) { return IlutRow{R.jw, nullptr, R.hk, R.hv, R.cap}; }
BILU_HD inline int iluk_upos(const IlukRow &R, int u) { return R.cap + u; }

BILU_HD inline void iluk_clear_lane(const IlukRow &R, int lane) { ilut_clear_lane(iluk_table(R), lane); }

// ---- row setup -----------------------------------------------------------------
// the lane's off-diagonal entry of A's row goes to position at (the caller's
// ordered count of the entries of its part before it): level 0, origin 1
BILU_HD inline void iluk_load_lane(const IlukRow &R, int col, int at)
{
    R.jw[at] = col;
    R.lv[at] = 0;
    R.og[at] = 1;
    ilut_table_put(iluk_table(R), col, at);
}

// ---- the selection step (pc-iluk.cxx:60-80) ----------------------------------------
// the lane's share of min jw[j .. nl): (column << 32) | position; INT64_MAX when the lane has none
BILU_HD inline long long iluk_min_lane(const IlukRow &R, int j, int nl, int lane)
{
    return ilut_min_lane(iluk_table(R), j, nl, lane);
}

// one lane: the minimum (at position at) goes to position j, level and origin with it
BILU_HD inline void iluk_swap(const IlukRow &R, int j, int at)
{
    if (at == j) return;
    const int col = R.jw[j];
    R.jw[j] = R.jw[at];
    R.jw[at] = col;
    const unsigned char l = R.lv[j], o = R.og[j];
    R.lv[j] = R.lv[at];
    R.og[j] = R.og[at];
    R.lv[at] = l;
    R.og[at] = o;
    R.hv[ilut_table_slot(iluk_table(R), col)] = at;  // (the minimum's own entry is never looked up again)
}

// ---- the merge (pc-iluk.cxx:82-103) --------------------------------------------------
// the level a column of pivot row k's U part (level ulev there) would enter with, plev = the pivot's level
BILU_HD inline int iluk_it(int ulev, int plev) { return ulev + plev + 1; }

// the column's position in the working row, -1 = absent
BILU_HD inline int iluk_lookup_lane(const IlukRow &R, int col)
{
    const int s = ilut_table_slot(iluk_table(R), col);
    return s < 0 ? -1 : R.hv[s];
}

// the lane's admitted hit (it <= level, col != i): the level of a present column
// (q >= 0) is raised to it, an absent one is appended at position at -- the
// caller's ordered count by ballot and prefix, on its side -- with origin 0.  The
// columns of one pivot row are distinct, so no two lanes share a position.
BILU_HD inline void iluk_merge_lane(const IlukRow &R, int col, int it, int q, int at)
{
    if (q >= 0) {
        if ((int)R.lv[q] < it) R.lv[q] = (unsigned char)it;
        return;
    }
    R.jw[at] = col;
    R.lv[at] = (unsigned char)it;
    R.og[at] = 0;
    ilut_table_put(iluk_table(R), col, at);
}

// ---- staging and pack -------------------------------------------------------------
// a finished row's parts wait in per-row staging areas of stride entries each
BILU_HD inline long long iluk_stage_off(int i, int stride) { return (long long)i * stride; }
BILU_HD inline unsigned iluk_stage_word(int col, int origin) { return (unsigned)col | (origin ? ILUK_ORIGIN : 0u); }
BILU_HD inline int iluk_stage_col(unsigned w) { return (int)(w & ~ILUK_ORIGIN); }
BILU_HD inline unsigned char iluk_stage_origin(unsigned w) { return (w & ILUK_ORIGIN) ? 1 : 0; }
// entries of F's row: the L part, the diagonal, the U part
BILU_HD inline int iluk_count(int lcnt, int ucnt) { return lcnt + 1 + ucnt; }
// the place of entry e among the m staged words of a U part once sorted by
// column (the columns are distinct): how many are smaller.  The L part leaves
// the selection step sorted already.
BILU_HD inline int iluk_rank(const unsigned *w, int m, int e)
{
    const int col = iluk_stage_col(w[e]);
    int r = 0;
    for (int k = 0; k < m; k++) r += iluk_stage_col(w[k]) < col;
    return r;
}

}  // namespace lssp_amd
