// sched_dev.h -- the lane-level bodies of the device schedule builder
// (tri_sched.hip): the packet schedule of k_tri_pk6 built from a
// triangular factor that lives in HBM, byte for byte what build_bp_schedule and
// build_packets6 (tri_bp.cpp, sched_host.h) build on the host.  Each kernel runs
// a body on its lanes and joins them at its wave-level points (ballots,
// shuffles); tools/sched_dev_check.cpp runs the same bodies as plain loops over
// 64 lanes between the same points, on exactly-sized heap arrays under a
// sanitizer, and compares every array with the host reference.
//
// No HIP header is needed on the host: the memory accesses that hand a word from
// one wave to another (the level words) go through a loader / storer the caller
// passes in.
#pragma once

#include <cstdint>

#include "bilu_dev.h"  // BILU_HD

namespace lssp_amd {

constexpr int BP_RING = 4096;  // LDS ring of recently computed values (32 KB)
constexpr int PK3_ROWS = 256;    // v6: rows per packet = compute lanes = loader lanes
constexpr int PK3_EXT = 4;       // v6: HBM x operands per packet row, at most (on average; the kernel
                                 // runs 2, 3 or 4 loads per lane, TriSched::pk6_ext; 2 before round 6)
constexpr int PK3_CAP = 4096;    // v6: packets per block (descriptors staged in LDS)
constexpr long PK6_REC_WORDS16 = 1024;  // 16-byte units of the LDS record slot (trisolve.hip PK6_REC16)
constexpr int PK6_MAXLEN = 24;   // strict entries of a row, at most (the longest record)
// k_tri_pk6's LDS operand array: the value ring [0, BP_RING), a +0.0 pad slot
// at BP_RING, then the two buffers of landed HBM operands (PK3_EXT per packet
// row of 256).  Byte offset of entry base + par * buffer + k:
constexpr int pk6_xs_off(int base, int par, int k) { return 8 * (base + par * 256 * PK3_EXT + k); }

constexpr int SCHED_LANES = 64;
// what the check pass reports (bits of its flag word)
constexpr int SCHED_BAD = 1;       // a row without a diagonal slot, a column on the wrong side or outside [0, n)
constexpr int SCHED_NONUNIT = 2;   // a diagonal that is not exactly 1.0

struct alignas(16) SchedU4 {
    uint32_t x, y, z, w;
};
struct alignas(16) SchedD2 {
    double x, y;
};

BILU_HD inline int sched_q(int n, bool upper, int r) { return upper ? n - 1 - r : r; }  // row <-> sweep position
BILU_HD inline int sched_strict_begin(const int *Tp, bool upper, int i) { return upper ? Tp[i] + 1 : Tp[i]; }
BILU_HD inline int sched_strict_end(const int *Tp, bool upper, int i) { return upper ? Tp[i + 1] : Tp[i + 1] - 1; }
// entry e of row i in summation order: ascending storage order for L, descending for U
BILU_HD inline int sched_entry(const int *Tp, bool upper, int i, int e) { return upper ? Tp[i + 1] - 1 - e : Tp[i] + e; }
BILU_HD inline int sched_ep(int maxlen) { return maxlen <= 4 ? 4 : maxlen <= 8 ? 8 : maxlen <= 16 ? 16 : 24; }
BILU_HD inline long sched_pad4(long w) { return (w + 3) & ~3L; }
// record words of a packet of nrow rows (C, V, D, ROW, each padded to 4 words)
BILU_HD inline long sched_rec_words(int EP, long nrow)
{
    return sched_pad4((long)(EP / 2) * nrow) + 2L * EP * nrow + sched_pad4(2 * nrow) + sched_pad4(nrow);
}
BILU_HD inline uint32_t sched_pack(int a, int b) { return (uint32_t)((a & 0xffff) | ((uint32_t)(b & 0xffff) << 16)); }

// ---- stage 1: one row of the check (tri_levels' rules) and the scalars ---------
// flags: SCHED_* bits; bw: max |i - j| over the strict entries (0: none);
// len: the strict entries.  A row whose range is not inside [0, nnz] is not read.
BILU_HD inline void sched_check_row(int n, int nnz, bool upper, const int *Tp, const int *Tj, const double *Tx, int i,
                                    int &flags, int &bw, int &len)
{
    flags = 0;
    bw = 0;
    len = 0;
    const int a = Tp[i], b = Tp[i + 1];
    if ((i == 0 && a != 0) || a < 0 || b > nnz || b - a < 1) {
        flags = SCHED_BAD;
        return;
    }
    len = b - a - 1;
    const int k0 = upper ? a + 1 : a, k1 = upper ? b : b - 1;
    for (int k = k0; k < k1; k++) {
        const int j = Tj[k];
        if (upper ? (j <= i || j >= n) : (j < 0 || j >= i)) {
            flags |= SCHED_BAD;
            continue;
        }
        const int d = upper ? j - i : i - j;
        bw = d > bw ? d : bw;
    }
    if (!((upper ? Tx[a] : Tx[b - 1]) == 1.0)) flags |= SCHED_NONUNIT;
}

// ---- stage 2: one try at a row's level ---------------------------------------
// lev[i] = max(lev[j] + 1) over the strict entries.  The level word is the flag:
// -1 until written.  (k, l) keep the row's progress between tries: entries
// before k are folded into l.  Returns true when the row is finished (l is its
// level); false when entry k's row has no level yet.
template <typename Load>
BILU_HD inline bool sched_level_try(const int *Tj, int kend, const int *lev, Load load, int &k, int &l)
{
    while (k < kend) {
        const int lj = load(lev + Tj[k]);
        if (lj < 0) return false;
        l = lj + 1 > l ? lj + 1 : l;
        k++;
    }
    return true;
}

// ---- stage 3: the sort key of sweep position q: (block, level), stable in q --
BILU_HD inline unsigned long long sched_key(long q, long B, int lev)
{
    return ((unsigned long long)(q / B) << 32) | (unsigned)lev;
}

// ---- stage 4: the operand code of one entry (tri_bp.cpp: "entries in summation
// order") -- an own-block producer whose position is within BP_RING of the end
// of the consumer's step: its ring slot, as -1 - slot; else the producer's row
BILU_HD inline int sched_code(int n, bool upper, long B, int b, int step_end, int j, const int *pos)
{
    const int bj = (int)(sched_q(n, upper, j) / B);
    if (bj == b) {
        const int pd = pos[j];
        if (step_end - pd <= BP_RING) return -1 - (int)((pd - (long)b * B) % BP_RING);
    }
    return j;
}

// ---- stage 5: the packet walk --------------------------------------------------
// A block's HBM operands are rows of its own block or of the block before
// (B >= the bandwidth), so the walk's stamps (the packet that last took a row as
// an operand) and slots (its place in that packet's operand list) cover 2 B
// sweep positions per block.  Index of operand row g in block b's window; < 0:
// outside it (cannot happen for a checked factor)
BILU_HD inline long sched_window(int n, bool upper, long B, int b, int g)
{
    const long w = (long)sched_q(n, upper, g) - ((long)b - 1) * B;
    return w >= 0 && w < 2 * B ? w : -1;
}
// lane e of a row's step: its operand (the code of entry e; -1: none, a ring
// operand or a lane past the row) and whether this packet has not taken it yet
BILU_HD inline void sched_walk_lane(int n, bool upper, long B, int b, const int *cols, int k0, int len, int lane,
                                    const int *stamp, int pid, int &g, long &w, bool &fresh, bool &bad)
{
    g = lane < len ? cols[k0 + lane] : -1;
    w = -1;
    fresh = false;
    if (g >= 0) {
        w = sched_window(n, upper, B, b, g);
        if (w < 0) bad = true;
        else fresh = stamp[w] != pid;
    }
}
// a packet may take one more row (it has nr): the LDS record slot of EP >= 16
BILU_HD inline bool sched_rec_fits(int EP, int nr) { return !(EP >= 16 && sched_rec_words(EP, nr + 1) > 4 * PK6_REC_WORDS16); }

// ---- stage 6: one row of a packet's record -----------------------------------
// w: the packet's record (4-byte words); cols: the row's codes after the final
// walk (< 0: ring slot -1 - code; >= 0: the operand's slot in the packet's
// list); C through pk6_xs_off, V pairs as 16-byte stores, D, ROW
BILU_HD inline void sched_fill_row(uint32_t *w, int EP, int nr, int r, int par, const int *cols, int k0, int len,
                                   const int *Tp, const double *Tx, bool upper, int i, bool unit)
{
    const long wc = sched_pad4((long)(EP / 2) * nr), wv = 2L * EP * nr, wd = sched_pad4(2L * nr);
    SchedD2 *V = reinterpret_cast<SchedD2 *>(w + wc);
    // entries 2 q and 2 q + 1: their values stored as one pair, their operand offsets packed in one word
    // (past the row's length: the +0.0 pad slot and 0.0); no per-lane arrays, so nothing spills
    auto pair = [&](int q) -> uint32_t {
        int cc[2];
        double vv[2];
        for (int h = 0; h < 2; h++) {
            const int e = 2 * q + h;
            cc[h] = pk6_xs_off(BP_RING, 0, 0);
            vv[h] = 0.0;
            if (e < len) {
                const int g = cols[k0 + e];
                cc[h] = g < 0 ? pk6_xs_off(-1 - g, 0, 0) : pk6_xs_off(BP_RING + 1, par, g);
                vv[h] = Tx[sched_entry(Tp, upper, i, e)];
            }
        }
        V[(long)q * nr + r] = SchedD2{vv[0], vv[1]};
        return sched_pack(cc[0], cc[1]);
    };
    if (EP == 4) {
        w[2L * r] = pair(0);
        w[2L * r + 1] = pair(1);
    } else {
        SchedU4 *C = reinterpret_cast<SchedU4 *>(w + (long)(EP / 2) * r);
        for (int q = 0; q < EP / 8; q++) {
            const uint32_t c0 = pair(4 * q), c1 = pair(4 * q + 1), c2 = pair(4 * q + 2), c3 = pair(4 * q + 3);
            C[q] = SchedU4{c0, c1, c2, c3};
        }
    }
    double *D = reinterpret_cast<double *>(w + wc + wv);
    D[r] = unit ? 1.0 : (upper ? Tx[Tp[i]] : Tx[Tp[i + 1] - 1]);
    w[wc + wv + wd + r] = (uint32_t)i;
}
// the zero words that pad C, D and ROW to whole 16-byte units (one lane per packet)
BILU_HD inline void sched_fill_pads(uint32_t *w, int EP, int nr)
{
    const long c = (long)(EP / 2) * nr, wc = sched_pad4(c), wv = 2L * EP * nr, wd = sched_pad4(2L * nr);
    for (long k = c; k < wc; k++) w[k] = 0u;
    for (long k = 2L * nr; k < wd; k++) w[wc + wv + k] = 0u;
    for (long k = nr; k < sched_pad4(nr); k++) w[wc + wv + wd + k] = 0u;
}

}  // namespace lssp_amd
