// bilu_create_dev.h -- the per-block-row bodies of lssp_amd_bilu_create_dev's two
// own kernels: k_bilu_graph (the block graph of a scalar CSR)
// and k_bilu_expand (the factored blocks expanded to the point factors L and U),
// both in bilu_factor.hip.  They are plain host + device functions, as the
// refactor's bodies are (bilu_refactor_dev.h), so that their index arithmetic
// also runs on the host, under a sanitizer, against independent restatements on
// exactly-sized arrays (tools/bilu_create_check.cpp).
#pragma once

#include <climits>

#include "bilu_dev.h"

namespace lssp_amd {

// Block row i of the block graph of the CSR (Ap, Aj), bs <= BILU_MAX_BS_DEV
// scalar rows per block row: the distinct block columns c / bs of the rows
// i*bs .. i*bs + bs-1, ascending -- what bilu_pattern collects with a mark array
// and a sort.  Every row's columns ascend strictly (checked before), so this is
// a bs-way merge of the rows' c / bs with duplicates removed: head[r] is the
// block column at row r's cursor, the smallest head goes out, every row standing
// on it moves on.  out == nullptr: the count alone.  Returns the count;
// *has_diag = the row holds block column i.
// The loops over r run to the constant BILU_MAX_BS_DEV and are unrolled, so
// cur / end / head are registers on the device, not an indexed private array.
BILU_HD inline int bilu_graph_row(int i, int bs, const int *Ap, const int *Aj, int *out, int *has_diag)
{
    int cur[BILU_MAX_BS_DEV], end[BILU_MAX_BS_DEV], head[BILU_MAX_BS_DEV];
#pragma unroll
    for (int r = 0; r < BILU_MAX_BS_DEV; r++) {
        cur[r] = end[r] = 0;
        if (r < bs) {
            cur[r] = Ap[(long)i * bs + r];
            end[r] = Ap[(long)i * bs + r + 1];
        }
        head[r] = cur[r] < end[r] ? Aj[cur[r]] / bs : INT_MAX;
    }
    int cnt = 0, diag = 0;
    for (;;) {
        int best = INT_MAX;
#pragma unroll
        for (int r = 0; r < BILU_MAX_BS_DEV; r++) best = head[r] < best ? head[r] : best;
        if (best == INT_MAX) break;
        if (out) out[cnt] = best;
        cnt++;
        diag |= best == i;
#pragma unroll
        for (int r = 0; r < BILU_MAX_BS_DEV; r++)
            while (head[r] == best) {
                cur[r]++;
                head[r] = cur[r] < end[r] ? Aj[cur[r]] / bs : INT_MAX;
            }
    }
    *has_diag = diag;
    return cnt;
}

// Where block row i's rows of a point factor lie: its bs rows hold len entries
// each, one after the other from entry `base` on.  before = the strict blocks of
// that side in the block rows 0 .. i-1, mine = block row i's own:
//   len = bs * mine + 1, base = bs^2 * before + bs * i   (64-bit: bs^2 * blocks)
struct BiluSpan {
    long long base;
    int len;
};
BILU_HD inline BiluSpan bilu_expand_span(int bs, int i, long long before, int mine)
{
    return BiluSpan{(long long)bs * bs * before + (long long)bs * i, bs * mine + 1};
}

// Entries t0, t0 + step, .. of block row i's part of L (upper: of U), its bs rows'
// entries numbered through, t = r * len + e, exactly as bilu_expand(.., scaled =
// true) writes them from the committed block values Fx (blocks column-major,
// the blocks right of the diagonal scaled already):
//   L row i*bs + r: per strict-lower block k = Bp[i] .. first[i]-1 the columns
//     Bj[k]*bs .. Bj[k]*bs + bs-1 with Fx[k*bs^2 + c*bs + r], then the unit
//     diagonal LAST;
//   U row i*bs + r: the unit diagonal FIRST, then the same over the blocks right
//     of the diagonal block (first[i] is the diagonal block when the row holds
//     it, else already the first block to its right).
// Every entry of a block is kept, zeros included.  The entry whose e is 0 also
// writes the row's pointer Tp[row]; block row nb - 1's last row writes Tp[n].
// Consecutive t are consecutive entries of Tj / Tx: a wave that walks t with its
// lanes stores whole cache lines (the reads of a block are strided by bs).
BILU_HD inline void bilu_expand_blockrow(bool upper, int bs, int nb, int i, long long before, const int *Bp,
                                         const int *Bj, const int *first, const double *Fx, int *Tp, int *Tj,
                                         double *Tx, int t0, int step)
{
    const int f = first[i], end = Bp[i + 1];
    const int k0 = upper ? f + (f < end && Bj[f] == i ? 1 : 0) : Bp[i];
    const int mine = upper ? end - k0 : f - k0;
    const BiluSpan s = bilu_expand_span(bs, i, before, mine);
    const int bs2 = bs * bs, tot = bs * s.len;
    for (int t = t0; t < tot; t += step) {
        const int r = t / s.len, e = t - r * s.len;
        const int row = i * bs + r;
        const long long at = s.base + t;
        if (e == 0) Tp[row] = (int)at;
        if (e == 0 && i == nb - 1 && r == bs - 1) Tp[row + 1] = (int)(at + s.len);
        if (e == (upper ? 0 : s.len - 1)) {
            Tj[at] = row;
            Tx[at] = 1.0;
            continue;
        }
        const int q = upper ? e - 1 : e, kb = q / bs, c = q - kb * bs;
        const long long k = (long long)k0 + kb;
        Tj[at] = Bj[k] * bs + c;
        Tx[at] = Fx[k * bs2 + (long long)c * bs + r];
    }
}

}  // namespace lssp_amd
