// iluk_symbolic_check.cpp -- the row body of lssp_amd_pc_create_dev's symbolic
// ILU(k) kernel on the host (no GPU, no HIP): the lane-level steps of
// lssp_amd/csrc/iluk_symbolic_dev.h, run by a plain loop over 64 lanes between
// the kernel's wave-level synchronisation points (k_iluk_symbolic and
// k_iluk_pack, iluk_symbolic.hip, have the same sequence), row after row, on
// exactly-sized heap arrays, so a sanitizer sees any access outside them:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ilssp_amd/csrc tools/iluk_symbolic_check.cpp -o /tmp/iluk_symbolic_check
//   /tmp/iluk_symbolic_check IN OUT LEVEL CAP
// IN  (binary): int32 n, nnz; Ap[n + 1], Aj[nnz] (int32); the rows sorted, each with its diagonal
// OUT (binary): int32 fnnz; Fp[n + 1], Fj[fnnz] (int32); fin[fnnz] (bytes: 1 = entry of A, 0 = fill);
//               dpos[n] (int32: the position of each row's diagonal in F)
// LEVEL: 0 .. 254; CAP: entries of the working row on each side of the diagonal, a power of two.
// Exit status 0: done; 3: a working row exceeded CAP entries on a side; 2: bad input.
// tests/test_pc_create_dev_cpu.py compares OUT with the oracle's ILUK pattern.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "iluk_symbolic_dev.h"

using namespace lssp_amd;

namespace {

template <typename T>
bool rd(FILE *f, T *p, size_t n)
{
    return n == 0 || fread(p, sizeof(T), n, f) == n;
}

struct Wave {  // what the kernel keeps in registers: one value per lane
    int col[ILUT_LANES], it[ILUT_LANES], q[ILUT_LANES], at[ILUT_LANES];
    bool valid[ILUT_LANES], fresh[ILUT_LANES];
};

// ballot + prefix on one side: at[lane] = base + the flagged lanes below; returns the flagged count
int ordered(const bool *flag, int base, int *at)
{
    int cnt = 0;
    for (int lane = 0; lane < ILUT_LANES; lane++)
        if (flag[lane]) at[lane] = base + cnt++;
    return cnt;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: %s IN OUT LEVEL CAP\n", argv[0]);
        return 2;
    }
    const int level = atoi(argv[3]), cap = atoi(argv[4]);
    if (level < 0 || level > ILUK_LEVEL_MAX || cap < 1 || (cap & (cap - 1))) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[2];
    if (!rd(f, hd, 2)) return 2;
    const int n = hd[0], nnz = hd[1];
    if (n < 1 || nnz < n) return 2;
    std::unique_ptr<int[]> Ap(new int[n + 1]), Aj(new int[nnz]);
    if (!rd(f, Ap.get(), n + 1) || !rd(f, Aj.get(), nnz)) return 2;
    fclose(f);

    // the working row, the table, the staging areas and the hand-off words: the kernel's sizes
    std::unique_ptr<int[]> jw(new int[iluk_row_words(cap)]), hk(new int[ilut_table_slots(cap)]),
        hv(new int[ilut_table_slots(cap)]);
    std::unique_ptr<unsigned char[]> lv(new unsigned char[iluk_row_words(cap)]),
        og(new unsigned char[iluk_row_words(cap)]);
    const IlukRow R{jw.get(), lv.get(), og.get(), hk.get(), hv.get(), cap};
    const int stride = cap;
    const size_t st = (size_t)iluk_stage_off(n, stride);
    std::unique_ptr<unsigned[]> sLj(new unsigned[st]), sUj(new unsigned[st]);
    std::unique_ptr<unsigned char[]> sUl(new unsigned char[st]);
    std::unique_ptr<int[]> lcnt(new int[n]), ucnt(new int[n]);
    Wave W;
    bool flag[ILUT_LANES];

    for (int i = 0; i < n; i++) {
        const int b = Ap[i], e = Ap[i + 1];
        for (int lane = 0; lane < ILUT_LANES; lane++) iluk_clear_lane(R, lane);
        int nl = 0, nu = 0;
        for (int c = b; c < e; c += ILUT_LANES) {
            for (int lane = 0; lane < ILUT_LANES; lane++) {
                W.valid[lane] = c + lane < e;
                W.col[lane] = W.valid[lane] ? Aj[c + lane] : i;
            }
            for (int lane = 0; lane < ILUT_LANES; lane++) flag[lane] = W.col[lane] < i;
            const int tl = ordered(flag, nl, W.at);
            for (int lane = 0; lane < ILUT_LANES; lane++) flag[lane] = W.col[lane] > i;
            const int tu = ordered(flag, iluk_upos(R, nu), W.at);
            if (nl + tl > cap || nu + tu > cap) return 3;
            for (int lane = 0; lane < ILUT_LANES; lane++)
                if (W.col[lane] != i) iluk_load_lane(R, W.col[lane], W.at[lane]);
            nl += tl;
            nu += tu;
        }
        for (int j = 0; j < nl; j++) {
            long long best = INT64_MAX;
            for (int lane = 0; lane < ILUT_LANES; lane++) {
                const long long m = iluk_min_lane(R, j, nl, lane);
                if (m < best) best = m;
            }
            const int k = (int)(best >> 32), at = (int)(best & 0xffffffffll);
            iluk_swap(R, j, at);
            const int cnt = ucnt[k];  // (the kernel waits here for row k)
            const int plev = R.lv[j];
            const unsigned *pj = sUj.get() + iluk_stage_off(k, stride);
            const unsigned char *pl = sUl.get() + iluk_stage_off(k, stride);
            for (int c = 0; c < cnt; c += ILUT_LANES) {
                for (int lane = 0; lane < ILUT_LANES; lane++) {
                    W.valid[lane] = c + lane < cnt;
                    W.col[lane] = W.valid[lane] ? iluk_stage_col(pj[c + lane]) : 0;
                    W.it[lane] = W.valid[lane] ? iluk_it(pl[c + lane], plev) : 0;
                    if (W.it[lane] > level || W.col[lane] == i) W.valid[lane] = false;
                    W.q[lane] = W.valid[lane] ? iluk_lookup_lane(R, W.col[lane]) : -1;
                    W.fresh[lane] = W.valid[lane] && W.q[lane] == -1;
                }
                for (int lane = 0; lane < ILUT_LANES; lane++) flag[lane] = W.fresh[lane] && W.col[lane] < i;
                const int tl = ordered(flag, nl, W.at);
                for (int lane = 0; lane < ILUT_LANES; lane++) flag[lane] = W.fresh[lane] && W.col[lane] > i;
                const int tu = ordered(flag, iluk_upos(R, nu), W.at);
                if (nl + tl > cap || nu + tu > cap) return 3;
                for (int lane = 0; lane < ILUT_LANES; lane++)
                    if (W.valid[lane]) iluk_merge_lane(R, W.col[lane], W.it[lane], W.q[lane], W.at[lane]);
                nl += tl;
                nu += tu;
            }
        }
        for (int lane = 0; lane < ILUT_LANES; lane++)
            for (int k = lane; k < nu; k += ILUT_LANES) {
                sUj[iluk_stage_off(i, stride) + k] = iluk_stage_word(R.jw[iluk_upos(R, k)], R.og[iluk_upos(R, k)]);
                sUl[iluk_stage_off(i, stride) + k] = R.lv[iluk_upos(R, k)];
            }
        ucnt[i] = nu;
        for (int lane = 0; lane < ILUT_LANES; lane++)
            for (int k = lane; k < nl; k += ILUT_LANES)
                sLj[iluk_stage_off(i, stride) + k] = iluk_stage_word(R.jw[k], R.og[k]);
        lcnt[i] = nl;
    }

    // compaction: counts, exclusive scan, pack (the U part sorted by rank)
    std::unique_ptr<int[]> Fp(new int[n + 1]), dpos(new int[n]);
    long long total = 0;
    for (int i = 0; i < n; i++) total += iluk_count(lcnt[i], ucnt[i]);
    if (total > 0x7fffffffLL) return 2;
    Fp[0] = 0;
    for (int i = 0; i < n; i++) Fp[i + 1] = Fp[i] + iluk_count(lcnt[i], ucnt[i]);
    const int fnnz = Fp[n];
    std::unique_ptr<int[]> Fj(new int[fnnz]);
    std::unique_ptr<unsigned char[]> fin(new unsigned char[fnnz]);
    std::unique_ptr<unsigned[]> srt(new unsigned[cap]);  // the pack's LDS copy of a U part
    for (int i = 0; i < n; i++) {
        const int nl = lcnt[i], nu = ucnt[i], o = Fp[i];
        const long long off = iluk_stage_off(i, stride);
        for (int k = 0; k < nl; k++) {
            Fj[o + k] = iluk_stage_col(sLj[off + k]);
            fin[o + k] = iluk_stage_origin(sLj[off + k]);
        }
        Fj[o + nl] = i;
        fin[o + nl] = 1;
        dpos[i] = o + nl;
        for (int k = 0; k < nu; k++) srt[k] = sUj[off + k];
        for (int lane = 0; lane < ILUT_LANES; lane++)
            for (int k = lane; k < nu; k += ILUT_LANES) {
                const int r = iluk_rank(srt.get(), nu, k);
                Fj[o + nl + 1 + r] = iluk_stage_col(srt[k]);
                fin[o + nl + 1 + r] = iluk_stage_origin(srt[k]);
            }
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(&fnnz, sizeof(int), 1, f);
    fwrite(Fp.get(), sizeof(int), n + 1, f);
    fwrite(Fj.get(), sizeof(int), fnnz, f);
    fwrite(fin.get(), 1, fnnz, f);
    fwrite(dpos.get(), sizeof(int), n, f);
    fclose(f);
    printf("ok: n %d fnnz %d level %d cap %d\n", n, fnnz, level, cap);
    return 0;
}
