// ilut_dev_check.cpp -- the row body of lssp_amd_ilut_create_dev's kernel on the
// host (no GPU, no HIP): the lane-level steps of lssp_amd/csrc/ilut_dev.h, run by
// a plain loop over 64 lanes between the kernel's wave-level synchronisation
// points (k_ilut, ilut_factor.hip, has the same sequence), row after row, on
// exactly-sized heap arrays, so a sanitizer sees any access outside them:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ilssp_amd/csrc tools/ilut_dev_check.cpp -o /tmp/ilut_dev_check && /tmp/ilut_dev_check IN OUT
// IN  (binary): int32 n, nnz, p, cap; double tol; Ap[n + 1], Aj[nnz] (int32), Ax[nnz] (double);
//               the rows sorted, each with its diagonal; p <= 0: ceil(nnz / n); cap a power of two
// OUT (binary): int32 nnzL, nnzU; Lp[n + 1], Lj, Lx, Up[n + 1], Uj, Ux
// Exit status 0: factored; 3: a working row exceeded cap entries on a side; 2: bad input.
// tests/test_ilut_create_dev_cpu.py compares OUT with the oracle's ILUT bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "ilut_dev.h"

using namespace lssp_amd;

namespace {

template <typename T>
bool rd(FILE *f, T *p, size_t n)
{
    return n == 0 || fread(p, sizeof(T), n, f) == n;
}

struct Wave {  // what the kernel keeps in registers: one value per lane
    int col[ILUT_LANES], q[ILUT_LANES], at[ILUT_LANES];
    double v[ILUT_LANES];
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
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[4];
    double tol;
    if (!rd(f, hd, 4) || !rd(f, &tol, 1)) return 2;
    const int n = hd[0], nnz = hd[1], cap = hd[3];
    int p = hd[2];
    if (n < 1 || nnz < n || cap < 1 || (cap & (cap - 1))) return 2;
    std::unique_ptr<int[]> Ap(new int[n + 1]), Aj(new int[nnz]);
    std::unique_ptr<double[]> Ax(new double[nnz]);
    if (!rd(f, Ap.get(), n + 1) || !rd(f, Aj.get(), nnz) || !rd(f, Ax.get(), nnz)) return 2;
    fclose(f);
    if (tol < 0) tol = 1e-3;
    if (p <= 0) p = (nnz + n - 1) / n;  // pc-ilut.cxx:436-438

    // the working row, the table, the staging areas and the hand-off words: the kernel's sizes
    const int keep = ilut_keep(p, n, cap);
    std::unique_ptr<int[]> jw(new int[ilut_row_words(cap)]), hk(new int[ilut_table_slots(cap)]),
        hv(new int[ilut_table_slots(cap)]);
    std::unique_ptr<double[]> w(new double[ilut_row_words(cap)]);
    const IlutRow R{jw.get(), w.get(), hk.get(), hv.get(), cap};
    const size_t st = (size_t)ilut_stage_off(n, keep);
    std::unique_ptr<int[]> sLj(new int[st]), sUj(new int[st]), lcnt(new int[n]), ucnt(new int[n]);
    std::unique_ptr<double[]> sLx(new double[st]), sUx(new double[st]), diag(new double[n]);
    Wave W;
    bool flag[ILUT_LANES];

    const int len0 = Ap[1] - Ap[0];
    diag[0] = ilut_guard(Ax[Ap[0]]);
    lcnt[0] = ucnt[0] = 0;
    for (int i = 1; i < n; i++) {
        const int b = Ap[i], e = Ap[i + 1];
        for (int lane = 0; lane < ILUT_LANES; lane++) ilut_clear_lane(R, lane);
        const double rel = tol * ilut_row_norm(Ax.get(), b, e);
        int nl = 0, nu = 0;
        for (int c = b; c < e; c += ILUT_LANES) {
            for (int lane = 0; lane < ILUT_LANES; lane++) {
                W.valid[lane] = c + lane < e;
                W.col[lane] = W.valid[lane] ? Aj[c + lane] : 0;
                W.v[lane] = W.valid[lane] ? Ax[c + lane] : 0.0;
            }
            for (int lane = 0; lane < ILUT_LANES; lane++) flag[lane] = W.valid[lane] && W.col[lane] < i;
            const int tl = ordered(flag, nl, W.at);
            for (int lane = 0; lane < ILUT_LANES; lane++) flag[lane] = W.valid[lane] && W.col[lane] > i;
            const int tu = ordered(flag, ilut_upos(R, nu), W.at);
            if (nl + tl > cap || nu + tu > cap) return 3;
            for (int lane = 0; lane < ILUT_LANES; lane++)
                if (W.valid[lane]) ilut_load_lane(R, i, W.col[lane], W.v[lane], W.at[lane]);
            nl += tl;
            nu += tu;
        }
        for (int j = 0; j < nl; j++) {
            long long best = INT64_MAX;
            for (int lane = 0; lane < ILUT_LANES; lane++) {
                const long long m = ilut_min_lane(R, j, nl, lane);
                if (m < best) best = m;
            }
            const int jrow = (int)(best >> 32), at = (int)(best & 0xffffffffll);
            ilut_swap(R, j, at);
            const double aik = R.w[j] / diag[jrow];  // (the kernel waits here for row jrow)
            R.w[j] = aik;
            const int cnt = jrow ? ucnt[jrow] : len0;
            const int *pj = jrow ? sUj.get() + ilut_stage_off(jrow, keep) : Aj.get() + Ap[0];
            const double *px = jrow ? sUx.get() + ilut_stage_off(jrow, keep) : Ax.get() + Ap[0];
            for (int c = 0; c < cnt; c += ILUT_LANES) {
                for (int lane = 0; lane < ILUT_LANES; lane++) {
                    W.valid[lane] = c + lane < cnt;
                    W.col[lane] = W.valid[lane] ? pj[c + lane] : 0;
                    if (W.valid[lane] && W.col[lane] <= jrow) W.valid[lane] = false;  // row 0 of A: its diagonal
                    W.v[lane] = W.valid[lane] ? ilut_mx(aik, px[c + lane]) : 0.0;
                    W.q[lane] = W.valid[lane] ? ilut_lookup_lane(R, i, W.col[lane]) : -1;
                    if (W.valid[lane] && !ilut_kept(W.q[lane], W.v[lane], rel)) W.valid[lane] = false;
                    W.fresh[lane] = W.valid[lane] && W.q[lane] == -1;
                }
                for (int lane = 0; lane < ILUT_LANES; lane++) flag[lane] = W.fresh[lane] && W.col[lane] < i;
                const int tl = ordered(flag, nl, W.at);
                for (int lane = 0; lane < ILUT_LANES; lane++) flag[lane] = W.fresh[lane] && W.col[lane] > i;
                const int tu = ordered(flag, ilut_upos(R, nu), W.at);
                if (nl + tl > cap || nu + tu > cap) return 3;
                for (int lane = 0; lane < ILUT_LANES; lane++)
                    if (W.valid[lane]) ilut_update_lane(R, W.col[lane], W.v[lane], W.q[lane], W.at[lane]);
                nl += tl;
                nu += tu;
            }
        }
        diag[i] = ilut_guard(R.w[ilut_dpos(R)]);
        const int ku = nu < p ? nu : p, kl = nl < p ? nl : p;
        if (ku > keep || kl > keep) return 2;  // ilut_keep's bound
        ilut_qsplit(R.w + ilut_upos(R, 0), R.jw + ilut_upos(R, 0), nu, ku);
        for (int lane = 0; lane < ILUT_LANES; lane++)
            for (int k = lane; k < ku; k += ILUT_LANES) {
                sUj[ilut_stage_off(i, keep) + k] = R.jw[ilut_upos(R, k)];
                sUx[ilut_stage_off(i, keep) + k] = R.w[ilut_upos(R, k)];
            }
        ucnt[i] = ku;
        ilut_qsplit(R.w, R.jw, nl, kl);
        for (int lane = 0; lane < ILUT_LANES; lane++)
            for (int k = lane; k < kl; k += ILUT_LANES) {
                sLj[ilut_stage_off(i, keep) + k] = R.jw[k];
                sLx[ilut_stage_off(i, keep) + k] = R.w[k];
            }
        lcnt[i] = kl;
    }

    // compaction: counts, exclusive scan, pack
    std::unique_ptr<int[]> Lp(new int[n + 1]), Up(new int[n + 1]);
    Lp[0] = Up[0] = 0;
    for (int i = 0; i < n; i++) {
        Lp[i + 1] = Lp[i] + ilut_count_l(i, lcnt[i]);
        Up[i + 1] = Up[i] + ilut_count_u(i, ucnt[i], len0);
    }
    const int nnzL = Lp[n], nnzU = Up[n];
    std::unique_ptr<int[]> Lj(new int[nnzL]), Uj(new int[nnzU]);
    std::unique_ptr<double[]> Lx(new double[nnzL]), Ux(new double[nnzU]);
    for (int i = 0; i < n; i++) {
        int o = Lp[i];
        for (int k = 0; i > 0 && k < lcnt[i]; k++, o++) {
            Lj[o] = sLj[ilut_stage_off(i, keep) + k];
            Lx[o] = sLx[ilut_stage_off(i, keep) + k];
        }
        Lj[o] = i;
        Lx[o] = 1.0;
        o = Up[i];
        if (i == 0) {
            for (int k = 0; k < len0; k++, o++) {
                Uj[o] = Aj[Ap[0] + k];
                Ux[o] = Ax[Ap[0] + k];
            }
            continue;
        }
        Uj[o] = i;
        Ux[o++] = diag[i];
        for (int k = 0; k < ucnt[i]; k++, o++) {
            Uj[o] = sUj[ilut_stage_off(i, keep) + k];
            Ux[o] = sUx[ilut_stage_off(i, keep) + k];
        }
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const int cnts[2] = {nnzL, nnzU};
    fwrite(cnts, sizeof(int), 2, f);
    fwrite(Lp.get(), sizeof(int), n + 1, f);
    fwrite(Lj.get(), sizeof(int), nnzL, f);
    fwrite(Lx.get(), sizeof(double), nnzL, f);
    fwrite(Up.get(), sizeof(int), n + 1, f);
    fwrite(Uj.get(), sizeof(int), nnzU, f);
    fwrite(Ux.get(), sizeof(double), nnzU, f);
    fclose(f);
    printf("ok: n %d nnzL %d nnzU %d keep %d cap %d\n", n, nnzL, nnzU, keep, cap);
    return 0;
}
