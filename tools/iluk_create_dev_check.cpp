// iluk_create_dev_check.cpp -- the index arithmetic of lssp_amd_iluk_create_dev's
// kernels on the host (no GPU, no HIP): the per-row bodies of k_fill1_pattern and
// k_fill1_levels (lssp_amd/csrc/iluk_create_dev.h) run against independent
// restatements -- the symbolic ILU(1) of the box's 5-/7-point stencil by the
// generic level-of-fill rule (lev(i, j) = min over k of lev(i, k) + lev(k, j) + 1,
// entries of level <= 1 kept), and the longest-path levels of its strict-lower
// DAG, rows ascending inside a level -- on exactly-sized heap arrays, so a
// sanitizer sees any access outside them:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ilssp_amd/csrc tools/iluk_create_dev_check.cpp -o /tmp/iluk_create_dev_check && /tmp/iluk_create_dev_check
// Exit status 0 and "ok" when every case matches.
#include <algorithm>
#include <cstdio>
#include <map>
#include <memory>
#include <vector>

#include "iluk_create_dev.h"

using namespace lssp_amd;

static int failures = 0;
#define CHECK(cond, ...)              \
    do {                              \
        if (!(cond)) {                \
            if (failures++ < 20) {    \
                fprintf(stderr, __VA_ARGS__); \
                fprintf(stderr, "\n");    \
            }                         \
        }                             \
    } while (0)

struct Pattern {
    std::vector<int> p, j;
    std::vector<unsigned char> in;  // 1: an entry of the stencil, 0: fill
};

// the symbolic ILU(1) of the box's stencil, row by row (IKJ): row i starts as
// the stencil's row at level 0; for each k < i of the row, ascending (fill just
// added included), every (k, j), j > k, of the finished row k offers level
// lev(i, k) + lev(k, j) + 1
static Pattern symbolic_ilu1(int nx, int ny, int nz)
{
    const long pl = (long)nx * ny, n = pl * nz;
    std::vector<std::map<int, int>> rows((size_t)n);
    Pattern F;
    F.p.push_back(0);
    for (long r = 0; r < n; r++) {
        const int i = (int)(r % nx), j = (int)(r / nx % ny), k = (int)(r / pl);
        std::map<int, int> &row = rows[(size_t)r];
        std::map<int, int> stencil;
        if (k > 0) stencil[(int)(r - pl)] = 0;
        if (j > 0) stencil[(int)(r - nx)] = 0;
        if (i > 0) stencil[(int)(r - 1)] = 0;
        stencil[(int)r] = 0;
        if (i < nx - 1) stencil[(int)(r + 1)] = 0;
        if (j < ny - 1) stencil[(int)(r + nx)] = 0;
        if (k < nz - 1) stencil[(int)(r + pl)] = 0;
        row = stencil;
        for (auto it = row.begin(); it != row.end() && it->first < r; ++it) {
            const int kk = it->first, lik = it->second;
            for (const auto &e : rows[(size_t)kk]) {
                if (e.first <= kk) continue;
                const int lev = lik + e.second + 1;
                if (lev > 1) continue;
                auto f = row.find(e.first);
                if (f == row.end()) row[e.first] = lev;
                else f->second = std::min(f->second, lev);
            }
        }
        for (const auto &e : row) {
            F.j.push_back(e.first);
            F.in.push_back((unsigned char)(stencil.count(e.first) ? 1 : 0));
        }
        F.p.push_back((int)F.j.size());
    }
    return F;
}

static void check_box(int nx, int ny, int nz)
{
    const long n = (long)nx * ny * nz;
    const Pattern W = symbolic_ilu1(nx, ny, nz);
    const long fnnz = fill1_row_start(0, 0, nz, nx, ny, nz);
    CHECK(fnnz == (long)W.j.size(), "%dx%dx%d: %ld entries, the symbolic ILU(1) has %zu", nx, ny, nz, fnnz, W.j.size());
    if (fnnz != (long)W.j.size()) return;
    // the kernel's arrays, exactly sized
    std::unique_ptr<int[]> Fp(new int[n + 1]), Fj(new int[fnnz]), dpos(new int[n]);
    std::unique_ptr<unsigned char[]> fin(new unsigned char[fnnz]);
    std::fill(Fj.get(), Fj.get() + fnnz, -1);
    std::fill(fin.get(), fin.get() + fnnz, (unsigned char)9);
    for (long r = 0; r < n; r++) {  // k_fill1_pattern's row
        const int i = (int)(r % nx), j = (int)(r / nx % ny), k = (int)(r / ((long)nx * ny));
        const long s = fill1_row_start(i, j, k, nx, ny, nz);
        const int len = fill1_row_len(i, j, k, nx, ny, nz);
        CHECK(s == W.p[r] && len == W.p[r + 1] - W.p[r], "%dx%dx%d row %ld: start %ld length %d, want %d %d", nx, ny, nz,
              r, s, len, W.p[r], W.p[r + 1] - W.p[r]);
        if (s < 0 || s + len > fnnz) continue;
        int dp = -1;
        const int got = fill1_row(i, j, k, nx, ny, nz, Fj.get() + s, fin.get() + s, &dp);
        CHECK(got == len, "%dx%dx%d row %ld: wrote %d of %d", nx, ny, nz, r, got, len);
        Fp[r] = (int)s;
        dpos[r] = (int)s + dp;
        if (r == n - 1) Fp[n] = (int)(s + len);
    }
    for (long r = 0; r <= n; r++) CHECK(Fp[r] == W.p[r], "%dx%dx%d: Fp[%ld]", nx, ny, nz, r);
    for (long e = 0; e < fnnz; e++) {
        CHECK(Fj[e] == W.j[e], "%dx%dx%d: Fj[%ld] = %d, want %d", nx, ny, nz, e, Fj[e], W.j[e]);
        CHECK(fin[e] == W.in[e], "%dx%dx%d: fin[%ld] = %d, want %d", nx, ny, nz, e, fin[e], W.in[e]);
    }
    for (long r = 0; r < n; r++)
        CHECK(dpos[r] >= W.p[r] && dpos[r] < W.p[r + 1] && W.j[dpos[r]] == r, "%dx%dx%d: dpos[%ld]", nx, ny, nz, r);

    // longest-path levels of the strict-lower DAG, rows ascending inside a level
    std::vector<int> lev((size_t)n, 0);
    int nlev = 0;
    for (long r = 0; r < n; r++) {
        int l = 0;
        for (int e = W.p[r]; e < W.p[r + 1] && W.j[e] < r; e++) l = std::max(l, lev[W.j[e]] + 1);
        lev[r] = l;
        nlev = std::max(nlev, l + 1);
    }
    std::vector<int> woff((size_t)nlev + 1, 0), wrows((size_t)n);
    for (long r = 0; r < n; r++) woff[lev[r] + 1]++;
    for (int l = 0; l < nlev; l++) woff[l + 1] += woff[l];
    {
        std::vector<int> at(woff.begin(), woff.end() - 1);
        for (long r = 0; r < n; r++) wrows[at[lev[r]]++] = (int)r;
    }
    CHECK(nlev == fill1_nlev(nx, ny, nz), "%dx%dx%d: %d levels, closed form %d", nx, ny, nz, nlev, fill1_nlev(nx, ny, nz));
    if (nlev != fill1_nlev(nx, ny, nz)) return;
    std::unique_ptr<int[]> tab(new int[2 * nlev + 1]), rows(new int[n]);
    CHECK(fill1_level_tables(nx, ny, nz, tab.get()) == n, "%dx%dx%d: the level sizes do not add up to n", nx, ny, nz);
    for (int l = 0; l <= nlev; l++) CHECK(tab[nlev + l] == woff[l], "%dx%dx%d: lev_off[%d]", nx, ny, nz, l);
    std::fill(rows.get(), rows.get() + n, -1);
    for (long r = 0; r < n; r++) {  // k_fill1_levels' row
        const int i = (int)(r % nx), j = (int)(r / nx % ny), k = (int)(r / ((long)nx * ny));
        const long pos = fill1_level_pos(i, j, k, nx, tab.get(), tab.get() + nlev);
        CHECK(pos >= 0 && pos < n, "%dx%dx%d row %ld: position %ld", nx, ny, nz, r, pos);
        if (pos >= 0 && pos < n) rows[pos] = (int)r;
    }
    for (long q = 0; q < n; q++) CHECK(rows[q] == wrows[q], "%dx%dx%d: rows[%ld] = %d, want %d", nx, ny, nz, q, rows[q], wrows[q]);
}

int main()
{
    const int boxes[][3] = {{3, 3, 1}, {3, 3, 2}, {4, 3, 2}, {7, 3, 20}, {9, 21, 13}, {5, 300, 1}};
    for (const auto &b : boxes) check_box(b[0], b[1], b[2]);
    if (failures) {
        fprintf(stderr, "%d mismatches\n", failures);
        return 1;
    }
    printf("ok: %zu boxes, F rows, flags, diagonal positions and level lists match the symbolic ILU(1)\n",
           sizeof(boxes) / sizeof(boxes[0]));
    return 0;
}
