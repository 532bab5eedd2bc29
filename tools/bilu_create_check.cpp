// bilu_create_check.cpp -- the index arithmetic of lssp_amd_bilu_create_dev's own
// kernels on the host (no GPU, no HIP): the per-block-row bodies of k_bilu_graph
// and k_bilu_expand (lssp_amd/csrc/bilu_create_dev.h) against independent
// restatements -- a set per block row for the block graph, bilu_expand's row by
// row push_back order for the point factors -- on exactly-sized heap arrays, so a
// sanitizer sees any access outside them:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ilssp_amd/csrc tools/bilu_create_check.cpp -o /tmp/bilu_create_check && /tmp/bilu_create_check
// Covered: bs 1 .. 8; the level 0, 1 and 2 fill patterns of random block graphs
// (the pattern is passed in, as the kernels get it); patterns with empty lower
// or empty upper parts, a block diagonal alone, block rows without their
// diagonal block; the first and last block rows of each.  Exit status 0 and
// "ok: <checks>" when every case matches.
#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "bilu_create_dev.h"

using namespace lssp_amd;

static long checks = 0;
static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        checks++;                         \
        if (!(cond)) {                    \
            failures++;                   \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
        }                                 \
    } while (0)

struct Pattern {
    int nb;
    std::vector<int> Bp, Bj;
};

static Pattern from_rows(const std::vector<std::set<int>> &rows)
{
    Pattern P{(int)rows.size(), {0}, {}};
    for (const auto &r : rows) {
        P.Bj.insert(P.Bj.end(), r.begin(), r.end());
        P.Bp.push_back((int)P.Bj.size());
    }
    return P;
}

// kind 0: a random graph with its diagonal; 1: lower parts only; 2: upper parts only;
// 3: the block diagonal alone; 4: random, a quarter of the block rows without their diagonal block
static Pattern make_graph(std::mt19937 &g, int nb, int per, int kind)
{
    std::vector<std::set<int>> rows(nb);
    for (int i = 0; i < nb; i++) {
        if (kind != 4 || g() % 4) rows[i].insert(i);
        if (kind == 3) continue;
        for (int q = 0; q < per; q++) {
            const int j = (int)(g() % nb);
            if ((kind == 1 && j > i) || (kind == 2 && j < i) || (kind == 4 && j == i)) continue;
            rows[i].insert(j);
        }
        if (rows[i].empty()) rows[i].insert((i + 1) % nb);  // (no empty block row)
    }
    return from_rows(rows);
}

// the ILU(level) fill pattern of a graph that holds its diagonal (the textbook level rule; any
// pattern serves here: the kernels take theirs as an argument)
static Pattern fill_pattern(const Pattern &G, int level)
{
    std::vector<std::map<int, int>> lev(G.nb);
    for (int i = 0; i < G.nb; i++) {
        for (int k = G.Bp[i]; k < G.Bp[i + 1]; k++) lev[i][G.Bj[k]] = 0;
        for (auto it = lev[i].begin(); it != lev[i].end() && it->first < i; ++it) {
            const int k = it->first, lk = it->second;
            for (const auto &kj : lev[k]) {
                if (kj.first <= k) continue;
                const int l = lk + kj.second + 1;
                if (l > level) continue;
                auto at = lev[i].find(kj.first);
                if (at == lev[i].end()) lev[i][kj.first] = l;
                else at->second = std::min(at->second, l);
            }
        }
    }
    std::vector<std::set<int>> rows(G.nb);
    for (int i = 0; i < G.nb; i++)
        for (const auto &e : lev[i]) rows[i].insert(e.first);
    return from_rows(rows);
}

// k_bilu_graph's body: a scalar CSR with sorted rows and holes inside the blocks of P (every block
// keeps an entry), its block graph against a set per block row
static void check_graph(std::mt19937 &g, const Pattern &P, int bs)
{
    const int nb = P.nb, n = nb * bs;
    std::vector<int> Ap{0}, Aj;
    for (int i = 0; i < nb; i++) {
        std::vector<std::vector<int>> rows(bs);
        for (int k = P.Bp[i]; k < P.Bp[i + 1]; k++) {
            bool any = false;
            for (int r = 0; r < bs; r++)
                for (int c = 0; c < bs; c++)
                    if (g() % 3 == 0) {
                        rows[r].push_back(P.Bj[k] * bs + c);
                        any = true;
                    }
            if (!any) {  // the block's one entry, in a row of its own choice
                const int r = (int)(g() % bs);
                rows[r].push_back(P.Bj[k] * bs + (int)(g() % bs));
                std::sort(rows[r].begin(), rows[r].end());
            }
        }
        for (int r = 0; r < bs; r++) {
            Aj.insert(Aj.end(), rows[r].begin(), rows[r].end());
            Ap.push_back((int)Aj.size());
        }
    }
    CHECK((int)Ap.size() == n + 1, "graph: row count");
    std::vector<int> ApX(Ap), AjX(Aj);  // exactly sized
    std::vector<int> cnt(nb), Gp(nb + 1, 0);
    for (int i = 0; i < nb; i++) {
        int diag = -1;
        cnt[i] = bilu_graph_row(i, bs, ApX.data(), AjX.data(), nullptr, &diag);
        std::set<int> want;
        for (int k = Ap[i * bs]; k < Ap[(i + 1) * bs]; k++) want.insert(Aj[k] / bs);
        CHECK(cnt[i] == (int)want.size(), "graph: bs %d block row %d count %d, want %zu", bs, i, cnt[i], want.size());
        CHECK(diag == (int)want.count(i), "graph: bs %d block row %d diagonal flag %d", bs, i, diag);
        Gp[i + 1] = Gp[i] + cnt[i];
    }
    std::vector<int> Gj(Gp[nb], -1);
    for (int i = 0; i < nb; i++) {
        int diag = -1;
        const int m = bilu_graph_row(i, bs, ApX.data(), AjX.data(), Gj.data() + Gp[i], &diag);
        CHECK(m == cnt[i], "graph: bs %d block row %d fill pass count", bs, i);
    }
    CHECK(Gp == P.Bp && Gj == P.Bj, "graph: bs %d nb %d differs from the pattern the matrix was made on", bs, nb);
}

// k_bilu_expand's body against bilu_expand(.., scaled = true) restated row by row; lanes: the
// stride the kernel walks a block row with (64), or 1
static void check_expand(std::mt19937 &g, const Pattern &P, int bs, int lanes)
{
    const int nb = P.nb, n = nb * bs, bs2 = bs * bs;
    std::uniform_real_distribution<double> u(-1, 1);
    std::vector<double> Fx(P.Bj.size() * (size_t)bs2);
    for (double &v : Fx) v = g() % 5 ? u(g) : 0.0;  // zeros are kept
    std::vector<int> first(nb), bl(nb + 1, 0), bu(nb + 1, 0);
    for (int i = 0; i < nb; i++) {
        int k = P.Bp[i];
        while (k < P.Bp[i + 1] && P.Bj[k] < i) k++;
        first[i] = k;
        int nl = 0, nu = 0;
        for (int q = P.Bp[i]; q < P.Bp[i + 1]; q++) {
            nl += P.Bj[q] < i;
            nu += P.Bj[q] > i;
        }
        bl[i + 1] = bl[i] + nl;
        bu[i + 1] = bu[i] + nu;
    }
    for (int upper = 0; upper < 2; upper++) {
        std::vector<int> Wp{0}, Wj;
        std::vector<double> Wx;
        for (int i = 0; i < nb; i++)
            for (int r = 0; r < bs; r++) {
                if (upper) {
                    Wj.push_back(i * bs + r);
                    Wx.push_back(1.0);
                }
                for (int k = P.Bp[i]; k < P.Bp[i + 1]; k++)
                    if (upper ? P.Bj[k] > i : P.Bj[k] < i)
                        for (int c = 0; c < bs; c++) {
                            Wj.push_back(P.Bj[k] * bs + c);
                            Wx.push_back(Fx[(size_t)k * bs2 + c * bs + r]);
                        }
                if (!upper) {
                    Wj.push_back(i * bs + r);
                    Wx.push_back(1.0);
                }
                Wp.push_back((int)Wj.size());
            }
        std::vector<int> Tp(n + 1, -7), Tj(Wj.size(), -7);
        std::vector<double> Tx(Wx.size(), -7.0);
        const std::vector<int> &before = upper ? bu : bl;
        for (int i = 0; i < nb; i++)
            for (int lane = 0; lane < lanes; lane++)
                bilu_expand_blockrow(upper != 0, bs, nb, i, before[i], P.Bp.data(), P.Bj.data(), first.data(),
                                     Fx.data(), Tp.data(), Tj.data(), Tx.data(), lane, lanes);
        CHECK(Tp == Wp, "expand: bs %d nb %d %c row pointers", bs, nb, upper ? 'U' : 'L');
        CHECK(Tj == Wj, "expand: bs %d nb %d %c columns", bs, nb, upper ? 'U' : 'L');
        CHECK(Tx == Wx, "expand: bs %d nb %d %c values", bs, nb, upper ? 'U' : 'L');
        const BiluSpan s0 = bilu_expand_span(bs, 0, 0, upper ? bu[1] : bl[1]);
        CHECK(s0.base == 0 && s0.len == Wp[1], "expand: the first block row's span");
    }
}

int main()
{
    std::mt19937 g(20240611);
    for (int bs = 1; bs <= BILU_MAX_BS_DEV; bs++)
        for (int nb : {1, 2, 7, 40})
            for (int kind = 0; kind < 5; kind++) {
                const Pattern G = make_graph(g, nb, 3, kind);
                check_graph(g, G, bs);
                for (int level = 0; level <= (kind == 0 ? 2 : 0); level++) {
                    const Pattern T = level ? fill_pattern(G, level) : G;
                    if (level == 2 && nb == 40) CHECK(T.Bj.size() > G.Bj.size(), "no fill at level 2");
                    check_expand(g, T, bs, 64);
                    check_expand(g, T, bs, 1);
                }
            }
    // the 64-bit span: bs^2 * blocks past 2^31
    const BiluSpan s = bilu_expand_span(8, 1000000, 40000000LL, 3);
    CHECK(s.base == 64LL * 40000000LL + 8000000LL && s.len == 25, "span arithmetic");
    if (failures) {
        fprintf(stderr, "%d of %ld checks failed\n", failures, checks);
        return 1;
    }
    printf("ok: %ld checks\n", checks);
    return 0;
}
