// bilu_refill_check.cpp -- the index arithmetic of lssp_amd_bilu_refactor's
// kernels on the host (no GPU, no HIP): the per-row bodies k_bilu_scatter and
// k_pk6_refill run (lssp_amd/csrc/bilu_refactor_dev.h) against independent
// restatements of bilu_pattern's placement and build_packets6's value placement,
// on exactly-sized heap arrays, so a sanitizer sees any access outside them:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ilssp_amd/csrc tools/bilu_refill_check.cpp -o /tmp/bilu_refill_check && /tmp/bilu_refill_check
// Exit status 0 and "ok" when every case matches.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "bilu_refactor_dev.h"

using namespace lssp_amd;

static int failures = 0;
#define CHECK(cond, ...)              \
    do {                              \
        if (!(cond)) {                \
            failures++;               \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");    \
        }                             \
    } while (0)

struct Pattern {
    int nb, bs;
    std::vector<int> Bp, Bj, first;
};

// a random block pattern: about per blocks a row, sorted; diag: every row holds its diagonal block
static Pattern make_pattern(std::mt19937 &g, int nb, int bs, int per, bool diag)
{
    Pattern P{nb, bs, {0}, {}, {}};
    for (int i = 0; i < nb; i++) {
        std::vector<int> row;
        if (diag || g() % 4) row.push_back(i);
        for (int q = 0; q < per; q++) row.push_back((int)(g() % nb));
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end()), row.end());
        P.Bj.insert(P.Bj.end(), row.begin(), row.end());
        P.Bp.push_back((int)P.Bj.size());
    }
    for (int i = 0; i < nb; i++) {
        int k = P.Bp[i];
        while (k < P.Bp[i + 1] && P.Bj[k] < i) k++;
        P.first.push_back(k);
    }
    return P;
}

// k_bilu_scatter's body against a map-based placement; also the refusals
static void check_scatter(std::mt19937 &g, const Pattern &P)
{
    const int bs = P.bs, bs2 = bs * bs, n = P.nb * bs;
    std::uniform_real_distribution<double> u(-1, 1);
    std::vector<int> Ap{0}, Aj;
    std::vector<double> Ax;
    for (int r = 0; r < n; r++) {
        const int i = r / bs;
        for (int k = P.Bp[i]; k < P.Bp[i + 1]; k++)
            for (int c = 0; c < bs; c++)
                if (g() % 8) {  // holes inside blocks
                    Aj.push_back(P.Bj[k] * bs + c);
                    Ax.push_back(u(g));
                }
        if (Aj.size() > (size_t)Ap.back() && g() % 2) {  // a duplicated column: the last one wins
            Aj.push_back(Aj[Ap.back() + g() % (Aj.size() - Ap.back())]);
            Ax.push_back(u(g));
        }
        // shuffle the row's entries (a permutation applied to both arrays)
        for (long a = (long)Aj.size() - 1; a > (long)Ap.back(); a--) {
            const long b = Ap.back() + (long)(g() % (unsigned long)(a - Ap.back() + 1));
            std::swap(Aj[a], Aj[b]);
            std::swap(Ax[a], Ax[b]);
        }
        Ap.push_back((int)Aj.size());
    }
    const int nnz = (int)Aj.size();
    const size_t nblk = P.Bj.size();
    std::vector<double> want(nblk * bs2, 0.0), got(nblk * bs2, 0.0);
    std::vector<unsigned char> hit(nblk, 0), hit_want(nblk, 0);
    for (int r = 0; r < n; r++)
        for (int k = Ap[r]; k < Ap[r + 1]; k++) {
            const int i = r / bs, cb = Aj[k] / bs;
            int at = -1;
            for (int q = P.Bp[i]; q < P.Bp[i + 1]; q++)
                if (P.Bj[q] == cb) at = q;
            want[(size_t)at * bs2 + (Aj[k] % bs) * bs + r % bs] = Ax[k];
            hit_want[at] = 1;
        }
    int bad = 0;
    for (int r = 0; r < n; r++)
        bad |= bilu_scatter_row(r, n, bs, nnz, Ap.data(), Aj.data(), Ax.data(), P.Bp.data(), P.Bj.data(), got.data(),
                                hit.data());
    CHECK(!bad, "scatter: a valid matrix was flagged (nb %d bs %d)", P.nb, bs);
    CHECK(!memcmp(want.data(), got.data(), sizeof(double) * want.size()), "scatter: values differ (nb %d bs %d)", P.nb, bs);
    CHECK(hit == hit_want, "scatter: hit marks differ (nb %d bs %d)", P.nb, bs);
    // refusals: nothing outside the arrays may be touched (the sanitizer's part), and the row is reported
    if (nnz > 0) {
        std::vector<int> Bj2 = Aj;
        const int k = (int)(g() % nnz);
        for (int v : {-1, n, n + 7, 1 << 30, -(1 << 30)}) {
            Bj2[k] = v;
            int b2 = 0;
            for (int r = 0; r < n; r++)
                b2 |= bilu_scatter_row(r, n, bs, nnz, Ap.data(), Bj2.data(), Ax.data(), P.Bp.data(), P.Bj.data(),
                                       got.data(), hit.data());
            CHECK(b2, "scatter: column %d not flagged", v);
        }
        std::vector<int> Ap2 = Ap;
        Ap2[n] = nnz + 5;
        CHECK(bilu_scatter_row(n - 1, n, bs, nnz, Ap2.data(), Aj.data(), Ax.data(), P.Bp.data(), P.Bj.data(), got.data(),
                               hit.data()),
              "scatter: a row range past nnz not flagged");
        Ap2[0] = -3;
        CHECK(bilu_scatter_row(0, n, bs, nnz, Ap2.data(), Aj.data(), Ax.data(), P.Bp.data(), P.Bj.data(), got.data(),
                               hit.data()),
              "scatter: a negative row range not flagged");
        // an entry in a block the pattern lacks
        for (int i = 0; i < P.nb; i++) {
            std::vector<char> has(P.nb, 0);
            for (int q = P.Bp[i]; q < P.Bp[i + 1]; q++) has[P.Bj[q]] = 1;
            int miss = -1;
            for (int j = 0; j < P.nb; j++)
                if (!has[j]) miss = j;
            if (miss < 0 || Ap[i * bs] == Ap[i * bs + 1]) continue;
            Bj2 = Aj;
            Bj2[Ap[i * bs]] = miss * bs;
            CHECK(bilu_scatter_row(i * bs, n, bs, nnz, Ap.data(), Bj2.data(), Ax.data(), P.Bp.data(), P.Bj.data(),
                                   got.data(), hit.data()),
                  "scatter: an entry of an absent block not flagged");
            break;
        }
    }
}

// k_pk6_refill's body against build_packets6's placement of bilu_expand's rows
static void check_refill(std::mt19937 &g, const Pattern &P, bool upper)
{
    const int bs = P.bs, bs2 = bs * bs, n = P.nb * bs;
    std::uniform_real_distribution<double> u(-1, 1);
    std::vector<double> Fx(P.Bj.size() * bs2);
    for (double &v : Fx) v = u(g);
    // each row's strict entries in the sweep's summation order (bilu_expand + build_bp_schedule)
    std::vector<std::vector<double>> ent(n);
    int maxlen = 0;
    for (int row = 0; row < n; row++) {
        const int i = row / bs, rr = row % bs;
        std::vector<double> &e = ent[row];
        for (int k = P.Bp[i]; k < P.Bp[i + 1]; k++)
            if (upper ? P.Bj[k] > i : P.Bj[k] < i)
                for (int c = 0; c < bs; c++) e.push_back(Fx[(size_t)k * bs2 + c * bs + rr]);
        if (upper) std::reverse(e.begin(), e.end());
        maxlen = std::max(maxlen, (int)e.size());
    }
    if (maxlen > 24) return;  // such a factor has no packets
    const int EP = maxlen <= 4 ? 4 : maxlen <= 8 ? 8 : maxlen <= 16 ? 16 : 24;
    std::vector<int> perm(n);
    for (int i = 0; i < n; i++) perm[i] = i;
    std::shuffle(perm.begin(), perm.end(), g);
    for (int p = 0; p < n;) {
        const int nr = std::min<int>(n - p, 1 + (int)(g() % 256));
        const Pk6Layout lay = pk6_layout(EP, nr);
        std::vector<uint32_t> want(lay.end, 0u), got;
        for (long w = 0; w < lay.v; w++) want[w] = (uint32_t)g();  // C: pattern-only, must survive
        double *V = reinterpret_cast<double *>(want.data() + lay.v);
        double *D = reinterpret_cast<double *>(want.data() + lay.d);
        for (int r = 0; r < nr; r++) {
            D[r] = 1.0;
            want[lay.row + r] = (uint32_t)perm[p + r];
        }
        got = want;  // V all +0.0, as build_packets6 leaves the unused slots
        for (int r = 0; r < nr; r++) {
            const std::vector<double> &e = ent[perm[p + r]];
            for (size_t q = 0; q < e.size(); q++) V[2L * ((long)(q / 2) * nr + r) + (q & 1)] = e[q];
        }
        for (int r = 0; r < nr; r++)
            pk6_refill_row(got.data(), EP, nr, r, (int)got[lay.row + r], upper, bs, P.nb, P.Bp.data(), P.Bj.data(),
                           P.first.data(), Fx.data());
        CHECK(want == got, "refill: record differs (nb %d bs %d upper %d nr %d EP %d)", P.nb, bs, (int)upper, nr, EP);
        p += nr;
    }
}

int main()
{
    std::mt19937 g(20251);
    int cases = 0;
    for (int bs = 1; bs <= 8; bs++)
        for (int per : {0, 1, 2, 3, 6})
            for (int nb : {1, 2, 37, 150}) {
                const Pattern P = make_pattern(g, nb, bs, per, (bs + per + nb) % 2 == 0);
                check_scatter(g, P);
                check_refill(g, P, false);
                check_refill(g, P, true);
                cases++;
            }
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("ok: %d patterns\n", cases);
    return 0;
}
