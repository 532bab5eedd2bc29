// iluk_refill_check.cpp -- the index arithmetic of lssp_amd_iluk_refactor's
// kernels on the host (no GPU, no HIP): the per-row bodies of k_iluk_match,
// k_iluk_scatter, k_pk6_refill_scalar and k_linef_refill
// (lssp_amd/csrc/iluk_refactor_dev.h), and the row rules and slot inversions of
// both line sweeps' coefficient streams (k_coef_refill, k_linef_refill,
// build_lineg), run against independent restatements of the pattern rule, of
// build_packets6's value placement and of the stream layouts, on exactly-sized
// heap arrays, so a sanitizer sees any access outside them:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ilssp_amd/csrc tools/iluk_refill_check.cpp -o /tmp/iluk_refill_check && /tmp/iluk_refill_check
// Exit status 0 and "ok" when every case matches.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "iluk_refactor_dev.h"

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

// a factor pattern with its flag bytes and the matrix it came from
struct Factor {
    int n;
    std::vector<int> Fp, Fj, dpos;
    std::vector<unsigned char> fin;
    std::vector<int> Ap, Aj;  // the (sorted) creating matrix: F's flag-1 entries
};

// rows of about per matrix entries and fill fill entries within +-reach of the
// diagonal; every nodiag-th row lacks its diagonal in A (flag 2 in F)
static Factor make_factor(std::mt19937 &g, int n, int per, int fill, int reach, int nodiag)
{
    Factor F;
    F.n = n;
    F.Fp.push_back(0);
    F.Ap.push_back(0);
    for (int i = 0; i < n; i++) {
        std::map<int, int> row;  // column -> flag
        auto col = [&]() { return std::min(n - 1, std::max(0, i - reach + (int)(g() % (2 * reach + 1)))); };
        for (int q = 0; q < fill; q++) row[col()] = 0;
        for (int q = 0; q < per; q++) row[col()] = 1;
        row[i] = nodiag && i % nodiag == nodiag - 1 ? 2 : 1;
        for (auto &kv : row) {
            if (kv.first == i) F.dpos.push_back((int)F.Fj.size());
            F.Fj.push_back(kv.first);
            F.fin.push_back((unsigned char)kv.second);
            if (kv.second == 1) F.Aj.push_back(kv.first);
        }
        F.Fp.push_back((int)F.Fj.size());
        F.Ap.push_back((int)F.Aj.size());
    }
    return F;
}

static int match_all(const Factor &F, const std::vector<int> &Ap, const std::vector<int> &Aj)
{
    // the arrays handed over exactly sized (a copy: data() of the caller's may have spare capacity)
    std::vector<int> ap(Ap), aj(Aj);
    ap.shrink_to_fit();
    aj.shrink_to_fit();
    int bad = 0;
    for (int r = 0; r < F.n; r++)
        bad |= iluk_match_row(r, (int)aj.size(), ap.data(), aj.data(), F.Fp.data(), F.Fj.data(), F.fin.data());
    return bad;
}

static void check_match_scatter(std::mt19937 &g, const Factor &F)
{
    const int n = F.n, nnz = (int)F.Aj.size();
    std::uniform_real_distribution<double> u(-1, 1);
    CHECK(!match_all(F, F.Ap, F.Aj), "match: the creating pattern was refused (n %d)", n);
    std::vector<double> Ax(nnz);
    for (double &v : Ax) v = u(g);
    // scatter against a per-row map
    std::vector<double> got(F.Fj.size(), 7.0), want(F.Fj.size());
    for (int r = 0; r < n; r++) {
        std::map<int, double> a;
        for (int k = F.Ap[r]; k < F.Ap[r + 1]; k++) a[F.Aj[k]] = Ax[k];
        for (int f = F.Fp[r]; f < F.Fp[r + 1]; f++)
            want[f] = F.fin[f] == 2 ? 1e-10 : a.count(F.Fj[f]) ? a[F.Fj[f]] : 0.0;
        iluk_scatter_row(r, F.Ap.data(), Ax.data(), F.Fp.data(), F.fin.data(), got.data());
    }
    CHECK(!memcmp(want.data(), got.data(), sizeof(double) * want.size()), "scatter: values differ (n %d)", n);
    for (size_t f = 0; f < got.size(); f++)
        if (F.fin[f] == 0) CHECK(!std::signbit(got[f]) && got[f] == 0.0, "scatter: fill is not +0.0");
    if (nnz < 2) return;
    // refusals: reported, and nothing outside the arrays touched (the sanitizer's part)
    auto rowof = [&](int k) { return (int)(std::upper_bound(F.Ap.begin(), F.Ap.end(), k) - F.Ap.begin()) - 1; };
    for (int rep = 0; rep < 8; rep++) {
        const int k = (int)(g() % nnz), r = rowof(k);
        {  // an entry moved one column (onto a free column, a fill position or its neighbour)
            std::vector<int> Aj = F.Aj;
            Aj[k] = Aj[k] + 1 < n ? Aj[k] + 1 : Aj[k] - 1;
            CHECK(match_all(F, F.Ap, Aj), "match: a moved entry passed");
        }
        {  // an entry removed
            std::vector<int> Ap = F.Ap, Aj = F.Aj;
            Aj.erase(Aj.begin() + k);
            for (int i = r + 1; i <= n; i++) Ap[i]--;
            CHECK(match_all(F, Ap, Aj), "match: a removed entry passed");
        }
        {  // an extra entry exactly on a fill position of the row
            for (int f = F.Fp[r]; f < F.Fp[r + 1]; f++)
                if (F.fin[f] == 0) {
                    std::vector<int> Ap = F.Ap, Aj = F.Aj;
                    Aj.insert(std::lower_bound(Aj.begin() + Ap[r], Aj.begin() + Ap[r + 1], F.Fj[f]), F.Fj[f]);
                    for (int i = r + 1; i <= n; i++) Ap[i]++;
                    CHECK(match_all(F, Ap, Aj), "match: an entry on a fill position passed");
                    break;
                }
        }
        {  // an entry on an inserted diagonal
            for (int f = F.Fp[r]; f < F.Fp[r + 1]; f++)
                if (F.fin[f] == 2) {
                    std::vector<int> Ap = F.Ap, Aj = F.Aj;
                    Aj.insert(std::lower_bound(Aj.begin() + Ap[r], Aj.begin() + Ap[r + 1], F.Fj[f]), F.Fj[f]);
                    for (int i = r + 1; i <= n; i++) Ap[i]++;
                    CHECK(match_all(F, Ap, Aj), "match: an entry on an inserted diagonal passed");
                }
        }
        if (F.Ap[r + 1] - F.Ap[r] >= 2) {  // the row in descending order; a repeated column
            std::vector<int> Aj = F.Aj;
            std::reverse(Aj.begin() + F.Ap[r], Aj.begin() + F.Ap[r + 1]);
            CHECK(match_all(F, F.Ap, Aj), "match: a descending row passed");
            Aj = F.Aj;
            Aj[F.Ap[r] + 1] = Aj[F.Ap[r]];
            CHECK(match_all(F, F.Ap, Aj), "match: a repeated column passed");
        }
        for (int v : {-1, n, n + 7, 1 << 30, -(1 << 30)}) {  // columns out of range
            std::vector<int> Aj = F.Aj;
            Aj[k] = v;
            CHECK(match_all(F, F.Ap, Aj), "match: column %d passed", v);
        }
    }
    // row ranges outside [0, nnz)
    std::vector<int> Ap = F.Ap;
    Ap[n] = nnz + 5;
    CHECK(match_all(F, Ap, F.Aj), "match: a row range past nnz passed");
    Ap = F.Ap;
    Ap[0] = -3;
    CHECK(match_all(F, Ap, F.Aj), "match: a negative row range passed");
    Ap = F.Ap;
    std::swap(Ap[n / 2], Ap[n / 2 + 1]);
    if (Ap != F.Ap) CHECK(match_all(F, Ap, F.Aj), "match: a descending row range passed");
}

// k_pk6_refill_scalar's body against build_packets6's placement of the rows
// build_bp_schedule hands it: L's strict entries ascending (D = the unit 1.0),
// U's in descending storage order with D = the stored pivot
static void check_packets(std::mt19937 &g, const Factor &F, bool upper, int *ep_seen)
{
    const int n = F.n;
    std::uniform_real_distribution<double> u(-1, 1);
    std::vector<double> Fx(F.Fj.size());
    for (double &v : Fx) v = u(g);
    std::vector<std::vector<double>> ent(n);
    int maxlen = 0;
    for (int i = 0; i < n; i++) {
        for (int f = F.Fp[i]; f < F.Fp[i + 1]; f++)
            if (upper ? F.Fj[f] > i : F.Fj[f] < i) ent[i].push_back(Fx[f]);
        if (upper) std::reverse(ent[i].begin(), ent[i].end());
        maxlen = std::max(maxlen, (int)ent[i].size());
    }
    if (maxlen > 24) return;  // such a factor has no packets
    const int EP = maxlen <= 4 ? 4 : maxlen <= 8 ? 8 : maxlen <= 16 ? 16 : 24;
    ep_seen[EP]++;
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
            D[r] = upper ? -5.0 : 1.0;  // U: a stale pivot the refill must replace
            want[lay.row + r] = (uint32_t)perm[p + r];
        }
        got = want;  // V all +0.0, as build_packets6 leaves the unused slots
        for (int r = 0; r < nr; r++) {
            const int row = perm[p + r];
            const std::vector<double> &e = ent[row];
            for (size_t q = 0; q < e.size(); q++) V[2L * ((long)(q / 2) * nr + r) + (q & 1)] = e[q];
            if (upper) D[r] = Fx[F.dpos[row]];
        }
        for (int r = 0; r < nr; r++)
            iluk_pk6_row(got.data(), EP, nr, r, (int)got[lay.row + r], upper, n, F.Fp.data(), F.Fj.data(), F.dpos.data(),
                         Fx.data());
        CHECK(want == got, "packets: record differs (n %d upper %d nr %d EP %d)", n, (int)upper, nr, EP);
        p += nr;
    }
}

// ---- the line sweeps' coefficient streams (k_coef_refill, k_linef_refill, build_lineg) ----
// The shared row rules and slot inversions against a restatement that shares
// nothing with them: a row's coefficients are looked up by NEIGHBOUR COLUMN (not
// classified by offset), and the rows are placed FORWARD, tile by tile, from
// (plane, line, i) to their slot (not inverted from the slot); everything not
// placed is +0.0.  Inputs: a lone L (strict part, a non-unit diagonal last), a
// lone U (pivot first) and the combined F with and without diagonal positions.
struct Tile {
    int j0, nj, k0, np, T;
    long cbase;
};

struct GridFactors {
    long n = 0;
    std::vector<int> Lp{0}, Lj, Up{0}, Uj, Fp{0}, Fj, dpos;
    std::vector<double> Lx, Ux, Fx;
    std::vector<std::map<long, double>> lrow, urow;  // per row: column -> value (diagonals included)
};

// lower(r) / upper(r): the strict neighbour columns of row r, ascending
template <class LO, class UP>
static GridFactors grid_factors(std::mt19937 &g, long n, LO lower, UP upper)
{
    std::uniform_real_distribution<double> u(-1, 1), d(0.5, 1.5);
    GridFactors G;
    G.n = n;
    G.lrow.resize(n);
    G.urow.resize(n);
    for (long r = 0; r < n; r++) {
        const double ldiag = d(g), piv = d(g);  // L's diagonal is NOT 1.0
        for (long c : lower(r)) {
            const double v = u(g);
            G.Lj.push_back((int)c), G.Lx.push_back(v), G.Fj.push_back((int)c), G.Fx.push_back(v);
            G.lrow[r][c] = v;
        }
        G.Lj.push_back((int)r), G.Lx.push_back(ldiag);
        G.lrow[r][r] = ldiag;
        G.dpos.push_back((int)G.Fj.size());
        G.Fj.push_back((int)r), G.Fx.push_back(piv);
        G.Uj.push_back((int)r), G.Ux.push_back(piv);
        G.urow[r][r] = piv;
        for (long c : upper(r)) {
            const double v = u(g);
            G.Uj.push_back((int)c), G.Ux.push_back(v), G.Fj.push_back((int)c), G.Fx.push_back(v);
            G.urow[r][c] = v;
        }
        G.Lp.push_back((int)G.Lj.size()), G.Up.push_back((int)G.Uj.size()), G.Fp.push_back((int)G.Fj.size());
    }
    for (auto *v : {&G.Lp, &G.Lj, &G.Up, &G.Uj, &G.Fp, &G.Fj, &G.dpos}) v->shrink_to_fit();
    for (auto *v : {&G.Lx, &G.Ux, &G.Fx}) v->shrink_to_fit();
    return G;
}

// the coefficients of natural row r on one sweep: the neighbours at the given
// distances, in component order, then (NA > noff) the diagonal
static void want_row(const GridFactors &G, long r, bool upper, const std::vector<long> &dist, int NA, bool unit,
                     double *out)
{
    const std::map<long, double> &row = upper ? G.urow[r] : G.lrow[r];
    for (size_t a = 0; a < dist.size(); a++) {
        const auto it = row.find(upper ? r + dist[a] : r - dist[a]);
        out[a] = it == row.end() ? 0.0 : it->second;
    }
    if (NA > (int)dist.size()) out[dist.size()] = !upper && unit ? 1.0 : row.at(r);
}

// the three inputs of a sweep: 0 the lone factor (stored diagonal), 1 F without
// diagonal positions, 2 F with them (both: L's diagonal the unit)
static FactorView view_of(const GridFactors &G, bool upper, int input)
{
    if (input == 0)
        return upper ? FactorView{G.Up.data(), G.Uj.data(), G.Ux.data(), nullptr, false}
                     : FactorView{G.Lp.data(), G.Lj.data(), G.Lx.data(), nullptr, false};
    return FactorView{G.Fp.data(), G.Fj.data(), G.Fx.data(), input == 2 ? G.dpos.data() : nullptr, true};
}

static long lay_out(std::vector<Tile> &tiles)
{
    long rows_total = 0;
    for (Tile &t : tiles) {
        t.cbase = rows_total;
        rows_total += (long)t.T * 8 * t.nj;
    }
    return rows_total;
}

// k_line2: the 5-/7-point ILU(0) of a box whose plane k is cut from plane k-1
// where cut[k]; 16 x 8 tiles between the cuts, the U tiles mirrored
static void check_line0(std::mt19937 &g, int nx, int ny, int nz, const std::vector<int> &cutk)
{
    const long pl = (long)nx * ny, n = pl * nz;
    std::vector<char> kin(nz, 1);
    kin[0] = 0;
    for (int k : cutk) kin[k] = 0;
    const GridFactors G = grid_factors(
        g, n,
        [&](long r) {
            const int i = (int)(r % nx), j = (int)((r / nx) % ny), k = (int)(r / pl);
            std::vector<long> c;
            if (k > 0 && kin[k]) c.push_back(r - pl);
            if (j > 0) c.push_back(r - nx);
            if (i > 0) c.push_back(r - 1);
            return c;
        },
        [&](long r) {
            const int i = (int)(r % nx), j = (int)((r / nx) % ny), k = (int)(r / pl);
            std::vector<long> c;
            if (i < nx - 1) c.push_back(r + 1);
            if (j < ny - 1) c.push_back(r + nx);
            if (k < nz - 1 && kin[k + 1]) c.push_back(r + pl);
            return c;
        });
    std::vector<std::pair<int, int>> kt;  // plane segments between the cuts, in tiles of <= 8 planes
    for (int k = 0; k < nz;) {
        int e = k + 1;
        while (e < nz && kin[e]) e++;
        for (int k0 = k; k0 < e; k0 += 8) kt.push_back({k0, std::min(8, e - k0)});
        k = e;
    }
    const int S = (int)kt.size(), W = (ny + 15) / 16;
    auto sig = [](int p) { return p >= 4 ? 1 : 0; };  // LV = 2: wave 1's planes run one level later
    for (int upper = 0; upper < 2; upper++)
        for (int input = 0; input < 3; input++)
            for (int NA = upper ? 4 : 3; NA <= 4; NA++) {
                std::vector<Tile> tiles((size_t)S * W);
                for (int K = 0; K < S; K++)
                    for (int J = 0, j0 = 0; J < W; J++) {
                        Tile t;
                        t.j0 = j0;
                        t.nj = ny / W + (J < ny % W ? 1 : 0);
                        j0 += t.nj;
                        t.k0 = kt[K].first;
                        t.np = kt[K].second;
                        t.T = (nx + t.nj + t.np - 2 + sig(t.np - 1) + 1) / 2 * 2;
                        if (!upper) tiles[(size_t)K * W + J] = t;
                        else {
                            t.j0 = ny - t.j0 - t.nj;
                            t.k0 = nz - t.k0 - t.np;
                            tiles[(size_t)(S - 1 - K) * W + (W - 1 - J)] = t;
                        }
                    }
                const long rows_total = lay_out(tiles);
                std::vector<double> want((size_t)rows_total * NA, 0.0), got((size_t)rows_total * NA, -3.0);
                long placed = 0;
                for (const Tile &t : tiles)
                    for (int p = 0; p < t.np; p++)
                        for (int l = 0; l < t.nj; l++)
                            for (int i = 0; i < nx; i++) {
                                const long v = i + l + p + sig(p);
                                const long rs = ((long)(t.k0 + p) * ny + (t.j0 + l)) * nx + i;
                                CHECK(v < t.T, "line0: a row past its tile's levels");
                                want_row(G, upper ? n - 1 - rs : rs, upper != 0, {pl, nx, 1}, NA, input != 0,
                                         want.data() + (size_t)(t.cbase + v * 8 * t.nj + p * t.nj + l) * NA);
                                placed++;
                            }
                CHECK(placed == n, "line0: the tiles place %ld of %ld rows (%d x %d x %d)", placed, n, nx, ny, nz);
                const FactorView f = view_of(G, upper != 0, input);
                for (const Tile &t : tiles)
                    for (int s = 0; s < t.T; s++)
                        for (int p = 0; p < 8; p++)
                            for (int l = 0; l < t.nj; l++) {
                                double *dst = got.data() + (size_t)(t.cbase + (long)s * 8 * t.nj + p * t.nj + l) * NA;
                                const long rs = line_slot_row(s, p, l, t.j0, t.k0, t.np, nx, ny, 2);
                                CHECK(rs < n, "line0: a slot's row past the grid");
                                if (rs >= 0 && rs < n) line_coef_row(rs, upper != 0, n, nx, pl, NA, f, dst);
                                else
                                    for (int a = 0; a < NA; a++) dst[a] = 0.0;
                            }
                CHECK(!memcmp(want.data(), got.data(), sizeof(double) * want.size()),
                      "line0: stream differs (%d x %d x %d upper %d input %d NA %d)", nx, ny, nz, upper, input, NA);
            }
}

static std::vector<int> widths(int m)  // mirror-symmetric widths <= 16 of the skewed columns
{
    for (int W = (m + 15) / 16;; W++) {
        const int base = m / W, extra = m % W;
        if (W % 2 == 0 && extra % 2) continue;
        std::vector<int> w(W, base);
        for (int q = 0; q < extra / 2; q++) w[q]++, w[W - 1 - q]++;
        if (extra % 2) w[W / 2]++;
        return w;
    }
}

// k_linef: the ILU(1) pattern of a 7-point box; S x W tiles of the skewed
// columns j' = j + k, the U tiles mirrored
static void check_linef(std::mt19937 &g, int nx, int ny, int nz)
{
    const long pl = (long)nx * ny, n = pl * nz;
    const GridFactors G = grid_factors(
        g, n,
        [&](long r) {
            const int i = (int)(r % nx), j = (int)((r / nx) % ny), k = (int)(r / pl);
            std::vector<long> c;
            if (k > 0) c.push_back(r - pl);
            if (k > 0 && i < nx - 1) c.push_back(r - pl + 1);
            if (k > 0 && j < ny - 1) c.push_back(r - pl + nx);
            if (j > 0) c.push_back(r - nx);
            if (j > 0 && i < nx - 1) c.push_back(r - nx + 1);
            if (i > 0) c.push_back(r - 1);
            return c;
        },
        [&](long r) {
            const int i = (int)(r % nx), j = (int)((r / nx) % ny), k = (int)(r / pl);
            std::vector<long> c;
            if (i < nx - 1) c.push_back(r + 1);
            if (j < ny - 1 && i > 0) c.push_back(r + nx - 1);
            if (j < ny - 1) c.push_back(r + nx);
            if (k < nz - 1 && j > 0) c.push_back(r + pl - nx);
            if (k < nz - 1 && i > 0) c.push_back(r + pl - 1);
            if (k < nz - 1) c.push_back(r + pl);
            return c;
        });
    const int m = ny + nz - 1;
    const std::vector<int> wd = widths(m);
    const int W = (int)wd.size(), S = (nz + 7) / 8;
    std::vector<int> js(W + 1, 0);
    for (int J = 0; J < W; J++) js[J + 1] = js[J] + wd[J];
    for (int upper = 0; upper < 2; upper++)
        for (int input = 0; input < 3; input++)
            for (int NA = upper ? 7 : 6; NA <= 7; NA++) {
                std::vector<Tile> tiles((size_t)S * W);
                for (int K = 0; K < S; K++)
                    for (int J = 0; J < W; J++) {
                        Tile t;
                        t.j0 = js[J];
                        t.nj = wd[J];
                        t.k0 = K * 8;
                        t.np = std::min(8, nz - t.k0);
                        const int T = nx + 2 * (t.nj - 1) + (t.np - 1) + ((t.np - 1) >> 2) + 1;
                        t.T = (T + 1) / 2 * 2;
                        if (!upper) tiles[(size_t)K * W + J] = t;
                        else {
                            t.j0 = m - t.j0 - t.nj;
                            t.k0 = nz - t.k0 - t.np;
                            tiles[(size_t)(S - 1 - K) * W + (W - 1 - J)] = t;
                        }
                    }
                const long rows_total = lay_out(tiles);
                std::vector<double> want((size_t)rows_total * NA, 0.0), got((size_t)rows_total * NA, -3.0);
                long placed = 0;
                for (const Tile &t : tiles) {
                    for (int p = 0; p < t.np; p++)
                        for (int l = 0; l < t.nj; l++) {
                            const int j = t.j0 + l - (t.k0 + p);
                            if (j < 0 || j >= ny) continue;
                            for (int i = 0; i < nx; i++) {
                                const long v = i + 2 * l + p + (p >> 2);
                                const long rs = ((long)(t.k0 + p) * ny + j) * nx + i;
                                want_row(G, upper ? n - 1 - rs : rs, upper != 0, {pl, pl - 1, pl - nx, nx, nx - 1, 1}, NA,
                                         input != 0, want.data() + (size_t)(t.cbase + v * 8 * t.nj + p * t.nj + l) * NA);
                                placed++;
                            }
                        }
                }
                CHECK(placed == n, "linef: the tiles place %ld of %ld rows (%d x %d x %d)", placed, n, nx, ny, nz);
                const FactorView f = view_of(G, upper != 0, input);
                for (const Tile &t : tiles) {
                    const long slots = (long)t.T * 8 * t.nj;
                    for (long s = 0; s < slots; s++) {
                        double *dst = got.data() + (size_t)(t.cbase + s) * NA;
                        const long rs = linef_slot_row(s, t.j0, t.nj, t.k0, t.np, nx, ny);
                        if (rs >= 0 && rs < n) linef_coef_row(rs, upper != 0, n, nx, pl, NA, f, dst);
                        else
                            for (int a = 0; a < NA; a++) dst[a] = 0.0;
                    }
                }
                CHECK(!memcmp(want.data(), got.data(), sizeof(double) * want.size()),
                      "linef: stream differs (%d x %d x %d upper %d input %d NA %d)", nx, ny, nz, upper, input, NA);
            }
}

int main()
{
    std::mt19937 g(20260);
    int cases = 0, ep_seen[25] = {0};
    // per / fill chosen so that the longest strict rows land in every EP class
    const int shapes[][5] = {{1, 0, 0, 3, 0},   {2, 1, 0, 2, 0},   {37, 2, 0, 6, 5},   {150, 2, 2, 9, 4},
                             {150, 4, 3, 12, 0}, {200, 6, 5, 20, 7}, {300, 10, 8, 25, 3}, {300, 14, 12, 30, 0},
                             {120, 3, 20, 40, 2}};
    for (const auto &s : shapes) {
        const Factor F = make_factor(g, s[0], s[1], s[2], s[3], s[4]);
        check_match_scatter(g, F);
        check_packets(g, F, false, ep_seen);
        check_packets(g, F, true, ep_seen);
        cases++;
    }
    for (int ep : {4, 8, 16, 24}) CHECK(ep_seen[ep] > 0, "no packet case of EP %d", ep);
    // one tile; ragged j tiles, 8 + 5 planes; tiles off the grid; 2 planes; a single plane column; 2-D
    const int boxes[][3] = {{4, 3, 2}, {9, 21, 13}, {5, 7, 20}, {13, 37, 11}, {3, 3, 9}, {6, 40, 2}, {6, 10, 1}};
    for (const auto &b : boxes) {
        check_linef(g, b[0], b[1], b[2]);
        cases++;
    }
    // k_line2: 9 + 8 lines and 8 + 1 planes; fewer than 8 planes and ragged lines; cuts (a one-plane
    // segment, a segment longer than a tile); 2-D
    check_line0(g, 2, 17, 9, {});
    check_line0(g, 5, 21, 5, {});
    check_line0(g, 4, 9, 12, {1, 2});
    check_line0(g, 3, 33, 20, {5, 16});
    check_line0(g, 6, 10, 1, {});
    cases += 5;
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("ok: %d cases (packets EP 4/8/16/24: %d/%d/%d/%d)\n", cases, ep_seen[4], ep_seen[8], ep_seen[16], ep_seen[24]);
    return 0;
}
