// sched_dev_check.cpp -- the device schedule builder (lssp_amd/csrc/tri_sched.hip)
// on the host (no GPU, no HIP): the lane-level bodies of lssp_amd/csrc/sched_dev.h
// run by plain loops over 64 lanes between the kernels' wave-level points, stage
// after stage as build_trisched_dev launches them, on exactly-sized heap arrays,
// so a sanitizer sees any access outside them; then the host builder
// (sched_host.h: what tri_bp.cpp uploads) on the same factor, and every array and
// scalar compared byte for byte:
//   c++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ilssp_amd/csrc tools/sched_dev_check.cpp -o /tmp/sched_dev_check && /tmp/sched_dev_check IN OUT
// IN  (binary): int32 n, nnzL, nnzU; Lp[n + 1], Lj[nnzL] (int32), Lx[nnzL] (double); Up, Uj, Ux the same.
//               L with its diagonal last in each row, U with its pivot first.
// OUT (binary): for L, then U: int32 hdr[12] = {B, nb, nsteps, npackets, EP, EXT, rows per packet, rec words,
//               idx words, unit, nlevels, origin = 1}, int64 packets counted at EXT = 2, 3, 4 (-1: not counted),
//               then blk[nb + 1], desc[max(4 npackets, 1)], rec, idx, perm[n], pos[n] (4-byte words).
//               U's rhs entries are L's schedule positions, as in a handle.
// Exit status 0: both builders agree on both factors; 1: they differ; 2: bad usage or file;
//             3: malformed factor (LSSP_AMD_EINVAL); 4: unsupported (LSSP_AMD_EUNSUPPORTED: a strict
//             row beyond 24 entries, a block beyond PK3_CAP packets).
// tests/test_sched_dev_cpu.py runs it over tests/sched_inputs.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <vector>

#include "sched_host.h"

namespace lssp_amd {
void parallel_for(long n, const std::function<void(long, long)> &f, long) { f(0, n); }
// the host builder's level pass (tri_levels, ilu_setup.cpp)
static int levels_host(int n, const std::vector<int> &Tp, const std::vector<int> &Tj, bool upper, std::vector<int> &lev)
{
    lev.assign(n, 0);
    for (int i = 0; i < n; i++)
        if (Tp[i + 1] - Tp[i] < 1) return LSSP_AMD_EINVAL;
    for (int q = 0; q < n; q++) {
        const int i = upper ? n - 1 - q : q;
        int l = 0;
        for (int k = upper ? Tp[i] + 1 : Tp[i]; k < (upper ? Tp[i + 1] : Tp[i + 1] - 1); k++) {
            const int j = Tj[k];
            if (upper ? (j <= i || j >= n) : (j < 0 || j >= i)) return LSSP_AMD_EINVAL;
            l = std::max(l, lev[j] + 1);
        }
        lev[i] = l;
    }
    return LSSP_AMD_OK;
}
}  // namespace lssp_amd

using namespace lssp_amd;

namespace {

template <typename T>
bool rd(FILE *f, T *p, size_t n)
{
    return n == 0 || fread(p, sizeof(T), n, f) == n;
}
template <typename T>
std::unique_ptr<T[]> arr(size_t n)
{
    return std::unique_ptr<T[]>(new T[std::max<size_t>(n, 1)]);
}

struct DevSched {  // what build_trisched_dev leaves in a TriSched
    int B = 0, nb = 0, nsteps = 0, unit = 0, nlevels = 0, npk = 0, ep = 4, ext = 2;
    long cnt_ext[3] = {-1, -1, -1};
    size_t nrec = 0, nidx = 0, ndesc = 0;
    std::unique_ptr<int[]> perm, pos, blk, desc, idx;
    std::unique_ptr<uint32_t[]> rec;
};

struct Walk {  // k_sched_walk's arguments
    int n, upper, nb, EP, cap;
    long B;
    const int *rp, *step_pos, *blk_step;
    int *cols, *stamp, *slot;
    long *npk, *recw, *idxw;
    int *desc, *pkxl, *xl, *blk;
};

// one block of k_sched_walk: the wave's registers are arrays over the lanes
int walk_block(const Walk &a, int b, bool final, long &total, bool &capx)
{
    const long sbase = 2 * a.B * b;
    int *stamp = a.stamp + sbase, *slot = a.slot + sbase;
    const long pk0 = final ? a.npk[b] : 0, rec0 = final ? a.recw[b] : 0, idx0 = final ? a.idxw[b] : 0;
    const long pkend = final ? a.npk[b + 1] : 0;
    const int xl0 = a.rp[std::min((long)b * a.B, (long)a.n)];
    int pid = 0;
    long npk = 0, recw = 0, idxw = 0, xo = 0;
    int g[SCHED_LANES], myslot[SCHED_LANES], dup[SCHED_LANES];
    long w[SCHED_LANES];
    bool fresh[SCHED_LANES], first[SCHED_LANES];
    for (int s = a.blk_step[b]; s < a.blk_step[b + 1]; s++) {
        int p = a.step_pos[s];
        const int pend = a.step_pos[s + 1];
        while (p < pend) {
            int nr = 0, nx = 0, emax = 0;
            while (p + nr < pend && nr < PK3_ROWS) {
                const int r = p + nr;
                if (!sched_rec_fits(a.EP, nr)) break;
                const int k0 = a.rp[r], len = a.rp[r + 1] - k0;
                bool bad = len > PK6_MAXLEN;
                int newx = 0;
                for (int lane = 0; lane < SCHED_LANES; lane++) {
                    sched_walk_lane(a.n, a.upper != 0, a.B, b, a.cols, k0, len, lane, stamp, pid, g[lane], w[lane],
                                    fresh[lane], bad);
                    newx += fresh[lane];
                }
                if (bad) return 1;
                if (nx + newx > a.cap) break;
                for (int lane = 0; lane < SCHED_LANES; lane++) dup[lane] = -1;
                if (newx > 1)
                    for (int e = 0; e < len; e++)
                        for (int lane = 0; lane < SCHED_LANES; lane++)
                            if (lane > e && fresh[lane] && fresh[e] && g[e] == g[lane] && dup[lane] < 0) dup[lane] = e;
                int cnt = 0;
                for (int lane = 0; lane < SCHED_LANES; lane++) {
                    first[lane] = fresh[lane] && dup[lane] < 0;
                    myslot[lane] = nx + cnt;
                    cnt += first[lane];
                    if (!first[lane] && g[lane] >= 0 && !fresh[lane]) myslot[lane] = slot[w[lane]];
                }
                for (int lane = 0; lane < SCHED_LANES; lane++)
                    if (dup[lane] >= 0) myslot[lane] = myslot[dup[lane]];
                for (int lane = 0; lane < SCHED_LANES; lane++) {
                    if (first[lane]) {
                        stamp[w[lane]] = pid;
                        slot[w[lane]] = myslot[lane];
                        if (final) a.xl[xl0 + xo + myslot[lane]] = g[lane];
                    }
                    if (final && g[lane] >= 0) a.cols[k0 + lane] = myslot[lane];
                }
                nx += cnt;
                emax = std::max(emax, len);
                nr++;
            }
            if (nr == 0) return 1;
            if (final) {
                if (pk0 + npk >= pkend) return 1;
                int *d = a.desc + 4 * (pk0 + npk);
                d[0] = (int)((rec0 + recw) / 4);
                d[1] = (int)(idx0 + idxw);
                d[2] = nr | (nx << 10) | (emax << 21);
                d[3] = p;
                a.pkxl[pk0 + npk] = (int)(xl0 + xo);
            }
            recw += sched_rec_words(a.EP, nr);
            idxw += nr + nx;
            xo += nx;
            npk++;
            p += nr;
            pid++;
        }
    }
    if (final) {
        a.blk[b] = (int)pk0;
        if (b == a.nb - 1) a.blk[a.nb] = (int)(pk0 + npk);
    } else {
        a.npk[b] = npk;
        a.recw[b] = recw;
        a.idxw[b] = idxw;
        if (b == 0) a.npk[a.nb] = a.recw[a.nb] = a.idxw[a.nb] = 0;
        total += npk;
        if (npk > PK3_CAP) capx = true;
    }
    return 0;
}

// build_trisched_dev, stage by stage
int dev_build(int n, int nnz, const int *Tp, const int *Tj, const double *Tx, bool upper, const int *rhs_pos,
              DevSched &t)
{
    // 1: k_sched_check
    int flags = 0, bw = 0, maxlen = 0;
    for (int i = 0; i < n; i++) {
        int fi, bi, li;
        sched_check_row(n, nnz, upper, Tp, Tj, Tx, i, fi, bi, li);
        flags |= fi;
        bw = std::max(bw, bi);
        maxlen = std::max(maxlen, li);
    }
    if (flags & SCHED_BAD) return LSSP_AMD_EINVAL;
    if (maxlen > PK6_MAXLEN) return LSSP_AMD_EUNSUPPORTED;
    const bool unit = !(flags & SCHED_NONUNIT);
    const int EP = sched_ep(maxlen);
    long B = std::max(64L, (long)std::max(bw, 1));
    if (B > n) B = n;
    const int nb = (int)((n + B - 1) / B);
    const int nstrict = nnz - n;

    // 2: k_sched_levels -- chunks in ticket order, the wave looping until all its lanes are done
    auto lev = arr<int>(n);
    std::fill(lev.get(), lev.get() + n, -1);
    int lmax = 0;
    auto load = [](const int *p) { return *p; };
    for (long c = 0; c < ((long)n + SCHED_LANES - 1) / SCHED_LANES; c++) {
        int k[SCHED_LANES], kend[SCHED_LANES], l[SCHED_LANES], row[SCHED_LANES];
        bool done[SCHED_LANES];
        for (int lane = 0; lane < SCHED_LANES; lane++) {
            const long q = c * SCHED_LANES + lane;
            done[lane] = q >= n;
            row[lane] = done[lane] ? 0 : sched_q(n, upper, (int)q);
            k[lane] = done[lane] ? 0 : sched_strict_begin(Tp, upper, row[lane]);
            kend[lane] = done[lane] ? 0 : sched_strict_end(Tp, upper, row[lane]);
            l[lane] = 0;
        }
        for (;;) {
            bool all = true, any = false;
            for (int lane = 0; lane < SCHED_LANES; lane++) {
                if (!done[lane] && sched_level_try(Tj, kend[lane], lev.get(), load, k[lane], l[lane])) {
                    lev[row[lane]] = l[lane];
                    lmax = std::max(lmax, l[lane]);
                    done[lane] = any = true;
                }
                all &= done[lane];
            }
            if (all) break;
            if (!any) return LSSP_AMD_ETIMEOUT;  // (the kernel would wait for another wave: none here)
        }
    }
    t.nlevels = lmax + 1;

    // 3: keys, the stable sort (rocprim's radix sort on the device), flags, scan, steps
    auto keys = arr<unsigned long long>(n);
    auto rows = arr<int>(n);
    for (long q = 0; q < n; q++) {
        rows[q] = sched_q(n, upper, (int)q);
        keys[q] = sched_key(q, B, lev[rows[q]]);
    }
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return keys[x] < keys[y]; });
    t.perm = arr<int>(n);
    t.pos = arr<int>(n);
    auto skeys = arr<unsigned long long>(n);
    for (int p = 0; p < n; p++) {
        skeys[p] = keys[order[p]];
        t.perm[p] = rows[order[p]];
    }
    auto sidx = arr<int>((size_t)n + 1);
    for (int p = 0, run = 0; p < n; p++) {
        run += p == 0 || skeys[p] != skeys[p - 1];
        sidx[p] = run;
    }
    const int nsteps = sidx[n - 1];
    auto step_pos = arr<int>((size_t)nsteps + 1), blk_step = arr<int>((size_t)nb + 1);
    for (long p = 0; p < n; p++) {
        t.pos[t.perm[p]] = (int)p;
        const int s = sidx[p] - 1;
        if (p == 0 || sidx[p - 1] != sidx[p]) step_pos[s] = (int)p;
        if (p % B == 0) blk_step[p / B] = s;
        if (p == 0) {
            step_pos[nsteps] = n;
            blk_step[nb] = nsteps;
        }
    }

    // 4: lengths, scan, codes
    auto rp = arr<int>((size_t)n + 1), cols = arr<int>(nstrict);
    rp[0] = 0;
    for (int p = 0; p < n; p++)
        rp[p + 1] = rp[p] + sched_strict_end(Tp, upper, t.perm[p]) - sched_strict_begin(Tp, upper, t.perm[p]);
    for (long p = 0; p < n; p++) {
        const int i = t.perm[p], b = (int)(p / B), send = step_pos[sidx[p]];
        const int k0 = rp[p], len = rp[p + 1] - k0;
        for (int e = 0; e < len; e++)
            cols[k0 + e] = sched_code(n, upper, B, b, send, Tj[sched_entry(Tp, upper, i, e)], t.pos.get());
    }

    // 5: the counting walks
    const size_t win = 2 * (size_t)B * nb, nb1 = (size_t)nb + 1;
    auto stamp = arr<int>(win), slot = arr<int>(win);
    auto cntA = arr<long>(3 * nb1), cntB = arr<long>(3 * nb1), offs = arr<long>(3 * nb1);
    Walk a{};
    a.n = n;
    a.upper = upper;
    a.nb = nb;
    a.EP = EP;
    a.B = B;
    a.rp = rp.get();
    a.step_pos = step_pos.get();
    a.blk_step = blk_step.get();
    a.cols = cols.get();
    a.stamp = stamp.get();
    a.slot = slot.get();
    auto count_at = [&](int cap, long *cnt, long &packets, bool &capx) {
        a.cap = cap;
        a.npk = cnt;
        a.recw = cnt + nb1;
        a.idxw = cnt + 2 * nb1;
        std::fill(stamp.get(), stamp.get() + win, -1);
        packets = 0;
        capx = false;
        for (int b = 0; b < nb; b++)
            if (walk_block(a, b, false, packets, capx)) return LSSP_AMD_EINVAL;
        return LSSP_AMD_OK;
    };
    int ext = PK3_EXT;
    long *cnt = cntA.get();
    bool capx = false;
    {
        long c4 = 0, ce = 0;
        bool cx = false;
        if (count_at(PK3_ROWS * PK3_EXT, cntA.get(), c4, capx)) return LSSP_AMD_EINVAL;
        t.cnt_ext[2] = c4;
        for (int e = 2; e < PK3_EXT; e++) {
            if (count_at(PK3_ROWS * e, cntB.get(), ce, cx)) return LSSP_AMD_EINVAL;
            t.cnt_ext[e - 2] = ce;
            if (ce <= c4 + c4 / 100) {
                ext = e;
                cnt = cntB.get();
                capx = cx;
                break;
            }
        }
    }
    if (capx) return LSSP_AMD_EUNSUPPORTED;

    // 6: scans, the final walk, the fill
    for (int k = 0; k < 3; k++) {
        long run = 0;
        for (size_t b = 0; b < nb1; b++) {
            offs[k * nb1 + b] = run;
            run += cnt[k * nb1 + b];
        }
    }
    const long npk = offs[nb], recw = offs[nb1 + nb], idxw = offs[2 * nb1 + nb];
    if (npk > INT_MAX || recw / 4 > INT_MAX || idxw > INT_MAX) return LSSP_AMD_EUNSUPPORTED;
    t.ndesc = std::max<size_t>(4 * (size_t)npk, 1);
    t.nrec = (size_t)recw + 4;
    t.nidx = (size_t)idxw + 1;
    t.blk = arr<int>(nb1);
    t.desc = arr<int>(t.ndesc);
    t.rec = arr<uint32_t>(t.nrec);
    t.idx = arr<int>(t.nidx);
    // (a device allocation holds anything: make unwritten words show)
    std::fill(t.desc.get(), t.desc.get() + t.ndesc, 0x5a5a5a5a);
    std::fill(t.rec.get(), t.rec.get() + t.nrec, 0x5a5a5a5au);
    std::fill(t.idx.get(), t.idx.get() + t.nidx, 0x5a5a5a5a);
    std::fill(t.rec.get() + recw, t.rec.get() + t.nrec, 0u);
    t.idx[idxw] = 0;
    auto pkxl = arr<int>((size_t)npk), xl = arr<int>(nstrict);
    a.cap = PK3_ROWS * ext;
    a.npk = offs.get();
    a.recw = offs.get() + nb1;
    a.idxw = offs.get() + 2 * nb1;
    a.desc = t.desc.get();
    a.pkxl = pkxl.get();
    a.xl = xl.get();
    a.blk = t.blk.get();
    std::fill(stamp.get(), stamp.get() + win, -1);
    {
        long dummy = 0;
        bool cx = false;
        for (int b = 0; b < nb; b++)
            if (walk_block(a, b, true, dummy, cx)) return LSSP_AMD_EINVAL;
    }
    const int *rhs = rhs_pos ? rhs_pos : t.pos.get();
    for (long pk = 0; pk < npk; pk++) {  // k_sched_fill: one wave per packet
        const int *d = t.desc.get() + 4 * pk;
        const int nr = d[2] & 1023, nx = (d[2] >> 10) & 2047, p = d[3];
        const int par = (int)(pk - t.blk[p / B]) & 1;
        uint32_t *w = t.rec.get() + 4L * d[0];
        for (int lane = 0; lane < SCHED_LANES; lane++)
            for (int r = lane; r < nr; r += SCHED_LANES) {
                const int i = t.perm[p + r], k0 = rp[p + r], len = rp[p + r + 1] - k0;
                sched_fill_row(w, EP, nr, r, par, cols.get(), k0, len, Tp, Tx, upper, i, unit);
                t.idx[(long)d[1] + r] = rhs[i];
            }
        sched_fill_pads(w, EP, nr);
        for (int x = 0; x < nx; x++) t.idx[(long)d[1] + nr + x] = t.pos[xl[pkxl[pk] + x]];
    }
    if (npk == 0) t.desc[0] = 0;
    t.B = (int)B;
    t.nb = nb;
    t.nsteps = nsteps;
    t.unit = unit;
    t.npk = (int)npk;
    t.ep = EP;
    t.ext = ext;
    return LSSP_AMD_OK;
}

template <typename T>
bool same(const char *side, const char *what, const T *a, size_t na, const T *b, size_t nb)
{
    if (na == nb && (na == 0 || memcmp(a, b, na * sizeof(T)) == 0)) return true;
    size_t k = 0;
    while (k < na && k < nb && a[k] == b[k]) k++;
    printf("differ: %s %s (sizes %zu / %zu, first difference at %zu)\n", side, what, na, nb, k);
    return false;
}

struct Factor {
    std::vector<int> Tp, Tj;
    std::vector<double> Tx;
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[3];
    if (!rd(f, hd, 3)) return 2;
    const int n = hd[0];
    if (n < 1 || hd[1] < 0 || hd[2] < 0) return 2;
    Factor F[2];
    for (int s = 0; s < 2; s++) {
        F[s].Tp.resize((size_t)n + 1);
        F[s].Tj.resize(hd[1 + s]);
        F[s].Tx.resize(hd[1 + s]);
        if (!rd(f, F[s].Tp.data(), (size_t)n + 1) || !rd(f, F[s].Tj.data(), F[s].Tj.size()) ||
            !rd(f, F[s].Tx.data(), F[s].Tx.size()))
            return 2;
        if (F[s].Tp[n] != hd[1 + s]) return 3;
    }
    fclose(f);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    bool ok = true;
    DevSched D[2];
    HostSched H[2];
    for (int s = 0; s < 2; s++) {
        const bool upper = s == 1;
        const char *side = upper ? "U" : "L";
        // exactly-sized copies for the device bodies
        const int nnz = hd[1 + s];
        auto Tp = arr<int>((size_t)n + 1), Tj = arr<int>(nnz);
        auto Tx = arr<double>(nnz);
        std::copy(F[s].Tp.begin(), F[s].Tp.end(), Tp.get());
        std::copy(F[s].Tj.begin(), F[s].Tj.end(), Tj.get());
        std::copy(F[s].Tx.begin(), F[s].Tx.end(), Tx.get());
        const int st = dev_build(n, nnz, Tp.get(), Tj.get(), Tx.get(), upper, upper ? D[0].pos.get() : nullptr, D[s]);
        // the host builder: its refusals are ilu_upload's (a row beyond 24 entries leaves npk = -1)
        std::vector<int> lev;
        int sh = levels_host(n, F[s].Tp, F[s].Tj, upper, lev);
        if (sh == LSSP_AMD_OK)
            sh = bp_schedule_host(n, F[s].Tp, F[s].Tj, F[s].Tx, upper, lev, upper ? &H[0].pos : nullptr, H[s],
                                  [](const char *) {});
        if (sh == LSSP_AMD_OK && H[s].npk < 0) sh = LSSP_AMD_EUNSUPPORTED;
        if (st != sh) {
            printf("differ: %s status %d / %d\n", side, st, sh);
            return 1;
        }
        if (st == LSSP_AMD_EINVAL) return 3;
        if (st == LSSP_AMD_EUNSUPPORTED) return 4;
        if (st != LSSP_AMD_OK) return 1;
        const DevSched &d = D[s];
        const HostSched &h = H[s];
        int nlev = 0;
        for (int i = 0; i < n; i++) nlev = std::max(nlev, lev[i] + 1);
        const int sd[] = {d.B, d.nb, d.nsteps, d.npk, d.ep, d.ext, PK3_ROWS, d.unit, d.nlevels};
        const int sv[] = {h.B, h.nb, h.nsteps, h.npk, h.ep, h.ext, h.rows, h.unit, nlev};
        ok &= same(side, "scalars", sd, 9, sv, 9);
        ok &= same(side, "packet counts", d.cnt_ext, 3, h.cnt_ext, 3);
        ok &= same(side, "perm", d.perm.get(), n, h.perm.data(), h.perm.size());
        ok &= same(side, "pos", d.pos.get(), n, h.pos.data(), h.pos.size());
        ok &= same(side, "blk", d.blk.get(), (size_t)d.nb + 1, h.blk.data(), h.blk.size());
        ok &= same(side, "desc", d.desc.get(), d.ndesc, h.desc.data(), h.desc.size());
        ok &= same(side, "rec", d.rec.get(), d.nrec, h.rec.data(), h.rec.size());
        ok &= same(side, "idx", d.idx.get(), d.nidx, h.idx.data(), h.idx.size());
        if (!ok) return 1;
        const int hdr[12] = {d.B, d.nb, d.nsteps, d.npk, d.ep, d.ext, PK3_ROWS, (int)d.nrec, (int)d.nidx, d.unit,
                             d.nlevels, 1};
        const long long cnts[3] = {d.cnt_ext[0], d.cnt_ext[1], d.cnt_ext[2]};
        fwrite(hdr, sizeof(int), 12, f);
        fwrite(cnts, sizeof(long long), 3, f);
        fwrite(d.blk.get(), sizeof(int), (size_t)d.nb + 1, f);
        fwrite(d.desc.get(), sizeof(int), d.ndesc, f);
        fwrite(d.rec.get(), sizeof(uint32_t), d.nrec, f);
        fwrite(d.idx.get(), sizeof(int), d.nidx, f);
        fwrite(d.perm.get(), sizeof(int), n, f);
        fwrite(d.pos.get(), sizeof(int), n, f);
        printf("ok: %s n %d B %d nb %d nsteps %d packets %d EP %d EXT %d levels %d unit %d\n", side, n, d.B, d.nb,
               d.nsteps, d.npk, d.ep, d.ext, d.nlevels, d.unit);
    }
    fclose(f);
    return 0;
}
