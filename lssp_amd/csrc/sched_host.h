// sched_host.h -- the pure-host part of the block-pipelined schedule build
// (tri_bp.cpp): everything build_bp_schedule and build_packets6 compute before
// their uploads, into a plain struct of vectors.  No HIP header: tri_bp.cpp
// calls these and uploads; tools/sched_dev_check.cpp compares the device
// builder's lane-level bodies (sched_dev.h) with them byte for byte.
#pragma once

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/lssp_amd.h"
#include "sched_dev.h"

namespace lssp_amd {

// [0, n) cut into contiguous ranges, one thread each (capi.cpp; the check tool has a serial one)
void parallel_for(long n, const std::function<void(long, long)> &f, long grain);

// a vector whose resize() leaves new elements uninitialised: the multi-GB
// streams are written once, by the block threads
template <typename T>
struct SchedNoInit : std::allocator<T> {
    template <typename U>
    struct rebind {
        using other = SchedNoInit<U>;
    };
    template <typename U, typename... A>
    void construct(U *p, A &&...a)
    {
        if constexpr (sizeof...(A) == 0) ::new ((void *)p) U;
        else ::new ((void *)p) U(std::forward<A>(a)...);
    }
};
template <typename T>
using SchedRaw = std::vector<T, SchedNoInit<T>>;

struct HostSched {
    int B = 0, nb = 0, nsteps = 0, unit = 0;
    std::vector<int> perm, pos;  // schedule position -> row, row -> schedule position
    // packets v6; npk < 0: a row longer than the longest record (no packet schedule)
    int npk = 0, ep = 4, ext = 2, rows = 256;
    std::vector<int> blk;      // [nb + 1] first packet of each block
    SchedRaw<int> desc;        // [max(4 npk, 1)]
    SchedRaw<uint32_t> rec;    // record words + 4 trailing zero words
    SchedRaw<int> idx;         // index words + a trailing 0
    long cnt_ext[3] = {0, 0, 0};  // packets at EXT = 2, 3, 4 (-1: not counted)
};

using SchedMark = std::function<void(const char *)>;

inline int packets6_host(int n, const std::vector<int> &perm, const std::vector<int> &pos, const std::vector<int> &rp,
                         const int *cols, const double *vals, const std::vector<double> &diag, bool unit,
                         const std::vector<int> &step_pos, const std::vector<int> &blk_step, int nb, long B,
                         const std::vector<int> &rhs_index, HostSched &t)
{
    const int ROWS = 256;  // rows per packet = compute lanes (512 measured slower)
    int maxlen = 0;
    for (int p = 0; p < n; p++) maxlen = std::max(maxlen, rp[p + 1] - rp[p]);
    if (maxlen > 24) return LSSP_AMD_EUNSUPPORTED;  // ILUT(tol, p <= 24), ILU(k) of stencils
    const int EP = maxlen <= 4 ? 4 : maxlen <= 8 ? 8 : maxlen <= 16 ? 16 : 24;
    // record words of a packet of n rows (C, V, D, ROW, each padded to 4 words);
    // EP >= 16 records are staged through a 16 KB LDS slot (trisolve.hip LREC)
    auto rec_words = [&](long nrow) {
        auto p4 = [](long w) { return (w + 3) & ~3L; };
        return p4((long)(EP / 2) * nrow) + 2L * EP * nrow + p4(2 * nrow) + p4(nrow);
    };
    auto pack = [](int a, int b) { return (uint32_t)((a & 0xffff) | ((uint32_t)(b & 0xffff) << 16)); };
    // blocks are independent: each thread builds its blocks' packets with
    // block-relative record / index offsets and its own operand stamps; the
    // blocks are then laid out in order and the offsets made absolute
    struct BlkPk {
        std::vector<int> desc;
        std::vector<uint32_t> rec;
        std::vector<int> idx;
    };
    // The HBM operands a packet may gather (xcap = EXT x 256: the loader lanes
    // fetch EXT each).  A packet is closed early when its rows' new operands
    // would pass the cap, so a small cap splits levels into several packets,
    // and every packet is a step of its block (7-pt 256^3 ILUT: 512 split 1,580
    // levels into 2,546 packets per block, profiles/r06/r06k_*; the U factor
    // needs 1,024).  Each extra load per lane costs the step ~3 %, so the
    // packets are first counted for EXT = 2, 3, 4 and the smallest EXT whose
    // count is within 1 % of EXT = 4's is kept.
    auto packets_at = [&](int cap) {
        std::atomic<long> total{0};
        parallel_for(nb, [&](long b0, long b1) {
            std::vector<int> stamp(n, -1);
            int pid = 0;
            long cnt = 0;
            for (long b = b0; b < b1; b++)
                for (int s = blk_step[b]; s < blk_step[b + 1]; s++) {
                    int p = step_pos[s];
                    while (p < step_pos[s + 1]) {
                        int nr = 0, nx = 0;
                        while (p + nr < step_pos[s + 1] && nr < ROWS) {
                            const int r = p + nr;
                            if (EP >= 16 && rec_words(nr + 1) > 4 * PK6_REC_WORDS16) break;
                            int newx = 0;
                            for (int k = rp[r]; k < rp[r + 1]; k++)
                                if (cols[k] >= 0 && stamp[cols[k]] != pid) newx++;
                            if (nx + newx > cap) break;
                            for (int k = rp[r]; k < rp[r + 1]; k++)
                                if (cols[k] >= 0 && stamp[cols[k]] != pid) stamp[cols[k]] = pid, nx++;
                            nr++;
                        }
                        p += nr;
                        pid++;
                        cnt++;
                    }
                }
            total += cnt;
        }, 1);
        return total.load();
    };
    int ext = PK3_EXT;
    t.cnt_ext[0] = t.cnt_ext[1] = -1;
    {
        const long c4 = packets_at(ROWS * PK3_EXT);
        t.cnt_ext[2] = c4;
        for (int e = 2; e < PK3_EXT; e++) {
            const long ce = packets_at(ROWS * e);
            t.cnt_ext[e - 2] = ce;
            if (ce <= c4 + c4 / 100) {
                ext = e;
                break;
            }
        }
    }
    const int xcap = ROWS * ext;
    std::vector<BlkPk> bp(nb);
    std::atomic<int> status{LSSP_AMD_OK};
    parallel_for(nb, [&](long b0, long b1) {
        std::vector<int> stamp(n, -1), slot(n, 0), xl;
        int pid = 0;
        for (long b = b0; b < b1 && status.load() == LSSP_AMD_OK; b++) {
            std::vector<int> &desc = bp[b].desc, &idx = bp[b].idx;
            std::vector<uint32_t> &rec = bp[b].rec;
            {
                // the block's packets at most: one per row, each array padded by
                // < 4 words -- reserved so the multi-MB vectors never regrow
                const long rows = std::min<long>((b + 1) * B, n) - b * B;
                const int steps = blk_step[b + 1] - blk_step[b];
                rec.reserve((size_t)(rows * ((EP / 2) + 2 * EP + 3) + 12L * (rows / 8 + steps + 1)));
                idx.reserve((size_t)(rows * (1 + PK3_EXT) + 8));
                desc.reserve((size_t)4 * (rows / 8 + steps + 1));
            }
            static_assert(pk6_xs_off(BP_RING + 1, 1, ROWS * PK3_EXT - 1) <= 0xffff, "16-bit operand offsets");
            for (int s = blk_step[b]; s < blk_step[b + 1]; s++) {
                int p = step_pos[s];
                while (p < step_pos[s + 1]) {
                    int nr = 0, emax = 0;
                    xl.clear();
                    while (p + nr < step_pos[s + 1] && nr < ROWS) {
                        const int r = p + nr;
                        if (EP >= 16 && rec_words(nr + 1) > 4 * PK6_REC_WORDS16) break;  // LDS record slot
                        int newx = 0;
                        for (int k = rp[r]; k < rp[r + 1]; k++)
                            if (cols[k] >= 0 && stamp[cols[k]] != pid) newx++;
                        if ((long)xl.size() + newx > (long)xcap) break;
                        for (int k = rp[r]; k < rp[r + 1]; k++) {
                            const int g = cols[k];
                            if (g >= 0 && stamp[g] != pid) {
                                stamp[g] = pid;
                                slot[g] = (int)xl.size();
                                xl.push_back(g);
                            }
                        }
                        emax = std::max(emax, rp[r + 1] - rp[r]);
                        nr++;
                    }
                    const int nx = (int)xl.size();
                    const int par = (int)(desc.size() / 4) & 1;  // the packet's index in its block, mod 2
                    const long ro = (long)rec.size() / 4, io = (long)idx.size();  // block-relative
                    desc.push_back((int)ro);
                    desc.push_back((int)io);
                    desc.push_back(nr | (nx << 10) | (emax << 21));
                    desc.push_back(p);
                    // C: (EP/2) words per row, V: 2*EP, D: 2, ROW: 1 -- each array padded to 4 words
                    auto pad4 = [](long w) { return (w + 3) & ~3L; };
                    const long wc = pad4((long)(EP / 2) * nr), wv = 2L * EP * nr, wd = pad4(2L * nr), wr = pad4(nr);
                    rec.resize(rec.size() + wc + wv + wd + wr, 0u);
                    uint32_t *w = rec.data() + 4 * ro;
                    double *V = reinterpret_cast<double *>(w + wc);
                    double *D = V + (long)EP * nr;
                    uint32_t *ROW = w + wc + wv + wd;
                    for (int r = 0; r < nr; r++) {
                        const int k0 = rp[p + r], len = rp[p + r + 1] - k0;
                        int cc[24];
                        for (int e = 0; e < 24; e++) cc[e] = pk6_xs_off(BP_RING, 0, 0);  // the +0.0 pad slot
                        for (int e = 0; e < len; e++) {
                            const int g = cols[k0 + e];
                            cc[e] = g < 0 ? pk6_xs_off(-1 - g, 0, 0) : pk6_xs_off(BP_RING + 1, par, slot[g]);
                            V[2L * ((long)(e / 2) * nr + r) + (e & 1)] = vals[k0 + e];
                        }
                        for (int q = 0; q < EP / 2; q++) w[(long)(EP / 2) * r + q] = pack(cc[2 * q], cc[2 * q + 1]);
                        D[r] = unit ? 1.0 : diag[p + r];
                        ROW[r] = (uint32_t)perm[p + r];
                    }
                    for (int r = 0; r < nr; r++) idx.push_back(rhs_index[perm[p + r]]);
                    for (int x = 0; x < nx; x++) idx.push_back(pos[xl[x]]);
                    p += nr;
                    pid++;
                }
            }
            if ((int)desc.size() / 4 > PK3_CAP) status = LSSP_AMD_EUNSUPPORTED;
        }
    }, 1);
    if (status.load() != LSSP_AMD_OK) return status.load();
    // lay the blocks out in order; offsets absolute
    std::vector<int> &blk = t.blk;
    blk.assign(nb + 1, 0);
    std::vector<long> rec_off(nb + 1, 0), idx_off(nb + 1, 0);
    for (int b = 0; b < nb; b++) {
        blk[b + 1] = blk[b] + (int)bp[b].desc.size() / 4;
        rec_off[b + 1] = rec_off[b] + (long)bp[b].rec.size();
        idx_off[b + 1] = idx_off[b] + (long)bp[b].idx.size();
    }
    if (rec_off[nb] / 4 > INT_MAX || idx_off[nb] > INT_MAX) return LSSP_AMD_EUNSUPPORTED;
    // the blocks laid out in order (offsets made absolute) in uninitialised
    // host arrays, filled by the block threads in parallel -- no single-thread
    // zero fill of the multi-GB record stream
    t.npk = blk[nb];
    t.ep = EP;
    t.ext = ext;
    t.rows = ROWS;
    const size_t ndesc = std::max<size_t>(4L * blk[nb], 1), nrec = rec_off[nb] + 4, nidx = idx_off[nb] + 1;
    t.desc.resize(ndesc);
    t.rec.resize(nrec);
    t.idx.resize(nidx);
    int *desc = t.desc.data(), *idx = t.idx.data();
    uint32_t *rec = t.rec.data();
    std::fill(rec + rec_off[nb], rec + nrec, 0u);  // the kernels' whole-unit reads past the end
    idx[nidx - 1] = 0;
    desc[0] = 0;
    parallel_for(nb, [&](long b0, long b1) {
        for (long b = b0; b < b1; b++) {
            BlkPk &k = bp[b];
            int *d = desc + 4L * blk[b];
            for (size_t e = 0; e < k.desc.size(); e += 4) {
                d[e] = k.desc[e] + (int)(rec_off[b] / 4);
                d[e + 1] = k.desc[e + 1] + (int)idx_off[b];
                d[e + 2] = k.desc[e + 2];
                d[e + 3] = k.desc[e + 3];
            }
            std::copy(k.rec.begin(), k.rec.end(), rec + rec_off[b]);
            std::copy(k.idx.begin(), k.idx.end(), idx + idx_off[b]);
            k = BlkPk();  // the block's host copy is done with
        }
    }, 1);
    return LSSP_AMD_OK;
}

// rhs_pos: the L sweep's row -> position array for the U factor (nullptr: the factor's own)
inline int bp_schedule_host(int n, const std::vector<int> &Tp, const std::vector<int> &Tj, const std::vector<double> &Tx,
                            bool upper, const std::vector<int> &lev, const std::vector<int> *rhs_pos, HostSched &t,
                            const SchedMark &mark)
{
    auto Q = [&](int r) { return upper ? n - 1 - r : r; };
    auto strict_begin = [&](int i) { return upper ? Tp[i] + 1 : Tp[i]; };
    auto strict_end = [&](int i) { return upper ? Tp[i + 1] : Tp[i + 1] - 1; };
    bool unit = true;
    int bw = 1;
    {
        std::mutex mu;
        parallel_for(n, [&](long i0, long i1) {
            bool u = true;
            int w = 1;
            for (long i = i0; i < i1; i++) {
                u &= (upper ? Tx[Tp[i]] : Tx[Tp[i + 1] - 1]) == 1.0;
                for (int k = strict_begin((int)i); k < strict_end((int)i); k++) w = std::max(w, std::abs((int)i - Tj[k]));
            }
            std::lock_guard<std::mutex> g(mu);
            unit &= u;
            bw = std::max(bw, w);
        }, 4096);
    }
    mark("bandwidth");
    long B = std::max(64L, (long)bw);  // one bandwidth per block: measured best
    if (B > n) B = n;
    const int nb = (int)((n + B - 1) / B);

    // rows of each block ordered by (level, q); blocks are independent (threads),
    // their step lists are concatenated in block order
    std::vector<int> &perm = t.perm, &pos = t.pos;
    perm.assign(n, 0);
    pos.assign(n, 0);
    std::vector<std::vector<int>> bsp(nb), bsl(nb);
    parallel_for(nb, [&](long b0, long b1) {
        for (long b = b0; b < b1; b++) {
            const long q0 = b * B, q1 = std::min<long>(q0 + B, n);
            int lmin = INT_MAX, lmax = 0;
            for (long q = q0; q < q1; q++) {
                const int r = upper ? n - 1 - (int)q : (int)q;
                lmin = std::min(lmin, lev[r]);
                lmax = std::max(lmax, lev[r]);
            }
            std::vector<int> cnt(lmax - lmin + 2, 0);
            for (long q = q0; q < q1; q++) cnt[lev[upper ? n - 1 - (int)q : (int)q] - lmin + 1]++;
            for (size_t l = 1; l < cnt.size(); l++) cnt[l] += cnt[l - 1];
            for (int l = 0; l <= lmax - lmin; l++)
                if (cnt[l + 1] > cnt[l]) {
                    bsp[b].push_back((int)q0 + cnt[l]);
                    bsl[b].push_back(l + lmin);
                }
            for (long q = q0; q < q1; q++) {
                const int r = upper ? n - 1 - (int)q : (int)q;
                const int p = (int)q0 + cnt[lev[r] - lmin]++;
                perm[p] = r;
                pos[r] = p;
            }
        }
    }, 1);
    mark("block level order");
    std::vector<int> step_pos, blk_step(nb + 1, 0);
    for (int b = 0; b < nb; b++) {
        blk_step[b] = (int)step_pos.size();
        step_pos.insert(step_pos.end(), bsp[b].begin(), bsp[b].end());
    }
    const int nsteps = (int)step_pos.size();
    blk_step[nb] = nsteps;
    step_pos.push_back(n);
    std::vector<int> step_of(n);
    parallel_for(nsteps, [&](long s0, long s1) {
        for (long s = s0; s < s1; s++)
            for (int p = step_pos[s]; p < step_pos[s + 1]; p++) step_of[p] = (int)s;
    }, 64);

    // entries in summation order; intra-block dependencies still inside the
    // ring window come from LDS (code -1 - slot), everything else from HBM
    std::vector<int> rp(n + 1, 0);
    for (int p = 0; p < n; p++) rp[p + 1] = rp[p] + strict_end(perm[p]) - strict_begin(perm[p]);
    // uninitialised: every slot is written below, by the position threads
    std::unique_ptr<int[]> cols(new int[std::max(rp[n], 1)]);
    std::unique_ptr<double[]> vals(new double[std::max(rp[n], 1)]);
    std::vector<double> diag;
    if (!unit) diag.resize(n);
    parallel_for(n, [&](long p0, long p1) {
        for (long p = p0; p < p1; p++) {
            const int i = perm[p], b = (int)(Q(i) / B), s = step_of[p];
            int o = rp[p];
            auto take = [&](int k) {
                const int j = Tj[k];
                const int bj = (int)(Q(j) / B);
                int code = j;
                if (bj == b) {
                    const int pd = pos[j];
                    if (step_pos[s + 1] - pd <= BP_RING) code = -1 - (int)((pd - (long)b * B) % BP_RING);
                }
                cols[o] = code;
                vals[o] = Tx[k];
                o++;
            };
            if (!upper)
                for (int k = Tp[i]; k < Tp[i + 1] - 1; k++) take(k);
            else
                for (int k = Tp[i + 1] - 1; k > Tp[i]; k--) take(k);
            if (!unit) diag[p] = upper ? Tx[Tp[i]] : Tx[Tp[i + 1] - 1];
        }
    }, 4096);
    mark("entries in sweep order");
    int st6;
    {
        // v6 packets; the rhs of the U sweep is the L sweep's output, read in
        // L's schedule order (the L sweep's rhs is permuted into L order first)
        std::vector<int> rhs_index(n);
        parallel_for(n, [&](long r0, long r1) {
            for (long r = r0; r < r1; r++) rhs_index[r] = rhs_pos && !rhs_pos->empty() ? (*rhs_pos)[r] : pos[r];
        }, 4096);
        st6 = packets6_host(n, perm, pos, rp, cols.get(), vals.get(), diag, unit, step_pos, blk_step, nb, B, rhs_index, t);
        // a row longer than the longest record: the sync-free sweep serves the factor
        if (st6 == LSSP_AMD_EUNSUPPORTED) t.npk = -1;
        else if (st6 != LSSP_AMD_OK) return st6;
    }
    t.B = (int)B;
    t.nb = nb;
    t.nsteps = nsteps;
    t.unit = unit ? 1 : 0;
    return LSSP_AMD_OK;
}

}  // namespace lssp_amd
