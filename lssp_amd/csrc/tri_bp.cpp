// tri_bp.cpp -- host setup of the block-pipelined triangular sweeps
// (k_tri_pk6, trisolve.hip).
//
// The factor's rows, in sweep order (q = r for L, q = n-1-r for U), are cut
// into contiguous blocks of B rows with B >= the factor's bandwidth, so every
// dependency of a row lies in its own block or in earlier ones.  One
// workgroup takes a block and walks it level by level ("steps"); values it
// needs from its own block come from an LDS ring of recent results, values
// from earlier blocks from HBM, where value-as-flag (TRI_SENTINEL) makes a
// not-yet-written value visible as such.  Only one cross-CU hand-off per block
// boundary is on the critical path instead of one per level.  The per-row
// arithmetic is untouched (entries in the reference's order), so the sweep
// stays bitwise.
#include <algorithm>
#include <cstring>

#include "internal.h"
#include "sched_host.h"

namespace lssp_amd {

// The schedule itself -- block order, steps, entries in summation order and the
// v6 packets (desc / record / index streams, layout in sched_host.h's
// packets6_host) -- is computed by bp_schedule_host (sched_host.h, no HIP);
// here it is uploaded.  tri_sched.hip builds the same bytes on the device.
int build_bp_schedule(lssp_amd_ctx *c, int n, const std::vector<int> &Tp, const std::vector<int> &Tj,
                      const std::vector<double> &Tx, bool upper, const std::vector<int> &lev, TriSched &t,
                      const TriSched *prod)
{
    (void)c;
    if (n <= 0) return LSSP_AMD_OK;
    SetupTimer tm;
    const char *side = upper ? "U" : "L";
    std::string nm;
    auto mark = [&](const char *what) {
        nm = std::string(side) + " " + what;
        tm.mark(nm.c_str());
    };
    HostSched h;
    LSSP_TRY(bp_schedule_host(n, Tp, Tj, Tx, upper, lev, prod ? &prod->h_pos : nullptr, h, mark));
    auto up = [](auto *&d, const auto *src, size_t cnt) -> int {
        using T = typename std::remove_const<typename std::remove_pointer<decltype(src)>::type>::type;
        LSSP_HIP(hipMalloc(&d, sizeof(T) * std::max<size_t>(cnt, 1)));
        if (cnt) LSSP_HIP(hipMemcpy(d, src, sizeof(T) * cnt, hipMemcpyHostToDevice));
        return LSSP_AMD_OK;
    };
    if (h.npk < 0) t.pk6_n = -1;  // a row longer than the longest record: the sync-free sweep serves the factor
    else {
        SetupTimer tu;
        t.pk6_n = h.npk;
        t.pk6_ep = h.ep;
        t.pk6_ext = h.ext;
        t.pk6_rows = h.rows;
        t.pk6_nrec = (long)h.rec.size();
        t.pk6_nidx = (long)h.idx.size();
        LSSP_TRY(up(t.pk6_blk, h.blk.data(), h.blk.size()));
        LSSP_TRY(up(t.pk6_desc, h.desc.data(), h.desc.size()));
        LSSP_TRY(up(t.pk6_rec, h.rec.data(), h.rec.size()));
        LSSP_TRY(up(t.pk6_idx, h.idx.data(), h.idx.size()));
        tu.mark("packet upload");
        LSSP_HIP(hipMalloc(&t.pk6_claim, sizeof(unsigned long long)));
        LSSP_HIP(hipMemset(t.pk6_claim, 0, sizeof(unsigned long long)));
        t.pk6_base = 0;
    }
    if (!upper) t.h_pos = h.pos;
    mark("packets (incl. upload)");
    t.bp_B = h.B;
    t.upper = upper;
    t.bp_nb = h.nb;
    t.bp_nsteps = h.nsteps;
    t.bp_unit = h.unit;
    t.bp_origin = 0;
    LSSP_TRY(up(t.bp_perm, h.perm.data(), h.perm.size()));  // position -> row: the apply's permutation kernels
    LSSP_TRY(up(t.bp_pos, h.pos.data(), h.pos.size()));     // row -> position: x back to natural order as a gather
    mark("permutation upload");
    return LSSP_AMD_OK;
}

}  // namespace lssp_amd
