// bilu_factor.hip -- BILUK on the GPU: the numeric block ILU(0) and the middle
// stage of the apply.
//
// k_bilu0_level restates lssp_pc_bilu0_fac (pc-biluk.cxx:198-277) on the
// arithmetic of bilu_dev.h, scheduled as ilu_factor.hip schedules k_ilu0_level:
// block row i only reads block rows Bj[k] < i of its own strict-lower pattern,
// so the host computes the levels of that DAG and every level is one launch --
// no spin-waits, no hand-off between workgroups.
//   for each strict-lower block k of block row i, ascending:
//       a_ik = a_ik * inv_k                                         (:234-235)
//       a_ij = a_ij - a_ik * a_kj  for j > k that block row k holds (:242-248)
//   inv_i = a_ii^-1; the identity when the row has no diagonal block (:255-270)
// One wave (a 64-lane workgroup) owns a block row, lane t = c*BS + r owns entry
// (r, c) of every block of the row.  An entry of a block product is an
// independent in-order sum over l (bilu_gemm_entry), so the lanes reproduce
// the host loop bit for bit.  The row's own a_ik is staged in LDS for the
// lanes of the other columns; a_kj and inv_k come from rows finished in
// earlier launches.  The inverse is the sequential bilu_inverse on the LDS copy
// of the diagonal block, run by lane 0 (LDS is dynamically indexable; a
// private double[64] would live in scratch).  A singular block raises *flag
// and stores zeros, so later rows stay inside their arrays.
//
// lssp_amd_bilu_refactor (second half of the file) runs the same
// launches on buffers that stay on the device: A's values scattered into the
// kept block pattern, the block graph compared, k_bilu0_level, the U blocks
// scaled, the packet records refilled (trisolve.hip k_pk6_refill).
//
// lssp_amd_bilu_create_dev (third part) makes the handle from a
// matrix in HBM: the block graph (k_bilu_graph), the symbolic ILU(k) of that
// graph and its level lists (iluk_symbolic.hip, unchanged), the refactor's own
// scatter / numeric / commit launches on a plan filled on the device, and the
// expansion of the committed blocks to the point factors (k_bilu_expand) that
// the device schedule builder reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "bilu_create_dev.h"
#include "bilu_dev.h"
#include "bilu_refactor_dev.h"
#include "internal.h"

namespace lssp_amd {

template <int BS>
__global__ __launch_bounds__(64) void k_bilu0_level(const int *__restrict__ rows, int cnt, const int *__restrict__ Bp,
                                                    const int *__restrict__ Bj, double *Bx, double *inv, int *flag)
{
    constexpr int BS2 = BS * BS;
    __shared__ double s_aik[BS2];
    __shared__ double s_d[BS2];
    __shared__ int s_piv[BS];
    __shared__ int s_sing;
    if ((int)blockIdx.x >= cnt) return;
    const int t = threadIdx.x;
    const bool act = t < BS2;
    const int r = t % BS, c = t / BS;
    const int i = rows[blockIdx.x];
    const int s = Bp[i], end = Bp[i + 1];
    int k = s;
    for (; k < end && Bj[k] < i; k++) {  // uniform over the workgroup
        const int idx = Bj[k];
        double *aik = Bx + (size_t)k * BS2;
        if (act) s_aik[t] = aik[t];
        __syncthreads();
        double v = 0.;
        if (act) v = bilu_gemm_entry(s_aik, inv + (size_t)idx * BS2, 1., s_aik[t], 0., BS, r, c);
        __syncthreads();
        if (act) {
            s_aik[t] = v;
            aik[t] = v;
        }
        __syncthreads();
        int q = Bp[idx];
        const int qe = Bp[idx + 1];
        for (int j = k + 1; j < end; j++) {
            const int col = Bj[j];
            while (q < qe && Bj[q] < col) q++;
            if (q < qe && Bj[q] == col && act) {
                double *aij = Bx + (size_t)j * BS2;
                aij[t] = bilu_gemm_entry(s_aik, Bx + (size_t)q * BS2, -1., aij[t], 1., BS, r, c);
            }
        }
        __syncthreads();  // s_aik is rewritten by the next k
    }
    double *d = inv + (size_t)i * BS2;
    if (k < end && Bj[k] == i) {
        if (act) s_d[t] = Bx[(size_t)k * BS2 + t];
        __syncthreads();
        if (t == 0) s_sing = bilu_inverse(s_d, BS, s_piv);
        __syncthreads();
        if (s_sing) {
            if (act) d[t] = 0.;
            if (t == 0) atomicOr(flag, 1);
        } else if (act) {
            d[t] = s_d[t];
        }
    } else if (act) {
        d[t] = r == c ? 1. : 0.;
    }
}

// z = D y of the apply (lssp_pc_bilu_solve, pc-biluk.cxx:48), one lane per row,
// summed as lssp_mv_mxy sums a row of D (mvops.cxx:118-135): from 0.0, adding
// y[i*bs + c] * inv_i(r, c) for c = 0 .. bs-1.  POS: y and z are indexed through
// pos[row] (the packet sweeps' schedule-ordered shadows; y is only read).
template <int BS, bool POS>
__global__ __launch_bounds__(256) void k_bdiag(int n, const double *__restrict__ Dinv, const int *__restrict__ pos,
                                               const double *__restrict__ y, double *__restrict__ z)
{
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const long blk = row / BS;
    const int r = (int)(row - blk * BS);
    const double *inv = Dinv + blk * BS * BS;
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < BS; c++) {
        const long col = blk * BS + c;
        s = s + inv[r + c * BS] * y[POS ? pos[col] : col];
    }
    z[POS ? pos[row] : row] = s;
}

// any block size (bs > 8 factors come from the host numeric path)
template <bool POS>
__global__ __launch_bounds__(256) void k_bdiag_n(int n, int bs, const double *__restrict__ Dinv,
                                                 const int *__restrict__ pos, const double *__restrict__ y,
                                                 double *__restrict__ z)
{
    const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    const long blk = row / bs;
    const int r = (int)(row - blk * bs);
    const double *inv = Dinv + blk * bs * bs;
    double s = 0.0;
    for (int c = 0; c < bs; c++) {
        const long col = blk * bs + c;
        s = s + inv[r + c * bs] * y[POS ? pos[col] : col];
    }
    z[POS ? pos[row] : row] = s;
}

template <bool POS>
static void bdiag_launch(lssp_amd_ctx *c, int n, int bs, const double *Dinv, const int *pos, const double *y,
                         double *z)
{
    const int grid = (n + 255) / 256;
    switch (bs) {
#define LSSP_BDIAG(B)                                                          \
    case B:                                                                    \
        k_bdiag<B, POS><<<grid, 256, 0, c->stream>>>(n, Dinv, pos, y, z); \
        break;
        LSSP_BDIAG(1)
        LSSP_BDIAG(2)
        LSSP_BDIAG(3)
        LSSP_BDIAG(4)
        LSSP_BDIAG(5)
        LSSP_BDIAG(6)
        LSSP_BDIAG(7)
        LSSP_BDIAG(8)
#undef LSSP_BDIAG
    default:
        k_bdiag_n<POS><<<grid, 256, 0, c->stream>>>(n, bs, Dinv, pos, y, z);
    }
}

int launch_bdiag(lssp_amd_ctx *c, int n, int bs, const double *Dinv, const int *pos, const double *y, double *z)
{
    if (n <= 0) return LSSP_AMD_OK;
    if (bs < 1 || n % bs != 0 || y == z) return LSSP_AMD_EINVAL;
    if (pos) bdiag_launch<true>(c, n, bs, Dinv, pos, y, z);
    else bdiag_launch<false>(c, n, bs, Dinv, pos, y, z);
    LSSP_HIP(hipGetLastError());
    return LSSP_AMD_OK;
}

void bilu_levels(int nb, const std::vector<int> &Bp, const std::vector<int> &Bj, std::vector<int> &off,
                 std::vector<int> &rows)
{
    std::vector<int> lev(nb, 0);
    int nlev = 0;
    for (int i = 0; i < nb; i++) {
        int l = 0;
        for (int k = Bp[i]; k < Bp[i + 1] && Bj[k] < i; k++) l = std::max(l, lev[Bj[k]] + 1);
        lev[i] = l;
        nlev = std::max(nlev, l + 1);
    }
    off.assign(nlev + 1, 0);
    rows.resize(nb);
    for (int i = 0; i < nb; i++) off[lev[i] + 1]++;
    for (int l = 0; l < nlev; l++) off[l + 1] += off[l];
    std::vector<int> fill(off.begin(), off.end() - 1);
    for (int i = 0; i < nb; i++) rows[fill[lev[i]]++] = i;
}

// k_bilu0_level<bs> over the level lists, one launch per level: the create's and
// the refactor's numeric factorization are these same launches
static void bilu0_launch_levels(lssp_amd_ctx *c, int bs, const std::vector<int> &off, const int *d_rows,
                                const int *d_Bp, const int *d_Bj, double *d_Bx, double *d_inv, int *d_flag)
{
    const int nlev = (int)off.size() - 1;
    for (int l = 0; l < nlev; l++) {
        const int cnt = off[l + 1] - off[l];
        const int *rl = d_rows + off[l];
        switch (bs) {
#define LSSP_BILU0(B)                                                                                  \
    case B:                                                                                            \
        k_bilu0_level<B><<<cnt, 64, 0, c->stream>>>(rl, cnt, d_Bp, d_Bj, d_Bx, d_inv, d_flag); \
        break;
            LSSP_BILU0(1)
            LSSP_BILU0(2)
            LSSP_BILU0(3)
            LSSP_BILU0(4)
            LSSP_BILU0(5)
            LSSP_BILU0(6)
            LSSP_BILU0(7)
            LSSP_BILU0(8)
#undef LSSP_BILU0
        }
    }
}

// In place on the host BCSR (block columns ascending): upload, one launch per
// level, download of the blocks and the inverted diagonal blocks.
int bilu0_factor_gpu(lssp_amd_ctx *c, HostBCSR &T, std::vector<double> &inv)
{
    const int nb = T.nb, bs = T.bs, bs2 = bs * bs;
    if (bs < 1 || bs > BILU_MAX_BS_DEV) return LSSP_AMD_EINVAL;
    inv.assign((size_t)nb * bs2, 0.0);
    if (nb <= 0) return LSSP_AMD_OK;
    const size_t nblk = T.Bj.size();
    std::vector<int> off, rows;
    bilu_levels(nb, T.Bp, T.Bj, off, rows);
    const int nlev = (int)off.size() - 1;
    int *d_Bp = nullptr, *d_Bj = nullptr, *d_rows = nullptr, *d_flag = nullptr;
    double *d_Bx = nullptr, *d_inv = nullptr;
    int st = LSSP_AMD_OK, flag = 0;
    auto fail = [&](hipError_t e) {
        if (e != hipSuccess && st == LSSP_AMD_OK) {
            fprintf(stderr, "lssp_amd: HIP error %s in bilu0_factor_gpu\n", hipGetErrorString(e));
            st = LSSP_AMD_EHIP;
        }
    };
    fail(hipMalloc(&d_Bp, sizeof(int) * (nb + 1)));
    fail(hipMalloc(&d_Bj, sizeof(int) * std::max<size_t>(nblk, 1)));
    fail(hipMalloc(&d_Bx, sizeof(double) * std::max<size_t>(nblk * bs2, 1)));
    fail(hipMalloc(&d_rows, sizeof(int) * nb));
    fail(hipMalloc(&d_inv, sizeof(double) * (size_t)nb * bs2));
    fail(hipMalloc(&d_flag, sizeof(int)));
    if (st == LSSP_AMD_OK) {
        fail(hipMemcpyAsync(d_Bp, T.Bp.data(), sizeof(int) * (nb + 1), hipMemcpyHostToDevice, c->stream));
        fail(hipMemcpyAsync(d_Bj, T.Bj.data(), sizeof(int) * nblk, hipMemcpyHostToDevice, c->stream));
        fail(hipMemcpyAsync(d_Bx, T.Bx.data(), sizeof(double) * nblk * bs2, hipMemcpyHostToDevice, c->stream));
        fail(hipMemcpyAsync(d_rows, rows.data(), sizeof(int) * nb, hipMemcpyHostToDevice, c->stream));
        fail(hipMemsetAsync(d_flag, 0, sizeof(int), c->stream));
    }
    const bool times = setup_times_on();
    if (times && st == LSSP_AMD_OK) fail(hipStreamSynchronize(c->stream));
    const double t0 = wall_time();
    if (st == LSSP_AMD_OK) {
        bilu0_launch_levels(c, bs, off, d_rows, d_Bp, d_Bj, d_Bx, d_inv, d_flag);
        fail(hipGetLastError());
        if (times) {
            fail(hipStreamSynchronize(c->stream));
            fprintf(stderr, "lssp_amd setup:   BILU(0) numeric kernels, %d levels %10.6f s\n", nlev, wall_time() - t0);
        }
        fail(hipMemcpyAsync(T.Bx.data(), d_Bx, sizeof(double) * nblk * bs2, hipMemcpyDeviceToHost, c->stream));
        fail(hipMemcpyAsync(inv.data(), d_inv, sizeof(double) * (size_t)nb * bs2, hipMemcpyDeviceToHost, c->stream));
        fail(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        fail(hipStreamSynchronize(c->stream));
    }
    for (void *p : {(void *)d_Bp, (void *)d_Bj, (void *)d_Bx, (void *)d_rows, (void *)d_inv, (void *)d_flag})
        if (p) (void)hipFree(p);
    if (st == LSSP_AMD_OK && flag) st = LSSP_AMD_EINVAL;  // singular diagonal block
    return st;
}

// ---------------------------------------------------------------------------
// lssp_amd_bilu_refactor: new values on the kept block pattern, on buffers
// that stay on the device (BiluPlan, internal.h)
// ---------------------------------------------------------------------------
// A's rows into the zeroed block buffer.  One row per lane: a row's entries have
// to be placed one after the other (the last of a duplicated column wins), so a
// wave that owned one block row could keep only its bs <= 8 rows' lanes busy;
// with a row per lane all 64 work, the rows of a wave are neighbours, so their
// entries share cache lines from one loop trip to the next, and the bs rows of
// a block row search the same few Bj words.  Rows of one block row write
// different entries of its blocks; the hit marks are idempotent byte stores.
__global__ __launch_bounds__(256) void k_bilu_scatter(int n, int bs, int nnz, const int *__restrict__ Ap,
                                                      const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                      const int *__restrict__ Bp, const int *__restrict__ Bj,
                                                      double *__restrict__ Bx, unsigned char *__restrict__ hit,
                                                      int *__restrict__ flag)
{
    int bad = 0;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < n; r += (long)gridDim.x * 256)
        bad |= bilu_scatter_row((int)r, n, bs, nnz, Ap, Aj, Ax, Bp, Bj, Bx, hit);
    if (bad) atomicOr(flag, 1);
}

// the pattern rule's second half: the blocks that received an entry are exactly
// the blocks of the creating matrix's graph (a fill block hit, or a graph block
// left empty, would change what a fresh create's symbolic pass gives)
__global__ __launch_bounds__(256) void k_bilu_graph_cmp(long nblk, const unsigned char *__restrict__ hit,
                                                        const unsigned char *__restrict__ in, int *__restrict__ flag)
{
    bool bad = false;
    for (long k = blockIdx.x * 256L + threadIdx.x; k < nblk; k += (long)gridDim.x * 256) bad |= hit[k] != in[k];
    if (bad) atomicOr(flag, 1);
}

// The factored blocks into the committed buffer, one lane per entry: a block
// right of the diagonal as inv_i * a_ij -- bilu_expand's bilu_gemm(inv_i, a_ij,
// 1., cache, 0., bs) entry by entry, the bs == 1 form included -- every other
// block as it is.
template <int BS>
__global__ __launch_bounds__(256) void k_bilu_commit(long nblk, const int *__restrict__ Brow,
                                                     const int *__restrict__ Bj, const double *__restrict__ Bx,
                                                     const double *__restrict__ inv, double *__restrict__ Fx)
{
    constexpr int BS2 = BS * BS;
    const long tot = nblk * BS2;
    for (long g = blockIdx.x * 256L + threadIdx.x; g < tot; g += (long)gridDim.x * 256) {
        const long k = g / BS2;
        const int t = (int)(g - k * BS2), r = t % BS, c = t / BS;
        const int i = Brow[k];
        const double *a = Bx + k * BS2;
        Fx[g] = Bj[k] > i ? bilu_gemm_entry(inv + (size_t)i * BS2, a, 1., 0., 0., BS, r, c) : a[t];
    }
}

static unsigned bilu_grid(long items)
{
    return (unsigned)std::max<long>(1, std::min<long>((items + 255) / 256, 16384));
}

// k_bilu_commit<bs> on the plan's buffers: the refactor's and the device create's
static int bilu_commit_launch(lssp_amd_ctx *c, BiluPlan &p)
{
    const int bs2 = p.bs * p.bs;
    switch (p.bs) {
#define LSSP_BCOMMIT(B)                                                                                      \
    case B:                                                                                                  \
        k_bilu_commit<B><<<bilu_grid(p.nblk * bs2), 256, 0, c->stream>>>(p.nblk, p.d_Brow, p.d_Bj, p.d_Bx, p.d_inv, \
                                                                         p.d_Fx);                            \
        break;
        LSSP_BCOMMIT(1)
        LSSP_BCOMMIT(2)
        LSSP_BCOMMIT(3)
        LSSP_BCOMMIT(4)
        LSSP_BCOMMIT(5)
        LSSP_BCOMMIT(6)
        LSSP_BCOMMIT(7)
        LSSP_BCOMMIT(8)
#undef LSSP_BCOMMIT
    default:
        return LSSP_AMD_EUNSUPPORTED;
    }
    LSSP_HIP(hipGetLastError());
    return LSSP_AMD_OK;
}

void bilu_plan_free(BiluPlan *p)
{
    if (!p) return;
    for (void *q : {(void *)p->d_Bp, (void *)p->d_Bj, (void *)p->d_Brow, (void *)p->d_in, (void *)p->d_hit,
                    (void *)p->d_Bx, (void *)p->d_inv, (void *)p->d_Fx, (void *)p->d_first, (void *)p->d_rows,
                    (void *)p->d_flag})
        if (q) (void)hipFree(q);
    delete p;
}

int bilu_plan_build(lssp_amd_ctx *c, lssp_amd_ilu *M)
{
    if (M->brf) return LSSP_AMD_OK;
    const int bs = M->bs, bs2 = bs * bs, nb = M->n / bs;
    const size_t nblk = M->bBj.size();
    // the refill leaves the records' D at its build-time 1.0: BILUK's L and U
    // store unit diagonals (bilu_expand), and that is what the schedules saw
    for (int i = 0; i < M->n; i++)
        if (M->Lx[M->Lp[i + 1] - 1] != 1.0 || M->Ux[M->Up[i]] != 1.0) return LSSP_AMD_EUNSUPPORTED;
    BiluPlan *p = new BiluPlan();
    p->nb = nb;
    p->bs = bs;
    p->nblk = (long)nblk;
    std::vector<int> rows, brow(nblk), first(nb);
    bilu_levels(nb, M->bBp, M->bBj, p->lev_off, rows);
    for (int i = 0; i < nb; i++) {
        int k = M->bBp[i];
        for (; k < M->bBp[i + 1]; k++) brow[k] = i;
        k = M->bBp[i];
        while (k < M->bBp[i + 1] && M->bBj[k] < i) k++;
        first[i] = k;
    }
    auto fill = [&]() -> int {
        const size_t nz = std::max<size_t>(nblk, 1);
        LSSP_HIP(hipMalloc(&p->d_Bp, sizeof(int) * (nb + 1)));
        LSSP_HIP(hipMalloc(&p->d_Bj, sizeof(int) * nz));
        LSSP_HIP(hipMalloc(&p->d_Brow, sizeof(int) * nz));
        LSSP_HIP(hipMalloc(&p->d_in, nz));
        LSSP_HIP(hipMalloc(&p->d_hit, nz));
        LSSP_HIP(hipMalloc(&p->d_Bx, sizeof(double) * nz * bs2));
        LSSP_HIP(hipMalloc(&p->d_Fx, sizeof(double) * nz * bs2));
        LSSP_HIP(hipMalloc(&p->d_inv, sizeof(double) * (size_t)nb * bs2));
        LSSP_HIP(hipMalloc(&p->d_first, sizeof(int) * nb));
        LSSP_HIP(hipMalloc(&p->d_rows, sizeof(int) * nb));
        LSSP_HIP(hipMalloc(&p->d_flag, sizeof(int) * 2));
        LSSP_HIP(hipMemcpyAsync(p->d_Bp, M->bBp.data(), sizeof(int) * (nb + 1), hipMemcpyHostToDevice, c->stream));
        LSSP_HIP(hipMemcpyAsync(p->d_Bj, M->bBj.data(), sizeof(int) * nblk, hipMemcpyHostToDevice, c->stream));
        LSSP_HIP(hipMemcpyAsync(p->d_Brow, brow.data(), sizeof(int) * nblk, hipMemcpyHostToDevice, c->stream));
        LSSP_HIP(hipMemcpyAsync(p->d_in, M->bIn.data(), nblk, hipMemcpyHostToDevice, c->stream));
        LSSP_HIP(hipMemcpyAsync(p->d_first, first.data(), sizeof(int) * nb, hipMemcpyHostToDevice, c->stream));
        LSSP_HIP(hipMemcpyAsync(p->d_rows, rows.data(), sizeof(int) * nb, hipMemcpyHostToDevice, c->stream));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        return LSSP_AMD_OK;
    };
    const int st = fill();
    if (st != LSSP_AMD_OK) {
        (void)hipGetLastError();
        bilu_plan_free(p);
        return st;
    }
    M->brf = p;
    return LSSP_AMD_OK;
}

int bilu_refactor_device(lssp_amd_ctx *c, lssp_amd_ilu *M, const lssp_amd_mat *A)
{
    PhaseClock clk(c, "bilu_refactor");
    LSSP_TRY(bilu_plan_build(c, M));
    LSSP_TRY(clk.mark("plan"));
    BiluPlan &p = *M->brf;
    const int n = M->n, bs = p.bs, bs2 = bs * bs;
    const long nblk = p.nblk;
    int flag = 0;
    // 1. zero, scatter; 2. graph compare -- on scratch only
    LSSP_HIP(hipMemsetAsync(p.d_Bx, 0, sizeof(double) * std::max<long>(nblk, 1) * bs2, c->stream));
    LSSP_HIP(hipMemsetAsync(p.d_hit, 0, std::max<long>(nblk, 1), c->stream));
    LSSP_HIP(hipMemsetAsync(p.d_flag, 0, sizeof(int) * 2, c->stream));
    k_bilu_scatter<<<bilu_grid(n), 256, 0, c->stream>>>(n, bs, A->nnz, A->Ap, A->Aj, A->Ax, p.d_Bp, p.d_Bj, p.d_Bx,
                                                       p.d_hit, p.d_flag);
    k_bilu_graph_cmp<<<bilu_grid(nblk), 256, 0, c->stream>>>(nblk, p.d_hit, p.d_in, p.d_flag);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipMemcpyAsync(&flag, p.d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (flag) return LSSP_AMD_EINVAL;  // not the block graph M was created from
    LSSP_TRY(clk.mark("scatter + graph compare"));
    // 3. the create's own launches
    bilu0_launch_levels(c, bs, p.lev_off, p.d_rows, p.d_Bp, p.d_Bj, p.d_Bx, p.d_inv, p.d_flag + 1);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipMemcpyAsync(&flag, p.d_flag + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (flag) return LSSP_AMD_EINVAL;  // singular diagonal block
    LSSP_TRY(clk.mark("numeric BILU(0)"));
    // 4. - 6.: the committed values, the record streams, the inverses
    LSSP_TRY(bilu_commit_launch(c, p));
    LSSP_TRY(clk.mark("U scaling"));
    LSSP_TRY(launch_pk6_refill(c, M->lower, false, bs, p.nb, p.d_Bp, p.d_Bj, p.d_first, p.d_Fx));
    LSSP_TRY(launch_pk6_refill(c, M->upper, true, bs, p.nb, p.d_Bp, p.d_Bj, p.d_first, p.d_Fx));
    LSSP_HIP(hipMemcpyAsync(M->d_Dinv, p.d_inv, sizeof(double) * (size_t)p.nb * bs2, hipMemcpyDeviceToDevice,
                            c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    LSSP_TRY(clk.mark("packet refill + Dinv"));
    return LSSP_AMD_OK;
}

// Lx / Ux / Dinv from the committed device values: one download of the block
// buffer and of the inverses, then bilu_expand (the U blocks are scaled already).
// A handle lssp_amd_bilu_create_dev made has no host copies at all yet
// (host_missing): its block pattern and graph flags come down from the plan
// first, and bilu_expand's patterns are kept as well.
int bilu_refactor_host_factors(lssp_amd_ilu *M)
{
    if (!M->host_stale || !M->brf) return LSSP_AMD_OK;
    lssp_amd_ctx *c = M->ctx;
    const BiluPlan &p = *M->brf;
    const size_t nblk = (size_t)p.nblk;
    if (M->host_missing) {
        std::vector<int> Bp((size_t)p.nb + 1), Bj(nblk);
        std::vector<unsigned char> in(nblk);
        LSSP_HIP(hipMemcpyAsync(Bp.data(), p.d_Bp, sizeof(int) * Bp.size(), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipMemcpyAsync(Bj.data(), p.d_Bj, sizeof(int) * nblk, hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipMemcpyAsync(in.data(), p.d_in, nblk, hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        M->bBp = std::move(Bp);
        M->bBj = std::move(Bj);
        M->bIn = std::move(in);
    }
    HostBCSR T;
    T.nb = p.nb;
    T.bs = p.bs;
    T.Bp = M->bBp;
    T.Bj = M->bBj;
    T.Bx.resize(nblk * p.bs * p.bs);
    std::vector<double> inv((size_t)p.nb * p.bs * p.bs);
    LSSP_HIP(hipMemcpyAsync(T.Bx.data(), p.d_Fx, sizeof(double) * T.Bx.size(), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(inv.data(), M->d_Dinv, sizeof(double) * inv.size(), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    HostCSR L, U;
    bilu_expand(T, inv, L, U, true);
    if (M->host_missing) {
        if (L.Ax.size() != (size_t)M->dev_nnzL || U.Ax.size() != (size_t)M->dev_nnzU) return LSSP_AMD_EINVAL;
        M->Lp = std::move(L.Ap);
        M->Lj = std::move(L.Aj);
        M->Up = std::move(U.Ap);
        M->Uj = std::move(U.Aj);
        M->host_missing = false;
    } else if (L.Ax.size() != M->Lx.size() || U.Ax.size() != M->Ux.size()) {
        return LSSP_AMD_EINVAL;
    }
    M->Lx = std::move(L.Ax);
    M->Ux = std::move(U.Ax);
    M->Dinv = std::move(inv);
    M->host_stale = false;
    return LSSP_AMD_OK;
}

// ---------------------------------------------------------------------------
// lssp_amd_bilu_create_dev: the handle's plan and point factors from a matrix in
// HBM
// ---------------------------------------------------------------------------
// k_ilut_check's rule (ilut_factor.hip) without the scalar diagonal, which BILUK
// does not need: Ap starts at 0, ends at nnz and never descends; every row's
// columns ascend strictly inside [0, n).  A row is read only when its range
// lies inside [0, nnz].
__global__ __launch_bounds__(256) void k_bilu_rows_check(int n, int nnz, const int *__restrict__ Ap,
                                                         const int *__restrict__ Aj, int *__restrict__ flag)
{
    bool bad = false;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < n; r += (long)gridDim.x * 256) {
        const int a = Ap[r], b = Ap[r + 1];
        if (r == 0) bad |= a != 0;
        if (r == n - 1) bad |= b != nnz;
        if (a < 0 || b > nnz || b < a) {
            bad = true;
            continue;
        }
        int prev = -1;
        for (int k = a; k < b; k++) {
            const int col = Aj[k];
            bad |= col <= prev || col >= n;
            prev = col;
        }
    }
    if (bad) atomicOr(flag, 1);
}

// The block graph, one block row per lane (bilu_graph_row): the bs-way merge is
// sequential inside a block row -- each step needs the smallest head -- so a wave
// that owned one block row could keep only its bs <= 8 rows' lanes busy and
// would pay a cross-lane minimum per block; with a block row per lane all 64
// lanes merge, the cursors live in registers, and neighbouring lanes read
// neighbouring rows of Aj, whose lines stay in cache from one step to the next
// (k_bilu_scatter's argument).  Gj == nullptr: the count pass -- cnt[i], cnt[nb]
// = 0 for the exclusive scan -- which also raises *flag for a block row without
// its diagonal block; else the fill pass into Gj + Gp[i].
__global__ __launch_bounds__(256) void k_bilu_graph(int nb, int bs, const int *__restrict__ Ap,
                                                    const int *__restrict__ Aj, const int *__restrict__ Gp,
                                                    int *__restrict__ Gj, int *__restrict__ cnt,
                                                    int *__restrict__ flag)
{
    bool bad = false;
    for (long i = blockIdx.x * 256L + threadIdx.x; i <= nb; i += (long)gridDim.x * 256) {
        if (i == nb) {
            if (!Gj) cnt[nb] = 0;
            continue;
        }
        int diag = 0;
        const int m = bilu_graph_row((int)i, bs, Ap, Aj, Gj ? Gj + Gp[i] : nullptr, &diag);
        if (!Gj) cnt[i] = m;
        bad |= !diag;
    }
    if (bad) atomicOr(flag, 1);
}

// per block row of the factor pattern: its blocks' block row (BiluPlan::d_Brow)
// and how many blocks lie left / right of the diagonal block (slot nb: 0, for
// the exclusive scans that place the rows of L and U)
__global__ __launch_bounds__(256) void k_bilu_sides(int nb, const int *__restrict__ Bp, const int *__restrict__ Bj,
                                                    const int *__restrict__ first, int *__restrict__ Brow,
                                                    int *__restrict__ cl, int *__restrict__ cu)
{
    for (long i = blockIdx.x * 256L + threadIdx.x; i <= nb; i += (long)gridDim.x * 256) {
        if (i == nb) {
            cl[nb] = cu[nb] = 0;
            continue;
        }
        const int s = Bp[i], e = Bp[i + 1], f = first[i];
        for (int k = s; k < e; k++) Brow[k] = (int)i;
        cl[i] = f - s;
        cu[i] = e - f - (f < e && Bj[f] == (int)i ? 1 : 0);
    }
}

// The expansion, one wave per block row (bilu_expand_blockrow): block row i's bs
// rows of a point factor are one contiguous run of bs * (bs * blocks + 1)
// entries, the lanes take consecutive entries of it, so Tj and Tx are written in
// whole cache lines.  The reads of a block are strided by bs doubles, but a
// block row's blocks are one contiguous piece of Fx of a few hundred bytes to a
// few KiB that this wave alone reads, every line of it within one or two loads
// of the wave: each line comes from L2 once and is then hit in the CU's cache,
// which is what a staging copy in LDS would buy (at the price of a barrier per
// block row and bank conflicts at stride bs), so there is none.
__global__ __launch_bounds__(256) void k_bilu_expand(int nb, int bs, bool upper, const int *__restrict__ Bp,
                                                     const int *__restrict__ Bj, const int *__restrict__ first,
                                                     const int *__restrict__ before, const double *__restrict__ Fx,
                                                     int *__restrict__ Tp, int *__restrict__ Tj,
                                                     double *__restrict__ Tx)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long i = blockIdx.x * 4L + wave; i < nb; i += (long)gridDim.x * 4)
        bilu_expand_blockrow(upper, bs, nb, (int)i, before[i], Bp, Bj, first, Fx, Tp, Tj, Tx, lane, 64);
}

static int bilu_scan_excl(lssp_amd_ctx *c, DevBufs &B, const int *in, int *out, size_t cnt)
{
    size_t bytes = 0;
    char *tmp = nullptr;
    LSSP_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0, cnt, rocprim::plus<int>(), c->stream));
    LSSP_HIP(B.get(&tmp, bytes));
    LSSP_HIP(rocprim::exclusive_scan(tmp, bytes, in, out, 0, cnt, rocprim::plus<int>(), c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));  // the scratch is freed next
    B.drop(tmp);
    return LSSP_AMD_OK;
}

namespace {
// the symbolic pass's plan (iluk_symbolic_dev) and the split of the block pattern
// the level pass reads: scratch of this create, freed on every path out of it
struct BlockSymbolic {
    lssp_amd_ctx *c;
    RefactorPlan *rp = nullptr;
    IlutDevFactors S;
    ~BlockSymbolic()
    {
        (void)hipStreamSynchronize(c->stream);
        iluk_split_free(&S);
        refactor_plan_free(rp);
    }
};
}  // namespace

int bilu_create_device(lssp_amd_ctx *c, lssp_amd_ilu *M, const lssp_amd_mat *A, int level, int bs, IlutDevFactors *F,
                       const std::function<int(const char *)> &mark)
{
    const int n = A->nrows, nnz = A->nnz, nb = n / bs, bs2 = bs * bs;
    if (bs < 1 || bs > BILU_MAX_BS_DEV || n != nb * bs) return LSSP_AMD_EUNSUPPORTED;
    if (nnz < nb) return LSSP_AMD_EUNSUPPORTED;  // some block row is empty: no diagonal block
    DevBufs B;
    int *flag = nullptr, *cnt = nullptr, *Gp = nullptr, *Gj = nullptr, h[2] = {1, 0};
    LSSP_HIP(B.get(&flag, 4));
    LSSP_HIP(hipMemsetAsync(flag, 0, 16, c->stream));
    // 1. nothing of A is trusted before this
    k_bilu_rows_check<<<bilu_grid(n), 256, 0, c->stream>>>(n, nnz, A->Ap, A->Aj, flag);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipMemcpyAsync(h, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (h[0]) return LSSP_AMD_EUNSUPPORTED;  // an unsorted row, a repeated column, a column outside [0, n)
    LSSP_TRY(mark("check"));
    // 2. the block graph: count, scan, fill
    LSSP_HIP(B.get(&cnt, (size_t)nb + 1));
    LSSP_HIP(B.get(&Gp, (size_t)nb + 1));
    k_bilu_graph<<<bilu_grid((long)nb + 1), 256, 0, c->stream>>>(nb, bs, A->Ap, A->Aj, nullptr, nullptr, cnt, flag + 1);
    LSSP_HIP(hipGetLastError());
    LSSP_TRY(bilu_scan_excl(c, B, cnt, Gp, (size_t)nb + 1));
    h[0] = 1;
    LSSP_HIP(hipMemcpyAsync(h, flag + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(h + 1, Gp + nb, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (h[0]) return LSSP_AMD_EUNSUPPORTED;  // a block row without its diagonal block
    const int ng = h[1];
    if (ng < nb || ng > nnz) return LSSP_AMD_EHIP;  // (every block holds an entry of A)
    if ((long)ng * bs2 + n > (long)INT_MAX) return LSSP_AMD_EUNSUPPORTED;
    LSSP_HIP(B.get(&Gj, (size_t)ng));
    k_bilu_graph<<<bilu_grid((long)nb + 1), 256, 0, c->stream>>>(nb, bs, A->Ap, A->Aj, Gp, Gj, cnt, flag + 1);
    LSSP_HIP(hipGetLastError());
    LSSP_TRY(mark("block graph"));
    // 3. the symbolic ILU(level) of the block graph (level 0: the graph itself), 4. its level lists
    BlockSymbolic sym{c};
    const std::function<int(const char *)> sub = [&](const char *phase) {
        return mark(strcmp(phase, "check") ? phase : "graph check");
    };
    LSSP_TRY(iluk_symbolic_dev(c, nb, ng, Gp, Gj, level, &sym.rp, sub));
    RefactorPlan &rp = *sym.rp;
    const long nblk = rp.nnz;
    if (nblk < nb || nblk * bs2 + n > (long)INT_MAX) return LSSP_AMD_EUNSUPPORTED;  // L, U keep 32-bit row pointers
    LSSP_TRY(iluk_split_pattern_dev(c, nb, rp, &sym.S));
    LSSP_TRY(iluk_plan_levels_dev(c, nb, rp, sym.S));
    // the plan lssp_amd_bilu_refactor works on: the symbolic pass's arrays are its pattern (the
    // origin byte is the graph byte, the diagonal block is the first non-lower one)
    BiluPlan *pp = new BiluPlan();
    M->brf = pp;  // the handle's from here on: freed with it on every failure
    BiluPlan &p = *pp;
    p.nb = nb;
    p.bs = bs;
    p.nblk = nblk;
    p.d_Bp = rp.d_Fp, p.d_Bj = rp.d_Fj, p.d_in = rp.d_fin, p.d_first = rp.d_dpos, p.d_rows = rp.d_rows;
    rp.d_Fp = rp.d_Fj = rp.d_dpos = rp.d_rows = nullptr;
    rp.d_fin = nullptr;
    p.lev_off = std::move(rp.lev_off);
    LSSP_HIP(hipMalloc(&p.d_Brow, sizeof(int) * (size_t)nblk));
    LSSP_HIP(hipMalloc(&p.d_hit, (size_t)nblk));
    LSSP_HIP(hipMalloc(&p.d_Bx, sizeof(double) * (size_t)nblk * bs2));
    LSSP_HIP(hipMalloc(&p.d_Fx, sizeof(double) * (size_t)nblk * bs2));
    LSSP_HIP(hipMalloc(&p.d_inv, sizeof(double) * (size_t)nb * bs2));
    LSSP_HIP(hipMalloc(&p.d_flag, sizeof(int) * 2));
    int *cl = nullptr, *cu = nullptr, *bl = nullptr, *bu = nullptr;
    LSSP_HIP(B.get(&cl, (size_t)nb + 1));
    LSSP_HIP(B.get(&cu, (size_t)nb + 1));
    LSSP_HIP(B.get(&bl, (size_t)nb + 1));
    LSSP_HIP(B.get(&bu, (size_t)nb + 1));
    k_bilu_sides<<<bilu_grid((long)nb + 1), 256, 0, c->stream>>>(nb, p.d_Bp, p.d_Bj, p.d_first, p.d_Brow, cl, cu);
    LSSP_HIP(hipGetLastError());
    LSSP_TRY(mark("levels"));
    // 5. the refactor's own kernels and launches (no graph compare: the pattern was just built from A)
    LSSP_HIP(hipMemsetAsync(p.d_Bx, 0, sizeof(double) * (size_t)nblk * bs2, c->stream));
    LSSP_HIP(hipMemsetAsync(p.d_hit, 0, (size_t)nblk, c->stream));
    LSSP_HIP(hipMemsetAsync(p.d_flag, 0, sizeof(int) * 2, c->stream));
    k_bilu_scatter<<<bilu_grid(n), 256, 0, c->stream>>>(n, bs, nnz, A->Ap, A->Aj, A->Ax, p.d_Bp, p.d_Bj, p.d_Bx,
                                                       p.d_hit, p.d_flag);
    LSSP_HIP(hipGetLastError());
    LSSP_TRY(mark("scatter"));
    bilu0_launch_levels(c, bs, p.lev_off, p.d_rows, p.d_Bp, p.d_Bj, p.d_Bx, p.d_inv, p.d_flag + 1);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipMemcpyAsync(h, p.d_flag, sizeof(int) * 2, hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (h[0]) return LSSP_AMD_EHIP;    // an entry of A outside the pattern made from A
    if (h[1]) return LSSP_AMD_EINVAL;  // singular diagonal block
    LSSP_TRY(mark("numeric BILU(0)"));
    LSSP_TRY(bilu_commit_launch(c, p));
    LSSP_TRY(mark("U scaling"));
    // 6. the point factors: the rows' places from one scan a side, then the fill
    LSSP_TRY(bilu_scan_excl(c, B, cl, bl, (size_t)nb + 1));
    LSSP_TRY(bilu_scan_excl(c, B, cu, bu, (size_t)nb + 1));
    LSSP_HIP(hipMemcpyAsync(h, bl + nb, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(h + 1, bu + nb, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    if (h[0] < 0 || h[1] < 0 || (long)h[0] + h[1] + nb != nblk) return LSSP_AMD_EHIP;
    F->nnzL = (int)((long)h[0] * bs2 + n);
    F->nnzU = (int)((long)h[1] * bs2 + n);
    LSSP_HIP(hipMalloc(&F->Lp, sizeof(int) * ((size_t)n + 1)));
    LSSP_HIP(hipMalloc(&F->Up, sizeof(int) * ((size_t)n + 1)));
    LSSP_HIP(hipMalloc(&F->Lj, sizeof(int) * (size_t)F->nnzL));
    LSSP_HIP(hipMalloc(&F->Lx, sizeof(double) * (size_t)F->nnzL));
    LSSP_HIP(hipMalloc(&F->Uj, sizeof(int) * (size_t)F->nnzU));
    LSSP_HIP(hipMalloc(&F->Ux, sizeof(double) * (size_t)F->nnzU));
    const unsigned eg = (unsigned)std::max<long>(1, std::min<long>(((long)nb + 3) / 4, 1L << 20));
    k_bilu_expand<<<eg, 256, 0, c->stream>>>(nb, bs, false, p.d_Bp, p.d_Bj, p.d_first, bl, p.d_Fx, F->Lp, F->Lj, F->Lx);
    k_bilu_expand<<<eg, 256, 0, c->stream>>>(nb, bs, true, p.d_Bp, p.d_Bj, p.d_first, bu, p.d_Fx, F->Up, F->Uj, F->Ux);
    LSSP_HIP(hipGetLastError());
    LSSP_HIP(hipStreamSynchronize(c->stream));  // the scans' outputs are freed on return
    return mark("expansion");
}

}  // namespace lssp_amd
