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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

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
    auto grid = [](long items) { return (unsigned)std::max<long>(1, std::min<long>((items + 255) / 256, 16384)); };
    int flag = 0;
    // 1. zero, scatter; 2. graph compare -- on scratch only
    LSSP_HIP(hipMemsetAsync(p.d_Bx, 0, sizeof(double) * std::max<long>(nblk, 1) * bs2, c->stream));
    LSSP_HIP(hipMemsetAsync(p.d_hit, 0, std::max<long>(nblk, 1), c->stream));
    LSSP_HIP(hipMemsetAsync(p.d_flag, 0, sizeof(int) * 2, c->stream));
    k_bilu_scatter<<<grid(n), 256, 0, c->stream>>>(n, bs, A->nnz, A->Ap, A->Aj, A->Ax, p.d_Bp, p.d_Bj, p.d_Bx, p.d_hit,
                                                  p.d_flag);
    k_bilu_graph_cmp<<<grid(nblk), 256, 0, c->stream>>>(nblk, p.d_hit, p.d_in, p.d_flag);
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
    switch (bs) {
#define LSSP_BCOMMIT(B)                                                                                        \
    case B:                                                                                                    \
        k_bilu_commit<B><<<grid(nblk * bs2), 256, 0, c->stream>>>(nblk, p.d_Brow, p.d_Bj, p.d_Bx, p.d_inv, p.d_Fx); \
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
// buffer and of the inverses, then bilu_expand (the U blocks are scaled already)
int bilu_refactor_host_factors(lssp_amd_ilu *M)
{
    if (!M->host_stale || !M->brf) return LSSP_AMD_OK;
    lssp_amd_ctx *c = M->ctx;
    const BiluPlan &p = *M->brf;
    HostBCSR T;
    T.nb = p.nb;
    T.bs = p.bs;
    T.Bp = M->bBp;
    T.Bj = M->bBj;
    T.Bx.resize((size_t)p.nblk * p.bs * p.bs);
    std::vector<double> inv(M->Dinv.size());
    LSSP_HIP(hipMemcpyAsync(T.Bx.data(), p.d_Fx, sizeof(double) * T.Bx.size(), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipMemcpyAsync(inv.data(), M->d_Dinv, sizeof(double) * inv.size(), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    HostCSR L, U;
    bilu_expand(T, inv, L, U, true);
    if (L.Ax.size() != M->Lx.size() || U.Ax.size() != M->Ux.size()) return LSSP_AMD_EINVAL;
    M->Lx = std::move(L.Ax);
    M->Ux = std::move(U.Ax);
    M->Dinv = std::move(inv);
    M->host_stale = false;
    return LSSP_AMD_OK;
}

}  // namespace lssp_amd
