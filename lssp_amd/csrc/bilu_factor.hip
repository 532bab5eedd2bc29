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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "bilu_dev.h"
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

// In place on the host BCSR (block columns ascending): upload, one launch per
// level, download of the blocks and the inverted diagonal blocks.
int bilu0_factor_gpu(lssp_amd_ctx *c, HostBCSR &T, std::vector<double> &inv)
{
    const int nb = T.nb, bs = T.bs, bs2 = bs * bs;
    if (bs < 1 || bs > BILU_MAX_BS_DEV) return LSSP_AMD_EINVAL;
    inv.assign((size_t)nb * bs2, 0.0);
    if (nb <= 0) return LSSP_AMD_OK;
    const size_t nblk = T.Bj.size();
    std::vector<int> lev(nb, 0);
    int nlev = 0;
    for (int i = 0; i < nb; i++) {
        int l = 0;
        for (int k = T.Bp[i]; k < T.Bp[i + 1] && T.Bj[k] < i; k++) l = std::max(l, lev[T.Bj[k]] + 1);
        lev[i] = l;
        nlev = std::max(nlev, l + 1);
    }
    std::vector<int> off(nlev + 1, 0), rows(nb);
    for (int i = 0; i < nb; i++) off[lev[i] + 1]++;
    for (int l = 0; l < nlev; l++) off[l + 1] += off[l];
    {
        std::vector<int> fill(off.begin(), off.end() - 1);
        for (int i = 0; i < nb; i++) rows[fill[lev[i]]++] = i;
    }
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
    static const bool times = getenv("LSSP_AMD_SETUP_TIMES") && atoi(getenv("LSSP_AMD_SETUP_TIMES"));
    if (times && st == LSSP_AMD_OK) fail(hipStreamSynchronize(c->stream));
    const double t0 = wall_time();
    if (st == LSSP_AMD_OK) {
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

}  // namespace lssp_amd
