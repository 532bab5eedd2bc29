// bilu_dev.h -- the canonical dense-block arithmetic of BILUK.
//
// The reference's block values come from whichever BLAS / LAPACK it was linked
// with (pc-biluk.cxx:62-102: dgetrf + dgetri, dgemm), so there is no bitwise
// target outside this project.  These functions are the project's own: the
// host factorization (ilu_setup.cpp) and the device one (bilu_factor.hip)
// both call them, and the tree builds with -ffp-contract=off on host and
// device, so both paths give the same bits.  Blocks are n x n, COLUMN-major
// (entry (r, c) at [c * n + r]), as lssp_mat_csr_to_bcsr stores them.
#pragma once

#include <cmath>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define BILU_HD __host__ __device__
#else
#define BILU_HD
#endif

namespace lssp_amd {

constexpr int BILU_MAX_BS = 32;      // host numeric path
constexpr int BILU_MAX_BS_DEV = 8;   // k_bilu0_level<BS>

// Entry (i, j) of C = beta*C + alpha*A*B in the order of netlib dgemm('N','N'):
// the column of C is cleared (beta == 0), kept (beta == 1) or scaled, then for
// l = 0 .. n-1: t = alpha*B(l,j); C(i,j) = C(i,j) + t*A(i,l).  Every entry is
// an independent in-order sum over l, so a lane per entry equals the host loop.
// n == 1 is the reference's scalar branch (pc-biluk.cxx:95-97).
BILU_HD inline double bilu_gemm_entry(const double *A, const double *B, double alpha, double c, double beta, int n,
                                      int i, int j)
{
    if (n == 1) return A[0] * B[0] * alpha + beta * c;
    if (beta == 0.) c = 0.;
    else if (beta != 1.) c = beta * c;
    for (int l = 0; l < n; l++) {
        const double t = alpha * B[l + j * n];
        c = c + t * A[i + l * n];
    }
    return c;
}

// C = beta*C + alpha*A*B; C must not overlap A or B
BILU_HD inline void bilu_gemm(const double *A, const double *B, double alpha, double *C, double beta, int n)
{
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++) C[i + j * n] = bilu_gemm_entry(A, B, alpha, C[i + j * n], beta, n, i, j);
}

// A <- A^-1 in place by Gauss-Jordan elimination with partial pivoting.  Step
// k: the pivot row is the FIRST row p >= k with the largest |A(p,k)| (a strict
// > scan from row k, so the lowest row wins ties); a pivot that is zero or NaN
// means singular (return 1, A left part-way).  Rows p and k are swapped, row k
// is divided by the pivot (its own column becomes 1 / pivot), and every other
// row r has f = A(r,k) eliminated: A(r,k) = -f * A(k,k), A(r,c) = A(r,c) -
// f*A(k,c) elsewhere.  Afterwards the row swaps are undone as column swaps in
// reverse order.  n == 1: 1.0 / a (pc-biluk.cxx:66-73).  piv holds n ints.
BILU_HD inline int bilu_inverse(double *A, int n, int *piv)
{
    if (n == 1) {
        if (!(fabs(A[0]) > 0.)) return 1;
        A[0] = 1.0 / A[0];
        return 0;
    }
    for (int k = 0; k < n; k++) {
        int p = k;
        double best = fabs(A[k + k * n]);
        for (int r = k + 1; r < n; r++) {
            const double v = fabs(A[r + k * n]);
            if (v > best) {
                best = v;
                p = r;
            }
        }
        const double pv = A[p + k * n];
        if (!(fabs(pv) > 0.)) return 1;
        piv[k] = p;
        if (p != k)
            for (int c = 0; c < n; c++) {
                const double t = A[k + c * n];
                A[k + c * n] = A[p + c * n];
                A[p + c * n] = t;
            }
        A[k + k * n] = 1.0;
        for (int c = 0; c < n; c++) A[k + c * n] = A[k + c * n] / pv;
        for (int r = 0; r < n; r++) {
            if (r == k) continue;
            const double f = A[r + k * n];
            A[r + k * n] = 0.;
            for (int c = 0; c < n; c++) A[r + c * n] = A[r + c * n] - f * A[k + c * n];
        }
    }
    for (int k = n - 1; k >= 0; k--) {
        const int p = piv[k];
        if (p == k) continue;
        for (int r = 0; r < n; r++) {
            const double t = A[r + k * n];
            A[r + k * n] = A[r + p * n];
            A[r + p * n] = t;
        }
    }
    return 0;
}

}  // namespace lssp_amd
