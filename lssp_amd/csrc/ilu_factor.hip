// ilu_factor.hip -- ILU(0) numeric factorization on the GPU.
//
// Restates lssp_pc_ilu0_fac (pc-iluk.cxx:347-409), the IKJ elimination the
// reference runs on the host for ILUK(k) on the level-k pattern, operation for
// operation, so the factors are bitwise the reference's:
//   for each strict-lower entry k of row i, ascending:
//       a_ik = a_ik * dinv[c_k]                         (reciprocal pivot, :386)
//       a_ij = a_ij - a_ik * u_kj   for j > k where row c_k holds a NONZERO
//                                   value at column c_j  (:388-390, wk[] != 0)
//   dinv[i] = 1 / a_ii, a tiny pivot replaced first   (:394-399)
// Row i only reads rows c_k < i of its own strict-lower pattern, so rows are
// processed level by level (levels of that DAG, computed on the host; the same
// levels as the L sweep), one lane per row, one launch per level.  Instead of
// the reference's dense scatter array wk[] a lane merges its row with row c_k
// (both sorted): the value wk[c] would hold is the LAST entry of row c_k with
// column c, and an exact zero there skips the update, as the reference's test
// does.  A block-diagonal matrix (block-Jacobi, blk < n) is factored in one
// pass: the first row of every block follows the reference's row-0 rule
// (pivot sign kept, the stored value left untouched, :367-375).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "iluk_create_dev.h"
#include "iluk_refactor_dev.h"
#include "internal.h"

namespace lssp_amd {

constexpr double ILU_ZERO_DIAG_VALUE = 1e-3;  // pc.cxx:6 (ilu_setup.cpp ZERO_DIAG_VALUE)
constexpr double ILU_ZERO_DIAG_TOL = 1e-10;   // pc.cxx:7

__global__ __launch_bounds__(256) void k_ilu0_level(const int *__restrict__ rows, int cnt, const int *__restrict__ Ap,
                                                    const int *__restrict__ C, double *Ax, double *dinv, int blk)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cnt) return;
    const int i = rows[t];
    const int s = Ap[i], end = Ap[i + 1];
    if (i % blk == 0) {  // first row of a (block-Jacobi) block
        double d0 = Ax[s];
        if (fabs(d0) < ILU_ZERO_DIAG_TOL) d0 = d0 > 0 ? ILU_ZERO_DIAG_VALUE : -ILU_ZERO_DIAG_VALUE;
        dinv[i] = 1. / d0;
        return;
    }
    int k = s;
    for (; k < end && C[k] < i; k++) {
        const int r = C[k];
        const double aik = Ax[k] * dinv[r];
        Ax[k] = aik;
        int q = Ap[r];
        const int qe = Ap[r + 1];
        for (int j = k + 1; j < end; j++) {
            const int c = C[j];
            while (q < qe && C[q] < c) q++;
            double w = 0.;
            for (int qq = q; qq < qe && C[qq] == c; qq++) w = Ax[qq];  // last duplicate wins, as wk[] does
            if (w != 0.) Ax[j] = Ax[j] - aik * w;
        }
    }
    double d = ILU_ZERO_DIAG_VALUE;
    if (k < end && C[k] == i) {
        if (fabs(Ax[k]) < ILU_ZERO_DIAG_TOL) Ax[k] = ILU_ZERO_DIAG_VALUE;
        d = Ax[k];
    }
    dinv[i] = 1. / d;
}

// levels of the strict-lower DAG (row i waits on rows C[k] < i of its sorted
// row): rows ordered by level, level l at rows[off[l] .. off[l + 1])
static int level_lists(int n, const std::vector<int> &Ap, const std::vector<int> &Aj, std::vector<int> &off,
                       std::vector<int> &rows)
{
    std::vector<int> lev(n, 0);
    int nlev = 0;
    for (int i = 0; i < n; i++) {
        int l = 0;
        for (int k = Ap[i]; k < Ap[i + 1] && Aj[k] < i; k++) l = std::max(l, lev[Aj[k]] + 1);
        lev[i] = l;
        nlev = std::max(nlev, l + 1);
    }
    off.assign(nlev + 1, 0);
    rows.resize(n);
    for (int i = 0; i < n; i++) off[lev[i] + 1]++;
    for (int l = 0; l < nlev; l++) off[l + 1] += off[l];
    {
        std::vector<int> fill(off.begin(), off.end() - 1);
        for (int i = 0; i < n; i++) rows[fill[lev[i]]++] = i;
    }
    return nlev;
}

// In place on the host CSR (sorted rows): upload, level-scheduled launches,
// download of the values.  blk: block size of a block-diagonal matrix (n: one
// block).
int ilu0_factor_gpu(lssp_amd_ctx *c, int n, int blk, const std::vector<int> &Ap, const std::vector<int> &Aj,
                    std::vector<double> &Ax)
{
    if (n <= 0) return LSSP_AMD_OK;
    if (blk <= 0 || blk > n) blk = n;
    const long nnz = Ap[n];
    std::vector<int> off, rows;
    const int nlev = level_lists(n, Ap, Aj, off, rows);
    int *d_Ap = nullptr, *d_Aj = nullptr, *d_rows = nullptr;
    double *d_Ax = nullptr, *d_dinv = nullptr;
    int st = LSSP_AMD_OK;
    auto fail = [&](hipError_t e) {
        if (e != hipSuccess && st == LSSP_AMD_OK) {
            fprintf(stderr, "lssp_amd: HIP error %s in ilu0_factor_gpu\n", hipGetErrorString(e));
            st = LSSP_AMD_EHIP;
        }
    };
    fail(hipMalloc(&d_Ap, sizeof(int) * (n + 1)));
    fail(hipMalloc(&d_Aj, sizeof(int) * std::max<long>(nnz, 1)));
    fail(hipMalloc(&d_Ax, sizeof(double) * std::max<long>(nnz, 1)));
    fail(hipMalloc(&d_rows, sizeof(int) * n));
    fail(hipMalloc(&d_dinv, sizeof(double) * n));
    if (st == LSSP_AMD_OK) {
        fail(hipMemcpyAsync(d_Ap, Ap.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice, c->stream));
        fail(hipMemcpyAsync(d_Aj, Aj.data(), sizeof(int) * nnz, hipMemcpyHostToDevice, c->stream));
        fail(hipMemcpyAsync(d_Ax, Ax.data(), sizeof(double) * nnz, hipMemcpyHostToDevice, c->stream));
        fail(hipMemcpyAsync(d_rows, rows.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
    }
    if (st == LSSP_AMD_OK) {
        for (int l = 0; l < nlev; l++) {
            const int cnt = off[l + 1] - off[l];
            k_ilu0_level<<<(cnt + 255) / 256, 256, 0, c->stream>>>(d_rows + off[l], cnt, d_Ap, d_Aj, d_Ax, d_dinv,
                                                                  blk);
        }
        fail(hipGetLastError());
        fail(hipMemcpyAsync(Ax.data(), d_Ax, sizeof(double) * nnz, hipMemcpyDeviceToHost, c->stream));
        fail(hipStreamSynchronize(c->stream));
    }
    for (void *p : {(void *)d_Ap, (void *)d_Aj, (void *)d_Ax, (void *)d_rows, (void *)d_dinv})
        if (p) (void)hipFree(p);
    return st;
}

// ---------------------------------------------------------------------------
// lssp_amd_ilu_refactor: the same factorization on buffers that stay on the
// device (RefactorPlan, internal.h)
// ---------------------------------------------------------------------------
// *diff |= 1 when the CSR pattern (Ap, Aj) is not the plan's (Fp, Fj); the
// entry counts are equal (checked on the host), so one index space serves both
__global__ __launch_bounds__(256) void k_pattern_diff(long n1, long nnz, const int *__restrict__ Ap,
                                                      const int *__restrict__ Fp, const int *__restrict__ Aj,
                                                      const int *__restrict__ Fj, int *__restrict__ diff)
{
    const long m = n1 > nnz ? n1 : nnz;
    bool d = false;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < m; i += (long)gridDim.x * 256) {
        if (i < n1) d |= Ap[i] != Fp[i];
        if (i < nnz) d |= Aj[i] != Fj[i];
    }
    if (d) atomicOr(diff, 1);
}

void refactor_plan_free(RefactorPlan *p)
{
    if (!p) return;
    for (void *q : {(void *)p->d_Fp, (void *)p->d_Fj, (void *)p->d_Fx, (void *)p->d_dinv, (void *)p->d_rows,
                    (void *)p->d_flag, (void *)p->d_fin, (void *)p->d_dpos})
        if (q) (void)hipFree(q);
    delete p;
}

// F's row i = L's strict entries, the diagonal, U's strict entries (L keeps its
// unit diagonal LAST, U its pivot FIRST): the pattern ilu_factor split them from
// with_flags (lssp_amd_iluk_refactor's own routes): also the handle's flag bytes
// and each row's diagonal position
int refactor_plan_build(lssp_amd_ctx *c, lssp_amd_ilu *M, bool with_flags)
{
    if (M->rf) return LSSP_AMD_OK;
    const int n = M->n;
    const long nnz = (long)M->Lp[n] + M->Up[n] - n;
    std::vector<int> Fp(n + 1), Fj((size_t)nnz);
    Fp[0] = 0;
    for (int i = 0; i < n; i++) Fp[i + 1] = Fp[i] + (M->Lp[i + 1] - M->Lp[i] - 1) + (M->Up[i + 1] - M->Up[i]);
    parallel_for(n, [&](long i0, long i1) {
        for (long i = i0; i < i1; i++) {
            int f = Fp[i];
            for (int k = M->Lp[i]; k < M->Lp[i + 1] - 1; k++) Fj[f++] = M->Lj[k];
            for (int k = M->Up[i]; k < M->Up[i + 1]; k++) Fj[f++] = M->Uj[k];
        }
    });
    RefactorPlan *p = new RefactorPlan();
    p->nnz = nnz;
    std::vector<int> rows;
    level_lists(n, Fp, Fj, p->lev_off, rows);
    std::vector<int> dpos;
    if (with_flags) {
        if ((long)M->fIn.size() != nnz) {
            delete p;
            return LSSP_AMD_EINVAL;
        }
        dpos.resize(n);
        for (int i = 0; i < n; i++) dpos[i] = Fp[i] + (M->Lp[i + 1] - M->Lp[i] - 1);
    }
    auto fill = [&]() -> int {
        LSSP_HIP(hipMalloc(&p->d_Fp, sizeof(int) * (n + 1)));
        LSSP_HIP(hipMalloc(&p->d_Fj, sizeof(int) * nnz));
        LSSP_HIP(hipMalloc(&p->d_Fx, sizeof(double) * nnz));
        LSSP_HIP(hipMalloc(&p->d_dinv, sizeof(double) * n));
        LSSP_HIP(hipMalloc(&p->d_rows, sizeof(int) * n));
        LSSP_HIP(hipMalloc(&p->d_flag, sizeof(int)));
        LSSP_HIP(hipMemcpyAsync(p->d_Fp, Fp.data(), sizeof(int) * (n + 1), hipMemcpyHostToDevice, c->stream));
        LSSP_HIP(hipMemcpyAsync(p->d_Fj, Fj.data(), sizeof(int) * nnz, hipMemcpyHostToDevice, c->stream));
        LSSP_HIP(hipMemcpyAsync(p->d_rows, rows.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
        if (with_flags) {
            LSSP_HIP(hipMalloc(&p->d_fin, (size_t)nnz));
            LSSP_HIP(hipMalloc(&p->d_dpos, sizeof(int) * n));
            LSSP_HIP(hipMemcpyAsync(p->d_fin, M->fIn.data(), (size_t)nnz, hipMemcpyHostToDevice, c->stream));
            LSSP_HIP(hipMemcpyAsync(p->d_dpos, dpos.data(), sizeof(int) * n, hipMemcpyHostToDevice, c->stream));
        }
        LSSP_HIP(hipStreamSynchronize(c->stream));
        return LSSP_AMD_OK;
    };
    const int st = fill();
    if (st != LSSP_AMD_OK) {
        (void)hipGetLastError();
        refactor_plan_free(p);
        return st;
    }
    M->rf = p;
    return LSSP_AMD_OK;
}

// ---------------------------------------------------------------------------
// lssp_amd_ilu_create_dev: the plan of a complete box without a host pass
// ---------------------------------------------------------------------------
// One thread per row, grid-strided: row r = (i, j, k) of the nx x ny x nz box
// must hold exactly {r - plane, r - nx, r - 1, r, r + 1, r + nx, r + plane},
// each where its neighbour exists, in that (ascending) order.  Ap is not
// trusted: a row is read only when its range lies inside [0, nnz) and has the
// expected length.  Any mismatch ORs *flag.
__global__ __launch_bounds__(256) void k_box_check(int n, int nnz, int nx, int ny, int nz, const int *__restrict__ Ap,
                                                   const int *__restrict__ Aj, int *__restrict__ flag)
{
    const long plane = (long)nx * ny;
    bool bad = false;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < n; r += (long)gridDim.x * 256) {
        const int i = (int)(r % nx);
        const long q = r / nx;
        const int j = (int)(q % ny), k = (int)(q / ny);
        const bool km = k > 0, jm = j > 0, im = i > 0, ip = i < nx - 1, jp = j < ny - 1, kp = k < nz - 1;
        const int len = 1 + km + jm + im + ip + jp + kp;
        const int a = Ap[r], b = Ap[r + 1];
        if (r == 0) bad |= a != 0;
        if (r == n - 1) bad |= b != nnz;
        if (a < 0 || b > nnz || b < a || b - a != len) {
            bad = true;
            continue;
        }
        int e = a;
        if (km) bad |= (long)Aj[e++] != r - plane;
        if (jm) bad |= (long)Aj[e++] != r - nx;
        if (im) bad |= (long)Aj[e++] != r - 1;
        bad |= (long)Aj[e++] != r;
        if (ip) bad |= (long)Aj[e++] != r + 1;
        if (jp) bad |= (long)Aj[e++] != r + nx;
        if (kp) bad |= (long)Aj[e++] != r + plane;
    }
    if (bad) atomicOr(flag, 1);
}

int box_pattern_check(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, int nx, int ny, int nz, int *ok)
{
    *ok = 0;
    if ((long)nx * ny * nz != (long)n) return LSSP_AMD_OK;
    int *d_flag = nullptr;
    LSSP_HIP(hipMalloc(&d_flag, sizeof(int)));
    auto run = [&]() -> int {
        LSSP_HIP(hipMemsetAsync(d_flag, 0, sizeof(int), c->stream));
        k_box_check<<<(unsigned)std::min<long>(((long)n + 255) / 256, 16384), 256, 0, c->stream>>>(n, nnz, nx, ny, nz,
                                                                                                 dAp, dAj, d_flag);
        LSSP_HIP(hipGetLastError());
        int bad = 1;
        LSSP_HIP(hipMemcpyAsync(&bad, d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        *ok = !bad;
        return LSSP_AMD_OK;
    };
    const int st = run();
    (void)hipFree(d_flag);
    return st;
}

// d_rows of a complete box in closed form.  Row (i, j, k) has level l = i + j +
// k; inside a level rows ascend, i.e. by k, then j.  With c2(m) = the number of
// (i, j) of the nx x ny plane on i + j = m and C2 its running sum (C2[x] = sum
// of c2(m), m < x), the rows of level l before (i, j, k) are the planes k' < k,
// c2(l - k') each = C2[l + 1] - C2[l - k + 1], and on plane k the lines j' < j
// that reach the diagonal m = i + j: j - max(0, m - nx + 1).  tab = C2[0 ..
// nlev], then lev_off[0 .. nlev].  A position outside [0, n) (never, on a box)
// is dropped and ORs *flag.
__global__ __launch_bounds__(256) void k_box_levels(int n, int nx, int ny, int nlev, const int *__restrict__ tab,
                                                    int *__restrict__ rows, int *__restrict__ flag)
{
    const int *C2 = tab, *off = tab + nlev + 1;
    bool bad = false;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < n; r += (long)gridDim.x * 256) {
        const int i = (int)(r % nx);
        const long q = r / nx;
        const int j = (int)(q % ny), k = (int)(q / ny);
        const int m = i + j, l = m + k;
        const long pos = (long)off[l] + (C2[l + 1] - C2[m + 1]) + (j - max(0, m - nx + 1));
        if (pos < 0 || pos >= n) bad = true;
        else rows[pos] = (int)r;
    }
    if (bad) atomicOr(flag, 1);
}

int refactor_plan_from_box(lssp_amd_ctx *c, int n, int nnz, const int *dAp, const int *dAj, int nx, int ny, int nz,
                           RefactorPlan **out)
{
    *out = nullptr;
    if ((long)nx * ny * nz != (long)n || nnz < n) return LSSP_AMD_EINVAL;
    const int nlev = nx + ny + nz - 2;
    // the two tables from the grid alone (no pass over the matrix)
    std::vector<int> tab(2 * (size_t)nlev + 2);
    int *C2 = tab.data(), *off = tab.data() + nlev + 1;
    C2[0] = 0;
    for (int m = 0; m < nlev; m++) {
        const int c2 = m <= nx + ny - 2 ? std::min(std::min(m, nx + ny - 2 - m), std::min(nx, ny) - 1) + 1 : 0;
        C2[m + 1] = C2[m] + c2;
    }
    off[0] = 0;
    for (int l = 0; l < nlev; l++) off[l + 1] = off[l] + (C2[l + 1] - C2[std::max(l - nz + 1, 0)]);
    if (off[nlev] != n) return LSSP_AMD_EINVAL;
    RefactorPlan *p = new RefactorPlan();
    p->nnz = nnz;
    p->lev_off.assign(off, off + nlev + 1);
    int *d_tab = nullptr;
    auto fill = [&]() -> int {
        LSSP_HIP(hipMalloc(&p->d_Fp, sizeof(int) * ((size_t)n + 1)));
        LSSP_HIP(hipMalloc(&p->d_Fj, sizeof(int) * (size_t)nnz));
        LSSP_HIP(hipMalloc(&p->d_Fx, sizeof(double) * (size_t)nnz));
        LSSP_HIP(hipMalloc(&p->d_dinv, sizeof(double) * (size_t)n));
        LSSP_HIP(hipMalloc(&p->d_rows, sizeof(int) * (size_t)n));
        LSSP_HIP(hipMalloc(&p->d_flag, sizeof(int)));
        LSSP_HIP(hipMalloc(&d_tab, sizeof(int) * tab.size()));
        LSSP_HIP(hipMemcpy(d_tab, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice));
        LSSP_HIP(hipMemcpyAsync(p->d_Fp, dAp, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToDevice, c->stream));
        LSSP_HIP(hipMemcpyAsync(p->d_Fj, dAj, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToDevice, c->stream));
        LSSP_HIP(hipMemsetAsync(p->d_flag, 0, sizeof(int), c->stream));
        k_box_levels<<<(unsigned)std::min<long>(((long)n + 255) / 256, 16384), 256, 0, c->stream>>>(n, nx, ny, nlev, d_tab,
                                                                                                  p->d_rows, p->d_flag);
        LSSP_HIP(hipGetLastError());
        int bad = 1;
        LSSP_HIP(hipMemcpyAsync(&bad, p->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        return bad ? LSSP_AMD_EINVAL : LSSP_AMD_OK;
    };
    const int st = fill();
    if (d_tab) (void)hipFree(d_tab);
    if (st != LSSP_AMD_OK) {
        (void)hipGetLastError();
        refactor_plan_free(p);
        return st;
    }
    *out = p;
    return LSSP_AMD_OK;
}

// ---------------------------------------------------------------------------
// lssp_amd_iluk_create_dev: the plan of a complete box's ILU(1) in closed form
// (iluk_create_dev.h), one row per lane, grid-strided
// ---------------------------------------------------------------------------
// Fp (row n - 1 also writes Fp[n]), Fj, the flag bytes and the diagonal
// positions.  A row whose range would leave [0, fnnz) (never, on a box) is
// dropped and ORs *flag, as does an end of the last row other than fnnz.
__global__ __launch_bounds__(256) void k_fill1_pattern(int n, long fnnz, int nx, int ny, int nz, int *__restrict__ Fp,
                                                       int *__restrict__ Fj, unsigned char *__restrict__ fin,
                                                       int *__restrict__ dpos, int *__restrict__ flag)
{
    bool bad = false;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < n; r += (long)gridDim.x * 256) {
        const int i = (int)(r % nx);
        const long q = r / nx;
        const int j = (int)(q % ny), k = (int)(q / ny);
        const long s = fill1_row_start(i, j, k, nx, ny, nz);
        const int len = fill1_row_len(i, j, k, nx, ny, nz);
        if (s < 0 || s + len > fnnz) {
            bad = true;
            continue;
        }
        int dp = 0;
        fill1_row(i, j, k, nx, ny, nz, Fj + s, fin + s, &dp);
        Fp[r] = (int)s;
        dpos[r] = (int)s + dp;
        if (r == n - 1) {
            Fp[n] = (int)(s + len);
            bad |= s + len != fnnz;
        }
    }
    if (bad) atomicOr(flag, 1);
}

// d_rows: tab = S3[0 .. nlev), then lev_off[0 .. nlev].  A position outside
// [0, n) (never, on a box) is dropped and ORs *flag.
__global__ __launch_bounds__(256) void k_fill1_levels(int n, int nx, int ny, int nlev, const int *__restrict__ tab,
                                                      int *__restrict__ rows, int *__restrict__ flag)
{
    bool bad = false;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < n; r += (long)gridDim.x * 256) {
        const int i = (int)(r % nx);
        const long q = r / nx;
        const int j = (int)(q % ny), k = (int)(q / ny);
        const long pos = fill1_level_pos(i, j, k, nx, tab, tab + nlev);
        if (pos < 0 || pos >= n) bad = true;
        else rows[pos] = (int)r;
    }
    if (bad) atomicOr(flag, 1);
}

long fill1_nnz(int nx, int ny, int nz) { return fill1_row_start(0, 0, nz, nx, ny, nz); }

int fill1_plan_pattern(lssp_amd_ctx *c, int n, int nx, int ny, int nz, RefactorPlan **out)
{
    *out = nullptr;
    const long fnnz = fill1_nnz(nx, ny, nz);
    if (nx < 1 || ny < 1 || nz < 1 || (long)nx * ny * nz != (long)n || fnnz > 0x7fffffffL) return LSSP_AMD_EINVAL;
    RefactorPlan *p = new RefactorPlan();
    p->nnz = fnnz;
    auto fill = [&]() -> int {
        LSSP_HIP(hipMalloc(&p->d_Fp, sizeof(int) * ((size_t)n + 1)));
        LSSP_HIP(hipMalloc(&p->d_Fj, sizeof(int) * (size_t)fnnz));
        LSSP_HIP(hipMalloc(&p->d_Fx, sizeof(double) * (size_t)fnnz));
        LSSP_HIP(hipMalloc(&p->d_dinv, sizeof(double) * (size_t)n));
        LSSP_HIP(hipMalloc(&p->d_rows, sizeof(int) * (size_t)n));
        LSSP_HIP(hipMalloc(&p->d_flag, sizeof(int)));
        LSSP_HIP(hipMalloc(&p->d_fin, (size_t)fnnz));
        LSSP_HIP(hipMalloc(&p->d_dpos, sizeof(int) * (size_t)n));
        LSSP_HIP(hipMemsetAsync(p->d_flag, 0, sizeof(int), c->stream));
        k_fill1_pattern<<<(unsigned)std::min<long>(((long)n + 255) / 256, 16384), 256, 0, c->stream>>>(
            n, fnnz, nx, ny, nz, p->d_Fp, p->d_Fj, p->d_fin, p->d_dpos, p->d_flag);
        LSSP_HIP(hipGetLastError());
        return LSSP_AMD_OK;
    };
    const int st = fill();
    if (st != LSSP_AMD_OK) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);
        refactor_plan_free(p);
        return st;
    }
    *out = p;
    return LSSP_AMD_OK;
}

int fill1_plan_levels(lssp_amd_ctx *c, RefactorPlan &p, int n, int nx, int ny, int nz)
{
    if (nx < 1 || ny < 1 || nz < 1) return LSSP_AMD_EINVAL;
    const int nlev = fill1_nlev(nx, ny, nz);
    std::vector<int> tab(2 * (size_t)nlev + 1);  // the two tables from the grid alone (no pass over the matrix)
    if (fill1_level_tables(nx, ny, nz, tab.data()) != (long)n) return LSSP_AMD_EINVAL;
    p.lev_off.assign(tab.begin() + nlev, tab.end());
    int *d_tab = nullptr;
    auto fill = [&]() -> int {
        LSSP_HIP(hipMalloc(&d_tab, sizeof(int) * tab.size()));
        LSSP_HIP(hipMemcpyAsync(d_tab, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice, c->stream));
        k_fill1_levels<<<(unsigned)std::min<long>(((long)n + 255) / 256, 16384), 256, 0, c->stream>>>(n, nx, ny, nlev, d_tab,
                                                                                                    p.d_rows, p.d_flag);
        LSSP_HIP(hipGetLastError());
        int bad = 1;
        LSSP_HIP(hipMemcpyAsync(&bad, p.d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        return bad ? LSSP_AMD_EINVAL : LSSP_AMD_OK;
    };
    const int st = fill();
    if (st != LSSP_AMD_OK) (void)hipStreamSynchronize(c->stream);
    if (d_tab) (void)hipFree(d_tab);
    return st;
}

int refactor_same_pattern(lssp_amd_ctx *c, const RefactorPlan &p, int n, const int *dAp, const int *dAj, int *same)
{
    LSSP_HIP(hipMemsetAsync(p.d_flag, 0, sizeof(int), c->stream));
    const long m = std::max<long>(n + 1, p.nnz);
    k_pattern_diff<<<(unsigned)std::min<long>((m + 255) / 256, 16384), 256, 0, c->stream>>>(n + 1, p.nnz, dAp, p.d_Fp,
                                                                                          dAj, p.d_Fj, p.d_flag);
    LSSP_HIP(hipGetLastError());
    int diff = 0;
    LSSP_HIP(hipMemcpyAsync(&diff, p.d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    *same = !diff;
    return LSSP_AMD_OK;
}

// ilu0_factor_gpu's launches on the plan's buffers (one block: blk = n)
int refactor_numeric(lssp_amd_ctx *c, RefactorPlan &p, int n, const double *dAx)
{
    LSSP_HIP(hipMemcpyAsync(p.d_Fx, dAx, sizeof(double) * p.nnz, hipMemcpyDeviceToDevice, c->stream));
    return refactor_levels(c, p, n);
}

// ---------------------------------------------------------------------------
// lssp_amd_iluk_refactor: the pattern rule and the scatter onto a pattern with
// fill (iluk_refactor_dev.h), one row per lane, grid-strided
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_iluk_match(int n, int nnz, const int *__restrict__ Ap,
                                                    const int *__restrict__ Aj, const int *__restrict__ Fp,
                                                    const int *__restrict__ Fj, const unsigned char *__restrict__ fin,
                                                    int *__restrict__ flag)
{
    int bad = 0;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < n; r += (long)gridDim.x * 256)
        bad |= iluk_match_row((int)r, nnz, Ap, Aj, Fp, Fj, fin);
    if (bad) atomicOr(flag, 1);
}

__global__ __launch_bounds__(256) void k_iluk_scatter(int n, const int *__restrict__ Ap, const double *__restrict__ Ax,
                                                      const int *__restrict__ Fp,
                                                      const unsigned char *__restrict__ fin, double *__restrict__ Fx)
{
    for (long r = blockIdx.x * 256L + threadIdx.x; r < n; r += (long)gridDim.x * 256)
        iluk_scatter_row((int)r, Ap, Ax, Fp, fin, Fx);
}

int iluk_match(lssp_amd_ctx *c, const RefactorPlan &p, int n, int nnz, const int *dAp, const int *dAj, int *ok)
{
    *ok = 0;
    LSSP_HIP(hipMemsetAsync(p.d_flag, 0, sizeof(int), c->stream));
    k_iluk_match<<<(unsigned)std::min<long>(((long)n + 255) / 256, 16384), 256, 0, c->stream>>>(n, nnz, dAp, dAj, p.d_Fp,
                                                                                              p.d_Fj, p.d_fin, p.d_flag);
    LSSP_HIP(hipGetLastError());
    int bad = 1;
    LSSP_HIP(hipMemcpyAsync(&bad, p.d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    *ok = !bad;
    return LSSP_AMD_OK;
}

int iluk_scatter(lssp_amd_ctx *c, RefactorPlan &p, int n, const int *dAp, const double *dAx)
{
    k_iluk_scatter<<<(unsigned)std::min<long>(((long)n + 255) / 256, 16384), 256, 0, c->stream>>>(n, dAp, dAx, p.d_Fp,
                                                                                                p.d_fin, p.d_Fx);
    LSSP_HIP(hipGetLastError());
    return LSSP_AMD_OK;
}

// k_ilu0_level over the kept level lists on d_Fx, in place
int refactor_levels(lssp_amd_ctx *c, RefactorPlan &p, int n)
{
    const int nlev = (int)p.lev_off.size() - 1;
    for (int l = 0; l < nlev; l++) {
        const int cnt = p.lev_off[l + 1] - p.lev_off[l];
        k_ilu0_level<<<(cnt + 255) / 256, 256, 0, c->stream>>>(p.d_rows + p.lev_off[l], cnt, p.d_Fp, p.d_Fj, p.d_Fx,
                                                              p.d_dinv, n);
    }
    LSSP_HIP(hipGetLastError());
    return LSSP_AMD_OK;
}

// the host copies Lx / Ux from the device factors (ilu_factor's split)
int refactor_host_factors(lssp_amd_ilu *M)
{
    if (M->brf) return bilu_refactor_host_factors(M);  // a BILUK handle (lssp_amd_bilu_refactor)
    if (M->host_missing && M->fd_Lp) {
        // a handle made from factors in HBM: its device copies come down once, then go
        lssp_amd_ctx *c = M->ctx;
        const size_t n1 = (size_t)M->n + 1, nl = (size_t)M->dev_nnzL, nu = (size_t)M->dev_nnzU;
        std::vector<int> Lp(n1), Lj(nl), Up(n1), Uj(nu);
        std::vector<double> Lx(nl), Ux(nu);
        LSSP_HIP(hipMemcpyAsync(Lp.data(), M->fd_Lp, sizeof(int) * n1, hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipMemcpyAsync(Lj.data(), M->fd_Lj, sizeof(int) * nl, hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipMemcpyAsync(Lx.data(), M->fd_Lx, sizeof(double) * nl, hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipMemcpyAsync(Up.data(), M->fd_Up, sizeof(int) * n1, hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipMemcpyAsync(Uj.data(), M->fd_Uj, sizeof(int) * nu, hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipMemcpyAsync(Ux.data(), M->fd_Ux, sizeof(double) * nu, hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        M->Lp = std::move(Lp);
        M->Lj = std::move(Lj);
        M->Lx = std::move(Lx);
        M->Up = std::move(Up);
        M->Uj = std::move(Uj);
        M->Ux = std::move(Ux);
        for (void *q : {(void *)M->fd_Lp, (void *)M->fd_Lj, (void *)M->fd_Lx, (void *)M->fd_Up, (void *)M->fd_Uj,
                        (void *)M->fd_Ux})
            (void)hipFree(q);
        M->fd_Lp = M->fd_Lj = M->fd_Up = M->fd_Uj = nullptr;
        M->fd_Lx = M->fd_Ux = nullptr;
        M->host_missing = M->host_stale = false;
        return LSSP_AMD_OK;
    }
    if (!M->host_stale || !M->rf) return LSSP_AMD_OK;
    lssp_amd_ctx *c = M->ctx;
    const int n = M->n;
    if (M->host_missing) {
        // a handle made by lssp_amd_ilu_create_dev: the patterns first, split from
        // the device F as ilu_factor splits them (row i of L: the columns below i,
        // then the unit diagonal; of U: the pivot, then the columns above i)
        std::vector<int> Fp((size_t)n + 1), Fj((size_t)M->rf->nnz);
        LSSP_HIP(hipMemcpyAsync(Fp.data(), M->rf->d_Fp, sizeof(int) * Fp.size(), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipMemcpyAsync(Fj.data(), M->rf->d_Fj, sizeof(int) * Fj.size(), hipMemcpyDeviceToHost, c->stream));
        LSSP_HIP(hipStreamSynchronize(c->stream));
        std::vector<int> Lp((size_t)n + 1), Up((size_t)n + 1);
        Lp[0] = Up[0] = 0;
        for (int i = 0; i < n; i++) {
            int nl = 0;
            while (Fp[i] + nl < Fp[i + 1] && Fj[Fp[i] + nl] < i) nl++;
            Lp[i + 1] = Lp[i] + nl + 1;
            Up[i + 1] = Up[i] + (Fp[i + 1] - Fp[i] - nl);
        }
        std::vector<int> Lj((size_t)Lp[n]), Uj((size_t)Up[n]);
        parallel_for(n, [&](long i0, long i1) {
            for (long i = i0; i < i1; i++) {
                const int nl = Lp[i + 1] - Lp[i] - 1, nu = Up[i + 1] - Up[i];
                for (int q = 0; q < nl; q++) Lj[Lp[i] + q] = Fj[Fp[i] + q];
                Lj[Lp[i + 1] - 1] = (int)i;
                for (int q = 0; q < nu; q++) Uj[Up[i] + q] = Fj[Fp[i] + nl + q];
            }
        });
        M->Lx.assign(Lj.size(), 0.0);
        M->Ux.assign(Uj.size(), 0.0);
        M->Lp = std::move(Lp);
        M->Lj = std::move(Lj);
        M->Up = std::move(Up);
        M->Uj = std::move(Uj);
        M->host_missing = false;
    }
    std::vector<double> Fx((size_t)M->rf->nnz);
    LSSP_HIP(hipMemcpyAsync(Fx.data(), M->rf->d_Fx, sizeof(double) * Fx.size(), hipMemcpyDeviceToHost, c->stream));
    LSSP_HIP(hipStreamSynchronize(c->stream));
    parallel_for(n, [&](long i0, long i1) {
        for (long i = i0; i < i1; i++) {
            const int nl = M->Lp[i + 1] - M->Lp[i] - 1, nu = M->Up[i + 1] - M->Up[i];
            size_t f = (size_t)(M->Lp[i] - i) + (size_t)M->Up[i];  // strict L entries + U entries of the rows before
            for (int q = 0; q < nl; q++) M->Lx[M->Lp[i] + q] = Fx[f + q];
            M->Lx[M->Lp[i + 1] - 1] = 1;
            for (int q = 0; q < nu; q++) M->Ux[M->Up[i] + q] = Fx[f + nl + q];
        }
    });
    M->host_stale = false;
    return LSSP_AMD_OK;
}

}  // namespace lssp_amd
