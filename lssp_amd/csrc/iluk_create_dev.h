// iluk_create_dev.h -- the per-row bodies of lssp_amd_iluk_create_dev's kernels
// (DESIGN.md 3.3d): k_fill1_pattern and k_fill1_levels (ilu_factor.hip) call
// them, one row per lane.  They are plain host + device functions so that their
// index arithmetic also runs on the host, under a sanitizer, against the
// symbolic ILU(1) of the box's stencil and its longest-path levels
// (tools/iluk_create_dev_check.cpp).
//
// The ILU(1) pattern F of the complete natural-order 7-point box nx x ny x nz
// (5-point grid: nz = 1), nx, ny >= 3 (pc-iluk.cxx:22-135 on that stencil; what
// linefill.hip's detect_fill1 demands of a host-made factor): row r = (i, j, k)
// holds column r + dk * pl + dj * nx + di (pl = nx * ny) for each of the 13
// neighbours (di, dj, dk) below that lies inside the box, ascending in this
// order.  The seven with |di| + |dj| + |dk| <= 1 are the matrix's own entries
// (flag 1), the other six are fill of level 1 (flag 0).
#pragma once

#include "bilu_dev.h"

namespace lssp_amd {

constexpr int FILL1_NB = 13, FILL1_DIAG = 6;

// neighbour q of the list above: its (di, dj, dk)
BILU_HD inline void fill1_nb(int q, int &di, int &dj, int &dk)
{
    //                 B  BE  BN   S  SE   W   .   E  NW   N  TS  TW   T
    const int DI[FILL1_NB] = {0, 1, 0, 0, 1, -1, 0, 1, -1, 0, 0, -1, 0};
    const int DJ[FILL1_NB] = {0, 0, 1, -1, -1, 0, 0, 0, 1, 1, -1, 0, 0};
    const int DK[FILL1_NB] = {-1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1};
    di = DI[q];
    dj = DJ[q];
    dk = DK[q];
}

// members of [lo, hi) below x
BILU_HD inline long fill1_below(long x, long lo, long hi) { return (x < lo ? lo : x > hi ? hi : x) - lo; }

// Fp[r] in closed form, r = (i, j, k) in [0, n]; r = n is (0, 0, nz) and gives
// F's entry count.  Neighbour (di, dj, dk) exists for the rows of the sub-box
// I x J x K with I = [max(0, -di), nx - max(0, di)) and J, K alike; of those,
// the rows before (i, j, k) in natural order are the planes of K below k, on
// plane k the lines of J below j, on line j the rows of I below i.
BILU_HD inline long fill1_row_start(long i, long j, long k, long nx, long ny, long nz)
{
    long s = 0;
    for (int q = 0; q < FILL1_NB; q++) {
        int di, dj, dk;
        fill1_nb(q, di, dj, dk);
        const long i0 = di < 0 ? 1 : 0, i1 = nx - (di > 0), j0 = dj < 0 ? 1 : 0, j1 = ny - (dj > 0);
        const long k0 = dk < 0 ? 1 : 0, k1 = nz - (dk > 0);
        if (k1 <= k0) continue;  // (nz = 1: no neighbour below or above the plane)
        s += fill1_below(k, k0, k1) * (j1 - j0) * (i1 - i0);
        if (k >= k0 && k < k1) {
            s += fill1_below(j, j0, j1) * (i1 - i0);
            if (j >= j0 && j < j1) s += fill1_below(i, i0, i1);
        }
    }
    return s;
}

// the length of row (i, j, k): the neighbours inside the box
BILU_HD inline int fill1_row_len(int i, int j, int k, int nx, int ny, int nz)
{
    const int ci = 1 + (i > 0) + (i < nx - 1), cj = 1 + (j > 0) + (j < ny - 1);
    // dk = 0: (0, 0), (+-1, 0), (0, +-1), (+1, -1), (-1, +1); dk = -1: (0, 0), (+1, 0), (0, +1); dk = +1 mirrored
    const int mid = ci + cj - 1 + (i < nx - 1 && j > 0) + (i > 0 && j < ny - 1);
    const int lo = k > 0 ? 1 + (i < nx - 1) + (j < ny - 1) : 0, hi = k < nz - 1 ? 1 + (i > 0) + (j > 0) : 0;
    return mid + lo + hi;
}

// Row (i, j, k) of F: its columns into cols[0 .. len), its flag bytes into
// fin[0 .. len); *dp = the diagonal's place in the row.  Returns len =
// fill1_row_len <= 13.
BILU_HD inline int fill1_row(int i, int j, int k, int nx, int ny, int nz, int *cols, unsigned char *fin, int *dp)
{
    const long pl = (long)nx * ny, r = ((long)k * ny + j) * nx + i;
    int len = 0;
    for (int q = 0; q < FILL1_NB; q++) {
        int di, dj, dk;
        fill1_nb(q, di, dj, dk);
        const int ii = i + di, jj = j + dj, kk = k + dk;
        if (ii < 0 || ii >= nx || jj < 0 || jj >= ny || kk < 0 || kk >= nz) continue;
        if (q == FILL1_DIAG) *dp = len;
        cols[len] = (int)(r + dk * pl + (long)dj * nx + di);
        fin[len] = (unsigned char)((di != 0) + (dj != 0) + (dk != 0) <= 1);
        len++;
    }
    return len;
}

// Row (i, j, k) is on level l = i + 2 j + 3 k of F's strict-lower DAG (its
// longest chain runs through W: l - 1, SE: l - 1, BN: l - 1); inside a level rows
// ascend, i.e. by k, then j (level_lists' order).  With c2(m) = the number of (i,
// j) of the plane on i + 2 j = m and S3[x] = c2(x) + c2(x - 3) + c2(x - 6) + ...,
// the rows of level l on the planes below k are c2(l), c2(l - 3), .., c2(l - 3 (k
// - 1)) = S3[l] - S3[l - 3 k], and on plane k the lines j' < j that meet m = i +
// 2 j inside the plane: j' >= (m - nx + 2) / 2 where m >= nx.  S3 and off (the
// levels' first positions) have nlev = nx + 2 ny + 3 nz - 5 and nlev + 1 entries.
// fill1_level_tables writes tab = S3[0 .. nlev), off[0 .. nlev] (2 nlev + 1
// entries) from the grid alone and returns off[nlev], which is n on a box:
// level l holds c2(l - 3 k) rows of each plane k, S3[l] - S3[l - 3 nz] in all.
inline int fill1_nlev(int nx, int ny, int nz) { return nx + 2 * ny + 3 * nz - 5; }
inline long fill1_level_tables(int nx, int ny, int nz, int *tab)
{
    const int nlev = fill1_nlev(nx, ny, nz);
    int *S3 = tab, *off = tab + nlev;
    for (int x = 0; x < 2 * nlev + 1; x++) tab[x] = 0;
    for (int j = 0; j < ny; j++)
        for (int i = 0; i < nx; i++) S3[i + 2 * j]++;
    for (int x = 3; x < nlev; x++) S3[x] += S3[x - 3];
    long o = 0;
    for (int l = 0; l < nlev; l++) {
        o += S3[l] - (l >= 3 * nz ? S3[l - 3 * nz] : 0);
        off[l + 1] = (int)o;
    }
    return o;
}

// fill1_level_pos returns the row's position in the level-ordered list.
BILU_HD inline long fill1_level_pos(int i, int j, int k, int nx, const int *S3, const int *off)
{
    const int m = i + 2 * j, l = m + 3 * k;
    const int jmin = m >= nx ? (m - nx + 2) / 2 : 0;
    return (long)off[l] + (S3[l] - S3[m]) + (j - jmin);
}

}  // namespace lssp_amd
