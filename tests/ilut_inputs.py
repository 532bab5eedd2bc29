"""Matrices of the lssp_amd_ilut_create_dev tests (CPU harness and GPU): sorted rows, each with its diagonal."""
import numpy as np

import oracle as O
from inputs import rand_csr


def csr(rows):
    """CSR arrays of a list of {col: val} rows, columns ascending"""
    Ap, Aj, Ax = [0], [], []
    for r in rows:
        for c in sorted(r):
            Aj.append(c)
            Ax.append(r[c])
        Ap.append(len(Aj))
    return np.array(Ap, np.int32), np.array(Aj, np.int32), np.array(Ax, np.float64)


def poisson7(N):
    A = O.poisson(3, N)
    return A.Ap, A.Aj, A.Ax


def box_random(nx, ny, nz, seed):
    """7-pt stencil on a box, random nonsymmetric values of both signs, no dominance: fill of every size, so the
    selection step swaps and qsplit cuts on values in no particular order"""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(nx * ny * nz):
        i, j, k = r % nx, r // nx % ny, r // (nx * ny)
        cols = [c for c, ok in ((r - nx * ny, k > 0), (r - nx, j > 0), (r - 1, i > 0), (r, True),
                                (r + 1, i < nx - 1), (r + nx, j < ny - 1), (r + nx * ny, k < nz - 1)) if ok]
        row = {c: float(rng.uniform(-1, 1)) for c in cols}
        row[r] = float(rng.uniform(1, 2))
        rows.append(row)
    return csr(rows)


def arrow(n, seed=3):
    """row 0 and column 0 full, plus a tridiagonal band: every later row fills completely at tol = 0"""
    rng = np.random.default_rng(seed)
    rows = [{c: float(rng.uniform(-1, -0.1)) for c in range(n)}]
    rows[0][0] = float(n)
    for i in range(1, n):
        row = {0: float(rng.uniform(-1, -0.1)), i: 4.0 + float(rng.uniform(0, 1))}
        if i > 1:
            row[i - 1] = float(rng.uniform(-1, -0.1))
        if i < n - 1:
            row[i + 1] = float(rng.uniform(-1, -0.1))
        rows.append(row)
    return csr(rows)


def tridiag(n, seed=4):
    rng = np.random.default_rng(seed)
    lo, di, up = rng.uniform(-1, -0.1, n), rng.uniform(2.5, 3.5, n), rng.uniform(-1, -0.1, n)
    rows = []
    for i in range(n):
        row = {i: float(di[i])}
        if i > 0:
            row[i - 1] = float(lo[i])
        if i < n - 1:
            row[i + 1] = float(up[i])
        rows.append(row)
    return csr(rows)


def random_sorted(seed, n=300, per_row=6):
    return rand_csr(n, per_row, seed, unsorted=False)


def pivot_cancels():
    """4 x 4: the second pivot is 2 - (1 / 1) * 2 = exactly 0.0, replaced by the guard"""
    return csr([{0: 1.0, 1: 2.0, 3: 0.5},
                {0: 1.0, 1: 2.0, 2: 1.0},
                {1: 0.5, 2: 3.0, 3: 1.0},
                {0: 0.25, 2: 1.0, 3: 5.0}])


def tiny_a00():
    """|a00| < 1e-10: the guard replaces row 0's divisor, U keeps the value"""
    return csr([{0: -1e-12, 1: 2.0, 3: 0.5},
                {0: 1.0, 1: 2.0, 2: 1.0},
                {1: 0.5, 2: 3.0, 3: 1.0},
                {0: 0.25, 2: 1.0, 3: 5.0}])


# (name, builder, tol, p): what the host harness of the row body and the GPU
# tests both factor; every one stays within 256 entries per part of the working row
CASES = [
    ("p7-8-fill", lambda: poisson7(8), 1e-4, 20),
    ("p7-8-drop", lambda: poisson7(8), 1e-2, 3),
    ("p7-8-default", lambda: poisson7(8), 1e-3, -1),
    ("box543-p1", lambda: box_random(5, 4, 3, 12), 0.0, 1),
    ("box543-p2", lambda: box_random(5, 4, 3, 12), 0.0, 2),
    ("arrow200", lambda: arrow(200), 0.0, 200),
    ("rand300", lambda: random_sorted(21), 1e-3, -1),
]
