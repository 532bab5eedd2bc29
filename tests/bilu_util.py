"""Inputs and a numpy restatement for the BILUK tests (test_bilu_cpu.py,
test_gpu_bilu.py).

block_grid: an N^dim grid of cells with a (2 dim + 1)-point stencil and bs
unknowns per cell.  Diagonal blocks are (1.5 dim + 0.1) J + U(-1, 1)^(bs x bs)
with J the anti-identity, so the block inversion has to pivot; off-diagonal
blocks are -w I + U(-0.2, 0.2)^(bs x bs), w ~ U(0.5, 1).

bilu_numpy: pc-biluk.cxx restated in numpy with the block inverse and the block
product passed in (LAPACK + netlib order, or numpy's own), for the CPU test's
bound; it shares no code with the library.
"""
from __future__ import annotations

import numpy as np

import oracle as O

# The shapes (dim, N, bs): 8^3 x 3 (n = 1536), 6^3 x 4 (864), 16^2 x 2 (512), 8^3 x 1 (512: looks
# like a structured ILU(0) to the line-sweep detection), 4^3 x 8 (512: the largest device block),
# 3^3 x 9 (243: the host numeric path, and rows too long for the packet sweeps).
# (dim, N, bs, level, shuffle, variant): levels 0 and 1 on the first two shapes; columns
# shuffled in half of the cases; "holes": a few in-block entries deleted from the CSR;
# "nodiag": one diagonal block deleted (its inverse is the identity)
CASES = [(3, 8, 3, 0, False, None), (3, 8, 3, 1, True, None), (3, 6, 4, 0, True, None), (3, 6, 4, 1, False, None),
         (2, 16, 2, 0, False, None), (3, 8, 1, 0, True, None), (3, 4, 8, 0, False, None), (3, 3, 9, 0, True, None),
         (2, 16, 2, 0, True, "holes"), (2, 16, 2, 0, False, "nodiag")]


def case_name(c):
    dim, N, bs, level, shuffle, variant = c
    return f"{N}^{dim}-bs{bs}-l{level}" + ("-shuf" if shuffle else "") + (f"-{variant}" if variant else "")


def block_grid(dim, N, bs, seed=0, shuffle=False, variant=None):
    """(Ap, Aj, Ax) of the block-stencil matrix.  variant: None, "holes" (a few
    off-diagonal entries of off-diagonal blocks deleted), "nodiag" (the diagonal
    block of the middle cell deleted), "zerodiag" (the diagonal block of cell 0 present
    and all 0.0: no elimination step touches it, so it is exactly singular when inverted)."""
    rng = np.random.default_rng(seed)
    nb = N ** dim
    strides = [N ** d for d in range(dim)]
    mid = nb // 2
    J = np.eye(bs)[::-1]
    rows = [[] for _ in range(nb * bs)]
    for i in range(nb):
        coord = [(i // s) % N for s in strides]
        nbrs = [(i - strides[d], coord[d] > 0) for d in reversed(range(dim))] + [(i, True)] + \
               [(i + strides[d], coord[d] < N - 1) for d in range(dim)]
        for j, ok in nbrs:
            if not ok:
                continue
            if j == i:
                B = (1.5 * dim + 0.1) * J + rng.uniform(-1, 1, (bs, bs))
                if variant == "zerodiag" and i == 0:
                    B = np.zeros((bs, bs))
                if variant == "nodiag" and i == mid:
                    continue
            else:
                B = -rng.uniform(0.5, 1) * np.eye(bs) + rng.uniform(-0.2, 0.2, (bs, bs))
            for r in range(bs):
                for c in range(bs):
                    if variant == "holes" and j != i and r != c and rng.uniform() < 0.1:
                        continue
                    rows[i * bs + r].append((j * bs + c, B[r, c]))
    Ap, Aj, Ax = [0], [], []
    for row in rows:
        if shuffle:
            row = [row[k] for k in rng.permutation(len(row))]
        Aj += [c for c, _ in row]
        Ax += [v for _, v in row]
        Ap.append(len(Aj))
    return np.array(Ap, np.int32), np.array(Aj, np.int32), np.array(Ax)


def diag_csr(n, bs, Dinv):
    """the block diagonal D as CSR (lssp_pc_biluk_assemble_diag_mat, pc-biluk.cxx:279-314)"""
    nb = n // bs
    blocks = np.asarray(Dinv).reshape(nb, bs, bs)  # [block, column, row]
    Dp = np.arange(n + 1, dtype=np.int32) * bs
    Dj = ((np.arange(n) // bs * bs)[:, None] + np.arange(bs)[None, :]).astype(np.int32)
    Dx = blocks.transpose(0, 2, 1)  # [block, row, column]
    return O.CSR(n, Dp, Dj.reshape(-1).copy(), np.ascontiguousarray(Dx).reshape(-1).copy())


def identity(n):
    return O.CSR(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))


def bilu_apply(n, bs, L, Dinv, U, rhs):
    """x = U^-1 D L^-1 rhs (lssp_pc_bilu_solve, pc-biluk.cxx:22-60) with the oracle's sweeps
    (an identity partner factor gives a single sweep) and product"""
    Lc, Uc, one = O.CSR(n, *L), O.CSR(n, *U), identity(n)
    y = O.ilu_apply(Lc, one, np.ascontiguousarray(rhs))
    z = O.spmv(0, diag_csr(n, bs, Dinv), y)
    return O.ilu_apply(one, Uc, z)


# ---- pc-biluk.cxx in numpy ---------------------------------------------------------
def gemm_netlib(A, B, alpha, C, beta):
    """netlib dgemm('N','N') order; n == 1 is pc-biluk.cxx:95-97"""
    n = A.shape[0]
    if n == 1:
        return A * B * alpha + beta * C
    C = np.zeros_like(C) if beta == 0 else (C.copy() if beta == 1 else beta * C)
    for l in range(n):
        C = C + (alpha * B[l:l + 1, :]) * A[:, l:l + 1]
    return C


def gemm_numpy(A, B, alpha, C, beta):
    return beta * C + alpha * (A @ B)


def inv_lapack(A):
    """dgetrf + dgetri, as pc-biluk.cxx:62-86; None when singular"""
    from scipy.linalg import lapack
    if A.shape[0] == 1:
        return None if A[0, 0] == 0.0 else 1.0 / A
    lu, piv, info = lapack.dgetrf(A)
    if info != 0:
        return None
    out, info = lapack.dgetri(lu, piv)
    return None if info != 0 else out


def inv_numpy(A):
    return np.linalg.inv(A)


def block_pattern(Ap, Aj, bs, level):
    """block rows' sorted block columns: A's own for level 0 (pc-biluk.cxx:339-346), else the
    oracle's ILUK(level) pattern of the block graph (lssp_pc_iluk_symbolic_fac)"""
    nb = (Ap.size - 1) // bs
    pat = [sorted({int(c) // bs for c in Aj[Ap[i * bs]:Ap[(i + 1) * bs]]}) for i in range(nb)]
    if level == 0:
        return pat
    Gp = np.zeros(nb + 1, np.int32)
    Gp[1:] = np.cumsum([len(p) for p in pat])
    Gj = np.array([c for p in pat for c in p], np.int32)
    Gx = np.where(Gj == np.repeat(np.arange(nb), np.diff(Gp)), 100.0, -1.0)
    L, U = O.ilu(O.CSR(nb, Gp, Gj, Gx), "iluk", level=level)
    return [sorted(set(L.Aj[L.Ap[i]:L.Ap[i + 1]].tolist()) | set(U.Aj[U.Ap[i]:U.Ap[i + 1]].tolist()))
            for i in range(nb)]


def bilu_numpy(Ap, Aj, Ax, bs, level, inv=inv_lapack, gemm=gemm_netlib):
    """((Lp, Lj, Lx), Dinv, (Up, Uj, Ux)) as lssp_pc_biluk_assemble leaves them"""
    n = Ap.size - 1
    nb = n // bs
    pat = block_pattern(Ap, Aj, bs, level)
    blk = [{j: np.zeros((bs, bs)) for j in p} for p in pat]
    for r in range(n):
        for k in range(Ap[r], Ap[r + 1]):
            blk[r // bs][int(Aj[k]) // bs][r % bs, int(Aj[k]) % bs] = Ax[k]
    invs = []
    for i in range(nb):
        cols = pat[i]
        for a, k in enumerate(cols):
            if k >= i:
                break
            blk[i][k] = gemm(blk[i][k].copy(), invs[k], 1.0, blk[i][k], 0.0)
            for j in cols[a + 1:]:
                if j in blk[k]:
                    blk[i][j] = gemm(blk[i][k], blk[k][j], -1.0, blk[i][j], 1.0)
        if i in blk[i]:
            d = inv(blk[i][i].copy())
            if d is None:
                raise ZeroDivisionError("bilu(0) singular diagonal submatrix")
            invs.append(d)
        else:
            invs.append(np.eye(bs))
    Lp, Lj, Lx, Up, Uj, Ux = [0], [], [], [0], [], []
    for i in range(nb):
        ub = {j: gemm(invs[i], blk[i][j], 1.0, np.zeros((bs, bs)), 0.0) for j in pat[i] if j > i}
        for r in range(bs):
            for j in pat[i]:
                if j < i:
                    Lj += range(j * bs, (j + 1) * bs)
                    Lx += blk[i][j][r].tolist()
            Lj.append(i * bs + r)
            Lx.append(1.0)
            Lp.append(len(Lj))
            Uj.append(i * bs + r)
            Ux.append(1.0)
            for j in pat[i]:
                if j > i:
                    Uj += range(j * bs, (j + 1) * bs)
                    Ux += ub[j][r].tolist()
            Up.append(len(Uj))
    Dinv = np.concatenate([d.T.reshape(-1) for d in invs])  # column-major blocks
    return ((np.array(Lp, np.int32), np.array(Lj, np.int32), np.array(Lx)), Dinv,
            (np.array(Up, np.int32), np.array(Uj, np.int32), np.array(Ux)))


def rel_distance(a, b):
    """max |delta| / max |value| over L, Dinv and U"""
    va = np.concatenate([a[0][2], a[1], a[2][2]])
    vb = np.concatenate([b[0][2], b[1], b[2][2]])
    return float(np.max(np.abs(va - vb)) / np.max(np.abs(va)))
