"""Shared helpers of the device-assembly tests (tests/golden/assemble.*): the
fixture loader and short numpy restatements of lssp_mat_csr_is_sorted /
lssp_mat_sort_column / lssp_mat_adjust_zero_diag / lssp_mat_get_block_diag
(matrix-utils.cxx:217-279, :387-698), vectorised so they run on matrices of a
few hundred thousand rows.  tests/test_assemble_cpu.py pins them to the
reference's own outputs."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def assemble_cases():
    with open(os.path.join(GOLDEN, "assemble.json")) as f:
        cases = json.load(f)["cases"]
    with np.load(os.path.join(GOLDEN, "assemble.npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    for c in cases:
        c["in"] = {k: arrays[f"{c['name']}__{k}"] for k in c["inputs"]}
        c["out"] = {k: arrays[f"{c['name']}__{k}"] for k in c["outputs"]}
    return cases


def _rows(Ap):
    return np.repeat(np.arange(Ap.size - 1, dtype=np.int64), np.diff(Ap))


def _descending(Ap, Aj):
    """entries k >= 1 of one row with Aj[k-1] > Aj[k]"""
    d = np.zeros(Aj.size, bool)
    if Aj.size > 1:
        d[1:] = Aj[:-1] > Aj[1:]
        start = Ap[:-1][np.diff(Ap) > 0]
        d[start] = False
    return d


def is_sorted(Ap, Aj) -> int:
    """lssp_mat_csr_is_sorted / lssp_mat_bcsr_is_sorted: equal neighbours are sorted"""
    return 0 if _descending(Ap, Aj).any() else 1


def sort_column(Ap, Aj, Ax):
    """lssp_mat_sort_column: only rows with a descending pair change; they come out
    ascending, every duplicate column with the value of its last occurrence"""
    Aj, Ax = Aj.copy(), Ax.copy()
    rows = _rows(Ap)
    uns = np.zeros(Ap.size - 1, bool)
    uns[rows[_descending(Ap, Aj)]] = True
    sel = np.flatnonzero(uns[rows])          # ascending: row by row, the row's own positions
    if sel.size == 0:
        return Aj, Ax
    order = np.lexsort((Aj[sel], rows[sel]))  # stable: equal (row, column) keep the input order
    r, c, v = rows[sel][order], Aj[sel][order], Ax[sel][order]
    last = np.ones(sel.size, bool)
    last[:-1] = (r[:-1] != r[1:]) | (c[:-1] != c[1:])
    ends = np.flatnonzero(last)
    run = np.cumsum(np.concatenate(([0], last[:-1].astype(np.int64))))
    Aj[sel] = c
    Ax[sel] = v[ends[run]]
    return Aj, Ax


def adjust_zero_diag(n, Ap, Aj, Ax, tol):
    """lssp_mat_adjust_zero_diag -> (Mp, Mj, Mx): (i, 1 * tol) appended to a row without a
    diagonal, then moved left past the trailing entries whose column is greater"""
    rows = _rows(Ap)
    q = np.arange(Aj.size, dtype=np.int64) - Ap[rows]
    has = np.zeros(n, bool)
    has[rows[Aj == rows]] = True
    Mp = np.zeros(n + 1, np.int64)
    np.cumsum(np.diff(Ap) + ~has, out=Mp[1:])
    le = Aj <= rows
    p = np.full(n, -1, np.int64)
    np.maximum.at(p, rows[le], q[le])
    p += 1                                   # after the last entry whose column is not greater
    Mj, Mx = np.zeros(Mp[-1], np.int32), np.zeros(Mp[-1])
    dest = Mp[rows] + q + (~has[rows] & (q >= p[rows]))
    Mj[dest], Mx[dest] = Aj, Ax
    new = np.flatnonzero(~has)
    Mj[Mp[new] + p[new]] = new
    Mx[Mp[new] + p[new]] = 1 * tol
    return Mp.astype(np.int32), Mj, Mx


def get_block_diag(n, Ap, Aj, Ax, blk):
    """lssp_mat_get_block_diag -> (Mp, Mj, Mx): blk == n copies; else each row keeps the
    columns of its own diagonal block, and a row left with none gets (row, 1.0)"""
    if blk == n:
        return Ap.copy(), Aj.copy(), Ax.copy()
    rows = _rows(Ap)
    start = rows // blk * blk
    keep = (Aj >= start) & (Aj < np.minimum(start + blk, n))
    cnt = np.bincount(rows[keep], minlength=n)
    Kp = np.concatenate(([0], np.cumsum(cnt)))
    Mp = np.concatenate(([0], np.cumsum(np.where(cnt == 0, 1, cnt))))
    Mj, Mx = np.zeros(Mp[-1], np.int32), np.zeros(Mp[-1])
    rk = rows[keep]
    dest = Mp[rk] + np.arange(rk.size) - Kp[rk]
    Mj[dest], Mx[dest] = Aj[keep], Ax[keep]
    none = np.flatnonzero(cnt == 0)
    Mj[Mp[none]], Mx[Mp[none]] = none, 1.0
    return Mp.astype(np.int32), Mj, Mx
