#!/usr/bin/env python3
"""Generate tests/golden/assemble.npz + assemble.json: lssp_mat_sort_column,
lssp_mat_adjust_zero_diag, lssp_mat_get_block_diag and the two is_sorted
functions computed by the REFERENCE ITSELF (matrix-utils.cxx:217-279,
:387-698), called in oracle/_ref/libref.so directly through ctypes (they have
C++ linkage: the mangled names below are those `nm -D` lists; lssp_mat_csr is
passed and returned by value, type-defs.h:15-24).

Run where the reference checker is built:
    make -C oracle all ref && python tests/golden/make_golden_assemble.py

Same layout as conv.npz / conv.json (inputs and outputs both stored, arrays
`<case>__<name>`, loaded with allow_pickle=False).  The inputs are seeded
numpy and the small hand-written rows below, so the script is the whole recipe.
adjust_zero_diag is never given a row that holds its diagonal twice: the
reference under-allocates its output there (matrix-utils.cxx:516, :522).
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import oracle as O  # noqa: E402
from inputs import conv_rand  # noqa: E402

_pi, _pd = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)


class MatCSR(ctypes.Structure):  # lssp_mat_csr
    _fields_ = [("num_rows", ctypes.c_int), ("num_cols", ctypes.c_int), ("num_nnzs", ctypes.c_int),
                ("Ap", _pi), ("Aj", _pi), ("Ax", _pd)]


class MatBCSR(ctypes.Structure):  # lssp_mat_bcsr
    _fields_ = [("num_rows", ctypes.c_int), ("num_cols", ctypes.c_int), ("num_nnzs", ctypes.c_int),
                ("blk_size", ctypes.c_int), ("Ap", _pi), ("Aj", _pi), ("Ax", _pd)]


REF = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref.so"))
_sort = REF._Z20lssp_mat_sort_columnR13lssp_mat_csr_
_sort.restype, _sort.argtypes = None, [ctypes.POINTER(MatCSR)]
_csr_sorted = REF._Z22lssp_mat_csr_is_sorted13lssp_mat_csr_
_csr_sorted.restype, _csr_sorted.argtypes = ctypes.c_bool, [MatCSR]
_bcsr_sorted = REF._Z23lssp_mat_bcsr_is_sorted14lssp_mat_bcsr_
_bcsr_sorted.restype, _bcsr_sorted.argtypes = ctypes.c_bool, [MatBCSR]
_azd = REF._Z25lssp_mat_adjust_zero_diag13lssp_mat_csr_d
_azd.restype, _azd.argtypes = MatCSR, [MatCSR, ctypes.c_double]
_gbd = REF._Z23lssp_mat_get_block_diag13lssp_mat_csr_i
_gbd.restype, _gbd.argtypes = MatCSR, [MatCSR, ctypes.c_int]


def _csr(nr, nc, Ap, Aj, Ax):
    """(struct, the arrays it points into -- keep them alive)"""
    Ap = np.ascontiguousarray(Ap, np.int32)
    Aj = np.ascontiguousarray(Aj, np.int32).copy()
    Ax = np.ascontiguousarray(Ax, np.float64).copy()
    pj = Aj if Aj.size else np.zeros(1, np.int32)  # the asserts want non-NULL
    px = Ax if Ax.size else np.zeros(1)
    return MatCSR(nr, nc, int(Ap[-1]), Ap.ctypes.data_as(_pi), pj.ctypes.data_as(_pi), px.ctypes.data_as(_pd)), \
        (Ap, Aj, Ax, pj, px)


def _out(M: MatCSR, n: int):
    """the arrays the reference filled; their length is what its row pointers say
    (adjust_zero_diag leaves M.num_nnzs at the input's)"""
    Mp = np.ctypeslib.as_array(M.Ap, (n + 1,)).copy()
    m = int(Mp[-1])
    if m == 0:
        return Mp, np.zeros(0, np.int32), np.zeros(0)
    return Mp, np.ctypeslib.as_array(M.Aj, (m,)).copy(), np.ctypeslib.as_array(M.Ax, (m,)).copy()


def ref_sort_column(nr, nc, Ap, Aj, Ax):
    A, keep = _csr(nr, nc, Ap, Aj, Ax)
    _sort(ctypes.byref(A))
    return keep[1], keep[2]


def ref_adjust_zero_diag(n, Ap, Aj, Ax, tol):
    A, keep = _csr(n, n, Ap, Aj, Ax)
    return _out(_azd(A, tol), n)


def ref_get_block_diag(n, Ap, Aj, Ax, blk):
    A, keep = _csr(n, n, Ap, Aj, Ax)
    return _out(_gbd(A, blk), n)


def ref_csr_is_sorted(nr, nc, Ap, Aj):
    A, keep = _csr(nr, nc, Ap, Aj, np.zeros(len(Aj)))
    return int(_csr_sorted(A))


def ref_bcsr_is_sorted(nbr, nbc, bs, Bp, Bj):
    Bp, Bj = np.ascontiguousarray(Bp, np.int32), np.ascontiguousarray(Bj, np.int32)
    pj = Bj if Bj.size else np.zeros(1, np.int32)
    Bx = np.zeros(max(Bj.size, 1) * bs * bs)
    A = MatBCSR(nbr, nbc, int(Bp[-1]), bs, Bp.ctypes.data_as(_pi), pj.ctypes.data_as(_pi), Bx.ctypes.data_as(_pd))
    return int(_bcsr_sorted(A))


def from_rows(rows, vals=None, seed=0):
    """CSR from a list of column lists; values seeded unless given"""
    Ap = np.zeros(len(rows) + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=Ap[1:])
    Aj = np.asarray([c for r in rows for c in r], np.int32)
    Ax = np.random.default_rng(seed).uniform(-1, 1, Aj.size) if vals is None else np.asarray(vals, np.float64)
    return Ap, Aj, Ax


def one_diag(n, Ap, Aj, Ax):
    """drop the repeated occurrences of a row's diagonal (see the module docstring)"""
    rows = np.repeat(np.arange(n), np.diff(Ap))
    d = np.flatnonzero(Aj == rows)
    drop = d[1:][rows[d[1:]] == rows[d[:-1]]]
    keep = np.ones(Aj.size, bool)
    keep[drop] = False
    Bp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=Bp[1:])
    return Bp, Aj[keep], Ax[keep]


def sort_inputs():
    rng = np.random.default_rng(4242)
    mats = {}
    # rows of length 0, 1, 2 (in and out of order); a sorted row with adjacent duplicates
    # (untouched); unsorted rows with duplicates (last value wins)
    mats["small_rows"] = (9, 8) + from_rows([[], [5], [2, 6], [6, 2], [1, 1, 3, 3, 7], [7, 3, 3, 1, 3, 7, 0],
                                             [4, 4], [5, 4, 5, 4, 5], []], seed=1)
    # one row of 1,000 unsorted entries drawn from 600 of 1,500 columns (many duplicates; the
    # reference's index buffer holds num_cols entries, :432, so a row is no longer than that)
    # between a sorted row of 300 with duplicates (untouched) and short rows
    pool = rng.choice(1500, 600, replace=False)
    long_uns = pool[rng.integers(0, 600, 1000)].tolist()
    long_srt = np.sort(pool[rng.integers(0, 600, 300)]).tolist()
    mats["long_row"] = (5, 1500) + from_rows([[3, 1], long_srt, long_uns, [], [1499, 0, 1499]], seed=2)
    mats["rect_37x53"] = (37, 53) + conv_rand(37, 53, 6, 13, True)
    mats["rnd_sq60"] = (60, 60) + conv_rand(60, 60, 7, 11, True)
    A = O.poisson(2, 6)
    mats["p5_6"] = (A.n, A.n, A.Ap, A.Aj, A.Ax)
    return mats


def azd_inputs():
    mats = {}
    # 0: sorted, the new entry first; 1: has its diagonal; 2: empty; 3: sorted, in the middle;
    # 4: unsorted, stops early (after 1: [6, 1, (4), 7, 5]); 5: unsorted with its diagonal;
    # 6: unsorted, every column greater (goes first); 7: sorted, last; 8: unsorted, none greater (stays last)
    mats["placements"] = (9,) + from_rows([[3, 5], [0, 1, 4], [], [1, 6], [6, 1, 7, 5], [8, 5, 0], [8, 7],
                                           [2, 4], [3, 0, 1]], seed=3)
    mats["n1_empty"] = (1,) + from_rows([[]])
    mats["n1_diag"] = (1,) + from_rows([[0]], vals=[-0.0])
    A = O.poisson(3, 4)
    mats["p7_4_none_missing"] = (A.n, A.Ap, A.Aj, A.Ax)
    mats["rnd_sq60"] = (60,) + one_diag(60, *conv_rand(60, 60, 7, 21, True))
    mats["rnd_sq23"] = (23,) + one_diag(23, *conv_rand(23, 23, 5, 22, False))
    return mats


def gbd_inputs():
    mats = {}
    mats["rnd_sq23"] = (23,) + conv_rand(23, 23, 6, 31, True)   # 23: no multiple of 3; empty rows
    A = O.poisson(2, 6)
    mats["p5_6"] = (A.n, A.Ap, A.Aj, A.Ax)
    # every entry outside its block for blk <= 3; an empty row
    mats["off_block"] = (7,) + from_rows([[6, 5], [4], [], [0, 6], [0, 1], [1, 2, 0], [0, 3]], seed=5)
    return mats


def main():
    arrays, cases = {}, []

    def add(kind, name, params, inputs, outputs):
        key = f"{kind}_{name}"
        for k, v in list(inputs.items()) + list(outputs.items()):
            arrays[f"{key}__{k}"] = np.ascontiguousarray(v)
        cases.append({"kind": kind, "name": key, "params": params, "inputs": sorted(inputs),
                      "outputs": sorted(outputs)})

    for name, (nr, nc, Ap, Aj, Ax) in sort_inputs().items():
        Sj, Sx = ref_sort_column(nr, nc, Ap, Aj, Ax)
        add("sort_column", name, {"nrows": nr, "ncols": nc}, {"Ap": Ap, "Aj": Aj, "Ax": Ax}, {"Sj": Sj, "Sx": Sx})
        v = ref_csr_is_sorted(nr, nc, Ap, Aj)
        add("csr_is_sorted", name, {"nrows": nr, "ncols": nc}, {"Ap": Ap, "Aj": Aj},
            {"sorted": np.array([v], np.int32)})
        w = ref_csr_is_sorted(nr, nc, Ap, Sj)
        add("csr_is_sorted", name + "_after_sort", {"nrows": nr, "ncols": nc}, {"Ap": Ap, "Aj": Sj},
            {"sorted": np.array([w], np.int32)})
    for name, (nr, nc, rows) in {"equal_neighbours": (3, 5, [[2, 2, 2], [0, 4, 4], [1]]),
                                 "descending_across_rows": (3, 5, [[3, 4], [0, 1], [0]]),
                                 "one_pair": (3, 5, [[0, 1], [2, 3, 4], [1, 0]]),
                                 "nnz0": (4, 4, [[], [], [], []])}.items():
        Ap, Aj, _ = from_rows(rows)
        add("csr_is_sorted", name, {"nrows": nr, "ncols": nc}, {"Ap": Ap, "Aj": Aj},
            {"sorted": np.array([ref_csr_is_sorted(nr, nc, Ap, Aj)], np.int32)})
        add("bcsr_is_sorted", name, {"nbrows": nr, "nbcols": nc, "bs": 2}, {"Bp": Ap, "Bj": Aj},
            {"sorted": np.array([ref_bcsr_is_sorted(nr, nc, 2, Ap, Aj)], np.int32)})
    for name, (n, Ap, Aj, Ax) in azd_inputs().items():
        for tol in (1e-8, 0.5):
            Mp, Mj, Mx = ref_adjust_zero_diag(n, Ap, Aj, Ax, tol)
            add("adjust_zero_diag", f"{name}_tol{tol:g}", {"n": n, "tol": float(tol).hex()},
                {"Ap": Ap, "Aj": Aj, "Ax": Ax}, {"Mp": Mp, "Mj": Mj, "Mx": Mx})
    for name, (n, Ap, Aj, Ax) in gbd_inputs().items():
        for blk in (1, 3, n - 1, n, n + 5):
            Mp, Mj, Mx = ref_get_block_diag(n, Ap, Aj, Ax, blk)
            add("get_block_diag", f"{name}_blk{blk}", {"n": n, "blk": blk}, {"Ap": Ap, "Aj": Aj, "Ax": Ax},
                {"Mp": Mp, "Mj": Mj, "Mx": Mx})

    np.savez_compressed(os.path.join(HERE, "assemble.npz"), **arrays)
    with open(os.path.join(HERE, "assemble.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_assemble.py",
                   "source": "oracle/_ref/libref.so (reference compiled in place, g++ -O2)", "cases": cases},
                  f, indent=1)
    print(f"{len(cases)} cases, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
