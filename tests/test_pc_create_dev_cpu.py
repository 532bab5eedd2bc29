"""CPU checks of lssp_amd_pc_create_dev: declared in the header, exported by the
library, bound in the ctypes table, the Python method, the version that
introduced it, and the symbolic kernel's row body
(lssp_amd/csrc/iluk_symbolic_dev.h) run on the host by
tools/iluk_symbolic_check.cpp -- a loop over 64 lanes between the kernel's
synchronisation points -- against the oracle's ILUK pattern: F is the union
pattern of the oracle's L and U, the flag bytes say "column is in A's row", and
dpos points at each row's diagonal."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
from ilut_inputs import arrow, csr, poisson7, random_sorted, tridiag
from pc_create_inputs import five, oracle_rows, symbolic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssp_amd.h")
LIB = os.path.join(ROOT, "lssp_amd", "lib", "liblssp_amd.so")
NAME = "lssp_amd_pc_create_dev"


def test_pc_create_dev_declared_exported_and_bound():
    import ctypes
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lssp_amd_\w+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (lssp_amd_\w+)", out))
    from lssp_amd import _lib
    lib = _lib.load()
    assert NAME in declared
    assert NAME in exported
    assert NAME in _lib.SIGNATURES
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
    # (ctx, A, kind, level, tol, p, blk, out) -> int
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int
    assert args[:2] == [ctypes.c_void_p, ctypes.c_void_p]
    assert args[2:7] == [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    assert len(args) == 8
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert m
    want = ("lssp_amd_ctx *ctx, const lssp_amd_mat *A, int kind, int level, double tol, int p, int blk, "
            "lssp_amd_ilu **out")
    assert re.sub(r"\s+", " ", m.group(1)).strip() == want


def test_python_handle_has_the_method():
    import lssp_amd
    assert callable(lssp_amd.DILU.pc_create_dev)


def test_version_is_at_least_11000():
    from lssp_amd import _lib
    assert _lib.load().lssp_amd_version() >= 11000


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("iluk") / "iluk_symbolic_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "lssp_amd", "csrc"),
                    os.path.join(ROOT, "tools", "iluk_symbolic_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp_path, Ap, Aj, level, cap):
    n, nnz = Ap.size - 1, Aj.size
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([n, nnz], np.int32).tofile(f)
        Ap.astype(np.int32).tofile(f)
        Aj.astype(np.int32).tofile(f)
    out = subprocess.run([exe, fin, fout, str(level), str(cap)], capture_output=True, text=True)
    if out.returncode != 0:
        return out.returncode, None
    assert out.stdout.startswith("ok:")
    with open(fout, "rb") as f:
        fnnz = int(np.fromfile(f, np.int32, 1)[0])
        got = (np.fromfile(f, np.int32, n + 1), np.fromfile(f, np.int32, fnnz), np.fromfile(f, np.uint8, fnnz),
               np.fromfile(f, np.int32, n))
        assert f.read() == b""
    return 0, got


CASES = [
    ("five-l0", five, 0), ("five-l1", five, 1), ("five-l2", five, 2),
    ("rand300-l1", lambda: random_sorted(21), 1), ("rand300-l2", lambda: random_sorted(21), 2),
    ("p7-6-l1", lambda: poisson7(6), 1), ("p7-6-l2", lambda: poisson7(6), 2), ("p7-6-l3", lambda: poisson7(6), 3),
    ("tridiag200-l1", lambda: tridiag(200), 1),
    ("arrow70-l1", lambda: arrow(70), 1),  # working rows of 69 entries: the merge takes several passes of the wave
    ("n1", lambda: csr([{0: 2.5}]), 1),
    ("n2", lambda: csr([{0: 2.0, 1: -1.0}, {0: -1.0, 1: 2.0}]), 1),
]


@pytest.mark.parametrize("name,make,level", CASES, ids=[c[0] for c in CASES])
def test_row_body_equals_the_oracle(harness, tmp_path, name, make, level):
    Ap, Aj, Ax = make()
    n = Ap.size - 1
    L, U = O.ilu(O.CSR(n, Ap, Aj, Ax), "iluk", level=level)
    want = oracle_rows(L, U)
    assert want == symbolic(Ap, Aj, level)  # the restatement the min-rule comparisons rest on
    if name == "five-l1":  # the case keeps discriminating between the two level rules
        assert want[3] == [0, 1, 3]
        assert symbolic(Ap, Aj, level, rule="min")[3] == [0, 1, 3, 4]
    if name == "arrow70-l1":
        assert max(len(r) for r in want) > 64
    st, got = _run(harness, tmp_path, Ap, Aj, level, 128)
    assert st == 0
    Fp, Fj, fin, dpos = got
    assert np.array_equal(Fp, np.concatenate(([0], np.cumsum([len(r) for r in want]))))
    assert np.array_equal(Fj, np.concatenate(want))
    inA = np.concatenate([np.isin(want[i], Aj[Ap[i]:Ap[i + 1]]) for i in range(n)])
    assert np.array_equal(fin, inA.astype(np.uint8))
    assert np.array_equal(Fj[dpos], np.arange(n))
    assert np.all((dpos >= Fp[:-1]) & (dpos < Fp[1:]))


def test_row_body_reports_a_working_row_beyond_the_capacity(harness, tmp_path):
    Ap, Aj, Ax = arrow(70)  # row 0 holds 69 entries right of its diagonal
    assert _run(harness, tmp_path, Ap, Aj, 1, 64)[0] == 3
    assert _run(harness, tmp_path, Ap, Aj, 1, 128)[0] == 0
