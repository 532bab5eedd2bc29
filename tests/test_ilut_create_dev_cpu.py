"""CPU checks of lssp_amd_ilut_create_dev: declared in the header, exported by the
library, bound in the ctypes table, the Python method, the version that
introduced it, and the kernel's row body (lssp_amd/csrc/ilut_dev.h) run on the host
by tools/ilut_dev_check.cpp -- a loop over 64 lanes between the kernel's
synchronisation points -- against the oracle's ILUT, bit for bit."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
from ilut_inputs import CASES, arrow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssp_amd.h")
LIB = os.path.join(ROOT, "lssp_amd", "lib", "liblssp_amd.so")
NAME = "lssp_amd_ilut_create_dev"


def test_ilut_create_dev_declared_exported_and_bound():
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
    # (ctx, A, tol, p, blk, out) -> int
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int
    assert args[:2] == [ctypes.c_void_p, ctypes.c_void_p]
    assert args[2:5] == [ctypes.c_double, ctypes.c_int, ctypes.c_int]
    assert len(args) == 6
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert m
    want = "lssp_amd_ctx *ctx, const lssp_amd_mat *A, double tol, int p, int blk, lssp_amd_ilu **out"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == want


def test_python_handle_has_the_method():
    import lssp_amd
    assert callable(lssp_amd.DILU.ilut_create_dev)


def test_version_is_at_least_10800():
    from lssp_amd import _lib
    assert _lib.load().lssp_amd_version() >= 10800


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("ilut") / "ilut_dev_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "lssp_amd", "csrc"),
                    os.path.join(ROOT, "tools", "ilut_dev_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp_path, Ap, Aj, Ax, tol, p, cap):
    n, nnz = Ap.size - 1, Aj.size
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([n, nnz, p, cap], np.int32).tofile(f)
        np.array([tol], np.float64).tofile(f)
        Ap.astype(np.int32).tofile(f)
        Aj.astype(np.int32).tofile(f)
        Ax.astype(np.float64).tofile(f)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    if out.returncode != 0:
        return out.returncode, None
    assert out.stdout.startswith("ok:")
    with open(fout, "rb") as f:
        nl, nu = np.fromfile(f, np.int32, 2)
        got = []
        for nz in (nl, nu):
            got += [np.fromfile(f, np.int32, n + 1), np.fromfile(f, np.int32, nz), np.fromfile(f, np.float64, nz)]
        assert f.read() == b""
    return 0, got


@pytest.mark.parametrize("name,make,tol,p", CASES, ids=[c[0] for c in CASES])
def test_row_body_equals_the_oracle(harness, tmp_path, name, make, tol, p):
    Ap, Aj, Ax = make()
    L, U = O.ilu(O.CSR(Ap.size - 1, Ap, Aj, Ax), "ilut", tol=tol, p=p)
    st, got = _run(harness, tmp_path, Ap, Aj, Ax, tol, p, 256)
    assert st == 0
    for nm, g, w in zip(("Lp", "Lj", "Lx", "Up", "Uj", "Ux"), got, (L.Ap, L.Aj, L.Ax, U.Ap, U.Aj, U.Ax)):
        assert np.array_equal(g, w), nm


def test_row_body_reports_a_working_row_beyond_the_capacity(harness, tmp_path):
    Ap, Aj, Ax = arrow(200)  # rows fill to 199 entries
    assert _run(harness, tmp_path, Ap, Aj, Ax, 0.0, 200, 128)[0] == 3
