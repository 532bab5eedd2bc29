"""CPU checks of the device schedule builder (lssp_amd/csrc/tri_sched.hip): the two new C-ABI
names are declared in the header, exported, bound in the ctypes table with the right signatures,
and the version that introduced them; and the builder's lane-level bodies (lssp_amd/csrc/sched_dev.h)
run on the host by tools/sched_dev_check.cpp -- loops over 64 lanes between the kernels' wave-level
points -- against the host builder (sched_host.h: what tri_bp.cpp uploads), byte for byte, on both
factors of every case of sched_inputs.py.  Each case asserts, on the schedule itself, that it exercises
what it is named for."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sched_inputs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssp_amd.h")
LIB = os.path.join(ROOT, "lssp_amd", "lib", "liblssp_amd.so")

WANT = {
    "lssp_amd_ilu_from_factors_dev": "lssp_amd_ctx *ctx, int n, const int *dLp, const int *dLj, const double *dLx, "
                                     "const int *dUp, const int *dUj, const double *dUx, lssp_amd_ilu **out",
    "lssp_amd_ilu_get_schedule": "const lssp_amd_ilu *M, int which, int hdr[12], int *blk, int *desc, unsigned *rec, "
                                 "int *idx, int *perm, int *pos",
}


@pytest.mark.parametrize("name", sorted(WANT))
def test_declared_exported_and_bound(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lssp_amd_\w+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (lssp_amd_\w+)", out))
    from lssp_amd import _lib
    lib = _lib.load()
    assert name in declared and name in exported and name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert getattr(lib, name).argtypes == args and res is ctypes.c_int
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == WANT[name]
    if name.endswith("from_factors_dev"):  # (ctx, n, 6 device arrays, out)
        assert args == [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6 + [ctypes.POINTER(ctypes.c_void_p)]
    else:  # (M, which, hdr, 6 arrays)
        assert args == [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 7


def test_python_handle_has_the_methods():
    import lssp_amd
    assert callable(lssp_amd.DILU.from_factors_dev) and callable(lssp_amd.DILU.schedule)


def test_version_is_at_least_10900():
    from lssp_amd import _lib
    assert _lib.load().lssp_amd_version() >= 10900


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("sched") / "sched_dev_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "lssp_amd", "csrc"),
                    os.path.join(ROOT, "tools", "sched_dev_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tmp_path, L, U):
    n = L[0].size - 1
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([n, L[1].size, U[1].size], np.int32).tofile(f)
        for Tp, Tj, Tx in (L, U):
            Tp.astype(np.int32).tofile(f)
            Tj.astype(np.int32).tofile(f)
            Tx.astype(np.float64).tofile(f)
    out = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    if out.returncode != 0:
        return out.returncode, out.stdout
    assert out.stdout.count("ok:") == 2, out.stdout
    sides = []
    with open(fout, "rb") as f:
        for _ in range(2):
            s = dict(zip(S.HDR, (int(v) for v in np.fromfile(f, np.int32, 12))))
            s["counts"] = [int(v) for v in np.fromfile(f, np.int64, 3)]
            s["blk"] = np.fromfile(f, np.int32, s["nb"] + 1)
            s["desc"] = np.fromfile(f, np.int32, max(4 * s["npackets"], 1))
            s["rec"] = np.fromfile(f, np.uint32, s["rec_words"])
            s["idx"] = np.fromfile(f, np.int32, s["idx_words"])
            s["perm"] = np.fromfile(f, np.int32, n)
            s["pos"] = np.fromfile(f, np.int32, n)
            sides.append(s)
        assert f.read() == b""
    return 0, sides


@pytest.mark.parametrize("name,make", S.CASES, ids=[c[0] for c in S.CASES])
def test_lane_bodies_equal_the_host_builder(harness, tmp_path, name, make):
    L, U = make()
    st, sides = _run(harness, tmp_path, L, U)
    assert st == 0, sides
    S.check_case(name, L, U, *sides)
    for s in sides:
        assert s["origin"] == 1 and s["rows"] == S.ROWS
        assert np.array_equal(s["pos"][s["perm"]], np.arange(L[0].size - 1))


def test_grid_ilu0_factor_too(harness, tmp_path):
    L, U = S.ilu0_p7_8()
    st, sides = _run(harness, tmp_path, L, U)
    assert st == 0 and sides[0]["EP"] == 4 and sides[0]["unit"] == 1 and sides[1]["unit"] == 0


@pytest.mark.parametrize("name,make,status", S.REFUSALS, ids=[c[0] for c in S.REFUSALS])
def test_refusals_give_the_matching_exit_status(harness, tmp_path, name, make, status):
    L, U = make()
    st, _ = _run(harness, tmp_path, L, U)
    assert st == {1: 3, 6: 4}[status]
