"""CPU checks of lssp_amd_bilu_create_dev: declared in the header, exported by the
library, bound in the ctypes table with matching argtypes, the Python method,
the version that introduced it, and the index arithmetic of its two own kernels'
per-block-row bodies (lssp_amd/csrc/bilu_create_dev.h: the block graph and the
expansion to L and U) run on the host against independent restatements
(tools/bilu_create_check.cpp)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssp_amd.h")
LIB = os.path.join(ROOT, "lssp_amd", "lib", "liblssp_amd.so")
NAME = "lssp_amd_bilu_create_dev"


def test_bilu_create_dev_declared_exported_and_bound():
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
    # (ctx, A, level, bs, out) -> int: lssp_amd_bilu_create's (level, bs) order
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int
    assert args[:2] == [ctypes.c_void_p, ctypes.c_void_p]
    assert args[2:4] == [ctypes.c_int, ctypes.c_int]
    assert len(args) == 5
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % NAME, src)
    assert m
    want = "lssp_amd_ctx *ctx, const lssp_amd_mat *A, int level, int bs, lssp_amd_ilu **out"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == want


def test_python_handle_has_the_method():
    import inspect

    import lssp_amd
    assert callable(lssp_amd.DILU.bilu_create_dev)
    # DILU.bilu's argument order: (dev, matrix, bs, level=0)
    assert list(inspect.signature(lssp_amd.DILU.bilu_create_dev).parameters) == ["dev", "A", "bs", "level"]
    assert inspect.signature(lssp_amd.DILU.bilu_create_dev).parameters["level"].default == 0


def test_version_is_at_least_11100():
    from lssp_amd import _lib
    assert _lib.load().lssp_amd_version() >= 11100


def test_kernel_row_bodies_match_the_host_restatements(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "bilu_create_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "lssp_amd", "csrc"),
                    os.path.join(ROOT, "tools", "bilu_create_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("ok:")
    assert int(out.stdout.split()[1]) > 1000
