"""CPU checks of lssp_amd_iluk_create_dev: declared in the header, exported by the
library, bound in the ctypes table with lssp_amd_ilu_create_dev's signature, the
Python method, the version that introduced it, and the index arithmetic of its
kernels' per-row bodies (lssp_amd/csrc/iluk_create_dev.h) run on the host against
independent restatements (tools/iluk_create_dev_check.cpp)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssp_amd.h")
LIB = os.path.join(ROOT, "lssp_amd", "lib", "liblssp_amd.so")
NAME = "lssp_amd_iluk_create_dev"


def test_iluk_create_dev_declared_exported_and_bound():
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
    # (ctx, A, kind, level, tol, p, blk, out) -> int, as its sibling
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES["lssp_amd_ilu_create_dev"]
    args = {}
    for name in (NAME, "lssp_amd_ilu_create_dev"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        args[name] = re.sub(r"\s+", " ", m.group(1)).strip()
    assert args[NAME] == args["lssp_amd_ilu_create_dev"]


def test_python_handle_has_the_method():
    import lssp_amd
    assert callable(lssp_amd.DILU.iluk_create_dev)


def test_version_is_at_least_10700():
    from lssp_amd import _lib
    assert _lib.load().lssp_amd_version() >= 10700


def test_kernel_row_bodies_match_the_symbolic_ilu1(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "iluk_create_dev_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "lssp_amd", "csrc"),
                    os.path.join(ROOT, "tools", "iluk_create_dev_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("ok:")
