"""CPU checks of lssp_amd_ilu_create_dev: declared in the header, exported by
the library, bound in the ctypes table, reachable from DILU, and the version
that introduced it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssp_amd.h")
LIB = os.path.join(ROOT, "lssp_amd", "lib", "liblssp_amd.so")
NAME = "lssp_amd_ilu_create_dev"


def test_create_dev_declared_exported_and_bound():
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
    # (ctx, A, kind, level, tol, p, blk, out): lssp_amd_ilu_create's arguments, the matrix as a handle
    assert len(_lib.SIGNATURES[NAME][1]) == 8


def test_dilu_create_dev_is_callable():
    import lssp_amd
    assert callable(lssp_amd.DILU.create_dev)


def test_version_is_at_least_10400():
    from lssp_amd import _lib
    assert _lib.load().lssp_amd_version() >= 10400
