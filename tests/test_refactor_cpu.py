"""CPU checks of the value-refresh entry points (lssp_amd_mat_update_values,
lssp_amd_ilu_refactor): declared in the header, exported by the library, bound
in the ctypes table, and the version that introduced them."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssp_amd.h")
LIB = os.path.join(ROOT, "lssp_amd", "lib", "liblssp_amd.so")
NAMES = ("lssp_amd_mat_update_values", "lssp_amd_ilu_refactor")


def test_refresh_calls_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lssp_amd_\w+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (lssp_amd_\w+)", out))
    from lssp_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in declared
        assert name in exported
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_python_handles_have_the_methods():
    import lssp_amd
    assert callable(lssp_amd.DMat.update_values) and callable(lssp_amd.DILU.refactor)


def test_version_is_at_least_10300():
    from lssp_amd import _lib
    assert _lib.load().lssp_amd_version() >= 10300
