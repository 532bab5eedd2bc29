"""CPU checks of the device-assembly entry points: the numpy restatements the
GPU tests compare against (tests/assemble_util.py) reproduce every fixture the
reference wrote (tests/golden/assemble.*) bit for bit, and the new names are
declared, exported and bound."""
import os
import re
import subprocess

import numpy as np
import pytest

import assemble_util as U
from conv_util import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssp_amd.h")
LIB = os.path.join(ROOT, "lssp_amd", "lib", "liblssp_amd.so")
NEW = ["lssp_amd_csr_is_sorted", "lssp_amd_bcsr_is_sorted", "lssp_amd_csr_sort_columns_dev",
       "lssp_amd_csr_adjust_zero_diag", "lssp_amd_csr_get_block_diag", "lssp_amd_mat_from_device"]

CASES = U.assemble_cases()


def restate(kind, p, i):
    if kind == "sort_column":
        return dict(zip(("Sj", "Sx"), U.sort_column(i["Ap"], i["Aj"], i["Ax"])))
    if kind == "csr_is_sorted":
        return {"sorted": np.array([U.is_sorted(i["Ap"], i["Aj"])], np.int32)}
    if kind == "bcsr_is_sorted":
        return {"sorted": np.array([U.is_sorted(i["Bp"], i["Bj"])], np.int32)}
    if kind == "adjust_zero_diag":
        return dict(zip(("Mp", "Mj", "Mx"),
                        U.adjust_zero_diag(p["n"], i["Ap"], i["Aj"], i["Ax"], float.fromhex(p["tol"]))))
    assert kind == "get_block_diag"
    return dict(zip(("Mp", "Mj", "Mx"), U.get_block_diag(p["n"], i["Ap"], i["Aj"], i["Ax"], p["blk"])))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_restatement_bitwise_vs_reference(c):
    got = restate(c["kind"], c["params"], c["in"])
    assert sorted(got) == sorted(c["out"])
    for k, v in c["out"].items():
        assert same(got[k], v), k


def test_fixtures_cover_the_listed_cases():
    by = {}
    for c in CASES:
        by.setdefault(c["kind"], []).append(c)
    assert set(by) == {"sort_column", "csr_is_sorted", "bcsr_is_sorted", "adjust_zero_diag", "get_block_diag"}
    lens = np.concatenate([np.diff(c["in"]["Ap"]) for c in by["sort_column"]])
    assert {0, 1, 2} <= set(lens.tolist()) and lens.max() >= 1000
    assert any(c["params"]["nrows"] != c["params"]["ncols"] for c in by["sort_column"])
    for kind in ("csr_is_sorted", "bcsr_is_sorted"):
        assert {int(c["out"]["sorted"][0]) for c in by[kind]} == {0, 1}
    assert any(c["params"]["n"] == 1 for c in by["adjust_zero_diag"])
    assert any(c["out"]["Mj"].size == c["in"]["Aj"].size for c in by["adjust_zero_diag"])   # nothing missing
    for c in by["get_block_diag"]:
        n = c["params"]["n"]
        assert c["params"]["blk"] in (1, 3, n - 1, n, n + 5)


def test_header_library_and_ctypes_table_hold_the_new_names():
    from lssp_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(lssp_amd_\w+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (lssp_amd_\w+)", out))
    for name in NEW + ["lssp_amd_version"]:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
    assert _lib.load().lssp_amd_version() >= 10200


def test_python_entry_points_exist():
    import lssp_amd
    from lssp_amd import convert as C
    for name in ("csr_is_sorted", "bcsr_is_sorted", "sort_columns", "adjust_zero_diag", "get_block_diag"):
        assert callable(getattr(C, name)), name
    assert callable(lssp_amd.DMat.from_device)
