"""The phase lines of LSSP_AMD_SETUP_TIMES=1 (GPU box only).

One child process makes a handle through each device creator, runs the three
refactors and destroys everything; its stderr must carry, call by call, exactly
the `lssp_amd <tag>: <phase> <seconds> s` lines listed in EXPECTED, in that
order, and none of them when the variable is unset.  The lists were recorded
from the library as it stood before the phase clocks were folded into one
(PhaseClock, internal.h): the tags and phase names are what the parsers under
tools/ match.

The `lssp_amd setup:` lines of the host setup (setup_mark, SetupTimer) are left
out: one of them is printed from a worker thread, so their order is not fixed.
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^lssp_amd ([a-z_]+): (.*?)[ \t]+([0-9.]+) s$")

CHILD = r'''
import os, sys, numpy as np
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import lssp_amd
import bilu_util, ilut_inputs, pc_create_inputs, sched_inputs
import test_gpu_create_dev as T0
import test_gpu_iluk_create_dev as T1


def call(name):
    os.write(2, ("== " + name + "\n").encode())


dev = lssp_amd.Device(0)
nx, ny, nz = min((b for b, _ in T0.CASES), key=lambda b: b[0] * b[1] * b[2])
A0 = T0._box7(nx, ny, nz, 1)
D0 = lssp_amd.DMat(dev, *A0)
call("ilu_create_dev")
M0 = lssp_amd.DILU.create_dev(dev, D0, kind=lssp_amd.ILUK, level=0)

nx, ny, nz = min((b for b, _ in T1.CASES), key=lambda b: b[0] * b[1] * b[2])
D1 = lssp_amd.DMat(dev, *T1._box7(nx, ny, nz, 1))
call("iluk_create_dev")
M1 = lssp_amd.DILU.iluk_create_dev(dev, D1, kind=lssp_amd.ILUK, level=1)

name, make, tol, p = min(ilut_inputs.CASES, key=lambda c: c[1]()[0].size)
D2 = lssp_amd.DMat(dev, *make())
call("ilut_create_dev")
M2 = lssp_amd.DILU.ilut_create_dev(dev, D2, tol=tol, p=p)
# strict rows of 199 entries: beyond the device schedule builder, so the download and the host schedules
D2b = lssp_amd.DMat(dev, *ilut_inputs.arrow(200))
call("ilut_create_dev, host schedules")
M2b = lssp_amd.DILU.ilut_create_dev(dev, D2b, tol=0.0, p=200)

Ap, Aj = pc_create_inputs.pattern("rand6")
D3 = lssp_amd.DMat(dev, Ap, Aj, pc_create_inputs.values(Ap, Aj, 0))
call("pc_create_dev")
M3 = lssp_amd.DILU.pc_create_dev(dev, D3, level=0)

L, U = min((make() for _, make in sched_inputs.CASES), key=lambda f: f[0][0].size)
dL = (dev.idx(L[0].size, L[0]), dev.idx(L[1].size, L[1]), dev.vec(L[2].size, L[2]))
dU = (dev.idx(U[0].size, U[0]), dev.idx(U[1].size, U[1]), dev.vec(U[2].size, U[2]))
call("ilu_from_factors_dev")
M4 = lssp_amd.DILU.from_factors_dev(dev, dL, dU)

D3.update_values(dev.vec(Aj.size, pc_create_inputs.values(Ap, Aj, 1)))
call("iluk_refactor")
M3.iluk_refactor(D3)

D0.update_values(dev.vec(A0[2].size, A0[2] * 1.5))
call("ilu_refactor")
M0.refactor(D0)

dim, N, bs, level, shuffle, variant = min((c for c in bilu_util.CASES if c[2] <= 8), key=lambda c: c[1] ** c[0] * c[2])
B = bilu_util.block_grid(dim, N, bs, seed=1, shuffle=shuffle, variant=variant)
call("bilu_create")
M5 = lssp_amd.DILU.bilu(dev, *B, bs, level=level)
D5 = lssp_amd.DMat(dev, B[0], B[1], B[2] * 1.25)
call("bilu_refactor")
M5.bilu_refactor(D5)
call("destroy")
for h in (M0, M1, M2, M2b, M3, M4, M5, D0, D1, D2, D2b, D3, D5):
    h.close()
dev.close()
print("ok")
'''.replace("ROOT", ROOT)

# (call, [(tag, phase), ...]) in the child's order
_SCHED = ["check", "levels", "order", "entries", "packets", "fill"]  # the device schedule builder's, per side
_BOTH = ["L " + s for s in _SCHED] + ["U " + s for s in _SCHED]


def _lines(tag, phases):
    return [(tag, p) for p in phases]


EXPECTED = [
    ("ilu_create_dev", _lines("create_dev", ["pattern check", "plan / levels", "numeric ILU(0)",
                                             "allocation + zeroing", "coefficient streams"])),
    ("iluk_create_dev", _lines("iluk_create_dev", ["pattern check", "F pattern", "levels", "scatter", "numeric",
                                                   "allocation", "refill"])),
    ("ilut_create_dev", _lines("ilut_create_dev", ["check", "numeric", "compaction"] + _BOTH)),
    ("ilut_create_dev, host schedules", _lines("ilut_create_dev", ["check", "numeric", "compaction", "download",
                                                                   "schedules"])),
    ("pc_create_dev", _lines("pc_create_dev", ["check", "symbolic", "levels", "scatter", "numeric", "split"] + _BOTH)),
    ("ilu_from_factors_dev", _lines("from_factors_dev", ["copies"] + _BOTH)),
    ("iluk_refactor", _lines("iluk_refactor", ["plan", "match", "scatter", "numeric", "refill"])),
    ("ilu_refactor", _lines("refactor", ["plan", "pattern compare", "numeric ILU(0)", "coefficient streams"])),
    ("bilu_create", []),  # the host setup's own lines only
    ("bilu_refactor", _lines("bilu_refactor", ["plan", "scatter + graph compare", "numeric BILU(0)", "U scaling",
                                               "packet refill + Dinv"])),
    ("destroy", []),
]

TAGS = {tag for _, lines in EXPECTED for tag, _ in lines}


def _run(env):
    res = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=170)
    assert res.returncode == 0 and "ok" in res.stdout, (res.stdout[-2000:], res.stderr[-4000:])
    return res.stderr.splitlines()


def test_every_call_prints_its_phase_lines_in_order():
    calls, seconds = [], []
    for line in _run(dict(os.environ, LSSP_AMD_SETUP_TIMES="1")):
        m = LINE.match(line)
        if line.startswith("== "):
            calls.append((line[3:], []))
        elif m and m.group(1) != "setup":
            calls[-1][1].append((m.group(1), m.group(2)))
            seconds.append(m.group(3))
    for got, want in zip(calls, EXPECTED):
        assert got == want
    assert len(calls) == len(EXPECTED)
    assert seconds and all(float(s) >= 0 for s in seconds)


def test_no_phase_line_without_the_variable():
    env = {k: v for k, v in os.environ.items() if k != "LSSP_AMD_SETUP_TIMES"}
    for line in _run(env):
        assert not (line.startswith("lssp_amd ") and line[9:].split(":")[0] in TAGS), line
