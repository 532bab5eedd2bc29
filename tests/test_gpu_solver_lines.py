"""The verb = 2 lines of BiCGSTAB, CG, QMRCGSTAB and ORTHOMIN, string for string.

tests/test_gpu_gmres_lines.py pins the GMRES family's lines by their parts and
tests/test_gpu_batch_stops.py the `itr:` lines of the batched drivers; the
header (maximal iteration, the three tolerances) and the footer (total
iteration, total time) of the four drivers here were read by no test.  One
set-up: 7-pt Poisson 6^3, no preconditioner, b = 1, x0 = 0, at most 3
iterations, all tolerances 0, restart 2 (ORTHOMIN's k; GMRES's m).

EXPECTED holds what each driver printed before the header, the footer and the
`itr:` line were folded into one printer each (solvers.cpp: print_header,
print_footer, print_itr): the lists were recorded from the build of the commit
before that fold.  The number after `total time:` is masked.  GMRES is here
once more so that the shared printers are pinned on the Gm side by full strings.
"""
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 6
TIME = re.compile(r"(total time: ).*\n$")

EXPECTED = {
    "bicgstab": [
        "bicgstab: maximal iteration: 3\n",
        "bicgstab: tolerance abs: 0\n",
        "bicgstab: tolerance rel: 0\n",
        "bicgstab: tolerance rbn: 0\n",
        "bicgstab: itr:     0, abs res: 5.668248e+00, rel res: 3.856754e-01, rbn: 3.856754e-01\n",
        "bicgstab: itr:     1, abs res: 1.913315e+00, rel res: 1.301846e-01, rbn: 1.301846e-01\n",
        "bicgstab: itr:     2, abs res: 4.089665e-01, rel res: 2.782665e-02, rbn: 2.782665e-02\n",
        "bicgstab: total iteration: 3\n",
        "bicgstab: total time: *\n",
    ],
    "cg": [
        "cg: maximal iteration: 3\n",
        "cg: tolerance abs: 0\n",
        "cg: tolerance rel: 0\n",
        "cg: tolerance rbn: 0\n",
        "cg: itr:     0, abs res: 1.200000e+01, rel res: 8.164966e-01, rbn: 8.164966e-01\n",
        "cg: itr:     1, abs res: 7.090288e+00, rel res: 4.824330e-01, rbn: 4.824330e-01\n",
        "cg: itr:     2, abs res: 3.647569e+00, rel res: 2.481856e-01, rbn: 2.481856e-01\n",
        "cg: total iteration: 3\n",
        "cg: total time: *\n",
    ],
    "qmrcgstab": [
        "qmrcgstab: maximal iteration: 3\n",
        "qmrcgstab: tolerance abs: 0\n",
        "qmrcgstab: tolerance rel: 0\n",
        "qmrcgstab: tolerance rbn: 0\n",
        "qmrcgstab: itr:    0, rel res: 3.856754e-01\n",
        "qmrcgstab: itr:    1, rel res: 1.301846e-01\n",
        "qmrcgstab: itr:    2, rel res: 2.782665e-02\n",
        "qmrcgstab: total iteration: 3\n",
        "qmrcgstab: total time: *\n",
        "qmrcgstab: absolute error (residual): 14.6969\n",
    ],
    "orthomin": [
        "orthomin: k parameter m: 2\n",
        "orthomin: maximal iteration: 3\n",
        "orthomin: tolerance abs: 0\n",
        "orthomin: tolerance rel: 0\n",
        "orthomin: tolerance rbn: 0\n",
        "orthomin: itr:     0, abs res: 9.295160e+00, rel res: 6.324555e-01, rbn: 6.324555e-01\n",
        "orthomin: itr:     1, abs res: 5.637424e+00, rel res: 3.835781e-01, rbn: 3.835781e-01\n",
        "orthomin: itr:     2, abs res: 3.062434e+00, rel res: 2.083722e-01, rbn: 2.083722e-01\n",
        "orthomin: total iteration: 3\n",
        "orthomin: total time: *\n",
    ],
    "gmres": [
        "gmres: restart parameter m: 2\n",
        "gmres: maximal iteration: 3\n",
        "gmres: tolerance abs: 0\n",
        "gmres: tolerance rel: 0\n",
        "gmres: tolerance rbn: 0\n",
        "gmres: itr:    2 /     2, abs res: 5.637424e+00, rel res: 3.835781e-01, rbn: 3.835781e-01\n",
        "gmres: itr:    4 /     4, abs res: 2.623551e+00, rel res: 1.785100e-01, rbn: 1.785100e-01\n",
        "gmres: total iteration: 4\n",
        "gmres: total time: *\n",
    ],
}
HEADER_LINES = {"bicgstab": 4, "cg": 4, "qmrcgstab": 4, "orthomin": 5}


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def mat(dev):
    import lssp_amd
    A = lssp_amd.DMat(dev, *lssp_amd.poisson(3, N))
    yield A
    A.close()


def _lines(dev, A, name, bval):
    import lssp_amd
    lines = []
    CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p)
    cb = CB(lambda user, msg: lines.append(msg.decode()) or 0)
    L = lssp_amd._lib.load()
    n = N ** 3
    x, b = dev.vec(n, np.zeros(n)), dev.vec(n, np.full(n, bval))
    L.lssp_amd_set_print(ctypes.cast(cb, ctypes.c_void_p), None)
    try:
        r = lssp_amd.solve(dev, A, None, x, b, solver=getattr(lssp_amd, name.upper()), tol_rel=0.0, tol_abs=0.0,
                           tol_rb=0.0, maxit=3, restart=2, verb=2)
    finally:
        L.lssp_amd_set_print(None, None)
    lines = [TIME.sub(r"\1*\n", ln) for ln in lines]
    print(name, r.nits, repr(r.residual))
    print(repr(lines))
    return r, lines


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_verbose_lines_are_the_recorded_ones(dev, mat, name):
    r, lines = _lines(dev, mat, name, 1.0)
    assert lines == EXPECTED[name]


@pytest.mark.parametrize("name", sorted(HEADER_LINES))
def test_early_exit_prints_the_header_and_nothing_else(dev, mat, name):
    """b = 0: the driver leaves through res <= tol_abs before its first iteration, without a footer"""
    r, lines = _lines(dev, mat, name, 0.0)
    k = HEADER_LINES[name]
    assert r.nits == 0
    assert lines == EXPECTED[name][:k]
    assert [ln.split(": ")[1] for ln in lines[-4:]] == ["maximal iteration", "tolerance abs", "tolerance rel",
                                                        "tolerance rbn"]
