"""The line sweeps' coefficient streams have ONE builder per kind -- k_coef_refill
(tiled ILU(0)), k_linef_refill (skewed ILU(1)) -- which every create feeds: the
host creates with the lone L and the lone U, the device creates and the
refactors with the combined factor F (GPU box only).

At the smallest shapes that reach every branch, the host-created handle's
factors, applies and both single sweeps equal the oracle's and the
device-created handle's bit for bit (np.array_equal), and a refactor with the
creating values -- the same streams written again from F -- changes nothing.
Two inputs only a host create can carry: a non-unit L diagonal (from_factors)
and a plane cut (block-Jacobi).  The one-workgroup 2-D route (k_lineg) takes
its rows from the same row rules; the same grids run on the tiles in a child
process under LSSP_AMD_LINEG=0.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from inputs import uniform

pytestmark = pytest.mark.gpu

TILES = {0: (1, 16, 8), 1: (2, 16, 8)}  # lssp_amd_ilu_sweep_layout of the tiled sweeps, by level


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


def _box(nx, ny, nz, seed):
    """5-/7-pt stencil on an nx x ny x nz box (natural order, i fastest), random
    nonsymmetric diagonally dominant values"""
    rng = np.random.default_rng(seed)
    n, pl = nx * ny * nz, nx * ny
    Ap, Aj, Ax = [0], [], []
    for r in range(n):
        i, j, k = r % nx, r // nx % ny, r // pl
        cols = [c for c, ok in ((r - pl, k > 0), (r - nx, j > 0), (r - 1, i > 0), (r, True),
                                (r + 1, i < nx - 1), (r + nx, j < ny - 1), (r + pl, k < nz - 1)) if ok]
        vals = rng.uniform(-1, -0.1, len(cols))
        vals[cols.index(r)] = 7.0 + rng.uniform(0, 1)
        Aj += cols
        Ax += list(vals)
        Ap.append(len(Aj))
    return np.array(Ap, np.int32), np.array(Aj, np.int32), np.array(Ax)


def _identity(n):
    return O.CSR(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))


def _expected(L, U):
    """the oracle's results for one pair of factors, computed once per case: two applies, both sweeps"""
    n, one = L.n, _identity(L.n)
    return dict(L=L, U=U, applies=[O.ilu_apply(L, U, uniform(200 + rep, n)) for rep in range(2)],
                lower=O.ilu_apply(L, one, uniform(300, n)), upper=O.ilu_apply(one, U, uniform(300, n)))


def _check(dev, M, e, layout, other=None):
    """M == the oracle (== other, a handle made another way) in factors, applies and both single sweeps"""
    n = e["L"].n
    assert M.sweep_layout() == layout  # an "unsupported" answer cannot pass unnoticed
    want = (e["L"].Ap, e["L"].Aj, e["L"].Ax, e["U"].Ap, e["U"].Aj, e["U"].Ax)
    for h in (M, other) if other else (M,):
        assert h.sweep_layout() == layout
        (Lp, Lj, Lx), (Up, Uj, Ux) = h.factors()
        for name, got, w in zip(("Lp", "Lj", "Lx", "Up", "Uj", "Ux"), (Lp, Lj, Lx, Up, Uj, Ux), want):
            assert np.array_equal(got, w), name
    x, z = dev.vec(n), dev.vec(n)
    for rep in range(2):
        r = dev.vec(n, uniform(200 + rep, n))
        M.apply(x, r)
        assert np.array_equal(x.download(), e["applies"][rep]), rep
        if other:
            other.apply(z, r)
            assert np.array_equal(x.download(), z.download()), rep
    r = dev.vec(n, uniform(300, n))
    for which, key in ((0, "lower"), (1, "upper")):
        M.trisolve(which, x, r)
        assert np.array_equal(x.download(), e[key]), key
        if other:
            other.trisolve(which, z, r)
            assert np.array_equal(x.download(), z.download()), key


def _tiled_case(dev, level, box):
    """host create == device create == oracle on the tiles; refactors with the same values change nothing"""
    import lssp_amd
    nx, ny, nz = box
    Ap, Aj, Ax = _box(nx, ny, nz, 7 * nx + 3 * ny + nz + level)
    e = _expected(*O.ilu(O.CSR(Ap.size - 1, Ap, Aj, Ax), "iluk", level=level))
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    Mh = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=level)
    Md = (lssp_amd.DILU.create_dev if level == 0 else lssp_amd.DILU.iluk_create_dev)(dev, D, kind=lssp_amd.ILUK,
                                                                                    level=level)
    _check(dev, Mh, e, TILES[level], other=Md)
    for M in (Mh, Md):  # the streams again, from F: host-made (lone L, lone U before) and device-made
        if level == 0:
            M.refactor(D)
        else:
            M.iluk_refactor(D)
    _check(dev, Mh, e, TILES[level], other=Md)
    for h in (Mh, Md, D):
        h.close()


# 2 x 17 x 9: two j tiles (9 + 8 lines, one ragged) and two plane tiles (8 + 1): both hand-off
# directions; 3 x 20 x 5: ny no multiple of 16, fewer planes than a tile holds
@pytest.mark.parametrize("box", [(2, 17, 9), (3, 20, 5)], ids=["2x17x9", "3x20x5"])
def test_tiled_ilu0_host_create_equals_device_create(dev, box):
    _tiled_case(dev, 0, box)


# 3 x 9 x 9: 17 skewed columns in three tiles, planes 8 + 1, tiles off the grid; 4 x 13 x 7: 19
# skewed columns = 3 x 6 + 1, the odd surplus in the middle tile
@pytest.mark.parametrize("box", [(3, 9, 9), (4, 13, 7)], ids=["3x9x9", "4x13x7"])
def test_skewed_ilu1_host_create_equals_device_create(dev, box):
    _tiled_case(dev, 1, box)


@pytest.mark.parametrize("level", [0, 1], ids=["ilu0", "ilu1"])
def test_2d_one_workgroup_route(dev, level):
    """5-point 6 x 10 on k_lineg, whose host build takes each row from the shared row rule (no
    device create and no refactor serves this route)"""
    import lssp_amd
    Ap, Aj, Ax = _box(6, 10, 1, 61 + level)
    e = _expected(*O.ilu(O.CSR(Ap.size - 1, Ap, Aj, Ax), "iluk", level=level))
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=level)
    _check(dev, M, e, (1 + level, 10, 1))
    M.close()


def _tiles_2d_child():
    """(child process, LSSP_AMD_LINEG=0) the same 6 x 10 grids on the tiles, both levels"""
    import lssp_amd
    d = lssp_amd.Device(0)
    for level in (0, 1):
        _tiled_case(d, level, (6, 10, 1))
    d.close()
    print("tiles-2d ok")


def test_2d_on_the_tiles_in_a_child_process():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, LSSP_AMD_LINEG="0",
               PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    r = subprocess.run(cmd + ["-c", "import test_gpu_line_streams as T; T._tiles_2d_child()"], env=env, cwd=here,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tiles-2d ok" in r.stdout, r.stdout + r.stderr


def test_from_factors_with_a_non_unit_l_diagonal(dev):
    """the ILU(0) pattern of the 2 x 17 x 9 box with values no ILUK makes: L's diagonal is not 1.0,
    so the L sweep streams it (NA = 4) and must take the STORED value; every value an exact binary
    fraction.  Against the oracle's two triangular solves."""
    import lssp_amd
    Ap, Aj, Ax = _box(2, 17, 9, 99)
    L, U = O.ilu(O.CSR(Ap.size - 1, Ap, Aj, Ax), "iluk", level=0)
    rng = np.random.default_rng(17)
    n = L.n
    Lx = rng.choice([-0.5, -0.25, -0.125, 0.25, 0.375], L.Ax.size)
    Lx[L.Ap[1:] - 1] = rng.choice([0.5, 2.0, 4.0, 1.5], n)  # the diagonal, last in its row
    Ux = rng.choice([-0.5, -0.25, 0.125, 0.75], U.Ax.size)
    Ux[U.Ap[:-1]] = rng.choice([2.0, 4.0, 8.0, 3.0], n)  # the pivot, first in its row
    L, U = O.CSR(n, L.Ap, L.Aj, Lx), O.CSR(n, U.Ap, U.Aj, Ux)
    M = lssp_amd.DILU.from_factors(dev, (L.Ap, L.Aj, L.Ax), (U.Ap, U.Aj, U.Ax))
    _check(dev, M, _expected(L, U), TILES[0])
    M.close()


def test_create_with_a_plane_cut(dev):
    """block-Jacobi blocks of four planes cut the 3 x 20 x 6 box between planes 3 and 4: no plane
    coupling at k = 4, tiles of 4 + 2 planes, through lssp_amd_ilu_create"""
    import lssp_amd
    nx, ny, nz = 3, 20, 6
    Ap, Aj, Ax = _box(nx, ny, nz, 23)
    blk = 4 * nx * ny
    e = _expected(*O.ilu(O.CSR(Ap.size - 1, Ap, Aj, Ax), "iluk", level=0, blk=blk))
    assert e["L"].nnz < O.ilu(O.CSR(Ap.size - 1, Ap, Aj, Ax), "iluk", level=0)[0].nnz  # the cut is there
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0, blk=blk)
    _check(dev, M, e, TILES[0])
    M.close()
