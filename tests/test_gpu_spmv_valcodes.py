"""The SpMV's value coding (lssp_amd_mat::Av, k_spmv3's COL_VAL mode): one byte
per row that names the row -- pattern and values, bit for bit -- in a table of
the matrix's distinct rows, instead of the row's values.  The coding changes
which bytes the product reads, never a value: every comparison here is
bitwise, against the oracle and against the same product under
LSSP_AMD_SPMV_VALCODE=0 (the row-code mode, which reads Ax), which a child
process computes because the knob is read once.

The grids are those of test_gpu_spmv_rowcodes.py with values that depend on the
offset alone (a constant-coefficient stencil), so a matrix has as many distinct
rows as patterns.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from test_gpu_spmv_rowcodes import GRIDS, NITS, oracle_products, products, same, solve6, subsets

pytestmark = pytest.mark.gpu

ROWVAL_MAX = 256
# one value per direction (k-, j-, i-, diagonal, i+, j+, k+): diagonally dominant as box's are
STENCIL = (-0.35, -0.45, -0.55, 7.5, -0.65, -0.75, -0.85)


def cbox(nx, ny, nz, stencil=STENCIL, scale=None):
    """box's matrix (test_gpu_spmv_rowcodes.py) with the value of an entry given by its
    direction; scale: one factor per row"""
    n = nx * ny * nz
    r = np.arange(n)
    i, j, k = r % nx, r // nx % ny, r // (nx * ny)
    cand = [(r - nx * ny, k > 0), (r - nx, j > 0), (r - 1, i > 0), (r, np.ones(n, bool)), (r + 1, i < nx - 1),
            (r + nx, j < ny - 1), (r + nx * ny, k < nz - 1)]
    cols = np.stack([c for c, _ in cand], 1)
    ok = np.stack([m for _, m in cand], 1)
    vals = np.tile(np.asarray(stencil, np.float64), (n, 1))
    if scale is not None:
        vals = vals * np.asarray(scale, np.float64)[:, None]
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum(ok.sum(1), out=Ap[1:])
    return Ap, cols[ok].astype(np.int32), vals[ok]


def grid(name):
    return cbox(*GRIDS[name][0])


def check_products(dev, D, Ap, Aj, Ax, nr, nc):
    for q, (a, o) in enumerate(zip(products(dev, D, nr, nc), oracle_products(Ap, Aj, Ax, nr, nc))):
        assert same(a, o), q


def compute(dev):
    """name -> [value-row count, the products, the solve] of every grid"""
    import lssp_amd
    res = {}
    for name in GRIDS:
        Ap, Aj, Ax = grid(name)
        n = Ap.size - 1
        D = lssp_amd.DMat(dev, Ap, Aj, Ax)
        res[name] = [np.array([float(D.valcodes)])] + products(dev, D, n, n) + solve6(dev, D, Ap, Aj, Ax)
        D.close()
    return res


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0, reduction=lssp_amd.TREE)
    yield d
    d.close()


@pytest.fixture(scope="module")
def coded(dev):
    return compute(dev)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys, numpy as np
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import lssp_amd
import test_gpu_spmv_valcodes as T
dev = lssp_amd.Device(0, reduction=lssp_amd.TREE)
res = T.compute(dev)
np.savez(sys.argv[1], **{f"{k}/{i}": a for k, v in res.items() for i, a in enumerate(v)})
print("ok")
'''.replace("ROOT", ROOT)


@pytest.fixture(scope="module")
def row_mode(tmp_path_factory):
    """compute() in a child process whose products read Ax"""
    path = str(tmp_path_factory.mktemp("valcode") / "row_mode.npz")
    res = subprocess.run([sys.executable, "-c", CHILD, path], env=dict(os.environ, LSSP_AMD_SPMV_VALCODE="0"),
                         capture_output=True, text=True, timeout=170)
    assert res.returncode == 0 and "ok" in res.stdout, (res.stdout[-2000:], res.stderr[-2000:])
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(GRIDS))
def test_constant_grid_bitwise_vs_oracle_and_row_mode(coded, row_mode, name):
    Ap, Aj, Ax = grid(name)
    n = Ap.size - 1
    got = coded[name]
    assert int(got[0][0]) == GRIDS[name][1]  # as many distinct rows as patterns
    for q, (a, o) in enumerate(zip(got[1:6], oracle_products(Ap, Aj, Ax, n, n))):
        assert same(a, o), (name, "product", q)
    A = O.CSR(n, Ap, Aj, Ax)
    L, U = O.ilu(A, "iluk", level=0)
    o = O.solve(O.BICGSTAB, A, np.ones(n), L=L, U=U, rtol=0.0, atol=0.0, rbtol=0.0, maxit=NITS, mode=O.TREE,
                trace_cap=200)
    assert int(got[6][0]) == o.nits
    assert same(got[7], o.trace) and same(got[8], o.x)
    # the row mode knows the same value rows (the codes are built, not used) and computes the same bits
    for i, a in enumerate(got):
        assert same(a, row_mode[f"{name}/{i}"]), (name, i)


def test_piecewise_constant(dev):
    import lssp_amd
    nx, ny, nz = GRIDS["7pt_9x8x7"][0]
    scale = np.where(np.arange(nx * ny * nz) // (nx * ny) >= 4, 2.0, 1.0)
    Ap, Aj, Ax = cbox(nx, ny, nz, scale=scale)
    n = Ap.size - 1
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    assert D.rowcodes == 27 and 27 < D.valcodes <= 54
    check_products(dev, D, Ap, Aj, Ax, n, n)
    D.close()


def banded(nvals):
    """600 rows of one 3-entry pattern; row i carries value row i % nvals of nvals distinct ones"""
    nr, nc, Ap, Aj, _ = subsets([0b111], noff=3)
    t = (np.arange(nr) % nvals).astype(np.float64)
    Ax = np.stack([-0.25 - t / 1024, 3.0 + t / 512, -0.5 - t / 2048], 1).reshape(-1)
    return nr, nc, Ap, Aj, Ax


@pytest.mark.parametrize("nvals", [ROWVAL_MAX, ROWVAL_MAX + 1])
def test_eligibility_edges(dev, nvals):
    import lssp_amd
    nr, nc, Ap, Aj, Ax = banded(nvals)
    assert np.unique(Ax.reshape(nr, 3), axis=0).shape[0] == nvals
    D = lssp_amd.DMat(dev, Ap, Aj, Ax, ncols=nc)
    assert D.ndiag == 3 and D.rowcodes == 1  # the layers below a refusal are intact
    assert D.valcodes == (ROWVAL_MAX if nvals == ROWVAL_MAX else 0)
    check_products(dev, D, Ap, Aj, Ax, nr, nc)
    D.close()


def test_eight_entry_rows(dev):
    """rows of 8, 7 and 1 entries whose values depend on the offset alone: three value rows, and
    the kernel's eighth gather, which a 7-pt grid never issues"""
    import lssp_amd
    nr, nc, Ap, Aj, _ = subsets([0xFF, 0x7F, 0b1])
    row = np.repeat(np.arange(nr), np.diff(Ap))
    Ax = np.asarray([-0.9, 0.4, -0.3, 5.5, 0.2, -0.6, 0.7, -0.8, 0.1])[Aj - row]
    D = lssp_amd.DMat(dev, Ap, Aj, Ax, ncols=nc)
    assert D.rowcodes == 3 and D.valcodes == 3
    check_products(dev, D, Ap, Aj, Ax, nr, nc)
    D.close()


def test_bit_equality(dev):
    """rows that differ in the sign of a stored zero alone are different rows"""
    import lssp_amd
    nr, nc, Ap, Aj, Ax = banded(1)
    Ax = Ax.copy()
    Ax[0::3] = 0.0
    D = lssp_amd.DMat(dev, Ap, Aj, Ax, ncols=nc)
    assert D.valcodes == 1
    D.close()
    Ax[3 * 300] = -0.0
    assert np.array_equal(Ax[3 * 300:3 * 301], Ax[3 * 299:3 * 300])  # equal as numbers
    D = lssp_amd.DMat(dev, Ap, Aj, Ax, ncols=nc)
    assert D.valcodes == 2
    check_products(dev, D, Ap, Aj, Ax, nr, nc)
    D.close()


def test_empty_rows_and_missing_diagonals(dev):
    import lssp_amd
    Ap, Aj, Ax = grid("7pt_9x8x7")
    n = Ap.size - 1
    row = np.repeat(np.arange(n), np.diff(Ap))
    keep = ~np.isin(row, (0, 255, 256, 503)) & ~((Aj == row) & (row % 5 == 0))
    Ap2 = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(row[keep], minlength=n), out=Ap2[1:])
    Aj2, Ax2 = Aj[keep], Ax[keep]
    D = lssp_amd.DMat(dev, Ap2, Aj2, Ax2)
    assert D.rowcodes > 0 and D.valcodes == D.rowcodes and D.ndiag == 7
    check_products(dev, D, Ap2, Aj2, Ax2, n, n)
    D.close()


def test_lifecycle(dev):
    import lssp_amd
    dims = GRIDS["7pt_9x8x7"][0]
    Ap, Aj, Ax = cbox(*dims)
    n = Ap.size - 1
    up = lssp_amd.DMat(dev, Ap, Aj, Ax)
    dAp, dAj, dAx = dev.idx(Ap.size, Ap), dev.idx(Aj.size, Aj), dev.vec(Ax.size, Ax)
    fd = lssp_amd.DMat.from_device(dev, n, n, Aj.size, dAp, dAj, dAx)
    assert (fd.valcodes, fd.rowcodes, fd.device_bytes) == (up.valcodes, up.rowcodes, up.device_bytes)
    assert up.valcodes == 27
    coded_bytes = up.device_bytes
    for a, b in zip(products(dev, fd, n, n), products(dev, up, n, n)):
        assert same(a, b)
    rand = np.random.default_rng(9).uniform(-1, 1, Ax.size)
    other = cbox(*dims, stencil=STENCIL[:3] + (9.25,) + STENCIL[4:])[2]
    for vals, want in ((rand, 0), (Ax, 27), (other, 27)):
        for D in (fd, up):
            D.update_values(dev.vec(vals.size, vals))
            assert D.valcodes == want and D.rowcodes == 27
            if want:
                assert D.device_bytes == coded_bytes
            else:
                assert D.device_bytes[1] < coded_bytes[1]  # the codes and the table are gone
            check_products(dev, D, Ap, Aj, vals, n, n)
        assert fd.device_bytes == up.device_bytes
    fd.close()
    up.close()


ORDER = r'''
import sys, numpy as np
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import lssp_amd
import test_gpu_spmv_valcodes as T
dev = lssp_amd.Device(0, reduction=lssp_amd.TREE)
Ap, Aj, Ax = lssp_amd.poisson(3, 64)
n = Ap.size - 1
D = lssp_amd.DMat(dev, Ap, Aj, Ax)
assert D.valcodes == 27
np.savez(sys.argv[1], *T.products(dev, D, n, n))
print("ok")
'''.replace("ROOT", ROOT)


def test_block_order(dev, tmp_path):
    """64^3 (plane = 16 blocks) in column groups of 2 and 16 block streams, in a child process
    (the knobs are read once): other workgroups take the blocks, the sums stay those of this
    process's default order"""
    import lssp_amd
    env = {"LSSP_AMD_SPMV_ORDER": "2", "LSSP_AMD_SPMV_STREAMS": "16"}
    assert not any(k in os.environ for k in env)
    path = str(tmp_path / "order.npz")
    res = subprocess.run([sys.executable, "-c", ORDER, path], env=dict(os.environ, **env), capture_output=True,
                         text=True, timeout=170)
    assert res.returncode == 0 and "ok" in res.stdout, (res.stdout[-2000:], res.stderr[-2000:])
    with np.load(path) as z:
        got = [z[k] for k in z.files]
    Ap, Aj, Ax = lssp_amd.poisson(3, 64)
    n = Ap.size - 1
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    assert D.valcodes == 27
    want = products(dev, D, n, n)
    D.close()
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert same(a, b)
