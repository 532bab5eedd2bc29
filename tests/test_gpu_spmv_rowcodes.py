"""The SpMV's row coding (lssp_amd_mat::Ac, k_spmv3's COL_ROW mode): one pattern
byte per row instead of the row pointer and a byte per entry.  The coding
changes which bytes the product reads, never a value: every comparison here is
bitwise, against the oracle and against the same product under
LSSP_AMD_SPMV_ROWCODE=0 (the offset-id mode), which a child process computes
because the knob is read once.

The grids are boxes (lssp_amd.poisson / oracle.poisson build cubes only): the
7-pt / 5-pt / 3-pt stencil in natural order with random, diagonally dominant
values, so that a misplaced entry changes the sum.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

# name -> (nx, ny, nz), patterns: one partial block; two blocks, the last
# partial; four full blocks; 2-D with a partial last block; 1-D
GRIDS = {"7pt_5x4x3": ((5, 4, 3), 27), "7pt_9x8x7": ((9, 8, 7), 27), "7pt_16x16x4": ((16, 16, 4), 27),
         "5pt_33x31": ((33, 31, 1), 9), "3pt_700": ((700, 1, 1), 3)}
NITS = 6


def box(nx, ny, nz, seed):
    """the stencil of an nx x ny x nz box (i fastest); dimensions of 1 drop their offsets"""
    n = nx * ny * nz
    r = np.arange(n)
    i, j, k = r % nx, r // nx % ny, r // (nx * ny)
    cand = [(r - nx * ny, k > 0), (r - nx, j > 0), (r - 1, i > 0), (r, np.ones(n, bool)), (r + 1, i < nx - 1),
            (r + nx, j < ny - 1), (r + nx * ny, k < nz - 1)]
    cols = np.stack([c for c, _ in cand], 1)
    ok = np.stack([m for _, m in cand], 1)
    rng = np.random.default_rng(seed)
    vals = rng.uniform(-1, -0.1, cols.shape)
    vals[:, 3] = 7.0 + rng.uniform(0, 1, n)
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum(ok.sum(1), out=Ap[1:])
    return Ap, cols[ok].astype(np.int32), vals[ok]


def grid(name):
    dims, _ = GRIDS[name]
    return box(*dims, seed=sum(dims))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    """bitwise, NaNs (a solve driven past convergence) matching NaNs"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


def vectors(nr, nc, seed=77):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nr)


def products(dev, M, nr, nc):
    """every public product: mxy, amxy, amxpby, amxpbyz, amxpbyz with z aliasing y"""
    xh, yh = vectors(nr, nc)
    x = dev.vec(nc, xh)
    out = []
    z = dev.vec(nr, yh)
    M.mv_mxy(x, z)
    out.append(z.download())
    z = dev.vec(nr, yh)
    M.mv_amxy(-2.5, x, z)
    out.append(z.download())
    z = dev.vec(nr, yh)
    M.mv_amxpby(1.25, x, -0.75, z)
    out.append(z.download())
    y, z = dev.vec(nr, yh), dev.vec(nr, np.zeros(nr))
    M.mv_amxpbyz(-0.375, x, 1.5, y, z)
    out.append(z.download())
    y = dev.vec(nr, yh)
    M.mv_amxpbyz(0.75, x, -1.25, y, y)
    out.append(y.download())
    return out


def oracle_products(Ap, Aj, Ax, nr, nc):
    A = O.CSR(nr, Ap, Aj, Ax)
    xh, yh = vectors(nr, nc)
    return [O.spmv(0, A, xh), O.spmv(1, A, xh, -2.5), O.spmv(2, A, xh, 1.25, -0.75, z=yh.copy()),
            O.spmv(3, A, xh, -0.375, 1.5, yh), O.spmv(3, A, xh, 0.75, -1.25, yh)]


def solve6(dev, D, Ap, Aj, Ax):
    """BiCGSTAB + ILU(0), NITS iterations, tree mode: the fused-dot products"""
    import lssp_amd
    n = Ap.size - 1
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0)
    xs, b = dev.vec(n, np.zeros(n)), dev.vec(n, np.ones(n))
    r = lssp_amd.solve(dev, D, M, xs, b, solver=lssp_amd.BICGSTAB, tol_rel=0.0, tol_abs=0.0, tol_rb=0.0,
                       maxit=NITS, trace_cap=200)
    out = [np.array([float(r.nits)]), np.asarray(r.trace, np.float64), xs.download()]
    M.close()
    return out


def compute(dev):
    """name -> [pattern count, the products, the solve] of every grid"""
    import lssp_amd
    res = {}
    for name in GRIDS:
        Ap, Aj, Ax = grid(name)
        n = Ap.size - 1
        D = lssp_amd.DMat(dev, Ap, Aj, Ax)
        res[name] = [np.array([float(D.rowcodes)])] + products(dev, D, n, n) + solve6(dev, D, Ap, Aj, Ax)
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
import test_gpu_spmv_rowcodes as T
dev = lssp_amd.Device(0, reduction=lssp_amd.TREE)
res = T.compute(dev)
np.savez(sys.argv[1], **{f"{k}/{i}": a for k, v in res.items() for i, a in enumerate(v)})
print("ok")
'''.replace("ROOT", ROOT)


@pytest.fixture(scope="module")
def id_mode(tmp_path_factory):
    """compute() in a child process whose products read the offset ids"""
    path = str(tmp_path_factory.mktemp("rowcode") / "id_mode.npz")
    res = subprocess.run([sys.executable, "-c", CHILD, path], env=dict(os.environ, LSSP_AMD_SPMV_ROWCODE="0"),
                         capture_output=True, text=True, timeout=170)
    assert res.returncode == 0 and "ok" in res.stdout, (res.stdout[-2000:], res.stderr[-2000:])
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(GRIDS))
def test_grid_bitwise_vs_oracle_and_id_mode(coded, id_mode, name):
    Ap, Aj, Ax = grid(name)
    n = Ap.size - 1
    got = coded[name]
    assert int(got[0][0]) == GRIDS[name][1]
    for q, (a, o) in enumerate(zip(got[1:6], oracle_products(Ap, Aj, Ax, n, n))):
        assert same(a, o), (name, "product", q)
    A = O.CSR(n, Ap, Aj, Ax)
    L, U = O.ilu(A, "iluk", level=0)
    o = O.solve(O.BICGSTAB, A, np.ones(n), L=L, U=U, rtol=0.0, atol=0.0, rbtol=0.0, maxit=NITS, mode=O.TREE,
                trace_cap=200)
    assert int(got[6][0]) == o.nits  # (NITS, unless the oracle too breaks down earlier)
    assert same(got[7], o.trace) and same(got[8], o.x)
    # the id mode knows the same patterns (the codes are built, not used) and computes the same bits
    for i, a in enumerate(got):
        assert same(a, id_mode[f"{name}/{i}"]), (name, i)


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
    assert D.rowcodes > 0 and D.ndiag == 7
    for q, (a, o) in enumerate(zip(products(dev, D, n, n), oracle_products(Ap2, Aj2, Ax2, n, n))):
        assert same(a, o), q
    D.close()


def subsets(masks, n=600, noff=9, seed=3):
    """row i takes the offsets 0 .. noff - 1 whose bit is set in masks[i % len(masks)]; n + noff - 1
    columns, so no row loses an entry at the boundary"""
    rows = [[i + o for o in range(noff) if masks[i % len(masks)] >> o & 1] for i in range(n)]
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=Ap[1:])
    Aj = np.asarray([c for r in rows for c in r], np.int32)
    return n, n + noff - 1, Ap, Aj, np.random.default_rng(seed).uniform(-1, 1, Aj.size)


# masks 1 .. P are P distinct non-empty subsets of the 9 offsets, none of them all 9
# (511), and together they use every offset (256 = offset 8 alone)
@pytest.mark.parametrize("which", ["max_patterns", "one_more", "nine_entries"])
def test_eligibility_edges(dev, which):
    import lssp_amd
    masks = {"max_patterns": list(range(1, 257)), "one_more": list(range(1, 258)),
             "nine_entries": list(range(1, 257))}[which]
    if which == "nine_entries":
        masks[44] = 511
    nr, nc, Ap, Aj, Ax = subsets(masks)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax, ncols=nc)
    assert D.ndiag == 9  # the layer below a refusal is intact
    assert D.rowcodes == (256 if which == "max_patterns" else 0)
    if D.rowcodes == 0:
        assert D.valcodes == 0
    for q, (a, o) in enumerate(zip(products(dev, D, nr, nc), oracle_products(Ap, Aj, Ax, nr, nc))):
        assert same(a, o), q
    D.close()


def band(noff, n=600):
    """n rows whose entries use exactly noff distinct offsets, three per row (the band of
    test_gpu_assemble.py)"""
    lo = -(noff // 2)
    rows = [[i + o for o in sorted({lo + (3 * i + t) % noff for t in range(3)}) if 0 <= i + o < n] for i in range(n)]
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=Ap[1:])
    Aj = np.asarray([c for r in rows for c in r], np.int32)
    assert np.unique(Aj - np.repeat(np.arange(n), np.diff(Ap))).size == noff
    return n, Ap, Aj, np.random.default_rng(1).uniform(-1, 1, Aj.size)


def test_255_offsets(dev):
    """255 distinct offsets: ids up to 254 in the pattern keys, whichever mode the pattern
    count gives the matrix"""
    import lssp_amd
    n, Ap, Aj, Ax = band(255)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    assert D.ndiag == 255 and 0 <= D.rowcodes <= 256
    for q, (a, o) in enumerate(zip(products(dev, D, n, n), oracle_products(Ap, Aj, Ax, n, n))):
        assert same(a, o), q
    D.close()


def test_256_offsets(dev):
    """a 256th distinct offset, the offset layer's refusal: no ids, so neither row nor value
    codes, and the products of the plain CSR"""
    import lssp_amd
    n, Ap, Aj, Ax = band(256)
    D = lssp_amd.DMat(dev, Ap, Aj, Ax)
    assert (D.ndiag, D.rowcodes, D.valcodes) == (0, 0, 0)
    for q, (a, o) in enumerate(zip(products(dev, D, n, n), oracle_products(Ap, Aj, Ax, n, n))):
        assert same(a, o), q
    D.close()


def test_construction_paths(dev):
    import lssp_amd
    Ap, Aj, Ax = grid("7pt_9x8x7")
    n = Ap.size - 1
    up = lssp_amd.DMat(dev, Ap, Aj, Ax)
    dAp, dAj, dAx = dev.idx(Ap.size, Ap), dev.idx(Aj.size, Aj), dev.vec(Ax.size, Ax)
    fd = lssp_amd.DMat.from_device(dev, n, n, Aj.size, dAp, dAj, dAx)
    assert (fd.rowcodes, fd.ndiag, fd.device_bytes) == (up.rowcodes, up.ndiag, up.device_bytes)
    assert fd.rowcodes == 27
    for a, b in zip(products(dev, fd, n, n), products(dev, up, n, n)):
        assert same(a, b)
    Ax2 = np.random.default_rng(9).uniform(-1, 1, Ax.size)
    for D in (fd, up):
        D.update_values(dev.vec(Ax2.size, Ax2))
        assert D.rowcodes == 27
        for q, (a, o) in enumerate(zip(products(dev, D, n, n), oracle_products(Ap, Aj, Ax2, n, n))):
            assert same(a, o), q
    fd.close()
    up.close()


ORDER = r'''
import sys, numpy as np
sys.path.insert(0, "ROOT"); sys.path.insert(0, "ROOT/tests")
import lssp_amd
import test_gpu_spmv_rowcodes as T
dev = lssp_amd.Device(0, reduction=lssp_amd.TREE)
Ap, Aj, Ax = lssp_amd.poisson(3, 64)
n = Ap.size - 1
D = lssp_amd.DMat(dev, Ap, Aj, Ax)
assert D.rowcodes == 27
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
    want = products(dev, D, n, n)
    D.close()
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert same(a, b)
