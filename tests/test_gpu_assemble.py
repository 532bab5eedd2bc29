"""Assembly on the device (lssp_amd_csr_is_sorted / _bcsr_is_sorted /
_csr_sort_columns_dev / _csr_adjust_zero_diag / _csr_get_block_diag and
lssp_amd_mat_from_device) -- bitwise:

  * against the reference's own outputs (tests/golden/assemble.*),
  * against the numpy restatements (tests/assemble_util.py, pinned by those
    fixtures in test_assemble_cpu.py) on a random matrix of 200,000 rows with
    repeated columns, empty rows, 0 / -0.0 / NaN / inf values and rows on both
    sides of the sort's one-thread limit (64 entries),
  * the device column sort against the host one (lssp_amd.sort_columns),
  * a handle from device arrays against lssp_amd_mat_upload of the same arrays:
    layout, bytes, all four products (both handles come from one builder, so
    each is held to the oracle's products as well), a solve,
  * COO in HBM -> CSR -> sorted -> handle -> solve with no host copy of the matrix,
  * malformed inputs return LSSP_AMD_EINVAL instead of faulting.
"""
import numpy as np
import pytest

import assemble_util as U
from conv_util import same
from inputs import conv_rand

pytestmark = pytest.mark.gpu

CASES = U.assemble_cases()


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


def _to_dev(dev, Ap, Aj, Ax):
    return dev.idx(Ap.size, Ap), dev.idx(Aj.size, Aj), dev.vec(Ax.size, Ax)


def run_device(dev, kind, p, i):
    from lssp_amd import convert as C
    if kind == "sort_column":
        dAp, dAj, dAx = _to_dev(dev, i["Ap"], i["Aj"], i["Ax"])
        C.sort_columns(dev, p["nrows"], p["ncols"], i["Aj"].size, dAp, dAj, dAx)
        assert same(dAp.download(), i["Ap"])
        return {"Sj": dAj.download(), "Sx": dAx.download()}
    if kind == "csr_is_sorted":
        v = C.csr_is_sorted(dev, p["nrows"], i["Aj"].size, dev.idx(i["Ap"].size, i["Ap"]),
                            dev.idx(i["Aj"].size, i["Aj"]))
        return {"sorted": np.array([int(v)], np.int32)}
    if kind == "bcsr_is_sorted":
        v = C.bcsr_is_sorted(dev, p["nbrows"], i["Bj"].size, dev.idx(i["Bp"].size, i["Bp"]),
                             dev.idx(i["Bj"].size, i["Bj"]))
        return {"sorted": np.array([int(v)], np.int32)}
    if kind == "adjust_zero_diag":
        m, *out = C.adjust_zero_diag(dev, p["n"], i["Aj"].size, *_to_dev(dev, i["Ap"], i["Aj"], i["Ax"]),
                                     float.fromhex(p["tol"]) if isinstance(p["tol"], str) else p["tol"])
    else:
        m, *out = C.get_block_diag(dev, p["n"], i["Aj"].size, *_to_dev(dev, i["Ap"], i["Aj"], i["Ax"]), p["blk"])
    got = dict(zip(("Mp", "Mj", "Mx"), (a.download() for a in out)))
    assert m == got["Mp"][-1] == got["Mj"].size
    return got


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_bitwise_vs_reference(dev, c):
    got = run_device(dev, c["kind"], c["params"], c["in"])
    for k, v in c["out"].items():
        assert same(got[k], v), k


LONG = {1000: 64, 2000: 65, 3000: 3001, 4000: 500, 150_000: 777}   # row -> length; row 4000 is sorted


@pytest.fixture(scope="module")
def big():
    """200,000 x 200,000: rows of 0..9 random columns (unsorted, repeated, empty rows), some
    longer ones around and far above the sort's one-thread limit, special values"""
    rng = np.random.default_rng(2024)
    n = 200_000
    lens = rng.integers(0, 10, n)
    for r, ln in LONG.items():
        lens[r] = ln
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum(lens, out=Ap[1:])
    Aj = rng.integers(0, n, Ap[-1]).astype(np.int32)
    Aj[Ap[3000]:Ap[3001]] = rng.integers(0, 900, 3001)                   # many duplicates
    Aj[Ap[4000]:Ap[4001]] = np.sort(rng.integers(0, 300, 500))           # sorted with duplicates: untouched
    Ax = rng.uniform(-1, 1, Aj.size)
    idx = rng.choice(Aj.size, Aj.size // 50, replace=False)
    Ax[idx] = np.resize(np.array([0.0, -0.0, np.nan, np.inf]), idx.size)
    return n, Ap, Aj, Ax


def test_sort_and_is_sorted_vs_restatement_and_host_large(dev, big):
    import lssp_amd
    from lssp_amd import convert as C
    n, Ap, Aj, Ax = big
    dAp, dAj, dAx = _to_dev(dev, Ap, Aj, Ax)
    assert U.is_sorted(Ap, Aj) == 0 and C.csr_is_sorted(dev, n, Aj.size, dAp, dAj) is False
    C.sort_columns(dev, n, n, Aj.size, dAp, dAj, dAx)
    gj, gx = dAj.download(), dAx.download()
    wj, wx = U.sort_column(Ap, Aj, Ax)
    assert same(gj, wj) and same(gx, wx)
    _, hj, hx = lssp_amd.sort_columns(Ap, Aj, Ax)                        # the host path on the same input
    assert same(gj, hj) and same(gx, hx)
    assert same(dAp.download(), Ap)
    assert C.csr_is_sorted(dev, n, Aj.size, dAp, dAj) is True
    assert C.bcsr_is_sorted(dev, n, Aj.size, dAp, dAj) is True
    # a single descending pair: in the last short row that can hold one, and inside a long row
    short = [r for r in np.flatnonzero(np.diff(Ap) > 1) if r not in LONG and wj[Ap[r + 1] - 2] > 0][-1]
    for k in (Ap[short + 1] - 1, Ap[3000] + 1500):
        one = wj.copy()
        assert one[k - 1] > 0
        one[k] = one[k - 1] - 1
        assert U.is_sorted(Ap, one) == 0
        assert C.csr_is_sorted(dev, n, Aj.size, dAp, dev.idx(one.size, one)) is False


def test_adjust_zero_diag_vs_restatement_large(dev, big):
    n, Ap, Aj, Ax = big
    got = run_device(dev, "adjust_zero_diag", {"n": n, "tol": 1e-8}, {"Ap": Ap, "Aj": Aj, "Ax": Ax})
    want = U.adjust_zero_diag(n, Ap, Aj, Ax, 1e-8)
    assert all(same(got[k], w) for k, w in zip(("Mp", "Mj", "Mx"), want))
    rows = np.repeat(np.arange(n), np.diff(Ap))
    assert got["Mj"].size == Aj.size + n - np.unique(rows[Aj == rows]).size


@pytest.mark.parametrize("blk", [1, 7, 1000, 200_000, 200_005])
def test_get_block_diag_vs_restatement_large(dev, big, blk):
    n, Ap, Aj, Ax = big
    got = run_device(dev, "get_block_diag", {"n": n, "blk": blk}, {"Ap": Ap, "Aj": Aj, "Ax": Ax})
    want = U.get_block_diag(n, Ap, Aj, Ax, blk)
    assert all(same(got[k], w) for k, w in zip(("Mp", "Mj", "Mx"), want))


# ---- lssp_amd_mat_from_device == lssp_amd_mat_upload --------------------------------

def _banded(n, noff, seed):
    """n rows whose entries use exactly noff distinct offsets col - row, three per row"""
    lo = -(noff // 2)
    rows = [[i + o for o in sorted({lo + (3 * i + t) % noff for t in range(3)}) if 0 <= i + o < n]
            for i in range(n)]
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=Ap[1:])
    Aj = np.asarray([c for r in rows for c in r], np.int32)
    assert np.unique(Aj - np.repeat(np.arange(n), np.diff(Ap))).size == noff
    return n, n, Ap, Aj, np.random.default_rng(seed).uniform(-1, 1, Aj.size)


def _fixed(nr, nc, k, seed):
    rng = np.random.default_rng(seed)
    Ap = np.arange(0, (nr + 1) * k, k, dtype=np.int32)
    return nr, nc, Ap, rng.integers(0, nc, nr * k).astype(np.int32), rng.uniform(-1, 1, nr * k)


def _matrices():
    import lssp_amd
    out = {}
    for name, (dim, N) in {"p5_6": (2, 6), "p7_4": (3, 4)}.items():
        Ap, Aj, Ax = lssp_amd.poisson(dim, N)
        out[name] = ((Ap.size - 1, Ap.size - 1, Ap, Aj, Ax), "coded")
    out["band255"] = (_banded(600, 255, 1), 255)
    out["band256"] = (_banded(600, 256, 2), "not coded")
    out["rnd400x9"] = (_fixed(400, 400, 9, 3), "windowed")
    out["scattered40k"] = (_fixed(40_000, 40_000, 5, 4), "plain")
    out["rect_37x53"] = ((37, 53) + conv_rand(37, 53, 6, 13), None)
    out["one_row"] = ((1, 9) + conv_rand(1, 9, 9, 16), None)
    out["nnz0"] = ((6, 6, np.zeros(7, np.int32), np.zeros(0, np.int32), np.zeros(0)), None)
    return out


def _products(dev, A, nr, nc, seed):
    rng = np.random.default_rng(seed)
    xh, yh = rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nr)
    x = dev.vec(nc, xh)
    out = []
    y = dev.vec(nr, yh)
    A.mv_amxpby(1.25, x, -0.75, y)
    out.append(y.download())
    y, z = dev.vec(nr, yh), dev.vec(nr, np.zeros(nr))
    A.mv_amxpbyz(-0.375, x, 1.5, y, z)
    out.append(z.download())
    y = dev.vec(nr, yh)
    A.mv_amxy(-2.5, x, y)
    out.append(y.download())
    y = dev.vec(nr, yh)
    A.mv_mxy(x, y)
    out.append(y.download())
    return out


def _oracle_products(nr, nc, Ap, Aj, Ax, seed):
    """_products' four products from the oracle, same vectors, same order"""
    import oracle as O
    rng = np.random.default_rng(seed)
    xh, yh = rng.uniform(-1, 1, nc), rng.uniform(-1, 1, nr)
    A = O.CSR(nr, Ap, Aj, Ax)
    return [O.spmv(2, A, xh, 1.25, -0.75, z=yh.copy()), O.spmv(3, A, xh, -0.375, 1.5, yh),
            O.spmv(1, A, xh, -2.5), O.spmv(0, A, xh)]


@pytest.mark.parametrize("name", ["p5_6", "p7_4", "band255", "band256", "rnd400x9", "scattered40k", "rect_37x53",
                                  "one_row", "nnz0"])
def test_from_device_equals_upload(dev, name):
    import lssp_amd
    (nr, nc, Ap, Aj, Ax), expect = _matrices()[name]
    up = lssp_amd.DMat(dev, Ap, Aj, Ax, ncols=nc)
    dAp, dAj, dAx = _to_dev(dev, Ap, Aj, Ax)
    fd = lssp_amd.DMat.from_device(dev, nr, nc, Aj.size, dAp, dAj, dAx)
    # the caller's arrays are unchanged, and the handle does not need them
    assert same(dAp.download(), Ap) and same(dAj.download(), Aj) and same(dAx.download(), Ax)
    for a in (dAp, dAj, dAx):
        a.free()
    assert (fd.nrows, fd.nnz, fd.nhalo, fd.row0) == (up.nrows, up.nnz, up.nhalo, up.row0)
    assert (fd.ndiag, fd.windowed) == (up.ndiag, up.windowed)
    assert fd.device_bytes == up.device_bytes
    if expect == "coded":
        assert fd.ndiag in (5, 7) and not fd.windowed
    elif expect == 255:
        assert fd.ndiag == 255
    elif expect == "not coded":
        assert fd.ndiag == 0
    elif expect == "windowed":
        assert fd.ndiag == 0 and fd.windowed
    elif expect == "plain":
        assert fd.ndiag == 0 and not fd.windowed
    if nr:
        # both handles come from one builder, so each is also held to the oracle's products
        want = _oracle_products(nr, nc, Ap, Aj, Ax, 5)
        for q, (a, b, o) in enumerate(zip(_products(dev, fd, nr, nc, 5), _products(dev, up, nr, nc, 5), want)):
            assert same(a, b), q
            assert same(a, o) and same(b, o), q
    fd.close()
    up.close()


def test_from_device_equals_upload_full_size(dev):
    """BASELINE's matrix (7-pt Poisson 216^3, 70 M entries: more rows than one grid of
    threads): same layout, bytes and product as the uploaded handle"""
    import lssp_amd
    Ap, Aj, Ax = lssp_amd.poisson(3, 216)
    n = Ap.size - 1
    up = lssp_amd.DMat(dev, Ap, Aj, Ax)
    dAp, dAj, dAx = _to_dev(dev, Ap, Aj, Ax)
    fd = lssp_amd.DMat.from_device(dev, n, n, Aj.size, dAp, dAj, dAx)
    for a in (dAp, dAj, dAx):
        a.free()
    assert (fd.ndiag, fd.windowed, fd.device_bytes) == (up.ndiag, up.windowed, up.device_bytes) and fd.ndiag == 7
    xh = np.random.default_rng(216).uniform(-1, 1, n)
    x, yf, yu = dev.vec(n, xh), dev.vec(n, xh), dev.vec(n, xh)
    fd.mv_amxpby(1.25, x, -0.75, yf)
    up.mv_amxpby(1.25, x, -0.75, yu)
    assert same(yf.download(), yu.download())
    for a in (fd, up, x, yf, yu):
        a.close()


def _solve(dev, A, n):
    import lssp_amd
    x, b = dev.vec(n, np.zeros(n)), dev.vec(n, np.ones(n))
    r = lssp_amd.solve(dev, A, None, x, b, solver=lssp_amd.BICGSTAB)
    return r.nits, r.residual, x.download()


def test_solve_on_both_handles_bitwise(dev):
    import lssp_amd
    Ap, Aj, Ax = lssp_amd.poisson(3, 8)
    n = Ap.size - 1
    up = lssp_amd.DMat(dev, Ap, Aj, Ax)
    fd = lssp_amd.DMat.from_device(dev, n, n, Aj.size, *_to_dev(dev, Ap, Aj, Ax))
    a, b = _solve(dev, fd, n), _solve(dev, up, n)
    assert a[0] == b[0] > 0 and a[1] == b[1] and same(a[2], b[2])


def test_coo_to_solve_without_a_host_copy(dev):
    """shuffled COO in HBM -> coo_to_csr -> sort_columns -> from_device -> solve == the solve on
    the uploaded sorted CSR"""
    import lssp_amd
    from lssp_amd import convert as C
    Ap, Aj, Ax = lssp_amd.poisson(3, 8)
    n, nnz = Ap.size - 1, Aj.size
    perm = np.random.default_rng(8).permutation(nnz)
    Ci = np.repeat(np.arange(n, dtype=np.int32), np.diff(Ap))[perm]
    dCi, dCj, dCx = _to_dev(dev, Ci, Aj[perm], Ax[perm])
    dAp, dAj, dAx = C.coo_to_csr(dev, n, nnz, dCi, dCj, dCx)
    assert C.csr_is_sorted(dev, n, nnz, dAp, dAj) is False
    C.sort_columns(dev, n, n, nnz, dAp, dAj, dAx)
    assert C.csr_is_sorted(dev, n, nnz, dAp, dAj) is True
    fd = lssp_amd.DMat.from_device(dev, n, n, nnz, dAp, dAj, dAx)
    for a in (dCi, dCj, dCx, dAp, dAj, dAx):
        a.free()
    up = lssp_amd.DMat(dev, Ap, Aj, Ax)
    assert fd.ndiag == up.ndiag == 7
    a, b = _solve(dev, fd, n), _solve(dev, up, n)
    assert a[0] == b[0] > 0 and a[1] == b[1] and same(a[2], b[2])


def test_malformed_inputs_raise_einval(dev):
    import lssp_amd
    from lssp_amd import convert as C
    Ap, Aj, Ax = conv_rand(100, 100, 5, 77)
    nnz = Aj.size

    def einval(fn, *a):
        with pytest.raises(lssp_amd.LsspError) as e:
            fn(dev, *a)
        assert e.value.status == 1

    def arrays(p=Ap, j=Aj, room=0):          # room: the arrays hold what a too-large nnz claims
        return dev.idx(p.size, p), dev.idx(j.size + room, j), dev.vec(Ax.size + room, Ax)

    bad_ptr = Ap.copy()
    bad_ptr[50] = bad_ptr[51] + 1                 # decreasing row pointers
    bad_col = Aj.copy()
    bad_col[3] = 100                              # a column equal to ncols
    neg_col = Aj.copy()
    neg_col[nnz - 1] = -1                         # a negative column
    for kw in ({"p": bad_ptr}, {"j": bad_col}, {"j": neg_col}):
        einval(lssp_amd.DMat.from_device, 100, 100, nnz, *arrays(**kw))
        einval(C.sort_columns, 100, 100, nnz, *arrays(**kw))
        einval(C.adjust_zero_diag, 100, nnz, *arrays(**kw), 1e-8)
        einval(C.get_block_diag, 100, nnz, *arrays(**kw), 4)
    einval(C.csr_is_sorted, 100, nnz, *arrays(p=bad_ptr)[:2])
    einval(C.bcsr_is_sorted, 100, nnz, *arrays(p=bad_ptr)[:2])
    einval(lssp_amd.DMat.from_device, 100, 100, nnz + 1, *arrays(room=1))      # Ap[nrows] != nnz
    einval(C.csr_is_sorted, 100, nnz + 1, *arrays(room=1)[:2])
    einval(C.sort_columns, 100, 100, nnz + 1, *arrays(room=1))
    einval(C.get_block_diag, 100, nnz, *arrays(), 0)                          # blk = 0
    # the device is still usable: the correct calls pass
    dAp, dAj, dAx = arrays()
    fd = lssp_amd.DMat.from_device(dev, 100, 100, nnz, dAp, dAj, dAx)
    up = lssp_amd.DMat(dev, Ap, Aj, Ax)
    for a, b in zip(_products(dev, fd, 100, 100, 6), _products(dev, up, 100, 100, 6)):
        assert same(a, b)
    C.sort_columns(dev, 100, 100, nnz, dAp, dAj, dAx)
    wj, wx = U.sort_column(Ap, Aj, Ax)
    assert same(dAj.download(), wj) and same(dAx.download(), wx)
    got = run_device(dev, "get_block_diag", {"n": 100, "blk": 4}, {"Ap": Ap, "Aj": Aj, "Ax": Ax})
    assert all(same(got[k], w) for k, w in zip(("Mp", "Mj", "Mx"), U.get_block_diag(100, Ap, Aj, Ax, 4)))
