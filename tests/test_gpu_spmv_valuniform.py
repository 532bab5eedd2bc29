"""The value-coded SpMV's uniform waves (k_spmv3's COL_VAL mode): in the fused-dot
instances a wave whose 64 rows of a block carry one code resolves the row's length
once, as a scalar, and adds exactly that many products; every other wave selects
per entry and per lane.  That changes no bit: every comparison here is bitwise,
against the oracle and against the same results under LSSP_AMD_SPMV_UNIFORM=0
(every wave per lane), which one child process computes for all shapes because
the knob is read once.

The five public products carry no fused dot (NRED = 0): they NEVER take the
uniform path -- their instances run the code they ran
before, the knob does not reach them, and what they check here is that this
stayed so.  The uniform waves are reached through solves only,
which need a square matrix:
  * 6 iterations of tree-mode BiCGSTAB + ILU(0), b = 1 (solve6): the NRED = 1 and,
    where the factor is line-swept, NRED = 3 instances;
  * 6 iterations of unpreconditioned tree-mode BiCGSTAB with a right-hand side that
    differs in every row (solve_plain): the NRED = 1 and NRED = 2 instances, with
    partials that differ from block to block and wave to wave, on every square
    shape -- the one with a whole wave of empty rows included, which ILU(0) cannot
    factor.
Every dot of a solve enters its trace, so a partial written to the wrong block,
slot or wave, or a wave of empty rows that contributed anything but +0.0, changes
the trace; v and t themselves are not handed out by the library.  The bands with
n + 2 / n + 7 columns, which keep every row whole, can only be multiplied; each has
a square companion for the solves (a diagonal matrix is the only square one whose
waves are all uniform).

Each shape first counts on the CPU, from Ap / Aj / Ax alone, how many 64-row
waves consist of bit-identical rows, so that a shape which stopped reaching a
path fails instead of passing for nothing.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from test_gpu_spmv_rowcodes import NITS, bits, oracle_products, products, same, solve6, subsets
from test_gpu_spmv_valcodes import ROWVAL_MAX, cbox

pytestmark = pytest.mark.gpu

BOTH, ALL_UNIFORM, NONE_UNIFORM = "both", "all", "none"


def plane_scale(nx, ny, nz, k0):
    return np.where(np.arange(nx * ny * nz) // (nx * ny) >= k0, 2.0, 1.0)


def band(n, vals):
    """n rows of the offsets 0 .. len(vals) - 1 with one value per offset; n + len(vals) - 1 columns,
    so no row loses an entry"""
    nr, nc, Ap, Aj, _ = subsets([(1 << len(vals)) - 1], n=n, noff=len(vals))
    row = np.repeat(np.arange(nr), np.diff(Ap))
    return nr, nc, Ap, Aj, np.asarray(vals, np.float64)[Aj - row]


def band_empty_wave():
    """the 3-entry band with rows 128 .. 191, one whole wave, empty"""
    nr, nc, Ap, Aj, Ax = band(600, (-0.25, 3.0, -0.5))
    row = np.repeat(np.arange(nr), np.diff(Ap))
    keep = (row < 128) | (row >= 192)
    Ap2 = np.zeros(nr + 1, np.int32)
    np.cumsum(np.bincount(row[keep], minlength=nr), out=Ap2[1:])
    return nr, nc, Ap2, Aj[keep], Ax[keep]


def tridiagonal_empty_wave(n=600):
    """square 3-pt matrix with rows 128 .. 191, one whole wave, empty (singular; no ILU(0))"""
    Ap, Aj, Ax = cbox(n, 1, 1)
    row = np.repeat(np.arange(n), np.diff(Ap))
    keep = (row < 128) | (row >= 192)
    Ap2 = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(row[keep], minlength=n), out=Ap2[1:])
    return n, n, Ap2, Aj[keep], Ax[keep]


def band_cycled(n, nvals):
    """the 3-entry band, row i carrying value row i % nvals of nvals distinct ones: no two rows of a
    wave are equal"""
    nr, nc, Ap, Aj, _ = band(n, (0.0, 0.0, 0.0))
    t = (np.arange(nr) % nvals).astype(np.float64)
    return nr, nc, Ap, Aj, np.stack([-0.25 - t / 1024, 3.0 + t / 512, -0.5 - t / 2048], 1).reshape(-1)


def band8_square(n):
    """square: the offsets -3 .. 4 with one value per offset (diagonally dominant), the rows at both
    ends cut; the interior waves are uniform with 8 entries, so the fused-dot instances meet v8 too"""
    vals = np.asarray((-0.9, 0.4, -0.3, 5.5, 0.2, -0.6, 0.7, -0.8))
    r = np.arange(n)
    cols = r[:, None] + np.arange(-3, 5)[None, :]
    ok = (cols >= 0) & (cols < n)
    Ap = np.zeros(n + 1, np.int32)
    np.cumsum(ok.sum(1), out=Ap[1:])
    return n, n, Ap, cols[ok].astype(np.int32), np.tile(vals, (n, 1))[ok]


def diagonal(n):
    return n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.full(n, 2.5)


def tridiagonal_cycled(n, nvals):
    """square 3-pt matrix whose interior rows cycle through nvals distinct value rows; with the two
    boundary rows nvals + 2 distinct rows"""
    Ap, Aj, _ = cbox(n, 1, 1)
    row = np.repeat(np.arange(n), np.diff(Ap))
    t = (row % nvals).astype(np.float64)
    Ax = np.where(Aj == row, 3.0 + t / 512, np.where(Aj < row, -0.25 - t / 1024, -0.5 - t / 2048))
    return n, n, Ap, Aj, Ax


def square(Ap, Aj, Ax):
    return Ap.size - 1, Ap.size - 1, Ap, Aj, Ax


# name -> (builder of (nr, nc, Ap, Aj, Ax), which kinds of wave must occur)
SHAPES = {
    # lines long enough for interior waves; 5 blocks: the second workgroup has one live block; the last wave
    # runs past nrows
    "7pt_130x3x3": (lambda: square(*cbox(130, 3, 3)), BOTH),
    # no plane-interior rows: uniform waves with four different codes in one workgroup
    "7pt_200x2x2": (lambda: square(*cbox(200, 2, 2)), BOTH),
    # 5-pt, the last wave partial.  Lines of 70 rows hold no uniform wave (a wave would have to start at
    # i = 1 .. 5 of a line, and 64 w mod 70 never does below 350 rows), so this one is all mixed waves ...
    "5pt_70x5": (lambda: square(*cbox(70, 5, 1)), NONE_UNIFORM),
    # ... and lines of 130 give what it was meant for: waves 1 and 3 of block 0 uniform, 0 and 2 mixed
    "5pt_130x3": (lambda: square(*cbox(130, 3, 1)), BOTH),
    # the scale changes at plane k = 1.  With three planes every plane has patterns of its own, so the two
    # scales never meet in one pattern ...
    "7pt_130x3x3_piecewise": (lambda: square(*cbox(130, 3, 3, scale=plane_scale(130, 3, 3, 1))), BOTH),
    # ... with four, planes 1 and 2 share theirs: uniform waves of one pattern and different values
    "7pt_130x3x4_piecewise": (lambda: square(*cbox(130, 3, 4, scale=plane_scale(130, 3, 4, 2))), BOTH),
    # uniform waves under v8 (the last, partial wave is the other kind)
    "band8_600": (lambda: band(600, (-0.9, 0.4, -0.3, 5.5, 0.2, -0.6, 0.7, -0.8)), BOTH),
    "band8_600_square": (lambda: band8_square(600), BOTH),
    # a uniform wave of empty rows: in the plain products (which never take the uniform path) ...
    "band3_600_empty_wave": (band_empty_wave, BOTH),
    # ... and, square, in the fused-dot instances of the unpreconditioned solve
    "3pt_600_empty_wave_square": (tridiagonal_empty_wave, BOTH),
    # 17 whole waves of one row: chunk reductions when no lane takes the general path
    "band3_1088_one_row": (lambda: band(1088, (-0.25, 3.0, -0.5)), ALL_UNIFORM),
    "diagonal_1088": (lambda: diagonal(1088), ALL_UNIFORM),
    # no two rows of a wave equal: the general path alone
    "band3_1088_cycled": (lambda: band_cycled(1088, ROWVAL_MAX), NONE_UNIFORM),
    "3pt_1088_cycled": (lambda: tridiagonal_cycled(1088, ROWVAL_MAX - 2), NONE_UNIFORM),
}


def wave_kinds(Ap, Aj, Ax):
    """(waves of 64 bit-identical rows, other waves) -- from the CSR arrays alone"""
    n = Ap.size - 1
    cnt = np.diff(Ap)
    assert cnt.max() <= 8
    row = np.repeat(np.arange(n), cnt)
    pos = np.arange(Aj.size) - Ap[row]
    sig = np.zeros((n, 17), np.int64)
    sig[:, 0] = cnt
    sig[row, 1 + pos] = Aj - row
    sig[row, 9 + pos] = bits(Ax)
    nw = -(-n // 64)
    uniform = sum(1 for w in range(nw) if 64 * w + 64 <= n and (sig[64 * w:64 * w + 64] == sig[64 * w]).all())
    return uniform, nw - uniform


NO_ILU = {"3pt_600_empty_wave_square"}  # empty rows: no pivot


def rhs(n):
    """a right-hand side that differs in every row"""
    return np.random.default_rng(5).uniform(0.5, 1.5, n)


def solve_plain(dev, D, n):
    """unpreconditioned BiCGSTAB, NITS iterations, tree mode, b = rhs(n)"""
    import lssp_amd
    xs, b = dev.vec(n, np.zeros(n)), dev.vec(n, rhs(n))
    r = lssp_amd.solve(dev, D, None, xs, b, solver=lssp_amd.BICGSTAB, tol_rel=0.0, tol_abs=0.0, tol_rb=0.0,
                       maxit=NITS, trace_cap=200)
    return [np.array([float(r.nits)]), np.asarray(r.trace, np.float64), xs.download()]


def compute(dev):
    """name -> [value-row count, the five products; square: solve_plain's three; factorable: solve6's three]"""
    import lssp_amd
    res = {}
    for name, (build, _) in SHAPES.items():
        nr, nc, Ap, Aj, Ax = build()
        D = lssp_amd.DMat(dev, Ap, Aj, Ax, ncols=nc)
        res[name] = [np.array([float(D.valcodes)])] + products(dev, D, nr, nc)
        if nr == nc:
            res[name] += solve_plain(dev, D, nr)
            if name not in NO_ILU:
                res[name] += solve6(dev, D, Ap, Aj, Ax)
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
import test_gpu_spmv_valuniform as T
dev = lssp_amd.Device(0, reduction=lssp_amd.TREE)
res = T.compute(dev)
np.savez(sys.argv[1], **{f"{k}/{i}": a for k, v in res.items() for i, a in enumerate(v)})
print("ok")
'''.replace("ROOT", ROOT)


@pytest.fixture(scope="module")
def general_mode(tmp_path_factory):
    """compute() in a child process all of whose waves take the per-lane path"""
    path = str(tmp_path_factory.mktemp("valuniform") / "general_mode.npz")
    res = subprocess.run([sys.executable, "-c", CHILD, path], env=dict(os.environ, LSSP_AMD_SPMV_UNIFORM="0"),
                         capture_output=True, text=True, timeout=170)
    assert res.returncode == 0 and "ok" in res.stdout, (res.stdout[-2000:], res.stderr[-2000:])
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(SHAPES))
def test_bitwise_vs_oracle_and_general_mode(coded, general_mode, name):
    build, kinds = SHAPES[name]
    nr, nc, Ap, Aj, Ax = build()
    uniform, other = wave_kinds(Ap, Aj, Ax)
    if kinds == BOTH:
        assert uniform > 0 and other > 0, (uniform, other)
    elif kinds == ALL_UNIFORM:
        assert uniform > 0 and other == 0, (uniform, other)
    else:
        assert uniform == 0 and other > 0, (uniform, other)
    got = coded[name]
    assert 0 < int(got[0][0]) <= ROWVAL_MAX  # value-coded: the product is COL_VAL's
    for q, (a, o) in enumerate(zip(got[1:6], oracle_products(Ap, Aj, Ax, nr, nc))):
        assert same(a, o), (name, "product", q)
    assert len(got) == (6 if nr != nc else 9 if name in NO_ILU else 12)
    if nr == nc:
        A = O.CSR(nr, Ap, Aj, Ax)
        o = O.solve(O.BICGSTAB, A, rhs(nr), rtol=0.0, atol=0.0, rbtol=0.0, maxit=NITS, mode=O.TREE, trace_cap=200)
        assert int(got[6][0]) == o.nits and o.trace.size > 2
        assert same(got[7], o.trace) and same(got[8], o.x)
    if nr == nc and name not in NO_ILU:
        L, U = O.ilu(A, "iluk", level=0)
        o = O.solve(O.BICGSTAB, A, np.ones(nr), L=L, U=U, rtol=0.0, atol=0.0, rbtol=0.0, maxit=NITS, mode=O.TREE,
                    trace_cap=200)
        assert int(got[9][0]) == o.nits
        assert same(got[10], o.trace) and same(got[11], o.x)
    assert len(got) == len([k for k in general_mode if k.startswith(name + "/")])
    for i, a in enumerate(got):
        assert same(a, general_mode[f"{name}/{i}"]), (name, i)


def test_shape_properties():
    """what the shape list promises about each matrix"""
    nr, _, Ap, Aj, Ax = SHAPES["7pt_130x3x3"][0]()
    assert nr == 1170 and -(-nr // 256) == 5 and nr % 64 != 0
    assert SHAPES["7pt_200x2x2"][0]()[0] == 800 and SHAPES["5pt_70x5"][0]()[0] == 350
    # four different uniform rows in the first workgroup's 1024 rows of 200 x 2 x 2
    nr, _, Ap, Aj, Ax = SHAPES["7pt_200x2x2"][0]()
    first = {tuple(Aj[Ap[r]:Ap[r + 1]] - r) for w in range(nr // 64) for r in [64 * w]
             if len({tuple(Aj[Ap[q]:Ap[q + 1]] - q) for q in range(64 * w, 64 * w + 64)}) == 1}
    assert len(first) == 4
    # the piecewise case: two uniform waves with one pattern and different values
    nr, _, Ap, Aj, Ax = SHAPES["7pt_130x3x4_piecewise"][0]()
    sigs = {}
    for w in range(nr // 64):
        rows = range(64 * w, 64 * w + 64)
        pats = {tuple(Aj[Ap[r]:Ap[r + 1]] - r) for r in rows}
        vals = {tuple(bits(Ax[Ap[r]:Ap[r + 1]])) for r in rows}
        if len(pats) == 1 and len(vals) == 1:
            sigs.setdefault(next(iter(pats)), set()).add(next(iter(vals)))
    assert any(len(v) > 1 for v in sigs.values())
    # 5-pt: a uniform wave next to a mixed one in block 0, and a partial last wave
    nr, _, Ap, Aj, Ax = SHAPES["5pt_130x3"][0]()
    kinds = [len({tuple(Aj[Ap[q]:Ap[q + 1]] - q) for q in range(64 * w, 64 * w + 64)}) == 1 for w in range(4)]
    assert kinds == [False, True, False, True] and nr % 64 != 0 and np.diff(Ap).max() == 5
    nr, nc, Ap, Aj, Ax = SHAPES["band8_600"][0]()
    assert (np.diff(Ap) == 8).all() and nc == nr + 7
    nr, nc, Ap, Aj, Ax = SHAPES["band3_600_empty_wave"][0]()
    assert (np.diff(Ap)[128:192] == 0).all() and (np.diff(Ap)[:128] == 3).all() and (np.diff(Ap)[192:] == 3).all()
    nr, nc, Ap, Aj, Ax = SHAPES["3pt_600_empty_wave_square"][0]()
    assert nr == nc and (np.diff(Ap)[128:192] == 0).all() and (np.diff(Ap)[192:599] == 3).all()
    nr, nc, Ap, Aj, Ax = SHAPES["band3_1088_one_row"][0]()
    assert nr == 1088 and nc == nr + 2 and nr % 64 == 0
    nr, nc, Ap, Aj, Ax = SHAPES["band3_1088_cycled"][0]()
    assert np.unique(Ax.reshape(nr, 3), axis=0).shape[0] == ROWVAL_MAX


@pytest.mark.parametrize("name", ["band3_600_empty_wave", "3pt_600_empty_wave_square"])
def test_empty_wave_outputs_are_positive_zero(coded, name):
    """y = A x of the wave of empty rows: +0.0, the sign bit included (the plain product: per lane)"""
    z = coded[name][1]
    assert np.array_equal(bits(z[128:192]), np.zeros(64, np.int64))
    assert np.all(z[:128] != 0.0) and np.all(z[192:] != 0.0)


def test_empty_wave_in_the_solve(coded):
    """the fused-dot instances on the wave of empty rows: the run goes its NITS iterations with finite,
    non-zero dots (so the products v = A p and t = A s were formed and summed), and since v and t are +0.0
    there, x moves by alpha p + omega s and r stays b in those rows: r = b - A x with A's rows empty"""
    name = "3pt_600_empty_wave_square"
    nr, nc, Ap, Aj, Ax = SHAPES[name][0]()
    got = coded[name]
    assert int(got[6][0]) == NITS and np.all(np.isfinite(got[7])) and np.all(np.isfinite(got[8]))
    assert np.all(got[8][128:192] != 0.0)
    # (bitwise against the oracle and the knob-off child: test_bitwise_vs_oracle_and_general_mode)
