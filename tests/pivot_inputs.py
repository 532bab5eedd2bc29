"""Value sets that take the value-dependent branches of the ILUK numeric
factorization (k_ilu0_level, ilu_factor.hip; ilu0_factor, ilu_setup.cpp;
pc-iluk.cxx:367-375 and :394-399), on the patterns of test_gpu_iluk_refactor.py:

  row-0 rule     first row of the matrix and of every block-Jacobi block: |d| < 1e-10
                 puts +-1e-3 (d's sign) into the reciprocal only, the stored pivot stays
  interior rule  any other row: |pivot| < 1e-10 stores +1e-3 (the sign is lost)
  unit pivots    every pivot exactly 1.0 (the sweeps may then skip their D slot)

Each set asserts through the oracle that its branch is taken, so a construction
that silently misses it fails where it is built, not as a test that passes for
the wrong reason.  Pure numpy + the CPU oracle; no GPU.
"""
import numpy as np

import oracle as O
import test_gpu_iluk_refactor as R  # _pattern, _values, _expected (its tests are not collected from here)
from inputs import uniform

TOL, REPL = 1e-10, 1e-3  # pc.cxx:6-7
BELOW = float(np.nextafter(TOL, 0.0))

# (pattern, level) pairs the CPU comparison with the reference runs on
CASES = [((9, 21, 13), 0), ((9, 21, 13), 1), ("holed", 1), ("holed", 2), ("rand6", 0), ("grid5", 2), ("box786", 4)]


def case_id(name, level):
    return f"{name if isinstance(name, str) else 'x'.join(map(str, name))}-l{level}"


def _rows(Ap):
    return np.repeat(np.arange(Ap.size - 1), np.diff(Ap))


def _diag_pos(Ap, Aj):
    """position of every row's diagonal (all patterns used here hold one per row)"""
    d = np.flatnonzero(Aj == _rows(Ap))
    assert d.size == Ap.size - 1
    return d


def _factor(Ap, Aj, Ax, level, blk=0):
    return O.ilu(O.CSR(Ap.size - 1, Ap, Aj, Ax), "iluk", level=level, blk=blk)


def pivots(U):
    """the stored pivots: U keeps row i's first"""
    return U.Ax[U.Ap[:-1]]


def _finite(L, U):
    return bool(np.isfinite(L.Ax).all() and np.isfinite(U.Ax).all())


def _multiplier_of_row0(Ap, Aj, Ax, L, first, recip):
    """the first row below `first` that holds column `first`: its multiplier is a * recip"""
    for r in range(first + 1, min(first + 40, Ap.size - 1)):
        if Aj[Ap[r]] == first:
            assert L.Aj[L.Ap[r]] == first and L.Ax[L.Ap[r]] == Ax[Ap[r]] * recip
            return
    # (no such row nearby: the stored pivot alone witnesses the rule)


_SETS = {}


def _cached(fn):
    def get(name, level):
        key = (fn.__name__, name, level)
        if key not in _SETS:
            a = fn(name, level)
            a.setflags(write=False)
            _SETS[key] = a
        return _SETS[key]
    get.__name__ = fn.__name__
    get.__doc__ = fn.__doc__
    return get


@_cached
def benign(name, level):
    """value set 0 of test_gpu_iluk_refactor.py: diagonals in [7, 8), off-diagonals in [-1, -0.1)"""
    return R._values(*R._pattern(name), 0)


@_cached
def cancel3(name, level):
    """value set 1 with the diagonals of rows n//3, n//2, n-1 moved so that the level's
    elimination leaves pivots 0 (to rounding), -2^-40 and +2^-40 there: the interior rule
    stores exactly +1e-3 at all three, whatever the sign"""
    Ap, Aj = R._pattern(name)
    n = Ap.size - 1
    Ax = R._values(Ap, Aj, 1)
    dpos = _diag_pos(Ap, Aj)
    rows = (n // 3, n // 2, n - 1)
    for r, delta in zip(rows, (0.0, -2.0 ** -40, 2.0 ** -40)):  # ascending: a later row sees the earlier replacements
        _, U = _factor(Ap, Aj, Ax, level)
        Ax[dpos[r]] -= U.Ax[U.Ap[r]] - delta
    L, U = _factor(Ap, Aj, Ax, level)
    piv = pivots(U)
    assert all(piv[r] == REPL for r in rows) and np.count_nonzero(piv == REPL) == 3
    assert _finite(L, U)
    return Ax


@_cached
def row0_neg(name, level):
    """value set 1 with A[0,0] = -1e-12: the stored pivot stays, its reciprocal is 1 / -1e-3"""
    Ap, Aj = R._pattern(name)
    Ax = R._values(Ap, Aj, 1)
    assert Aj[0] == 0
    Ax[0] = -1e-12
    L, U = _factor(Ap, Aj, Ax, level)
    assert U.Ax[0] == -1e-12 and _finite(L, U)
    _multiplier_of_row0(Ap, Aj, Ax, L, 0, 1.0 / -REPL)
    return Ax


@_cached
def unit(name, level):
    """diagonals 1.0, every strict-lower value 0.0, upper values of set 1: every multiplier is
    0, every pivot stays exactly 1.0 and the fill stays 0"""
    Ap, Aj = R._pattern(name)
    Ax = R._values(Ap, Aj, 1)
    rows = _rows(Ap)
    Ax[Aj < rows] = 0.0
    Ax[Aj == rows] = 1.0
    L, U = _factor(Ap, Aj, Ax, level)
    assert np.all(pivots(U) == 1.0)
    strict = np.ones(L.Ax.size, bool)
    strict[L.Ap[1:] - 1] = False  # L keeps its unit diagonal last
    assert np.all(L.Ax[strict] == 0.0) and np.all(L.Ax[~strict] == 1.0)
    return Ax


SETS = {f.__name__: f for f in (benign, cancel3, row0_neg, unit)}
SPECIAL = ("cancel3", "row0_neg", "unit")


def expected(which, name, level):
    """test_gpu_iluk_refactor._expected for a set: the oracle's factors, four applies, both sweeps"""
    if which == "benign":
        return R._expected(name, level, 0)
    return R._expected(name, level, None, SETS[which](name, level), tag=which)


THRESHOLD_PIVOTS = [-1e-12, 2.0, 2.0, TOL, REPL, REPL, -TOL, 2.0]


def thresholds():
    """a 300-row diagonal matrix: row 0 = -1e-12 (row-0 rule), interior pivots exactly at the
    tolerance (kept, either sign: the test is <, not <=) and one ulp inside it (replaced by
    +1e-3, either sign)"""
    key = "thresholds"
    if key not in _SETS:
        n = 300
        Ap, Aj = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
        Ax = 2.0 + uniform(9, n)
        Ax[:8] = [-1e-12, 2.0, 2.0, TOL, BELOW, -BELOW, -TOL, 2.0]
        L, U = _factor(Ap, Aj, Ax, 0)
        assert BELOW < TOL and np.array_equal(pivots(U)[:8], THRESHOLD_PIVOTS)
        assert np.array_equal(pivots(U)[8:], Ax[8:]) and np.count_nonzero(pivots(U) == REPL) == 2
        assert O.ilu_apply(L, U, np.ones(n))[0] == -1e12
        for a in (Ap, Aj, Ax):
            a.setflags(write=False)
        _SETS[key] = (Ap, Aj, Ax)
    return _SETS[key]


BLOCK_BOX = (9, 21, 13)


def block_rows(blk):
    """value set 1 on the 9 x 21 x 13 box for block-Jacobi blocks of blk rows: the first row of
    the second block holds -1e-12, of the third +1e-12.  Both stored pivots stay and the
    multipliers below them use 1 / -1e-3 and 1 / 1e-3 (the row-0 rule per block)"""
    key = ("block_rows", blk)
    if key not in _SETS:
        Ap, Aj = R._pattern(BLOCK_BOX)
        n = Ap.size - 1
        assert 2 * blk < n
        Ax = R._values(Ap, Aj, 1)
        dpos = _diag_pos(Ap, Aj)
        Ax[dpos[blk]], Ax[dpos[2 * blk]] = -1e-12, 1e-12
        L, U = _factor(Ap, Aj, Ax, 0, blk=blk)
        piv = pivots(U)
        assert piv[blk] == -1e-12 and piv[2 * blk] == 1e-12 and _finite(L, U)
        assert not np.any(piv == REPL)
        for first, recip in ((blk, 1.0 / -REPL), (2 * blk, 1.0 / REPL)):
            r = first + 1  # row first + 1 of a box holds column first (nx > 1, first + 1 not on a line start)
            at = Ap[r] + int(np.searchsorted(Aj[Ap[r]:Ap[r + 1]], first))
            assert Aj[at] == first
            lat = L.Ap[r] + int(np.flatnonzero(L.Aj[L.Ap[r]:L.Ap[r + 1]] == first)[0])
            assert L.Ax[lat] == Ax[at] * recip and abs(L.Ax[lat]) > 100.0
        Ax.setflags(write=False)
        _SETS[key] = (Ap, Aj, Ax)
    return _SETS[key]
