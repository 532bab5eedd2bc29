"""Triangular factors of the device schedule builder's tests (tools/sched_dev_check.cpp on the CPU,
lssp_amd_ilu_from_factors_dev on the GPU), and readers of a schedule's streams.

A factor pair is ((Lp, Lj, Lx), (Up, Uj, Ux)): L with its diagonal last in each row, U with its pivot
first.  Strict values are small, so every sweep stays finite."""
import numpy as np

import oracle as O

BP_RING = 4096  # lssp_amd/csrc/sched_dev.h
ROWS = 256
REC_SLOT_WORDS = 4096  # the LDS record slot of EP >= 16 records, in 4-byte words
# the header fields of lssp_amd_ilu_get_schedule, in order
HDR = ("B", "nb", "nsteps", "npackets", "EP", "EXT", "rows", "rec_words", "idx_words", "unit", "nlevels", "origin")


def _val(i, j):
    return ((i * 7 + j * 13) % 19 - 9) / 64.0 or 0.015625


def lower(n, cols_of, unit=True):
    """cols_of(i) -> ascending strict columns < i"""
    Tp, Tj, Tx = [0], [], []
    for i in range(n):
        cs = list(cols_of(i))
        for j in cs:
            Tj.append(j)
            Tx.append(_val(i, j) / max(len(cs), 1))
        Tj.append(i)
        Tx.append(1.0 if unit else 1.5 + (i % 5) * 0.125)
        Tp.append(len(Tj))
    return np.array(Tp, np.int32), np.array(Tj, np.int32), np.array(Tx, np.float64)


def upper(n, cols_of, unit=False):
    """cols_of(i) -> ascending strict columns > i"""
    Tp, Tj, Tx = [0], [], []
    for i in range(n):
        cs = list(cols_of(i))
        Tj.append(i)
        Tx.append(1.0 if unit else 2.0 + (i % 7) * 0.25)
        for j in cs:
            Tj.append(j)
            Tx.append(_val(i, j) / max(len(cs), 1))
        Tp.append(len(Tj))
    return np.array(Tp, np.int32), np.array(Tj, np.int32), np.array(Tx, np.float64)


def mirror(n, lcols):
    """the U pattern that mirrors an L pattern: row i of U holds n - 1 - j for the L columns j of row n - 1 - i"""
    return lambda i: sorted(n - 1 - j for j in lcols(n - 1 - i))


def _random_cols(n, per_row, seed):
    rng = np.random.default_rng(seed)
    picks = [np.unique(rng.integers(0, max(i, 1), per_row)) if i else np.array([], int) for i in range(n)]
    return lambda i: [int(c) for c in picks[i] if c < i]


def diag_only(n):
    return lower(n, lambda i: []), upper(n, lambda i: [])


def chain(n):
    lc = lambda i: [i - 1] if i else []
    return lower(n, lc), upper(n, mirror(n, lc))


def ilut_p7_16():
    A = O.poisson(3, 16)
    L, U = O.ilu(A, "ilut", tol=1e-4, p=20)
    return (L.Ap, L.Aj, L.Ax), (U.Ap, U.Aj, U.Ax)


def ilu0_p7_8():
    A = O.poisson(3, 8)
    L, U = O.ilu(A, "iluk", level=0)
    return (L.Ap, L.Aj, L.Ax), (U.Ap, U.Aj, U.Ax)


def random_rows(n, per_row, seed):
    lc = _random_cols(n, per_row, seed)
    return lower(n, lc), upper(n, mirror(n, _random_cols(n, per_row, seed + 1)))


def wide_level(n=2000, far=1000):
    """rows >= far hold one entry, far rows back: the bandwidth makes one block of `far` rows a single level"""
    lc = lambda i: [i - far] if i >= far else []
    return lower(n, lc), upper(n, mirror(n, lc))


def rec_slot(n=2000, far=1000, k=17):
    """wide_level with 17 entries per row: EP = 24 records, whose LDS slot holds 64 rows"""
    lc = lambda i: list(range(i - far, i - far + k)) if i >= far else []
    return lower(n, lc), upper(n, mirror(n, lc))


def beyond_ring(n=12000, back=4500, far=6000):
    """every row i >= back reads row i - back; row `far` also reads row 0, so B = far: the i - back operands
    of a block's later rows lie in their own block, more than BP_RING positions before their step's end"""
    lc = lambda i: ([0] if i == far else []) + ([i - back] if i >= back else [])
    return lower(n, lc), upper(n, mirror(n, lc))


def staggered(n=4096, W=1024, d=300):
    """three staggered runs of HBM operands per packet: entries at i - W, i - W + d, i - W + 2 d"""
    lc = lambda i: [j for j in (i - W, i - W + d, i - W + 2 * d) if 0 <= j < i]
    return lower(n, lc), upper(n, mirror(n, lc))


def unrelated(n=700):
    """L a chain, U a random pattern: the U sweep's rhs entries are positions of another schedule"""
    lc = lambda i: [i - 1] if i else []
    return lower(n, lc), upper(n, mirror(n, _random_cols(n, 6, 77)))


# (name, builder): every case runs on the CPU harness (both sides) and on the GPU
CASES = [
    ("n1", lambda: diag_only(1)),
    ("n2", lambda: diag_only(2)),
    ("chain5000", lambda: chain(5000)),
    ("ilut-p7-16", ilut_p7_16),
    ("rand-ep8", lambda: random_rows(600, 6, 5)),
    ("rand-ep16", lambda: random_rows(600, 12, 9)),
    ("wide-level", wide_level),
    ("rec-slot", rec_slot),
    ("beyond-ring", beyond_ring),
    ("staggered-ext3", staggered),
    ("unrelated", unrelated),
]


def row25():
    """a strict row of 25 entries"""
    lc = lambda i: list(range(25)) if i == 30 else []
    return lower(40, lc), upper(40, lambda i: [])


def l_col_not_below():
    (Lp, Lj, Lx), U = chain(50)
    Lj = Lj.copy()
    Lj[Lp[20]] = 20  # the strict entry of row 20 names the row itself
    return (Lp, Lj, Lx), U


def u_col_not_above():
    L, (Up, Uj, Ux) = chain(50)
    Uj = Uj.copy()
    Uj[Up[20] + 1] = 20
    return L, (Up, Uj, Ux)


def no_diag_slot():
    (Lp, Lj, Lx), U = diag_only(50)
    Lp = Lp.copy()
    Lp[21:] -= 1  # row 20 is empty
    return (Lp, Lj[:-1].copy(), Lx[:-1].copy()), U


# (name, builder, status): LSSP_AMD_EINVAL = 1, LSSP_AMD_EUNSUPPORTED = 6
REFUSALS = [
    ("row25", row25, 6),
    ("l-col-not-below", l_col_not_below, 1),
    ("u-col-not-above", u_col_not_above, 1),
    ("no-diag-slot", no_diag_slot, 1),
]


# ---- reading a schedule -------------------------------------------------------------
def levels(T, up):
    Tp, Tj, _ = T
    n = Tp.size - 1
    lev = np.zeros(n, np.int64)
    for i in (range(n - 1, -1, -1) if up else range(n)):
        ks = range(Tp[i] + 1, Tp[i + 1]) if up else range(Tp[i], Tp[i + 1] - 1)
        lev[i] = max((lev[Tj[k]] + 1 for k in ks), default=0)
    return lev


def rec_words(ep, nr):
    p4 = lambda w: (w + 3) & ~3
    return p4(ep // 2 * nr) + 2 * ep * nr + p4(2 * nr) + p4(nr)


def packets(s):
    """per packet of a schedule dict: (block, first position, rows, operands, operand positions)"""
    B, desc, idx, blk = s["B"], s["desc"], s["idx"], s["blk"]
    out = []
    for b in range(s["nb"]):
        for k in range(blk[b], blk[b + 1]):
            ro, io, w, p = (int(v) for v in desc[4 * k:4 * k + 4])
            nr, nx = w & 1023, (w >> 10) & 2047
            assert p // B == b
            out.append((b, p, nr, nx, idx[io + nr:io + nr + nx]))
    return out


def closed_early(s, T, up):
    """the packets closed by a rule and not by the end of their step: (rows, operands) of each"""
    lev, perm = levels(T, up), s["perm"]
    pk = packets(s)
    return [(a[2], a[3]) for a, b in zip(pk, pk[1:]) if a[0] == b[0] and lev[perm[a[1] + a[2] - 1]] == lev[perm[b[1]]]]


def check_case(name, L, U, sl, su):
    """what each case of sched_inputs.CASES is there for, asserted on the schedules (sl, su) themselves"""
    n = L[0].size - 1
    if name in ("n1", "n2"):
        for s in (sl, su):
            assert (s["B"], s["nb"], s["npackets"], s["EP"], s["nlevels"]) == (n, 1, 1, 4, 1)
        assert L[1].size == n and U[1].size == n
    elif name == "chain5000":
        for s in (sl, su):
            assert (s["B"], s["nb"], s["nsteps"], s["npackets"]) == (64, 79, 5000, 5000) and n % 64 == 8
            heads = [p for p in packets(s) if p[1] % 64 == 0 and p[0] > 0]
            assert len(heads) == 78 and all(p[3] == 1 and p[4][0] // 64 == p[0] - 1 for p in heads)
    elif name == "ilut-p7-16":
        assert (sl["EP"], su["EP"], sl["unit"], su["unit"]) == (24, 24, 1, 0)
        # (B = 256, one grid plane: its levels hold at most a few dozen rows, so no packet of this factor
        # reaches the 64 rows of the record slot -- that rule is the next case's)
        assert sl["B"] == 256 and max(p[2] for p in packets(sl) + packets(su)) < 64
    elif name == "rec-slot":
        assert (sl["EP"], su["EP"]) == (24, 24)
        assert rec_words(24, 64) <= REC_SLOT_WORDS < rec_words(24, 65)
        for s, T, up in ((sl, L, False), (su, U, True)):
            early = closed_early(s, T, up)
            assert early and all(nr == 64 and nx <= 2 * ROWS for nr, nx in early)
    elif name == "rand-ep8":
        assert (sl["EP"], su["EP"]) == (8, 8)
    elif name == "rand-ep16":
        assert (sl["EP"], su["EP"]) == (16, 16)
    elif name == "wide-level":
        for s, T, up in ((sl, L, False), (su, U, True)):
            assert any(nr == ROWS for nr, nx in closed_early(s, T, up))
    elif name == "beyond-ring":
        for s in (sl, su):
            assert s["B"] == 6000
            own = [(p, x) for b, p, nr, nx, xs in packets(s) for x in xs if x // 6000 == b]
            assert own and any(p - x > BP_RING for p, x in own)
    elif name == "staggered-ext3":
        # EXT = 3 is kept only when the count at cap 512 exceeds the count at cap 1024 by more than 1 %
        # and the count at cap 768 does not; the harness also writes the three counts out
        assert sl["EXT"] == 3 and any(ROWS * 2 < nx <= ROWS * 3 for b, p, nr, nx, xs in packets(sl))
        if "counts" in sl:
            c2, c3, c4 = sl["counts"]
            assert c2 > c4 + c4 // 100 and c3 <= c4 + c4 // 100
    elif name == "unrelated":
        assert not np.array_equal(sl["pos"], su["pos"])
        b, p, nr, nx, xs = packets(su)[0]
        io = int(su["desc"][1])
        rows = su["perm"][p:p + nr]
        assert np.array_equal(su["idx"][io:io + nr], sl["pos"][rows])
        assert not np.array_equal(su["idx"][io:io + nr], su["pos"][rows])
    else:
        raise AssertionError("a case without its assertion: " + name)
