"""Inputs and a numpy statement of the distributed handle's local numbering, shared by
tests/test_dist_dev_cpu.py and tests/test_gpu_dist_dev.py."""
import numpy as np

from inputs import splitmix64, uniform

CHUNK = 256  # rows per SpMV chunk (the halo-free run is counted in these)


def rank_rows(n: int, world: int, rank: int):
    """the canonical partition: (row0, nlocal) of a rank"""
    blk = (n + world - 1) // world
    r0 = min(rank * blk, n)
    return r0, max(0, min(blk, n - r0))


def local_rows(Ap, Aj, Ax, r0: int, nl: int):
    """rows [r0, r0 + nl) of a global CSR, global columns"""
    e0, e1 = int(Ap[r0]), int(Ap[r0 + nl])
    return (Ap[r0:r0 + nl + 1] - e0).astype(np.int32), Aj[e0:e1].copy(), Ax[e0:e1].copy()


def halo_plan(Ap, Aj, r0: int, nl: int):
    """What the distributed builder derives from a rank's rows: the halo columns (ascending =
    grouped by owner, then ascending), the columns renumbered [owned | halo], the longest run
    [ich0, ich1) of 256-row chunks none of whose rows reads a halo column (the first of equals)
    and the widest |col - row| over the rows of that run."""
    Aj = np.asarray(Aj, np.int64)
    owned = (Aj >= r0) & (Aj < r0 + nl)
    hcols = np.unique(Aj[~owned])
    lj = np.where(owned, Aj - r0, nl + np.searchsorted(hcols, Aj))
    rows = np.repeat(np.arange(nl), np.diff(Ap))
    nch = (nl + CHUNK - 1) // CHUNK
    ch_halo = np.zeros(nch, bool)
    ch_halo[np.unique(rows[~owned] // CHUNK)] = True
    best0 = best1 = run0 = 0
    for ch in range(nch + 1):
        if ch == nch or ch_halo[ch]:
            if ch - run0 > best1 - best0:
                best0, best1 = run0, ch
            run0 = ch + 1
    inrun = (rows >= best0 * CHUNK) & (rows < best1 * CHUNK)
    max_off = int(np.abs(lj[inrun] - rows[inrun]).max()) if inrun.any() else 0
    return hcols.astype(np.int32), lj.astype(np.int32), best0, best1, max_off


def random_rows(n: int, seed: int):
    """n rows: the diagonal (8 + i % 5) and 6 columns anywhere, the row's entries in a scrambled
    (unsorted) order; every third row repeats one of its off-diagonal columns, so a halo column
    turns up twice in a row, and some rows hit their own diagonal again.  More than 255 distinct
    col - row, and owners that are no neighbours."""
    r = splitmix64(seed, 8 * n)
    Ap = np.zeros(n + 1, np.int32)
    Aj, Ax = [], []
    for i in range(n):
        cols = [int(r[8 * i + t] % np.uint64(n)) for t in range(6)]
        if i % 3 == 0:
            cols[5] = cols[0]
        cols.insert(int(r[8 * i + 6] % np.uint64(7)), i)
        vals = [(8.0 + i % 5) if c == i and k == cols.index(i) else -0.125 * (1 + (k + i) % 4)
                for k, c in enumerate(cols)]
        Aj += cols
        Ax += vals
        Ap[i + 1] = len(Aj)
    return Ap, np.asarray(Aj, np.int32), np.asarray(Ax, np.float64)


def tridiag(n: int):
    Ap, Aj, Ax = [0], [], []
    for i in range(n):
        for c, v in ((i - 1, -1.0), (i, 2.5), (i + 1, -1.25)):
            if 0 <= c < n:
                Aj.append(c)
                Ax.append(v)
        Ap.append(len(Aj))
    return np.asarray(Ap, np.int32), np.asarray(Aj, np.int32), np.asarray(Ax, np.float64)


def step_values(Ap, Aj, Ax, r0: int, seed: int):
    """a time step's values on a rank's rows: Ax (1 + 0.25 uniform(seed)), then every diagonal
    set to 1 + the sum of the row's other magnitudes, so the matrix stays diagonally dominant"""
    new = Ax * (1.0 + 0.25 * uniform(seed, Ax.size))
    rows = np.repeat(np.arange(Ap.size - 1), np.diff(Ap))
    diag = Aj == rows + r0
    off = np.bincount(rows[~diag], weights=np.abs(new[~diag]), minlength=Ap.size - 1)
    new[diag] = 1.0 + off[rows[diag]]
    return new
