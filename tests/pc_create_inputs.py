"""Matrices and the pattern restatement of the lssp_amd_pc_create_dev tests (CPU harness and GPU)."""
import numpy as np

from ilut_inputs import csr
from inputs import rand_csr, uniform


def five():
    """5 x 5: a full diagonal plus (0,1), (1,4), (3,0), (3,1).  At level 1 row 3 of F is {0, 1, 3} under the
    reference's level rule (a repeated hit RAISES the level: (3,1), an entry of A, is hit through pivot 0 and
    goes from level 0 to level 1, so (3,4) = (3,1) x (1,4) would enter at level 2 and is dropped) and
    {0, 1, 3, 4} under the textbook min rule ((3,1) stays at level 0, (3,4) enters at level 1)"""
    rows = [{0: 4.0, 1: -1.0}, {1: 4.5, 4: -0.5}, {2: 5.0}, {0: -0.75, 1: -0.25, 3: 5.5}, {4: 6.0}]
    return csr(rows)


def symbolic(Ap, Aj, level, rule="max"):
    """pc-iluk.cxx:22-135 restated: the sorted rows of F's pattern, as a list of column lists.  rule "max" is the
    reference's (a hit on a present column raises its level), "min" the textbook one (lowers it)"""
    n = Ap.size - 1
    Ucols, Ulev, F = [], [], []
    for i in range(n):
        lev = {int(c): 0 for c in Aj[Ap[i]:Ap[i + 1]] if c != i}
        done = set()
        while True:
            todo = [c for c in lev if c < i and c not in done]
            if not todo:
                break
            k = min(todo)
            done.add(k)
            for col, ul in zip(Ucols[k], Ulev[k]):
                it = ul + lev[k] + 1
                if it > level or col == i:
                    continue
                if col not in lev:
                    lev[col] = it
                elif rule == "max":
                    lev[col] = max(lev[col], it)
                else:
                    lev[col] = min(lev[col], it)
        up = sorted(c for c in lev if c > i)
        Ucols.append(up)
        Ulev.append([lev[c] for c in up])
        F.append(sorted(list(lev) + [i]))
    return F


def oracle_rows(L, U):
    """the union pattern of the oracle's factors: row i = L's strict part, the diagonal, U's strict part"""
    n = L.Ap.size - 1
    return [sorted(set(int(c) for c in L.Aj[L.Ap[i]:L.Ap[i + 1]]) | set(int(c) for c in U.Aj[U.Ap[i]:U.Ap[i + 1]]))
            for i in range(n)]


# ---- the pattern builders of test_gpu_iluk_refactor.py --------------------------------
_PAT = {}


def box(nx, ny, nz, holes=False):
    """pattern of the 7-pt stencil on an nx x ny x nz box (nz = 1: 5-pt), natural order, rows
    sorted; holes: every 17th row lacks its r + 1 and r - nx entries"""
    key = (nx, ny, nz, holes)
    if key not in _PAT:
        n = nx * ny * nz
        Ap, Aj = [0], []
        for r in range(n):
            i, j, k = r % nx, r // nx % ny, r // (nx * ny)
            cut = holes and r % 17 == 16
            Aj += [c for c, ok in ((r - nx * ny, k > 0), (r - nx, j > 0 and not cut), (r - 1, i > 0), (r, True),
                                   (r + 1, i < nx - 1 and not cut), (r + nx, j < ny - 1), (r + nx * ny, k < nz - 1))
                   if ok]
            Ap.append(len(Aj))
        _PAT[key] = (np.array(Ap, np.int32), np.array(Aj, np.int32))
    return _PAT[key]


def values(Ap, Aj, k):
    """value set k on a pattern: off-diagonals in [-1, -0.1), diagonals in [7, 8)"""
    n, nnz = Ap.size - 1, Aj.size
    Ax = -0.55 + 0.45 * uniform(9000 + 31 * k, nnz)
    d = Aj == np.repeat(np.arange(n), np.diff(Ap))
    Ax[d] = 7.5 + 0.5 * uniform(9500 + 31 * k, nnz)[d]
    return Ax


RAND6_SEED = 11  # test_gpu_iluk_refactor.py's; the min rule's level-1 pattern differs from the reference's on it


def pattern(name):
    if name == "grid5":
        return box(40, 50, 1)
    if name == "holed":
        return box(9, 21, 13, holes=True)
    if name == "rand6":
        return rand_csr(3000, 6, RAND6_SEED, unsorted=False)[:2]
    if name == "box786":
        return box(7, 8, 6)
    if name == "five":
        return five()[:2]
    nx, ny, nz = name
    return box(nx, ny, nz)
