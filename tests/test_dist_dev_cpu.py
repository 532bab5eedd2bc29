"""CPU side of the device-made distributed handles (lssp_amd_mat_from_device_dist,
lssp_amd_mat_local_block, lssp_amd_mat_local_block_refresh): the argument checks that answer
before anything touches the device, and the numpy statement of the local numbering
(dist_dev_util.halo_plan) that tests/test_gpu_dist_dev.py holds the device builder against.
Here that statement is compared with the walk over every entry that the host upload used to
make (an ordered map of the halo columns, a scan of every chunk's rows), and its numbering is
used for the product the ranks of tests/test_dist_cpu.py compute with the gathered x."""
import ctypes

import numpy as np
import pytest

import oracle as O
from dist_dev_util import halo_plan, local_rows, random_rows, rank_rows, tridiag
from inputs import uniform

EINVAL = 1


def _lib():
    from lssp_amd import _lib as L
    return L.load()


def test_new_calls_are_declared_and_in_the_ctypes_table():
    from lssp_amd import _lib as L
    for name in ("lssp_amd_mat_from_device_dist", "lssp_amd_mat_local_block", "lssp_amd_mat_local_block_refresh"):
        assert name in L.SIGNATURES
        assert getattr(L.load(), name) is not None


def test_null_arguments_return_einval():
    """NULL context, NULL handles and NULL out-pointers answer LSSP_AMD_EINVAL before the
    context is read (the context here is a placeholder that must never be dereferenced)."""
    lib = _lib()
    out = ctypes.c_void_p()
    fake = ctypes.create_string_buffer(64)  # stands for a non-NULL handle; the NULL beside it decides
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    assert lib.lssp_amd_mat_from_device_dist(None, 8, 0, 8, 0, None, None, None, ctypes.byref(out)) == EINVAL
    assert lib.lssp_amd_mat_from_device_dist(ctx, 8, 0, 8, 0, None, None, None, None) == EINVAL
    assert lib.lssp_amd_mat_local_block(None, None, None) == EINVAL
    assert lib.lssp_amd_mat_local_block(None, ctx, ctypes.byref(out)) == EINVAL
    assert lib.lssp_amd_mat_local_block(ctx, None, ctypes.byref(out)) == EINVAL
    assert lib.lssp_amd_mat_local_block(ctx, ctx, None) == EINVAL
    assert lib.lssp_amd_mat_local_block_refresh(None, None, None) == EINVAL
    assert lib.lssp_amd_mat_local_block_refresh(None, ctx, ctx) == EINVAL
    assert lib.lssp_amd_mat_local_block_refresh(ctx, None, ctx) == EINVAL
    assert lib.lssp_amd_mat_local_block_refresh(ctx, ctx, None) == EINVAL
    assert out.value is None


def _host_walk(Ap, Aj, r0, nl):
    """the walk of the host upload: an ordered map of the halo columns over every entry, the
    renumbering entry by entry, every chunk's rows scanned for a halo column (strict >: the
    first longest run wins)"""
    halo = {}
    for g in Aj:
        if g < r0 or g >= r0 + nl:
            halo[int(g)] = 0
    hcols = sorted(halo)
    for q, g in enumerate(hcols):
        halo[g] = q
    lj = [int(g) - r0 if r0 <= g < r0 + nl else nl + halo[int(g)] for g in Aj]
    nch = (nl + 255) // 256
    run0 = best0 = best1 = 0
    for ch in range(nch + 1):
        free = ch < nch
        if free:
            for i in range(ch * 256, min((ch + 1) * 256, nl)):
                if any(lj[k] >= nl for k in range(Ap[i], Ap[i + 1])):
                    free = False
                    break
        if not free:
            if ch - run0 > best1 - best0:
                best0, best1 = run0, ch
            run0 = ch + 1
    mo = 0
    for i in range(best0 * 256, min(best1 * 256, nl)):
        for k in range(Ap[i], Ap[i + 1]):
            mo = max(mo, abs(lj[k] - i))
    return hcols, lj, best0, best1, mo


def _cases():
    yield "7-pt 12^3 over 2", O.poisson(3, 12), 2
    yield "7-pt 10^3 over 3", O.poisson(3, 10), 3
    yield "7-pt 16^3 over 4", O.poisson(3, 16), 4
    Ap, Aj, Ax = random_rows(600, 0xD157)
    yield "random 600 over 3", O.CSR(600, Ap, Aj, Ax), 3
    Ap, Aj, Ax = tridiag(5)
    yield "tridiagonal 5 over 4", O.CSR(5, Ap, Aj, Ax), 4
    yield "7-pt 6^3 over 1", O.poisson(3, 6), 1


@pytest.mark.parametrize("name,A,world", list(_cases()), ids=[c[0] for c in _cases()])
def test_numpy_plan_equals_the_host_walk_and_carries_the_product(name, A, world):
    xg = uniform(0xD157, A.n)
    want = O.spmv(0, A, xg)
    got = []
    for rank in range(world):
        r0, nl = rank_rows(A.n, world, rank)
        Ap, Aj, Ax = local_rows(A.Ap, A.Aj, A.Ax, r0, nl)
        hcols, lj, ich0, ich1, mo = halo_plan(Ap, Aj, r0, nl)
        w = _host_walk(Ap, Aj, r0, nl)
        assert (list(hcols), list(lj), ich0, ich1, mo) == w, (name, rank)
        # ascending global order is grouped by owner: the owners of the list never decrease
        blk = (A.n + world - 1) // world
        assert np.all(np.diff(hcols // blk) >= 0) and np.all(np.diff(hcols) > 0)
        # the rows of the run read no halo column; NaN there would reach y otherwise
        xl = np.concatenate([xg[r0:r0 + nl], xg[hcols]])
        yl = O.spmv(0, O.CSR(nl, Ap, lj, Ax), xl) if nl else np.zeros(0)
        xn = np.concatenate([xg[r0:r0 + nl], np.full(hcols.size, np.nan)])
        yn = O.spmv(0, O.CSR(nl, Ap, lj, Ax), xn) if nl else np.zeros(0)
        assert not np.isnan(yn[ich0 * 256:min(ich1 * 256, nl)]).any()
        # what the gloo ranks of test_dist_cpu compute: the local rows on the gathered x
        assert np.array_equal(yl, O.spmv(0, O.CSR(nl, Ap, Aj, Ax), xg) if nl else yl)
        got.append(yl)
    assert np.array_equal(np.concatenate(got), want)


def test_the_cases_reach_what_they_are_for():
    """the shapes of tests/test_gpu_dist_dev.py: a non-empty run on both ranks of 12^3 / 2; no
    halo-free chunk on the middle rank of 10^3 / 3; the run strictly inside on the middle ranks of
    16^3 / 4; non-neighbour owners, a repeated halo column and more than 255 offsets in the random
    rows; a rank with one row and one with none in the tridiagonal"""
    def plan(A, world, rank):
        r0, nl = rank_rows(A.n, world, rank)
        Ap, Aj, _ = local_rows(A.Ap, A.Aj, A.Ax, r0, nl)
        return (r0, nl, Ap, Aj) + halo_plan(Ap, Aj, r0, nl)
    A = O.poisson(3, 12)
    for rank in range(2):
        _, nl, _, _, hcols, _, i0, i1, _ = plan(A, 2, rank)
        assert nl == 864 and hcols.size == 144 and i1 > i0
    A = O.poisson(3, 10)
    assert [rank_rows(A.n, 3, r)[1] for r in range(3)] == [334, 334, 332]
    _, _, _, _, hcols, _, i0, i1, _ = plan(A, 3, 1)
    assert i0 == i1 and set(hcols // 334) == {0, 2}
    A = O.poisson(3, 16)
    for rank in (1, 2):
        assert plan(A, 4, rank)[6:8] == (1, 3)
    Ap, Aj, Ax = random_rows(600, 0xD157)
    A = O.CSR(600, Ap, Aj, Ax)
    r0, nl, lp, lj, hcols, *_ = plan(A, 3, 0)
    assert set(hcols // 200) == {1, 2}
    rows = np.repeat(np.arange(600), np.diff(Ap))
    assert np.unique(Aj - rows).size > 255
    rep = [i for i in range(nl) if len(set(lj[lp[i]:lp[i + 1]])) < lp[i + 1] - lp[i]
           and any(c >= 200 for c in lj[lp[i]:lp[i + 1]] if list(lj[lp[i]:lp[i + 1]]).count(c) > 1)]
    assert rep, "no row repeats a halo column"
    assert any(np.any(np.diff(Aj[Ap[i]:Ap[i + 1]]) < 0) for i in range(600))
    assert [rank_rows(5, 4, r) for r in range(4)] == [(0, 2), (2, 2), (4, 1), (5, 0)]
