"""BILUK on the GPU: the device numeric factorization, the apply and solves.

  * factors: lssp_amd_bilu_create (k_bilu0_level for bs <= 8) is bitwise
    lssp_amd_bilu_factor_host (which tests/test_bilu_cpu.py pins to LAPACK);
  * apply: x = U^-1 D L^-1 rhs bitwise the oracle's sweeps and product on the
    handle's own L, Dinv, U -- in place, repeated (both shadow parities),
    asynchronous, and from a handle made by lssp_amd_ilu_from_ldu;
  * solves with BILUK(0): convergence, the gain over no preconditioner, the
    true residual, and run-to-run bitwise determinism.
"""
import numpy as np
import pytest

import oracle as O
from bilu_util import CASES, bilu_apply, block_grid, case_name, diag_csr
from inputs import uniform

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import lssp_amd
    d = lssp_amd.Device(0)
    yield d
    d.close()


def _case_matrix(c):
    dim, N, bs, level, shuffle, variant = c
    return block_grid(dim, N, bs, seed=100 + CASES.index(c), shuffle=shuffle, variant=variant)


def _same(a, b):
    """bitwise"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("c", CASES, ids=[case_name(c) for c in CASES])
def test_device_factors_bitwise_host_and_apply_bitwise_oracle(dev, c):
    import lssp_amd
    Ap, Aj, Ax = _case_matrix(c)
    bs, level = c[2], c[3]
    n = Ap.size - 1
    M = lssp_amd.DILU.bilu(dev, Ap, Aj, Ax, bs, level=level)
    hL, hD, hU = lssp_amd.bilu_factor_host(Ap, Aj, Ax, bs, level)
    L, U = M.factors()
    gbs, D = M.diag()
    assert gbs == bs
    for got, want in zip((*L, D, *U), (*hL, hD, *hU)):
        assert _same(got, want)
    assert (M.nnzL, M.nnzU) == (hL[1].size, hU[1].size)
    # a bs = 1 BILUK of a grid looks like a structured ILU(0): it must not take the line sweeps
    assert M.sweep_layout() == (0, 0, 0)

    rhs = uniform(0xB11 + n, n)
    want = bilu_apply(n, bs, L, D, U, rhs)
    x, r = dev.vec(n), dev.vec(n, rhs)
    M.apply(x, r)
    assert _same(x.download(), want)
    M.apply(x, r)  # the second apply runs on the other pair of shadows
    assert _same(x.download(), want)
    M.apply(r, r)  # x aliasing rhs
    assert _same(r.download(), want)
    r.upload(rhs)
    x.upload(np.zeros(n))
    M.apply_async(x, r)
    M.check()
    assert _same(x.download(), want)
    # the single sweeps on a BILUK handle
    one = O.CSR(n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))
    M.trisolve(0, x, r)
    assert _same(x.download(), O.ilu_apply(O.CSR(n, *L), one, rhs))
    M.trisolve(1, x, r)
    assert _same(x.download(), O.ilu_apply(one, O.CSR(n, *U), rhs))
    # the same factors uploaded as the reference's host setup leaves them
    Dc = diag_csr(n, bs, D)
    F = lssp_amd.DILU.from_ldu(dev, L, (Dc.Ap, Dc.Aj, Dc.Ax), U)
    assert F.diag()[0] == bs and _same(F.diag()[1], D) and F.sweep_layout() == (0, 0, 0)
    for _ in range(2):
        F.apply(x, r)
        assert _same(x.download(), want)
    F.close()
    M.close()


def test_ilu_handles_report_no_block_size(dev):
    import lssp_amd
    Ap, Aj, Ax = lssp_amd.poisson(3, 6)
    M = lssp_amd.DILU.create(dev, Ap, Aj, Ax, kind=lssp_amd.ILUK, level=0)
    assert M.diag() == (0, None)
    M.close()


def test_singular_block_is_einval_and_the_context_stays_usable(dev):
    import lssp_amd
    Az = block_grid(2, 16, 2, seed=9, variant="zerodiag")
    with pytest.raises(lssp_amd.LsspError) as e:
        lssp_amd.DILU.bilu(dev, *Az, 2)
    assert e.value.status == 1  # LSSP_AMD_EINVAL, as the host path
    with pytest.raises(lssp_amd.LsspError):
        lssp_amd.bilu_factor_host(*Az, 2)
    Ap, Aj, Ax = block_grid(2, 16, 2, seed=9)
    M = lssp_amd.DILU.bilu(dev, Ap, Aj, Ax, 2)  # the next create on the same context succeeds
    hL, hD, hU = lssp_amd.bilu_factor_host(Ap, Aj, Ax, 2)
    assert _same(M.diag()[1], hD) and _same(M.factors()[0][2], hL[2]) and _same(M.factors()[1][2], hU[2])
    M.close()


def test_bad_block_sizes(dev):
    import lssp_amd
    Ap, Aj, Ax = block_grid(2, 6, 2, seed=5)
    for bs in (5, 0, 72):  # n % bs != 0; bs < 1; bs > 32
        with pytest.raises(lssp_amd.LsspError) as e:
            lssp_amd.DILU.bilu(dev, Ap, Aj, Ax, bs)
        assert e.value.status == 1


SOLVE_SHAPES = [(3, 8, 3), (3, 6, 4), (2, 16, 2)]


@pytest.mark.parametrize("shape", SOLVE_SHAPES, ids=[f"{N}^{d}-bs{bs}" for d, N, bs in SOLVE_SHAPES])
def test_solves_with_biluk(dev, shape):
    import lssp_amd
    dim, N, bs = shape
    Ap, Aj, Ax = block_grid(dim, N, bs, seed=300 + bs)
    n = Ap.size - 1
    sp, sj, sx = lssp_amd.sort_columns(Ap, Aj, Ax)
    A = lssp_amd.DMat(dev, sp, sj, sx)
    Ao = O.CSR(n, sp, sj, sx)
    M = lssp_amd.DILU.bilu(dev, Ap, Aj, Ax, bs, level=0)
    bh = uniform(77, n)
    b = dev.vec(n, bh)
    maxit = 1000
    nits = {}
    for name, solver, kw in (("bicgstab", lssp_amd.BICGSTAB, {}), ("gmres", lssp_amd.GMRES, {"restart": 30}),
                             ("rgmres", lssp_amd.RGMRES, {"restart": 30}), ("rlgmres", lssp_amd.RLGMRES, {"restart": 30})):
        xs = []
        for rep in range(2):  # the same solve twice on one handle: bitwise identical
            x = dev.vec(n, np.zeros(n))
            r = lssp_amd.solve(dev, A, M, x, b, solver=solver, tol_rel=1e-7, maxit=maxit, **kw)
            xs.append(x.download())
        assert 0 < r.nits < maxit, (name, r.nits)
        true = np.linalg.norm(bh - O.spmv(0, Ao, xs[0])) / np.linalg.norm(bh)
        print(f"\n{name} {shape}: {r.nits} its, true relative residual {true:.3e}")
        # a cap two orders above tol_rel: the left-preconditioned drivers monitor the preconditioned residual
        assert true <= 1e-5, (name, true)
        assert _same(xs[0], xs[1]), name
        nits[name] = r.nits
    if dim == 3:
        x = dev.vec(n, np.zeros(n))
        r0 = lssp_amd.solve(dev, A, None, x, b, solver=lssp_amd.BICGSTAB, tol_rel=1e-7, maxit=maxit)
        print(f"bicgstab {shape}: {nits['bicgstab']} its with BILUK(0), {r0.nits} without")
        assert 4 * nits["bicgstab"] <= r0.nits
    M.close()
    A.close()
