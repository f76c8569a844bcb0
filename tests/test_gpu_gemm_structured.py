"""The structured products of zgemm (csrc/gemm_kernels.hip) at the ABI, and the solver that uses them:

  DFTK_MI_GEMM_B_UPPER     X * inv(R): the k loop of a tile column stops at the diagonal, and inside the diagonal block the
                           entries of B below the diagonal are staged as zeros.  The call must equal the dense call on
                           triu(B) BIT FOR BIT (the k order inside a tile is the same, what the dense call adds on top are
                           exact zeros; with a K split both calls share one plan and the chunks behind the diagonal hold
                           zeros), and a NaN anywhere strictly below the diagonal of B must not reach C.
  DFTK_MI_GEMM_SYM_RESULT  'N' products with a Hermitian result (the Newton-Schulz step of dftk_mi_heev_lowest): every entry
                           on or above the diagonal is computed -- in REAL rows for the "tall" REAL layout, where a complex
                           row holds two of them -- and what is not computed is left untouched.  The solver's mirror pass
                           (dftk_mi_eig_mirror_tall) is run on that output on the device -- the full product, exactly
                           Hermitian, padding row zero -- and by itself on matrices with NaN wherever it must not read.
  dftk_mi_heev_lowest      at sizes right above its threshold (384) and with an odd number of tile rows (518), real symmetric
                           and complex Hermitian, and at the sizes where its Newton-Schulz step takes the symmetric-result
                           product (1509 real, 1280 complex; asserted from the launch plan): the pairs against LAPACK,
                           columns and eigenvalues from nev on untouched (the split answered, not the full solver that takes
                           over when the split fails its checks), and two calls give bitwise-equal vectors.

References are NumPy products in float64 / complex128 on the host.  Shapes: m = 100 (predicated tiles only), 128 (one full row
tile), 300 (a shifted row tile), 1000 (several row panels); n = k = 63, 64, 65 (one tile, with and without a ragged / shifted
neighbour), 128, 129, 192, 200 (even and odd tile counts, shifted last tile column), 503 (the benchmark's width, with a K split
at these heights)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check, cplx  # noqa: E402

from test_gpu_eig import check_pairs, rr_like  # noqa: E402
from test_gpu_kernels import Basis, dev  # noqa: E402

B_UPPER, GEMM_REAL, SYM_RESULT = 2, 8, 32
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs(lib):
    return Basis(lib, 8, 8, 8)


def zgemm(lib, bs, trans, m, n, k, alpha, Ad, lda, Bd, ldb, beta, Cd, ldc, flags):
    st = lib.dftk_mi_zgemm_ex(bs.h, trans, m, n, k, cplx(alpha), Ad.data_ptr(), lda, Bd.data_ptr(), ldb, cplx(beta),
                              Cd.data_ptr(), ldc, flags)
    bs.sync()
    return st


def triangular_case(lib, bs, real, m, n, k, alpha, beta, seed):
    """(structured call on B with NaN strictly below the diagonal, dense call on triu(B), host reference, error bound)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, k)) + 1j * rng.standard_normal((m, k))
    Bt = np.triu(rng.standard_normal((k, n)) + 1j * rng.standard_normal((k, n)))
    Bnan = Bt.copy()
    Bnan[np.tril_indices(k, -1, n)] = np.nan + 1j * np.nan
    C0 = rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))
    fl = GEMM_REAL if real else 0
    Ad = dev(A.T.copy())
    out = []
    for Bh, flags in ((Bnan, fl | B_UPPER), (Bt, fl)):
        Cd = dev(C0.T.copy())
        assert zgemm(lib, bs, b"N", m, n, k, alpha, Ad, m, dev(Bh.T.copy()), k, beta, Cd, m, flags) == 0
        out.append(np.ascontiguousarray(Cd.cpu().numpy().T))
    Beff = Bt.real if real else Bt
    ref = alpha * (A @ Beff) + beta * C0
    # summation error of a length-k inner product, k eps sum |a||b|; a factor 4 covers the three-product complex
    # multiplication and the alpha / beta epilogue
    bound = 4 * k * EPS * (abs(alpha) * (np.abs(A) @ np.abs(Beff)) + abs(beta) * np.abs(C0)) + 1e-300
    return out[0], out[1], ref, bound


@pytest.mark.parametrize("real", [True, False], ids=["REAL", "complex"])
@pytest.mark.parametrize("coef", [(1.0, 0.0), (-0.7 + 0.2j, 0.3)], ids=["plain", "alpha_beta"])
@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 192, 200, 503])
@pytest.mark.parametrize("m", [100, 128, 300, 1000])
def test_b_upper_equals_the_dense_call_on_triu_bit_for_bit(lib, bs, m, n, coef, real):
    alpha, beta = coef
    if real:
        alpha = alpha.real      # a REAL product is a real product: real alpha
    got, dense, ref, bound = triangular_case(lib, bs, real, m, n, n, alpha, beta, 1000 * m + n)
    assert np.isfinite(got.view(float)).all(), "a NaN below the diagonal of B reached C"
    assert np.all(np.abs(got - ref) <= bound), float(np.max(np.abs(got - ref) / bound))
    assert np.array_equal(got.view(np.uint64), dense.view(np.uint64))


@pytest.mark.parametrize("real", [True, False], ids=["REAL", "complex"])
@pytest.mark.parametrize("n", [65, 128, 129, 192, 200, 503])
def test_b_upper_folded_launch_equals_the_dense_call(lib, bs, n, real):
    """Tall enough that the plan has no K split (more tiles than resident workgroups): the triangular call then runs two
    column tiles per workgroup (tile p after tile gn - 1 - p; the middle one alone for an odd count), with a ragged last row
    tile.  Same contract: the dense call on triu(B), bit for bit."""
    gn = -(-n // (64 if real else 32))
    m = (512 // gn + 1) * 128 + 37
    out = (C.c_int * 12)()
    check(lib.dftk_mi_zgemm_plan_host(b"N", m, n, n, B_UPPER | (GEMM_REAL if real else 0), out))
    assert out[5] == 1 and out[3] == 0 and out[4] == 0, list(out)      # no K split, no border launch
    cnt = C.c_int()
    check(lib.dftk_mi_zgemm_fold_host(b"N", m, n, n, B_UPPER | (GEMM_REAL if real else 0), 0, None, C.byref(cnt)))
    assert cnt.value == (m // 128 + 1) * gn                            # the folded launch is taken, over every tile
    got, dense, ref, bound = triangular_case(lib, bs, real, m, n, n, 0.7 if real else 0.7 - 0.2j, 0.3, 7 * n + int(real))
    assert np.isfinite(got.view(float)).all(), "a NaN below the diagonal of B reached C"
    assert np.all(np.abs(got - ref) <= bound), float(np.max(np.abs(got - ref) / bound))
    assert np.array_equal(got.view(np.uint64), dense.view(np.uint64))


@pytest.mark.parametrize("real", [True, False], ids=["REAL", "complex"])
def test_b_upper_with_more_rows_in_B_than_columns(lib, bs, real):
    """k > n: the rows of B from n on lie below the diagonal altogether.  The call is accepted and is the dense call on
    triu(B), as for k = n (pinned: the tile columns stop at the diagonal, the rows beyond are never read)."""
    got, dense, ref, bound = triangular_case(lib, bs, real, 300, 129, 200, 1.0, 0.0, 77)
    assert np.isfinite(got.view(float)).all()
    assert np.all(np.abs(got - ref) <= bound)
    assert np.array_equal(got.view(np.uint64), dense.view(np.uint64))


FILL = 7.0 + 3.0j


def symmetric_pair(n, cplx_, rng):
    """Hermitian X with norm below 1 and Y = 1.5 I - 0.5 X^2: X Y is Hermitian"""
    X = rng.standard_normal((n, n)) + (1j * rng.standard_normal((n, n)) if cplx_ else 0)
    X = (X + X.conj().T) / 2
    X = X / (1.1 * np.linalg.norm(X, 2))
    Y = 1.5 * np.eye(n) - 0.5 * (X @ X)
    Y = (Y + Y.conj().T) / 2
    return X, Y


def mirror_on_device(lib, bs, Cd, n, real, ldt):
    check(lib.dftk_mi_eig_mirror_tall(bs.h, n, int(real), Cd.data_ptr(), ldt))
    bs.sync()
    return Cd.cpu().numpy().T


@pytest.mark.parametrize("n", [127, 128, 129, 402])
def test_sym_result_complex(lib, bs, n):
    rng = np.random.default_rng(n)
    X, Y = symmetric_pair(n, True, rng)
    Cd = torch.full((n, n), FILL, dtype=torch.complex128, device="cuda")
    assert zgemm(lib, bs, b"N", n, n, n, 1.0, dev(X.T.copy()), n, dev(Y.T.copy()), n, 0.0, Cd, n, SYM_RESULT) == 0
    got = Cd.cpu().numpy().T
    ref = X @ Y
    tol = 4 * n * EPS * np.linalg.norm(X, 2) * np.linalg.norm(Y, 2)
    iu = np.triu_indices(n)
    assert np.abs(got[iu] - ref[iu]).max() <= tol
    # nothing but the product or the old contents anywhere; whole tiles below the diagonal are skipped where there are any
    assert np.all((np.abs(got - ref) <= tol) | (got == FILL))
    if n > 128 + 32:
        assert got[n - 1, 0] == FILL
    # the mirror pass of the solver, on the device: the full product, exactly Hermitian, real diagonal; the upper triangle
    # is what the product wrote (the diagonal apart)
    full = mirror_on_device(lib, bs, Cd, n, False, n)
    assert np.abs(full - ref).max() <= tol
    assert np.array_equal(full, full.conj().T)
    assert not np.diag(full).imag.any()
    assert np.array_equal(np.triu(full, 1), np.triu(got, 1)) and np.array_equal(np.diag(full).real, np.diag(got).real)
    # 'C' products know no symmetric result
    assert zgemm(lib, bs, b"C", n, n, n, 1.0, dev(X.T.copy()), n, dev(Y.T.copy()), n, 0.0, Cd, n, SYM_RESULT) < 0


@pytest.mark.parametrize("n", [127, 128, 129, 402])
def test_sym_result_real_tall(lib, bs, n):
    """REAL "tall" layout: complex row i of A and C holds the REAL rows 2 i and 2 i + 1 (a zero padding row for odd n); the
    diagonal is met in REAL rows, i.e. a tile is needed when 2 * (its first complex row) <= its last column."""
    rng = np.random.default_rng(n + 1)
    X, Y = symmetric_pair(n, False, rng)
    ldt = (n + 1) // 2
    Xp = np.zeros((2 * ldt, n))
    Xp[:n] = X
    tall = Xp[0::2] + 1j * Xp[1::2]                       # ldt x n
    Cd = torch.full((n, ldt), FILL, dtype=torch.complex128, device="cuda")
    assert zgemm(lib, bs, b"N", ldt, n, n, 1.0, dev(tall.T.copy()), ldt, dev(Y.astype(complex).T.copy()), n, 0.0, Cd, ldt,
                 GEMM_REAL | SYM_RESULT) == 0

    def real_rows(Ct):                                    # ldt x n complex -> 2 ldt x n real
        R = np.empty((2 * ldt, n))
        R[0::2], R[1::2] = Ct.real, Ct.imag
        return R

    got = real_rows(Cd.cpu().numpy().T)
    ref = np.zeros((2 * ldt, n))
    ref[:n] = X @ Y
    fill = real_rows(np.full((ldt, n), FILL))
    tol = 4 * n * EPS * np.linalg.norm(X, 2) * np.linalg.norm(Y, 2)
    iu = np.triu_indices(n)
    assert np.abs(got[:n][iu] - ref[:n][iu]).max() <= tol
    assert np.all((np.abs(got - ref) <= tol) | (got == fill))
    if n > 2 * 128 + 64:
        assert got[n - 1, 0] == fill[n - 1, 0]            # REAL rows from 256 on skip the first tile column
    # the mirror pass of the solver, on the device: the full product, exactly symmetric, padding row exactly zero
    full = real_rows(mirror_on_device(lib, bs, Cd, n, True, ldt))
    assert np.abs(full - ref).max() <= tol
    assert np.array_equal(full[:n], full[:n].T)
    assert not full[n:].any()
    assert np.array_equal(np.triu(full[:n]), np.triu(got[:n]))


@pytest.mark.parametrize("real,n", [(False, 33), (False, 200), (True, 33), (True, 95), (True, 200)])
def test_mirror_pass_alone(lib, bs, real, n):
    """dftk_mi_eig_mirror_tall on a matrix whose lower triangle (and, REAL, padding rows -- two extra complex rows of them
    here) holds NaN: entry (i, j), i > j, becomes conj(entry (j, i)), a complex diagonal loses its imaginary part, the
    padding becomes zero, the upper triangle is left as it is.  Sizes: 33 and 95 end inside a 32 x 32 tile, 200 spans seven."""
    rng = np.random.default_rng(n + int(real))
    if real:
        ldt = (n + 1) // 2 + 2
        U = np.triu(rng.standard_normal((n, n)))
        M = np.full((2 * ldt, n), np.nan)
        M[:n][np.triu_indices(n)] = U[np.triu_indices(n)]
        tall = np.empty((ldt, n), dtype=complex)          # (not re + 1j * im: 1j * nan is nan + nan j)
        tall.real, tall.imag = M[0::2], M[1::2]
        Cd = dev(tall.T.copy())
        Ct = mirror_on_device(lib, bs, Cd, n, True, ldt)
        out = np.empty((2 * ldt, n))
        out[0::2], out[1::2] = Ct.real, Ct.imag
        assert np.array_equal(out[:n], U + np.triu(U, 1).T) and not out[n:].any()
    else:
        U = np.triu(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
        M = U.copy()
        M[np.tril_indices(n, -1)] = np.nan + 1j * np.nan
        out = mirror_on_device(lib, bs, dev(M.T.copy()), n, False, n)
        want = np.triu(U, 1) + np.triu(U, 1).conj().T + np.diag(np.diag(U).real)
        assert np.array_equal(out, want)


def sym_step_workgroups(lib, n, cplx_):
    """workgroups of the FULL Newton-Schulz product of an n x n problem at its planned K split (zgemm_sym_result_pays)"""
    m = n if cplx_ else (n + 1) // 2
    out = (C.c_int * 12)()
    check(lib.dftk_mi_zgemm_plan_host(b"N", m, n, n, 0 if cplx_ else GEMM_REAL, out))
    assert out[3] == 0 and out[4] == 0, list(out)         # no border launch at these sizes
    gm = out[1] + (1 if m % 128 else 0)
    gn = out[2] + out[11]
    return gm * gn * out[5]


# 384 / 518: the sizes right above the solver's threshold.  1509 real (nev = n / 3) and 1280 complex: the sizes at which the
# Newton-Schulz step runs as a symmetric-result product and the mirror kernel completes the iterate (the full product would
# need two rounds of workgroups there; csrc/gemm_kernels.hip, zgemm_sym_result_pays)
@pytest.mark.parametrize("n,nev,cplx_,sym", [(384, 192, False, False), (384, 192, True, False), (518, 259, False, False),
                                             (518, 259, True, False), (1509, 503, False, True), (1280, 640, True, True)])
def test_heev_lowest_pairs_and_determinism(lib, n, nev, cplx_, sym):
    # the symmetric-result product and its mirror pass run exactly where this test says they do
    assert (sym_step_workgroups(lib, n, cplx_) > 512) == sym
    h = C.c_void_p()
    check(lib.dftk_mi_basis_create(8, 8, 8, 1.0, 0, C.byref(h)))

    def lowest(A):
        Ad = torch.tensor(np.ascontiguousarray(A.T), dtype=torch.complex128, device="cuda")
        Vd = torch.zeros((n, n), dtype=torch.complex128, device="cuda")
        W = np.zeros(n)
        check(lib.dftk_mi_heev_lowest(h, n, nev, Ad.data_ptr(), n, W.ctypes.data, Vd.data_ptr(), n))
        torch.cuda.synchronize()
        Vall = Vd.cpu().numpy().T
        # the split itself answered: the full solver, which takes over when the sign iteration or the count check fails
        # (a wrong mirror pass makes them fail), writes all n pairs
        assert not Vall[:, nev:].any() and not W[nev:].any(), "the full solver took over"
        return W[:nev].copy(), np.ascontiguousarray(Vall[:, :nev])

    try:
        rng = np.random.default_rng(n + int(cplx_))
        A = rr_like(n, nev, rng, cplx_, 0.3)
        lam, V = lowest(A)
        ref = np.linalg.eigvalsh(A)
        nrm = max(abs(ref[0]), abs(ref[-1]))
        assert np.abs(lam - ref[:nev]).max() < 1e-11 * nrm
        assert np.abs(V.conj().T @ V - np.eye(nev)).max() < 1e-12
        check_pairs(A, lam, V, nev)                       # (the residual bound of test_gpu_eig.py)
        if not cplx_:
            assert np.abs(V.imag).max() == 0.0
        lam2, V2 = lowest(A)
        assert np.array_equal(V.view(np.uint64), V2.view(np.uint64))
        assert np.array_equal(lam, lam2)
    finally:
        lib.dftk_mi_basis_destroy(h)
