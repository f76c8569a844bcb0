"""DFTK_MI_LAND_IN_PLACE: results of the LOBPCG driver and of the Gamma-real density pass are written
where they are needed instead of being copied or added there afterwards.  Every floating-point operation keeps its operands,
so each case runs with the switch on and off IN ONE PROCESS and the results must be BITWISE equal; the LOBPCG cases also need
strictly fewer kernel launches with the switch on (``dftk_mi_launch_count``): the passes are really gone.

  zgemm_to            D = alpha op(A) B + beta C with D != C against the in-place call: both transposes, REAL and complex,
                      flags 0 / UPPER / triangular B, beta 0 and 1; m = 130 (one full row tile + predicated rest), 257, 1029
                      (shifted last row tile); n = 5, 64, 67, 131 (below one column tile, one, one + ragged rest, folded pair
                      + rest); k = 7, 64, 203; a folded triangular launch; one K-split 'C' shape (k = 20000, n = 67).
  ortho!(X)           from the routine's scratch copy (rows 4099, M = 5 and 67): orthonormal start (one pass, no copy back),
                      condition number 1e4 (two passes: the misprediction), forced SVD fallback.
  LOBPCG              Gamma-real and general complex, cube 18^3 and the triclinic 12 x 15 x 18 cell, M = 7 and 12: three
                      consecutive calls, the second and third promised the kept A X under a changed potential, with and
                      without kept y-planes; plus one block above the small-block threshold of ortho!(X, Y).
  density             real-symmetric orbitals, odd band count, a launch group of all-zero weights, with and without planes.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check, cplx  # noqa: E402

import exx_twin as twin  # noqa: E402
from test_gpu_kernels import Basis, dev  # noqa: E402

UPPER, B_UPPER, GEMM_REAL = 1, 2, 8
SWITCH = "DFTK_MI_LAND_IN_PLACE"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs(lib):
    return Basis(lib, 8, 8, 8)


def launches(lib):
    n = C.c_int64()
    check(lib.dftk_mi_launch_count(C.byref(n), None))
    return n.value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------------ zgemm_to
PADC = 3
SENTINEL = complex(-7.25e300, 3.5e-300)      # a bit pattern no product of these operands has


def colmajor(a, ld):
    """(rows x cols) -> host image (cols, ld) of the column-major device array with leading dimension ld"""
    h = np.full((a.shape[1], ld), SENTINEL)
    h[:, :a.shape[0]] = a.T
    return h


def gemm_case(lib, bs, trans, real, m, n, k, flags, beta, rng):
    """in-place call on a copy of C0, out-of-place call into a sentinel-filled D: what was written, and what C holds"""
    fl = flags | (GEMM_REAL if real else 0)
    A = rng.standard_normal((m, k)) + 1j * rng.standard_normal((m, k))
    B = rng.standard_normal((k, n)) + 1j * rng.standard_normal((k, n))
    if flags & B_UPPER:
        B = np.triu(B)            # ('C' products require the zeros in the array)
    C0 = rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n))
    Ad = dev(A.T.copy()) if trans == "N" else dev(np.conj(A).copy())       # 'C': the array holds A^H's argument, k x m
    lda = m if trans == "N" else k
    Bd = dev(B.T.copy())
    ldc = m + PADC
    c0 = colmajor(C0, ldc)
    alpha = 0.75 if real else 0.75 - 0.5j
    c1 = dev(c0)
    check(lib.dftk_mi_zgemm_ex(bs.h, trans.encode(), m, n, k, cplx(alpha), Ad.data_ptr(), lda, Bd.data_ptr(), k, cplx(beta),
                               c1.data_ptr(), ldc, fl))
    c2 = dev(c0)
    d = dev(np.full_like(c0, SENTINEL))
    check(lib.dftk_mi_zgemm_to(bs.h, trans.encode(), m, n, k, cplx(alpha), Ad.data_ptr(), lda, Bd.data_ptr(), k, cplx(beta),
                               c2.data_ptr(), ldc, d.data_ptr(), fl))
    bs.sync()
    return bits(c0), bits(c1.cpu().numpy()), bits(c2.cpu().numpy()), bits(d.cpu().numpy())


def assert_out_of_place(c0, c1, c2, d, m, n, flags, what):
    d3, c13, c03 = (x.reshape(x.shape[0], -1, 2) for x in (d, c1, c0))      # [column, row, (re, im)] as bit patterns
    written = (d3 != bits(np.array([SENTINEL]))).any(axis=-1)
    assert np.array_equal(c2, c0), f"{what}: C was written"
    assert not written[:, m:].any(), f"{what}: the padding of D was written"
    need = np.ones((n, m), dtype=bool)
    if flags & UPPER:
        need = np.arange(m)[None, :] <= np.arange(n)[:, None]            # entry (i, j), i <= j: host image [j, i]
        assert written[:, :m][need].all(), f"{what}: an entry on or above the diagonal was not written"
    else:
        assert written[:, :m].all(), f"{what}: an entry of D was not written"
    w = written
    assert np.array_equal(d3[w], c13[w]), f"{what}: D differs from the in-place result"
    assert np.array_equal(c13[~w], c03[~w]), f"{what}: the in-place call wrote an entry the out-of-place call left alone"


@pytest.mark.parametrize("real", [True, False], ids=["REAL", "complex"])
@pytest.mark.parametrize("trans", ["N", "C"])
def test_zgemm_to_equals_the_in_place_product(lib, bs, trans, real):
    rng = np.random.default_rng(11 + 2 * int(real) + (trans == "C"))
    for m in (130, 257, 1029):
        for n in (5, 64, 67, 131):
            for k in (7, 64, 203):
                for flags in (0, UPPER, B_UPPER):
                    for beta in (0.0, 1.0):
                        c0, c1, c2, d = gemm_case(lib, bs, trans, real, m, n, k, flags, beta, rng)
                        assert_out_of_place(c0, c1, c2, d, m, n, flags, f"{trans} m={m} n={n} k={k} flags={flags} beta={beta}")


@pytest.mark.parametrize("real", [True, False], ids=["REAL", "complex"])
def test_zgemm_to_folded_triangular_launch(lib, bs, real):
    """tall enough that the triangular product runs two column tiles per workgroup (asserted from the fold list)"""
    n = 131
    gn = -(-n // (64 if real else 32))
    m = (512 // gn + 1) * 128 + 37
    cnt = C.c_int()
    check(lib.dftk_mi_zgemm_fold_host(b"N", m, n, n, B_UPPER | (GEMM_REAL if real else 0), 0, None, C.byref(cnt)))
    assert cnt.value > 0
    rng = np.random.default_rng(5 + int(real))
    for beta in (0.0, 1.0):
        c0, c1, c2, d = gemm_case(lib, bs, "N", real, m, n, n, B_UPPER, beta, rng)
        assert_out_of_place(c0, c1, c2, d, m, n, B_UPPER, f"folded beta={beta}")


@pytest.mark.parametrize("real", [True, False], ids=["REAL", "complex"])
def test_zgemm_to_k_split(lib, bs, real):
    """'C', k = 20000, n = 67: the slabs of the K split are summed by the reduce kernel, which stores to D"""
    m, n, k = 130, 67, 20000
    out = (C.c_int * 12)()
    check(lib.dftk_mi_zgemm_plan_host(b"C", m, n, k, GEMM_REAL if real else 0, out))
    assert max(out[5], out[8]) > 1, list(out)
    rng = np.random.default_rng(21 + int(real))
    for flags in (0, UPPER):
        for beta in (0.0, 1.0):
            c0, c1, c2, d = gemm_case(lib, bs, "C", real, m, n, k, flags, beta, rng)
            assert_out_of_place(c0, c1, c2, d, m, n, flags, f"K split flags={flags} beta={beta}")


# ------------------------------------------------------------------------------------------------------ ortho!(X)
def ortho(lib, bs, X, flags):
    Xd = dev(X.T.copy())
    nch, svd = C.c_int(), C.c_int()
    l0 = launches(lib)
    check(lib.dftk_mi_ortho_qr(bs.h, X.shape[0], X.shape[1], Xd.data_ptr(), X.shape[0], flags, C.byref(nch), C.byref(svd)))
    bs.sync()
    return bits(Xd.cpu().numpy()), nch.value, svd.value, launches(lib) - l0


@pytest.mark.parametrize("m", [5, 67])
def test_ortho_from_the_scratch_copy(lib, bs, monkeypatch, m):
    """force_svd | 2 enters ortho!(X) with the block in the scratch copy, as the LOBPCG driver does.  Bitwise the result of
    the entry from X.  Launches: a pass count of one needs no copy back (moving the block in replaces it: same count as from
    X, where one pass ends in the scratch copy); a count of two pays the move and the copy back (two more than from X)."""
    n = 4099
    rng = np.random.default_rng(m)
    Q, _ = np.linalg.qr(rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m)))
    V, _ = np.linalg.qr(rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m)))
    ill = (Q * np.logspace(0, -4, m)) @ V.conj().T           # condition number 1e4
    for X, passes, force in ((Q, 1, 0), (ill, 2, 0), (ill, None, 1)):
        res = {}
        for flag in ("1", "0"):
            monkeypatch.setenv(SWITCH, flag)
            res[flag] = (ortho(lib, bs, X, force | 2), ortho(lib, bs, X, force))
        monkeypatch.delenv(SWITCH)
        (on2, on), (off2, off) = res["1"], res["0"]
        for r in (on2, on, off2):
            assert np.array_equal(r[0], off[0]) and r[1:3] == off[1:3]
        assert off2[3] == off[3] == on[3]                    # the bit is honoured with the switch on only
        if force:
            assert off[2] == 1 and off[1] == 100
        else:
            assert off[1] == passes and off[2] == 0          # one Cholesky factorisation per pass, no shift, no SVD
            assert on2[3] - on[3] == (0 if passes == 1 else 2)


# ------------------------------------------------------------------------------------------------------ LOBPCG
_cache = {}


def lobpcg_setup(grid, kcoord, supercell=(1, 1, 1), Ecut=None):
    """silicon on one of the two kernel-test grids (tests/exx_twin.py) at Gamma (real-symmetric format) or at a general
    k-point, three densities (three local potentials) and a 12-band start block"""
    key = (grid, tuple(kcoord), supercell)
    if key not in _cache:
        lat, atoms, pos = dftk.silicon_cell(supercell)
        fft_size = None
        if grid is not None:
            Ecut, fft_size, lattice = twin.KERNEL_TEST_GRIDS[grid]
            lat = lat if lattice is None else lattice
        model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_pw"))
        basis = dftk.PlaneWaveBasis(model, Ecut, dftk.ExplicitKpoints([list(kcoord)], [1.0]), coarse_start=False, fft_size=fft_size)
        assert bool(basis.kpoints[0].gamma_real) == (not any(kcoord))
        rho1 = dftk.guess_density(basis)
        z = torch.arange(basis.fft_size[2], device="cuda", dtype=torch.float64)
        rho2 = rho1 * (1.0 + 0.2 * torch.cos(2 * np.pi * z / basis.fft_size[2]))[:, None, None]
        rho3 = rho1 * (1.0 + 0.1 * torch.sin(2 * np.pi * z / basis.fft_size[2]))[:, None, None]
        gen = torch.Generator(device="cuda").manual_seed(3)
        X0 = dftk.random_orbitals(basis, basis.kpoints[0], 40 if grid is None else 12, gen)
        _cache[key] = (basis, (rho1, rho2, rho3), X0)
    return _cache[key]


def counter(lib, name):
    n = C.c_int64()
    check(getattr(lib, name)(C.byref(n)))
    return n.value


def three_calls(basis, rhos, X0, M, planes, limits, n_occ, n_conv_check):
    """call 1 from the start block, calls 2 and 3 from the block the call before returned, promised the kept A X, each under
    another potential; between them (planes) the density pass over the returned block.  `limits`: iteration limits of the
    three calls (the tolerance is out of reach, so they ARE the iteration counts).  Returns everything that is compared."""
    lib = basis.lib
    general = not basis.kpoints[0].gamma_real
    got = []
    X = X0[:M]
    occ = np.zeros(M)
    occ[:n_occ] = 2.0
    l0 = launches(lib)
    for i, (rho, maxiter) in enumerate(zip(rhos, limits)):
        _, ham = dftk.energy_hamiltonian(basis, None, None, rho=rho)
        a0, p0 = counter(lib, "dftk_mi_ax_reuse_count"), counter(lib, "dftk_mi_planes_reuse_count")
        r = dftk.lobpcg_hyper(ham[0], X, prec=dftk.PreconditionerTPA(ham[0]), tol=1e-14, n_conv_check=n_conv_check,
                              maxiter=maxiter, reuse_AX=i > 0)
        assert counter(lib, "dftk_mi_ax_reuse_count") - a0 == (1 if i > 0 else 0)
        assert counter(lib, "dftk_mi_planes_reuse_count") - p0 == (1 if i > 0 and planes and not general else 0)
        assert r.n_iter == maxiter
        hist, n_svd = dftk.lobpcg_residual_history(ham[0])
        got += [bits(r.λ), bits(r.residual_norms), bits(hist), bits(r.X.cpu().numpy()), n_svd]
        if general:
            # the A X the call keeps for the next one, through its inner products with the returned X
            ax = lib.dftk_mi_lobpcg_last_AX(basis.kpoints[0].handle)
            assert ax
            dots = (dftk._lib.dftk_mi_cplx * M)()
            n_G = r.X.shape[1]
            check(lib.dftk_mi_columnwise_dots(basis.handle, n_G, M, ax, n_G, r.X.data_ptr(), r.X.stride(0), dots))
            got.append(bits(np.array([complex(d.re, d.im) for d in dots])))
        if not general:
            rho_out = dftk.compute_density(basis, [r.X], [occ], real_symmetric=[True])
            got.append(bits(rho_out.cpu().numpy()))
        X = r.X
        if i == 0:
            sorted_on_return = bool(np.all(np.diff(r.λ) >= 0))
    return got, launches(lib) - l0, sorted_on_return


def on_and_off(monkeypatch, run, planes=True, general_driver=False):
    out = {}
    try:
        monkeypatch.setenv("DFTK_MI_PLANES_REUSE", "1" if planes else "0")
        if general_driver:       # (read per call: a block of at most 8 bands goes to the general driver, not the fused one)
            monkeypatch.setenv("DFTK_MI_KBATCH_SEQUENTIAL", "1")
        for flag in ("1", "0"):
            monkeypatch.setenv(SWITCH, flag)
            out[flag] = run()
    finally:
        for name in (SWITCH, "DFTK_MI_PLANES_REUSE", "DFTK_MI_KBATCH_SEQUENTIAL"):
            monkeypatch.delenv(name, raising=False)
    return out["1"], out["0"]


def assert_same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and np.array_equal(x, y), f"item {i} differs"
        else:
            assert x == y, f"item {i}: {x} != {y}"


# limits (0, 1, 2): call 1 ends before the first Rayleigh-Ritz step -- its Rayleigh quotients are those of the random start
# block, unsorted, so the exit sorts (item 5) -- and leaves the pair index at 0 (1 after the sort with the switch on); call 2
# ends at 1, call 3 at 2.  limits (2, 1, 2): the kept block of call 2 is the A X storage of pair 0, that of call 3 pair 1.
@pytest.mark.parametrize("limits", [(0, 1, 2), (2, 1, 2)])
@pytest.mark.parametrize("planes", [True, False], ids=["planes", "no_planes"])
@pytest.mark.parametrize("M", [7, 12])
@pytest.mark.parametrize("grid", ["cubic_18", "triclinic_12x15x18"])
def test_lobpcg_gamma_real(monkeypatch, grid, M, planes, limits):
    basis, rhos, X0 = lobpcg_setup(grid, (0.0, 0.0, 0.0))
    check(basis.lib.dftk_mi_basis_set_fft_batch(basis.handle, 3))     # (4 and 6 pairs: two launch groups, the last one ragged)
    try:
        on, off = on_and_off(monkeypatch, lambda: three_calls(basis, rhos, X0, M, planes, limits, 4, 4), planes)
    finally:
        check(basis.lib.dftk_mi_basis_set_fft_batch(basis.handle, 32))
    assert_same(on[0], off[0])
    assert on[1] < off[1], (on[1], off[1])
    assert on[2] and off[2]        # (limits[0] == 0: sorted on return although the Rayleigh quotients were not)


@pytest.mark.parametrize("limits", [(0, 1, 2), (2, 1, 2)])
@pytest.mark.parametrize("M", [7, 12])
@pytest.mark.parametrize("grid", ["cubic_18", "triclinic_12x15x18"])
def test_lobpcg_general_complex(monkeypatch, grid, M, limits):
    basis, rhos, X0 = lobpcg_setup(grid, (0.25, 0.0, 0.125))
    on, off = on_and_off(monkeypatch, lambda: three_calls(basis, rhos, X0, M, False, limits, 4, 4), False, general_driver=True)
    assert_same(on[0], off[0])
    assert on[1] < off[1], (on[1], off[1])


@pytest.mark.parametrize("kcoord", [(0.0, 0.0, 0.0), (0.25, 0.0, 0.125)], ids=["gamma_real", "complex"])
def test_lobpcg_block_above_the_small_block_threshold(monkeypatch, kcoord):
    """Si (2,2,2) at Ecut 12, 40 bands: rows x columns exceeds the 65536 elements below which ortho!(X, Y) keeps today's
    placement, so a second round of it writes its projected block to the scratch block (zgemm_to with beta = 1)."""
    basis, rhos, X0 = lobpcg_setup(None, kcoord, (2, 2, 2), 12)
    rows = X0.shape[1] if any(kcoord) else (X0.shape[1] + 1) // 2
    assert rows * 40 > 65536
    on, off = on_and_off(monkeypatch, lambda: three_calls(basis, rhos, X0, 40, True, (3, 2, 3), 32, 32), True)
    assert_same(on[0], off[0])
    assert on[1] < off[1], (on[1], off[1])


# ------------------------------------------------------------------------------------------------------ density
@pytest.mark.parametrize("planes", [True, False], ids=["planes", "no_planes"])
@pytest.mark.parametrize("grid", ["cubic_18", "triclinic_12x15x18"])
def test_density_of_real_symmetric_orbitals(monkeypatch, grid, planes):
    """7 bands (the last pair holds one band), fft_batch 3 (pairs 0-2 and the ragged group of pair 3), weights (2, 2, 2, 2,
    1, 0, 0): nothing is skipped; weights (2, 2, 2, 2, 0, 0, 0) with fft_batch 2: the group of pairs 2 and 3 is all zero
    and the pass skips it.  With planes the block is the one a LOBPCG call returned and the next call starts from them."""
    basis, rhos, X0 = lobpcg_setup(grid, (0.0, 0.0, 0.0))
    lib = basis.lib

    def run():
        out = []
        _, ham = dftk.energy_hamiltonian(basis, None, None, rho=rhos[0])
        r = dftk.lobpcg_hyper(ham[0], X0[:7], prec=dftk.PreconditionerTPA(ham[0]), tol=1e-14, n_conv_check=4, maxiter=2)
        for batch, occ in ((3, [2, 2, 2, 2, 1, 0, 0]), (2, [2, 2, 2, 2, 0, 0, 0])):
            check(lib.dftk_mi_basis_set_fft_batch(basis.handle, batch))
            rho = dftk.compute_density(basis, [r.X], [np.array(occ, dtype=float)], real_symmetric=[True])
            out.append(bits(rho.cpu().numpy()))
        # the skipped group is filled at the start of the next call (planes), from the block itself
        _, ham2 = dftk.energy_hamiltonian(basis, None, None, rho=rhos[1])
        p0 = counter(lib, "dftk_mi_planes_reuse_count")
        r2 = dftk.lobpcg_hyper(ham2[0], r.X, prec=dftk.PreconditionerTPA(ham2[0]), tol=1e-14, n_conv_check=4, maxiter=1,
                               reuse_AX=True)
        assert counter(lib, "dftk_mi_planes_reuse_count") - p0 == (1 if planes else 0)
        out += [bits(r2.λ), bits(r2.X.cpu().numpy())]
        return out
    try:
        on, off = on_and_off(monkeypatch, run, planes)
    finally:
        check(lib.dftk_mi_basis_set_fft_batch(basis.handle, 32))
    assert_same(on, off)
