"""Exact exchange without a GPU: the interaction kernels of dftk.jl_amd/exchange.py (descriptor-only bases, device="cpu"),
the model layer (model_HF, PBE0), the refusals, and the NumPy twin (tests/exx_twin.py) against itself and against closed
forms -- so that the GPU tests compare the device with a reference that has been checked on its own."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
import oracle  # noqa: E402

import exx_twin as twin  # noqa: E402

GAMMA = [[0.0, 0.0, 0.0]]
MADELUNG_SC = 2.8372974794806          # Madelung constant of the simple cubic lattice (unit cube, unit charges)


def si_basis(model=None, kcoords=GAMMA, **kw):
    lat, atoms, pos = dftk.silicon_cell()
    model = dftk.model_HF(lat, atoms, pos) if model is None else model(lat, atoms, pos)
    kg = dftk.ExplicitKpoints(kcoords, [1.0 / len(kcoords)] * len(kcoords))
    return dftk.PlaneWaveBasis(model, 5, kg, fft_size=(18, 18, 18), device="cpu", **kw)


@pytest.fixture(scope="module")
def obasis():
    lat, atoms, pos = oracle.basis.silicon_primitive()
    model = oracle.Model(lat, atoms, pos, terms=("Kinetic",))
    return oracle.PlaneWaveBasis(model, 5, oracle.ExplicitKpoints(GAMMA, [1.0]), fft_size=(18, 18, 18))


# ------------------------------------------------------------------------------------------------------- kernels
def test_probe_charge_is_the_madelung_constant_of_the_simple_cubic_lattice():
    """Coulomb(ProbeCharge()) on a simple cubic cell of edge L = 10 at Ecut = 20: the G = 0 value is the Ewald sum of unit
    Gaussian charges on the lattice without the origin, MADELUNG_SC L^2 - 4 pi alpha with alpha = pi^2 / Ecut, to 1e-8
    relative (NumPy: 277.52849283 against 277.52849261, 8e-10 -- what the reciprocal sum misses beyond the sphere)."""
    L, Ecut = 10.0, 20.0
    Si = dftk.silicon_cell()[1][0]
    model = dftk.Model(L * np.eye(3), [Si], [np.zeros(3)], terms=("Kinetic", dftk.ExactExchange()))
    basis = dftk.PlaneWaveBasis(model, Ecut, dftk.ExplicitKpoints(GAMMA, [1.0]), device="cpu")
    K = basis.terms.exx_kernel.numpy()
    expect = MADELUNG_SC * L ** 2 - 4 * math.pi * (math.pi ** 2 / Ecut)
    assert abs(K[0] - expect) <= 1e-8 * expect, (K[0], expect)
    omodel = oracle.Model(L * np.eye(3), [oracle.ElementPsp("Si", oracle.load_psp_hgh("Si", "lda"))], [np.zeros(3)],
                          terms=("Kinetic",))
    ob = oracle.PlaneWaveBasis(omodel, Ecut, oracle.ExplicitKpoints(GAMMA, [1.0]), fft_size=basis.fft_size)
    Kt = twin.kernel_coulomb_probe_charge(ob)
    assert abs(Kt[0] - expect) <= 1e-8 * expect
    np.testing.assert_allclose(K, Kt, rtol=1e-13)


def test_host_kernels_equal_the_twin_and_their_limits(obasis):
    Omega = obasis.model.unit_cell_volume
    mu, Rcut = 0.31, 2.7
    pairs = [
        (dftk.Coulomb(), twin.kernel_coulomb_probe_charge(obasis)),
        (dftk.Coulomb(dftk.ProbeCharge(alpha=0.8)), twin.kernel_coulomb_probe_charge(obasis, 0.8)),
        (dftk.Coulomb(dftk.ReplaceSingularity(3.5)), twin.kernel_coulomb_replace(obasis, 3.5)),
        (dftk.ShortRangeCoulomb(mu), twin.kernel_short_range(obasis, mu)),
        (dftk.SphericallyTruncatedCoulomb(), twin.kernel_spherically_truncated(obasis)),
        (dftk.SphericallyTruncatedCoulomb(Rcut), twin.kernel_spherically_truncated(obasis, Rcut)),
    ]
    for kernel, expect in pairs:
        basis = si_basis(lambda *a, k=kernel: dftk.model_HF(*a, exx_kernel=k))
        got = basis.terms.exx_kernel.numpy()
        assert np.array_equal(got, dftk.compute_kernel_fourier(kernel, basis).numpy())
        assert got.shape == expect.shape and got.dtype == np.float64
        np.testing.assert_allclose(got, expect, rtol=1e-13, err_msg=repr(kernel))
    # G = 0 values
    assert pairs[2][1][0] == 3.5
    assert pairs[3][1][0] == pytest.approx(math.pi / mu ** 2, rel=1e-15)
    R0 = np.cbrt(3 * Omega / (4 * math.pi))
    assert pairs[4][1][0] == pytest.approx(2 * math.pi * R0 ** 2, rel=1e-15)
    assert pairs[5][1][0] == pytest.approx(2 * math.pi * Rcut ** 2, rel=1e-15)
    # erfc + erf = 1: short range plus the long-range formula is the bare Coulomb kernel off G = 0
    total = twin.kernel_short_range(obasis, mu)[1:] + twin.long_range_formula(obasis, mu)[1:]
    np.testing.assert_allclose(total, twin.kernel_coulomb_replace(obasis, 0.0)[1:], rtol=1e-14)
    # the truncated kernel tends to its G = 0 value: 4 pi / G^2 (1 - cos(R G)) -> 2 pi R^2
    G2 = twin.sphere_G2(obasis)
    small = 1e-6
    assert 4 * math.pi / small * (1 - math.cos(Rcut * math.sqrt(small))) == pytest.approx(2 * math.pi * Rcut ** 2, rel=1e-4)
    assert G2[0] == 0 and np.all(G2[1:] > 0)
    # the scaling factor of the term is folded into the kernel the device sees
    scaled = si_basis(lambda *a: dftk.model_DFT(*a, functionals=dftk.PBE0())).terms.exx_kernel.numpy()
    np.testing.assert_allclose(scaled, 0.25 * pairs[0][1], rtol=1e-13)


# ------------------------------------------------------------------------------------------------------- model
def test_model_hf_and_pbe0():
    lat, atoms, pos = dftk.silicon_cell()
    atomic = ("Kinetic", "AtomicLocal", "AtomicNonlocal", "Ewald", "PspCorrection")
    hf = dftk.model_HF(lat, atoms, pos)
    assert hf.term_types == atomic + ("Hartree", "ExactExchange")
    assert hf.exact_exchange == dftk.ExactExchange(1.0, dftk.Coulomb(dftk.ProbeCharge()))
    sr = dftk.model_HF(lat, atoms, pos, exx_kernel=dftk.ShortRangeCoulomb(0.2))
    assert sr.exact_exchange.kernel == dftk.ShortRangeCoulomb(0.2)
    for kw, a in ((dict(), 0.25), (dict(exx_fraction=0.1), 0.1)):
        m = dftk.model_DFT(lat, atoms, pos, functionals=dftk.PBE0(**kw))
        assert m.term_types == atomic + ("Hartree", "Xc", "ExactExchange")
        assert m.functionals == ("gga_x_pbe", "gga_c_pbe")
        assert m.functional_scales == (1 - a, 1.0)
        assert m.exact_exchange == dftk.ExactExchange(a, dftk.Coulomb())
    k = dftk.SphericallyTruncatedCoulomb()
    assert dftk.model_DFT(lat, atoms, pos, functionals=dftk.PBE0(exx_kernel=k)).exact_exchange.kernel is k
    # models without the term are what they were
    lda = dftk.model_DFT(lat, atoms, pos)
    assert lda.exact_exchange is None and lda.functional_scales == (1.0, 1.0) and "ExactExchange" not in lda.term_types
    temp = dftk.model_HF(lat, atoms, pos, temperature=0.01)
    assert temp.term_types[-2:] == ("ExactExchange", "Entropy")          # (Entropy goes last: standard_models.jl:56-58)


def test_refusals():
    with pytest.raises(ValueError, match="Gamma"):
        si_basis(kcoords=[[0.25, 0.0, 0.0]])
    with pytest.raises(ValueError, match="Gamma"):
        si_basis(kcoords=[[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]])
    with pytest.raises(NotImplementedError, match="gamma_real"):
        si_basis(gamma_real=True)
    assert si_basis().gamma_real is False
    assert si_basis(gamma_real=False).gamma_real is False
    for kernel in (dftk.WignerSeitzTruncatedCoulomb(), dftk.LongRangeCoulomb(), dftk.Coulomb(dftk.VoxelAveraged())):
        with pytest.raises(NotImplementedError, match="exact exchange"):
            si_basis(lambda *a, k=kernel: dftk.model_HF(*a, exx_kernel=k))
    from dftk_jl_amd.exchange import check_gamma_only
    with pytest.raises(ValueError, match="comm_kpts"):
        check_gamma_only(GAMMA, n_ranks_kpts=2)
    with pytest.raises(ValueError, match="comm_pw"):
        check_gamma_only(GAMMA, n_ranks_pw=2)
    lat, atoms, pos = dftk.silicon_cell()
    with pytest.raises(NotImplementedError, match="exact exchange"):
        dftk.plan_planewave_sharded(dftk.model_HF(lat, atoms, pos), 5, 2)
    # a basis without the term keeps its Gamma-real default
    assert si_basis(lambda *a: dftk.model_DFT(*a)).gamma_real is None


# ------------------------------------------------------------------------------------------------------- the twin
@pytest.fixture(scope="module")
def orbitals(obasis):
    n = len(obasis.kpoints[0].mapping)
    rng = np.random.default_rng(5)
    psi = np.linalg.qr(rng.standard_normal((n, 7)) + 1j * rng.standard_normal((n, 7)))[0]
    occ = np.array([2.0, 2.0, 1.3, 0.4, 0.0, 0.0, 0.0])
    return psi, occ, twin.kernel_coulomb_probe_charge(obasis)


def test_twin_operator_is_hermitian_and_negative_semidefinite(obasis, orbitals):
    psi, occ, K = orbitals
    kpt = obasis.kpoints[0]
    Vx = twin.exchange_matrix(obasis, kpt, K, psi[:, :4], occ[:4] / 2)
    assert np.abs(Vx - Vx.conj().T).max() <= 1e-13 * np.abs(Vx).max()
    lam = np.linalg.eigvalsh((Vx + Vx.conj().T) / 2)
    assert lam.max() <= 1e-12 * abs(lam.min()) and lam.min() < 0


def test_twin_energy_is_half_the_occupied_expectation_values(obasis, orbitals):
    psi, occ, K = orbitals
    kpt = obasis.kpoints[0]
    W = twin.exchange_apply(obasis, kpt, K, psi[:, :4], occ[:4] / 2, psi[:, :4])
    half = 0.5 * np.sum(occ[:4] * np.real(np.sum(np.conj(psi[:, :4]) * W, axis=0)))
    E = twin.exchange_energy(obasis, kpt, K, psi[:, :4], occ[:4], 2)
    assert E < 0 and abs(E - half) <= 1e-13 * abs(E)


@pytest.mark.parametrize("extra", [True, False])
def test_twin_ace_reproduces_the_operator_on_its_sketch(obasis, orbitals, extra):
    psi, occ, K = orbitals
    kpt = obasis.kpoints[0]
    a = twin.ace(obasis, kpt, K, psi, occ, 2, sketch_with_extra_orbitals=extra)
    assert a["n_occ"] == 4 and a["n_sketch"] == (7 if extra else 4)
    sk = psi[:, :a["n_sketch"]]
    compressed = -a["xi"] @ (a["xi"].conj().T @ sk)
    cond = np.linalg.cond(a["M"])
    assert np.abs(compressed - a["W"]).max() <= 100 * cond * np.finfo(float).eps * np.abs(a["W"]).max()
    assert abs(a["E"] - twin.exchange_energy(obasis, kpt, K, psi[:, :4], occ[:4], 2)) <= 1e-13 * abs(a["E"])


def test_twin_one_occupied_plane_wave(obasis):
    """phi = e_G0 with weight w: Vx e_G = -w K(G - G0) / Omega e_G, zero where G - G0 is outside the sphere.  No transform
    on the right-hand side: the normalisation and the sphere convention of the twin."""
    kpt = obasis.kpoints[0]
    n = len(kpt.mapping)
    K = twin.kernel_coulomb_probe_charge(obasis)
    row = {tuple(g): i for i, g in enumerate(kpt.G_vectors)}
    i0, w = n // 2, 0.7
    phi = np.zeros((n, 1), dtype=complex)
    phi[i0] = 1.0
    Vx = twin.exchange_matrix(obasis, kpt, K, phi, [w])
    expect = np.zeros(n)
    for i in range(n):
        j = row.get(tuple(kpt.G_vectors[i] - kpt.G_vectors[i0]))
        expect[i] = -w * K[j] / obasis.model.unit_cell_volume if j is not None else 0.0
    assert 0 < np.count_nonzero(expect) < n
    assert np.abs(Vx - np.diag(expect)).max() <= 1e-13 * np.abs(expect).max()


def test_twin_in_double_is_within_a_tenth_of_rtol_of_long_double():
    """What lets tests/test_gpu_exx_kernels.py assert RTOL = 1e-12 on the device: the complex128 twin is within 1e-13 of
    the same loops in long double on every shape of that file (measured 3.8e-16 .. 1.1e-15 relative to max |W|)."""
    worst = 0.0
    for grid in twin.KERNEL_TEST_GRIDS:
        for n_occ in (1, 3, 9):
            for n_bands in (1, 5):
                worst = max(worst, twin.kernel_test_case(grid, n_occ, n_bands)[6])
    print(f"\ntwin complex128 vs long double, worst of the device test's shapes: {worst:.2e}")
    assert np.finfo(np.longdouble).eps < 1e-18          # long double is extended precision here
    assert worst <= twin.RTOL_FFT / 10
