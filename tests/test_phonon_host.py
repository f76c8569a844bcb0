"""Host side of the phonon layer (dftk.jl_amd/phonon.py, ``dynmat_ewald`` of terms.py): no GPU needed.

``dynmat_ewald`` is checked against central differences of ``energy_forces_ewald`` (a pre-existing entry point) at steps h
and h / 2.  The yardstick's own error is estimated without the new code as |FD(h) - FD(h / 2)|: pure truncation makes the
error of FD(h / 2) a third of that, and the closed form must agree with FD(h / 2) to within that estimate.  The symmetry and
the acoustic sum rule are exact in exact arithmetic: their bound is rounding only, a multiple of eps times the largest
entry."""
import numpy as np
import pytest

import dftk_jl_amd as dftk

EPS = np.finfo(float).eps

# triclinic cell, three atoms with unequal charges at general positions
LATTICE = np.array([[7.1, 0.6, -0.4], [0.3, 6.2, 0.9], [-0.5, 0.7, 8.3]]).T
CHARGES = [1.0, 4.0, 3.0]
POSITIONS = np.array([[0.11, 0.23, 0.37], [0.58, 0.41, 0.09], [0.83, 0.77, 0.62]])


@pytest.fixture(scope="module")
def ewald():
    return dftk.dynmat_ewald(LATTICE, CHARGES, POSITIONS)


def _fd(h):
    out = np.zeros((3, 3, 3, 3))
    for s in range(3):
        for al in range(3):
            d = np.zeros((3, 3))
            d[s, al] = h
            Fp = dftk.energy_forces_ewald(LATTICE, CHARGES, POSITIONS + d)[1]
            Fm = dftk.energy_forces_ewald(LATTICE, CHARGES, POSITIONS - d)[1]
            out[:, :, al, s] = -((Fp - Fm) / (2 * h)).T
    return out


def test_dynmat_ewald_against_central_differences_of_the_forces(ewald):
    assert ewald.shape == (3, 3, 3, 3) and ewald.dtype == np.float64
    fd1, fd2 = _fd(1e-3), _fd(5e-4)
    yard = np.abs(fd1 - fd2).max()                 # the yardstick's own error estimate, without the new code
    e1, e2 = np.abs(ewald - fd1).max(), np.abs(ewald - fd2).max()
    print(f"\ndynmat_ewald: |D| max {np.abs(ewald).max():.3e}, err h=1e-3 {e1:.3e}, h=5e-4 {e2:.3e} (ratio {e1 / e2:.2f}), "
          f"|FD(h) - FD(h/2)| {yard:.3e}")
    assert 2.0 < e1 / e2 < 5.0                     # the reference is not drowned in noise
    assert e2 <= yard


def test_dynmat_ewald_is_symmetric_and_obeys_the_acoustic_sum_rule(ewald):
    M = ewald.transpose(1, 0, 3, 2).reshape(9, 9)
    scale = np.abs(M).max()
    # exact in exact arithmetic: the bound is rounding of sums of ~1e4 terms of that size
    assert np.abs(M - M.T).max() <= 1e3 * EPS * scale
    assert np.abs(ewald.sum(axis=1)).max() <= 1e3 * EPS * scale
    assert np.abs(ewald.sum(axis=3)).max() <= 1e3 * EPS * scale


def test_dynmat_ewald_without_atoms_and_with_given_eta(ewald):
    assert dftk.dynmat_ewald(LATTICE, [], []).shape == (3, 0, 3, 0)
    other = dftk.dynmat_ewald(LATTICE, CHARGES, POSITIONS, eta=0.9)      # the energy does not depend on eta
    assert np.abs(other - ewald).max() <= 1e-10 * np.abs(ewald).max()


def test_dynmat_red_to_cart():
    rng = np.random.default_rng(5)
    D = rng.standard_normal((3, 2, 3, 2))
    got = dftk.dynmat_red_to_cart(LATTICE, D)
    # E(u_cart) = 1/2 u_cart' D_cart u_cart with u_red = inv(L) u_cart
    u = rng.standard_normal((2, 3))
    ured = u @ np.linalg.inv(LATTICE).T
    e_red = np.einsum("tb,btas,sa->", ured, D, ured)
    e_cart = np.einsum("tb,btas,sa->", u, got, u)
    assert abs(e_red - e_cart) <= 1e-12 * abs(e_red)
    assert np.allclose(dftk.dynmat_red_to_cart(np.eye(3), D), D, rtol=0, atol=0)


def test_mass_matrix():
    from dftk_jl_amd.psp import AMU_IN_ELECTRON_MASSES
    lat, atoms, pos = dftk.silicon_cell()
    M = dftk.mass_matrix(dftk.model_DFT(lat, atoms, pos))
    assert M.shape == (6, 6) and np.count_nonzero(M - np.diag(np.diag(M))) == 0
    assert np.allclose(np.diag(M), 28.085 * AMU_IN_ELECTRON_MASSES, rtol=1e-12)
    assert atoms[0].mass == pytest.approx(28.085 * 1822.888486209, rel=1e-12)
    C_ = dftk.ElementPsp("C", dftk.load_psp("C", "lda"), mass=5.0)
    assert np.array_equal(np.diag(dftk.mass_matrix([atoms[0], C_])), [atoms[0].mass] * 3 + [5.0] * 3)
    assert np.array_equal(np.diag(dftk.mass_matrix([atoms[0], C_], masses={"Si": 2.0})), [2.0] * 3 + [5.0] * 3)
    assert np.array_equal(np.diag(dftk.mass_matrix([atoms[0], C_], masses=[1.0, 3.0])), [1.0] * 3 + [3.0] * 3)
    with pytest.raises(ValueError):
        dftk.mass_matrix(atoms, masses=[1.0])
    with pytest.raises(ValueError):
        dftk.mass_matrix(atoms, masses=[1.0, -1.0])


def test_phonon_modes_of_two_masses_on_a_spring():
    """E = kappa / 2 |u_1 - u_2|^2: three zero modes and a triply degenerate sqrt(kappa (1 / m1 + 1 / m2))."""
    kappa, m1, m2 = 0.37, 3.0, 11.0
    D = np.zeros((3, 2, 3, 2))
    for a in range(3):
        D[a, 0, a, 0] = D[a, 1, a, 1] = kappa
        D[a, 0, a, 1] = D[a, 1, a, 0] = -kappa
    lat, atoms, pos = dftk.silicon_cell()
    basis = dftk.PlaneWaveBasis(dftk.model_DFT(np.eye(3) * 9.0, atoms, pos), 3, device="cpu", build_terms=False)
    # (D above is Cartesian: with the lattice 9 I the reduced matrix is 81 D)
    res = dftk.phonon_modes(basis, dynmat=81.0 * D, masses=[m1, m2])
    assert set(res) == {"mass_matrix", "frequencies", "dynmat", "dynmat_cart", "vectors", "vectors_cart"}
    assert np.allclose(res["dynmat_cart"], D, rtol=1e-14, atol=0)
    w = res["frequencies"]
    omega = np.sqrt(kappa * (1 / m1 + 1 / m2))
    assert np.abs(w[:3]).max() <= 1e-7 and np.allclose(w[3:], omega, rtol=1e-12)    # sqrt of an eigenvalue of size eps
    Dm = D.transpose(1, 0, 3, 2).reshape(6, 6)
    M, v = res["mass_matrix"], res["vectors_cart"]
    assert np.abs(Dm @ v - M @ v * (np.sign(w) * w * w)[None, :]).max() <= 1e-14
    assert np.allclose(v.T @ M @ v, np.eye(6), atol=1e-13)
    assert np.allclose(res["vectors"] * 9.0, v, rtol=1e-14)
    # a negative eigenvalue gives a negative frequency
    assert np.allclose(dftk.phonon_modes(basis, dynmat=-81.0 * D, masses=[m1, m2])["frequencies"][:3], -omega, rtol=1e-12)


def _cpu_basis(**kw):
    lat, atoms, pos = dftk.silicon_cell()
    model_kw = {k: kw.pop(k) for k in ("symmetries", "magnetic_moments") if k in kw}
    model = kw.pop("model", None) or dftk.model_DFT(lat, atoms, pos, **model_kw)
    return dftk.PlaneWaveBasis(model, 3, kw.pop("kgrid", dftk.MonkhorstPack((1, 1, 1))), device="cpu", build_terms=False, **kw)


def test_out_of_scope_requests_are_refused():
    plain = _cpu_basis()
    for call in (lambda b, **kw: dftk.compute_dynmat(b, None, None, **kw),
                 lambda b, **kw: dftk.compute_delta_H_psi_alpha_s(b, None, 0, 0, **kw),
                 lambda b, **kw: dftk.compute_dynmat_term("Ewald", b, None, None, **kw)):
        with pytest.raises(NotImplementedError, match="q != 0"):
            call(plain, q=[0.5, 0, 0])
        with pytest.raises(NotImplementedError, match="collinear"):
            call(_cpu_basis(magnetic_moments=[1, -1]))
        with pytest.raises(ValueError, match="symmetries=False"):
            call(_cpu_basis(symmetries=True, kgrid=dftk.MonkhorstPack((2, 2, 2))))
        lat, atoms, pos = dftk.silicon_cell()
        with pytest.raises(NotImplementedError, match="exact exchange"):
            call(_cpu_basis(model=dftk.model_HF(lat, atoms, pos)))

        class Two:
            size, rank = 2, 0
        sharded = _cpu_basis()
        sharded.comm_pw = Two()
        with pytest.raises(NotImplementedError, match="comm_pw"):
            call(sharded)
        spread = _cpu_basis()
        spread.comm_kpts = Two()
        with pytest.raises(NotImplementedError, match="comm_kpts"):
            call(spread)
    # q = 0 given explicitly is in scope, and a basis without a device has no hot path
    assert dftk.compute_dynmat_term("Ewald", plain, None, None, q=[0, 0, 0]).shape == (3, 2, 3, 2)
    assert dftk.compute_dynmat_term("Kinetic", plain, None, None) is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dftk.compute_dynmat(plain, None, None)
