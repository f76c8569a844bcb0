"""DFT+U, the part that needs no GPU: Wigner matrices of the real spherical harmonics, manifolds and their errors, the
``Hubbard`` constructors, the model plumbing, the energy in closed form, the symmetrisation, the refusals that are decided
before the device is touched, and the NumPy twin of tests/hubbard_gen.py against itself (gradient, rotation identity)."""
import itertools
import types

import numpy as np
import pytest

import dftk_jl_amd as dftk
from dftk_jl_amd import hubbard as hub

import hubbard_gen
from test_upf_host import E_QUAD

U = 2.0 ** -52


@pytest.fixture(scope="module")
def psp():
    return hubbard_gen.hubbard_psp()


def si_model(psp, positions=None, **kw):
    lat, _, pos = dftk.silicon_cell()
    Si = dftk.ElementPsp("Si", psp=psp)
    return dftk.model_DFT(lat, [Si, Si], pos if positions is None else positions, functionals=("lda_x", "lda_c_vwn"), **kw), Si


# ------------------------------------------------------------------------------------------------ Wigner matrices
@pytest.mark.parametrize("l", [1, 2])
def test_wigner_reference_cases(l):
    """the four cases of the reference's test, as mathematics"""
    d = 2 * l + 1
    assert np.allclose(dftk.wigner_d_matrix(l, np.eye(3)), np.eye(d), atol=1e-13)
    assert np.allclose(dftk.wigner_d_matrix(l, -np.eye(3)), (-1) ** l * np.eye(d), atol=1e-13)
    D = dftk.wigner_d_matrix(l, np.diag([1.0, -1.0, -1.0]))
    # real harmonics in the order m = -l .. l: l = 1 is (y, z, x); l = 2 is (xy, yz, 2z^2 - x^2 - y^2, xz, x^2 - y^2)
    want = {1: np.diag([-1.0, -1.0, 1.0]), 2: np.diag([-1.0, 1.0, 1.0, -1.0, 1.0])}[l]
    assert np.allclose(D, want, atol=1e-13)
    swap = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    D = dftk.wigner_d_matrix(l, swap)
    if l == 1:                                # y <-> x, z stays
        want = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    else:                                     # xy stays, yz <-> xz, x^2 - y^2 changes sign
        want = np.zeros((5, 5))
        want[0, 0] = want[2, 2] = 1.0
        want[1, 3] = want[3, 1] = 1.0
        want[4, 4] = -1.0
    assert np.allclose(D, want, atol=1e-13)
    assert np.array_equal(dftk.wigner_d_matrix(0, swap), np.ones((1, 1)))


def cubic_group():
    ops = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product([1.0, -1.0], repeat=3):
            W = np.zeros((3, 3))
            for i, (p, s) in enumerate(zip(perm, signs)):
                W[i, p] = s
            ops.append(W)
    return ops


@pytest.mark.parametrize("l", [0, 1, 2, 3])
def test_wigner_is_an_orthogonal_representation_of_the_cubic_group(l):
    ops = cubic_group()
    assert len(ops) == 48
    Ds = [dftk.wigner_d_matrix(l, W) for W in ops]
    worst_o = max(np.max(np.abs(D @ D.T - np.eye(2 * l + 1))) for D in Ds)
    # Y(W1 W2 r) = D(W1) Y(W2 r) = D(W1) D(W2) Y(r)
    worst_p = max(np.max(np.abs(dftk.wigner_d_matrix(l, W1 @ W2) - D1 @ D2))
                  for (W1, D1), (W2, D2) in itertools.product(list(zip(ops, Ds)), repeat=2))
    print(f"l = {l}: orthogonality {worst_o:.1e}, products {worst_p:.1e}")
    assert worst_o <= 1e-12 and worst_p <= 1e-12
    # against the twin's matrices (seeded random directions, its own harmonics)
    assert max(np.max(np.abs(D - hubbard_gen.twin_wigner(l, W))) for W, D in zip(ops, Ds)) <= 1e-11


def test_wigner_beyond_l3_is_refused():
    with pytest.raises(NotImplementedError):
        dftk.wigner_d_matrix(4, np.eye(3))


# ------------------------------------------------------------------------------------------------ manifolds
def test_manifold_spellings_resolve_identically(psp):
    model, Si = si_model(psp)
    spellings = [dftk.OrbitalManifold(Si, "3D"), dftk.OrbitalManifold("Si", "3D"), dftk.OrbitalManifold([0, 1], "3D"),
                 dftk.OrbitalManifold(Si, (2, 1)), dftk.OrbitalManifold("Si", dict(l=2, i=1)),
                 dftk.OrbitalManifold([0, 1], dict(l=2, i=1))]
    resolved = [dftk.resolve_hubbard_manifold(m, model) for m in spellings]
    for r in resolved:
        assert r.psp is psp and r.iatoms == (0, 1) and (r.l, r.i) == (2, 1)
    assert dftk.resolve_hubbard_manifold(dftk.OrbitalManifold("Si", "3P"), model).l == 1
    assert dftk.OrbitalManifold(Si, "3D") == dftk.OrbitalManifold("Si", "3D")


def test_manifold_errors(psp):
    model, Si = si_model(psp)
    with pytest.raises(ValueError, match="no atoms"):
        dftk.resolve_hubbard_manifold(dftk.OrbitalManifold("Ni", "3D"), model)
    with pytest.raises(ValueError, match="no atoms"):
        dftk.resolve_hubbard_manifold(dftk.OrbitalManifold([], "3D"), model)
    with pytest.raises(ValueError, match="3F"):
        dftk.resolve_hubbard_manifold(dftk.OrbitalManifold("Si", "3F"), model)
    # two pseudopotentials in one manifold
    lat, _, pos = dftk.silicon_cell()
    other = dftk.ElementPsp("Si", psp=hubbard_gen.hubbard_psp(("3S", "3P")))
    mixed = dftk.model_DFT(lat, [Si, other], pos)
    with pytest.raises(ValueError, match="multiple psps"):
        dftk.resolve_hubbard_manifold(dftk.OrbitalManifold([0, 1], "3P"), mixed)
    # an atom without a pseudopotential
    bare = types.SimpleNamespace(atoms=[Si, types.SimpleNamespace(symbol="H")], positions=pos,
                                 symmetries=[dftk.symmetry.identity()])
    with pytest.raises(ValueError, match="must have a psp"):
        dftk.resolve_hubbard_manifold(dftk.OrbitalManifold([0, 1], "3P"), bare)
    # the inversion about the bond centre exchanges the two atoms of the diamond cell: one atom alone is no atom group
    sym, _ = si_model(psp, symmetries=True)
    assert len(sym.symmetries) == 48
    with pytest.raises(ValueError, match="Inconsistency between orbital manifold and model symmetries"):
        dftk.resolve_hubbard_manifold(dftk.OrbitalManifold([0], "3P"), sym)
    assert dftk.resolve_hubbard_manifold(dftk.OrbitalManifold([0, 1], "3P"), sym).iatoms == (0, 1)
    # l > 3
    with pytest.raises(NotImplementedError, match="l = 4"):
        dftk.resolve_hubbard_manifold(dftk.OrbitalManifold("Si", (4, 1)), model)


def test_hubbard_constructors():
    a, b = dftk.OrbitalManifold("Si", "3P"), dftk.OrbitalManifold([0], (2, 1))
    h = dftk.Hubbard((a, 0.1), (b, 0.2))
    assert h.manifolds == (a, b) and h.U == (0.1, 0.2)
    g = dftk.Hubbard([a, b], [0.1, 0.2])
    assert g.manifolds == h.manifolds and g.U == h.U
    assert dftk.Hubbard((a, 0.3)).U == (0.3,)
    assert dftk.Hubbard().manifolds == () and dftk.Hubbard().U == () and dftk.Hubbard([], []).U == ()
    with pytest.raises(ValueError, match="must match"):
        dftk.Hubbard([a, b], [0.1])
    with pytest.raises(TypeError):
        dftk.Hubbard(a, 0.1)


def test_model_keeps_the_term_apart(psp):
    h = dftk.Hubbard((dftk.OrbitalManifold("Si", "3P"), 0.1))
    model, _ = si_model(psp, extra_terms=[h])
    assert model.hubbard is h and model.term_types[-1] == "Hubbard" and model.term_types.count("Hubbard") == 1
    assert "Hartree" in model.term_types and "Xc" in model.term_types
    lat, atoms, pos = dftk.silicon_cell()
    atomic = dftk.model_atomic(lat, atoms, pos, extra_terms=[h])
    assert atomic.hubbard is h and atomic.term_types[-1] == "Hubbard"
    assert si_model(psp)[0].hubbard is None
    with pytest.raises(ValueError, match="more than one Hubbard"):
        si_model(psp, extra_terms=[h, dftk.Hubbard()])
    with pytest.raises(NotImplementedError, match="ExactExchange"):
        dftk.model_atomic(lat, atoms, pos, extra_terms=["Hartree", dftk.ExactExchange(), h])
    with pytest.raises(NotImplementedError, match="ExactExchange"):
        dftk.model_DFT(lat, atoms, pos, functionals=dftk.PBE0(), extra_terms=[h])
    d = dftk.model_to_dict(model)
    assert "Hubbard" in d["terms"] and d["hubbard"] == {"manifolds": [{"atoms": "Si", "projectors": "3P"}], "U": [0.1]}
    two = dftk.Hubbard((dftk.OrbitalManifold([0, 1], (2, 1)), 0.2), (dftk.OrbitalManifold("Si", "3P"), 0.3))
    assert dftk.model_to_dict(si_model(psp, extra_terms=[two])[0])["hubbard"] == {
        "manifolds": [{"atoms": [0, 1], "projectors": {"l": 2, "i": 1}}, {"atoms": "Si", "projectors": "3P"}], "U": [0.2, 0.3]}
    assert "hubbard" not in dftk.model_to_dict(si_model(psp)[0])


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_entry_points_without_a_hubbard_term_refuse(psp):
    h = dftk.Hubbard((dftk.OrbitalManifold("Si", "3P"), 0.1))
    model, _ = si_model(psp, extra_terms=[h])
    basis = types.SimpleNamespace(model=model, comm_pw=types.SimpleNamespace(size=1), comm_kpts=types.SimpleNamespace(size=1))
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.compute_forces(basis, None, None)
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.compute_forces_cart(basis, None, None)
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.compute_forces_term("AtomicLocal", basis, None, None)
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.compute_stresses_cart(basis, None, None)
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.compute_dynmat(basis, None, None)
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.apply_kernel(basis, None)
    ham = [types.SimpleNamespace(basis=basis)]
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.apply_chi0(ham, None, None, 0.0, None, None)
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.solve_OmegaPlusK_split(dict(basis=basis, ham=ham, psi=None, occupation=None, eF=0.0, eigenvalues=None,
                                         occupation_threshold=1e-6, rho=None), None)
    for which in ("comm_pw", "comm_kpts"):
        sharded = types.SimpleNamespace(model=model, comm_pw=types.SimpleNamespace(size=1),
                                        comm_kpts=types.SimpleNamespace(size=1))
        setattr(sharded, which, types.SimpleNamespace(size=2))
        with pytest.raises(NotImplementedError, match="sharded"):
            hub.hubbard_term(sharded)
        with pytest.raises(NotImplementedError, match="sharded"):
            dftk.compute_hubbard_n(sharded, None, None)


# ------------------------------------------------------------------------------------------------ energy, symmetrisation
def hand_term(ls, n_atoms, Us):
    term = hub.HubbardTerm()
    term.manifolds = [hub.ResolvedOrbitalManifold(None, tuple(range(n_atoms)), l, 1) for l in ls]
    term.U = list(Us)
    return term


def test_energy_of_a_diagonal_n_in_closed_form():
    rng = np.random.default_rng(3)
    term = hand_term([1, 2], 2, [0.3, 0.7])
    ns, want = [], 0.0
    for l, u in zip([1, 2], [0.3, 0.7]):
        d = 2 * l + 1
        n = np.zeros((2, 2, 2, d, d), dtype=complex)
        for s in range(2):
            for ia in range(2):
                nu = rng.random(d)
                n[s, ia, ia] = np.diag(nu)
                want += 1 * 0.5 * u * float(np.sum(nu * (1 - nu)))
        n[0, 0, 1] = rng.standard_normal((d, d))       # (cross-atom blocks do not enter)
        ns.append(n)
    got = hub.hubbard_energy(term, ns, 1)
    assert abs(got - want) <= 8 * U * abs(want)
    assert abs(hubbard_gen.twin_energy([0.3, 0.7], ns, 1) - want) <= 8 * U * abs(want)
    # integer occupations cost nothing, half filling costs U / 8 per orbital
    full = [np.zeros((1, 1, 1, 3, 3), dtype=complex)]
    full[0][0, 0, 0] = np.diag([1.0, 0.0, 1.0])
    assert hub.hubbard_energy(hand_term([1], 1, [0.5]), full, 2) == 0.0
    full[0][0, 0, 0] = np.eye(3) / 2
    assert hub.hubbard_energy(hand_term([1], 1, [0.5]), full, 2) == 2 * 0.5 * 0.5 * 3 * 0.25


def random_hermitian_n(rng, n_spin, n_atoms, d):
    n = np.zeros((n_spin, n_atoms, n_atoms, d, d), dtype=complex)
    for s in range(n_spin):
        for i in range(n_atoms):
            for j in range(n_atoms):
                a = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
                n[s, i, j] = a + a.conj().T if i == j else a
    return n


@pytest.mark.parametrize("l", [1, 2])
def test_symmetrising_twice_is_symmetrising_once(psp, l):
    model, _ = si_model(psp, symmetries=True)
    man = dftk.resolve_hubbard_manifold(dftk.OrbitalManifold("Si", (l, 1)), model)
    n = random_hermitian_n(np.random.default_rng(l), 2, 2, 2 * l + 1)
    once = dftk.symmetrize_hubbard_n(model, man, n, model.symmetries)
    twice = dftk.symmetrize_hubbard_n(model, man, once, model.symmetries)
    scale = np.max(np.abs(n))
    print(f"l = {l}: |S S n - S n| = {np.max(np.abs(twice - once)):.1e}, |S n - n| = {np.max(np.abs(once - n)):.1e}")
    assert np.max(np.abs(twice - once)) <= 1e-12 * scale and np.max(np.abs(once - n)) > 0.1 * scale
    assert np.all(once[:, 0, 1] == 0) and np.all(once[:, 1, 0] == 0)          # cross-atom blocks stay zero
    for s in range(2):
        for ia in range(2):
            assert np.max(np.abs(once[s, ia, ia] - once[s, ia, ia].conj().T)) <= 1e-13 * scale
    # the identity alone keeps the atom-diagonal blocks
    same = dftk.symmetrize_hubbard_n(model, man, n, [dftk.symmetry.identity()])
    assert max(np.max(np.abs(same[:, ia, ia] - n[:, ia, ia])) for ia in range(2)) <= 1e-13 * scale
    # the twin (its own Wigner matrices and preimage search)
    tw = hubbard_gen.twin_symmetrize(model.lattice, [model.positions[i] for i in man.iatoms], l, n, model.symmetries)
    assert np.max(np.abs(tw - once)) <= 1e-11 * scale


# ------------------------------------------------------------------------------------------------ the twin against itself
def random_setup(rng, n_G=40, n_bands=5, n_k=2):
    """two "atoms" with (3S, 3P, 3D) each as random orthonormal columns, random orthonormal bands"""
    n_proj = 18
    Phi = [np.linalg.qr(rng.standard_normal((n_G, n_proj)) + 1j * rng.standard_normal((n_G, n_proj)))[0] for _ in range(n_k)]
    psi = [np.linalg.qr(rng.standard_normal((n_G, n_bands)) + 1j * rng.standard_normal((n_G, n_bands)))[0]
           for _ in range(n_k)]
    occ = [np.array([2.0, 2.0, 1.3, 0.4, 0.0])] * n_k
    return Phi, psi, occ, [0.25, 0.75][:n_k], [1] * n_k


def test_twin_gradient_against_central_differences():
    """E is a quartic polynomial of the orbitals, so (E(psi + h d) - E(psi - h d)) / 2h = E' + c h^2 exactly: the error
    falls by 4 from h to h / 2, and a third of the difference of the two quotients is the error of the second.  The test
    allows that estimate (times 1.5 for its own rounding) plus the rounding of the quotient, 8 x 2^-52 |E| / (h / 2)."""
    rng = np.random.default_rng(11)
    Phi, psi, occ, kw, spins = random_setup(rng)
    cols = hubbard_gen.manifold_columns(2, [((0, 1), "3P"), ((0, 1), "3D")])
    Us = [0.4, 0.9]

    def energy(ps):
        return hubbard_gen.twin_energy(Us, hubbard_gen.twin_hubbard_n(Phi, ps, occ, kw, spins, 2, 1, cols), 2)

    n = hubbard_gen.twin_hubbard_n(Phi, psi, occ, kw, spins, 2, 1, cols)
    grad = hubbard_gen.twin_gradient(Phi, psi, occ, kw, spins, Us, n, cols)
    delta = [rng.standard_normal(p.shape) + 1j * rng.standard_normal(p.shape) for p in psi]
    analytic = 2 * sum(float(np.real(np.vdot(d, g))) for d, g in zip(delta, grad))
    quotients = []
    for h in (1e-2, 5e-3):
        plus = energy([p + h * d for p, d in zip(psi, delta)])
        minus = energy([p - h * d for p, d in zip(psi, delta)])
        quotients.append((plus - minus) / (2 * h))
    err = [abs(q - analytic) for q in quotients]
    estimate = abs(quotients[0] - quotients[1]) / 3
    rounding = 8 * U * abs(energy(psi)) / 5e-3
    print(f"analytic {analytic:.12f}; errors {err[0]:.3e}, {err[1]:.3e} (ratio {err[0] / err[1]:.3f}); estimate {estimate:.3e}")
    assert 3.9 <= err[0] / err[1] <= 4.1
    assert err[1] <= 1.5 * estimate + rounding


def test_rotation_identity_with_a_degenerate_spectrum():
    """Phi D Phi' = (Phi V) diag(U / 2 (1 - 2 nu)) (Phi V)' for n = V nu V', also when nu is degenerate (any orthonormal
    basis of an eigenspace serves)."""
    rng = np.random.default_rng(5)
    Phi = np.linalg.qr(rng.standard_normal((60, 5)) + 1j * rng.standard_normal((60, 5)))[0]
    Q = np.linalg.qr(rng.standard_normal((5, 5)) + 1j * rng.standard_normal((5, 5)))[0]
    n = Q @ np.diag([0.2, 0.2, 0.2, 0.9, 0.9]) @ Q.conj().T
    u = 0.37
    dense = Phi @ (0.5 * u * (np.eye(5) - 2 * n)) @ Phi.conj().T
    nu, V = np.linalg.eigh((n + n.conj().T) / 2)
    rot = Phi @ V
    rotated = rot @ np.diag(0.5 * u * (1 - 2 * nu)) @ rot.conj().T
    err = np.max(np.abs(dense - rotated))
    print(f"rotation identity: {err:.1e}")
    # both sides are products of five matrices with entries below 1 and inner dimension 5
    assert err <= 64 * 5 * U * np.max(np.abs(dense)) + 64 * U * u


def test_generated_file_has_the_d_channel(psp):
    assert psp.lmax == 2 and psp.find_pswfc("3D") == (2, 1) and psp.count_n_pswfc() == 9
    assert psp.count_n_proj_radial(2) == 0


def test_d_channel_transform_against_its_closed_form(psp):
    """the host's weighted sum of the 3D channel against 4 pi sqrt(pi / 2) a^7 exp(-q^2 a^2 / 2), within E_QUAD of
    tests/test_upf_host.py times the channel's largest value: the d channel may use the orbital bounds of
    tests/test_gpu_bands.py"""
    from dftk_jl_amd import psp_upf
    q = np.concatenate([[0.0, 1e-8, 1e-3], np.linspace(0.05, 12.0, 240)])
    for label in hubbard_gen.LABELS:
        l, i = psp.find_pswfc(label)
        want = hubbard_gen.closed_form(label)(q)
        err = np.max(np.abs(psp_upf.eval_psp_pswfc_fourier_upf(psp, i, l, q) - want)) / np.max(np.abs(want))
        print(f"{label}: host transform against the closed form {err:.2e}")
        assert err <= E_QUAD
