"""Cells with several species on the device: the set-up kernels (per-species tables of dftk_mi_atomic_superposition and
dftk_mi_build_projectors_hgh), H, and both force entry points against the oracle or the NumPy restatements of
test_gpu_forces.py, on a sheared seven-atom cell whose species groups are interleaved in ``model.atoms`` -- Si, C and Fe
from the table, a synthetic "Si" with every tabulated HGH channel (grouped apart from Si by its identifier) and a
synthetic species without projectors; then the species-group permutation of the forces, term-wise finite differences
for one atom of every species (the reference's "Forces term-wise TiO2", test/forces.jl:103, in spirit), and
zincblende SiC: SCF against the oracle, forces against the SCF energy, and the 24 operations of its symmetry group."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import psp as lpsp  # noqa: E402

import oracle  # noqa: E402
from oracle import psp as opsp  # noqa: E402

from test_gpu_forces import _numpy_local, _numpy_nonlocal  # noqa: E402
from test_gpu_kernels import Basis, KBlock, relerr  # noqa: E402
from test_hgh_channels import synthetic_library_psp, synthetic_oracle_psp  # noqa: E402

FUN = ("lda_x", "lda_c_vwn")
RTOL = 1e-12
LATTICE = np.array([[7.4, 0.9, -0.6], [0.4, 6.9, 1.1], [-0.7, 0.5, 7.8]])     # columns: sheared, non-orthogonal
POSITIONS = [np.array(p) for p in ([0.02, 0.03, 0.05], [0.27, 0.21, 0.09], [0.51, 0.46, 0.13], [0.77, 0.69, 0.33],
                                   [0.14, 0.62, 0.58], [0.43, 0.88, 0.71], [0.69, 0.31, 0.86])]
SPECIES = ["Si", "X", "C", "Fe", "H", "Si", "X"]       # groups Si {0, 5}, X {1, 6}, C {2}, Fe {3}, H {4}
KCOORDS, KWEIGHTS = [[0.0, 0.0, 0.0], [0.23, -0.31, 0.17]], [0.5, 0.5]
# (33 valence electrons: a temperature in both models, which nothing below depends on)
# an H-like local-only species: one l = 0 channel without projectors (owns no column of P)
BARE = dict(Zion=1, rloc=0.26, cloc=[-3.9, 0.61], rp=[0.0])


def library_atoms():
    el = {"Si": dftk.ElementPsp("Si", lpsp.load_psp("Si", "lda")), "C": dftk.ElementPsp("C", lpsp.load_psp("C", "lda")),
          "Fe": dftk.ElementPsp("Fe", lpsp.load_psp("Fe", "lda")), "X": dftk.ElementPsp("Si", synthetic_library_psp()),
          "H": dftk.ElementPsp("H", lpsp._psp(BARE["Zion"], BARE["rloc"], BARE["cloc"], BARE["rp"], [[]],
                                              identifier="synthetic/h-local-only"))}
    return [el[s] for s in SPECIES]


def oracle_atoms():
    el = {s: oracle.ElementPsp(s, oracle.load_psp_hgh(s, "lda")) for s in ("Si", "C", "Fe")}
    el["X"] = oracle.ElementPsp("Si", synthetic_oracle_psp())
    el["H"] = oracle.ElementPsp("H", opsp.make_psp(BARE["Zion"], BARE["rloc"], BARE["cloc"], BARE["rp"],
                                                    [np.zeros((0, 0))], identifier="synthetic/h-local-only"))
    return [el[s] for s in SPECIES]


def library_basis(atoms=None, positions=None, fft_size=None, Ecut=8):
    model = dftk.model_DFT(LATTICE, library_atoms() if atoms is None else atoms,
                           POSITIONS if positions is None else positions, functionals=FUN, symmetries=False,
                           temperature=0.01)
    # (complex blocks at Gamma too: the random orbitals below are not real-symmetric)
    return dftk.PlaneWaveBasis(model, Ecut, dftk.ExplicitKpoints(KCOORDS, KWEIGHTS), fft_size=fft_size, device="cuda:0",
                               gamma_real=False)


@pytest.fixture(scope="module")
def cell():
    basis = library_basis()
    omodel = oracle.model_DFT(LATTICE, oracle_atoms(), POSITIONS, functionals=FUN, temperature=0.01)
    ob = oracle.PlaneWaveBasis(omodel, 8, oracle.ExplicitKpoints(KCOORDS, KWEIGHTS), fft_size=basis.fft_size)
    return basis, ob


@pytest.fixture(scope="module")
def state(cell):
    """Random orthonormal orbitals, random occupations, a perturbed guess density."""
    basis, _ = cell
    rng = np.random.default_rng(17)
    psi, occ = [], []
    for kpt in basis.kpoints:
        A = rng.standard_normal((kpt.n_G, 6)) + 1j * rng.standard_normal((kpt.n_G, 6))
        psi.append(torch.from_numpy(np.ascontiguousarray(np.linalg.qr(A)[0].T)).to("cuda:0"))
        occ.append(rng.uniform(0.1, 2.0, 6))
    g = torch.Generator(device="cuda:0").manual_seed(5)
    rho = dftk.guess_density(basis) * (1 + 0.1 * torch.rand(basis.fft_size[::-1], dtype=torch.float64, device="cuda:0",
                                                            generator=g))
    return psi, occ, rho


def test_groups_are_interleaved_and_split_by_identifier(cell):
    basis, ob = cell
    assert basis.model.atom_groups == ob.model.atom_groups == [[0, 5], [1, 6], [2], [3], [4]]
    n_p = [el.psp.count_n_proj() for el in basis.model.atoms]
    assert n_p == [5, 29, 1, 14, 0, 5, 29]


# ------------------------------------------------------------------------------------------ set-up and H vs the oracle
def _close(got, ref, rtol=RTOL):
    return np.max(np.abs(got - ref)) <= rtol * np.max(np.abs(ref))


def test_setup_matches_oracle(cell, monkeypatch):
    basis, ob = cell
    assert _close(basis.terms.V_loc.cpu().numpy(), ob.terms.V_loc)
    assert _close(dftk.guess_density(basis).cpu().numpy(), oracle.guess_density(ob))
    np.testing.assert_array_equal(basis.terms.D, ob.terms.D)
    for ik, kpt in enumerate(basis.kpoints):
        assert np.array_equal(kpt.mapping, ob.kpoints[ik].mapping)
        P, Po = basis.terms.P[ik].cpu().numpy().T, ob.terms.P[ik]
        assert P.shape == Po.shape == (kpt.n_G, 83)
        for c in range(P.shape[1]):
            assert _close(P[:, c], Po[:, c]), (ik, c)
    # the torch construction of the same objects (DFTK_MI_TORCH_SETUP=1) against the library calls
    monkeypatch.setenv("DFTK_MI_TORCH_SETUP", "1")
    twin = library_basis()
    g_twin = dftk.guess_density(twin)
    monkeypatch.delenv("DFTK_MI_TORCH_SETUP")
    assert _close(basis.terms.V_loc.cpu().numpy(), twin.terms.V_loc.cpu().numpy())
    assert _close(dftk.guess_density(basis).cpu().numpy(), g_twin.cpu().numpy())
    for ik in range(len(basis.kpoints)):
        assert float((basis.terms.P[ik] - twin.terms.P[ik]).abs().max()) < 1e-13 * float(twin.terms.P[ik].abs().max())


def test_apply_H_parts_match_oracle(cell):
    """The library-built P and D of the cell in dftk_mi_apply_H_parts (1 local, 2 kinetic, 4 nonlocal, 7 all) against
    the oracle's Hamiltonian blocks, as test_apply_H_vs_oracle."""
    basis, ob = cell
    lib = basis.lib
    rng = np.random.default_rng(23)
    nx, ny, nz = basis.fft_size
    V = ob.terms.V_loc + 0.1 * rng.standard_normal((nz, ny, nx))
    _, ham = oracle.energy_hamiltonian(ob, None, None, rho=oracle.guess_density(ob))
    bs = Basis(lib, nx, ny, nz, ob.model.unit_cell_volume)
    for ik, kpt in enumerate(ob.kpoints):
        H = ham[ik]
        H.potential = V
        kb = KBlock(lib, bs, kpt.mapping, H.kinetic)
        kb.set_projectors(basis.terms.P[ik].cpu().numpy().T, basis.terms.D)
        kb.set_potential(V)
        psi = np.linalg.qr(rng.standard_normal((H.n_G, 7)) + 1j * rng.standard_normal((H.n_G, 7)))[0]
        assert relerr(kb.apply(psi, 1), H.apply_local(psi)) < RTOL
        assert relerr(kb.apply(psi, 2), H.kinetic[:, None] * psi) < RTOL
        assert relerr(kb.apply(psi, 4), H.apply_nonlocal(psi)) < RTOL
        assert relerr(kb.apply(psi, 7), H.mul(psi)) < RTOL


def test_projector_builder_refuses_untabulated_channels(cell):
    """(l, n_proj) = (2, 3) and (3, 2) have no HGH form: an error, and P is not written."""
    basis, _ = cell
    kpt = basis.kpoints[1]
    G32 = kpt.G_vectors.to(torch.int32).contiguous()
    Bh = np.asfortranarray(basis.model.recip_lattice, dtype=np.float64)
    kh = np.ascontiguousarray(kpt.coordinate, dtype=np.float64)
    rp = np.array([[0.4, 0.5, 0.6, 0.7]])
    species = np.zeros(1, dtype=np.int32)
    pos = np.array([[0.1, 0.2, 0.3]])
    P = torch.full((64, kpt.n_G), 7.0 + 3.0j, dtype=torch.complex128, device="cuda:0")

    def call(nproj, P_ptr):
        n_p = C.c_int(-1)
        nproj = np.asarray([nproj], dtype=np.int32)
        st = basis.lib.dftk_mi_build_projectors_hgh(basis.handle, kpt.n_G, G32.data_ptr(), Bh.ctypes.data, kh.ctypes.data,
                                                     basis.model.unit_cell_volume, 1, rp.ctypes.data, nproj.ctypes.data,
                                                     1, species.ctypes.data, pos.ctypes.data, P_ptr, kpt.n_G, C.byref(n_p))
        basis.sync()
        return st, n_p.value
    assert call([3, 3, 2, 1], None) == (0, 29)
    for bad in ([0, 0, 3, 0], [0, 0, 0, 2], [4, 0, 0, 0], [1, 1, 1, 1 + 1]):
        st, _ = call(bad, P.data_ptr())
        assert st != 0, bad
        assert bool((P == 7.0 + 3.0j).all()), bad


# ------------------------------------------------------------------------------------------ forces on the cell
def test_forces_match_numpy(cell, state):
    basis, _ = cell
    psi, occ, rho = state
    Fl = dftk.compute_forces_term("AtomicLocal", basis, psi, occ, rho=rho)
    Fn = dftk.compute_forces_term("AtomicNonlocal", basis, psi, occ, rho=rho)
    Fl_ref = _numpy_local(basis, rho)
    Fn_ref = _numpy_nonlocal(basis, psi, occ)
    assert np.max(np.abs(Fl - Fl_ref)) <= 1e-11 * np.max(np.abs(Fl_ref)), (Fl, Fl_ref)
    assert np.max(np.abs(Fn - Fn_ref)) <= 1e-11 * np.max(np.abs(Fn_ref)), (Fn, Fn_ref)
    assert np.all(Fn[4] == 0)                          # the species without projectors
    assert np.all(np.abs(Fl[4]) > 0)


def test_forces_follow_the_atom_order(cell, state):
    """The same cell with the atoms in another order (the G sphere does not depend on it: the same psi): the forces are
    the permuted rows, the energies unchanged."""
    basis, _ = cell
    psi, occ, rho = state
    perm = [4, 6, 3, 0, 2, 5, 1]
    atoms = library_atoms()
    other = library_basis([atoms[i] for i in perm], [POSITIONS[i] for i in perm], fft_size=basis.fft_size)
    assert other.model.atom_groups == [[0], [1, 6], [2], [3, 5], [4]]
    for k1, k2 in zip(basis.kpoints, other.kpoints):
        assert np.array_equal(k1.mapping, k2.mapping)
    for name in ("AtomicLocal", "AtomicNonlocal", "Ewald"):
        F = dftk.compute_forces_term(name, basis, psi, occ, rho=rho)
        Fp = dftk.compute_forces_term(name, other, psi, occ, rho=rho)
        assert np.max(np.abs(Fp - F[perm])) <= 1e-13 * np.max(np.abs(F)), (name, Fp, F[perm])
    E, _ = dftk.energy_hamiltonian(basis, psi, occ, rho=rho, only_energies=True)
    Ep, _ = dftk.energy_hamiltonian(other, psi, occ, rho=rho, only_energies=True)
    for name in ("Kinetic", "AtomicLocal", "AtomicNonlocal", "Ewald", "PspCorrection", "Hartree", "Xc"):
        assert abs(Ep[name] - E[name]) <= 1e-12 * max(abs(E[name]), 1.0), (name, Ep[name], E[name])


def test_termwise_forces_match_finite_differences(cell, state):
    """Central differences of each energy at fixed psi and rho, one atom of every species displaced along a generic
    direction (the first atom of each group, the tolerance of test_gpu_forces.py)."""
    basis, _ = cell
    psi, occ, rho = state
    F = {name: dftk.compute_forces_term(name, basis, psi, occ, rho=rho) for name in ("AtomicLocal", "AtomicNonlocal", "Ewald")}
    rng = np.random.default_rng(29)
    eps = 1e-5
    for group in basis.model.atom_groups:
        ia = group[0]
        d = rng.standard_normal(3)
        d /= np.linalg.norm(d)

        def energies(sign):
            pos = [p + (sign * eps * d if i == ia else 0) for i, p in enumerate(POSITIONS)]
            return dftk.energy_hamiltonian(library_basis(positions=pos, fft_size=basis.fft_size), psi, occ, rho=rho,
                                           only_energies=True)[0]
        Ep, Em = energies(1), energies(-1)
        for name, f in F.items():
            fd = (Ep[name] - Em[name]) / (2 * eps)
            assert abs(f[ia] @ d + fd) < 1e-7, (SPECIES[ia], name, f[ia] @ d, -fd)


# ------------------------------------------------------------------------------------------ zincblende SiC
A_SIC = 8.24
SIC_LATTICE = A_SIC / 2 * np.array([[0.0, 1, 1], [1, 0, 1], [1, 1, 0]])
SIC_POSITIONS = [np.zeros(3), np.ones(3) / 4]
SIC_DISPLACED = [np.array([0.01, 0.02, -0.015]), np.ones(3) / 4 + np.array([-0.01, 0.005, 0.02])]


def _sic_library(positions, kgrid, fft_size=None, symmetries=False, temperature=1e-3):
    atoms = [dftk.ElementPsp("Si", lpsp.load_psp("Si", "lda")), dftk.ElementPsp("C", lpsp.load_psp("C", "lda"))]
    # (a small temperature, as test_gpu_forces.py: the Fermi level search of the first steps needs no integer filling)
    model = dftk.model_DFT(SIC_LATTICE, atoms, positions, functionals=FUN, symmetries=symmetries, temperature=temperature)
    return dftk.PlaneWaveBasis(model, 15, kgrid, fft_size=fft_size, device="cuda:0")


def _sic_scf(positions, tol=1e-10):
    basis = _sic_library(positions, dftk.MonkhorstPack((2, 2, 2)))
    return dftk.self_consistent_field(basis, tol=tol, nbandsalg=dftk.AdaptiveBands(basis.model, n_bands_converge=6))


def test_displaced_sic_scf_and_forces():
    res = _sic_scf(SIC_DISPLACED)
    basis = res["basis"]
    atoms = [oracle.ElementPsp("Si", oracle.load_psp_hgh("Si", "lda")), oracle.ElementPsp("C", oracle.load_psp_hgh("C", "lda"))]
    ob = oracle.PlaneWaveBasis(oracle.model_DFT(SIC_LATTICE, atoms, SIC_DISPLACED, functionals=FUN, temperature=1e-3), 15,
                               oracle.MonkhorstPack((2, 2, 2)), fft_size=basis.fft_size)
    ores = oracle.self_consistent_field(ob, tol=1e-10, nbandsalg=oracle.AdaptiveBands(ob.model, n_bands_converge=6))
    assert res["converged"] and ores["converged"]
    assert abs(res["energies"].total - ores["energies"].total) < 1e-8 * 2
    for name in ores["energies"]:
        assert abs(res["energies"][name] - ores["energies"][name]) < 1e-7, name
    for lam, olam in zip(res["eigenvalues"], ores["eigenvalues"]):
        np.testing.assert_allclose(lam[:6], olam[:6], atol=1e-7)
    assert np.linalg.norm(res["rho"].cpu().numpy() - ores["rho"]) * np.sqrt(ob.dvol) < 1e-7
    # total forces against the SCF energy
    F = dftk.compute_forces(res)
    d = np.random.default_rng(31).standard_normal((2, 3))
    d /= np.linalg.norm(d)
    eps = 1e-5
    Ep = _sic_scf([p + eps * x for p, x in zip(SIC_DISPLACED, d)], tol=1e-11)["energies"].total
    Em = _sic_scf([p - eps * x for p, x in zip(SIC_DISPLACED, d)], tol=1e-11)["energies"].total
    assert abs(np.sum(F * d) + (Ep - Em) / (2 * eps)) < 1e-7


def _ops(symops):
    return sorted((tuple(s.W.reshape(-1).tolist()), tuple(np.round(np.mod(s.w, 1.0), 8) % 1.0)) for s in symops)


def test_sic_symmetry_group_and_reduced_mesh():
    """Zincblende has 24 operations (Td): inversion swaps Si and C.  The library's search finds the oracle's, the
    irreducible 2x2x2 mesh gives the full mesh's SCF, and the forces vanish."""
    lat_atoms = [dftk.ElementPsp("Si", lpsp.load_psp("Si", "lda")), dftk.ElementPsp("C", lpsp.load_psp("C", "lda"))]
    model = dftk.model_DFT(SIC_LATTICE, lat_atoms, SIC_POSITIONS, functionals=FUN, symmetries=True, temperature=1e-3)
    oatoms = [oracle.ElementPsp("Si", oracle.load_psp_hgh("Si", "lda")), oracle.ElementPsp("C", oracle.load_psp_hgh("C", "lda"))]
    omodel = oracle.model_DFT(SIC_LATTICE, oatoms, SIC_POSITIONS, functionals=FUN, symmetries=True)
    assert len(model.symmetries) == len(omodel.symmetries) == 24
    assert _ops(model.symmetries) == _ops(omodel.symmetries)
    si = dftk.model_DFT(SIC_LATTICE, [lat_atoms[0]] * 2, SIC_POSITIONS, functionals=FUN, symmetries=True)
    assert len(si.symmetries) == 48                                     # the same sites with one species: diamond
    b_sym = dftk.PlaneWaveBasis(model, 15, dftk.MonkhorstPack((2, 2, 2)), device="cuda:0")
    b_full = _sic_library(SIC_POSITIONS, dftk.MonkhorstPack((2, 2, 2)).reducible(), fft_size=b_sym.fft_size)
    assert len(b_sym.kpoints) < len(b_full.kpoints)
    r_sym = dftk.self_consistent_field(b_sym, tol=1e-10)
    r_full = dftk.self_consistent_field(b_full, tol=1e-10)
    assert abs(r_sym["energies"].total - r_full["energies"].total) < 1e-9
    assert np.linalg.norm(r_sym["rho"].cpu().numpy() - r_full["rho"].cpu().numpy()) * np.sqrt(b_sym.dvol) < 1e-7
    assert np.max(np.abs(dftk.compute_forces(r_sym))) < 1e-9
    assert np.max(np.abs(dftk.compute_forces(r_full))) < 1e-9
