"""The non-linear core correction through the public interface: GTH silicon written as a UPF file with a Gaussian core
density (tests/nlcc_gen.py) in the displaced cell, cut-off and k-grids of tests/test_gpu_upf.py -- the core cube, SCF
energies against the oracle's XC on rho + rho_core, forces against differences of the SCF energy, the ``use_nlcc`` switch,
collinear spin, every block kind, the torch twin, ``apply_kernel``, a mixed HGH + UPF cell, and the refusals that stay.

The core is made up (no physical pseudopotential has it); what is tested is that every path sees rho + rho_core / n_spin in
the XC term and rho everywhere else, and that the Xc forces are the derivative of that energy."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd.terms import local_potential_fused  # noqa: E402
from oracle import terms as oterms  # noqa: E402

import nlcc_gen  # noqa: E402
import upf_gen  # noqa: E402
from nlcc_gen import CORE, E_QUAD_CORE  # noqa: E402
from test_gpu_response import KERNEL_TOL, kernel_drho, relmax  # noqa: E402
from test_gpu_upf import DISPLACED, ECUT, FUN, PBE, TOL, _kgrid, _scf  # noqa: E402

FD_STEP, FD_BOUND = 1e-5, 1e-7      # tests/test_gpu_upf.py::test_forces_match_energy_differences


@pytest.fixture(scope="module")
def psp():
    return {(f, c): nlcc_gen.core_psp("Si", f, core=c) for f in ("lda", "pbe") for c in (True, False)}


def _basis(p, positions=DISPLACED, gamma=False, functionals=FUN, fft_size=None, **kw):
    lat, _, _ = dftk.silicon_cell()
    mk = {k: kw.pop(k) for k in list(kw) if k in ("magnetic_moments", "spin_polarization", "use_nlcc")}
    model = dftk.model_DFT(lat, [dftk.ElementPsp("Si", psp=p)] * 2, positions, functionals=functionals, **mk)
    return dftk.PlaneWaveBasis(model, ECUT, _kgrid(gamma), fft_size=fft_size, device="cuda:0", **kw)


class _OracleCube:
    """what oracle.terms.xc_energy_potential asks of a basis, on the cube of a device basis"""

    def __init__(self, basis):
        self._G = basis.G_vectors_cart_cube().cpu().numpy()
        self.model = SimpleNamespace(functionals=tuple(basis.model.functionals))
        self.dvol = basis.dvol

    def G_vectors_cart_cube(self):
        return self._G

    def fft_cube(self, f):
        return np.fft.fftn(f)

    def irfft_cube(self, c):
        return np.fft.ifftn(c).real


def _oracle_xc(basis, rho):
    core = basis.terms.rho_core.cpu().numpy()
    return oterms.xc_energy_potential(_OracleCube(basis), rho.cpu().numpy() + core)[0]


@pytest.fixture(scope="module")
def lda_222(psp):
    """the SCFs most tests share: LDA on the 2 x 2 x 2 grid, with and without the core"""
    bc = _basis(psp["lda", True])
    bn = _basis(psp["lda", False], fft_size=bc.fft_size)
    return bc, bn, _scf(bc), _scf(bn)


@pytest.fixture(scope="module")
def pbe_gamma(psp):
    bc = _basis(psp["pbe", True], gamma=True, functionals=PBE)
    bn = _basis(psp["pbe", False], gamma=True, functionals=PBE, fft_size=bc.fft_size)
    return bc, bn, _scf(bc), _scf(bn)


# ------------------------------------------------------------------------------------------------ set-up
def _twin_core_cube(basis, ff_of_species, atoms):
    m = basis.model
    return upf_gen.twin_superposition(basis.fft_size, m.recip_lattice, m.unit_cell_volume, ff_of_species, atoms)


def test_core_cube_against_the_closed_form(lda_222, pbe_gamma):
    bc, bn, _, _ = lda_222
    T = bc.terms
    want = _twin_core_cube(bc, [nlcc_gen.closed_core_ff("Si")], [(0, np.asarray(p)) for p in bc.model.positions])
    got = T.rho_core.cpu().numpy()
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f"rho_core: {err:.2e} of its largest value {np.max(np.abs(want)):.3e}; integral {got.sum() * bc.dvol:.12f}")
    assert err <= 10 * E_QUAD_CORE
    assert abs(got.sum() * bc.dvol - 2 * CORE["Si"][0]) <= 10 * E_QUAD_CORE * 2 * CORE["Si"][0]      # ff(0) = c per atom
    assert T.grad_core is None and T.core_ff.shape == (1, bc.N)                    # LDA: no gradient cubes
    assert bn.terms.rho_core is None and bn.terms.core_ff is None and bn.terms.grad_core is None
    # PBE keeps the three gradient cubes of the same superposition
    Tp = pbe_gamma[0].terms
    assert Tp.grad_core.shape == (3,) + tuple(Tp.rho_core.shape) and bool(torch.isfinite(Tp.grad_core).all())
    G = pbe_gamma[0].G_vectors_cart_cube().cpu().numpy()
    cf = np.fft.fftn(Tp.rho_core.cpu().numpy())
    for a in range(3):
        ref = np.fft.ifftn(1j * G[..., a] * cf).real
        assert np.max(np.abs(Tp.grad_core[a].cpu().numpy() - ref)) <= 1e-12 * np.max(np.abs(ref))


def _sic(carbon, si=None, **kw):
    lat, _, _ = dftk.silicon_cell()
    lat = np.asarray(lat) * (8.24 / 10.26)
    atoms = [dftk.ElementPsp("Si", psp=si or dftk.load_psp("Si", "lda")), dftk.ElementPsp("C", psp=carbon)]
    model = dftk.model_DFT(lat, atoms, DISPLACED, functionals=FUN)
    return dftk.PlaneWaveBasis(model, ECUT, _kgrid(False), device="cuda:0", **kw)


@pytest.fixture(scope="module")
def sic():
    bc = _sic(nlcc_gen.core_psp("C", core=True))
    bn = _sic(nlcc_gen.core_psp("C", core=False), fft_size=bc.fft_size)
    return bc, bn, _scf(bc), _scf(bn)


def test_mixed_cell_sic_hgh_silicon_and_core_corrected_carbon(sic):
    """two species, one with a core: a zero row in the form-factor table, the cube of the carbon atom alone; the SCF and
    its E_xc; Xc forces on the carbon atom only"""
    bc, bn, rc, rn = sic
    assert len(bc.model.atom_groups) == 2
    T = bc.terms
    assert bool((T.core_ff[0] == 0).all()) and float(T.core_ff[1].max()) > 0.9 * CORE["C"][0]
    want = _twin_core_cube(bc, [lambda q: np.zeros_like(q), nlcc_gen.closed_core_ff("C")],
                           [(s, np.asarray(p)) for s, p in enumerate(bc.model.positions)])
    got = T.rho_core.cpu().numpy()
    assert np.max(np.abs(got - want)) <= 10 * E_QUAD_CORE * np.max(np.abs(want))
    assert abs(rc["energies"]["Xc"] - _oracle_xc(bc, rc["rho"])) < 1e-11 * max(1.0, abs(rc["energies"]["Xc"]))
    assert abs(rc["energies"].total - rn["energies"].total) > 1e-4
    Fx = dftk.compute_forces_term("Xc", bc, rc["psi"], rc["occupation"], rho=rc["rho"])
    assert Fx.shape == (2, 3) and np.all(Fx[0] == 0) and np.max(np.abs(Fx[1])) > 1e-5
    assert dftk.compute_forces_term("Xc", bn, rn["psi"], rn["occupation"], rho=rn["rho"]) is None
    F = dftk.compute_forces(rc)
    parts = [dftk.compute_forces_term(n, bc, rc["psi"], rc["occupation"], rho=rc["rho"]) for n in bc.model.term_types]
    assert np.allclose(F, sum(p for p in parts if p is not None), rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------ SCF
def test_scf_lda_with_a_core(lda_222):
    bc, bn, rc, rn = lda_222
    exc, ref = rc["energies"]["Xc"], _oracle_xc(bc, rc["rho"])
    print(f"LDA: E_xc {exc:.12f}, oracle on rho + rho_core {ref:.12f}; total with / without the core "
          f"{rc['energies'].total:.10f} / {rn['energies'].total:.10f}")
    assert abs(exc - ref) < 1e-11 * max(1.0, abs(ref))                 # (tests/test_gpu_scf.py, LDA against the oracle)
    assert abs(rc["energies"].total - rn["energies"].total) > 1e-4     # the core is not ignored
    # without the core in the argument the same oracle is far off
    assert abs(exc - oterms.xc_energy_potential(_OracleCube(bc), rc["rho"].cpu().numpy())[0]) > 1e-4


def test_scf_pbe_with_a_core(pbe_gamma):
    bc, bn, rc, rn = pbe_gamma
    exc, ref = rc["energies"]["Xc"], _oracle_xc(bc, rc["rho"])
    print(f"PBE: E_xc {exc:.12f}, oracle on rho + rho_core {ref:.12f}; total with / without the core "
          f"{rc['energies'].total:.10f} / {rn['energies'].total:.10f}")
    assert abs(exc - ref) < 1e-10 * max(1.0, abs(ref))                 # (tests/test_gpu_scf.py, PBE against the oracle)
    assert abs(rc["energies"].total - rn["energies"].total) > 1e-4


def test_use_nlcc_false_is_the_file_without_a_core(psp, lda_222):
    bc, bn, _, rn = lda_222
    b0 = _basis(psp["lda", True], fft_size=bc.fft_size, use_nlcc=False)
    assert b0.terms.rho_core is None and b0.terms.core_ff is None
    r0 = _scf(b0)
    assert abs(r0["energies"].total - rn["energies"].total) <= 10 * TOL
    for name, v in rn["energies"].items():
        assert abs(r0["energies"][name] - v) <= 10 * TOL, name
    assert dftk.compute_forces_term("Xc", b0, r0["psi"], r0["occupation"], rho=r0["rho"]) is None
    assert np.max(np.abs(dftk.compute_forces(r0) - dftk.compute_forces(rn))) <= 10 * TOL


# ------------------------------------------------------------------------------------------------ forces
def _forces_against_differences(p, res, basis, **kw):
    F = dftk.compute_forces(res)
    Fx = dftk.compute_forces_term("Xc", basis, res["psi"], res["occupation"], rho=res["rho"])
    d = np.random.default_rng(11).standard_normal((2, 3))
    d /= np.linalg.norm(d)

    def energy(sign):
        b = _basis(p, [q + sign * FD_STEP * x for q, x in zip(DISPLACED, d)], fft_size=basis.fft_size, **kw)
        return _scf(b, tol=1e-11)["energies"].total
    gap = abs(np.sum(F * d) + (energy(1) - energy(-1)) / (2 * FD_STEP))
    print(f"forces: F.d + dE/dt = {gap:.2e} (bound {FD_BOUND:.0e}); largest Xc force {np.max(np.abs(Fx)):.3e}, Xc share "
          f"of F.d {np.sum(Fx * d):.3e}")
    # a missing Xc force must not pass: its size is at least 100 times the bound
    assert np.max(np.abs(Fx)) >= 100 * FD_BOUND and abs(np.sum(Fx * d)) >= 100 * FD_BOUND
    assert gap < FD_BOUND
    return Fx


def test_forces_match_energy_differences_lda(psp, lda_222):
    bc, bn, rc, rn = lda_222
    _forces_against_differences(psp["lda", True], rc, bc)
    assert dftk.compute_forces_term("Xc", bn, rn["psi"], rn["occupation"], rho=rn["rho"]) is None
    for name in ("AtomicLocal", "AtomicNonlocal", "Ewald", "Xc"):
        assert dftk.compute_forces_term(name, bc, rc["psi"], rc["occupation"], rho=rc["rho"]).shape == (2, 3)


def test_forces_match_energy_differences_pbe(psp, pbe_gamma):
    bc, _, rc, _ = pbe_gamma
    _forces_against_differences(psp["pbe", True], rc, bc, gamma=True, functionals=PBE)


# ------------------------------------------------------------------------------------------------ spin and block kinds
@pytest.mark.parametrize("functionals", [("lda_x", "lda_c_pw"), PBE], ids=["lda", "pbe"])
def test_collinear_zero_moments_match_unpolarised(psp, functionals):
    """each channel gets exactly half of the core density (and of its gradient)"""
    import warnings
    p = psp["pbe" if functionals == PBE else "lda", True]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        b1 = _basis(p, functionals=functionals)
        b2 = _basis(p, functionals=functionals, fft_size=b1.fft_size, spin_polarization="collinear")
        r1, r2 = _scf(b1), _scf(b2)
    assert b2.terms.rho_core.shape == b1.terms.rho_core.shape                  # ONE cube, the total
    assert abs(r1["energies"].total - r2["energies"].total) < 1e-9
    assert abs(r1["energies"]["Xc"] - r2["energies"]["Xc"]) < 1e-9
    F1, F2 = dftk.compute_forces(r1), dftk.compute_forces(r2)
    X1 = dftk.compute_forces_term("Xc", b1, r1["psi"], r1["occupation"], rho=r1["rho"])
    X2 = dftk.compute_forces_term("Xc", b2, r2["psi"], r2["occupation"], rho=r2["rho"])
    assert np.max(np.abs(X1)) > 1e-5
    assert np.max(np.abs(F2 - F1)) < 1e-8 and np.max(np.abs(X2 - X1)) < 1e-8


def test_gamma_real_matches_complex(psp):
    p = psp["lda", True]
    b0 = _basis(p, gamma=True, gamma_real=False)
    b1 = _basis(p, gamma=True, gamma_real=True, fft_size=b0.fft_size)
    assert b1.kpoints[0].gamma_real and not b0.kpoints[0].gamma_real
    r0, r1 = _scf(b0), _scf(b1)
    assert abs(r1["energies"].total - r0["energies"].total) < 1e-9
    for name, v in r0["energies"].items():
        assert abs(r1["energies"][name] - v) < 1e-8, name
    assert np.max(np.abs(dftk.compute_forces(r1) - dftk.compute_forces(r0))) < 1e-8


def test_batched_kblocks_match_sequential(psp, lda_222, monkeypatch):
    bc, _, rc, _ = lda_222
    monkeypatch.setenv("DFTK_MI_KBATCH_SEQUENTIAL", "1")
    r1 = _scf(_basis(psp["lda", True], fft_size=bc.fft_size))
    monkeypatch.delenv("DFTK_MI_KBATCH_SEQUENTIAL", raising=False)
    assert abs(rc["energies"].total - r1["energies"].total) < 1e-8
    assert abs(rc["energies"]["Xc"] - r1["energies"]["Xc"]) < 1e-8


# ------------------------------------------------------------------------------------------------ torch twin
@pytest.mark.parametrize("which", ["lda", "pbe"])
def test_torch_twin_adds_the_core(which, lda_222, pbe_gamma, monkeypatch):
    """DFTK_MI_TORCH_LOCAL=1 against the fused entry at the tolerances of tests/test_gpu_scf.py (the LDA and the PBE twin
    tests), and both far from the same model without the core"""
    bc, bn, rc, _ = lda_222 if which == "lda" else pbe_gamma
    rho = rc["rho"]
    E1, ham1 = dftk.energy_hamiltonian(bc, None, None, rho=rho)
    monkeypatch.setenv("DFTK_MI_TORCH_LOCAL", "1")
    E2, ham2 = dftk.energy_hamiltonian(bc, None, None, rho=rho)
    monkeypatch.delenv("DFTK_MI_TORCH_LOCAL")
    for name in ("AtomicLocal", "Hartree", "Xc"):
        assert abs(E1[name] - E2[name]) < 1e-12 * max(1.0, abs(E2[name])), name
    V1, V2 = ham1[0].potential, ham2[0].potential
    assert float((V1 - V2).abs().max()) < (1e-12 if which == "lda" else 1e-11) * float(V2.abs().max())
    E0, ham0 = dftk.energy_hamiltonian(bn, None, None, rho=rho)
    assert abs(E0["Xc"] - E1["Xc"]) > 1e-4 and E0["Hartree"] == E1["Hartree"]
    assert float((ham0[0].potential - V1).abs().max()) > 1e-4


# ------------------------------------------------------------------------------------------------ response
def test_apply_kernel_on_a_core_corrected_state(lda_222):
    """against central differences of the potential with rho_core fixed, as tests/test_gpu_response.py does without a core
    (its step, its direction, its tolerance)"""
    bc, bn, rc, _ = lda_222
    rho = rc["rho"]
    drho = kernel_drho(bc, rho)
    h = 1e-4 * float(rho.max()) / float(drho.abs().max())
    Vp = local_potential_fused(bc, rho + h * drho, want_energies=False)["V"]
    Vm = local_potential_fused(bc, rho - h * drho, want_energies=False)["V"]
    fd = ((Vp - Vm) / (2 * h)).cpu().numpy()
    got = dftk.apply_kernel(bc, drho, rho).cpu().numpy()
    err = relmax(got, fd)
    without = relmax(dftk.apply_kernel(bn, drho, rho).cpu().numpy(), fd)
    print(f"apply_kernel with a core: rel max err against central differences {err:.3e}; f_xc(rho) alone: {without:.3e}")
    assert err < KERNEL_TOL
    assert without > 100 * KERNEL_TOL                                     # the kernel of rho alone is the wrong one


# ------------------------------------------------------------------------------------------------ refusals that stay
def test_stresses_and_phonons_still_refuse(psp):
    r = _scf(_basis(psp["lda", True], gamma=True))
    with pytest.raises(NotImplementedError, match="UPF"):
        dftk.compute_stresses_cart(r)
    with pytest.raises(NotImplementedError, match="UPF"):
        dftk.compute_dynmat(r)
