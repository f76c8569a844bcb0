"""Meta-GGA (SCAN) from the point-wise forms up to the SCF: energy <-> Hamiltonian consistency, the recorded ABINIT values of
the reference's "Silicon SCAN (small)" test, and the SCF plumbing (tau in the result, restart, bands, forces).

Tolerances:
* consistency (test/hamiltonian_consistency.jl of the reference): the Richardson-extrapolated central difference of
  E(psi + h dpsi) at h = 2e-4 and 1e-4 against sum_k w_k sum_n f_n 2 Re <dpsi_n | H psi_n>.  The identical check with PBE runs
  in the same test (code that existed before); SCAN gets 10 x its relative error.  The steps are small enough that both are
  dominated by the rounding of the energy difference (1e-16 E / h), not by the fifth derivative.  The check does not depend on
  the constants of SCAN being right, only on v_rho, v_sigma, v_tau and the operator being the derivatives of the energy coded.
* ABINIT: tests/golden/silicon_scan_abinit.json, 5e-5 Ha on bands 1-7 of every irreducible k-point and on the total energy --
  the reference test's own ``test_tol`` and ``n_ignored = 1``.
* force: the tolerance of tests/test_gpu_forces.py for PBE (1e-7 on a central difference at eps = 1e-5).
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd.eigen import nearest_index  # noqa: E402

SCAN = ("mgga_x_scan", "mgga_c_scan")
PBE = ("gga_x_pbe", "gga_c_pbe")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "silicon_scan_abinit.json")


A_ABINIT = 2 * 5.131570667152971       # the lattice constant the recorded values were computed at


def silicon_basis(functionals, Ecut, kgrid, positions=None, a=10.26, symmetries=False, **kw):
    lat, atoms, pos = dftk.silicon_cell(functional="pbe", a=a)
    model = dftk.model_DFT(lat, atoms, pos if positions is None else positions, functionals=functionals,
                           symmetries=symmetries)
    return dftk.PlaneWaveBasis(model, Ecut, kgrid, device="cuda:0", **kw)


def directional_derivative(functionals):
    """(extrapolated central difference of the energy along dpsi, 2 Re <dpsi | H psi> weighted by occupations)"""
    basis = silicon_basis(functionals, 7, dftk.ExplicitKpoints([[0.2, -0.1, 0.3]], [1.0]))
    kpt = basis.kpoints[0]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    psi = dftk.ortho_qr(basis, dftk.random_orbitals(basis, kpt, 4, gen))
    dpsi = dftk.random_orbitals(basis, kpt, 4, gen)
    dpsi = dpsi / torch.linalg.norm(dpsi)
    occ = [np.full(4, 2.0)]
    uses_tau = basis.model.uses_tau

    def densities(p):
        rho = dftk.compute_density(basis, [p], occ)
        return rho, (dftk.compute_kinetic_energy_density(basis, [p], occ) if uses_tau else None)

    def energy(h):
        p = (psi + h * dpsi).contiguous()
        rho, tau = densities(p)
        E, _ = dftk.energy_hamiltonian(basis, [p], occ, rho=rho, only_energies=True, **(dict(tau=tau) if uses_tau else {}))
        return E.total

    def central(h):
        return (energy(h) - energy(-h)) / (2 * h)
    h = 2e-4
    fd = (4 * central(h / 2) - central(h)) / 3
    rho, tau = densities(psi)
    _, ham = dftk.energy_hamiltonian(basis, [psi], occ, rho=rho, **(dict(tau=tau) if uses_tau else {}))
    assert (ham[0].tau_potential is not None) == uses_tau
    Hpsi = ham[0] @ psi
    ref = float(sum(occ[0][n] * 2 * torch.vdot(dpsi[n], Hpsi[n]).real.item() for n in range(4)) * basis.kweights[0])
    return fd, ref


def test_energy_hamiltonian_consistency():
    fd_pbe, ref_pbe = directional_derivative(PBE)
    fd_scan, ref_scan = directional_derivative(SCAN)
    e_pbe = abs(fd_pbe - ref_pbe) / abs(ref_pbe)
    e_scan = abs(fd_scan - ref_scan) / abs(ref_scan)
    print(f"MGGA consistency: PBE {e_pbe:.2e} (dE = {ref_pbe:.6f}), SCAN {e_scan:.2e} (dE = {ref_scan:.6f})")
    assert e_pbe < 1e-8
    assert abs(ref_scan - ref_pbe) > 1e-6 * abs(ref_pbe)            # (another Hamiltonian)
    assert e_scan <= 10 * e_pbe


def test_energy_hamiltonian_needs_tau():
    basis = silicon_basis(SCAN, 5, dftk.ExplicitKpoints([[0.0, 0.0, 0.0]], [1.0]))
    rho = dftk.guess_density(basis)
    with pytest.raises(ValueError, match="tau"):
        dftk.energy_hamiltonian(basis, None, None, rho=rho)
    tau = dftk.guess_kinetic_energy_density(basis, rho)
    assert tau.shape == rho.shape and float(tau.min()) >= 0.0
    E, ham = dftk.energy_hamiltonian(basis, None, None, rho=rho, tau=tau)
    assert np.isfinite(E["Xc"]) and ham[0].tau_potential is not None
    pbe = silicon_basis(PBE, 5, dftk.ExplicitKpoints([[0.0, 0.0, 0.0]], [1.0]))
    assert dftk.guess_kinetic_energy_density(pbe, rho) is None


@pytest.fixture(scope="module")
def scan_abinit():
    with open(GOLDEN) as fh:
        gold = json.load(fh)
    # as the recorded calculation: the four irreducible k-points with their weights, rho and tau symmetrised (the 27^3 grid
    # does not carry the fractional translations of the diamond structure: the unreduced mesh gives another density)
    basis = silicon_basis(SCAN, 15, dftk.ExplicitKpoints(gold["kcoords"], gold["kweights"]), fft_size=(27, 27, 27),
                          a=gold["lattice_constant"], symmetries=True)
    res = dftk.self_consistent_field(basis, tol=1e-8, nbandsalg=dftk.AdaptiveBands(basis.model, n_bands_converge=8))
    return gold, basis, res


def test_silicon_scan_against_recorded_abinit_values(scan_abinit):
    """Silicon, HGH PBE pseudopotential, Ecut 15, 27^3, the four irreducible points of the 3x3x3 mesh: bands 1-7 within
    5e-5 Ha at each of them, total energy within 5e-5 Ha."""
    gold, basis, res = scan_abinit
    assert res["converged"]
    coords = [k.coordinate for k in basis.kpoints]
    n_cmp = 8 - gold["bands_ignored"]
    for kc, row in zip(gold["kcoords"], gold["eigenvalues"]):
        ik = nearest_index(coords, kc)
        d = np.asarray(coords[ik]) - np.asarray(kc)
        assert np.abs(d - np.round(d)).max() < 1e-10
        diff = np.abs(np.asarray(res["eigenvalues"][ik])[:8] - np.asarray(row))
        print(f"MGGA abinit k = {kc}: |d eps| = {np.array2string(diff, precision=2)}")
        assert diff[:n_cmp].max() < gold["tolerance"], (kc, diff)
    dE = res["energies"].total - gold["total_energy"]
    print(f"MGGA abinit E = {res['energies'].total:.9f}, dE = {dE:.2e}")
    assert abs(dE) < gold["tolerance"]


@pytest.fixture(scope="module")
def small_scf():
    basis = silicon_basis(SCAN, 7, dftk.MonkhorstPack((2, 2, 2)).reducible())
    return basis, dftk.self_consistent_field(basis, tol=1e-9)


def test_scfres_carries_tau_and_restarts(small_scf, tmp_path):
    basis, res = small_scf
    assert res["converged"]
    tau = dftk.compute_kinetic_energy_density(basis, res["psi"], res["occupation"], res["occupation_threshold"])
    assert torch.equal(res["tau"], tau)
    assert abs(float(tau.sum()) * basis.dvol - res["energies"]["Kinetic"]) < 1e-10 * abs(res["energies"]["Kinetic"])
    path = str(tmp_path / "scan.npz")
    dftk.save_scfres(path, res)
    back = dftk.load_scfres(path, basis)
    assert torch.equal(back["tau"], res["tau"])
    again = dftk.self_consistent_field(basis, rho=back["rho"], psi=back["psi"], tau=back["tau"], tol=1e-9)
    assert again["converged"] and again["n_iter"] <= 3
    assert abs(again["energies"].total - res["energies"].total) < 1e-9
    d = dftk.scfres_to_dict(res)
    assert np.asarray(d["τ"]).shape == (1,) + tuple(res["tau"].shape)


def test_compute_bands_reads_tau(small_scf):
    basis, res = small_scf
    kc = [k.coordinate.tolist() for k in basis.kpoints[:2]]
    bands = dftk.compute_bands(res, dftk.ExplicitKpoints(kc, [0.5, 0.5]), n_bands=4, tol=1e-6)
    for ik in range(2):
        assert np.abs(np.asarray(bands["eigenvalues"][ik])[:4] - np.asarray(res["eigenvalues"][ik])[:4]).max() < 1e-5


def test_force_matches_energy_difference():
    kg = dftk.ExplicitKpoints([[0.25, 0.0, -0.25]], [1.0])
    pos = [np.ones(3) / 8 + np.array([0.02, -0.01, 0.015]), -np.ones(3) / 8]

    def scf(p):
        return dftk.self_consistent_field(silicon_basis(SCAN, 7, kg, positions=p, fft_size=(18, 18, 18)), tol=1e-11)
    res = scf(pos)
    assert res["converged"]
    F = dftk.compute_forces(res)
    d = np.zeros((2, 3))
    d[0, 0] = 1.0
    eps = 1e-5
    Ep = scf([p + eps * x for p, x in zip(pos, d)])["energies"].total
    Em = scf([p - eps * x for p, x in zip(pos, d)])["energies"].total
    fd = (Ep - Em) / (2 * eps)
    print(f"MGGA force: F = {F[0][0]:.9f}, -dE/dx = {-fd:.9f}")
    assert abs(np.sum(np.asarray(F) * d) + fd) < 1e-7
