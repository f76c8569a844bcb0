"""PBE with collinear spin through the whole SCF (the reference's test/iron_pbe.jl combination): ``local_potential_fused``
routes a two-component density with a GGA functional to ``dftk_mi_local_potential_collinear_gga``; the SCF loop, mixing,
symmetrisation and the checkpoints are the ones of the LDA collinear path and needed no change.

(a) silicon without magnetisation: the collinear PBE run is the unpolarised PBE run.
(b) bcc iron, the cell and discretisation of tests/test_gpu_spin.py with PBE: it converges, E_xc is the NumPy twin's at the
    converged density, starting from the opposite moment exchanges the channels, and the magnetisation survives.  Total
    energy and magnetisation are printed and recorded in DESIGN.md, not pinned: the reference's ABINIT numbers for iron PBE
    were computed with another pseudopotential (q16 PBE) than its test's cell uses (q8 LDA) and are not comparable.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from tests.test_oracle_golden import IRON_LATTICE  # noqa: E402

import test_gpu_spin_gga_pipeline as P  # noqa: E402

PBE = ("gga_x_pbe", "gga_c_pbe")


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.manual_seed(3)


def test_collinear_pbe_without_magnetisation_equals_unpolarised_pbe():
    """Silicon, PBE, Ecut 7, two k-points, fft 18^3 (the set-up of the LDA twin of this test in tests/test_gpu_spin.py):
    energy to 1e-9, both channels' eigenvalues to 1e-7, rho_up = rho / 2 to 1e-7."""
    lat, atoms, pos = dftk.silicon_cell()
    kg = dftk.ExplicitKpoints([[0, 0, 0], [0.25, 0.0, -0.5]], [0.5, 0.5])
    m1 = dftk.model_DFT(lat, atoms, pos, functionals=PBE)
    m2 = dftk.model_DFT(lat, atoms, pos, functionals=PBE, spin_polarization="collinear")
    b1 = dftk.PlaneWaveBasis(m1, 7, kg, fft_size=(18, 18, 18))
    b2 = dftk.PlaneWaveBasis(m2, 7, kg, fft_size=(18, 18, 18))
    r1 = dftk.self_consistent_field(b1, tol=1e-9)
    r2 = dftk.self_consistent_field(b2, tol=1e-9)
    assert r1["converged"] and r2["converged"] and r2["rho"].shape == (2, 18, 18, 18)
    assert abs(r1["energies"].total - r2["energies"].total) < 1e-9
    for ik in range(2):
        for s_ in range(2):
            np.testing.assert_allclose(r2["eigenvalues"][ik + 2 * s_][:4], r1["eigenvalues"][ik][:4], atol=1e-7)
    assert float(torch.linalg.norm(r2["rho"][0] - r1["rho"] / 2)) * np.sqrt(b1.dvol) < 1e-7
    assert float(torch.linalg.norm(r2["rho"][1] - r1["rho"] / 2)) * np.sqrt(b1.dvol) < 1e-7


def iron_pbe_basis(moment):
    Fe = dftk.ElementPsp("Fe", dftk.load_psp("Fe", "lda"))
    model = dftk.model_DFT(IRON_LATTICE, [Fe], [np.zeros(3)], functionals=PBE, temperature=0.01, smearing="fermi_dirac",
                           magnetic_moments=(moment,), symmetries=True)
    return dftk.PlaneWaveBasis(model, 15, dftk.MonkhorstPack((4, 4, 4), (0.5, 0.5, 0.5)), fft_size=(20, 20, 20))


def test_iron_pbe_collinear_scf(tmp_path):
    db = iron_pbe_basis(4.0)
    res = dftk.self_consistent_field(db, rho=dftk.guess_density(db, (4.0,)), tol=1e-9)
    assert res["converged"]
    rho = res["rho"].cpu().numpy()
    assert rho.shape == (2, 20, 20, 20)
    # E_xc of the result against the NumPy twin (numpy.fft gradients, the restatement's point-wise values) at this density
    _, E = P.twin(np.float64, rho, None, None, threshold=dftk.terms._DENSITY_THRESHOLD, shape=(20, 20, 20),
                  recip=np.asarray(db.model.recip_lattice), volume=db.model.unit_cell_volume)
    assert abs(res["energies"]["Xc"] - float(E[1])) < 1e-9, (res["energies"]["Xc"], float(E[1]))
    mag = float((rho[0] - rho[1]).sum() * db.dvol)
    print(f"[iron PBE collinear] E_total = {res['energies'].total:.10f} Ha, magnetisation = {mag:.6f} mu_B, "
          f"n_iter = {res['n_iter']}, E_xc = {res['energies']['Xc']:.10f}")
    assert abs(mag) > 0.5
    # the opposite starting moment: the same energy, the channels exchanged (both runs stop at a density residual of 1e-9;
    # the densities are compared at the 1e-7 of the other collinear tests)
    db2 = iron_pbe_basis(-4.0)
    res2 = dftk.self_consistent_field(db2, rho=dftk.guess_density(db2, (-4.0,)), tol=1e-9)
    assert res2["converged"]
    assert abs(res2["energies"].total - res["energies"].total) < 1e-8
    rho2 = res2["rho"].cpu().numpy()
    assert np.linalg.norm(rho2[0] - rho[1]) * np.sqrt(db.dvol) < 1e-7 and np.linalg.norm(rho2[1] - rho[0]) * np.sqrt(db.dvol) < 1e-7
    mag2 = float((rho2[0] - rho2[1]).sum() * db.dvol)
    assert abs(mag2 + mag) < 1e-6 and mag * mag2 < 0
    # the wire format and an .npz round trip of a PBE collinear result (nothing in io.py had to be touched)
    d = dftk.scfres_to_dict(res)
    assert np.array(d["eigenvalues"]).shape[:2] == (2, 6) and np.array(d["ρ"]).shape == (2, 20, 20, 20)
    assert d["spin_polarization"] == "collinear" and d["n_spin_components"] == 2
    fn = str(tmp_path / "iron_pbe.npz")
    dftk.save_scfres(fn, res)
    back = dftk.load_scfres(fn, db)
    assert len(back["psi"]) == len(db.kpoints) == 12 and torch.equal(back["rho"].cpu(), res["rho"].cpu())
    for p, q in zip(back["psi"], res["psi"]):
        assert torch.equal(p, q)
    again = dftk.self_consistent_field(db, rho=back["rho"], psi=back["psi"], tol=1e-8)
    assert again["converged"] and abs(again["energies"].total - res["energies"].total) < 1e-8
    # stresses of a collinear PBE model stay refused (dftk_mi_stress_xc takes the gradient of one spin component)
    with pytest.raises(NotImplementedError):
        dftk.compute_stresses_cart(res)


def test_vwn_with_spin_stays_refused():
    """lda_c_vwn has no spin-polarised form in the library"""
    lat, atoms, pos = dftk.silicon_cell()
    kg = dftk.ExplicitKpoints([[0, 0, 0]], [1.0])
    m = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"), spin_polarization="collinear")
    b = dftk.PlaneWaveBasis(m, 5, kg, fft_size=(12, 12, 12))
    rho = dftk.guess_density(b)
    with pytest.raises(NotImplementedError):
        dftk.energy_hamiltonian(b, None, None, rho=rho)
