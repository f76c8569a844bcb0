"""What a meta-GGA model is refused, decided on descriptors before any device work: every case is raised on a model or basis
built without a GPU (``device="cpu"``), with its message matched."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402

SCAN = ("mgga_x_scan", "mgga_c_scan")


def scan_model(**kw):
    lat, atoms, pos = dftk.silicon_cell(functional="pbe")
    return dftk.model_DFT(lat, atoms, pos, functionals=kw.pop("functionals", SCAN), **kw)


@pytest.fixture(scope="module")
def basis():
    return dftk.PlaneWaveBasis(scan_model(), 5, dftk.ExplicitKpoints([[0.0, 0.0, 0.0]], [1.0]), device="cpu")


def test_the_two_names_are_known():
    m = scan_model()
    assert m.uses_tau and m.functionals == SCAN
    assert scan_model(functionals=("mgga_x_scan",)).uses_tau
    assert not scan_model(functionals=("gga_x_pbe", "gga_c_pbe")).uses_tau


@pytest.mark.parametrize("name", ["mgga_x_tpss", "mgga_c_r2scan", "mgga_x_r2scan", "hyb_mgga_x_scan0"])
def test_other_meta_gga_names(name):
    with pytest.raises(NotImplementedError, match="meta-GGA"):
        scan_model(functionals=(name, "mgga_c_scan"))


def test_collinear_spin():
    with pytest.raises(NotImplementedError, match="meta-GGA with collinear spin"):
        scan_model(magnetic_moments=[1.0, -1.0])
    with pytest.raises(NotImplementedError, match="meta-GGA with collinear spin"):
        scan_model(spin_polarization="collinear")


def test_hubbard_and_exact_exchange():
    lat, atoms, pos = dftk.silicon_cell(functional="pbe")
    base = ["Kinetic", "AtomicLocal", "AtomicNonlocal", "Ewald", "PspCorrection", "Hartree", "Xc"]
    for extra in ("ExactExchange", "Hubbard"):
        with pytest.raises(NotImplementedError, match="meta-GGA together with a Hubbard or ExactExchange"):
            dftk.Model(lat, atoms, pos, base + [extra], functionals=SCAN)


def test_core_correction():
    class Psp:
        identifier = "fake-upf-with-core"

        def has_core_density(self):
            return True

    class Atom:
        symbol, charge_ionic, psp = "Si", 4, Psp()
    lat, _, pos = dftk.silicon_cell()
    with pytest.raises(NotImplementedError, match="meta-GGA with a pseudopotential that carries a core correction"):
        dftk.Model(lat, [Atom(), Atom()], pos, ["Kinetic", "Xc"], functionals=SCAN)


def test_gamma_real_and_communicators():
    kg = dftk.ExplicitKpoints([[0.0, 0.0, 0.0]], [1.0])
    with pytest.raises(NotImplementedError, match="gamma_real=True is not available for meta-GGA"):
        dftk.PlaneWaveBasis(scan_model(), 5, kg, device="cpu", gamma_real=True)

    class TwoRanks:
        size, rank = 2, 0
    for kw in (dict(comm_pw=TwoRanks()), dict(comm_kpts=TwoRanks())):
        with pytest.raises(NotImplementedError, match="meta-GGA functionals run on one rank"):
            dftk.PlaneWaveBasis(scan_model(), 5, kg, device="cpu", **kw)


def test_post_processing_and_other_solvers(basis):
    rho = torch.zeros(tuple(reversed(basis.fft_size)), dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="stress tensor.*meta-GGA"):
        dftk.compute_stresses_cart(basis, None, None, rho)
    with pytest.raises(NotImplementedError, match="density response.*meta-GGA"):
        dftk.apply_kernel(basis, rho, rho=rho)
    with pytest.raises(NotImplementedError, match="density response.*meta-GGA"):
        dftk.apply_chi0_4P([type("H", (), {"basis": basis})()], None, None, 0.0, None, None)
    with pytest.raises(NotImplementedError, match="density response.*meta-GGA"):
        dftk.solve_OmegaPlusK_split(dict(basis=basis), None)
    with pytest.raises(NotImplementedError, match="refine_scfres.*meta-GGA"):
        dftk.refine_scfres(dict(basis=basis), basis)
    with pytest.raises(NotImplementedError, match="dynamical matrix.*meta-GGA"):
        dftk.compute_dynmat(dict(basis=basis))
    with pytest.raises(NotImplementedError, match="direct_minimization.*meta-GGA"):
        dftk.direct_minimization(basis)
    with pytest.raises(NotImplementedError, match="Chi0Mixing.*meta-GGA"):
        dftk.Chi0Mixing([]).mix_density(basis, rho)
    with pytest.raises(NotImplementedError, match="Chi0Mixing.*meta-GGA"):
        dftk.ScfStepper(basis, rho=rho, mixing=dftk.Chi0Mixing([]))


def test_tau_without_a_functional_of_it():
    lat, atoms, pos = dftk.silicon_cell()
    b = dftk.PlaneWaveBasis(dftk.model_DFT(lat, atoms, pos), 5, dftk.ExplicitKpoints([[0.0, 0.0, 0.0]], [1.0]), device="cpu")
    rho = torch.zeros(tuple(reversed(b.fft_size)), dtype=torch.float64)
    with pytest.raises(ValueError, match="tau given, but the model has no meta-GGA functional"):
        dftk.ScfStepper(b, rho=rho, tau=rho)
    assert dftk.guess_kinetic_energy_density(b, rho) is None
