"""UPF pseudopotentials end to end on the device: GTH silicon written as a UPF file (tests/upf_gen.py) against the HGH
table it was made from -- set-up arrays, SCF energies / eigenvalues / forces, forces against differences of the SCF energy,
every block kind, a mixed HGH + UPF cell, and the refusals.

Bounds.  The two pseudopotentials differ by the quadrature error of the file's mesh, E_QUAD (tests/test_upf_host.py).  The
set-up arrays are compared within 10 x E_QUAD x their scale.  For the SCF results the bound is 10 x the first-order
estimate of what the twin's form-factor errors induce in the energy of the HGH state (local energy of the differences,
nonlocal energy with the projector differences, the energy correction), computed on the CPU, with the SCF tolerance as its
floor, 1e-10, for every compared quantity."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import psp as psp_mod  # noqa: E402
from dftk_jl_amd.terms import atom_decay_length  # noqa: E402

import upf_gen  # noqa: E402
from test_upf_host import E_QUAD, N_MESH  # noqa: E402

FUN = ("lda_x", "lda_c_vwn")
PBE = ("gga_x_pbe", "gga_c_pbe")
DISPLACED = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]
ECUT = 7
TOL = 1e-10


def _upf(functional="lda", rhoatom=True):
    hgh = dftk.load_psp("Si", functional)
    r = upf_gen.uniform_mesh(N_MESH, 30.0)
    rho = upf_gen.gaussian_density_real(4.0, atom_decay_length(10, 4), r) if rhoatom else None
    return hgh, dftk.parse_psp_upf(upf_gen.write_upf(hgh, r, rhoatom=rho), identifier=f"si-{functional}-{rhoatom}.upf")


@pytest.fixture(scope="module")
def si():
    return _upf()


def _kgrid(gamma):
    return dftk.ExplicitKpoints([[0, 0, 0]], [1.0]) if gamma else dftk.MonkhorstPack((2, 2, 2)).reducible()


def _basis(psp, positions=DISPLACED, gamma=False, functionals=FUN, fft_size=None, **kw):
    lat, _, _ = dftk.silicon_cell()
    mk = {k: kw.pop(k) for k in list(kw) if k in ("magnetic_moments", "spin_polarization")}
    model = dftk.model_DFT(lat, [dftk.ElementPsp("Si", psp=psp)] * 2, positions, functionals=functionals, **mk)
    return dftk.PlaneWaveBasis(model, ECUT, _kgrid(gamma), fft_size=fft_size, device="cuda:0", **kw)


def _scf(basis, **kw):
    res = dftk.self_consistent_field(basis, tol=kw.pop("tol", TOL), **kw)
    assert res["converged"]
    return res


# ------------------------------------------------------------------------------------------------ set-up
@pytest.mark.parametrize("gamma", [False, True], ids=["mp222", "gamma"])
def test_setup_arrays_match_hgh(si, gamma):
    hgh, upf = si
    bh, bu = _basis(hgh, gamma=gamma), _basis(upf, gamma=gamma)
    assert bh.fft_size == bu.fft_size and len(bh.kpoints) == len(bu.kpoints)
    Th, Tu = bh.terms, bu.terms
    Vh, Vu = Th.V_loc.cpu().numpy(), Tu.V_loc.cpu().numpy()
    print("V_loc", np.max(np.abs(Vu - Vh)) / np.max(np.abs(Vh)))
    assert np.max(np.abs(Vu - Vh)) <= 10 * E_QUAD * np.max(np.abs(Vh))
    assert np.array_equal(Tu.D, Th.D) or np.max(np.abs(Tu.D - Th.D)) <= 10 * E_QUAD * np.max(np.abs(Th.D))
    for Ph, Pu in zip(Th.P, Tu.P):
        Ph, Pu = Ph.cpu().numpy(), Pu.cpu().numpy()
        assert Ph.shape == Pu.shape
        for c in range(Ph.shape[0]):
            assert np.max(np.abs(Pu[c] - Ph[c])) <= 10 * E_QUAD * np.max(np.abs(Ph[c])), c
    assert abs(Tu.E_pspcorr - Th.E_pspcorr) <= 10 * E_QUAD * abs(Th.E_pspcorr)
    rh, ru = dftk.guess_density(bh).cpu().numpy(), dftk.guess_density(bu).cpu().numpy()
    print("guess density", np.max(np.abs(ru - rh)) / np.max(np.abs(rh)))
    assert np.max(np.abs(ru - rh)) <= 10 * E_QUAD * np.max(np.abs(rh))
    # a file without PP_RHOATOM keeps the Gaussian guess: the same library call as HGH, bit for bit
    _, bare = _upf(rhoatom=False)
    assert np.array_equal(dftk.guess_density(_basis(bare, gamma=gamma)).cpu().numpy(), rh)


def test_torch_setup_path_matches_the_library_entries(si, monkeypatch):
    """DFTK_MI_TORCH_SETUP: V_loc, P and the guess density of a UPF model through the torch constructions (host quadrature
    values) against the table entries of the library"""
    _, upf = si
    ba = _basis(upf)
    monkeypatch.setenv("DFTK_MI_TORCH_SETUP", "1")
    bt = _basis(upf, fft_size=ba.fft_size)
    Va, Vt = ba.terms.V_loc.cpu().numpy(), bt.terms.V_loc.cpu().numpy()
    assert np.max(np.abs(Vt - Va)) <= 10 * E_QUAD * np.max(np.abs(Va))
    for Pa, Pt in zip(ba.terms.P, bt.terms.P):
        Pa, Pt = Pa.cpu().numpy(), Pt.cpu().numpy()
        for c in range(Pa.shape[0]):
            assert np.max(np.abs(Pt[c] - Pa[c])) <= 10 * E_QUAD * np.max(np.abs(Pa[c])), c
    rt = dftk.guess_density(bt).cpu().numpy()
    monkeypatch.delenv("DFTK_MI_TORCH_SETUP")
    ra = dftk.guess_density(ba).cpu().numpy()
    assert np.max(np.abs(rt - ra)) <= 10 * E_QUAD * np.max(np.abs(ra))


def test_spin_density_guess_matches_hgh(si):
    """per-atom coefficients (magnetic moments) through the table entry: the file's PP_RHOATOM is the Gaussian of the HGH
    guess, so the two collinear guesses must agree"""
    hgh, upf = si
    mm = [1.5, -0.5]
    bh = _basis(hgh, functionals=("lda_x", "lda_c_pw"), magnetic_moments=mm)
    bu = _basis(upf, functionals=("lda_x", "lda_c_pw"), magnetic_moments=mm, fft_size=bh.fft_size)
    rh, ru = dftk.guess_density(bh, mm).cpu().numpy(), dftk.guess_density(bu, mm).cpu().numpy()
    assert rh.shape[0] == 2 and np.max(np.abs(rh[0] - rh[1])) > 1e-3
    assert np.max(np.abs(ru - rh)) <= 10 * E_QUAD * np.max(np.abs(rh))


# ------------------------------------------------------------------------------------------------ SCF
def _first_order_estimate(bh, res, hgh, upf):
    """|dE| to first order in the twin's form-factor differences, from the HGH state, on the CPU."""
    model = bh.model
    tw = upf_gen.twin_channels(upf)
    atoms = [(0, np.asarray(p)) for p in model.positions]
    rho = res["rho"].cpu().numpy()
    rho = rho if rho.ndim == 3 else rho.sum(axis=0)

    def closed_local(q):
        return psp_mod.eval_psp_local_fourier(hgh, torch.from_numpy(np.ascontiguousarray(q))).numpy()

    def d_local(q):
        u, inv = np.unique(q, return_inverse=True)
        return (upf_gen.twin_local(*tw["local"], hgh.Zion, u) - closed_local(u))[inv]

    dE_loc = upf_gen.twin_local_energy(bh.fft_size, model.recip_lattice, model.unit_cell_volume, [d_local], atoms, rho)

    def d_radial(l, i):
        def f(q):
            u, inv = np.unique(q, return_inverse=True)
            want = psp_mod.eval_psp_projector_fourier(hgh, i + 1, l, torch.from_numpy(u)).numpy()
            return (upf_gen.twin_hankel(*tw[(l, i)], l, u) - want)[inv]
        return f

    species = [[[d_radial(l, i) for i in range(hgh.count_n_proj_radial(l))] if l <= hgh.lmax else [] for l in range(4)]]
    dE_nl = 0.0
    for ik, kpt in enumerate(bh.kpoints):
        G = kpt.G_vectors.cpu().numpy()
        dP = upf_gen.twin_projectors(G, np.asarray(kpt.coordinate), model.recip_lattice, model.unit_cell_volume, species,
                                     atoms)
        P = bh.terms.P[ik].cpu().numpy().T
        psi = res["psi"][ik].cpu().numpy().T                       # (n_G, n_bands)
        occ = np.asarray(res["occupation"][ik], dtype=float)[:psi.shape[1]]
        a, b = P.conj().T @ psi, dP.conj().T @ psi
        dE_nl += bh.kweights[ik] * float(np.sum(occ * 2 * np.real(np.sum(a.conj() * (bh.terms.D @ b), axis=0))))
    dE_corr = (upf_gen.twin_energy_correction(upf) - psp_mod.eval_psp_energy_correction(hgh)) * len(atoms) * (
        sum(a.charge_ionic for a in model.atoms) / model.unit_cell_volume)
    return abs(dE_loc) + abs(dE_nl) + abs(dE_corr)


def _compare(rh, ru, est):
    b_tot = b_one = 10 * max(est, TOL)
    dE = abs(ru["energies"].total - rh["energies"].total)
    print(f"first-order estimate {est:.2e}; total energy differs by {dE:.2e} (bound {b_tot:.1e})")
    assert dE <= b_tot
    for name, v in rh["energies"].items():
        d = abs(ru["energies"][name] - v)
        print(f"  {name}: {d:.2e} (bound {b_one:.1e})")
        assert d <= b_one, name
    for eh, eu in zip(rh["eigenvalues"], ru["eigenvalues"]):
        n_occ = 4
        d = np.max(np.abs(np.asarray(eu)[:n_occ] - np.asarray(eh)[:n_occ]))
        assert d <= b_one, d
    Fh, Fu = dftk.compute_forces(rh), dftk.compute_forces(ru)
    print(f"  forces: {np.max(np.abs(Fu - Fh)):.2e} (bound {b_one:.1e}), largest {np.max(np.abs(Fh)):.2e}")
    assert np.max(np.abs(Fh)) > 1e-3                  # displaced off symmetry
    assert np.max(np.abs(Fu - Fh)) <= b_one


@pytest.fixture(scope="module")
def scf_222(si):
    hgh, upf = si
    bh, bu = _basis(hgh), _basis(upf)
    return bh, bu, _scf(bh), _scf(bu)


def test_scf_matches_hgh_mp222(si, scf_222):
    bh, bu, rh, ru = scf_222
    _compare(rh, ru, _first_order_estimate(bh, rh, *si))


def test_scf_matches_hgh_gamma(si):
    hgh, upf = si
    bh, bu = _basis(hgh, gamma=True), _basis(upf, gamma=True)
    rh, ru = _scf(bh), _scf(bu)
    _compare(rh, ru, _first_order_estimate(bh, rh, hgh, upf))


def test_scf_matches_hgh_pbe():
    hgh, upf = _upf("pbe")
    bh, bu = _basis(hgh, functionals=PBE), _basis(upf, functionals=PBE)
    rh, ru = _scf(bh), _scf(bu)
    _compare(rh, ru, _first_order_estimate(bh, rh, hgh, upf))


# ------------------------------------------------------------------------------------------------ forces
def test_forces_match_energy_differences(si, scf_222):
    """step and tolerance of tests/test_gpu_forces.py::test_total_forces_match_energy_finite_differences"""
    _, upf = si
    _, bu, _, ru = scf_222
    F = dftk.compute_forces(ru)
    d = np.random.default_rng(11).standard_normal((2, 3))
    d /= np.linalg.norm(d)
    eps = 1e-5

    def energy(sign):
        b = _basis(upf, [p + sign * eps * x for p, x in zip(DISPLACED, d)], fft_size=bu.fft_size)
        return _scf(b, tol=1e-11)["energies"].total
    assert abs(np.sum(F * d) + (energy(1) - energy(-1)) / (2 * eps)) < 1e-7
    Fc = dftk.compute_forces_cart(ru)
    assert np.allclose(Fc, F @ np.linalg.inv(bu.model.lattice), rtol=0, atol=1e-14)
    for name in ("AtomicLocal", "AtomicNonlocal", "Ewald"):
        assert dftk.compute_forces_term(name, bu, ru["psi"], ru["occupation"], rho=ru["rho"]).shape == (2, 3)


# ------------------------------------------------------------------------------------------------ block kinds
def test_gamma_real_matches_complex(si):
    _, upf = si
    b0 = _basis(upf, gamma=True, gamma_real=False)
    b1 = _basis(upf, gamma=True, gamma_real=True, fft_size=b0.fft_size)
    assert b1.kpoints[0].gamma_real and not b0.kpoints[0].gamma_real
    r0, r1 = _scf(b0), _scf(b1)
    assert abs(r1["energies"].total - r0["energies"].total) < 1e-9
    for name, v in r0["energies"].items():
        assert abs(r1["energies"][name] - v) < 1e-8, name
    assert np.max(np.abs(dftk.compute_forces(r1) - dftk.compute_forces(r0))) < 1e-8


def test_batched_kblocks_match_sequential(si, scf_222, monkeypatch):
    _, upf = si
    _, bu, _, ru = scf_222
    monkeypatch.setenv("DFTK_MI_KBATCH_SEQUENTIAL", "1")
    r1 = _scf(_basis(upf, fft_size=bu.fft_size))
    monkeypatch.delenv("DFTK_MI_KBATCH_SEQUENTIAL", raising=False)
    assert abs(ru["energies"].total - r1["energies"].total) < 1e-8
    assert abs(ru["eF"] - r1["eF"]) < 1e-7


def test_two_level_start_on_and_off(si):
    """(Ecut 16 and two k-points as tests/test_gpu_two_level_start.py: the companion basis at Ecut / 4 must hold the bands)"""
    _, upf = si
    lat, _, _ = dftk.silicon_cell()
    model = dftk.model_DFT(lat, [dftk.ElementPsp("Si", psp=upf)] * 2, DISPLACED, functionals=FUN)
    kg = dftk.ExplicitKpoints([[0.0, 0.25, -0.5], [0.25, 0.25, 0.0]], [0.5, 0.5])
    b2 = dftk.PlaneWaveBasis(model, 16.0, kg, device="cuda:0", coarse_start=True)
    b1 = dftk.PlaneWaveBasis(model, 16.0, kg, device="cuda:0", coarse_start=False, fft_size=b2.fft_size)
    assert b2.coarse is not None and b1.coarse is None      # the companion basis was built from the UPF model
    assert b2.coarse.terms.P[0].shape[0] == b2.terms.P[0].shape[0]
    r2, r1 = _scf(b2), _scf(b1)
    assert r2["converged"] and r1["converged"]
    assert abs(r2["energies"].total - r1["energies"].total) < 1e-9


def test_collinear_zero_moments_match_unpolarised(si, scf_222):
    _, upf = si
    _, bu, _, ru = scf_222
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        b2 = _basis(upf, fft_size=bu.fft_size, functionals=("lda_x", "lda_c_pw"), spin_polarization="collinear")
        b1 = _basis(upf, fft_size=bu.fft_size, functionals=("lda_x", "lda_c_pw"))
        r2, r1 = _scf(b2), _scf(b1)
    assert abs(r1["energies"].total - r2["energies"].total) < 1e-9
    assert np.max(np.abs(dftk.compute_forces(r2) - dftk.compute_forces(r1))) < 1e-8


# ------------------------------------------------------------------------------------------------ mixed cell
def test_mixed_cell_sic(si):
    hgh, upf = si
    lat, _, _ = dftk.silicon_cell()
    lat = np.asarray(lat) * (8.24 / 10.26)          # zincblende SiC is a wide-gap insulator at its own lattice constant
    carbon = dftk.ElementPsp("C", psp=dftk.load_psp("C", "lda"))

    def run(si_psp):
        model = dftk.model_DFT(lat, [dftk.ElementPsp("Si", psp=si_psp), carbon], DISPLACED, functionals=FUN)
        assert len(model.atom_groups) == 2
        basis = dftk.PlaneWaveBasis(model, ECUT, _kgrid(False), device="cuda:0")
        res = _scf(basis)
        assert res["converged"]
        return basis, res
    bh, rh = run(hgh)
    bu, ru = run(upf)
    # (the estimate counts the Si atom alone: the carbon tables of the mixed cell are the closed forms themselves)
    bound = 10 * max(E_QUAD * abs(rh["energies"].total), TOL)
    assert abs(ru["energies"].total - rh["energies"].total) <= bound
    Fh, Fu = dftk.compute_forces(rh), dftk.compute_forces(ru)
    print(f"SiC: energy differs by {abs(ru['energies'].total - rh['energies'].total):.2e}, forces by "
          f"{np.max(np.abs(Fu - Fh)):.2e} (bound {bound:.1e})")
    assert np.max(np.abs(Fh)) > 1e-3 and np.max(np.abs(Fu - Fh)) <= bound


# ------------------------------------------------------------------------------------------------ refusals
def test_stresses_and_phonons_refuse_upf(si):
    hgh, upf = si
    rh, ru = _scf(_basis(hgh, gamma=True)), _scf(_basis(upf, gamma=True))
    with pytest.raises(NotImplementedError, match="UPF"):
        dftk.compute_stresses_cart(ru)
    with pytest.raises(NotImplementedError, match="UPF"):
        dftk.compute_dynmat(ru)
    assert dftk.compute_stresses_cart(rh).shape == (3, 3)
    assert np.asarray(dftk.compute_dynmat(rh)).size == 36
