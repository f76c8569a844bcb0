"""Band structures and projected densities of states, the part that needs no GPU: the PP_PSWFC reader, the host transform
of the pseudo-atomic wavefunctions against their closed forms, k-path interpolation, band counts, ``sum_pdos``, every refusal
that is decided before the device is touched, and the NumPy twin of the orbital path (tests/pswfc_gen.py) against itself."""
import math

import numpy as np
import pytest
import torch

import dftk_jl_amd as dftk
from dftk_jl_amd import psp as psp_mod
from dftk_jl_amd import psp_upf
from dftk_jl_amd.comm import KptComm

import pswfc_gen
import upf_gen
from test_upf_host import E_QUAD

DISPLACED = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]


# ------------------------------------------------------------------------------------------------ reader
@pytest.fixture(scope="module")
def si3():
    return pswfc_gen.pswfc_psp(("3S", "3P", "4S"))


def test_reader_round_trip(si3):
    u = si3
    r = upf_gen.uniform_mesh(pswfc_gen.N_MESH, pswfc_gen.R_MAX)
    assert u.count_n_pswfc() == 1 + 3 + 1
    assert [u.count_n_pswfc_radial(l) for l in range(u.lmax + 1)] == [2, 1]
    assert u.count_n_pswfc_radial(3) == 0
    assert u.pswfc_label(1, 0) == "3S" and u.pswfc_label(2, 0) == "4S" and u.pswfc_label(1, 1) == "3P"
    assert u.find_pswfc("3S") == (0, 1) and u.find_pswfc("4S") == (0, 2) and u.find_pswfc("3P") == (1, 1)
    with pytest.raises(ValueError, match="5D"):
        u.find_pswfc("5D")
    for label in ("3S", "3P", "4S"):
        l, i = u.find_pswfc(label)
        _, _, occ, energy = pswfc_gen.ORBITALS[label]
        np.testing.assert_allclose(u.r2_pswfcs[l][i - 1], r * pswfc_gen.orbital_chi(label, r), rtol=4e-16, atol=1e-300)
        assert u.pswfc_occs[l][i - 1] == occ and u.pswfc_energies[l][i - 1] == energy
        rr, wf = u.pswfc_channel(l, i - 1)
        assert len(rr) == len(r) and np.array_equal(wf, u.weights(len(r)) * u.r2_pswfcs[l][i - 1])


def test_order_of_n_within_l_is_the_files():
    u = pswfc_gen.pswfc_psp(("4S", "3P", "3S"))
    assert u.pswfc_labels[0] == ["4S", "3S"] and u.pswfc_labels[1] == ["3P"]
    assert u.find_pswfc("3S") == (0, 2)
    assert pswfc_gen.pswfc_psp(("3S",), energies=False).pswfc_energies[0] == [None]


def test_channels_are_not_cut_at_rcut():
    text = pswfc_gen.pswfc_text(("3S", "3P"))
    u = dftk.PspUpf(text, rcut=10.0)
    assert u.ircut < len(u.rgrid)
    r, wf = u.pswfc_channel(0, 0)
    assert len(r) == len(u.rgrid) == len(wf)
    assert len(u.projector_channel(0, 0)[0]) == u.ircut


def test_file_without_the_block_parses_as_before():
    text = pswfc_gen.pswfc_text(("3S", "3P"))
    a, b = dftk.parse_psp_upf(text, identifier="x"), dftk.parse_psp_upf(pswfc_gen.strip_pswfc(text), identifier="x")
    assert b.count_n_pswfc() == 0 and b.r2_pswfcs == [[], []] and a.count_n_pswfc() == 4
    for name in ("Zion", "lmax", "rcut", "ircut"):
        assert getattr(a, name) == getattr(b, name)
    for name in ("rgrid", "drgrid", "vloc", "r2_rhoion", "r2_rhocore"):
        assert np.array_equal(getattr(a, name), getattr(b, name))
    for l in range(a.lmax + 1):
        assert np.array_equal(a.h[l], b.h[l])
        assert all(np.array_equal(x, y) for x, y in zip(a.r2_projs[l], b.r2_projs[l]))
    # the block that upf_gen writes by default (one 3S orbital r exp(-r)) is read too
    hgh = dftk.load_psp("Si", "lda")
    r = upf_gen.log_mesh(200)
    c = dftk.parse_psp_upf(upf_gen.write_upf(hgh, r))
    assert c.count_n_pswfc() == 1 and c.pswfc_label(1, 0) == "3S" and c.pswfc_occs[0] == [2.0]
    np.testing.assert_allclose(c.r2_pswfcs[0][0], r * r * np.exp(-r), rtol=4e-16)


def test_hgh_has_no_orbitals():
    hgh = dftk.load_psp("Si", "lda")
    assert hgh.count_n_pswfc() == 0 and hgh.count_n_pswfc_radial(0) == 0
    with pytest.raises(ValueError):
        psp_mod.eval_psp_pswfc_fourier(hgh, 1, 0, torch.zeros(1, dtype=torch.float64))


def test_pswfc_transform_against_closed_form(si3):
    """host sum and the twin's Simpson rule against 4 pi sqrt(pi/2) a^(2l+3) exp(-q^2 a^2 / 2), within E_QUAD of
    tests/test_upf_host.py times the channel's largest value (the measured figures are in the header of tests/pswfc_gen.py)"""
    q = np.concatenate([[0.0, 1e-8, 1e-3], np.linspace(0.05, 12.0, 240)])
    r = si3.rgrid
    w = upf_gen.twin_weights(r)
    for label in ("3S", "3P", "4S"):
        l, i = si3.find_pswfc(label)
        want = pswfc_gen.closed_form(label)(q)
        host = psp_upf.eval_psp_pswfc_fourier_upf(si3, i, l, q)
        via_psp = psp_mod.eval_psp_pswfc_fourier(si3, i, l, torch.from_numpy(q)).numpy()
        twin = upf_gen.twin_hankel(r, w * si3.r2_pswfcs[l][i - 1], l, q)
        scale = np.max(np.abs(want))
        eh, et = np.max(np.abs(host - want)) / scale, np.max(np.abs(twin - want)) / scale
        print(f"{label}: host {eh:.2e}, twin {et:.2e} (relative to the channel's largest value)")
        assert np.array_equal(host, via_psp)
        assert eh <= E_QUAD and et <= E_QUAD, (label, eh, et)


# ------------------------------------------------------------------------------------------------ k-paths, counts, sums
class _Model:
    def __init__(self, lattice):
        self.lattice = np.asarray(lattice, dtype=float)
        self.recip_lattice = 2 * math.pi * np.linalg.inv(self.lattice.T)


TRICLINIC = _Model(np.array([[5.0, 0.7, -0.3], [0.2, 6.1, 0.9], [0.4, -0.5, 7.3]]).T)


def _check_path(model, kpath, density):
    ki = dftk.kpath_interpolate(model, kpath, density)
    kc, dist = np.array(ki["kcoords"]), ki["kdistances"]
    B = model.recip_lattice
    at = 0
    pos = []
    for path in kpath.paths:
        pos.append((at, path[0]))
        for a, b in zip(path[:-1], path[1:]):
            ka, kb = np.asarray(kpath.points[a], float), np.asarray(kpath.points[b], float)
            n = max(2, math.ceil(np.linalg.norm(B @ (kb - ka)) * density))
            np.testing.assert_allclose(kc[at:at + n], ka + np.linspace(0, 1, n)[:, None] * (kb - ka), atol=1e-14)
            assert np.array_equal(kc[at + n - 1], kb)
            at += n - 1
            pos.append((at, b))
        at += 1
    assert at == len(kc) == len(dist)
    assert ki["labels"] == pos
    assert [len(b) for b in ki["branches"]] and sum(len(b) for b in ki["branches"]) == len(kc)
    assert np.all(np.diff(dist) >= 0) and dist[0] == 0
    return ki


def test_kpath_interpolate_triclinic():
    pts = {"G": [0, 0, 0], "X": [0.5, 0, 0], "M": [0.5, 0.5, 0], "R": [0.5, 0.5, 0.5], "tiny": [0.5, 0.5, 0.501]}
    ki = _check_path(TRICLINIC, dftk.KPath(pts, [["G", "X", "M", "G", "R"]]), 17.0)
    kc, dist = np.array(ki["kcoords"]), ki["kdistances"]
    # no joint twice, distances are the Cartesian lengths
    assert np.all(np.linalg.norm(np.diff(kc, axis=0), axis=1) > 0)
    steps = np.linalg.norm(np.diff(kc, axis=0) @ TRICLINIC.recip_lattice.T, axis=1)
    np.testing.assert_allclose(np.diff(dist), steps, rtol=1e-12)
    # a segment shorter than one spacing still has its two ends
    short = dftk.kpath_interpolate(TRICLINIC, dftk.KPath(pts, [["R", "tiny"]]), 1.0)
    assert len(short["kcoords"]) == 2


def test_kpath_two_branches():
    lat, _, _ = dftk.silicon_cell()
    model = _Model(lat)
    pts = {"L": [0.5, 0.5, 0.5], "G": [0, 0, 0], "X": [0.5, 0, 0.5], "U": [0.625, 0.25, 0.625], "K": [0.375, 0.375, 0.75]}
    ki = _check_path(model, dftk.KPath(pts, [["L", "G", "X", "U"], ["K", "G"]]), 12.0)
    b0, b1 = ki["branches"]
    assert b1[0] == b0[-1] + 1 and ki["labels"][3] == (b0[-1], "U") and ki["labels"][4] == (b1[0], "K")
    # the second branch starts at the distance the first one ended at: no jump across U | K
    assert ki["kdistances"][b1[0]] == ki["kdistances"][b0[-1]]
    assert np.all(np.diff(ki["kdistances"][b1[0]:]) > 0)
    with pytest.raises(ValueError):
        dftk.kpath_interpolate(model, dftk.KPath(pts, [["G"]]), 12.0)


def test_default_n_bands_bandstructure():
    for n in (1, 4, 7, 100):
        assert dftk.default_n_bands_bandstructure(n) == math.ceil(n + 5 * math.sqrt(n))
    assert dftk.default_n_bands_bandstructure(4) == 14 and dftk.default_n_bands_bandstructure(7) == 21
    lat, atoms, pos = dftk.silicon_cell()
    assert dftk.default_n_bands_bandstructure(dftk.model_DFT(lat, atoms, pos)) == 14          # 4 SCF bands
    assert dftk.default_n_bands_bandstructure(dict(occupation=[np.zeros(7)])) == 21


def test_sum_pdos():
    rng = np.random.default_rng(0)
    labels = pswfc_gen.twin_labels([("3S", "3P"), ("3S", "3P")])
    res = dict(pdos=rng.random((5, len(labels), 2)), projector_labels=labels, eps=np.arange(5.0))
    p = dftk.sum_pdos(res, [lambda o: o["l"] == 1 and o["iatom"] == 0])
    np.testing.assert_array_equal(p, res["pdos"][:, 1:4, :].sum(axis=1))
    # a column that two filters accept is counted once; no filter, no column
    both = dftk.sum_pdos(res, [lambda o: o["label"] == "3S", lambda o: o["l"] == 0, lambda o: o["m"] == 1])
    cols = [j for j, o in enumerate(labels) if o["l"] == 0 or o["m"] == 1]
    np.testing.assert_allclose(both, res["pdos"][:, cols, :].sum(axis=1), rtol=1e-15)
    assert np.array_equal(dftk.sum_pdos(res, []), np.zeros((5, 2)))


# ------------------------------------------------------------------------------------------------ refusals
def _cpu_basis(psp=None, kgrid=None, **kw):
    lat, atoms, _ = dftk.silicon_cell()
    if psp is not None:
        atoms = [dftk.ElementPsp("Si", psp=psp)] * 2
    mk = {k: kw.pop(k) for k in list(kw) if k in ("temperature", "smearing")}
    model = dftk.model_DFT(lat, atoms, DISPLACED, functionals=("lda_x", "lda_c_vwn"), **mk)
    return dftk.PlaneWaveBasis(model, 5, kgrid or dftk.MonkhorstPack((2, 1, 1)), device="cpu", build_terms=False, **kw)


GX = dftk.ExplicitKpoints([[0, 0, 0], [0.25, 0, 0.25]], [0.5, 0.5])


def test_refusals_without_a_device():
    basis = _cpu_basis()
    with pytest.raises(ValueError, match="converged density is required"):
        dftk.compute_bands(basis, GX)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dftk.compute_bands(basis, GX, rho=torch.zeros(1))
    lat, atoms, pos = dftk.silicon_cell()
    gamma = dftk.ExplicitKpoints([[0, 0, 0]], [1.0])
    for model in (dftk.model_HF(lat, atoms, pos), dftk.model_DFT(lat, atoms, pos, functionals=dftk.PBE0())):
        bx = dftk.PlaneWaveBasis(model, 5, gamma, device="cpu", build_terms=False)
        with pytest.raises(NotImplementedError, match="exact exchange"):
            dftk.compute_bands(bx, GX, rho=torch.zeros(1))
        with pytest.raises(NotImplementedError, match="exact exchange"):
            dftk.compute_bands(dict(basis=bx, rho=torch.zeros(1), eF=0.0, occupation=[np.zeros(4)]), GX)
    with pytest.raises(NotImplementedError, match="comm_kpts"):
        dftk.compute_bands(_cpu_basis(comm_kpts=KptComm(0, 2)), GX, rho=torch.zeros(1))
    with pytest.raises(NotImplementedError, match="comm_pw"):
        dftk.compute_bands(_cpu_basis(kgrid=gamma, comm_pw=KptComm(0, 2)), GX, rho=torch.zeros(1))
    with pytest.raises(TypeError):
        dftk.compute_bands(basis, [[0, 0, 0]], rho=torch.zeros(1))


def test_orbital_refusals_without_a_device():
    hgh_basis = _cpu_basis(temperature=0.01)
    with pytest.raises(ValueError, match=r"atom 0 \(Si\).*PspHgh"):
        dftk.atomic_orbital_projectors(hgh_basis)
    with pytest.raises(ValueError, match="no pseudo-atomic orbitals"):
        dftk.atomic_orbital_projections(hgh_basis, [None, None])
    with pytest.raises(ValueError, match="no pseudo-atomic orbitals"):
        dftk.compute_pdos([0.0], hgh_basis, psi=[None, None], eigenvalues=[np.zeros(2)] * 2)
    upf = pswfc_gen.pswfc_psp()
    cold = _cpu_basis(psp=upf)
    with pytest.raises(ValueError, match="finite temperature"):
        dftk.compute_pdos([0.0], cold, psi=[None, None], eigenvalues=[np.zeros(2)] * 2)
    with pytest.raises(ValueError, match="finite temperature"):
        dftk.compute_pdos([0.0], dict(basis=cold, psi=[None, None], eigenvalues=[np.zeros(2)] * 2), temperature=0.0,
                          smearing="gaussian")
    with pytest.raises(ValueError, match="finite temperature"):
        dftk.compute_pdos([0.0], _cpu_basis(psp=upf, temperature=0.01, smearing="none"), psi=[None], eigenvalues=[None])
    warm = _cpu_basis(psp=upf, temperature=0.01)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dftk.compute_pdos([0.0], warm, psi=[None, None], eigenvalues=[np.zeros(2)] * 2)
    with pytest.raises(NotImplementedError, match="comm_kpts"):
        dftk.atomic_orbital_projectors(_cpu_basis(psp=upf, comm_kpts=KptComm(0, 2)))
    # nothing selected
    with pytest.raises(ValueError, match="no orbital selected"):
        dftk.atomic_orbital_projectors(warm, isonmanifold=lambda o: False)


# ------------------------------------------------------------------------------------------------ the twin against itself
@pytest.fixture(scope="module")
def twin_case():
    basis = _cpu_basis(psp=pswfc_gen.pswfc_psp(), kgrid=dftk.MonkhorstPack((2, 2, 1)), temperature=0.01)
    model = basis.model
    rng = np.random.default_rng(5)
    per_atom = [("3S", "3P"), ("3S", "3P")]
    Phis, projs, eigs = [], [], []
    for kpt in basis.kpoints:
        G = kpt.G_vectors.numpy()
        Phi = pswfc_gen.twin_orbitals(G, kpt.coordinate, model.recip_lattice, model.unit_cell_volume, model.positions,
                                      per_atom)
        Phi_t, lam = pswfc_gen.twin_lowdin(Phi)
        psi = np.linalg.qr(rng.standard_normal((len(G), 10)) + 1j * rng.standard_normal((len(G), 10)))[0]
        Phis.append((Phi, Phi_t, lam))
        projs.append(pswfc_gen.twin_projections(Phi_t, psi))
        eigs.append(np.sort(rng.uniform(-0.3, 0.4, 10)))
    return basis, Phis, projs, eigs


def test_twin_orbitals_are_orthonormal_and_span_the_same_space(twin_case):
    _, Phis, _, _ = twin_case
    for Phi, Phi_t, lam in Phis:
        assert Phi.shape[1] == 8 and lam.min() > 0
        err = np.max(np.abs(Phi_t.conj().T @ Phi_t - np.eye(8)))
        print(f"|Phi~' Phi~ - I| = {err:.2e}, cond(S) = {lam.max() / lam.min():.2e}")
        assert err <= 8 * 2.0 ** -52 * lam.max() / lam.min()
        # Loewdin: Phi~ = Phi S^-1/2 is the orthonormal set closest to Phi, and Phi~' Phi = S^1/2 is Hermitian positive
        M = Phi_t.conj().T @ Phi
        assert np.max(np.abs(M - M.conj().T)) <= 1e-12 * np.max(np.abs(M)) and np.linalg.eigvalsh((M + M.conj().T) / 2).min() > 0


def test_twin_sum_rule(twin_case):
    _, _, projs, _ = twin_case
    for p in projs:
        tot = p.sum(axis=1)
        print(f"sum_p |c_p|^2 per band in [{tot.min():.3e}, {tot.max():.3e}]")
        assert np.all(p >= 0) and np.all(tot <= 1 + 1e-12)


def test_twin_pdos_integrates_to_the_projections(twin_case):
    """Gaussian smearing: the trapezoid rule of step T/2 reaching 12 T beyond the extreme eigenvalues integrates every band's
    Gaussian to 1 within 2 exp(-4 pi^2) ~ 1e-17, so the integral of the PDOS is filled_occ sum_k w_k sum_n |c_pn|^2."""
    basis, _, projs, eigs = twin_case
    T = 0.01
    lo, hi = min(e.min() for e in eigs) - 12 * T, max(e.max() for e in eigs) + 12 * T
    eps = lo + (T / 2) * np.arange(int(math.ceil((hi - lo) / (T / 2))) + 1)
    D = pswfc_gen.twin_pdos(eps, projs, eigs, basis.kweights, [k.spin for k in basis.kpoints],
                            basis.model.filled_occupation, "gaussian", T)
    got = (T / 2) * (D[:, :, 0].sum(axis=0) - 0.5 * (D[0, :, 0] + D[-1, :, 0]))
    want = basis.model.filled_occupation * sum(w * p.sum(axis=0) for w, p in zip(basis.kweights, projs))
    err = np.max(np.abs(got - want) / want)
    print(f"trapezoid integral of the twin's PDOS against the projections: {err:.2e} relative")
    assert err <= 1e-10
    # and pointwise the sum over an orthonormal set never exceeds the DOS of the same bands
    dos = np.array([dftk.compute_dos(e, basis, eigs, smearing="gaussian", temperature=T)[0] for e in eps[::40]])
    assert np.all(D[::40, :, 0].sum(axis=1) <= dos + 1e-12)
