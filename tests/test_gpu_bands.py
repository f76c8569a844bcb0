"""Band structures and projected densities of states through the public interface, on the device.

Cell: displaced Si2 at Ecut 7 (as tests/test_gpu_upf.py).  Yardstick of the bands: the oracle's Hamiltonian blocks for the
same density at the same explicit k-points and fft_size, ``to_dense()``, ``numpy.linalg.eigh``; eigenvalues agree within 1e-7,
the bound tests/test_gpu_scf.py holds eigenvalues to.  Yardstick of the orbitals: the NumPy twin of tests/pswfc_gen.py (closed
form radial parts, Loewdin by eigh, the reference's loops); the generated UPF carries the orbitals 3S and 3P, whose quadrature
error is below E_QUAD of tests/test_upf_host.py.  Bounds of the orbital tests:
  Phi~       (10 E_QUAD + L) max |Phi~|, L = 8 max(the twin's own orthonormality defect, n_proj 2^-52 sqrt(cond S)): the Loewdin
             bound of tests/test_gpu_pdos_kernels.py with the twin's defect standing for its (unmeasured) error;
  |C|^2      2 |C| dC + dC^2 with dC = |psi_n| sqrt(n_G) (the Phi~ bound) + 8 n_G 2^-52 |psi_n| |phi_p|;
  PDOS       16 x 2^-52 weight sum |g| |C|^2 per k-block (the kernel's bound) + weight sum |g| d|C|^2.
Every test prints what it measured (``pytest -s``)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd.mixing import occupation_derivative  # noqa: E402
import oracle  # noqa: E402

import pswfc_gen  # noqa: E402
from test_upf_host import E_QUAD  # noqa: E402

LDA = ("lda_x", "lda_c_vwn")
PBE = ("gga_x_pbe", "gga_c_pbe")
DISPLACED = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]
ECUT = 7
U = 2.0 ** -52
GX9 = [[0.5 * t, 0.0, 0.5 * t] for t in np.linspace(0, 1, 9)]
N_BANDS = 8


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.manual_seed(20240917)


def explicit(kcoords):
    return dftk.ExplicitKpoints([list(k) for k in kcoords], [1.0 / len(kcoords)] * len(kcoords))


def si_basis(psp=None, functionals=LDA, kgrid=None, table="lda", **kw):
    lat, _, _ = dftk.silicon_cell()
    psp = dftk.load_psp("Si", table) if psp is None else psp
    mk = {k: kw.pop(k) for k in list(kw) if k in ("magnetic_moments", "spin_polarization", "temperature", "smearing")}
    model = dftk.model_DFT(lat, [dftk.ElementPsp("Si", psp=psp)] * 2, DISPLACED, functionals=functionals, **mk)
    return dftk.PlaneWaveBasis(model, ECUT, kgrid or dftk.MonkhorstPack((2, 2, 2)).reducible(), device="cuda:0", **kw)


def scf(basis, tol=1e-10):
    res = dftk.self_consistent_field(basis, tol=tol)
    assert res["converged"]
    return res


_CACHE = {}


def hgh_scf(functionals=LDA):
    if functionals not in _CACHE:
        _CACHE[functionals] = scf(si_basis(functionals=functionals, table="pbe" if functionals == PBE else "lda"))
    return _CACHE[functionals]


def upf_scf():
    if "upf" not in _CACHE:
        _CACHE["upf"] = scf(si_basis(psp=pswfc_gen.pswfc_psp()), tol=1e-8)
    return _CACHE["upf"]


def dense_bands(res, kcoords, functionals, table):
    basis = res["basis"]
    lat, _, _ = dftk.silicon_cell()
    oSi = oracle.ElementPsp("Si", oracle.load_psp_hgh("Si", table))
    ob = oracle.PlaneWaveBasis(oracle.model_DFT(lat, [oSi, oSi], DISPLACED, functionals=functionals), ECUT,
                               oracle.ExplicitKpoints([list(k) for k in kcoords], [1.0 / len(kcoords)] * len(kcoords)),
                               fft_size=basis.fft_size)
    _, oham = oracle.energy_hamiltonian(ob, None, None, rho=res["rho"].cpu().numpy())
    return [np.linalg.eigvalsh(H.to_dense()) for H in oham]


# ------------------------------------------------------------------------------------------------ bands
@pytest.mark.parametrize("functionals", [LDA, PBE], ids=["lda", "pbe"])
def test_bands_against_dense_diagonalisation(functionals):
    res = hgh_scf(functionals)
    bands = dftk.compute_bands(res, explicit(GX9), n_bands=N_BANDS, tol=1e-9)
    assert bands["converged"] and len(bands["eigenvalues"]) == 9 and bands["eF"] == res["eF"] and bands["rho"] is res["rho"]
    assert all(len(e) == N_BANDS for e in bands["eigenvalues"]) and all(p.shape[0] == N_BANDS for p in bands["psi"])
    assert bands["basis"].fft_size == res["basis"].fft_size and bands["basis"].Ecut == res["basis"].Ecut
    assert len(bands["occupation"]) == 9 and np.allclose(bands["occupation"][0][:4], 2.0)
    dense = dense_bands(res, GX9, functionals, "pbe" if functionals == PBE else "lda")
    err = max(np.max(np.abs(e - d[:N_BANDS])) for e, d in zip(bands["eigenvalues"], dense))
    print(f"bands against dense eigh: {err:.2e}")
    assert err <= 1e-7
    # residuals of the converged bands with the existing mul_
    _, ham = dftk.energy_hamiltonian(bands["basis"], None, None, rho=res["rho"])
    worst = 0.0
    for H, X, lam in zip(ham, bands["psi"], bands["eigenvalues"]):
        X = X.contiguous()
        R = H.mul_(torch.empty_like(X), X) - torch.from_numpy(lam).cuda()[:, None] * X
        worst = max(worst, float(torch.linalg.norm(R, dim=1).max()))
    print(f"largest residual {worst:.2e}")
    assert worst <= 1e-9


def test_gamma_real_and_complex_blocks_agree():
    rho = hgh_scf()["rho"]
    out = []
    for flag in (True, False):
        bands = dftk.compute_bands(si_basis(gamma_real=flag), explicit(GX9[:3]), n_bands=N_BANDS, rho=rho, tol=1e-7)
        assert bands["basis"].kpoints[0].gamma_real is flag and not bands["basis"].kpoints[1].gamma_real
        assert bands["occupation"] is None and bands["eF"] is None
        out.append(bands["eigenvalues"])
    err = max(np.max(np.abs(a - b)) for a, b in zip(*out))
    print(f"Gamma-real against complex blocks: {err:.2e}")
    assert err <= 1e-9


def test_scf_mesh_is_reproduced():
    res = hgh_scf()
    basis = res["basis"]
    bands = dftk.compute_bands(res, dftk.ExplicitKpoints(basis.kcoords_global, basis.kweights_global), n_bands=4, tol=1e-9)
    err = max(np.max(np.abs(a - np.asarray(b)[:4])) for a, b in zip(bands["eigenvalues"], res["eigenvalues"]))
    print(f"SCF mesh through compute_bands: {err:.2e}")
    assert err <= 1e-7


def test_monkhorst_pack_mesh_and_dos():
    res = hgh_scf()
    bands = dftk.compute_bands(res, dftk.MonkhorstPack((3, 3, 3)), n_bands=6, tol=1e-5)
    assert len(bands["eigenvalues"]) == 27 and abs(sum(bands["basis"].kweights) - 1) < 1e-14
    D = dftk.compute_dos(res["eF"], bands["basis"], bands["eigenvalues"], smearing="gaussian", temperature=0.01)
    Dv = dftk.compute_dos(float(bands["eigenvalues"][0][3]), bands["basis"], bands["eigenvalues"], smearing="gaussian",
                          temperature=0.01)
    print(f"DOS at eF {D}, at the valence band top {Dv}")
    assert np.all(np.isfinite(D)) and np.all(D >= 0) and Dv[0] > D[0]


def test_kchunk_and_keep_psi():
    res = hgh_scf()
    whole = dftk.compute_bands(res, explicit(GX9[:5]), n_bands=N_BANDS, tol=1e-8)
    parts = dftk.compute_bands(res, explicit(GX9[:5]), n_bands=N_BANDS, tol=1e-8, kchunk=2, keep_psi=False)
    assert "psi" not in parts and len(parts["diagonalization"]) == 3 and len(parts["basis"].kpoints) == 5
    err = max(np.max(np.abs(a - b)) for a, b in zip(whole["eigenvalues"], parts["eigenvalues"]))
    print(f"kchunk=2 against one solve: {err:.2e}")
    assert err <= 1e-9
    kept = dftk.compute_bands(res, explicit(GX9[:5]), n_bands=N_BANDS, tol=1e-8, kchunk=3)
    assert [tuple(p.shape) for p in kept["psi"]] == [tuple(p.shape) for p in whole["psi"]]
    with pytest.raises(ValueError):
        dftk.compute_bands(res, explicit(GX9[:5]), kchunk=0)


def test_kpath_form():
    res = hgh_scf()
    pts = {"G": [0, 0, 0], "X": [0.5, 0, 0.5], "L": [0.5, 0.5, 0.5]}
    kpath = dftk.KPath(pts, [["L", "G", "X"]])
    ki = dftk.kpath_interpolate(res["basis"].model, kpath, 8)
    bands = dftk.compute_bands(res, kpath, n_bands=5, kline_density=8)
    assert len(bands["eigenvalues"]) == len(ki["kcoords"]) == len(bands["kinter"]["kdistances"]) > 6
    assert bands["kinter"]["labels"] == ki["labels"] and np.array_equal(bands["kinter"]["kdistances"], ki["kdistances"])
    for kpt, k in zip(bands["basis"].kpoints, ki["kcoords"]):
        assert np.array_equal(kpt.coordinate, k)
    # valence band maximum at Gamma, the lowest band there is the lowest of the path
    iG = dict((name, i) for i, name in ki["labels"])["G"]
    assert max(e[3] for e in bands["eigenvalues"]) == bands["eigenvalues"][iG][3]
    assert min(e[0] for e in bands["eigenvalues"]) == bands["eigenvalues"][iG][0]


def test_compute_bands_between_scf_steps_leaves_the_scf_bit_identical():
    def run(with_bands):
        basis = si_basis()
        seen = []

        def cb(info):
            if with_bands:
                seen.append(dftk.compute_bands(basis, explicit(GX9[:3]), n_bands=5, rho=info["rho"])["eigenvalues"])
        return dftk.self_consistent_field(basis, tol=1e-9, callback=cb), seen
    ref, _ = run(False)
    got, seen = run(True)
    assert len(seen) >= 3 and all(np.all(np.isfinite(e)) for s in seen for e in s)
    assert got["energies"].total == ref["energies"].total and got["n_iter"] == ref["n_iter"]
    assert torch.equal(got["rho"], ref["rho"])
    for a, b in zip(got["eigenvalues"], ref["eigenvalues"]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_collinear_channels_equal_the_unpolarised_bands():
    fun = ("lda_x", "lda_c_pw")
    rho = hgh_scf()["rho"]
    plain = dftk.compute_bands(si_basis(functionals=fun), explicit(GX9[:4]), n_bands=6, rho=rho, tol=1e-9)
    spin = dftk.compute_bands(si_basis(functionals=fun, spin_polarization="collinear"), explicit(GX9[:4]), n_bands=6,
                              rho=torch.stack([rho / 2, rho / 2]), tol=1e-9)
    assert len(spin["eigenvalues"]) == 8 and [k.spin for k in spin["basis"].kpoints] == [1] * 4 + [2] * 4
    err = max(np.max(np.abs(s - plain["eigenvalues"][i % 4])) for i, s in enumerate(spin["eigenvalues"]))
    print(f"collinear channels against the unpolarised bands: {err:.2e}")
    assert err <= 1e-7


# ------------------------------------------------------------------------------------------------ orbitals
def twin_of(basis, labels_per_atom=(("3S", "3P"), ("3S", "3P"))):
    """per k-block (Phi~ of the twin, eigenvalues of S, the twin's orthonormality defect)"""
    model = basis.model
    out = []
    for kpt in basis.kpoints:
        Phi = pswfc_gen.twin_orbitals(kpt.G_vectors.cpu().numpy(), kpt.coordinate, model.recip_lattice,
                                      model.unit_cell_volume, model.positions, labels_per_atom)
        Phi_t, lam = pswfc_gen.twin_lowdin(Phi)
        out.append((Phi_t, lam, np.max(np.abs(Phi_t.conj().T @ Phi_t - np.eye(Phi_t.shape[1])))))
    return out


def phi_bound(Phi_t, lam, defect):
    """relative to max |Phi~| (the module's docstring)"""
    n = Phi_t.shape[1]
    return 10 * E_QUAD + 8 * max(defect, n * U * math.sqrt(lam.max() / lam.min()))


def test_atomic_orbital_projectors():
    basis = upf_scf()["basis"]
    projectors, labels = dftk.atomic_orbital_projectors(basis)
    assert labels == pswfc_gen.twin_labels([("3S", "3P"), ("3S", "3P")])
    assert [(o["l"], o["n"], o["m"]) for o in labels[:4]] == [(0, 1, 0), (1, 1, -1), (1, 1, 0), (1, 1, 1)]
    assert len(projectors) == len(basis.kpoints)
    for kpt, P, (Phi_t, lam, defect) in zip(basis.kpoints, projectors, twin_of(basis)):
        assert tuple(P.shape) == (8, kpt.n_G)
        got = P.cpu().numpy().T
        tol = phi_bound(Phi_t, lam, defect)
        orth = np.max(np.abs(got.conj().T @ got - np.eye(8)))
        err = np.max(np.abs(got - Phi_t)) / np.max(np.abs(Phi_t))
        print(f"k = {kpt.coordinate}: |Phi~'Phi~ - I| {orth:.1e}, against the twin {err:.1e}, bound {tol:.1e}")
        assert orth <= tol and err <= tol


def test_isonmanifold_and_second_radial_function():
    basis = upf_scf()["basis"]
    projectors, labels = dftk.atomic_orbital_projectors(basis, isonmanifold=lambda o: o["label"] == "3P")
    assert len(labels) == 6 and all(o["l"] == 1 and o["label"] == "3P" for o in labels)
    assert [o["iatom"] for o in labels] == [0, 0, 0, 1, 1, 1] and [o["m"] for o in labels[:3]] == [-1, 0, 1]
    tw = twin_of(basis, (("3P",), ("3P",)))
    for P, (Phi_t, lam, defect) in zip(projectors, tw):
        got = P.cpu().numpy().T
        tol = phi_bound(Phi_t, lam, defect)
        assert got.shape[1] == 6 and np.max(np.abs(got.conj().T @ got - np.eye(6))) <= tol
        assert np.max(np.abs(got - Phi_t)) <= tol * np.max(np.abs(Phi_t))
    # only the first atom
    _, one = dftk.atomic_orbital_projectors(basis, isonmanifold=lambda o: o["iatom"] == 0)
    assert len(one) == 4 and {o["iatom"] for o in one} == {0}
    # a file with 3S, 3P and 4S: two radial functions for l = 0, in the file's order
    b3 = si_basis(psp=pswfc_gen.pswfc_psp(("3S", "3P", "4S")), kgrid=explicit(GX9[1:3]))
    projectors, labels = dftk.atomic_orbital_projectors(b3)
    assert len(labels) == 10 and labels == pswfc_gen.twin_labels([("3S", "3P", "4S")] * 2)
    assert [(o["l"], o["n"], o["label"]) for o in labels[:2]] == [(0, 1, "3S"), (0, 2, "4S")]
    for P, (Phi_t, lam, defect) in zip(projectors, twin_of(b3, (("3S", "3P", "4S"),) * 2)):
        got = P.cpu().numpy().T
        tol = phi_bound(Phi_t, lam, defect)
        print(f"3S 3P 4S: cond(S) {lam.max() / lam.min():.1e}, against the twin "
              f"{np.max(np.abs(got - Phi_t)) / np.max(np.abs(Phi_t)):.1e}, bound {tol:.1e}")
        assert np.max(np.abs(got - Phi_t)) <= tol * np.max(np.abs(Phi_t))


def projection_bounds(psi, Phi_t, lam, defect):
    """(twin |C|^2, its bound), both (n_bands, n_proj); psi is n_G x n_bands"""
    n_G = psi.shape[0]
    Cm = psi.conj().T @ Phi_t
    dphi = phi_bound(Phi_t, lam, defect) * np.max(np.abs(Phi_t)) * math.sqrt(n_G)
    dC = np.linalg.norm(psi, axis=0)[:, None] * (dphi + 8 * n_G * U * np.linalg.norm(Phi_t, axis=0)[None, :])
    return np.abs(Cm) ** 2, 2 * np.abs(Cm) * dC + dC ** 2


def test_atomic_orbital_projections():
    res = upf_scf()
    basis = res["basis"]
    projections, labels = dftk.atomic_orbital_projections(basis, res["psi"])
    assert len(labels) == 8
    for proj, psik, tw in zip(projections, res["psi"], twin_of(basis)):
        assert tuple(proj.shape) == (psik.shape[0], 8)
        got = proj.cpu().numpy()
        want, bound = projection_bounds(psik.cpu().numpy().T, *tw)
        tot = got.sum(axis=1)
        print(f"|C|^2 error / bound {np.max(np.abs(got - want) / bound):.2e}; sum_p per band in [{tot.min():.4f}, {tot.max():.4f}]")
        assert np.all(np.abs(got - want) <= bound)
        assert np.all(got >= 0) and np.all(tot <= 1 + 1e-12)
        assert np.all(tot[:4] > 0.5)          # the valence bands of silicon are made of 3s and 3p


@pytest.mark.parametrize("smearing", ["gaussian", "fermi_dirac"])
def test_compute_pdos_against_the_twin(smearing):
    res = upf_scf()
    basis, T = res["basis"], 0.01
    eps = np.linspace(-0.35, 0.55, 200)
    out = dftk.compute_pdos(eps, basis, res["psi"], res["eigenvalues"], smearing=smearing, temperature=T)
    assert out["pdos"].shape == (200, 8, 1) and len(out["projector_labels"]) == 8 and np.array_equal(out["eps"], eps)
    filled = basis.model.filled_occupation
    projs, bound = [], np.zeros((200, 8))
    for psik, eig, w, tw in zip(res["psi"], res["eigenvalues"], basis.kweights, twin_of(basis)):
        want, dproj = projection_bounds(psik.cpu().numpy().T, *tw)
        projs.append(want)
        g = np.abs(occupation_derivative(smearing, (np.asarray(eig)[None, :want.shape[0]] - eps[:, None]) / T)) / T
        bound += filled * w * (16 * U * (g @ want) + g @ dproj)
    twin = pswfc_gen.twin_pdos(eps, projs, res["eigenvalues"], basis.kweights, [k.spin for k in basis.kpoints], filled,
                               smearing, T)
    err = np.abs(out["pdos"][:, :, 0] - twin[:, :, 0])
    print(f"{smearing}: PDOS error / bound {np.max(err / np.maximum(bound, 1e-300)):.2e}, largest value {twin.max():.3f}")
    assert np.all(err <= bound + 1e-300)
    # the sum over the orthonormal set never exceeds the DOS of the same bands
    total = dftk.sum_pdos(out, [lambda o: True])
    dos = np.array([dftk.compute_dos(e, basis, res["eigenvalues"], smearing=smearing, temperature=T) for e in eps])
    assert total.shape == dos.shape == (200, 1) and np.all(total <= dos + 1e-12)
    s_part = dftk.sum_pdos(out, [lambda o: o["l"] == 0])
    p_part = dftk.sum_pdos(out, [lambda o: o["l"] == 1])
    np.testing.assert_allclose(s_part + p_part, total, rtol=1e-13, atol=1e-300)


def test_pdos_integral_identity():
    res = upf_scf()
    basis, T = res["basis"], 0.01
    lo = min(np.min(e) for e in res["eigenvalues"]) - 12 * T
    hi = max(np.max(e) for e in res["eigenvalues"]) + 12 * T
    eps = lo + (T / 2) * np.arange(int(math.ceil((hi - lo) / (T / 2))) + 1)
    out = dftk.compute_pdos(eps, basis, res["psi"], res["eigenvalues"], smearing="gaussian", temperature=T)
    D = out["pdos"][:, :, 0]
    got = (T / 2) * (D.sum(axis=0) - 0.5 * (D[0] + D[-1]))
    projections, _ = dftk.atomic_orbital_projections(basis, res["psi"])
    want = basis.model.filled_occupation * sum(w * p.cpu().numpy().sum(axis=0) for w, p in zip(basis.kweights, projections))
    err = np.max(np.abs(got - want) / want)
    print(f"{len(eps)} energies: trapezoid integral of the PDOS against the projections, {err:.2e} relative")
    assert err <= 1e-10


def test_pdos_from_a_bands_result_and_collinear_shape():
    res = upf_scf()
    eps = np.linspace(-0.3, 0.5, 33)
    bands = dftk.compute_bands(res, explicit(GX9[:3]), n_bands=6, tol=1e-8)
    a = dftk.compute_pdos(eps, bands, smearing="gaussian", temperature=0.01)
    b = dftk.compute_pdos(eps, bands["basis"], bands["psi"], bands["eigenvalues"], smearing="gaussian", temperature=0.01)
    assert a["pdos"].shape == (33, 8, 1) and np.array_equal(a["pdos"], b["pdos"]) and a["pdos"].max() > 1
    # the model's own smearing and temperature are the defaults
    warm = si_basis(psp=pswfc_gen.pswfc_psp(), kgrid=explicit(GX9[:3]), temperature=0.01, smearing="gaussian")
    c = dftk.compute_pdos(eps, warm, bands["psi"], bands["eigenvalues"])
    assert np.array_equal(c["pdos"], a["pdos"])
    # collinear: both channels of a non-magnetic density
    fun = ("lda_x", "lda_c_pw")
    rho = res["rho"]
    plain = dftk.compute_bands(si_basis(psp=pswfc_gen.pswfc_psp(), functionals=fun), explicit(GX9[:3]), n_bands=6, rho=rho,
                               tol=1e-9)
    spin = dftk.compute_bands(si_basis(psp=pswfc_gen.pswfc_psp(), functionals=fun, spin_polarization="collinear"),
                              explicit(GX9[:3]), n_bands=6, rho=torch.stack([rho / 2, rho / 2]), tol=1e-9)
    p1 = dftk.compute_pdos(eps, plain, smearing="gaussian", temperature=0.01)["pdos"]
    p2 = dftk.compute_pdos(eps, spin, smearing="gaussian", temperature=0.01)["pdos"]
    assert p2.shape == (33, 8, 2)
    err = max(np.max(np.abs(p2[:, :, 0] - p2[:, :, 1])), np.max(np.abs(2 * p2[:, :, 0] - p1[:, :, 0])))
    print(f"collinear PDOS channels: {err:.2e} (largest value {p1.max():.2f})")
    # the channels are solved separately to residuals of 1e-9: eigenvectors agree to residual / gap, the gaps between the
    # (groups of degenerate) levels of these k-points are above 1e-3, and |C|^2 carries twice that: 2e-6, taken as 1e-5
    assert err <= 1e-5 * p1.max()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_on_the_device():
    lat, _, _ = dftk.silicon_cell()
    upf = pswfc_gen.pswfc_psp()
    mixed = dftk.model_DFT(lat, [dftk.ElementPsp("Si", psp=upf), dftk.ElementPsp("C", psp=dftk.load_psp("C", "lda"))],
                           DISPLACED, functionals=LDA)
    bm = dftk.PlaneWaveBasis(mixed, ECUT, explicit(GX9[:2]), device="cuda:0")
    with pytest.raises(ValueError, match=r"atom 1 \(C\)"):
        dftk.atomic_orbital_projectors(bm)
    hgh = hgh_scf()
    with pytest.raises(ValueError, match="no pseudo-atomic orbitals"):
        dftk.compute_pdos([0.0], hgh["basis"], hgh["psi"], hgh["eigenvalues"], smearing="gaussian", temperature=0.01)
    res = upf_scf()
    with pytest.raises(ValueError, match="finite temperature"):
        dftk.compute_pdos([0.0], res["basis"], res["psi"], res["eigenvalues"])
    _, atoms, pos = dftk.silicon_cell()
    bx = dftk.PlaneWaveBasis(dftk.model_HF(lat, atoms, pos), ECUT, dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cuda:0")
    with pytest.raises(NotImplementedError, match="exact exchange"):
        dftk.compute_bands(bx, explicit(GX9[:2]), rho=hgh["rho"])
    with pytest.raises(ValueError, match="converged density is required"):
        dftk.compute_bands(hgh["basis"], explicit(GX9[:2]))
