"""DFT+U through the public interface, on the device.

Cell: displaced Si2 at Ecut 7 (as tests/test_gpu_bands.py), with the generated UPF file of tests/hubbard_gen.py (orbitals
3S, 3P and 3D; quadrature error below E_QUAD of tests/test_upf_host.py, tests/test_hubbard_host.py measures it).  Yardstick:
the NumPy twin of tests/hubbard_gen.py fed the downloaded orbitals and its own Phi.  Bounds:
  Phi~          ``phi_bound`` of tests/test_gpu_bands.py (relative to max |Phi~|), as a column norm: x max |Phi~| sqrt(n_G);
  C = Phi~' psi dC = |psi_n| (that column bound + 8 n_G 2^-52 |phi_p|), ``projection_bounds`` of tests/test_gpu_bands.py;
  n             sum_k sum_n |w| (|C1| dC2 + |C2| dC1 + dC1 dC2) + (n_bands + 4) 2^-52 sum |w| |C1| |C2| (the kernel's bound);
  Phi D Phi' psi  (2 e + e^2) |D|_2 |psi_n| with e the Frobenius bound of the manifold's columns of Phi~, plus
                64 x 2^-52 (|H_U psi_n| + |H_0 psi_n|) for the difference of two H psi;
  eigenvalues   1e-7 against the dense diagonalisation, the bound of tests/test_gpu_bands.py, taken over as it is;
  two solves of one Hamiltonian to residual tol: their eigenvalues differ by at most 2 tol (|lambda - theta| <= |r|).
Every test prints what it measured (``pytest -s``)."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
import oracle  # noqa: E402

import hubbard_gen  # noqa: E402
from test_gpu_bands import DISPLACED, ECUT, GX9, explicit, phi_bound  # noqa: E402

LDA = ("lda_x", "lda_c_vwn")
SPIN_LDA = ("lda_x", "lda_c_pw")
U = 2.0 ** -52
SYMMETRIC = [1.02 * np.ones(3) / 8, -1.02 * np.ones(3) / 8]     # keeps the threefold axis, its mirrors and the inversion
_PSP = {}
_CACHE = {}


@pytest.fixture(autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    torch.manual_seed(20250211)


def psp():
    if "upf" not in _PSP:
        _PSP["upf"] = hubbard_gen.hubbard_psp()
    return _PSP["upf"]


def hubbard_of(*pairs):
    return dftk.Hubbard(*[(dftk.OrbitalManifold("Si", lab), u) for lab, u in pairs])


def si_basis(hubbard=None, functionals=LDA, kgrid=None, positions=DISPLACED, symmetries=False, pseudo=None, **kw):
    lat, _, _ = dftk.silicon_cell()
    mk = {k: kw.pop(k) for k in list(kw) if k in ("magnetic_moments", "spin_polarization")}
    extra = dict(extra_terms=[hubbard]) if hubbard is not None else {}
    model = dftk.model_DFT(lat, [dftk.ElementPsp("Si", psp=psp() if pseudo is None else pseudo)] * 2, positions,
                           functionals=functionals, symmetries=symmetries, **extra, **mk)
    return dftk.PlaneWaveBasis(model, ECUT, kgrid or dftk.MonkhorstPack((2, 2, 2)).reducible(), device="cuda:0", **kw)


def cached_scf(name, make, tol=1e-10):
    if name not in _CACHE:
        res = dftk.self_consistent_field(make(), tol=tol)
        assert res["converged"], name
        _CACHE[name] = res
    return _CACHE[name]


def plain_scf():
    return cached_scf("plain", lambda: si_basis())


def u_scf(u=0.1):
    return cached_scf(("3P", u), lambda: si_basis(hubbard_of(("3P", u))))


def twin_phi(basis):
    """per k-block (Phi~ of the twin over all 18 orbitals, its relative bound)"""
    model = basis.model
    out = []
    for kpt in basis.kpoints:
        Phi_t, lam = hubbard_gen.twin_orbitals(kpt.G_vectors.cpu().numpy(), kpt.coordinate, model.recip_lattice,
                                               model.unit_cell_volume, model.positions)
        defect = np.max(np.abs(Phi_t.conj().T @ Phi_t - np.eye(Phi_t.shape[1])))
        out.append((Phi_t, phi_bound(Phi_t, lam, defect)))
    return out


def host(psi):
    return [p.cpu().numpy().T for p in psi]


# ------------------------------------------------------------------------------------------------ occupations
def occupation_bound(Phi_t, rel, psik, w, cols_i, cols_j):
    n_G = psik.shape[0]
    dphi = rel * np.max(np.abs(Phi_t)) * math.sqrt(n_G)
    Cm = Phi_t.conj().T @ psik                                                          # (n_proj, n_bands)
    dC = (dphi + 8 * n_G * U * np.linalg.norm(Phi_t, axis=0))[:, None] * np.linalg.norm(psik, axis=0)[None, :]
    a, aw = np.abs(Cm), np.abs(w)
    ai, aj, di, dj = a[cols_i], a[cols_j], dC[cols_i], dC[cols_j]
    return ((ai * aw) @ dj.T + (di * aw) @ aj.T + (di * aw) @ dj.T + (psik.shape[1] + 4) * U * ((ai * aw) @ aj.T))


@pytest.mark.parametrize("spin", ["none", "collinear"])
def test_occupations_against_the_twin(spin):
    if spin == "none":
        res, kw = plain_scf(), {}
        b0 = res["basis"]
    else:
        # three steps from a magnetic guess: the channels differ, and the occupations need no converged state
        kw = dict(functionals=SPIN_LDA, spin_polarization="collinear", magnetic_moments=[1.0, 1.0])
        if "collinear" not in _CACHE:
            b0 = si_basis(**kw)
            stepper = dftk.ScfStepper(b0, rho=dftk.guess_density(b0, [1.0, 1.0]), tol=1e-8)
            for _ in range(3):
                info = stepper.step()
            _CACHE["collinear"] = dict(info, basis=b0)
        res = _CACHE["collinear"]
        b0 = res["basis"]
    n_spin, filled = b0.model.n_spin_components, b0.model.filled_occupation
    tw = twin_phi(b0)
    psi = host(res["psi"])
    spins = [k.spin for k in b0.kpoints]
    for labels in (("3P",), ("3D",), ("3P", "3D")):
        basis = si_basis(hubbard_of(*[(lab, 0.1) for lab in labels]), **kw)
        assert [tuple(k.coordinate) for k in basis.kpoints] == [tuple(k.coordinate) for k in b0.kpoints]
        got = dftk.compute_hubbard_n(basis, res["psi"], res["occupation"])
        cols = hubbard_gen.manifold_columns(2, [((0, 1), lab) for lab in labels])
        want = hubbard_gen.twin_hubbard_n([t[0] for t in tw], psi, res["occupation"], basis.kweights, spins, filled, n_spin,
                                          cols)
        assert len(got) == len(labels)
        worst = 0.0
        for g, t, per_atom, lab in zip(got, want, cols, labels):
            d = 2 * hubbard_gen.ORBITALS[lab][0] + 1
            assert g.shape == (n_spin, 2, 2, d, d) and g.dtype == complex
            assert np.all(g[:, 0, 1] == 0) and np.all(g[:, 1, 0] == 0)                  # cross-atom blocks stay zero
            for s in range(n_spin):
                for ia, c in enumerate(per_atom):
                    bound = np.zeros((d, d))
                    for (Phi_t, rel), psik, occ, wk, sp in zip(tw, psi, res["occupation"], basis.kweights, spins):
                        if sp == s + 1:
                            w = wk * np.asarray(occ)[:psik.shape[1]] / filled
                            bound += occupation_bound(Phi_t, rel, psik, w, c, c)
                    worst = max(worst, np.max(np.abs(g[s, ia, ia] - t[s, ia, ia]) / bound))
                    tr = np.trace(g[s, ia, ia]).real
                    assert -1e-12 <= tr <= d + 1e-12
        print(f"{spin} {labels}: occupation error / bound {worst:.2e}; tr n(3P) = {np.trace(got[0][0, 0, 0]).real:.4f}")
        assert worst <= 1
    if spin == "collinear":
        g = dftk.compute_hubbard_n(basis, res["psi"], res["occupation"])[0]
        assert np.max(np.abs(g[0] - g[1])) > 1e-6                                       # a magnetic state: the channels differ


# ------------------------------------------------------------------------------------------------ operator
def random_n(rng, n_spin, d, real=False):
    n = np.zeros((n_spin, 2, 2, d, d), dtype=complex)
    for s in range(n_spin):
        for ia in range(2):
            a = rng.standard_normal((d, d)) + (0 if real else 1j) * rng.standard_normal((d, d))
            n[s, ia, ia] = (a + a.conj().T) / (4 * d)
    return n


def test_operator_against_the_twin():
    rho = plain_scf()["rho"]
    rng = np.random.default_rng(4)
    Us = (0.3, 0.7)
    basis = si_basis(hubbard_of(("3P", Us[0]), ("3D", Us[1])))
    n = [random_n(rng, 1, 3), random_n(rng, 1, 5)]
    cols = hubbard_gen.manifold_columns(2, [((0, 1), "3P"), ((0, 1), "3D")])
    E_U, ham_U = dftk.energy_hamiltonian(basis, None, None, rho=rho, hubbard_n=n)
    E_0, ham_0 = dftk.energy_hamiltonian(basis, None, None, rho=rho)
    assert E_0["Hubbard"] == 0.0 and all(H.hubbard is None for H in ham_0) and all(H.hubbard is not None for H in ham_U)
    assert abs(E_U["Hubbard"] - hubbard_gen.twin_energy(Us, n, 2)) <= 64 * U * abs(E_U["Hubbard"])
    tw = twin_phi(basis)
    worst = 0.0
    for ik in (0, 3, 7):
        kpt = basis.kpoints[ik]
        X = torch.randn((6, kpt.n_G), dtype=torch.complex128, device="cuda")
        # (alternating: every mul_ finds the other Hamiltonian's rows in the slot and puts its own back)
        HU = ham_U[ik].mul_(torch.empty_like(X), X).cpu().numpy().T
        H0 = ham_0[ik].mul_(torch.empty_like(X), X).cpu().numpy().T
        HU2 = ham_U[ik].mul_(torch.empty_like(X), X).cpu().numpy().T
        assert np.array_equal(HU, HU2)
        Phi_t, rel = tw[ik]
        D = hubbard_gen.twin_coupling(Us, n, 1, cols, Phi_t.shape[1])
        x = X.cpu().numpy().T
        want = hubbard_gen.twin_operator(Phi_t, D) @ x
        e = rel * np.max(np.abs(Phi_t)) * math.sqrt(kpt.n_G * 16)                       # 16 manifold columns
        bound = ((2 * e + e * e) * np.linalg.norm(D, 2) * np.linalg.norm(x, axis=0)
                 + 64 * U * (np.linalg.norm(HU, axis=0) + np.linalg.norm(H0, axis=0)))
        err = np.linalg.norm(HU - H0 - want, axis=0)
        worst = max(worst, np.max(err / bound))
        assert np.linalg.norm(want) > 1e-3 * np.linalg.norm(HU)
    print(f"(H_U - H_0) psi against the twin's Phi D Phi' psi: error / bound {worst:.2e}")
    assert worst <= 1


def test_gamma_real_block_against_the_complex_block():
    rho = plain_scf()["rho"]
    n = [random_n(np.random.default_rng(8), 1, 3, real=True)]
    out = []
    tol = 1e-9
    for flag in (True, False):
        basis = si_basis(hubbard_of(("3P", 0.5)), kgrid=explicit(GX9[:1]), gamma_real=flag)
        assert basis.kpoints[0].gamma_real is flag
        bands = dftk.compute_bands(basis, explicit(GX9[:1]), n_bands=6, rho=rho, tol=tol, hubbard_n=n)
        assert bands["converged"] and bands["basis"].kpoints[0].gamma_real is flag
        out.append(bands["eigenvalues"][0])
    plain = dftk.compute_bands(si_basis(kgrid=explicit(GX9[:1])), explicit(GX9[:1]), n_bands=6, rho=rho, tol=tol)
    err = np.max(np.abs(out[0] - out[1]))
    shift = np.max(np.abs(out[1] - plain["eigenvalues"][0]))
    print(f"Gamma-real against complex with the Hubbard rows: {err:.2e} (the rows move the levels by {shift:.2e})")
    assert err <= 2 * tol and shift > 1e-3
    # occupations with an imaginary part (a k-mesh that is not closed under k -> -k): the Gamma-real block refuses them,
    # the complex block takes them; rounding-sized imaginary parts pass
    gr, cx = (si_basis(hubbard_of(("3P", 0.5)), kgrid=explicit(GX9[:1]), gamma_real=flag) for flag in (True, False))
    skew = 1j * (np.triu(np.ones((3, 3)), 1) - np.tril(np.ones((3, 3)), -1))[None, None, None]      # Hermitian, imaginary
    bent = [n[0] + 1e-6 * skew]
    with pytest.raises(ValueError, match="gamma_real=False"):
        dftk.energy_hamiltonian(gr, None, None, rho=rho, hubbard_n=bent)
    E_c, _ = dftk.energy_hamiltonian(cx, None, None, rho=rho, hubbard_n=bent)
    noisy = [n[0] + 1e-14 * skew]
    E_r, _ = dftk.energy_hamiltonian(gr, None, None, rho=rho, hubbard_n=noisy)
    assert abs(E_r["Hubbard"] - E_c["Hubbard"]) <= 1e-10
    # with further k-points the automatic choice is off for a Hubbard model, and on without the term
    lanes = dict(kgrid=explicit(GX9[:3]), n_lanes=2)
    assert not si_basis(hubbard_of(("3P", 0.5)), **lanes).kpoints[0].gamma_real and si_basis(**lanes).kpoints[0].gamma_real
    assert si_basis(hubbard_of(("3P", 0.5)), kgrid=explicit(GX9[:1])).kpoints[0].gamma_real


def test_batched_small_blocks_against_the_sequential_path(monkeypatch):
    rho = plain_scf()["rho"]
    n = [random_n(np.random.default_rng(9), 1, 3)]
    tol = 1e-9
    out = []
    for sequential in (False, True):
        if sequential:
            monkeypatch.setenv("DFTK_MI_KBATCH_SEQUENTIAL", "1")
        else:
            monkeypatch.delenv("DFTK_MI_KBATCH_SEQUENTIAL", raising=False)
        basis = si_basis(hubbard_of(("3P", 0.5)))
        assert basis.kbatch
        bands = dftk.compute_bands(basis, dftk.MonkhorstPack((2, 2, 2)).reducible(), n_bands=4, n_extra=2, rho=rho, tol=tol,
                                   hubbard_n=n)
        assert bands["converged"] and bands["basis"].kbatch
        out.append(bands["eigenvalues"])
    err = max(np.max(np.abs(a - b)) for a, b in zip(*out))
    print(f"batched small-block LOBPCG against DFTK_MI_KBATCH_SEQUENTIAL=1: {err:.2e}")
    assert err <= 2 * tol


# ------------------------------------------------------------------------------------------------ eigenvalues
def test_eigenvalues_against_dense_diagonalisation():
    res = u_scf()
    basis = res["basis"]
    k = GX9[3]
    bands = dftk.compute_bands(res, explicit([k]), n_bands=8, tol=1e-9)
    assert bands["converged"]
    lat, _, _ = dftk.silicon_cell()
    oSi = oracle.ElementPsp("Si", oracle.load_psp_hgh("Si", "lda"))
    ob = oracle.PlaneWaveBasis(oracle.model_DFT(lat, [oSi, oSi], DISPLACED, functionals=LDA), ECUT,
                               oracle.ExplicitKpoints([list(k)], [1.0]), fft_size=basis.fft_size)
    _, oham = oracle.energy_hamiltonian(ob, None, None, rho=res["rho"].cpu().numpy())
    kpt = bands["basis"].kpoints[0]
    assert np.array_equal(oham[0].kpoint.mapping, kpt.mapping)
    Phi_t, _ = twin_phi(bands["basis"])[0]
    cols = hubbard_gen.manifold_columns(2, [((0, 1), "3P")])
    D = hubbard_gen.twin_coupling([0.1], res["hubbard_n"], 1, cols, Phi_t.shape[1])
    dense = oham[0].to_dense() + hubbard_gen.twin_operator(Phi_t, D)
    want = np.linalg.eigvalsh((dense + dense.conj().T) / 2)[:8]
    bare = np.linalg.eigvalsh(oham[0].to_dense())[:8]
    err = np.max(np.abs(bands["eigenvalues"][0] - want))
    print(f"eigenvalues against dense eigh with the twin's Phi D Phi': {err:.2e} "
          f"(the Hubbard rows move them by {np.max(np.abs(want - bare)):.2e})")
    assert err <= 1e-7 and np.max(np.abs(want - bare)) > 1e-4


# ------------------------------------------------------------------------------------------------ SCF
def test_u_zero_is_the_plain_model():
    """A term with U = 0 adds rows with zero couplings and E = 0: every energy agrees with the plain model's to the SCF
    tolerance, 1e-10 (measured: no difference at all)."""
    ref = plain_scf()
    res = cached_scf("U0", lambda: si_basis(hubbard_of(("3P", 0.0))))
    assert res["energies"]["Hubbard"] == 0.0 and "Hubbard" not in ref["energies"]
    worst = max(abs(res["energies"][k] - ref["energies"][k]) for k in ref["energies"])
    print(f"U = 0 against the model without the term: largest energy difference {worst:.2e}")
    assert worst <= 1e-10
    assert res["hubbard_n"] is not None and "hubbard_n" not in ref
    # an empty term: no manifold, no set-up, nothing to compute
    empty = dftk.self_consistent_field(si_basis(dftk.Hubbard()), tol=1e-6)
    assert empty["energies"]["Hubbard"] == 0.0 and empty["hubbard_n"] == []


def test_symmetric_and_full_mesh_give_the_same_occupations():
    """n is a projection of the density matrix P onto orthonormal orbitals, |dn| <= |dP|_2 <= |dV| / gap, and
    |dV| <= (4 pi / |G_min|^2 + 1) |drho| (Hartree kernel plus the LDA kernel, which is below 1 at these densities); the
    density is within 4 |rho_out - rho_in| of the fixed point for a damped, Anderson-accelerated iteration that contracts by
    more than 3/4 per step.  Both SCFs contribute."""
    hub = hubbard_of(("3P", 0.1))
    full = cached_scf("sym-off", lambda: si_basis(hub, positions=SYMMETRIC, kgrid=dftk.MonkhorstPack((2, 2, 2))))
    sym = cached_scf("sym-on", lambda: si_basis(hub, positions=SYMMETRIC, kgrid=dftk.MonkhorstPack((2, 2, 2)),
                                                symmetries=True))
    assert len(sym["basis"].symmetries) > 2 and len(sym["basis"].kpoints) < len(full["basis"].kpoints) == 8
    gap = min(min(e[4] for e in r["eigenvalues"]) - max(e[3] for e in r["eigenvalues"]) for r in (full, sym))
    Gmin = min(np.linalg.norm(full["basis"].model.recip_lattice @ g) for g in np.eye(3))
    bound = (4 * math.pi / Gmin ** 2 + 1) / gap * 4 * (full["history_drho"][-1] + sym["history_drho"][-1])
    err = np.max(np.abs(full["hubbard_n"][0] - sym["hubbard_n"][0]))
    print(f"{len(sym['basis'].symmetries)} symmetries, {len(sym['basis'].kpoints)} k-points: |n_sym - n_full| = {err:.2e}, "
          f"bound {bound:.2e} (gap {gap:.3f})")
    assert err <= bound
    # the symmetric cell's matrices are invariant themselves, and those of the two atoms are each other's images
    n = sym["hubbard_n"][0]
    again = dftk.symmetrize_hubbard_n(sym["basis"].model, dftk.resolve_hubbard_manifold(hub.manifolds[0], sym["basis"].model),
                                      n, sym["basis"].symmetries)
    assert np.max(np.abs(again - n)) <= 1e-13
    assert abs(sym["energies"].total - full["energies"].total) <= 1e-8


def test_hellmann_feynman_in_u():
    """dE / dU = E_Hubbard / U at self-consistency (the functional is stationary in the orbitals).  Central quotients with
    h and 2 h: their difference is the truncation estimate; the SCFs' energy noise is what their last two steps differ by."""
    u, h = 0.1, 0.01
    res = u_scf(u)
    target = res["energies"]["Hubbard"] / u
    quotients, noise = [], []
    for step in (h, 2 * h):
        plus, minus = u_scf(u + step), u_scf(u - step)
        quotients.append((plus["energies"].total - minus["energies"].total) / (2 * step))
        noise.append(sum(abs(r["history_Etot"][-1] - r["history_Etot"][-2]) + abs(r["energies"].total - r["history_Etot"][-1])
                         for r in (plus, minus)) / step)
    truncation = abs(quotients[0] - quotients[1])
    print(f"dE/dU: quotients {quotients[0]:.10f} (h) {quotients[1]:.10f} (2h), E_Hubbard / U {target:.10f}; "
          f"truncation estimate {truncation:.2e}, noise / h {noise[0]:.2e}")
    assert abs(quotients[0] - target) <= truncation + noise[0]
    assert target > 1e-2


def test_step_energies_come_from_the_projections(monkeypatch):
    """With a Hubbard operator in H the Ritz values contain <psi|V_U|psi>: the per-step AtomicNonlocal of a Hubbard model
    must be the projection-GEMM value with and without DFTK_MI_EXACT_STEP_ENERGIES."""
    def steps(exact):
        if exact:
            monkeypatch.setenv("DFTK_MI_EXACT_STEP_ENERGIES", "1")
        else:
            monkeypatch.delenv("DFTK_MI_EXACT_STEP_ENERGIES", raising=False)
        stepper = dftk.ScfStepper(si_basis(hubbard_of(("3P", 0.3))), tol=1e-10)
        assert stepper.ritz_energies is False
        return stepper, [stepper.step() for _ in range(3)]
    stepper, infos = steps(False)
    _, exact = steps(True)
    for a, b in zip(infos, exact):
        assert a["energies"]["AtomicNonlocal"] == b["energies"]["AtomicNonlocal"]
        assert a["energies"]["Hubbard"] == b["energies"]["Hubbard"]
    assert infos[0]["ham"][0].hubbard is None and infos[1]["ham"][0].hubbard is not None      # a cold start's first step
    info = infos[-1]
    direct, _ = dftk.energy_hamiltonian(stepper.basis, info["psi"], info["occupation"], rho=info["rho"], only_energies=True,
                                        hubbard_n=info["hubbard_n"])
    err = abs(direct["AtomicNonlocal"] - info["energies"]["AtomicNonlocal"])
    # what the Ritz-value form would have reported: off by the Hubbard expectation value
    ritz, _ = dftk.energy_hamiltonian(stepper.basis, info["psi"], info["occupation"], rho=info["rho"], only_energies=True,
                                      eigenvalues=info["eigenvalues"], ritz_occupation_threshold=1e-6,
                                      ritz_potential=dftk.ScfStepper._ritz_potential(info["ham"]))
    off = abs(ritz["AtomicNonlocal"] - direct["AtomicNonlocal"])
    print(f"per-step AtomicNonlocal against the projections: {err:.1e}; the Ritz-value form is off by {off:.2e}")
    assert err <= 64 * U * abs(direct["AtomicNonlocal"]) and off > 1e-4
    assert info["hubbard_n"] is not None and info["energies"]["Hubbard"] > 0


# ------------------------------------------------------------------------------------------------ bands and I/O
def test_bands_reproduce_the_scf_and_hubbard_n_survives_io(tmp_path):
    res = u_scf()
    basis = res["basis"]
    bands = dftk.compute_bands(res, dftk.ExplicitKpoints(basis.kcoords_global, basis.kweights_global), n_bands=4, tol=1e-9)
    err = max(np.max(np.abs(a - np.asarray(b)[:4])) for a, b in zip(bands["eigenvalues"], res["eigenvalues"]))
    without = dftk.compute_bands(basis, dftk.ExplicitKpoints(basis.kcoords_global, basis.kweights_global), n_bands=4, tol=1e-9,
                                 rho=res["rho"])
    moved = max(np.max(np.abs(a - b)) for a, b in zip(bands["eigenvalues"], without["eigenvalues"]))
    print(f"SCF mesh through compute_bands: {err:.2e}; without hubbard_n the bands sit {moved:.2e} away")
    assert err <= 1e-7 and moved > 1e-4
    keyword = dftk.compute_bands(basis, explicit(GX9[:2]), n_bands=4, tol=1e-9, rho=res["rho"], hubbard_n=res["hubbard_n"])
    from_res = dftk.compute_bands(res, explicit(GX9[:2]), n_bands=4, tol=1e-9)
    assert max(np.max(np.abs(a - b)) for a, b in zip(keyword["eigenvalues"], from_res["eigenvalues"])) <= 2e-9
    # JSON and checkpoint
    for name in ("scf.json", "scf.npz"):
        path = os.path.join(tmp_path, name)
        dftk.save_scfres(path, res)
        back = dftk.load_scfres(path, basis) if name.endswith("npz") else dftk.load_scfres(path)
        assert len(back["hubbard_n"]) == 1 and np.array_equal(back["hubbard_n"][0], res["hubbard_n"][0])
        assert "Hubbard" in back["terms"] and back["energies"]["Hubbard"] == res["energies"]["Hubbard"]
    # a restart takes its first step with the operator in place, and stays converged
    stepper = dftk.ScfStepper(basis, rho=back["rho"], psi=back["psi"], hubbard_n=back["hubbard_n"], tol=1e-8)
    info = stepper.step()
    assert info["ham"][0].hubbard is not None
    print(f"restart: first step |rho_out - rho_in| = {info['history_drho'][-1]:.2e}")
    assert info["history_drho"][-1] <= 1e-7
    with pytest.raises(ValueError, match="no Hubbard term"):
        dftk.ScfStepper(plain_scf()["basis"], hubbard_n=back["hubbard_n"])


def test_compute_hubbard_n_between_scf_steps_leaves_the_scf_bit_identical():
    def run(extra):
        basis = si_basis(hubbard_of(("3P", 0.2)))
        seen = []

        def cb(info):
            if extra:
                seen.append(dftk.compute_hubbard_n(basis, info["psi"], info["occupation"]))
        return dftk.self_consistent_field(basis, tol=1e-9, callback=cb), seen
    ref, _ = run(False)
    got, seen = run(True)
    assert len(seen) >= 3 and np.array_equal(seen[-1][0], got["hubbard_n"][0])
    assert got["energies"].total == ref["energies"].total and got["n_iter"] == ref["n_iter"]
    assert torch.equal(got["rho"], ref["rho"]) and np.array_equal(got["hubbard_n"][0], ref["hubbard_n"][0])
    for a, b in zip(got["eigenvalues"], ref["eigenvalues"]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_on_the_device():
    res = u_scf()
    for call in (dftk.compute_forces, dftk.compute_forces_cart, dftk.compute_stresses_cart, dftk.compute_dynmat):
        with pytest.raises(NotImplementedError, match="Hubbard"):
            call(res)
    dV = torch.zeros_like(res["rho"])
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.apply_chi0(res, dV)
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.apply_kernel(res["basis"], dV, rho=res["rho"])
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.solve_OmegaPlusK_split(res, [torch.zeros_like(p) for p in res["psi"]])
    # HGH tables carry no pseudo-atomic orbitals
    hgh = si_basis(hubbard_of(("3P", 0.1)), pseudo=dftk.load_psp("Si", "lda"))
    plain = plain_scf()
    with pytest.raises(ValueError, match="no pseudo-atomic orbitals|carries no pseudo-atomic"):
        dftk.compute_hubbard_n(hgh, plain["psi"], plain["occupation"])
    with pytest.raises(ValueError, match="no Hubbard term"):
        dftk.compute_hubbard_n(plain["basis"], plain["psi"], plain["occupation"])
    with pytest.raises(ValueError, match="hubbard_n holds"):
        dftk.energy_hamiltonian(res["basis"], None, None, rho=res["rho"], hubbard_n=[])
