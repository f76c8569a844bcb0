"""``unfold_bz`` and the Wannier interface end to end on the GPU: silicon, LDA, Ecut 5, every SCF converged to 1e-10.

A. ``unfold_bz(scfres)`` of a symmetric 2x2x2 mesh, a shifted 3x3x3 mesh and a collinear-spin 2x2x2 run (equal moments on
   both atoms keep the whole group): total energy to 1.5e-8 relative, psi' psi = I to n_G eps, the eigenvalue residual of
   every band with the unfolded Hamiltonian at most twice its residual at the irreducible point (Hamiltonian of the same
   density) plus n_G eps |H| with |H| taken as Ecut (a lower estimate: the bound is the stricter for it), the density of the
   unfolded state equal to the result's to 1e-12 relative, the input left bit for bit alone.
B. The unfolded 4x4x4 state against a full-mesh SCF of the same cell, 4 valence bands: singular values of every M^{k,b} and
   Omega_I within 10x the difference between two full-mesh SCFs from different seeds.
C. The gauge check on the device path (n_G eps per (k, b) with that k-point's n_G), ``compute_amn`` against the twin, ``projection_gauge`` lowering Omega_OD + Omega_D,
   the centres of bond-centred Gaussians on the bond midpoints, ``write_wannier90_files`` parsed back, the refusals.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd.wannier import HARTREE_TO_EV  # noqa: E402

import wannier_twin as twin  # noqa: E402

EPS = np.finfo(float).eps
ECUT = 5
N_W = 4
# the four bonds of the atom at (1/8, 1/8, 1/8) end on the atom at -(1/8, 1/8, 1/8) and its images by a_1, a_2, a_3
BOND_CENTRES = [np.zeros(3), np.array([0.5, 0, 0]), np.array([0, 0.5, 0]), np.array([0, 0, 0.5])]


def silicon_model(functionals=("lda_x", "lda_c_vwn"), **kw):
    lat, atoms, pos = dftk.silicon_cell()
    return dftk.model_DFT(lat, atoms, pos, functionals=functionals, symmetries=True, **kw)


def run_scf(mesh, shift=(0, 0, 0), reduce=True, seed=0, **model_kw):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    basis = dftk.PlaneWaveBasis(silicon_model(**model_kw), ECUT, dftk.MonkhorstPack(mesh, shift),
                                use_symmetries_for_kpoint_reduction=reduce)
    res = dftk.self_consistent_field(basis, tol=1e-10, seed=seed)
    assert res["converged"]
    return res


_RUNS = {}


def cached(key, make):
    if key not in _RUNS:
        _RUNS[key] = make()
    return _RUNS[key]


def irreducible(case):
    return cached(("irr", case), {"2x2x2": lambda: run_scf((2, 2, 2)),
                                  "3x3x3-shifted": lambda: run_scf((3, 3, 3), (0.5, 0.5, 0.5)),
                                  # (the spin-polarised LDA forms of the library: lda_x + lda_c_pw)
                                  "2x2x2-spin": lambda: run_scf((2, 2, 2), magnetic_moments=[1.0, 1.0],
                                                                functionals=("lda_x", "lda_c_pw")),
                                  "4x4x4": lambda: run_scf((4, 4, 4))}[case])


def unfolded_444():
    return cached("unf444", lambda: dftk.unfold_bz(irreducible("4x4x4")))


def wannier_444():
    """unfolded 4x4x4 state, its neighbours, overlaps and bond-centred projections: computed once, never modified"""
    def make():
        res = unfolded_444()
        nnkp = dftk.compute_nnkp(res["basis"])
        projections = [dftk.GaussianWannierProjection(c) for c in BOND_CENTRES]
        M = dftk.compute_mmn(res["basis"], res["psi"], nnkp, N_W)
        A = dftk.compute_amn(res["basis"], res["psi"], projections, N_W)
        return dict(res=res, nnkp=nnkp, projections=projections, M=M, A=A)
    return cached("w444", make)


def snapshot(res):
    return dict(psi=[p.clone() for p in res["psi"]], rho=res["rho"].clone(), eig=[np.array(e, copy=True) for e in res["eigenvalues"]],
                occ=[np.array(o, copy=True) for o in res["occupation"]], basis=res["basis"], n_k=len(res["basis"].kpoints))


def band_residuals(ham, psi, eigenvalues):
    out = []
    for H, p, e in zip(ham, psi, eigenvalues):
        lam = torch.as_tensor(np.asarray(e), dtype=torch.float64, device=p.device)
        out.append(torch.linalg.norm((H @ p) - lam[:, None] * p, dim=1).cpu().numpy())
    return out


# ======================================================================================================= A
@pytest.mark.parametrize("case", ["2x2x2", "3x3x3-shifted", "2x2x2-spin"])
def test_unfold_bz_of_an_scf(case):
    res = irreducible(case)
    basis = res["basis"]
    n_spin = basis.model.n_spin_components
    before = snapshot(res)
    unf = dftk.unfold_bz(res)
    ub = unf["basis"]
    mesh = basis.kgrid.kgrid_size
    assert len(basis.kpoints) < len(ub.kpoints) == n_spin * int(np.prod(mesh))
    assert len(basis.symmetries) > 1 and ub.fft_size == basis.fft_size
    # the input is left alone, bit for bit
    assert res["basis"] is before["basis"] and len(res["psi"]) == before["n_k"] == len(basis.kpoints)
    assert all(torch.equal(torch.view_as_real(a), torch.view_as_real(b)) for a, b in zip(res["psi"], before["psi"]))
    assert torch.equal(res["rho"], before["rho"])
    assert all(np.array_equal(a, b) for a, b in zip(res["eigenvalues"], before["eig"]))
    assert all(np.array_equal(a, b) for a, b in zip(res["occupation"], before["occ"]))
    assert unf["rho"] is res["rho"] and unf["eF"] == res["eF"] and unf["energies"] is res["energies"]
    # total energy
    E, ham_unf = dftk.energy_hamiltonian(ub, unf["psi"], unf["occupation"], rho=res["rho"], eigenvalues=unf["eigenvalues"],
                                         eF=res["eF"])
    E_ref = float(res["energies"].total)
    print(f"\nunfold_bz {case}: E {float(E.total):.12f} vs {E_ref:.12f}, relative {abs(float(E.total) - E_ref) / abs(E_ref):.2e}")
    assert abs(float(E.total) - E_ref) <= 1.5e-8 * abs(E_ref)
    # orthonormality
    for kpt, p in zip(ub.kpoints, unf["psi"]):
        G = (p.conj() @ p.T).cpu().numpy()
        assert np.max(np.abs(G - np.eye(len(G)))) <= kpt.n_G * EPS
    # residuals: the same density on both sides
    _, ham_irr = dftk.energy_hamiltonian(basis, res["psi"], res["occupation"], rho=res["rho"], eigenvalues=res["eigenvalues"],
                                         eF=res["eF"])
    r_irr = band_residuals(ham_irr, res["psi"], res["eigenvalues"])
    r_unf = band_residuals(ham_unf, unf["psi"], unf["eigenvalues"])
    worst = 0.0
    for kpt, r in zip(ub.kpoints, r_unf):
        ik, _ = dftk.unfold_mapping(basis, kpt)
        bound = 2 * r_irr[ik] + kpt.n_G * EPS * ECUT
        worst = max(worst, float(np.max(r / bound)))
        assert np.all(r <= bound), (kpt.coordinate, r, r_irr[ik])
    print(f"unfold_bz {case}: worst residual / bound = {worst:.3f}")
    # density
    rho = dftk.compute_density(ub, unf["psi"], unf["occupation"])
    drho = float(torch.linalg.norm(rho - res["rho"]) / torch.linalg.norm(res["rho"]))
    print(f"unfold_bz {case}: relative density difference {drho:.2e}")
    assert drho <= 1e-12


def test_apply_symop_python_layer():
    res = irreducible("2x2x2")
    basis = res["basis"]
    ik = next(i for i, k in enumerate(basis.kpoints) if k.coordinate.any())
    kpt, psi = basis.kpoints[ik], res["psi"][ik]
    ident = basis.symmetries[0]
    assert ident.isone() and dftk.apply_symop(ident, basis, kpt, psi) == (kpt, psi)
    op = next(s for s in basis.symmetries if s.tau.any())
    Skpt, out = dftk.apply_symop(op, basis, kpt, psi)
    Sk, kshift = twin.symop_image(op.S, kpt.coordinate)
    assert np.allclose(Skpt.coordinate, Sk) and out.shape == (psi.shape[0], Skpt.n_G)
    ref, _ = twin.apply_symop(op.S, op.tau, kshift, kpt.mapping, Skpt.mapping, basis.fft_size, psi.cpu().numpy().T)
    assert np.max(np.abs(out.cpu().numpy().T - ref.astype(complex))) <= 64 * EPS * float(psi.abs().max())
    _, one = dftk.apply_symop(op, basis, kpt, psi[1])                     # a single orbital
    assert one.shape == (Skpt.n_G,) and torch.equal(torch.view_as_real(one), torch.view_as_real(out[1]))
    with pytest.raises(TypeError):
        dftk.apply_symop(op, basis, kpt, psi.cpu())
    with pytest.raises(ValueError):
        dftk.apply_symop(op, basis, kpt, psi[:, :-1].contiguous())
    shear = dftk.symmetry.SymOp.make(np.array([[1, 0, 0], [1, 1, 0], [0, 0, 1]]), np.zeros(3))
    with pytest.raises(dftk.DftkMiError):                                  # not a symmetry of the sphere
        dftk.apply_symop(shear, basis, kpt, psi)


# ======================================================================================================= B
def singular_values(M):
    return np.linalg.svd(M, compute_uv=False)


def test_unfolded_state_against_full_mesh_scf():
    w = wannier_444()
    ub, nnkp = w["res"]["basis"], w["nnkp"]
    full = [cached(("full", seed), lambda s=seed: run_scf((4, 4, 4), reduce=False, seed=s)) for seed in (0, 1)]
    for f in full:
        assert len(f["basis"].kpoints) == len(ub.kpoints) == 64
        assert all(np.array_equal(a.coordinate, b.coordinate) for a, b in zip(f["basis"].kpoints, ub.kpoints))
    Mf = [dftk.compute_mmn(f["basis"], f["psi"], nnkp, N_W) for f in full]
    sv_u, sv_0, sv_1 = singular_values(w["M"]), singular_values(Mf[0]), singular_values(Mf[1])
    om_u, om_0, om_1 = (dftk.wannier_spreads(M, nnkp)["omega_I"] for M in (w["M"], Mf[0], Mf[1]))
    floor_sv, floor_om = float(np.max(np.abs(sv_0 - sv_1))), abs(om_0 - om_1)
    d_sv, d_om = float(np.max(np.abs(sv_u - sv_0))), abs(om_u - om_0)
    print(f"\nfull-mesh SCF, two seeds: Omega_I {om_0:.12f} / {om_1:.12f}, noise floor {floor_om:.3e} (Omega_I), {floor_sv:.3e} "
          f"(singular values); unfolded against full: {d_om:.3e}, {d_sv:.3e}")
    assert om_u > 0
    # measured on one MI355X: the two full-mesh runs differ by 6.5e-10 bohr^2 in Omega_I (of 20.73) and by 6.6e-11 in the
    # singular values; the unfolded state is 1.6e-9 and 9.0e-11 away from the first of them
    assert d_sv <= 10 * floor_sv
    assert d_om <= 10 * floor_om


# ======================================================================================================= C
def test_gauge_rotation_on_the_device_path():
    w = wannier_444()
    res, nnkp, M = w["res"], w["nnkp"], w["M"]
    basis = res["basis"]
    rng = np.random.default_rng(11)
    n_k = len(basis.kpoints)
    U = np.stack([np.linalg.qr(rng.standard_normal((N_W, N_W)) + 1j * rng.standard_normal((N_W, N_W)))[0] for _ in range(n_k)])
    rotated = [torch.from_numpy(U[ik].T.copy()).to(p.device) @ p[:N_W] for ik, p in enumerate(res["psi"])]
    M_dev = dftk.compute_mmn(basis, rotated, nnkp, N_W)
    M_host = dftk.rotate_mmn(M, U, nnkp)
    # per (k, b), with that k-point's own number of plane waves
    worst = 0.0
    for ik, kpt in enumerate(basis.kpoints):
        for j in range(nnkp["nntot"]):
            err = float(np.max(np.abs(M_dev[ik, j] - M_host[ik, j])))
            worst = max(worst, err / (kpt.n_G * EPS))
            assert err <= kpt.n_G * EPS, (ik, j, err)
    print(f"\ngauge check: worst max |M(rotated psi) - U' M U| over (k, b) = {worst:.2e} of n_G eps")
    n_G = min(k.n_G for k in basis.kpoints)
    o0, o1 = dftk.wannier_spreads(M, nnkp)["omega_I"], dftk.wannier_spreads(M_dev, nnkp)["omega_I"]
    print(f"gauge check: Omega_I {o0:.15f} -> {o1:.15f}, relative change {abs(o0 - o1) / o0:.2e} (n_G eps = {n_G * EPS:.2e})")
    assert abs(o0 - o1) <= n_G * EPS * o0
    # the identity where no plane wave is shared is the Python layer's rule
    I4 = dftk.overlap_Mmn_k_kpb(basis, res["psi"], 0, 1, (40, 0, 0), N_W)
    assert np.array_equal(I4, np.eye(N_W))
    ik, ikpb, G = nnkp["nnkpts"][5]
    assert np.array_equal(dftk.overlap_Mmn_k_kpb(basis, res["psi"], ik, ikpb, G, N_W), M[ik, 5])
    ref, absM = twin.overlap_Mmn_k_kpb(res["psi"][ik].cpu().numpy().T, basis.kpoints[ik].mapping, res["psi"][ikpb].cpu().numpy().T,
                                       basis.kpoints[ikpb].mapping, basis.fft_size, basis.fft_size, G, N_W)
    assert np.all(np.abs(M[ik, 5] - ref.astype(complex)) <= basis.kpoints[ik].n_G * EPS * absM)


def test_compute_amn_against_the_twin():
    w = wannier_444()
    res = w["res"]
    basis = res["basis"]
    atom = np.ones(3) / 8
    sp3 = [dftk.HydrogenicWannierProjection(atom, 3, 0, 0, 1.6)] + [dftk.HydrogenicWannierProjection(atom, 3, 1, m, 1.6)
                                                                    for m in (-1, 0, 1)]
    for projections, name in ((w["projections"], "Gaussian"), (sp3, "hydrogenic s, p")):
        for ik in (0, 37):
            kpt = basis.kpoints[ik]
            A = dftk.compute_amn_kpoint(basis, kpt, res["psi"][ik], projections, N_W)
            ref = twin.compute_amn_kpoint(basis, kpt.coordinate, kpt.mapping, basis.fft_size, res["psi"][ik].cpu().numpy().T,
                                          projections, N_W)
            err = float(np.max(np.abs(A - ref.astype(complex))))
            # a dot product of n_G terms of two unit vectors, the guess itself good to (333 + 32) eps per entry
            bound = (kpt.n_G + 400) * EPS
            print(f"\ncompute_amn {name}, k-point {ik}: max error {err:.2e} (bound {bound:.2e})")
            assert A.shape == (N_W, len(projections)) and err <= bound
    assert np.array_equal(w["A"][37], dftk.compute_amn_kpoint(basis, basis.kpoints[37], res["psi"][37], w["projections"], N_W))


def test_projected_gauge_localises_on_the_bonds():
    w = wannier_444()
    nnkp, M, A = w["nnkp"], w["M"], w["A"]
    lattice = np.asarray(w["res"]["basis"].model.lattice)
    raw = dftk.wannier_spreads(M, nnkp)
    U = dftk.projection_gauge(A)
    loc = dftk.wannier_spreads(dftk.rotate_mmn(M, U, nnkp), nnkp)
    print(f"\nOmega_I {raw['omega_I']:.6f}; Kohn-Sham gauge Omega_OD + Omega_D = {raw['omega_OD'] + raw['omega_D']:.6f}, projected "
          f"gauge {loc['omega_OD'] + loc['omega_D']:.6f}; spreads {loc['spreads']}")
    assert abs(loc["omega_I"] - raw["omega_I"]) <= 1e-12 * raw["omega_I"]
    assert loc["omega_OD"] + loc["omega_D"] < raw["omega_OD"] + raw["omega_D"]
    # Centres.  The finite-difference centre -sum_b w_b b Im ln M_nn is exact for a function that is symmetric about its centre
    # (odd cumulants vanish); one of spread s^2 and unit skewness is moved by |b|^2 s^3 / 6 (the synthetic host case,
    # tests/test_wannier_host.py::test_centre_finite_difference_error).  The bond orbitals are symmetric about the bond
    # midpoint only up to the accuracy of the SCF, so this is the margin they are given.
    b = np.max(np.linalg.norm(nnkp["bvectors_cart"], axis=1))
    for n, c in enumerate(BOND_CENTRES):
        d = np.linalg.solve(lattice, loc["centers"][n]) - c
        d = lattice @ (d - np.rint(d))
        tol = b ** 2 * loc["spreads"][n] ** 1.5 / 6
        print(f"bond {n}: centre off the midpoint by {np.linalg.norm(d):.3e} bohr (margin {tol:.3e})")
        assert np.linalg.norm(d) <= tol
    # The bond midpoints 0 and 1/2 are their own images under c -> -c modulo the lattice, so the four centres above would not
    # show a sign error (the synthetic host test does).  One function that would: a single Gaussian on the atom at
    # +(1/8, 1/8, 1/8) projected on the four valence bands.  The site symmetry T_d fixes the atom and nothing else nearby,
    # so the centre is the atom; -(1/8, 1/8, 1/8) is 4.4 bohr away and no lattice vector apart.
    res = w["res"]
    atom = np.ones(3) / 8
    A1 = dftk.compute_amn(res["basis"], res["psi"], [dftk.GaussianWannierProjection(atom)], N_W)
    one = dftk.wannier_spreads(dftk.rotate_mmn(M, dftk.projection_gauge(A1), nnkp), nnkp)
    d = np.linalg.solve(lattice, one["centers"][0]) - atom
    d = lattice @ (d - np.rint(d))
    tol = b ** 2 * one["spreads"][0] ** 1.5 / 6
    print(f"atom-centred function: centre off the atom by {np.linalg.norm(d):.3e} bohr (margin {tol:.3e}), spread {one['spreads'][0]:.4f}")
    assert np.linalg.norm(d) <= tol and tol < 1.0


def parse_complex_rows(lines):
    return np.array([complex(float(x.split()[-2]), float(x.split()[-1])) for x in lines])


def test_write_wannier90_files(tmp_path):
    res = irreducible("2x2x2")
    prefix = str(tmp_path / "w90" / "si")
    projections = [dftk.GaussianWannierProjection(c) for c in BOND_CENTRES]
    out = dftk.write_wannier90_files(res, prefix, 5, N_W, projections, wannier_plot=True, num_iter=20)
    basis, psi, nnkp = out["scfres"]["basis"], out["scfres"]["psi"], out["nnkp"]
    n_k, n_bands = len(basis.kpoints), 5
    assert n_k == 8 and sorted(f for f in os.listdir(tmp_path / "w90") if not f.startswith("UNK")) == \
        ["si.amn", "si.eig", "si.mmn", "si.nnkp", "si.win"]
    assert np.array_equal(out["M"], dftk.compute_mmn(basis, psi, nnkp, n_bands))
    assert np.array_equal(out["A"], dftk.compute_amn(basis, psi, projections, n_bands))
    assert dftk.read_w90_nnkp(prefix)["nnkpts"] == nnkp["nnkpts"]
    win = open(prefix + ".win").read()
    assert "num_wann             =   4" in win and "num_bands            =   5" in win and "mp_grid : 2 2 2" in win
    assert "num_iter             =   20" in win and "wannier_plot   = True" in win
    eig = [x.split() for x in open(prefix + ".eig").read().splitlines()]
    assert len(eig) == n_k * n_bands
    for idx, row in enumerate(eig):
        k, n = divmod(idx, n_bands)
        val = float(out["scfres"]["eigenvalues"][k][n]) * HARTREE_TO_EV
        assert (int(row[0]), int(row[1])) == (n + 1, k + 1) and abs(float(row[2]) - val) <= 0.5e-18 + 2 * EPS * abs(val)
    amn = open(prefix + ".amn").read().splitlines()
    assert [int(x) for x in amn[1].split()] == [n_bands, n_k, N_W]
    A_file = parse_complex_rows(amn[2:]).reshape(n_k, N_W, n_bands).transpose(0, 2, 1)
    assert np.max(np.abs(A_file - out["A"])) <= 1e-18 + 4 * EPS
    mmn = open(prefix + ".mmn").read().splitlines()
    assert [int(x) for x in mmn[1].split()] == [n_bands, n_k, nnkp["nntot"]]
    at = 2
    for e, (ik, ikpb, G) in enumerate(nnkp["nnkpts"]):
        assert [int(x) for x in mmn[at].split()] == [ik + 1, ikpb + 1, G[0], G[1], G[2]]
        block = parse_complex_rows(mmn[at + 1:at + 1 + n_bands ** 2]).reshape(n_bands, n_bands).T
        assert np.max(np.abs(block - out["M"][ik, e % nnkp["nntot"]])) <= 1e-18 + 4 * EPS
        at += 1 + n_bands ** 2
    assert at == len(mmn)
    # UNK files: one per k-point, every band normalised on the grid
    nx, ny, nz = basis.fft_size
    unk = open(tmp_path / "w90" / "UNK00003.1").read().splitlines()
    assert unk[0].split() == [str(nx), str(ny), str(nz), "3", str(n_bands)] and len(unk) == 1 + n_bands * nx * ny * nz
    u = parse_complex_rows(unk[1:1 + nx * ny * nz])
    assert abs(np.sum(np.abs(u) ** 2) * basis.dvol - 1) <= 1e-10
    assert len([f for f in os.listdir(tmp_path / "w90") if f.startswith("UNK")]) == n_k


def test_refusals_on_the_device(tmp_path):
    res = irreducible("2x2x2")
    spin = irreducible("2x2x2-spin")
    gauss = dftk.default_wannier_centers(N_W, seed=1)
    with pytest.raises(NotImplementedError, match="spin"):
        dftk.write_wannier90_files(spin, str(tmp_path / "s"), 4, N_W, gauss)
    with pytest.raises(NotImplementedError, match="bands_plot"):
        dftk.write_wannier90_files(res, str(tmp_path / "b"), 4, N_W, gauss, bands_plot=True)
    with pytest.raises(ValueError):
        dftk.write_wannier90_files(res, str(tmp_path / "p"), 4, 3, gauss)
    assert not os.listdir(tmp_path)
    basis = res["basis"]
    with pytest.raises(ValueError, match="unfold"):
        dftk.compute_nnkp(basis)
    unf = dftk.unfold_bz(res)
    nnkp = dftk.compute_nnkp(unf["basis"])
    with pytest.raises(ValueError, match="n_bands"):
        dftk.compute_mmn(unf["basis"], unf["psi"], nnkp, unf["psi"][0].shape[0] + 1)
    with pytest.raises(TypeError):
        dftk.compute_mmn(unf["basis"], [p.cpu() for p in unf["psi"]], nnkp, 2)
    with pytest.raises(TypeError):
        dftk.compute_amn_kpoint(unf["basis"], unf["basis"].kpoints[0], unf["psi"][0], [lambda basis, ps: ps[:, 0]], 2)
    with pytest.raises(RuntimeError, match="total energy"):               # a density that is not the state's
        dftk.unfold_bz(dict(res, rho=res["rho"] * 1.001))
