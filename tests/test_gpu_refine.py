"""``refine_scfres`` / ``refine_energies`` / ``refine_forces`` on the device (dftk_jl_amd/refine.py).

1. The reference's own test (test/refine.jl, thresholds and system from there): silicon with atom 1 displaced by
   (-0.022, 0.028, 0.035), LDA, Gamma only, tol 1e-10, Ecut 15 -> 35; relative errors of the energy, the density and the
   forces against the Ecut-35 SCF before (>) and after (<) the refinement; E.total equals the SCF energy to 1e-6.
2. ``refine_energies``: every term of dE against central differences of the pre-existing
   ``energy_hamiltonian(basis_ref, psi + eps dpsi, occ, rho = rho + eps drho)`` at two step sizes (the yardstick is checked
   against itself first), tolerance 1e-8 x the largest term; Ecut 5 -> 9.
3. ``refine_forces``: dF the same way against central differences of ``compute_forces``.
   Both on three systems: Gamma only, two explicit k-points (Gamma and (1/2, 0, 0), complex orbitals), and the UPF species
   with a non-linear core correction of nlcc_gen.py.
4. Consistency: a ``basis_ref`` with the Ecut of the SCF basis gives a density correction at the level of the SCF tolerance;
   a Gamma-real SCF result refines like the complex iteration's; the irreducible 2 x 2 x 2 mesh against the full mesh; the
   SCF state and a following SCF step are unchanged by a refinement; the transferred orbitals stay orthonormal and the
   corrections lie in the tangent space.
5. ``refine_scfres`` against the dense NumPy twin of tests/refine_twin.py (Gamma; Gamma and (1/2, 0, 0)), and ``apply_Omega`` +
   ``apply_K`` against the pre-existing ``solve_OmegaPlusK_split``.
6. The refusals on the device.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402

DEV = "cuda:0"
LDA = ("lda_x", "lda_c_pw")
SHIFT = np.array([-0.022, 0.028, 0.035])
FD_TOL = 1e-8


A_REFERENCE = 2 * 5.131570667152971       # the lattice constant of the reference's test cases (test/testcases.jl:13-15)


def displaced_model(**kw):
    lat, atoms, pos = dftk.silicon_cell(a=A_REFERENCE)
    pos = [np.asarray(p, dtype=float).copy() for p in pos]
    pos[0] = pos[0] + SHIFT
    return dftk.model_DFT(lat, atoms, pos, functionals=LDA, **kw)


def gamma_basis(model, Ecut, **kw):
    return dftk.PlaneWaveBasis(model, Ecut, dftk.MonkhorstPack((1, 1, 1)), device=DEV, **kw)


def rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------ 1: the reference's test
@pytest.fixture(scope="module")
def reference_case():
    model = displaced_model()
    tol = 1e-10
    basis = gamma_basis(model, 15)
    scfres = dftk.self_consistent_field(basis, tol=tol)
    basis_ref = gamma_basis(model, 35)
    refinement = dftk.refine_scfres(scfres, basis_ref, tol=tol)
    scfres_ref = dftk.self_consistent_field(basis_ref, tol=tol)
    return dict(scfres=scfres, refinement=refinement, scfres_ref=scfres_ref)


def test_reference_refinement_of_energy_density_and_forces(reference_case):
    scfres, refinement, scfres_ref = (reference_case[k] for k in ("scfres", "refinement", "scfres_ref"))
    assert scfres["converged"] and scfres_ref["converged"] and refinement.OmegaPlusK_res["converged"]
    en = dftk.refine_energies(refinement)
    E, dE = en["E"], en["dE"]
    F, dF = dftk.refine_forces(refinement)
    E_ref = scfres_ref["energies"].total
    assert abs(E.total - scfres["energies"].total) <= 1e-6 * abs(scfres["energies"].total)
    before = dict(E=abs(E.total - E_ref) / abs(E_ref), rho=rel(refinement.rho.cpu().numpy(), scfres_ref["rho"].cpu().numpy()))
    after = dict(E=abs(E.total + dE.total - E_ref) / abs(E_ref),
                 rho=rel((refinement.rho + refinement.drho).cpu().numpy(), scfres_ref["rho"].cpu().numpy()))
    F_ref = dftk.compute_forces(scfres_ref)
    before["F"], after["F"] = rel(F, F_ref), rel(F + dF, F_ref)
    print(f"\nrefinement 15 -> 35: relative errors before {before}, after {after}")
    assert before["E"] > 2e-4 and after["E"] < 1.5e-4
    assert before["rho"] > 3e-3 and after["rho"] < 1.5e-3
    assert before["F"] > 5e-3 and after["F"] < 2e-3


def test_result_fields_and_tangent_space(reference_case):
    r = reference_case["refinement"]
    basis_ref = r.basis
    assert r.psi[0].shape == (4, basis_ref.kpoints[0].n_G) and r.dpsi[0].shape == r.psi[0].shape
    assert r.rho.shape == r.drho.shape and "dpsi" not in r.OmegaPlusK_res
    p, d = r.psi[0].cpu().numpy(), r.dpsi[0].cpu().numpy()
    assert np.abs(p.conj() @ p.T - np.eye(4)).max() < 1e-12          # the transfer keeps the orbitals orthonormal
    assert np.abs(p.conj() @ d.T).max() < 1e-10                      # psi' dpsi = 0
    assert abs(float(r.drho.sum().item())) * basis_ref.dvol < 1e-10  # no charge in the correction


# ------------------------------------------------------------------------------------------ 2, 3: derivatives
TWO_K = dftk.ExplicitKpoints([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], [0.5, 0.5])
_CASES = {}


def build_case(kind):
    """Ecut 5 -> 9 in the displaced cell: "gamma" (HGH, Gamma only, the automatic Gamma-real SCF), "complex" (the same with
    the general complex iteration), "two_k" (Gamma and (1/2, 0, 0) with weights 1/2: complex orbitals at a k-point that is
    not its own inverse image under the transfer's dG = 0), "nlcc" (the UPF species of nlcc_gen.py with a core density)"""
    if kind not in _CASES:
        if kind == "nlcc":
            import nlcc_gen
            lat, _, pos = dftk.silicon_cell(a=A_REFERENCE)
            pos = [np.asarray(p, dtype=float).copy() for p in pos]
            pos[0] = pos[0] + SHIFT
            model = dftk.model_DFT(lat, [dftk.ElementPsp("Si", psp=nlcc_gen.core_psp("Si", "lda", core=True))] * 2, pos,
                                   functionals=LDA)
        else:
            model = displaced_model()
        kgrid = TWO_K if kind == "two_k" else dftk.MonkhorstPack((1, 1, 1))
        kw = dict(gamma_real=False) if kind == "complex" else {}
        basis = dftk.PlaneWaveBasis(model, 5, kgrid, device=DEV, **kw)
        scfres = dftk.self_consistent_field(basis, tol=1e-10)
        basis_ref = dftk.PlaneWaveBasis(model, 9, kgrid, device=DEV, **kw)
        _CASES[kind] = dict(scfres=scfres, refinement=dftk.refine_scfres(scfres, basis_ref, tol=1e-10))
    return _CASES[kind]


@pytest.fixture(scope="module")
def small_case():
    return build_case("gamma")


@pytest.fixture(params=["gamma", "two_k", "nlcc"])
def fd_case(request):
    return build_case(request.param)


def central(f, h):
    return (f(h) - f(-h)) / (2 * h)


def test_refine_energies_against_central_differences(fd_case):
    r = fd_case["refinement"]
    names = list(r.basis.model.term_types)

    def energies(eps):
        psi = [p + eps * d for p, d in zip(r.psi, r.dpsi)]
        E, _ = dftk.energy_hamiltonian(r.basis, psi, r.occupation, rho=r.rho + eps * r.drho, only_energies=True)
        return np.array([E[n] for n in names])

    fine, coarse = central(energies, 1e-3), central(energies, 2e-3)
    scale = np.abs(fine).max()
    print(f"\nyardstick: largest term {scale:.6e}, step 2e-3 vs 1e-3: {np.abs(fine - coarse).max() / scale:.3e}")
    assert np.abs(fine - coarse).max() <= FD_TOL * scale          # the yardstick against itself
    yard = (4 * fine - coarse) / 3
    en = dftk.refine_energies(r)
    for n, y in zip(names, yard):
        print(f"dE {n}: {en['dE'][n]:+.12e}, yardstick {y:+.12e}, |diff| / scale {abs(en['dE'][n] - y) / scale:.3e}")
    for n, y in zip(names, yard):
        assert abs(en["dE"][n] - y) <= FD_TOL * scale, n
    assert abs(en["dE"].total - yard.sum()) <= FD_TOL * scale
    E0 = energies(0.0)
    for n, e in zip(names, E0):
        assert abs(en["E"][n] - e) <= 1e-12 * max(1.0, abs(e)), n


def test_refine_forces_against_central_differences(fd_case):
    r = fd_case["refinement"]

    def forces(eps):
        psi = [p + eps * d for p, d in zip(r.psi, r.dpsi)]
        return dftk.compute_forces(r.basis, psi, r.occupation, rho=r.rho + eps * r.drho)

    fine, coarse = central(forces, 1e-3), central(forces, 2e-3)
    scale = np.abs(fine).max()
    print(f"\nforce yardstick: largest component {scale:.6e}, step 2e-3 vs 1e-3: {np.abs(fine - coarse).max() / scale:.3e}")
    assert np.abs(fine - coarse).max() <= FD_TOL * scale
    yard = (4 * fine - coarse) / 3
    F, dF = dftk.refine_forces(r)
    print(f"dF: |device - yardstick| / scale = {np.abs(dF - yard).max() / scale:.3e}")
    assert np.abs(dF - yard).max() <= FD_TOL * scale
    assert np.abs(F - forces(0.0)).max() <= 1e-12


# ------------------------------------------------------------------------------------------ against the dense twin
REFINE_MEASURED = 3.5e-11       # drho 2.1e-11 (Gamma) / 3.5e-11 (two k-points), e2 1.5e-15, density matrix change 3.2e-11
REFINE_TOL = min(1e-6, 10 * REFINE_MEASURED)


def dense_of(ham_k):
    """the dense matrix of a Hamiltonian block from ``mul_`` on the identity (as the response tests build it)"""
    n = ham_k.n_G
    eye = torch.eye(n, dtype=torch.complex128, device=DEV)
    return (ham_k @ eye).cpu().numpy().T


def twin_side(basis, ham, rho):
    import oracle.terms as ot
    import refine_twin as twin

    def v_xc(r):
        return sum(ot._FUNCTIONALS[name](r)[1] for name in basis.model.functionals)
    return dict(fft_size=basis.fft_size, volume=basis.model.unit_cell_volume, recip=np.asarray(basis.model.recip_lattice),
                weights=list(basis.kweights), mappings=[k.mapping for k in basis.kpoints], H=[dense_of(h) for h in ham],
                kin=[k.kinetic.cpu().numpy() for k in basis.kpoints], fxc=twin.fxc_central(v_xc, rho.cpu().numpy()))


@pytest.mark.parametrize("kind", ["gamma", "two_k"])
def test_refine_scfres_against_the_dense_twin(kind):
    """Ecut 5 -> 9, Gamma only or Gamma and (1/2, 0, 0) with weights 1/2, the general complex iteration, device tolerance 1e-11, against ``refine_scfres_dense`` of
    tests/refine_twin.py: dense H of both bases (``mul_`` on the identity), f_xc from central differences of the oracle's
    v_xc, (Omega + K)_11 inverted exactly on a real basis of the tangent space (1064 dimensions).  Compared: the density
    correction, e2 = M^-1 resHF, and dpsi through the change of the density matrix dpsi psi' + psi dpsi'.  The largest of the
    three relative errors measured on the MI355X is REFINE_MEASURED; the assertion is ten times it, never more than 1e-6."""
    import refine_twin as twin
    model = displaced_model()
    kgrid = TWO_K if kind == "two_k" else dftk.MonkhorstPack((1, 1, 1))
    basis = dftk.PlaneWaveBasis(model, 5, kgrid, device=DEV, gamma_real=False)
    scfres = dftk.self_consistent_field(basis, tol=1e-12)
    basis_ref = dftk.PlaneWaveBasis(model, 9, kgrid, device=DEV, gamma_real=False)
    r = dftk.refine_scfres(scfres, basis_ref, tol=1e-11)
    occ = r.occupation
    nk = len(basis.kpoints)
    psi = [p[:4].cpu().numpy().T for p in scfres["psi"]]
    # the large side from pre-existing entry points, fed with the TWIN's transfers
    psir_t = [twin.transfer_blochwave_kpt(psi[k], basis.kpoints[k].mapping, basis.fft_size, basis_ref.kpoints[k].mapping,
                                          basis_ref.fft_size) for k in range(nk)]
    rhor_t = twin.transfer_density(scfres["rho"].cpu().numpy(), basis.fft_size, basis_ref.fft_size)
    psir_d = [torch.from_numpy(np.ascontiguousarray(p.T)).to(DEV) for p in psir_t]
    rhor_d = torch.from_numpy(rhor_t).to(DEV)
    _, hamr = dftk.energy_hamiltonian(basis_ref, psir_d, occ, rho=rhor_d)
    large = twin_side(basis_ref, hamr, rhor_d)
    _, hamg = dftk.energy_hamiltonian(basis_ref, psir_d, occ, rho=dftk.compute_density(basis_ref, psir_d, occ))
    large["Hgrad"] = [dense_of(h) for h in hamg]
    small = twin_side(basis, scfres["ham"], scfres["rho"])
    ref = twin.refine_scfres_dense(small, large, psi, occ)
    # the device's e2 from its public pieces
    res = [-g for g in dftk.compute_projected_gradient(basis_ref, r.psi, occ)]
    resLF = dftk.transfer_blochwave(res, basis_ref, basis)
    resHF = [a - b for a, b in zip(res, dftk.transfer_blochwave(resLF, basis, basis_ref))]
    e2 = [x.cpu().numpy().T for x in dftk.invert_refinement_metric(basis_ref, r.psi, resHF)]
    dpsi, psir = [x.cpu().numpy().T for x in r.dpsi], [x.cpu().numpy().T for x in r.psi]
    assert all(np.array_equal(a, b) for a, b in zip(psir, psir_t))

    def dP(p, d):
        return d @ p.conj().T + p @ d.conj().T
    errs = dict(drho=np.abs(r.drho.cpu().numpy() - ref["drho"]).max() / np.abs(ref["drho"]).max(),
                e2=max(np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(e2, ref["e2"])),
                dP=max(np.linalg.norm(dP(p, a) - dP(p, b)) / np.linalg.norm(dP(p, b))
                       for p, a, b in zip(psir, dpsi, ref["dpsi"])))
    print(f"\nrefine_scfres against the dense twin, {kind}: {errs} (bound {REFINE_TOL:.1e})")
    assert max(errs.values()) < REFINE_TOL


def test_invert_refinement_metric_warns_instead_of_failing(small_case):
    r = small_case["refinement"]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(3)
    re, im = (torch.randn(r.psi[0].shape, generator=gen, device=DEV, dtype=torch.float64) for _ in range(2))
    res = [torch.complex(re, im)]
    with pytest.warns(UserWarning, match="did not converge"):
        x = dftk.invert_refinement_metric(r.basis, r.psi, res, maxiter=1)
    assert bool(torch.isfinite(x[0].abs()).all())
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        x = dftk.invert_refinement_metric(r.basis, r.psi, res, maxiter=200)      # converges: no warning
    assert float((r.psi[0].conj() @ x[0].T).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------ the Hessian pieces
OMEGA_K_MEASURED = 1.4e-11      # Gamma 8.7e-12, two k-points 1.3e-11
OMEGA_K_TOL = min(1e-6, 10 * OMEGA_K_MEASURED)


@pytest.mark.parametrize("kind", ["gamma", "two_k"])
def test_apply_Omega_plus_apply_K_undo_the_split_solver(kind):
    """``apply_Omega`` + ``apply_K`` against the pre-existing ``solve_OmegaPlusK_split``: its answer d to a random
    perturbation dH psi satisfies (Omega + K) d = -P dH psi (hessian.jl:111-114) -- the sign convention ``refine_scfres`` relies
    on when it hands its right-hand side over.  The bound is that of the solver (tolerance 1e-11 on the density): the largest
    relative residual measured on the MI355X, times ten, never more than 1e-6."""
    from dftk_jl_amd.refine import proj_tangent, rayleigh_coefficients
    scfres = build_case(kind)["scfres"]
    basis = scfres["basis"]
    psi, occ = dftk.select_occupied_orbitals(basis, scfres["psi"], scfres["occupation"], threshold=scfres["occupation_threshold"])
    psi = [p.contiguous() for p in psi]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    dH = []
    for p_all, p in zip(scfres["psi"], psi):
        full = torch.zeros_like(p_all)
        re, im = (torch.randn(p.shape, generator=gen, device=DEV, dtype=torch.float64) for _ in range(2))
        full[:p.shape[0]] = 1e-2 * torch.complex(re, im)
        dH.append(full)
    sol = dftk.solve_OmegaPlusK_split(scfres, dH, tol=1e-11)
    assert sol["converged"]
    d = [x[:p.shape[0]].contiguous() for x, p in zip(sol["dpsi"], psi)]
    lhs = [a + b for a, b in zip(dftk.apply_Omega(d, psi, scfres["ham"], rayleigh_coefficients(scfres["ham"], psi)),
                                 dftk.apply_K(basis, d, psi, scfres["rho"], occ))]
    rhs = proj_tangent(basis, [x[:p.shape[0]] for x, p in zip(dH, psi)], psi)
    err = max(float(torch.linalg.norm(a + b) / torch.linalg.norm(b)) for a, b in zip(lhs, rhs))
    print(f"\n(Omega + K) d + P dH psi, {kind}: relative residual {err:.3e} (bound {OMEGA_K_TOL:.1e})")
    assert err < OMEGA_K_TOL


# ------------------------------------------------------------------------------------------ 4: consistency
def test_same_ecut_gives_a_correction_at_the_scf_tolerance(small_case):
    scfres = small_case["scfres"]
    basis = scfres["basis"]
    twin = gamma_basis(basis.model, 5)
    r = dftk.refine_scfres(scfres, twin, tol=1e-10)
    nrm = float(torch.linalg.norm(r.drho).item()) * np.sqrt(twin.dvol)
    print(f"\nsame Ecut: ||drho|| = {nrm:.3e}")
    assert nrm < 1e-8                                   # the SCF stopped at ||rho_out - rho_in|| < 1e-10
    assert torch.equal(r.psi[0], scfres["psi"][0][:4])  # the transfer onto the same sphere moves every number to its row


def test_gamma_real_and_complex_scf_results_refine_alike():
    """A Gamma-real SCF result is accepted as ``apply_chi0`` accepts one, and refines to the same corrections as the result
    of the general complex iteration, within the bound of the self-consistent response (SPLIT_TOL of test_gpu_response.py:
    the two SCFs and the two response solves each stop at their own tolerance)."""
    from test_gpu_response import SPLIT_TOL
    real, cplx = build_case("gamma"), build_case("complex")
    assert real["scfres"]["basis"].kpoints[0].gamma_real and not cplx["scfres"]["basis"].kpoints[0].gamma_real
    a, b = real["refinement"], cplx["refinement"]
    err = float((a.drho - b.drho).abs().max() / b.drho.abs().max())
    dEa, dEb = dftk.refine_energies(a)["dE"], dftk.refine_energies(b)["dE"]
    big = max(abs(v) for v in dEb.values())
    errE = max(abs(dEa[n] - dEb[n]) for n in dEb) / big
    print(f"\nGamma-real against complex: drho {err:.3e}, dE {errE:.3e} (bound {SPLIT_TOL:.1e})")
    assert err < SPLIT_TOL and errE < SPLIT_TOL


def test_irreducible_mesh_against_the_full_mesh():
    """2 x 2 x 2 in the undisplaced cell (48 symmetries with the HGH species): the refinement on the irreducible k-points,
    with the symmetrised density correction, against the full mesh."""
    from test_gpu_response import SPLIT_TOL
    lat, atoms, pos = dftk.silicon_cell(a=A_REFERENCE)
    model = dftk.model_DFT(lat, atoms, pos, functionals=LDA, symmetries=True)
    out = []
    for reduce_k in (True, False):
        kw = dict(use_symmetries_for_kpoint_reduction=reduce_k)
        basis = dftk.PlaneWaveBasis(model, 5, dftk.MonkhorstPack((2, 2, 2)), device=DEV, **kw)
        scfres = dftk.self_consistent_field(basis, tol=1e-10)
        basis_ref = dftk.PlaneWaveBasis(model, 9, dftk.MonkhorstPack((2, 2, 2)), device=DEV, **kw)
        r = dftk.refine_scfres(scfres, basis_ref, tol=1e-10)
        out.append((len(basis.kpoints), r, dftk.refine_energies(r)))
    (n_irr, a, ea), (n_full, b, eb) = out
    assert n_irr < n_full == 8
    err = float((a.drho - b.drho).abs().max() / b.drho.abs().max())
    big = max(abs(v) for v in eb["dE"].values())
    errE = max(abs(ea["dE"][n] - eb["dE"][n]) for n in eb["dE"]) / big
    print(f"\nirreducible ({n_irr} k-points) against full mesh: drho {err:.3e}, dE {errE:.3e} (bound {SPLIT_TOL:.1e})")
    assert err < SPLIT_TOL and errE < SPLIT_TOL
    assert abs(ea["E"].total - eb["E"].total) < 1e-8


def test_a_refinement_leaves_the_scf_state_alone():
    energies = []
    for with_refinement in (False, True):
        model = displaced_model()
        basis = gamma_basis(model, 5)
        stepper = dftk.ScfStepper(basis, tol=1e-12)
        for _ in range(8):
            info = stepper.step()
        if with_refinement:
            res = dict(info, basis=basis, occupation_threshold=stepper.nbandsalg.occupation_threshold)
            r = dftk.refine_scfres(res, gamma_basis(model, 9), tol=1e-8)
            assert float(r.drho.abs().max()) > 0
        energies.append([stepper.step()["energies"].total for _ in range(2)])
    print(f"\ncontinued SCF energies without / with a refinement: {energies}")
    assert np.abs(np.array(energies[0]) - np.array(energies[1])).max() < 1e-13


# ------------------------------------------------------------------------------------------ 5: refusals
def test_out_of_scope_requests_are_refused(small_case):
    scfres = small_case["scfres"]
    lat, atoms, pos = dftk.silicon_cell()
    pbe = dftk.model_DFT(lat, atoms, pos, functionals=("gga_x_pbe", "gga_c_pbe"))
    with pytest.raises(NotImplementedError, match="GGA"):
        dftk.refine_scfres(scfres, gamma_basis(pbe, 9))
    with pytest.raises(NotImplementedError, match="collinear spin"):
        dftk.refine_scfres(scfres, gamma_basis(dftk.model_DFT(lat, atoms, pos, functionals=LDA, magnetic_moments=[1.0, 1.0]), 9))
    with pytest.raises(NotImplementedError, match="exact exchange"):
        dftk.refine_scfres(scfres, gamma_basis(dftk.model_HF(lat, atoms, pos), 9))
    import hubbard_gen
    Si = dftk.ElementPsp("Si", psp=hubbard_gen.hubbard_psp())
    plus_u = dftk.model_DFT(lat, [Si, Si], pos, functionals=LDA,
                            extra_terms=[dftk.Hubbard((dftk.OrbitalManifold("Si", "3P"), 0.1))])
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.refine_scfres(scfres, gamma_basis(plus_u, 9))
    with pytest.raises(ValueError, match="temperature"):
        dftk.refine_scfres(scfres, gamma_basis(displaced_model(temperature=0.01), 9))
    # ... and with the offending model on the side of the SCF result (only its descriptors are read before the refusal)
    for model, exc, word in ((dftk.model_DFT(lat, atoms, pos, functionals=LDA, magnetic_moments=[1.0, 1.0]),
                              NotImplementedError, "collinear spin"),
                             (dftk.model_HF(lat, atoms, pos), NotImplementedError, "exact exchange"),
                             (plus_u, NotImplementedError, "Hubbard"),
                             (displaced_model(temperature=0.01), ValueError, "temperature")):
        with pytest.raises(exc, match=word):
            dftk.refine_scfres(dict(scfres, basis=gamma_basis(model, 5)), gamma_basis(scfres["basis"].model, 9))
    with pytest.raises(ValueError, match="k-point"):
        dftk.refine_scfres(scfres, dftk.PlaneWaveBasis(scfres["basis"].model, 9, dftk.MonkhorstPack((2, 1, 1)), device=DEV))
    with pytest.raises(ValueError, match="contain"):
        dftk.refine_scfres(scfres, gamma_basis(scfres["basis"].model, 3))
    other = dftk.model_DFT(1.01 * np.asarray(lat), atoms, pos, functionals=LDA)
    with pytest.raises(ValueError, match="lattice"):
        dftk.refine_scfres(scfres, gamma_basis(other, 9))
    partial = dict(scfres, occupation=[np.array([2.0, 2.0, 2.0, 1.0] + [0.0] * (len(scfres["occupation"][0]) - 4))])
    with pytest.raises(ValueError, match="full occupation"):
        dftk.refine_scfres(partial, gamma_basis(scfres["basis"].model, 9))
