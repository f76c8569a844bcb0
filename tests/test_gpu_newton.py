"""``newton``, ``solve_OmegaPlusK_cg`` and ``apply_OmegaPlusK`` on the device.

Fixtures: those of test_gpu_direct_minimization.py re-stated -- silicon, LDA, Ecut 3 on a 9^3 cube with the four irreducible
k-points of the 3 x 3 x 3 mesh (the reference's test/scf_compare.jl) -- and a displaced cell at Gamma, Ecut 5, without
symmetries, small enough for the dense twin of tests/refine_twin.py (a tangent space of 2 (n_G - 4) 4 real dimensions).

* Operator: ``apply_OmegaPlusK`` with the real-space cache on and off against ``apply_Omega_dense + apply_K_dense``; the error
  of the existing ``refine.apply_Omega + apply_K`` against the same twin is measured in the same test and both new paths must
  be within 4 x that (fp64 chains of the same length; the factor covers another summation order).
* The reference's self-adjointness test (test/hessian.jl:102-113) and its scf_compare test of Newton (:24-33).
* Residual: (Omega + K) dpsi + P rhs rebuilt with the EXISTING ``apply_Omega + apply_K``: weighted norm <= 2 tol for
  tol = 1e-6, 1e-8, 1e-10; dpsi against ``solve_OmegaPlusK_dense`` within 2 tol / lambda_min, lambda_min the smallest
  eigenvalue of the twin's dense operator on the tangent space, computed here.
* Consistency with ``solve_OmegaPlusK_split`` on two k-points to 8 tol, tol = 1e-8 (the reference's test_solve_OmegaPlusK rule).
* Scope and safety cases.  ``negative_curvature`` is covered on the host twin (tests/test_newton_host.py): a start far enough
  to make the device operator indefinite is found only by trying.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd.refine import proj_tangent, rayleigh_coefficients  # noqa: E402

import nlcc_gen  # noqa: E402
import refine_twin  # noqa: E402
from test_gpu_refine import twin_side  # noqa: E402

DEV = "cuda:0"
TOL = 1e-7
LDA = ("lda_x", "lda_c_pw")
KCOORDS = [[0, 0, 0], [1 / 3, 0, 0], [1 / 3, 1 / 3, 0], [-1 / 3, 1 / 3, 0]]
KWEIGHTS = [1 / 27, 8 / 27, 6 / 27, 12 / 27]
DISPLACED = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]
GAMMA = dict(kcoords=[[0, 0, 0]], kweights=[1.0])
TWO_K = dict(kcoords=[[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]], kweights=[0.5, 0.5])


def si_basis(functionals=LDA, kcoords=KCOORDS, kweights=KWEIGHTS, Ecut=3, fft_size=(9, 9, 9), positions=None, atoms=None,
             gamma_real=False, **kw):
    kw.setdefault("symmetries", positions is None)
    lat, hgh, pos = dftk.silicon_cell()
    model = dftk.model_DFT(lat, atoms or hgh, positions or pos, functionals=functionals, **kw)
    return dftk.PlaneWaveBasis(model, Ecut, dftk.ExplicitKpoints(kcoords, kweights), fft_size=fft_size, device=DEV,
                               gamma_real=gamma_real)


def gamma_basis(fft_size=None, **kw):
    kw.setdefault("positions", DISPLACED)
    return si_basis(**GAMMA, Ecut=5, fft_size=fft_size, **kw)


def scf(basis, tol, **kw):
    res = dftk.self_consistent_field(basis, tol=tol, **kw)
    assert res["converged"]
    return res


def occupied(basis, res):
    psi, occ = dftk.select_occupied_orbitals(basis, res["psi"], res["occupation"])
    return [p.contiguous() for p in psi], occ


def run_newton(basis, start_tol=1e-2, **kw):
    """Newton from the occupied orbitals of an SCF stopped at ``start_tol``"""
    psi0, _ = occupied(basis, dftk.self_consistent_field(basis, tol=start_tol))
    res = dftk.newton(basis, psi0, **kw)
    assert res["converged"], (res["n_iter"], res["history_drho"])
    return res


def drho_max(a, b):
    return float((a["rho"] - b["rho"]).abs().max().item())


def report(name, res, ref):
    d = drho_max(res, ref)
    print(f"\n{name}: {res['n_iter']} Newton steps, CG iterations {res['cg_iterations']}, history_drho "
          f"{[f'{x:.2e}' for x in res['history_drho']]}, max|rho_Newton - rho_SCF| = {d:.2e} (bound {10 * TOL:.0e}), "
          f"E_Newton - E_SCF = {res['energies'].total - ref['energies'].total:.2e}")
    return d


def randn_like(blocks, gen, scale=1.0):
    out = []
    for p in blocks:
        re, im = (torch.randn(p.shape, generator=gen, device=DEV, dtype=torch.float64) for _ in range(2))
        out.append(scale * torch.complex(re, im))
    return out


def wdot(basis, a, b):
    return float(sum(w * float((x.conj() * y).sum().real.item()) for w, x, y in zip(basis.kweights, a, b)))


def to_host(blocks):
    return [x.cpu().numpy().T for x in blocks]


def old_operator(basis, d, psi, ham, rho, occ):
    """the pre-existing composition: apply_Omega + apply_K of refine.py"""
    return [a + b for a, b in zip(dftk.apply_Omega(d, psi, ham, rayleigh_coefficients(ham, psi)),
                                  dftk.apply_K(basis, d, psi, rho, occ))]


# ------------------------------------------------------------------------------------------ Gamma: against the dense twin
@pytest.fixture(scope="module")
def gamma_case():
    """the displaced cell at Gamma: basis, SCF at 1e-10, its occupied orbitals, the tangent space with the cache on and off
    and the dense twin's side (dense H from ``mul_`` on the identity, f_xc from central differences)"""
    basis = gamma_basis()
    res = scf(basis, 1e-10)
    psi, occ = occupied(basis, res)
    ts_on = dftk.TangentSpace(basis, psi, occ, cache_realspace=True)
    ts_off = dftk.TangentSpace(basis, psi, occ, cache_realspace=False)
    assert ts_on.psi_r is not None and ts_off.psi_r is None and ts_on.cache_bytes == 4 * 16 * int(np.prod(basis.fft_size))
    side = twin_side(basis, ts_on.ham, ts_on.rho)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    rhs = randn_like(psi, gen, 1e-2)
    return dict(basis=basis, scfres=res, psi=psi, occ=occ, ts_on=ts_on, ts_off=ts_off, side=side, rhs=rhs, gen=gen)


def test_operator_with_and_without_the_cache_against_the_dense_twin(gamma_case):
    c = gamma_case
    basis, psi, occ = c["basis"], c["psi"], c["occ"]
    d = randn_like(psi, c["gen"])
    dh, ph = to_host(d), to_host(psi)
    want = [a + b for a, b in zip(refine_twin.apply_Omega_dense(c["side"], dh, ph), refine_twin.apply_K_dense(c["side"], dh, ph, occ))]
    scale = max(np.abs(x).max() for x in want)

    def err(blocks):
        return max(np.abs(a - b).max() for a, b in zip(to_host(blocks), want)) / scale
    e_old = err(old_operator(basis, d, psi, c["ts_on"].ham, c["ts_on"].rho, occ))
    e_on = err(dftk.apply_OmegaPlusK(c["ts_on"], d))
    e_off = err(dftk.apply_OmegaPlusK(c["ts_off"], d))
    print(f"\n(Omega + K) d against the dense twin: apply_Omega + apply_K {e_old:.3e}, cache on {e_on:.3e}, cache off {e_off:.3e} "
          f"(bound 4 x the first)")
    assert e_old > 0
    assert e_on <= 4 * e_old and e_off <= 4 * e_old
    # the result lies in the tangent space and the input is not modified
    out = dftk.apply_OmegaPlusK(c["ts_on"], d)
    assert float((psi[0].conj() @ out[0].T).abs().max()) < 1e-12


@pytest.fixture(scope="module")
def gamma_dense(gamma_case):
    """the twin's dense operator on a real basis of the tangent space (weights 1 at Gamma: symmetric), its smallest
    eigenvalue, and the exact answer to the right-hand side of ``gamma_case``"""
    c = gamma_case
    side, occ = c["side"], c["occ"]
    ph = to_host(c["psi"])
    p = ph[0]
    Q = np.linalg.svd(np.eye(p.shape[0]) - p @ p.conj().T)[0][:, :p.shape[0] - p.shape[1]]
    a, b = Q.shape[1], p.shape[1]
    D = 2 * a * b
    A = np.zeros((D, D))
    for j in range(D):
        e = np.zeros(D)
        e[j] = 1.0
        dj = [Q @ (e[:a * b] + 1j * e[a * b:]).reshape(a, b)]
        o = refine_twin.apply_Omega_dense(side, dj, ph)[0] + refine_twin.apply_K_dense(side, dj, ph, occ)[0]
        col = (Q.conj().T @ o).reshape(-1)
        A[:, j] = np.concatenate([col.real, col.imag])
    assert np.abs(A - A.T).max() < 1e-8 * np.abs(A).max()
    lam_min = float(np.linalg.eigvalsh((A + A.T) / 2)[0])
    assert lam_min > 0
    exact = refine_twin.solve_OmegaPlusK_dense(side, ph, to_host(c["rhs"]), occ)[0]
    return dict(lam_min=lam_min, exact=exact)


def test_residual_and_error_against_the_dense_solve(gamma_case, gamma_dense):
    c = gamma_case
    basis, psi, occ, rhs = c["basis"], c["psi"], c["occ"], c["rhs"]
    lam_min, exact = gamma_dense["lam_min"], gamma_dense["exact"]
    Prhs = proj_tangent(basis, rhs, psi)
    for tol in (1e-6, 1e-8, 1e-10):
        sol = dftk.solve_OmegaPlusK_cg(basis, psi, rhs, occ, tol=tol, tangent_space=c["ts_on"])
        assert sol["converged"] and not sol["negative_curvature"] and sol["tol"] == tol
        assert sol["residual_norms"][0] <= tol and sol["n_iter"] == len(sol["residual_history"])
        res = [x + y for x, y in zip(old_operator(basis, sol["dpsi"], psi, c["ts_on"].ham, c["ts_on"].rho, occ), Prhs)]
        rnorm = wdot(basis, res, res) ** 0.5
        diff = to_host(sol["dpsi"])[0] - exact
        enorm = float(np.linalg.norm(diff))
        print(f"\nsolve_OmegaPlusK_cg tol {tol:.0e}: {sol['n_iter']} iterations, own residual {sol['residual_norms'][0]:.2e}, "
              f"residual rebuilt with apply_Omega + apply_K {rnorm:.2e} (bound {2 * tol:.0e}), |dpsi - dense| {enorm:.2e} "
              f"(bound 2 tol / lambda_min = {2 * tol / lam_min:.2e}, lambda_min {lam_min:.3e})")
        assert rnorm <= 2 * tol
        assert enorm <= 2 * tol / lam_min
        assert float((psi[0].conj() @ sol["dpsi"][0].T).abs().max()) < 1e-12       # on the tangent space


def test_cache_off_solves_the_same_system(gamma_case, gamma_dense):
    """both paths stop at a residual norm <= tol, so the answers differ by at most 2 tol / lambda_min"""
    c = gamma_case
    on = dftk.solve_OmegaPlusK_cg(c["basis"], c["psi"], c["rhs"], c["occ"], tol=1e-10, cache_realspace=True)
    off = dftk.solve_OmegaPlusK_cg(c["basis"], c["psi"], c["rhs"], c["occ"], tol=1e-10, cache_realspace=False)
    d = float(torch.linalg.norm(on["dpsi"][0] - off["dpsi"][0]).item())
    bound = 2 * 1e-10 / gamma_dense["lam_min"]
    print(f"\ncache on against off: {on['n_iter']} / {off['n_iter']} iterations, |dpsi_on - dpsi_off| = {d:.2e} (bound {bound:.2e})")
    assert on["converged"] and off["converged"] and on["n_apply"] == on["n_iter"] - 1
    assert d <= bound


# ------------------------------------------------------------------------------------------ the reference's tests
@pytest.fixture(scope="module")
def si_kpts():
    basis = si_basis()
    return basis, scf(basis, TOL / 10)


@pytest.fixture(scope="module")
def si_kpts_newton(si_kpts):
    basis = si_kpts[0]
    start = dftk.self_consistent_field(basis, maxiter=1)
    psi0, _ = occupied(basis, start)                       # remove virtual orbitals
    return dftk.newton(basis, psi0, tol=TOL)


def test_newton_from_one_scf_step_reaches_the_scf_density(si_kpts, si_kpts_newton):
    basis, ref = si_kpts
    res = si_kpts_newton
    assert res["converged"] and res["n_iter"] <= 20
    assert report("silicon LDA, 4 k-points", res, ref) < 10 * TOL
    assert abs(res["energies"].total - ref["energies"].total) < 10 * TOL
    # the result reads like an scfres
    assert res["algorithm"] == "Newton" and res["eF"] is None and res["n_bands_converge"] == 4 and res["basis"] is basis
    assert len(res["history_Etot"]) == len(res["history_drho"]) == len(res["cg_iterations"]) == res["n_iter"]
    assert len(res["cg_residual_norms"]) == res["n_iter"] and all(r <= TOL / 100 for r in res["cg_residual_norms"])
    assert res["history_drho"][-1] < TOL and all(d >= TOL for d in res["history_drho"][:-1])
    for p, lam, occ, kpt in zip(res["psi"], res["eigenvalues"], res["occupation"], basis.kpoints):
        assert p.shape == (4, kpt.n_G) and np.all(np.diff(lam) >= 0) and np.array_equal(occ, [2.0] * 4)
        gram = (p.conj() @ p.T).cpu().numpy()
        assert np.abs(gram - np.eye(4)).max() < 1e-12
    for lam, lam_ref in zip(res["eigenvalues"], ref["eigenvalues"]):
        assert np.abs(lam - np.asarray(lam_ref)[:4]).max() < 1e-5


def test_self_adjointness_of_the_solve(si_kpts):
    """test/hessian.jl:102-113: <phi, solve(rhs)>_w = <solve(phi), rhs>_w to atol 1e-7, with rhs the projected gradient at
    the orbitals of an unconverged SCF and phi random orthonormal orbitals"""
    basis = si_kpts[0]
    psi, occ = occupied(basis, dftk.self_consistent_field(basis, tol=1e-2))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(17)
    rhs = dftk.compute_projected_gradient(basis, psi, occ)
    phi = [dftk.random_orbitals(basis, kpt, 4, gen) for kpt in basis.kpoints]
    ts = dftk.TangentSpace(basis, psi, occ)
    a = wdot(basis, phi, dftk.solve_OmegaPlusK_cg(basis, psi, rhs, occ, tangent_space=ts)["dpsi"])
    b = wdot(basis, dftk.solve_OmegaPlusK_cg(basis, psi, phi, occ, tangent_space=ts)["dpsi"], rhs)
    print(f"\nself-adjointness: {a:.12e} against {b:.12e}, difference {abs(a - b):.2e} (atol 1e-7)")
    assert abs(a - b) <= 1e-7


def test_consistency_with_the_split_solver_on_two_kpoints():
    tol = 1e-8
    basis = si_basis(**TWO_K, Ecut=5, fft_size=None, positions=DISPLACED)
    res = scf(basis, 1e-10)
    psi, occ = occupied(basis, res)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    rhs = randn_like(psi, gen, 1e-2)
    dH = []
    for p_all, r in zip(res["psi"], rhs):
        full = torch.zeros_like(p_all)
        full[:r.shape[0]] = r
        dH.append(full)
    split = dftk.solve_OmegaPlusK_split(res, dH, tol=tol)
    sol = dftk.solve_OmegaPlusK_cg(basis, psi, rhs, occ, tol=tol)
    assert split["converged"] and sol["converged"]
    errs = [float((a - b[:a.shape[0]]).abs().max()) for a, b in zip(sol["dpsi"], split["dpsi"])]
    print(f"\nCG against the split solver: max|dpsi_cg - dpsi_split| per k-point {errs} (bound {8 * tol:.0e}), "
          f"{sol['n_iter']} CG iterations")
    assert max(errs) < 8 * tol


# ------------------------------------------------------------------------------------------ scope
@pytest.fixture(scope="module")
def gamma_runs(gamma_case):
    """at Gamma with the switch off: the SCF at tol and tol / 10 and the Newton run (cache on)"""
    basis = gamma_case["basis"]
    return basis, scf(basis, TOL), scf(basis, TOL / 10), run_newton(basis, tol=TOL, cache_realspace=True)


def test_gamma_real_switch_on_against_off(gamma_runs):
    basis_off, loose, tight, off = gamma_runs
    basis_on = gamma_basis(fft_size=basis_off.fft_size, gamma_real=True)
    assert basis_on.kpoints[0].gamma_real and not basis_off.kpoints[0].gamma_real
    on = run_newton(basis_on, tol=TOL)
    assert report("Gamma-real switch on, against the SCF with it off", on, tight) < 10 * TOL
    assert report("Gamma-real switch off", off, tight) < 10 * TOL
    scf_own = abs(loose["energies"].total - tight["energies"].total)
    diff = abs(on["energies"].total - off["energies"].total)
    print(f"\nE_Newton(on) - E_Newton(off) = {diff:.2e}; the SCF's own E(tol) - E(tol / 10) = {scf_own:.2e}")
    assert diff <= 10 * max(scf_own, 1e-14)
    assert all(p.shape == (4, k.n_G) and p.dtype == torch.complex128 for p, k in zip(on["psi"], basis_on.kpoints))


def test_cache_on_against_off(gamma_runs):
    basis, _, tight, on = gamma_runs
    off = run_newton(basis, tol=TOL, cache_realspace=False)
    d = drho_max(on, off)
    print(f"\nNewton with the cache on against off: max|rho_on - rho_off| = {d:.2e} (bound {10 * TOL:.0e}), CG iterations "
          f"{on['cg_iterations']} / {off['cg_iterations']}")
    assert d < 10 * TOL and report("cache off", off, tight) < 10 * TOL


def test_upf_with_core_correction():
    psp = nlcc_gen.core_psp("Si", "lda", core=True)
    basis = gamma_basis(functionals=("lda_x", "lda_c_vwn"), atoms=[dftk.ElementPsp("Si", psp=psp)] * 2)
    assert basis.terms.rho_core is not None
    assert report("silicon UPF + NLCC at Gamma", run_newton(basis, tol=TOL), scf(basis, TOL / 10)) < 10 * TOL


def test_irreducible_mesh_against_the_full_mesh():
    lat, atoms, pos = dftk.silicon_cell()
    model = dftk.model_DFT(lat, atoms, pos, functionals=LDA, symmetries=True)
    out = []
    for reduce_k in (True, False):
        basis = dftk.PlaneWaveBasis(model, 5, dftk.MonkhorstPack((2, 2, 2)), device=DEV,
                                    use_symmetries_for_kpoint_reduction=reduce_k)
        out.append((len(basis.kpoints), run_newton(basis, tol=TOL)))
    (n_irr, a), (n_full, b) = out
    assert n_irr < n_full == 8
    d = drho_max(a, b)
    print(f"\nirreducible ({n_irr} k-points, CG {a['cg_iterations']}) against the full mesh (CG {b['cg_iterations']}): "
          f"max|rho_irr - rho_full| = {d:.2e} (bound {10 * TOL:.0e}), dE = {a['energies'].total - b['energies'].total:.2e}")
    assert d < 10 * TOL and abs(a["energies"].total - b["energies"].total) < 10 * TOL


def test_forces_of_the_result(gamma_runs):
    _, loose, tight, res = gamma_runs
    f_loose, f_tight = dftk.compute_forces_cart(loose), dftk.compute_forces_cart(tight)
    bound = 10 * float(np.abs(f_loose - f_tight).max())
    f = dftk.compute_forces_cart(res)
    err = float(np.abs(f - f_tight).max())
    print(f"\nforces: max|F_Newton - F_SCF| = {err:.2e}, bound 10 |F_SCF(tol) - F_SCF(tol / 10)| = {bound:.2e}, "
          f"max|F| = {np.abs(f_tight).max():.2e}")
    assert np.abs(f_tight).max() > 1e-3
    assert err <= bound


def test_callback_and_custom_criterion(gamma_case):
    basis = gamma_case["basis"]
    psi0, _ = occupied(basis, dftk.self_consistent_field(basis, tol=1e-2))
    seen = []
    res = dftk.newton(basis, psi0, is_converged=lambda info: info["n_iter"] >= 2, callback=seen.append)
    assert res["converged"] and res["n_iter"] == 2
    assert [i["n_iter"] for i in seen[:-1]] == [1, 2] and seen[-1]["stage"] == "finalize"
    assert all(i["algorithm"] == "Newton" and i["rho"].shape == i["rho_in"].shape for i in seen[:-1])
    stop = dftk.newton(basis, psi0, tol=1e-14, maxiter=1)
    assert not stop["converged"] and stop["n_iter"] == 1
    cg_seen = []
    sol = dftk.solve_OmegaPlusK_cg(basis, gamma_case["psi"], gamma_case["rhs"], gamma_case["occ"], tol=1e-6,
                                   callback=cg_seen.append, tangent_space=gamma_case["ts_on"])
    assert [i["n_iter"] for i in cg_seen[:-1]] == list(range(sol["n_iter"])) and cg_seen[-1]["stage"] == "finalize"
    few = dftk.solve_OmegaPlusK_cg(basis, gamma_case["psi"], gamma_case["rhs"], gamma_case["occ"], tol=1e-14, maxiter=2,
                                   tangent_space=gamma_case["ts_on"])
    assert not few["converged"] and few["n_iter"] == 2 and not few["negative_curvature"]


# ------------------------------------------------------------------------------------------ safety
def test_a_run_leaves_the_scf_state_and_an_earlier_result_alone(gamma_runs):
    basis, _, tight, _ = gamma_runs
    rho0, psi0 = tight["rho"].clone(), [p.clone() for p in tight["psi"]]
    e0 = tight["energies"].total
    before = dftk.energy_hamiltonian(basis, tight["psi"], tight["occupation"], rho=tight["rho"])[0]
    kw0, ham_pot = list(basis.kweights), tight["ham"][0].potential.clone()
    start, _ = occupied(basis, dftk.self_consistent_field(basis, tol=1e-2))
    start0 = [p.clone() for p in start]
    a = dftk.newton(basis, start, tol=TOL, maxiter=2)
    b = dftk.newton(basis, start, tol=TOL, maxiter=2)
    assert a["history_Etot"] == b["history_Etot"] and a["history_drho"] == b["history_drho"]        # bitwise
    assert a["cg_iterations"] == b["cg_iterations"]
    assert all(torch.equal(p, q) for p, q in zip(start, start0))                                    # psi0 is not modified
    assert torch.equal(tight["rho"], rho0) and all(torch.equal(p, q) for p, q in zip(tight["psi"], psi0))
    assert tight["energies"].total == e0 and list(basis.kweights) == kw0
    assert torch.equal(tight["ham"][0].potential, ham_pot)
    after = dftk.energy_hamiltonian(basis, tight["psi"], tight["occupation"], rho=tight["rho"])[0]
    assert dict(after) == dict(before)
    # an SCF continued after a Newton run goes on as without one
    energies = []
    for with_newton in (False, True):
        stepper = dftk.ScfStepper(gamma_basis(fft_size=basis.fft_size), tol=1e-12)
        for _ in range(6):
            info = stepper.step()
        if with_newton:
            sb = info["ham"][0].basis
            p, _ = dftk.select_occupied_orbitals(sb, info["psi"], info["occupation"])
            assert dftk.newton(sb, [x.contiguous() for x in p], tol=1e-6)["converged"]
        energies.append([stepper.step()["energies"].total for _ in range(2)])
    assert np.abs(np.array(energies[0]) - np.array(energies[1])).max() < 1e-13


def test_refusals_on_a_device_basis(gamma_case):
    basis, psi, occ = gamma_case["basis"], gamma_case["psi"], gamma_case["occ"]
    n_G = basis.kpoints[0].n_G
    for shape in ((3, n_G), (7, n_G), (4, n_G - 1)):
        with pytest.raises(ValueError, match="select_occupied_orbitals"):
            dftk.newton(basis, [torch.zeros(shape, dtype=torch.complex128, device="cuda")])
    with pytest.raises(ValueError, match="blocks"):
        dftk.newton(basis, [])
    with pytest.raises(ValueError, match="psi0"):
        dftk.newton(basis, None)
    hot = gamma_basis(fft_size=basis.fft_size, temperature=0.01)
    with pytest.raises(ValueError, match="temperature"):
        dftk.newton(hot, psi)
    pbe = gamma_basis(functionals=("gga_x_pbe", "gga_c_pbe"), fft_size=basis.fft_size)
    for call in (lambda: dftk.newton(pbe, psi), lambda: dftk.solve_OmegaPlusK_cg(pbe, psi, psi, occ),
                 lambda: dftk.TangentSpace(pbe, psi, occ)):
        with pytest.raises(NotImplementedError, match="GGA"):
            call()
    spin = gamma_basis(fft_size=basis.fft_size, magnetic_moments=[1.0, 1.0])
    with pytest.raises(NotImplementedError, match="collinear spin"):
        dftk.newton(spin, psi + psi)
    with pytest.raises(ValueError, match="full occupation"):
        dftk.solve_OmegaPlusK_cg(basis, psi, psi, [np.array([2.0, 2.0, 2.0, 1.0])])
    with pytest.raises(ValueError, match="shape of psi"):
        dftk.solve_OmegaPlusK_cg(basis, psi, [psi[0][:3].contiguous()], occ)
    with pytest.raises(TypeError, match="CUDA"):
        dftk.solve_OmegaPlusK_cg(basis, psi, [psi[0].cpu()], occ)
    with pytest.raises(NotImplementedError, match="solve_OmegaPlusK_split"):
        dftk.solve_OmegaPlusK()
