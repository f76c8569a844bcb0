"""Host-only checks of the potential-mixing SCF (dftk_jl_amd/potential_mixing.py; no device):

* ``ensure_damping_within_range``: the 18 cases of the reference's test/adaptive_damping.jl, exact equality;
* the constructors of ``AdaptiveDamping``;
* ``propose_backtrack_damping`` / ``trial_damping`` branch by branch on hand-made infos, ``ScfAcceptImprovingStep`` on both
  of its conditions;
* ``_potential_mixing_loop`` on a toy problem whose energy is exactly quadratic along every search direction, so that the
  quadratic model is exact and the backtracked damping is the analytic line minimiser;
* every refusal of ``scf_potential_mixing`` on descriptor-only bases (``device="cpu"``), raised before any device work.
"""
import math

import numpy as np
import pytest

import dftk_jl_amd as dftk
from dftk_jl_amd import KptComm
from dftk_jl_amd import potential_mixing as pm

torch = pytest.importorskip("torch")


class E:
    def __init__(self, total):
        self.total = total


def reference_damping():
    return dftk.AdaptiveDamping(alpha_min=0.05, alpha_max=1.0, alpha_trial_init=0.8, alpha_trial_min=0.2,
                                alpha_trial_enhancement=1.1, modeltol=0.1)


# ------------------------------------------------------------------------------------------ damping range, constructors
@pytest.mark.parametrize("alpha, alpha_next, expected", [
    (0.2, 0.1, 0.1), (-0.2, 0.1, 0.1),                                      # if within range we accept
    (1.5, 1.5, 1.0), (-1.5, 1.5, 1.0),                                      # if above maximum, then limit
    (0.2, 0.2, 0.19), (0.2, 0.5, 0.19), (-0.2, 0.2, 0.19), (-0.2, 0.5, 0.19),   # ensure shrinkage
    (0.2, 0.01, 0.05), (-0.2, 0.01, 0.05),                                  # ... but not below alpha_min
    (-0.2, -0.07, -0.07), (0.2, -0.07, -0.07), (-0.2, -0.2, -0.1), (0.2, -0.2, -0.1), (-0.2, -0.5, -0.1),
    (0.2, -0.5, -0.1),                                                      # ensure sign is kept
    (-0.2, -1e-3, 0.05), (0.2, -1e-3, 0.05),                                # ... unless too small
])
def test_ensure_damping_within_range(alpha, alpha_next, expected):
    assert dftk.ensure_damping_within_range(reference_damping(), alpha, alpha_next) == expected


def test_constructors():
    d = dftk.AdaptiveDamping()
    assert (d.alpha_min, d.alpha_max, d.alpha_trial_init, d.alpha_trial_min, d.alpha_trial_enhancement, d.modeltol) == \
        (0.05, 1.0, 0.8, 0.2, 1.1, 0.1)
    d = dftk.AdaptiveDamping(1.5)
    assert (d.alpha_min, d.alpha_max, d.alpha_trial_init, d.alpha_trial_min) == (0.375, 1.875, 1.5, 1.5)
    d = dftk.AdaptiveDamping(0.4, modeltol=0.3)
    assert (d.alpha_min, d.alpha_max, d.alpha_trial_init, d.alpha_trial_min, d.modeltol) == (0.1, 1.0, 0.8, 0.4, 0.3)
    with pytest.raises(TypeError):
        dftk.AdaptiveDamping(0.4, 0.5)
    assert dftk.FixedDamping().alpha == 0.8 and dftk.FixedDamping(0.3).alpha == 0.3
    assert dftk.trial_damping(dftk.FixedDamping(0.3)) == 0.3
    assert dftk.propose_backtrack_damping(dftk.FixedDamping(0.3)) == 0.3
    assert dftk.trial_damping(dftk.AdaptiveDamping(1.5)) == 1.5
    assert dftk.ScfAcceptStepAll()(None, None) is True


# ------------------------------------------------------------------------------------------ hand-made infos
def infos(alpha0, slope, curv, E0=-1.0, error=0.0, n_trials=1):
    """Two infos whose scalar block gives the model phi(alpha) = E0 + slope alpha + curv alpha^2 / 2 (dvol = 1) and whose
    observed energy at alpha0 is off the model by ``error`` times the observed energy change."""
    E_model = E0 + slope * alpha0 + curv * alpha0 ** 2 / 2
    E_next = E0 + (E_model - E0) / (1 - error) if error else E_model
    sums = dict(dot_out=slope * alpha0, dot_step=0.0, dot_kernel=curv * alpha0 ** 2)
    return (dict(energies=E(E0), dvol=1.0),
            dict(energies=E(E_next), alpha=alpha0, sums=sums, diagonalization=[{}] * n_trials))


def test_quadratic_model():
    info, nxt = infos(0.8, -1.0, 4.0)
    alpha, relerror = dftk.scf_damping_quadratic_model(info, nxt)
    assert alpha == 0.25 and relerror < 1e-14
    # trusted (error < modeltol) needs a negative slope, tight (error < modeltol / 5) does not
    info, nxt = infos(0.8, -1.0, 4.0, error=0.05)
    alpha, relerror = dftk.scf_damping_quadratic_model(info, nxt)
    assert alpha == 0.25 and abs(relerror - 0.05) < 1e-12
    info, nxt = infos(0.8, +1.0, 4.0, error=0.05)
    assert dftk.scf_damping_quadratic_model(info, nxt)[0] is None
    info, nxt = infos(0.8, +1.0, 4.0, error=0.01)
    assert dftk.scf_damping_quadratic_model(info, nxt)[0] == -0.25
    # no minimum along the direction, or a model that misses the observation
    info, nxt = infos(0.8, -1.0, -4.0)
    assert dftk.scf_damping_quadratic_model(info, nxt)[0] is None
    info, nxt = infos(0.8, -1.0, 4.0, error=0.2)
    alpha, relerror = dftk.scf_damping_quadratic_model(info, nxt)
    assert alpha is None and abs(relerror - 0.2) < 1e-12
    assert dftk.scf_damping_quadratic_model(info, nxt, modeltol=0.3)[0] == 0.25


def test_propose_backtrack_damping_branches():
    damping = reference_damping()
    # give up below 1.75 alpha_min: alpha is returned as it is
    info, nxt = infos(0.08, -1.0, 4.0)
    assert dftk.propose_backtrack_damping(damping, info, nxt) == 0.08
    # model accepted: its minimiser, inside the range
    info, nxt = infos(0.8, -1.0, 4.0)
    assert dftk.propose_backtrack_damping(damping, info, nxt) == 0.25
    # model rejected with a small error: half; with relerror >= 10: a quarter
    info, nxt = infos(0.8, -1.0, 4.0, error=0.5)
    assert dftk.propose_backtrack_damping(damping, info, nxt) == 0.4
    info, nxt = infos(0.8, -1.0, 4.0, error=20.0)
    assert dftk.propose_backtrack_damping(damping, info, nxt) == 0.2
    # clamp: a minimiser beyond 0.95 alpha shrinks to it, one below alpha_min rises to it, a negative one keeps its sign
    info, nxt = infos(0.8, -4.0, 4.0)
    assert dftk.propose_backtrack_damping(damping, info, nxt) == 0.95 * 0.8
    info, nxt = infos(0.8, -0.08, 4.0)
    assert dftk.propose_backtrack_damping(damping, info, nxt) == 0.05
    info, nxt = infos(0.8, +1.0, 4.0, error=0.01)
    assert dftk.propose_backtrack_damping(damping, info, nxt) == -0.25


def test_trial_damping_branches():
    damping = reference_damping()
    assert dftk.trial_damping(damping) == 0.8
    # a step that was good at once: enhancement 1.1 on the model's minimiser when that is larger than alpha
    info, nxt = infos(0.3, -2.0, 4.0)
    assert dftk.trial_damping(damping, info, nxt, True) == pytest.approx(1.1 * 0.5, rel=1e-15)
    info, nxt = infos(0.8, -1.0, 4.0)                                   # ... else alpha stays
    assert dftk.trial_damping(damping, info, nxt, True) == 0.8
    info, nxt = infos(0.3, -2.0, 4.0, error=0.5)                        # ... model not meaningful: alpha stays
    assert dftk.trial_damping(damping, info, nxt, True) == 0.3
    info, nxt = infos(1.0, -2.0, 4.0)
    del nxt["sums"]                                                     # at alpha_max the model is not even computed
    assert dftk.trial_damping(damping, info, nxt, True) == 1.0
    # backtracked or unsuccessful steps: the alpha that was used, clamped into [alpha_trial_min, alpha_max]
    info, nxt = infos(0.3, -2.0, 4.0, n_trials=2)
    assert dftk.trial_damping(damping, info, nxt, True) == 0.3
    info, nxt = infos(0.3, -2.0, 4.0)
    assert dftk.trial_damping(damping, info, nxt, False) == 0.3
    info, nxt = infos(-0.07, -2.0, 4.0, n_trials=3)
    assert dftk.trial_damping(damping, info, nxt, True) == 0.2
    info, nxt = infos(0.5, -40.0, 4.0)                                  # enhancement clamped at alpha_max
    assert dftk.trial_damping(damping, info, nxt, True) == 1.0


def test_accept_improving_step():
    def pair(dE, r0, r1):
        return (dict(energies=E(-1.0), Pinv_dV=torch.full((4,), r0, dtype=torch.float64)),
                dict(energies=E(-1.0 + dE), Pinv_dV=torch.full((4,), r1, dtype=torch.float64)))
    accept = dftk.ScfAcceptImprovingStep()
    assert accept(*pair(-1e-3, 1.0, 2.0))              # energy falls, residual rises
    assert accept(*pair(+1e-3, 1.0, 0.5))              # energy rises, residual falls
    assert not accept(*pair(+1e-3, 1.0, 2.0))          # both rise
    assert not accept(*pair(+1e-3, 1.0, 1.0))          # (strict: an equal residual does not count)
    assert dftk.ScfAcceptImprovingStep(max_energy_change=1e-2)(*pair(+1e-3, 1.0, 2.0))
    assert dftk.ScfAcceptImprovingStep(max_relative_residual=3.0)(*pair(+1e-3, 1.0, 2.0))
    # the norms come from the scalar block where the loop has left it
    a, b = pair(+1e-3, 1.0, 2.0)
    a["sums"], b["sums"] = dict(pinv_norm2=4.0), dict(pinv_norm2=1.0)
    assert accept(a, b)


# ------------------------------------------------------------------------------------------ the loop on a toy problem
class Toy:
    """rho(V) = rho0 + chi0 V with chi0 = -diag(d), d > 0; V_out(rho) = V_ext + K rho with K = diag(k);
    E = -1/2 (rho - rho0)' chi0^-1 (rho - rho0) + V_ext . rho + 1/2 rho' K rho.  Along any direction dV the energy is a
    quadratic in alpha whose slope is <V_out - V_in, drho> / alpha0 and whose curvature is
    (-<V_next - V_in, drho> + <drho, K drho>) / alpha0^2 exactly: dE/dV = -d (V_out - V), d2E/dV2 = d (1 + k d).
    k d in [1.5, 2.5]: the plain step alpha = 1.5 multiplies every error component by 1 - 1.5 (1 + k d) in [-4.25, -2.75]
    -- it overshoots and the energy rises -- while the line minimiser lies near 1 / 3."""

    def __init__(self, n=64, seed=3):
        rng = np.random.default_rng(seed)
        t = lambda x: torch.from_numpy(x)                          # noqa: E731
        self.d = t(rng.uniform(0.5, 2.0, n))
        self.k = t(rng.uniform(1.5, 2.5, n)) / self.d
        self.rho0 = t(rng.uniform(0.5, 1.5, n))
        self.Vext = t(rng.standard_normal(n))
        self.V_fix = (self.Vext + self.k * self.rho0) / (1 + self.k * self.d)
        self.calls = []

    def energy(self, rho):
        return float((0.5 * (rho - self.rho0) ** 2 / self.d + self.Vext * rho + 0.5 * self.k * rho ** 2).sum())

    def EVrho(self, Vin, diagtol=None, psi=None, eigenvalues=None, occupation=None):
        rho = self.rho0 - self.d * Vin
        self.calls.append(psi)
        return dict(Vin=Vin, Vout=self.Vext + self.k * rho, rho=rho, psi=("psi", len(self.calls)), eigenvalues=None,
                    occupation=None, energies=E(self.energy(rho)), diagonalization={})


def run_toy(damping, accept_step, tol=1e-11, maxiter=60):
    toy = Toy()
    V0 = torch.zeros(64, dtype=torch.float64)
    trials = []

    def model_sums(info, info_next):
        if info is not None:
            trials.append((info, info_next))
        return pm._torch_sums(info, info_next, "secant")
    info, converged, stats = pm._potential_mixing_loop(
        toy.EVrho, lambda dV, info, rho_in, n_iter: dV, lambda x, alpha, Pf: x + alpha * Pf, model_sums, V0,
        torch.zeros_like(V0), damping, accept_step, 1.0, tol=tol, maxiter=maxiter)
    return toy, info, converged, stats, trials


def test_toy_line_search():
    damping = dftk.AdaptiveDamping(alpha_min=0.05, alpha_max=1.5, alpha_trial_init=1.5, alpha_trial_min=0.2)
    accept = dftk.ScfAcceptImprovingStep()
    toy, info, converged, stats, trials = run_toy(damping, accept)
    # the first trial, alpha = 1.5, is rejected: the energy rises and so does the residual
    first, second = trials[0], trials[1]
    assert first[1]["alpha"] == 1.5 and not accept(*first)
    assert first[1]["energies"].total > first[0]["energies"].total
    # the model is exact on this problem ...
    alpha_model, relerror = dftk.scf_damping_quadratic_model(*first, modeltol=damping.modeltol)
    assert relerror < 1e-10
    # ... and the second trial sits at the exact line minimiser -slope / curv, clamped as prescribed
    info0 = first[0]
    dV = info0["Vout"] - info0["Vin"]
    slope = -float((toy.d * dV * dV).sum())
    curv = float((toy.d * (1 + toy.k * toy.d) * dV * dV).sum())
    assert abs(alpha_model - (-slope / curv)) < 1e-13
    expected = dftk.ensure_damping_within_range(damping, 1.5, alpha_model)
    assert second[0] is info0 and second[1]["alpha"] == expected and 0.25 < expected < 0.45
    assert accept(*second)
    assert stats["n_backtracks"][0] == 2 and stats["alphas"][0] == expected
    # the guess of the second trial: alpha_next <= alpha / 2, so the OLDER orbitals (those of info) are handed over
    assert toy.calls[2] == info0["psi"]
    # convergence to the analytic fixed point
    assert converged and float((info["Vin"] - toy.V_fix).abs().max()) < 1e-9
    assert len(stats["alphas"]) == len(stats["n_backtracks"]) == len(stats["model_relerrors"]) == stats["n_iter"] - 1
    assert stats["history_drho"][-1] < 1e-11
    # accepted energies never rise under ScfAcceptImprovingStep unless the residual fell
    for (a, b) in trials:
        if b["alpha"] in stats["alphas"] and b["energies"].total - a["energies"].total >= 1e-12:
            assert b["sums"]["pinv_norm2"] < a["sums"]["pinv_norm2"]


def test_toy_fixed_damping_and_max_backtracks():
    # fixed damping proposes the same alpha again: one trial per iteration whatever accept_step says; at 0.3 it converges
    toy, info, converged, stats, _ = run_toy(dftk.FixedDamping(0.3), dftk.ScfAcceptImprovingStep())
    assert converged and set(stats["n_backtracks"]) == {1} and set(stats["alphas"]) == {0.3}
    assert float((info["Vin"] - toy.V_fix).abs().max()) < 1e-9
    # an accept_step that never accepts: max_backtracks trials, the last one is committed
    damping = dftk.AdaptiveDamping(alpha_min=0.05, alpha_max=1.5, alpha_trial_init=1.5, alpha_trial_min=0.2)
    toy, info, converged, stats, _ = run_toy(damping, lambda a, b: False, maxiter=3)
    assert stats["n_backtracks"] == [3, 3] and not converged


# ------------------------------------------------------------------------------------------ refusals, descriptors only
def cpu_basis(Ecut=5, functionals=("lda_x", "lda_c_pw"), kgrid=None, atoms=None, positions=None, **kw):
    lat, hgh, pos = dftk.silicon_cell()
    basis_kw = {k: kw.pop(k) for k in list(kw) if k in ("comm_pw", "comm_kpts")}
    model = dftk.model_DFT(lat, atoms or hgh, positions or pos, functionals=functionals, **kw)
    return dftk.PlaneWaveBasis(model, Ecut, kgrid or dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu", build_terms=False,
                               **basis_kw)


def test_refusals_on_descriptors():
    import hubbard_gen
    Si = dftk.ElementPsp("Si", psp=hubbard_gen.hubbard_psp())
    hf = dftk.PlaneWaveBasis(dftk.model_HF(*dftk.silicon_cell()), 5, dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu",
                             build_terms=False)
    cases = [
        (cpu_basis(functionals=("mgga_x_scan", "mgga_c_scan")), "meta-GGA"),
        (hf, "exact exchange"),
        (cpu_basis(atoms=[Si, Si], extra_terms=[dftk.Hubbard((dftk.OrbitalManifold("Si", "3P"), 0.1))]), "Hubbard"),
        (cpu_basis(comm_pw=KptComm(0, 2)), "comm_pw"),
        (cpu_basis(kgrid=dftk.MonkhorstPack((2, 1, 1)), comm_kpts=KptComm(0, 2)), "comm_kpts"),
    ]
    for basis, word in cases:
        for solver in (dftk.scf_potential_mixing, dftk.scf_potential_mixing_adaptive):
            with pytest.raises(NotImplementedError, match=word):
                solver(basis)
    base = cpu_basis()
    for mixing in (dftk.LdosMixing(), dftk.DielectricMixing(), dftk.HybridMixing()):
        with pytest.raises(NotImplementedError, match="SimpleMixing, KerkerMixing or KerkerDosMixing"):
            dftk.scf_potential_mixing(base, mixing=mixing)
    # the reference's curvature on models apply_kernel refuses: its refusal, before any device work
    for basis, word in ((cpu_basis(functionals=("gga_x_pbe", "gga_c_pbe")), "GGA"),
                        (cpu_basis(magnetic_moments=[1.0, 1.0]), "collinear spin"),
                        (cpu_basis(functionals=("lda_xc_teter93",)), "lda_xc_teter93")):
        with pytest.raises(NotImplementedError, match=word):
            dftk.scf_potential_mixing_adaptive(basis, curvature="kernel")
        assert pm.check_supported(basis) == "secant" and pm.check_supported(basis, curvature="secant") == "secant"
    assert pm.check_supported(base) == "kernel" and pm.check_supported(base, curvature="secant") == "secant"
    with pytest.raises(ValueError, match="curvature"):
        dftk.scf_potential_mixing(base, curvature="exact")
    with pytest.raises(ValueError, match="psi has 2 blocks"):
        dftk.scf_potential_mixing(base, psi=[None, None])
    nx, ny, nz = base.fft_size
    with pytest.raises(ValueError, match="V must have the shape"):
        dftk.scf_potential_mixing(base, V=torch.zeros((nz, ny, nx + 1), dtype=torch.float64))
    with pytest.raises(ValueError, match="V must have the shape"):
        dftk.scf_potential_mixing(cpu_basis(magnetic_moments=[1.0, 1.0]), V=torch.zeros((nz, ny, nx), dtype=torch.float64))
    with pytest.raises(ValueError, match="max_backtracks"):
        dftk.scf_potential_mixing(base, max_backtracks=0)
    with pytest.raises(TypeError, match="AdaptiveDamping"):
        dftk.scf_potential_mixing_adaptive(base, damping=dftk.FixedDamping(0.5))
    # in scope, but descriptor-only: refused at the first device call, after every check
    for call in (lambda: dftk.scf_potential_mixing(base, damping=0.5),
                 lambda: dftk.scf_potential_mixing_adaptive(cpu_basis(functionals=("gga_x_pbe", "gga_c_pbe")))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
