"""Direct minimisation of the energy over the occupied orbitals (host mirror of src/scf/direct_minimization.jl).

The reference hands the problem to Optim.jl: L-BFGS on a product of Stiefel manifolds (one per k-block), preconditioned by
Teter-Payne-Allan divided by the k-weight, ``InitialStatic()`` + ``BackTracking()`` as line search, no vector transport.
Here that algorithm is written out.  The optimiser's state lives on the device behind ``dftk_mi_lbfgs_*`` (csrc/dm_kernels.hip:
the history of (s, y) pairs and a two-loop recursion whose coefficients never reach the host), the tangent projection is
``dftk_mi_stiefel_project_tangent``, the retraction is the polar one (``dftk_mi_lowdin_ortho`` of psi + alpha d).  Pairs with
<s, y> <= 0 are dropped (Optim drops only the infinite case), so the trajectory need not equal Optim's; the minimiser does.

Orbital blocks are band-major ``(n_bands, n_G)`` complex128 CUDA tensors in the full-sphere layout (a basis with the
Gamma-real switch on included: the half format stays inside LOBPCG).  Scope: zero temperature, full occupations, LDA and
PBE, spin none and collinear, one rank; everything else is refused on descriptors before any device work.
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np
import torch

from . import _lib
from .densities import compute_density
from .packed import PackedHandle, mean_kin, packed_dot, rayleigh_ritz  # noqa: F401  (packed_dot: used here and by callers)
from .terms import energy_hamiltonian

ARMIJO_C1 = 1e-4            # LineSearches.BackTracking defaults: c_1, rho_hi, rho_lo, iterations
STEP_HI, STEP_LO = 0.5, 0.1
MAX_TRIALS = 50


# ------------------------------------------------------------------------------------------ line search
def backtracking(phi, phi0, dphi0, alpha0=1.0, c1=ARMIJO_C1, max_trials=MAX_TRIALS):
    """``LineSearches.BackTracking(order=3)`` from the static first step ``alpha0`` on scalars: ``phi(alpha)`` is the
    objective along the search curve, ``phi0 = phi(0)``, ``dphi0 = phi'(0) < 0``.  Accept when
    phi(alpha) <= phi0 + c1 alpha dphi0; the first retry takes the minimiser of the parabola through (phi0, dphi0, phi(alpha)),
    later ones that of the cubic through the last two trials, each clipped to [0.1 alpha, 0.5 alpha]; a non-finite value
    halves alpha.  ``RuntimeError`` after ``max_trials`` evaluations.  Returns ``(alpha, phi(alpha), trials)``."""
    a_prev, a = alpha0, alpha0
    f_prev = phi0
    f = phi(a)
    trials, retries = 1, 0
    while True:
        if not math.isfinite(f):
            a_prev, a = a, 0.5 * a
            retries = 0                          # (the interpolation restarts from the first finite value)
        elif f <= phi0 + c1 * a * dphi0:
            return a, f, trials
        else:
            retries += 1
            if retries == 1:
                a_new = -dphi0 * a * a / (2.0 * (f - phi0 - dphi0 * a))
            else:
                r1, r0 = f - phi0 - dphi0 * a, f_prev - phi0 - dphi0 * a_prev
                div = 1.0 / (a_prev ** 2 * a ** 2 * (a - a_prev))
                ca = (a_prev ** 2 * r1 - a ** 2 * r0) * div
                cb = (-a_prev ** 3 * r1 + a ** 3 * r0) * div
                # the minimiser of phi0 + dphi0 t + cb t^2 + ca t^3, (-cb + sqrt(cb^2 - 3 ca dphi0)) / (3 ca), in the form that
                # does not cancel for cb > 0 and passes to the parabola's -dphi0 / (2 cb) as ca -> 0
                root = math.sqrt(max(cb * cb - 3.0 * ca * dphi0, 0.0))
                if cb > 0:
                    a_new = -dphi0 / (cb + root)
                else:
                    a_new = (-cb + root) / (3.0 * ca) if ca != 0 else math.inf
            if not math.isfinite(a_new):
                a_new = STEP_HI * a
            a_prev, f_prev = a, f
            a = max(min(a_new, STEP_HI * a), STEP_LO * a)
        if trials >= max_trials:
            raise RuntimeError(f"direct_minimization: the line search found no acceptable step in {max_trials} trials "
                               f"(phi0 = {phi0!r}, dphi0 = {dphi0!r}, last alpha = {a_prev!r})")
        f = phi(a)
        trials += 1


# ------------------------------------------------------------------------------------------ checks
def n_bands_full(model):
    return int(-(-model.n_electrons // (model.n_spin_components * model.filled_occupation)))


def check_supported(basis, psi=None, who="direct_minimization"):
    """The refusals of this solver, on descriptors alone (no device work)."""
    model = basis.model
    from .model import refuse_meta_gga
    refuse_meta_gga(model, f"{who} (the gradient has no div-A-grad term, the line search no tau)")
    if model.temperature != 0:
        raise ValueError(f"{who}: only full occupations are supported (the model has a temperature)")
    per_band = model.n_spin_components * model.filled_occupation
    n_bands = n_bands_full(model)
    if n_bands * per_band != model.n_electrons:
        raise ValueError(f"{who}: {model.n_electrons} electrons do not fill {n_bands} bands of {per_band} electrons each")
    from .exchange import refuse as refuse_exchange
    from .hubbard import refuse as refuse_hubbard
    refuse_exchange(model, who)
    refuse_hubbard(model, who)
    if basis.comm_kpts.size > 1:
        raise NotImplementedError(f"{who}: a basis whose k-points are sharded over comm_kpts is not implemented (one rank)")
    if basis.comm_pw.size > 1:
        raise NotImplementedError(f"{who}: a basis whose plane waves are sharded over comm_pw is not implemented (one rank)")
    if psi is not None:
        if len(psi) != len(basis.kpoints):
            raise ValueError(f"{who}: psi has {len(psi)} blocks, the basis {len(basis.kpoints)} k-blocks")
        for ik, (kpt, p) in enumerate(zip(basis.kpoints, psi)):
            if tuple(p.shape) != (n_bands, kpt.n_G):
                raise ValueError(f"{who}: psi[{ik}] is {tuple(p.shape)}, expected {(n_bands, kpt.n_G)} (n_bands = "
                                 f"ceil(n_electrons / (n_spin * filled_occupation)) rows; select_occupied_orbitals removes "
                                 "the others)")
    return n_bands


# ------------------------------------------------------------------------------------------ device pieces
def project_tangent_(basis, kpt, g, x):
    """Optim's ``project_tangent!(Stiefel(), g, x)`` on one band-major block, in place: g -= x (x'g + g'x) / 2."""
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_stiefel_project_tangent(basis.lane_handles[kpt.lane], kpt.n_G, g.shape[0], x.data_ptr(),
                                                         x.stride(0), g.data_ptr(), g.stride(0)))
    basis.post_call(kpt.lane)
    return g


def retract_(basis, kpt, x):
    """Optim's ``retract!(Stiefel(), x)``: the polar factor of the block, in place (``dftk_mi_lowdin_ortho``)."""
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_lowdin_ortho(basis.lane_handles[kpt.lane], kpt.n_G, x.shape[0], x.data_ptr(), x.stride(0),
                                              None))
    basis.post_call(kpt.lane)
    return x


class LbfgsNative(PackedHandle):
    """The L-BFGS history behind the C ABI (``dftk_mi_lbfgs_*``) for packed vectors shaped like ``blocks`` (band-major
    tensors; only their shapes are read)."""

    def __init__(self, basis, shapes, memory=10):
        super().__init__(basis, shapes, "dftk_mi_lbfgs_create", int(memory))

    def update(self, x, g):
        """-> (<s, y>, kept)"""
        sy, kept = C.c_double(0.0), C.c_int(0)
        self._call("dftk_mi_lbfgs_update", *self._tables(x, g), C.byref(sy), C.byref(kept))
        return float(sy.value), bool(kept.value)

    def direction(self, g, scale, kpoints=None, mean_kin=None):
        """d = -H g as new blocks; ``kpoints`` and ``mean_kin`` (one float64 array per block) switch the preconditioner on"""
        n = len(self.shapes)
        d = [torch.empty_like(b) for b in g]
        gp, gl, dp, dl = self._tables(g, d)
        sc = (C.c_double * n)(*[float(s) for s in scale])
        kbs = mks = None
        if kpoints is not None:
            keep = [np.ascontiguousarray(m, dtype=np.float64) for m in mean_kin]
            kbs = (C.c_void_p * n)(*[k.handle.value for k in kpoints])
            mks = (C.c_void_p * n)(*[m.ctypes.data for m in keep])
        self._call("dftk_mi_lbfgs_direction", gp, gl, kbs, mks, sc, dp, dl)
        return d

    def reset(self):
        _lib.check(self.basis.lib.dftk_mi_lbfgs_reset(self.handle))

    @property
    def history(self):
        return int(self.basis.lib.dftk_mi_lbfgs_history(self.handle))


def energy_gradient(basis, psi, occupation):
    """``fg!`` of the reference (:149-163) with the gradient projected onto the tangent space: the total energy, the
    blocks 2 filled_occ w_k H_k psi_k projected at psi_k, and what the evaluation built on the way."""
    filled = basis.model.filled_occupation
    rho = compute_density(basis, psi, occupation)
    energies, ham = energy_hamiltonian(basis, psi, occupation, rho=rho)
    G = []
    for kpt, w, Hk, p in zip(basis.kpoints, basis.kweights, ham, psi):
        g = Hk @ p
        g *= 2.0 * filled * float(w)
        G.append(project_tangent_(basis, kpt, g, p))
    return dict(E=energies.total, G=G, rho=rho, energies=energies, ham=ham, psi=psi)


# ------------------------------------------------------------------------------------------ driver
def direct_minimization(basis, psi=None, tol=1e-6, is_converged=None, maxiter=1000, memory=10, callback=None, seed=0):
    """``direct_minimization(basis; psi, tol, is_converged, maxiter, callback, seed)`` (direct_minimization.jl:68-201) with
    Optim's preconditioned L-BFGS (``memory`` pairs) written out.  Convergence: ``ScfConvergenceDensity(tol)`` on
    |rho_out - rho| sqrt(dvol), rho_out being the density of the unit step along the next search direction (the first trial
    point of the next line search, whose energy and gradient that line search reuses); as in the reference one more step is
    taken after the criterion holds.  Returns a dict with the keys of an ``scfres`` that post-processing reads, plus
    ``linesearch_trials`` and ``linesearch_steps`` (phi0, dphi0, alpha, phi per iteration), ``history_pairs_kept`` and
    ``linesearch_failed`` (the run ended, as Optim's does, because a line search found no acceptable step)."""
    n_bands = check_supported(basis, psi)
    if int(memory) < 1:
        raise ValueError("direct_minimization: memory >= 1 is required")
    basis._require_gpu()
    t0 = time.time()
    model = basis.model
    filled = model.filled_occupation
    is_converged = is_converged or (lambda info: info["history_drho"][-1] < tol)       # ScfConvergenceDensity
    occupation = [np.full(n_bands, float(filled)) for _ in basis.kpoints]
    sqrt_dvol = math.sqrt(basis.dvol)

    with basis.on_library_stream():
        if psi is None:
            from .eigen import random_orbitals
            gen = torch.Generator(device=basis.device)
            gen.manual_seed(int(seed))
            psi = [random_orbitals(basis, kpt, n_bands, gen) for kpt in basis.kpoints]
        else:
            psi = [p.to(device=basis.device, dtype=torch.complex128).clone().contiguous() for p in psi]
        for kpt, p in zip(basis.kpoints, psi):           # the start point on the manifold
            retract_(basis, kpt, p)

        lb = LbfgsNative(basis, [p.shape for p in psi], memory)
        try:
            cur = energy_gradient(basis, psi, occupation)
            lb.update(cur["psi"], cur["G"])
            history_Etot, history_drho, trials_log, steps_log, kept_log = [], [], [], [], []
            converged, n_iter, linesearch_failed = False, 0, False
            info = None

            def search_direction():
                mk = mean_kin(basis, cur["psi"])
                d = lb.direction(cur["G"], basis.kweights, basis.kpoints, mk)
                for kpt, dk, p in zip(basis.kpoints, d, cur["psi"]):
                    project_tangent_(basis, kpt, dk, p)
                return d, float(packed_dot(cur["G"], d).item())

            def trial(d, alpha):
                x = []
                for kpt, p, dk in zip(basis.kpoints, cur["psi"], d):
                    x.append(retract_(basis, kpt, torch.add(p, dk, alpha=alpha)))
                return energy_gradient(basis, x, occupation)

            while not converged:
                d, dphi0 = search_direction()
                if not dphi0 < 0:                        # Optim's rule: not a descent direction -> restart the history
                    lb.reset()
                    lb.update(cur["psi"], cur["G"])
                    d, dphi0 = search_direction()
                cache = {1.0: trial(d, 1.0)}
                if n_iter >= 1:
                    drho = float(torch.linalg.norm(cache[1.0]["rho"] - cur["rho"]).item()) * sqrt_dvol
                    history_drho.append(drho)
                    history_Etot.append(cur["E"])
                    info = dict(ham=cur["ham"], basis=basis, energies=cur["energies"], occupation=occupation,
                                rho=cache[1.0]["rho"], rho_in=cur["rho"], psi=cur["psi"], runtime=time.time() - t0,
                                history_drho=history_drho, history_Etot=history_Etot, stage="iterate", algorithm="DM",
                                n_iter=n_iter)
                    converged = bool(is_converged(info))
                    if callback is not None:
                        callback(info)
                if n_iter >= maxiter:
                    break
                last = {}

                def phi(alpha):
                    res = cache.pop(alpha, None) or trial(d, alpha)
                    last["res"], last["alpha"] = res, alpha
                    return res["E"]

                try:
                    alpha, f, trials = backtracking(phi, cur["E"], dphi0)
                except RuntimeError:
                    # Optim ends the run at the current point when its line search fails (at the rounding floor of the
                    # energy no step can show a decrease any more); the result says so
                    linesearch_failed = True
                    break
                steps_log.append(dict(phi0=cur["E"], dphi0=dphi0, alpha=alpha, phi=f))
                trials_log.append(trials)
                cur = last["res"]
                _, kept = lb.update(cur["psi"], cur["G"])
                kept_log.append(kept)
                n_iter += 1

            eigenvalues, psi_rr = rayleigh_ritz(basis, cur["ham"], cur["psi"])
            basis.sync()
        finally:
            lb.close()

    result = dict(basis=basis, ham=cur["ham"], energies=cur["energies"], converged=converged, rho=cur["rho"], psi=psi_rr,
                  eigenvalues=eigenvalues, occupation=occupation, eF=None, n_bands_converge=n_bands, n_iter=n_iter,
                  history_Etot=history_Etot, history_drho=history_drho, algorithm="DM", seed=seed,
                  runtime=time.time() - t0, linesearch_trials=trials_log, linesearch_steps=steps_log,
                  history_pairs_kept=kept_log, linesearch_failed=linesearch_failed, stage="finalize")
    if callback is not None:
        callback(result)
    return result
