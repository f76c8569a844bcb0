"""Potential-mixing SCF with a backtracking line search and adaptive damping (host mirror of src/scf/potential_mixing.jl;
Herbst & Levitt, "A robust and efficient line search for self-consistent field iterations").

* ``ScfAcceptStepAll``, ``ScfAcceptImprovingStep`` (:3-22): when a trial step of the line search is taken.
* ``scf_damping_quadratic_model`` (:29-78): the quadratic model of E(V_in + alpha dV) along the search direction.
* ``AdaptiveDamping`` with ``ensure_damping_within_range``, ``propose_backtrack_damping``, ``trial_damping`` (:81-144) and
  ``FixedDamping`` (:146-151).
* ``total_local_potential`` / ``hamiltonian_with_total_potential``: the two seams to the Hamiltonian (Hamiltonian.jl).
* ``scf_potential_mixing`` (:160-293) and ``scf_potential_mixing_adaptive`` (:301-307): the drivers.

An ``info`` is a dict with the keys of the reference's named tuple, ASCII as elsewhere (``rho``, ``psi``, ``eF``, ``alpha``,
``Pinv_dV``).  The loop itself (``_potential_mixing_loop``) takes the step function, the mixing, the accelerator and the
scalar block as arguments, so the line search runs on host tensors as well (tests/test_potmix_host.py).

The cube-sized scalars of a trial step -- <V_out - V_in, drho>, <V_next - V_in, drho>, <drho, K drho>, |P^-1 dV|^2 and
|rho_next - rho_in|^2 -- come from ONE library call (``dftk_mi_diff_dots``, csrc/potmix_kernels.hip: one launch, one host
synchronisation, no temporary); they are kept under ``info["sums"]`` and everything that needs one reads it there.
``DFTK_MI_TORCH_LOCAL=1`` selects their torch twin.

Curvature of the model, <drho, K drho> (an extension with a switch): ``curvature="kernel"`` is the reference's form, K drho from
``apply_kernel`` (spin-unpolarised LDA, with or without core correction); ``"secant"`` takes K drho ~ V_out(rho_next) -
V_out(rho_in), the two output potentials the loop holds anyway -- exact in the Hartree part, off at second order in drho in the
exchange-correlation part, i.e. inside what ``modeltol`` tolerates -- and serves every model; ``None`` picks ``"kernel"`` where
``apply_kernel`` takes the model and ``"secant"`` elsewhere.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
import os
import time

import numpy as np
import torch

from .hamiltonian import DftHamiltonianBlock
from .mixing import KerkerDosMixing, KerkerMixing, SimpleMixing, _torch_mix
from .scf import AdaptiveBands, AndersonAcceleration, AndersonNative, determine_diagtol, next_density
from .eigen import lobpcg_hyper
from .terms import energy_hamiltonian, guess_density

EPS = float(np.finfo(np.float64).eps)
SUM_KEYS = ("dot_out", "dot_step", "dot_kernel", "pinv_norm2", "drho_norm2")


# ------------------------------------------------------------------------------------------ accepting a step
def ScfAcceptStepAll():
    """``ScfAcceptStepAll()`` (:3-5)"""
    def accept_step(info, info_next):
        return True
    return accept_step


def _pinv_norm(info):
    """norm(info.Pinv_dV): from the scalar block of the step where it is there"""
    sums = info.get("sums")
    if sums is not None and "pinv_norm2" in sums:
        return math.sqrt(max(sums["pinv_norm2"], 0.0))
    return float(torch.linalg.norm(info["Pinv_dV"]))


def ScfAcceptImprovingStep(max_energy_change=1e-12, max_relative_residual=1.0):
    """``ScfAcceptImprovingStep(; max_energy_change, max_relative_residual)`` (:11-22): accept a step if the energy is at most
    increasing by ``max_energy_change`` or the residual is at most ``max_relative_residual`` times that of the step before."""
    def accept_step(info, info_next):
        energy_change = info_next["energies"].total - info["energies"].total
        relative_residual = _pinv_norm(info_next) / _pinv_norm(info)
        return energy_change < max_energy_change or relative_residual < max_relative_residual
    accept_step.max_energy_change = max_energy_change
    accept_step.max_relative_residual = max_relative_residual
    return accept_step


# ------------------------------------------------------------------------------------------ quadratic model
def _torch_sums(info, info_next, curvature):
    """The scalar block (``SUM_KEYS``) of the step info -> info_next from their arrays with torch, on any device: what
    ``dftk_mi_diff_dots`` returns on the device path, for infos that carry none (hand-made ones, host tensors).
    ``curvature``: "secant", "kernel" or a callable drho -> K drho.  ``info`` None (the first point): the two norms only."""
    P = info_next.get("Pinv_dV")
    if info is None:
        d = info_next["rho"] - info_next["rho_in"]
        return dict(pinv_norm2=float((P * P).sum()), drho_norm2=float((d * d).sum()))
    drho = info_next["rho"] - info["rho"]
    if callable(curvature):
        Kdrho = curvature(drho)
    elif curvature == "secant":
        Kdrho = info_next["Vout"] - info["Vout"]
    else:
        from .response import apply_kernel
        Kdrho = apply_kernel(info["basis"], drho, rho=info["rho"])
    out = dict(dot_out=float(((info["Vout"] - info["Vin"]) * drho).sum()),
               dot_step=float(((info_next["Vin"] - info["Vin"]) * drho).sum()),
               dot_kernel=float((drho * Kdrho).sum()), drho_norm2=float((drho * drho).sum()))
    if P is not None:
        out["pinv_norm2"] = float((P * P).sum())
    return out


def quadratic_model_coefficients(info, info_next, curvature=None):
    """``(slope, curv)`` of the quadratic model (:54-56), see ``scf_damping_quadratic_model``"""
    sums = info_next.get("sums")
    if sums is None or "dot_kernel" not in sums:
        sums = _torch_sums(info, info_next, curvature if curvature is not None else info_next.get("curvature") or "kernel")
    dvol = info["dvol"] if "dvol" in info else info["basis"].dvol
    alpha0 = info_next["alpha"]
    return float(sums["dot_out"] / alpha0 * dvol), float(dvol * (-sums["dot_step"] + sums["dot_kernel"]) / alpha0 ** 2)


def scf_damping_quadratic_model(info, info_next, modeltol=0.1, curvature=None):
    """``scf_damping_quadratic_model(info, info_next; modeltol)`` (:29-78): a damping from the quadratic model
    phi(alpha) = E(V_in) + slope alpha + curv alpha^2 / 2 of the energy along dV, with
    slope = <V_out - V_in, drho> dvol / alpha0 and curv = (-<V_next - V_in, drho> + <drho, K drho>) dvol / alpha0^2.
    Returns ``(alpha, relerror)``; ``alpha`` is None when the model is not trusted.  The three inner products are those of
    ``info_next["sums"]`` where the loop has left them; otherwise they are formed from the arrays with ``curvature``
    ("kernel" -- also None --, "secant", or a callable drho -> K drho)."""
    slope, curv = quadratic_model_coefficients(info, info_next, curvature)
    alpha0 = info_next["alpha"]
    E0, E_next = info["energies"].total, info_next["energies"].total
    Emodel = E0 + slope * alpha0 + curv * alpha0 ** 2 / 2
    # (0 / 0 -> NaN as in the reference: every comparison below is then false and the model is discarded)
    denom = abs(E_next - E0)
    model_relerror = abs(E_next - Emodel) / denom if denom > 0 else (math.nan if E_next == Emodel else math.inf)
    info_next["model_relerror"] = model_relerror

    minimum_exists = curv > EPS                      # does the model predict a minimum along the search direction
    trusted_model = model_relerror < modeltol        # model fits observation
    tight_model = model_relerror < modeltol / 5      # model fits observation very well
    if minimum_exists and (tight_model or (slope < -EPS and trusted_model)):
        return -slope / curv, model_relerror
    return None, model_relerror


# ------------------------------------------------------------------------------------------ damping
class AdaptiveDamping:
    """``AdaptiveDamping`` (:81-99): adaptive damping using the quadratic model.  ``AdaptiveDamping(alpha_trial_min)``, one
    positional argument, selects the reference's derived defaults: alpha_min = alpha_trial_min / 4,
    alpha_max = max(1.25 alpha_trial_min, 1), alpha_trial_init = max(alpha_trial_min, 0.8)."""

    def __init__(self, *args, alpha_min=None, alpha_max=None, alpha_trial_init=None, alpha_trial_min=None,
                 alpha_trial_enhancement=1.1, modeltol=0.1):
        if len(args) > 1:
            raise TypeError("AdaptiveDamping takes at most one positional argument (alpha_trial_min)")
        if args:
            if alpha_trial_min is not None:
                raise TypeError("AdaptiveDamping: alpha_trial_min given twice")
            alpha_trial_min = float(args[0])
            alpha_min = alpha_trial_min / 4 if alpha_min is None else alpha_min
            alpha_max = max(1.25 * alpha_trial_min, 1.0) if alpha_max is None else alpha_max
            alpha_trial_init = max(alpha_trial_min, 0.8) if alpha_trial_init is None else alpha_trial_init
        self.alpha_min = 0.05 if alpha_min is None else float(alpha_min)                  # minimal damping
        self.alpha_max = 1.0 if alpha_max is None else float(alpha_max)                   # maximal damping
        self.alpha_trial_init = 0.8 if alpha_trial_init is None else float(alpha_trial_init)   # trial damping of the first step
        self.alpha_trial_min = 0.2 if alpha_trial_min is None else float(alpha_trial_min)      # minimal trial damping of a step
        self.alpha_trial_enhancement = float(alpha_trial_enhancement)   # factor on alpha_trial after an immediately good step
        self.modeltol = float(modeltol)     # maximal relative error on the predicted energy for the model to be trusted

    def __repr__(self):
        return (f"AdaptiveDamping(alpha_min={self.alpha_min}, alpha_max={self.alpha_max}, alpha_trial_init="
                f"{self.alpha_trial_init}, alpha_trial_min={self.alpha_trial_min}, alpha_trial_enhancement="
                f"{self.alpha_trial_enhancement}, modeltol={self.modeltol})")


class FixedDamping:
    """``FixedDamping(alpha = 0.8)`` (:146-151)"""

    def __init__(self, alpha=0.8):
        self.alpha = float(alpha)

    def __repr__(self):
        return f"FixedDamping({self.alpha})"


def _clamp(x, lo, hi):
    return max(lo, min(hi, x))


def ensure_damping_within_range(damping, alpha, alpha_next):
    """``ensure_damping_within_range(damping, alpha, alpha_next)`` (:101-113)"""
    alpha_sign = float(np.sign(alpha_next))
    if abs(alpha_next) <= damping.alpha_min / 5:
        alpha_sign = +1.0
    if alpha_sign > 0.0:
        alpha_next = min(0.95 * abs(alpha), abs(alpha_next))      # avoid getting stuck
    else:
        alpha_next = min(0.50 * abs(alpha), abs(alpha_next))      # don't move too far backwards (model validity)
    alpha_next = _clamp(alpha_next, damping.alpha_min, damping.alpha_max)
    return float(alpha_sign * alpha_next)


def propose_backtrack_damping(damping, info=None, info_next=None):
    """``propose_backtrack_damping(damping, info, info_next)`` (:115-127, :150)"""
    if isinstance(damping, FixedDamping):
        return damping.alpha
    if abs(info_next["alpha"]) < 1.75 * damping.alpha_min:
        return info_next["alpha"]            # too close to alpha_min to be worth making another step ... just give up
    alpha_next, relerror = scf_damping_quadratic_model(info, info_next, modeltol=damping.modeltol)
    if alpha_next is None:
        # model failed ... use heuristics: half for small model error, else use a quarter
        alpha_next = info_next["alpha"] / (2 if relerror < 10 else 4)
    return ensure_damping_within_range(damping, info_next["alpha"], alpha_next)


def trial_damping(damping, info=None, info_next=None, step_successful=None):
    """``trial_damping(damping)`` and ``trial_damping(damping, info, info_next, step_successful)`` (:129-144, :151)"""
    if isinstance(damping, FixedDamping):
        return damping.alpha
    if info_next is None:
        return damping.alpha_trial_init
    n_backtrack = len(info_next["diagonalization"])
    alpha_trial = abs(info_next["alpha"])                  # by default use the alpha that worked in this step
    if step_successful and n_backtrack == 1:               # first step was good => speed things up
        if alpha_trial >= damping.alpha_max:
            return damping.alpha_max                       # no need to compute the model
        alpha_model = scf_damping_quadratic_model(info, info_next, modeltol=damping.modeltol)[0]
        if alpha_model is not None:                        # model is meaningful
            alpha_trial = max(damping.alpha_trial_enhancement * abs(alpha_model), alpha_trial)
    return _clamp(alpha_trial, damping.alpha_trial_min, damping.alpha_max)


# ------------------------------------------------------------------------------------------ Hamiltonian seams
def _spin_stacked_shape(basis):
    nx, ny, nz = basis.fft_size
    return (nz, ny, nx) if basis.model.n_spin_components == 1 else (basis.model.n_spin_components, nz, ny, nx)


def total_local_potential(ham):
    """``total_local_potential(ham)`` (Hamiltonian.jl): the summed local potential the blocks of ``ham`` apply, a
    ``(nz, ny, nx)`` cube, or ``(2, nz, ny, nx)`` with collinear spin (the spin-up blocks come first)."""
    if ham[0].potential is None:
        raise ValueError("total_local_potential: the Hamiltonian has no local potential")
    if ham[0].basis.model.n_spin_components == 2:
        return torch.stack([ham[0].potential, ham[len(ham) // 2].potential])
    return ham[0].potential


def hamiltonian_with_total_potential(ham, V):
    """``hamiltonian_with_total_potential(ham, V)``: new blocks for every k-point of ``ham`` that apply the total local
    potential ``V`` beside the kinetic and nonlocal terms (``DftHamiltonianBlock.for_all_kpoints``).  The blocks of ``ham``
    are not touched: they keep their potential and bind it again when they are applied next."""
    basis = ham[0].basis
    if not torch.is_tensor(V) or tuple(V.shape) != _spin_stacked_shape(basis):
        raise ValueError(f"hamiltonian_with_total_potential: V must have the shape {_spin_stacked_shape(basis)}, got "
                         f"{tuple(V.shape) if torch.is_tensor(V) else type(V).__name__}")
    return DftHamiltonianBlock.for_all_kpoints(basis, V)


# ------------------------------------------------------------------------------------------ checks
def kernel_curvature_refusal(basis):
    """The refusal ``apply_kernel`` would raise for this model, found on descriptors alone; None when it takes the model."""
    from .response import _KERNEL_LDA
    from .terms import _GGA_BITS
    from .refine import check_supported as kernel_scope
    try:
        kernel_scope(basis, "scf_potential_mixing(curvature='kernel'): apply_kernel")
        for name in basis.model.functionals:
            if name in _GGA_BITS:
                raise NotImplementedError(f"apply_kernel: the kernel of the GGA functional {name} is not implemented")
            if name not in _KERNEL_LDA:
                raise NotImplementedError(f"apply_kernel: the kernel of {name} is not implemented (closed forms exist for "
                                          f"{_KERNEL_LDA})")
    except NotImplementedError as e:
        return e
    return None


def check_supported(basis, mixing=None, psi=None, V=None, max_backtracks=3, curvature=None, who="scf_potential_mixing"):
    """The refusals of this solver, on descriptors alone (no device work).  Returns the curvature form in use."""
    model = basis.model
    from .model import refuse_meta_gga
    from .exchange import refuse as refuse_exchange
    from .hubbard import refuse as refuse_hubbard
    refuse_meta_gga(model, who)                       # (as the reference: :186-188)
    refuse_exchange(model, f"{who} (the orbitals that build the Fock operator are no function of the potential)")
    refuse_hubbard(model, f"{who} (the occupation matrices are no function of the potential)")
    if basis.comm_kpts.size > 1:
        raise NotImplementedError(f"{who}: a basis whose k-points are sharded over comm_kpts is not implemented (one rank)")
    if basis.comm_pw.size > 1:
        raise NotImplementedError(f"{who}: a basis whose plane waves are sharded over comm_pw is not implemented (one rank)")
    if mixing is not None and not isinstance(mixing, (SimpleMixing, KerkerMixing, KerkerDosMixing)):
        raise NotImplementedError(f"{who}: mixing must be SimpleMixing, KerkerMixing or KerkerDosMixing (the reference's "
                                  f"assertion), got {type(mixing).__name__}")
    if curvature not in (None, "kernel", "secant"):
        raise ValueError(f"{who}: curvature is None, 'kernel' or 'secant'")
    refusal = kernel_curvature_refusal(basis) if curvature != "secant" else None
    if curvature == "kernel" and refusal is not None:
        raise refusal
    if psi is not None and len(psi) != len(basis.kpoints):
        raise ValueError(f"{who}: psi has {len(psi)} blocks, the basis {len(basis.kpoints)} k-blocks")
    if V is not None and (not torch.is_tensor(V) or tuple(V.shape) != _spin_stacked_shape(basis)):
        raise ValueError(f"{who}: V must have the shape {_spin_stacked_shape(basis)}, got "
                         f"{tuple(V.shape) if torch.is_tensor(V) else type(V).__name__}")
    if int(max_backtracks) < 1:
        raise ValueError(f"{who}: max_backtracks must be at least 1")
    return "secant" if (curvature == "secant" or refusal is not None) else "kernel"


# ------------------------------------------------------------------------------------------ scalar block
def diff_dots(basis, pairs):
    """``dftk_mi_diff_dots``: [sum (a - b) (c - d) for (a, b, c, d) in pairs] over float64 device arrays of one size (b, d may
    be None) -- one launch, one host synchronisation.  ``DFTK_MI_TORCH_LOCAL=1``: the torch twin, one stacked fetch."""
    n = pairs[0][0].numel()
    for quad in pairs:
        for x in quad:
            if x is not None and not (x.is_cuda and x.dtype == torch.float64 and x.is_contiguous() and x.numel() == n):
                raise TypeError("diff_dots: contiguous float64 CUDA arrays of one size required")
    if os.environ.get("DFTK_MI_TORCH_LOCAL") is not None:
        diff = lambda x, y: x if y is None else x - y                  # noqa: E731
        return [float(v) for v in torch.stack([(diff(a, b) * diff(c, d)).sum() for a, b, c, d in pairs]).cpu()]
    from . import _lib
    m = len(pairs)
    tabs = [(C.c_void_p * m)(*[(q[j].data_ptr() if q[j] is not None else None) for q in pairs]) for j in range(4)]
    out = (C.c_double * m)()
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_diff_dots(basis.handle, n, m, *tabs, out))
    return [float(v) for v in out]


def _device_model_sums(basis, curvature, want_model):
    """The scalar block of a trial step on the device: every scalar of the step in ONE ``diff_dots`` call."""
    def model_sums(info, info_next):
        P = info_next["Pinv_dV"]
        if info is None:                  # the first point: no step to model
            rho, rho_in = info_next["rho"], info_next["rho_in"]
            return dict(zip(("pinv_norm2", "drho_norm2"), diff_dots(basis, [(P, None, P, None), (rho, rho_in, rho, rho_in)])))
        rho, rho_next = info["rho"], info_next["rho"]
        pairs = [(info["Vout"], info["Vin"], rho_next, rho), (info_next["Vin"], info["Vin"], rho_next, rho)]
        keys = ["dot_out", "dot_step"]
        if want_model:
            keys.append("dot_kernel")
            if curvature == "kernel":
                from .response import apply_kernel
                pairs.append((rho_next, rho, apply_kernel(basis, rho_next - rho, rho=rho), None))
            else:
                pairs.append((rho_next, rho, info_next["Vout"], info["Vout"]))
        pairs += [(P, None, P, None), (rho_next, rho, rho_next, rho)]
        return dict(zip(keys + ["pinv_norm2", "drho_norm2"], diff_dots(basis, pairs)))
    return model_sums


# ------------------------------------------------------------------------------------------ the loop
def _potential_mixing_loop(EVrho, mix, accelerate, model_sums, V, rho_in, damping, accept_step, dvol, psi=None,
                           max_backtracks=3, maxiter=100, is_converged=None, determine_tol=determine_diagtol, callback=None,
                           tol=1e-6, extra=None):
    """The iteration of ``scf_potential_mixing`` (:210-283) with its pieces as arguments:

    * ``EVrho(Vin, diagtol=, psi=, eigenvalues=, occupation=)`` -> dict(Vin, Vout, rho, psi, eigenvalues, occupation, energies,
      diagonalization, ...): diagonalise at V_in, build the density, its energies and its potential;
    * ``mix(dV, info, rho_in, n_iter)`` -> P^-1 dV (``mix_potential``);
    * ``accelerate(Vin, alpha, Pinv_dV)`` -> V_in + alpha * (accelerated step) (Anderson);
    * ``model_sums(info, info_next)`` -> the scalar block of the step info -> info_next (``SUM_KEYS``; ``info`` None at the first
      point: ``pinv_norm2`` and ``drho_norm2`` only).

    ``extra``: keys added to every info (``basis`` ...).  Returns ``(info, converged, stats)`` with ``stats`` the per-iteration
    lists ``alphas``, ``n_backtracks``, ``model_relerrors`` and the histories."""
    is_converged = is_converged or (lambda info: info["history_drho"][-1] < tol)        # ScfConvergenceDensity(tol)
    extra = dict(extra or {}, dvol=dvol)
    sqrt_dvol = math.sqrt(dvol)
    n_iter, converged, t0 = 1, False, time.time()
    alpha_trial = trial_damping(damping)
    diagtol = determine_tol(n_iter, [])
    info = EVrho(V, diagtol=diagtol, psi=psi)
    Pinv_dV = mix(info["Vout"] - info["Vin"], info, rho_in, n_iter)
    info = dict(info, **extra, alpha=math.nan, diagonalization=[info["diagonalization"]], rho_in=rho_in, n_iter=n_iter,
                Pinv_dV=Pinv_dV, diagtol=diagtol)
    info["sums"] = model_sums(None, info)
    n_matvec = int(info.get("n_matvec", 0))
    history_Etot, history_drho, alphas, n_backtracks, model_relerrors = [], [], [], [], []

    while n_iter < maxiter:
        history_Etot.append(info["energies"].total)
        history_drho.append(math.sqrt(max(info["sums"]["drho_norm2"], 0.0)) * sqrt_dvol)
        info = dict(info, stage="iterate", algorithm="SCF", converged=converged, runtime=time.time() - t0,
                    history_Etot=history_Etot, history_drho=history_drho, n_matvec=n_matvec)
        if callback is not None:
            callback(info)
        if is_converged(info):
            converged = True
            break
        n_iter += 1
        info = dict(info, n_iter=n_iter)

        dV = (accelerate(info["Vin"], alpha_trial, info["Pinv_dV"]) - info["Vin"]) / alpha_trial

        # determine damping and take next step
        guess = info["psi"]
        alpha = alpha_trial
        successful = False                   # successful line search (final step is considered good)
        n_backtrack = 1
        diagonalization = []
        info_next = info
        while n_backtrack <= max_backtracks:
            diagtol = determine_tol(info_next["n_iter"], info_next["history_drho"])
            Vnext = info["Vin"] + alpha * dV
            info_next = EVrho(Vnext, diagtol=diagtol, psi=guess, eigenvalues=info["eigenvalues"],
                              occupation=info["occupation"])
            Pinv_dV_next = mix(info_next["Vout"] - info_next["Vin"], info_next, info["rho"], n_iter)
            diagonalization.append(info_next["diagonalization"])
            n_matvec += int(info_next.get("n_matvec", 0))
            info_next = dict(info_next, **extra, alpha=alpha, diagonalization=diagonalization, rho_in=info["rho"],
                             n_iter=n_iter, Pinv_dV=Pinv_dV_next, history_drho=history_drho, history_Etot=history_Etot,
                             diagtol=diagtol)
            info_next["sums"] = model_sums(info, info_next)

            successful = bool(accept_step(info, info_next))
            if successful or n_backtrack >= max_backtracks:
                break
            n_backtrack += 1

            # adjust alpha to try again ...
            alpha_next = propose_backtrack_damping(damping, info, info_next)
            if alpha_next == alpha:          # backtracking further not useful ...
                break

            # adjust to the guess fitting alpha best
            guess = info_next["psi"] if alpha_next > alpha / 2 else info["psi"]
            alpha = alpha_next

        # update alpha_trial and commit the next state
        alpha_trial = trial_damping(damping, info, info_next, successful)
        alphas.append(info_next["alpha"])
        n_backtracks.append(len(diagonalization))
        model_relerrors.append(info_next.get("model_relerror", math.nan))
        info = info_next

    stats = dict(alphas=alphas, n_backtracks=n_backtracks, model_relerrors=model_relerrors, history_Etot=history_Etot,
                 history_drho=history_drho, n_iter=n_iter, n_matvec=n_matvec, runtime=time.time() - t0)
    return info, converged, stats


# ------------------------------------------------------------------------------------------ drivers
def make_EVrho(basis, ham, nbandsalg=None, eigensolver=lobpcg_hyper, diag_miniter=1, generator=None, seed=0, tol=1e-6):
    """``EVrho`` of the reference (:199-208) for a device basis: ``EVrho(Vin; diagtol, psi, eigenvalues, occupation)`` binds
    ``Vin`` beside the other terms of ``ham``, diagonalises, builds the density (``next_density``) and takes the energies and
    ``Vout`` of that density from the one fused local-potential call of ``energy_hamiltonian``."""
    nbandsalg = nbandsalg if nbandsalg is not None else AdaptiveBands(basis.model)

    def EVrho(Vin, diagtol=tol / 10, psi=None, eigenvalues=None, occupation=None):
        ham_V = hamiltonian_with_total_potential(ham, Vin)
        res_V = next_density(ham_V, nbandsalg, eigensolver, psi=psi, eigenvalues=eigenvalues, occupation=occupation,
                             tol=diagtol, generator=generator, seed=seed, miniter=diag_miniter)
        energies, new_ham = energy_hamiltonian(basis, res_V["psi"], res_V["occupation"], rho=res_V["rho"],
                                               eigenvalues=res_V["eigenvalues"], eF=res_V["eF"])
        return dict(res_V, basis=basis, ham=new_ham, energies=energies, Vin=Vin,
                    Vout=total_local_potential(new_ham).contiguous())
    return EVrho


def scf_potential_mixing(basis, damping=FixedDamping(0.8), nbandsalg=None, rho=None, V=None, psi=None, tol=1e-6, maxiter=100,
                         eigensolver=lobpcg_hyper, diag_miniter=1, determine_tol=determine_diagtol, mixing=None,
                         is_converged=None, callback=None, anderson_m=10, accept_step=None, max_backtracks=3, seed=0,
                         curvature=None):
    """``scf_potential_mixing(basis; damping, nbandsalg, rho, V, psi, tol, maxiter, eigensolver, diag_miniter, diagtolalg,
    mixing, is_converged, callback, acceleration, accept_step, max_backtracks, seed)`` (:160-293): SCF on the total local
    potential.  Every iteration takes the Anderson-accelerated, preconditioned step dV from V_in and searches along it:
    a trial V_in + alpha dV is diagonalised, and ``accept_step(info, info_next)`` decides whether it is taken; if not,
    ``propose_backtrack_damping`` gives the next alpha (at most ``max_backtracks`` trials), restarting from the orbitals that
    fit it best.  ``damping``: ``FixedDamping(0.8)`` unless given, a plain number means ``FixedDamping``;
    ``AdaptiveDamping`` needs further defaults changed, see ``scf_potential_mixing_adaptive``.  ``mixing``: ``SimpleMixing()``
    unless given; ``KerkerMixing`` and ``KerkerDosMixing`` are the others the reference admits.  ``determine_tol(n_iter,
    history_drho)``: ``AdaptiveDiagtol()`` unless given.  ``anderson_m``: the history of ``AndersonAcceleration(; m)``.
    ``curvature``: the form of <drho, K drho> in the quadratic model (module docstring).

    Returns a dict with the keys of the result of ``self_consistent_field`` (``ham`` is built from the last output
    potential; ``diagonalization`` is that of the accepted last trial, so that ``save_scfres`` takes the result), and
    ``alphas`` (the accepted alpha per iteration), ``n_backtracks`` (trials per iteration), ``model_relerrors`` (relative
    error of the quadratic model where an iteration evaluated it, NaN elsewhere).  ``callback(info)`` sees
    ``stage="iterate"`` once per iteration -- with ``alpha`` and ``diagonalization``, a list over the trials of the
    iteration -- and ``stage="finalize"`` with the result."""
    who = "scf_potential_mixing"
    if isinstance(damping, numbers.Real):
        damping = FixedDamping(damping)
    if not isinstance(damping, (FixedDamping, AdaptiveDamping)):
        raise TypeError(f"{who}: damping is a number, a FixedDamping or an AdaptiveDamping")
    mixing = SimpleMixing() if mixing is None else mixing
    curvature = check_supported(basis, mixing, psi, V, max_backtracks, curvature, who)
    basis._require_gpu()
    t0 = time.time()
    nbandsalg = nbandsalg if nbandsalg is not None else AdaptiveBands(basis.model)
    accept_step = accept_step if accept_step is not None else ScfAcceptStepAll()
    if determine_tol is None:
        determine_tol = determine_diagtol
    gen = torch.Generator(device=basis.device)
    gen.manual_seed(seed + 7919 * basis.comm_kpts.rank)
    accel = AndersonAcceleration(m=anderson_m) if _torch_mix() else AndersonNative(basis, m=anderson_m)

    with basis.on_library_stream():
        rho = guess_density(basis) if rho is None else rho
        # initial guess for V (if none given)
        ham0 = energy_hamiltonian(basis, None, None, rho=rho, only_hamiltonian=True)[1]
        if V is None:
            V = total_local_potential(ham0)
        V = V.to(device=basis.device, dtype=torch.float64).contiguous()

        EVrho = make_EVrho(basis, ham0, nbandsalg, eigensolver=eigensolver, diag_miniter=diag_miniter, generator=gen,
                           seed=seed, tol=tol)

        def mix(dV, info, rho_in, n_iter):          # mix_potential(mixing, basis, dV; ...) = mix_density(...)
            out = mixing.mix_density(basis, dV, eF=info["eF"], eigenvalues=info["eigenvalues"], psi=info["psi"],
                                     occupation=info["occupation"], rho_in=rho_in, n_iter=n_iter)
            return out.to(torch.float64).contiguous()

        try:
            info, converged, stats = _potential_mixing_loop(
                EVrho, mix, accel, _device_model_sums(basis, curvature, isinstance(damping, AdaptiveDamping)), V, rho, damping,
                accept_step, basis.dvol, psi=psi, max_backtracks=int(max_backtracks), maxiter=maxiter,
                is_converged=is_converged, determine_tol=determine_tol, callback=callback, tol=tol,
                extra=dict(basis=basis, curvature=curvature))
        finally:
            if hasattr(accel, "close"):
                accel.close()
        ham = hamiltonian_with_total_potential(ham0, info["Vout"])
        basis.sync()

    result = dict(ham=ham, basis=basis, energies=info["energies"], converged=converged, rho=info["rho"],
                  eigenvalues=info["eigenvalues"], occupation=info["occupation"], eF=info["eF"], n_iter=stats["n_iter"],
                  psi=info["psi"], n_bands_converge=info["n_bands_converge"], diagonalization=info["diagonalization"][-1],
                  stage="finalize", algorithm="SCF", history_drho=stats["history_drho"], history_Etot=stats["history_Etot"],
                  occupation_threshold=nbandsalg.occupation_threshold, seed=seed, runtime=time.time() - t0,
                  n_matvec=stats["n_matvec"], mixing=mixing, damping_alg=damping,
                  damping=float(stats["alphas"][-1]) if stats["alphas"] else float(trial_damping(damping)),
                  alphas=stats["alphas"], n_backtracks=stats["n_backtracks"], model_relerrors=stats["model_relerrors"],
                  curvature=curvature, Vin=info["Vin"], Vout=info["Vout"])
    if callback is not None:
        callback(result)
    return result


def scf_potential_mixing_adaptive(basis, tol=1e-6, damping=AdaptiveDamping(), **kwargs):
    """``scf_potential_mixing_adaptive(basis; tol, damping = AdaptiveDamping(), kwargs...)`` (:301-307): the defaults adaptive
    damping needs -- ``diag_miniter = 2``, ``ScfAcceptImprovingStep(max_energy_change = tol)`` and
    ``AdaptiveDiagtol(ratio_rhodiff = 0.03, diagtol_first = 5e-3, diagtol_max = 1e-3)`` -- each of which a keyword replaces."""
    if not isinstance(damping, AdaptiveDamping):
        raise TypeError("scf_potential_mixing_adaptive: damping must be an AdaptiveDamping")

    def determine_tol(n_iter, history_drho):
        return determine_diagtol(n_iter, history_drho, ratio=0.03, diagtol_first=5e-3, diagtol_max=1e-3)
    kw = dict(diag_miniter=2, accept_step=ScfAcceptImprovingStep(max_energy_change=tol), determine_tol=determine_tol)
    kw.update(kwargs)
    return scf_potential_mixing(basis, tol=tol, damping=damping, **kw)
