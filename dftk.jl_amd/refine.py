"""First-order refinement of a converged SCF on a larger basis (host mirror of src/postprocess/refine.jl; Cances, Dusson,
Kemlin, Levitt, *Practical error bounds for properties in plane-wave electronic structure calculations*, SIAM J. Sci.
Comput. 44 (5), 2022), with ``apply_Omega`` / ``apply_K`` of src/response/hessian.jl:25-73 and the tangent-space helpers of
src/scf/newton.jl:49-68.  Corrections are signed so that X + dX is the refined quantity.

The SCF result of a cheap basis is lifted to ``basis_ref`` (transfer.py) and ONE Newton step (Omega + K) dP = -R(P) is solved
there, split by frequency: on the plane waves the small basis lacks, Omega + K is replaced by the metric M
(``invert_refinement_metric``: ``dftk_mi_refinement_metric_solve``, one library call per k-point), on the small basis it
is inverted by ``solve_OmegaPlusK_split`` -- the same linear system as the reference's ``solve_OmegaPlusK`` for the fully
occupied models accepted here (hessian.jl:111-176 and :266-359 both return dpsi with (Omega + K) dpsi = -dH_ext psi).

Spellings are ASCII (``Omega`` for the reference's capital omega, ``d`` / ``delta`` for its delta), as in response.py.  Orbital
blocks are band-major ``(n_bands, n_G)`` complex128 CUDA tensors.  Scope: spin-unpolarised LDA, HGH or UPF species (with or
without non-linear core correction), full occupations, one rank; everything else is refused before any device work.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .densities import compute_density
from .packed import overlaps, sub_product
from .response import (EPS, _check_block, apply_kernel, compute_delta_rho, multiply_psi_by_potential, occupied_empty_masks,
                       solve_OmegaPlusK_split)
from .terms import _GGA_BITS, Energies, energy_hamiltonian, total_density
from .transfer import check_same_kpoints, check_same_lattice, transfer_blochwave, transfer_density

METRIC_TOL = 100 * EPS          # refine.jl:66
METRIC_MAXITER = 20


# ------------------------------------------------------------------------------------------ checks
def check_supported(basis, who="refine_scfres"):
    """The refusals of this layer, on descriptors alone (no device work): ``NotImplementedError`` names the reason."""
    model = basis.model
    from .model import refuse_meta_gga
    refuse_meta_gga(model, who)
    if model.n_spin_components != 1:
        raise NotImplementedError(f"{who}: collinear spin is not implemented (the exchange-correlation kernel is "
                                  "spin-unpolarised)")
    if any(f in _GGA_BITS for f in model.functionals):
        raise NotImplementedError(f"{who}: GGA functionals are not implemented (no GGA kernel in apply_kernel)")
    from .exchange import refuse as refuse_exchange
    from .hubbard import refuse as refuse_hubbard
    refuse_exchange(model, f"{who} (no exchange kernel term)")
    refuse_hubbard(model, f"{who} (no Hubbard kernel term)")
    if basis.comm_pw.size > 1:
        raise NotImplementedError(f"{who}: a basis whose plane waves are sharded over comm_pw is not implemented")
    if basis.comm_kpts.size > 1:
        raise NotImplementedError(f"{who}: a basis whose k-points are sharded over comm_kpts is not implemented (one rank)")


def check_full_occupation(basis, occupation):
    """occupation.jl:232-237: every occupation equals ``filled_occupation``; ``ValueError`` otherwise."""
    filled = basis.model.filled_occupation
    for occ_k in occupation:
        if not np.all(np.asarray(occ_k, dtype=float) == filled):
            raise ValueError(f"Only full occupation is supported, but {np.asarray(occ_k)} has partial occupation.")


def select_occupied_orbitals(basis, psi, occupation, threshold=0.0):
    """``select_occupied_orbitals(basis, psi, occupation; threshold)`` (orbitals.jl:7-21): the bands up to the last one
    occupied above ``threshold``, as views, with their occupations.  ``(psi, occupation)``."""
    masks = occupied_empty_masks(occupation, threshold)
    sel_psi = [psik[:n] for psik, (n, _) in zip(psi, masks)]
    sel_occ = [np.asarray(occ, dtype=float)[:n] for occ, (n, _) in zip(occupation, masks)]
    if threshold == 0 and sel_psi:
        model = basis.model
        n_bands = -(-model.n_electrons // (model.n_spin_components * model.filled_occupation))
        if n_bands != sel_psi[0].shape[0]:
            raise ValueError(f"select_occupied_orbitals: {sel_psi[0].shape[0]} occupied bands kept, {n_bands} expected for an "
                             "insulator")
    return sel_psi, sel_occ


def _check_contains(basis, basis_ref):
    """every sphere of basis_ref contains the sphere of basis at the same k-point (on descriptors: the integer G vectors)"""
    for ik, (a, b) in enumerate(zip(basis.kpoints, basis_ref.kpoints)):
        nx, ny, nz = basis_ref.fft_size
        G = a.G_vectors.cpu().numpy()
        ok = np.all(np.abs(G) <= (np.array([nx, ny, nz]) - 1) // 2, axis=1)
        lin = (G[:, 0] % nx) + nx * ((G[:, 1] % ny) + ny * (G[:, 2] % nz))
        if not (ok.all() and np.isin(lin, b.mapping).all()):
            raise ValueError(f"refine_scfres: the sphere of basis_ref at k-point {ik} does not contain that of the SCF basis "
                             "(basis_ref must have the larger Ecut and a grid that holds it)")


# ------------------------------------------------------------------------------------------ tangent space
def proj_tangent_kpt_(basis, kpt, dpsik, psik):
    """``proj_tangent_kpt!`` (newton.jl:57-60): dpsik -= psik (psik' dpsik), two library zgemm calls."""
    return sub_product(basis, kpt, dpsik, psik, overlaps(basis, kpt, psik, dpsik))


def proj_tangent(basis, dpsi, psi):
    return [proj_tangent_kpt_(basis, kpt, d.clone().contiguous(), p) for kpt, d, p in zip(basis.kpoints, dpsi, psi)]


def compute_projected_gradient(basis, psi, occupation):
    """``compute_projected_gradient`` (newton.jl:49-54): with H the Hamiltonian of the density of ``psi``, the blocks
    ``(1 - psi_k psi_k') H_k psi_k``.  As in the reference's code there is NO factor f_n on band n: ``occupation`` enters
    through the density that H is built from, and nowhere else (for the full occupations accepted here the factor would be
    the constant ``filled_occupation``, and (Omega + K) of hessian.jl is scaled to go without it)."""
    check_supported(basis, "compute_projected_gradient")
    basis._require_gpu()
    rho = compute_density(basis, psi, occupation)
    _, ham = energy_hamiltonian(basis, psi, occupation, rho=rho)
    return [proj_tangent_kpt_(basis, kpt, Hk @ psik.contiguous(), psik) for kpt, Hk, psik in zip(basis.kpoints, ham, psi)]


def apply_Omega(dpsi, psi, ham, Lambda):
    """``apply_Omega(dpsi, psi, H, Lambda)`` (hessian.jl:31-39): P (H d - d Lambda) with d = P dpsi and Lambda_k = psi_k' H_k
    psi_k (as ``rayleigh_coefficients`` returns them)."""
    basis = ham[0].basis
    out = []
    for kpt, Hk, d, p, L in zip(basis.kpoints, ham, proj_tangent(basis, dpsi, psi), psi, Lambda):
        Od = Hk @ d
        sub_product(basis, kpt, Od, d, L)
        out.append(proj_tangent_kpt_(basis, kpt, Od, p))
    return out


def apply_K(basis, dpsi, psi, rho, occupation):
    """``apply_K(basis, dpsi, psi, rho, occupation)`` (hessian.jl:47-73): P (dV psi) with dV the Hartree and
    exchange-correlation kernel applied to the density change of d = P dpsi."""
    d = proj_tangent(basis, dpsi, psi)
    drho = compute_delta_rho(basis, psi, d, occupation)
    dV = apply_kernel(basis, drho, rho)
    Kd = multiply_psi_by_potential(basis, [p.contiguous() for p in psi], dV)
    return [proj_tangent_kpt_(basis, kpt, x, p) for kpt, x, p in zip(basis.kpoints, Kd, psi)]


def rayleigh_coefficients(ham, psi):
    """Lambda_k = psi_k' H_k psi_k (refine.jl:147-150)"""
    basis = ham[0].basis
    return [overlaps(basis, kpt, p, Hk @ p.contiguous()) for kpt, Hk, p in zip(basis.kpoints, ham, psi)]


# ------------------------------------------------------------------------------------------ metric
def invert_refinement_metric(basis, psi, res, tol=METRIC_TOL, maxiter=METRIC_MAXITER):
    """``invert_refinement_metric(basis, psi, res)`` (refine.jl:43-84): x with M_n x_n = P res_n for every band n of every
    k-point, M_n = P T_n^{1/2} P T_n^{1/2} P, T_n = kinetic + mean kinetic energy of band n, P = 1 - psi psi'.  One library
    call per k-point (``dftk_mi_refinement_metric_solve``: preconditioned CG on all columns at once).  A column that did not
    reach ``tol`` within ``maxiter`` passes gives a warning, as in the reference."""
    if basis.comm_pw.size > 1:
        raise NotImplementedError("invert_refinement_metric: a basis whose plane waves are sharded over comm_pw is not "
                                  "implemented")
    basis._require_gpu()
    out = []
    for ik, (kpt, psik, resk) in enumerate(zip(basis.kpoints, psi, res)):
        _check_block("invert_refinement_metric: psi", psik, kpt.n_G)
        _check_block("invert_refinement_metric: res", resk, kpt.n_G)
        if resk.shape != psik.shape:
            raise ValueError("invert_refinement_metric: one right-hand side per orbital")
        n = psik.shape[0]
        x = torch.empty_like(resk)
        iters = np.zeros(max(n, 1), dtype=np.int32)
        rn = np.zeros(max(n, 1))
        if n:
            basis.pre_call()
            _lib.check(basis.lib.dftk_mi_refinement_metric_solve(kpt.handle, n, psik.data_ptr(), psik.stride(0), resk.data_ptr(),
                                                                 resk.stride(0), float(tol), int(maxiter), x.data_ptr(),
                                                                 x.stride(0), iters.ctypes.data, rn.ctypes.data))
            basis.post_call(kpt.lane)
            bad = np.nonzero(rn[:n] > tol)[0]
            if len(bad):
                warnings.warn(f"CG for `invert_refinement_metric` did not converge at k-point {ik}, this is unexpected.  "
                              f"Residual norm after {int(iters[bad].max())} iterations is {float(rn[bad].max()):.3e}.")
        out.append(x)
    return out


# ------------------------------------------------------------------------------------------ driver
@dataclass
class RefinementResult:
    """refine.jl:86-105.  ``basis``: the refinement basis; ``psi``, ``rho``, ``occupation``: the SCF result transferred to it,
    virtual orbitals removed; ``dpsi``, ``drho``: the first-order corrections (refined quantities are psi + dpsi and
    rho + drho); ``OmegaPlusK_res``: what the inversion of (Omega + K) on the small basis returned, without its dpsi."""
    basis: object
    psi: list
    rho: torch.Tensor
    occupation: list
    dpsi: list
    drho: torch.Tensor
    OmegaPlusK_res: dict


def refine_scfres(scfres, basis_ref, tol=1e-6, occ_threshold=EPS, **kw):
    """``refine_scfres(scfres, basis_ref; tol, occ_threshold, kwargs...)`` (refine.jl:116-167).  ``tol`` and the further
    keywords go to ``solve_OmegaPlusK_split`` on the basis of ``scfres``."""
    basis = scfres["basis"]
    check_supported(basis)
    check_supported(basis_ref)
    check_same_lattice(basis, basis_ref, "refine_scfres")
    check_same_kpoints(basis, basis_ref, "refine_scfres")
    if basis.model.temperature != 0 or basis_ref.model.temperature != 0:
        raise ValueError("refine_scfres: only full occupations are supported (the model has a temperature)")
    # virtual orbitals must be removed
    psi, occ = select_occupied_orbitals(basis, scfres["psi"], scfres["occupation"], threshold=occ_threshold)
    check_full_occupation(basis, occ)
    _check_contains(basis, basis_ref)
    basis._require_gpu()
    basis_ref._require_gpu()
    psi = [p.contiguous() for p in psi]

    psir = transfer_blochwave(psi, basis, basis_ref)
    rhor = transfer_density(scfres["rho"], basis, basis_ref)
    _, hamr = energy_hamiltonian(basis_ref, psir, occ, rho=rhor)

    # minus the residual, -R(P); its low- and high-frequency parts
    res = [-g for g in compute_projected_gradient(basis_ref, psir, occ)]
    resLF = transfer_blochwave(res, basis_ref, basis)
    resHF = [r - x for r, x in zip(res, transfer_blochwave(resLF, basis, basis_ref))]

    # -M_22^-1 R_2(P) as an approximation of -(Omega + K)_22^-1 R_2(P)
    e2 = invert_refinement_metric(basis_ref, psir, resHF)

    # (Omega + K) applied to it, brought down to the small basis
    Lambda = rayleigh_coefficients(hamr, psir)
    OpKe2 = [a + b for a, b in zip(apply_Omega(e2, psir, hamr, Lambda), apply_K(basis_ref, e2, psir, rhor, occ))]
    OpKe2 = transfer_blochwave(OpKe2, basis_ref, basis)
    rhs = [a - b for a, b in zip(OpKe2, resLF)]

    # (Omega + K) e1 = -rhs on the small basis: rhs takes the place of dH_ext psi; the extra bands of scfres get no
    # right-hand side and no response
    dHext = []
    for psik_all, r in zip(scfres["psi"], rhs):
        full = torch.zeros_like(psik_all)
        full[:r.shape[0]] = r
        dHext.append(full)
    OpK_res = solve_OmegaPlusK_split(scfres, dHext, tol=tol, **kw)
    e1 = transfer_blochwave([d[:p.shape[0]].contiguous() for d, p in zip(OpK_res["dpsi"], psi)], basis, basis_ref)
    dpsi = [a + b for a, b in zip(e1, e2)]

    drho = compute_delta_rho(basis_ref, psir, dpsi, occ)
    OpK_res = {k: v for k, v in OpK_res.items() if k != "dpsi"}
    return RefinementResult(basis_ref, psir, rhor, occ, dpsi, drho, OpK_res)


# ------------------------------------------------------------------------------------------ refined quantities
def refine_energies(refinement):
    """``refine_energies(refinement)`` (refine.jl:174-183): ``{"E": Energies, "dE": Energies}``, E the energies of
    (psi, rho) on the refinement basis and dE, term by term, the derivative of ``energy(basis, psi + eps dpsi, occupation;
    rho = rho + eps drho)`` at eps = 0, written out: 2 Re <dpsi|T|psi> sums for Kinetic and AtomicNonlocal, int V drho for
    AtomicLocal, Hartree and Xc (V the term's potential at rho, with a core correction at rho + rho_core), zero for the
    terms that depend on neither."""
    from .eigen import columnwise_dots
    from .terms import _local_potential_call
    basis, psi, occ = refinement.basis, refinement.psi, refinement.occupation
    rho, dpsi, drho = refinement.rho, refinement.dpsi, refinement.drho
    basis._require_gpu()
    T = basis.terms
    with basis.on_library_stream():
        E, ham = energy_hamiltonian(basis, psi, occ, rho=rho)
        dE = Energies()
        drho_t = total_density(drho)
        for name in T.names:
            if name in ("Kinetic", "AtomicNonlocal"):
                which = 2 if name == "Kinetic" else 4
                acc = 0.0
                if not (name == "AtomicNonlocal" and T.P is None):
                    for ik, (Hk, p, d) in enumerate(zip(ham, psi, dpsi)):
                        Tp = Hk.mul_(torch.empty_like(p), p.contiguous(), which=which)
                        dots = columnwise_dots(basis, d.contiguous(), Tp).real
                        acc += basis.kweights[ik] * float(np.sum(np.asarray(occ[ik], dtype=float) * 2.0 * dots))
                dE[name] = acc
            elif name == "AtomicLocal":
                dE[name] = float((T.V_loc * drho_t).sum().item()) * basis.dvol
            elif name == "Hartree":
                dE[name] = float((apply_kernel(basis, total_density(rho), rho, RPA=True) * drho_t).sum().item()) * basis.dvol
            elif name == "Xc":
                vxc = _local_potential_call(basis, rho, basis.model.functionals, False, want_potential=True,
                                            want_energies=False)["V"]
                dE[name] = float((vxc * drho_t).sum().item()) * basis.dvol
            else:                                   # Ewald, PspCorrection, Entropy (T = 0): no orbital or density dependence
                dE[name] = 0.0
        basis.sync()
    return {"E": E, "dE": dE}


def refine_forces(refinement):
    """``refine_forces(refinement)`` (refine.jl:190-203): ``(F, dF)`` in reduced coordinates, F the forces of (psi, rho) on the
    refinement basis and dF the derivative of ``compute_forces(basis, psi + eps dpsi, occupation; rho = rho + eps drho)`` at
    eps = 0: the local term is linear in rho (``dftk_mi_forces_local(_table)`` on drho), the nonlocal term comes from the
    ``dforces`` output of ``dftk_mi_dynmat_nonlocal``, and with a non-linear core correction the Xc force of the potential
    change f_xc drho.  dF is symmetrised like F."""
    from .forces import _forces_local, _forces_xc_of_potential, compute_forces
    from .phonon import _dynmat_nonlocal
    from .symmetry import symmetrize_forces
    from .terms import model_uses_nlcc
    basis, psi, occ = refinement.basis, refinement.psi, refinement.occupation
    rho, dpsi, drho = refinement.rho, refinement.dpsi, refinement.drho
    basis._require_gpu()
    model = basis.model
    F = compute_forces(basis, psi, occ, rho=rho)
    dF = np.zeros_like(F)
    with basis.on_library_stream():
        if "AtomicLocal" in model.term_types:
            dF += _forces_local(basis, drho)
        if "AtomicNonlocal" in model.term_types and basis.terms.P is not None:
            zeros = [np.zeros(len(o)) for o in occ]
            df, _ = _dynmat_nonlocal(basis, [p.contiguous() for p in psi], occ, dpsi=[d.contiguous() for d in dpsi],
                                     doccupation=zeros)
            dF += symmetrize_forces(basis, df)
        if "Xc" in model.term_types and model_uses_nlcc(model):
            dvxc = apply_kernel(basis, total_density(drho), rho) - apply_kernel(basis, total_density(drho), rho, RPA=True)
            dF += _forces_xc_of_potential(basis, dvxc.contiguous())
        basis.sync()
    return F, dF
