"""The dynamical matrix and the phonon modes at q = 0 (src/postprocess/phonon.jl: ``compute_dynmat``, ``phonon_modes``,
``compute_δHψ_αs``; spelled ``compute_delta_H_psi_alpha_s`` here, ASCII as in response.py).

In reduced coordinates ``D[beta, t, alpha, s] = d^2 E / dR_{t,beta} dR_{s,alpha} = -dF_{t,beta} / dR_{s,alpha}``.  Only the
terms whose forces depend explicitly on the density or the orbitals contribute (local.jl:183-213, nonlocal.jl:307-383,
ewald.jl:181-251); Hartree, Xc, Kinetic, Entropy and PspCorrection enter through the response to the displacement, which
``solve_OmegaPlusK_split`` gives for every (alpha, s):

* Ewald: the Hessian of the Ewald energy, analytic on the host (``terms.dynmat_ewald``).
* AtomicLocal: ``-F_loc[d_rho]`` (``dftk_mi_forces_local`` is linear in the density) plus, for s = t, the second
  derivative of the local energy at fixed density (``dftk_mi_dynmat_local``).
* AtomicNonlocal: minus the derivative of ``dftk_mi_forces_nonlocal`` along (d_psi, d_occupation) plus, for s = t,
  ``sum_nk w_nk <psi| d_alpha d_beta (P_s D_s P_s') |psi>`` (both ``dftk_mi_dynmat_nonlocal``).

The perturbation itself is ``dV_{alpha,s} psi`` (``dftk_mi_local_potential_displacement`` and the local apply) plus the
nonlocal ``d(P_s D_s P_s') / dR_{s,alpha} psi`` (``dftk_mi_nonlocal_displacement_apply``: the three alpha of one atom in
one call per k-point).  Scope: q = 0, no spin, LDA kernels, HGH pseudopotentials, one rank, a basis without symmetries;
everything else is refused by these entry points (the response layer's own refusals are untouched).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .forces import _forces_local, _group_order, _projector_col_start
from .terms import dynmat_ewald, local_species_tables

_NO_DYNMAT = ("Kinetic", "Hartree", "Xc", "PspCorrection", "Entropy")


# ------------------------------------------------------------------------------------------ checks
def _check_supported(basis, q=None):
    from .exchange import refuse
    from .model import refuse_meta_gga
    model = basis.model
    refuse_meta_gga(model, "the dynamical matrix (compute_dynmat)")
    refuse(model, "the dynamical matrix (no response with the Fock operator)")
    from .hubbard import refuse as refuse_hubbard
    refuse_hubbard(model, "the dynamical matrix")
    from .psp_upf import refuse_upf
    refuse_upf(model, "the dynamical matrix and the displacement perturbation")
    if q is not None and np.any(np.asarray(q, dtype=float) != 0):
        raise NotImplementedError("phonons at q != 0 are not implemented: q = 0 only")
    if model.n_spin_components != 1:
        raise NotImplementedError("the dynamical matrix with collinear spin is not implemented")
    if basis.comm_pw.size > 1:
        raise NotImplementedError("the dynamical matrix of a basis whose plane waves are sharded over comm_pw is not "
                                  "implemented")
    if basis.comm_kpts.size > 1:
        raise NotImplementedError("the dynamical matrix of a basis whose k-points are spread over comm_kpts is not "
                                  "implemented")
    if any(not s.isone() for s in basis.symmetries):
        raise ValueError("the dynamical matrix needs a basis without symmetries (a displacement breaks them, and "
                         "apply_chi0 symmetrises with the group of the basis): build the model with symmetries=False")


# ------------------------------------------------------------------------------------------ the perturbation
def _delta_V_atom(basis, s):
    """The three cubes d V_loc / d R_{s,alpha} (``dftk_mi_local_potential_displacement``), shape (3, nz, ny, nx)."""
    model = basis.model
    par, _, _ = local_species_tables(model)
    species = next(i for i, g in enumerate(model.atom_groups) if s in g)
    Bh = np.asfortranarray(model.recip_lattice, dtype=np.float64)
    pos = np.ascontiguousarray(model.positions[s], dtype=np.float64)
    nx, ny, nz = basis.fft_size
    out = torch.empty((3, nz, ny, nx), dtype=torch.float64, device=basis.device)
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_local_potential_displacement(basis._cube_handle, Bh.ctypes.data, par.shape[0],
                                                              par.ctypes.data, species, pos.ctypes.data, out.data_ptr()))
    basis.post_call(0)
    return out


def _delta_H_psi_atom(basis, psi, s):
    """``[[dH_{alpha,s} psi_k for k] for alpha]``: the three perturbations of atom ``s`` (``model.atoms`` order), the
    nonlocal parts of one k-point in one library call."""
    from .response import multiply_psi_by_potential
    model = basis.model
    T = basis.terms
    names = model.term_types
    out = [[torch.zeros_like(p) for p in psi] for _ in range(3)]
    if "AtomicNonlocal" in names and T is not None and T.P is not None:
        col_start = _projector_col_start(model)
        atom = _group_order(model).index(s)
        n_atoms = len(model.atoms)

        def one(ik, psik):
            kpt = basis.kpoints[ik]
            kh = np.ascontiguousarray(kpt.coordinate, dtype=np.float64)
            nb = psik.shape[0]
            buf = torch.empty((3, nb, psik.shape[1]), dtype=torch.complex128, device=psik.device)
            basis.pre_call()
            _lib.check(basis.lib.dftk_mi_nonlocal_displacement_apply(kpt.handle, kh.ctypes.data, atom, n_atoms,
                                                                     col_start.ctypes.data, nb, psik.data_ptr(),
                                                                     psik.stride(0), buf.data_ptr(), buf.stride(1)))
            basis.post_call(kpt.lane)
            return buf
        for ik, buf in enumerate(basis.run_on_lanes(one, psi)):
            for al in range(3):
                out[al][ik] = buf[al]
    if "AtomicLocal" in names:
        dV = _delta_V_atom(basis, s)
        for al in range(3):
            for ik, x in enumerate(multiply_psi_by_potential(basis, psi, dV[al])):
                out[al][ik] = out[al][ik] + x
    return out


def compute_delta_H_psi_alpha_s(basis, psi, alpha, s, q=None):
    """``compute_δHψ_αs(basis, ψ, α, s, q)`` (phonon.jl:96-107): the products of the orbitals with the change of the
    Hamiltonian when atom ``s`` moves along the reduced direction ``alpha``, one block per k-point."""
    _check_supported(basis, q)
    basis._require_gpu()
    if not (0 <= int(alpha) < 3 and 0 <= int(s) < len(basis.model.atoms)):
        raise ValueError("compute_delta_H_psi_alpha_s: alpha in 0..2 and s an atom index")
    with basis.on_library_stream():
        out = _delta_H_psi_atom(basis, psi, int(s))[int(alpha)]
        basis.sync()
    return out


# ------------------------------------------------------------------------------------------ the terms
def _dynmat_nonlocal(basis, psi, occupation, dpsi=None, doccupation=None, hess=False):
    """``(dforces, hess)`` of ``dftk_mi_dynmat_nonlocal`` summed over the k-points, atoms in ``model.atoms`` order:
    dforces (n_atoms, 3) along (dpsi, doccupation), or None; hess (n_atoms, 3, 3) indexed [a, beta, alpha], or None."""
    model = basis.model
    n_atoms = len(model.atoms)
    order = _group_order(model)
    col_start = _projector_col_start(model)

    def one(ik, psik):
        kpt = basis.kpoints[ik]
        nb = psik.shape[0]
        occ = np.asarray(occupation[ik], dtype=float)[:nb]
        w = np.ascontiguousarray(basis.kweights[ik] * occ, dtype=np.float64)
        df = np.zeros((n_atoms, 3))
        hs = np.zeros((n_atoms, 3, 3))
        kh = np.ascontiguousarray(kpt.coordinate, dtype=np.float64)
        dp, wd = None, None
        if dpsi is not None:
            dp = dpsi[ik]
            wd = np.ascontiguousarray(basis.kweights[ik] * np.asarray(doccupation[ik], dtype=float)[:nb], dtype=np.float64)
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_dynmat_nonlocal(kpt.handle, kh.ctypes.data, nb, psik.data_ptr(), psik.stride(0),
                                                     dp.data_ptr() if dp is not None else None,
                                                     dp.stride(0) if dp is not None else 0, w.ctypes.data,
                                                     wd.ctypes.data if wd is not None else None, n_atoms,
                                                     col_start.ctypes.data, df.ctypes.data if dp is not None else None,
                                                     hs.ctypes.data if hess else None))
        return df, hs

    parts = basis.run_on_lanes(one, psi)
    df_g = sum(p[0] for p in parts)
    hs_g = sum(p[1] for p in parts)
    df = np.zeros((n_atoms, 3))
    hs = np.zeros((n_atoms, 3, 3))
    df[order] = df_g
    hs[order] = hs_g
    return (df if dpsi is not None else None), (hs if hess else None)


def _dynmat_local_explicit(basis, rho):
    """d^2 E_loc / dR_{a,beta} dR_{a,alpha} at fixed density (``dftk_mi_dynmat_local``), (n_atoms, 3, 3) [a, beta, alpha]."""
    from .terms import total_density
    model = basis.model
    order = _group_order(model)
    par, species, positions = local_species_tables(model)
    Bh = np.asfortranarray(model.recip_lattice, dtype=np.float64)
    rho_tot = total_density(rho).to(torch.float64).contiguous()
    out = np.zeros((len(order), 3, 3))
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_dynmat_local(basis._cube_handle, Bh.ctypes.data, par.shape[0], par.ctypes.data, len(order),
                                              species.ctypes.data, positions.ctypes.data, rho_tot.data_ptr(),
                                              out.ctypes.data))
    H = np.zeros_like(out)
    H[order] = out
    return H


def compute_dynmat_term(name, basis, psi, occupation, *, rho=None, dpsis=None, drhos=None, doccupations=None, q=None):
    """``compute_dynmat(term, basis, ψ, occupation; ρ, δψs, δρs, δoccupations)`` for the term named ``name``: a real
    (3, n_atoms, 3, n_atoms) array in reduced coordinates, or None for terms that enter through the response only.
    ``dpsis[alpha][s]`` / ``drhos[alpha][s]`` / ``doccupations[alpha][s]``: the response to the displacement (alpha, s)."""
    _check_supported(basis, q)
    model = basis.model
    n = len(model.atoms)
    if name not in model.term_types:
        raise ValueError(f"term {name} is not part of the model")
    if name in _NO_DYNMAT:
        return None
    if name == "Ewald":
        return dynmat_ewald(model.lattice, [a.charge_ionic for a in model.atoms], model.positions)
    basis._require_gpu()
    D = np.zeros((3, n, 3, n))
    with basis.on_library_stream():
        if name == "AtomicLocal":
            if rho is None or drhos is None:
                raise ValueError("the AtomicLocal dynamical matrix needs the density and its responses")
            H = _dynmat_local_explicit(basis, rho)
            for s in range(n):
                D[:, s, :, s] += H[s]
                for al in range(3):
                    D[:, :, al, s] -= _forces_local(basis, drhos[al][s]).T
            return D
        if name == "AtomicNonlocal":
            if basis.terms is None or basis.terms.P is None:
                return D
            if dpsis is None or doccupations is None:
                raise ValueError("the AtomicNonlocal dynamical matrix needs the orbital and occupation responses")
            _, H = _dynmat_nonlocal(basis, psi, occupation, hess=True)
            for s in range(n):
                D[:, s, :, s] += H[s]
                for al in range(3):
                    dF, _ = _dynmat_nonlocal(basis, psi, occupation, dpsis[al][s], doccupations[al][s])
                    D[:, :, al, s] -= dF.T
            return D
    raise NotImplementedError(f"the dynamical matrix of term {name} is outside the MI355X hot path")


def compute_dynmat(basis_or_scfres, psi=None, occupation=None, *, rho=None, ham=None, eF=None, eigenvalues=None,
                   occupation_threshold=None, tol=1e-8, q=None, return_responses=False, **kw_response):
    """``compute_dynmat(scfres; tol, ...)`` / ``compute_dynmat(basis, ψ, occupation; ρ, ham, εF, eigenvalues, ...)``
    (phonon.jl:14-58) at q = 0: the real (3, n_atoms, 3, n_atoms) dynamical matrix in reduced coordinates, ``model.atoms``
    order.  One ``solve_OmegaPlusK_split`` (tolerance ``tol``; further keywords such as ``RPA`` are passed on) per
    displacement.  ``return_responses``: also the dict of responses ``compute_dynmat_term`` takes."""
    from .response import solve_OmegaPlusK_split
    if isinstance(basis_or_scfres, dict):
        res = basis_or_scfres
    else:
        res = dict(basis=basis_or_scfres, psi=psi, occupation=occupation, rho=rho, ham=ham, eF=eF, eigenvalues=eigenvalues,
                   occupation_threshold=occupation_threshold)
    basis = res["basis"]
    _check_supported(basis, q)
    basis._require_gpu()
    missing = [k for k in ("psi", "occupation", "rho", "ham", "eF", "eigenvalues", "occupation_threshold")
               if res.get(k) is None]
    if missing:
        raise ValueError(f"compute_dynmat: missing {', '.join(missing)}")
    model = basis.model
    n = len(model.atoms)
    psi_, occ_ = res["psi"], res["occupation"]
    dpsis = [[None] * n for _ in range(3)]
    drhos = [[None] * n for _ in range(3)]
    doccs = [[None] * n for _ in range(3)]
    for s in range(n):
        with basis.on_library_stream():
            dH = _delta_H_psi_atom(basis, psi_, s)
        for al in range(3):
            r = solve_OmegaPlusK_split(res, dH[al], tol=tol, **kw_response)
            dpsis[al][s], drhos[al][s], doccs[al][s] = r["dpsi"], r["drho"], r["doccupation"]
    responses = dict(dpsis=dpsis, drhos=drhos, doccupations=doccs)
    D = np.zeros((3, n, 3, n))
    for name in model.term_types:
        d = compute_dynmat_term(name, basis, psi_, occ_, rho=res["rho"], **responses)
        if d is not None:
            D += d
    return (D, responses) if return_responses else D


# ------------------------------------------------------------------------------------------ modes
def dynmat_red_to_cart(lattice, dynmat):
    """``dynmat_red_to_cart`` (phonon.jl:2-12): both displacement indices are covectors,
    ``D_cart[:, t, :, s] = inv(L') D_red[:, t, :, s] inv(L)``."""
    inv_l = np.linalg.inv(np.asarray(lattice, dtype=float))
    return np.einsum("ib,btas,aj->itjs", inv_l.T, np.asarray(dynmat, dtype=float), inv_l)


def mass_matrix(model_or_atoms, masses=None):
    """The diagonal (3 n_atoms, 3 n_atoms) mass matrix in atomic units (phonon.jl:60-70).  ``masses``: one mass per atom,
    or a dict symbol -> mass that overrides ``ElementPsp.mass`` (the standard atomic weight) for those elements."""
    atoms = list(getattr(model_or_atoms, "atoms", model_or_atoms))
    if masses is not None and not isinstance(masses, dict):
        m = np.asarray(masses, dtype=float).reshape(-1)
        if len(m) != len(atoms):
            raise ValueError("mass_matrix: one mass per atom")
    else:
        m = np.zeros(len(atoms))
        for i, a in enumerate(atoms):
            mi = (masses or {}).get(a.symbol, getattr(a, "mass", None))
            if mi is None:
                raise ValueError(f"mass_matrix: no mass known for {a.symbol}: pass masses=")
            m[i] = float(mi)
    if np.any(m <= 0):
        raise ValueError("mass_matrix: masses must be positive")
    return np.diag(np.repeat(m, 3))


def _modes(dynmat_cart, M):
    """Frequencies and vectors of ``D v = lambda M v`` (phonon.jl:72-84): ``sign(lambda) sqrt(|lambda|)``; D is
    (3, n, 3, n), the matrix index is 3 * atom + direction; the vectors are M-orthonormal."""
    n3 = M.shape[0]
    Dm = np.asarray(dynmat_cart, dtype=float).transpose(1, 0, 3, 2).reshape(n3, n3)
    Dm = (Dm + Dm.T) / 2
    isq = 1.0 / np.sqrt(np.diag(M))
    lam, u = np.linalg.eigh(isq[:, None] * Dm * isq[None, :])
    return np.sign(lam) * np.sqrt(np.abs(lam)), isq[:, None] * u


def phonon_modes(scfres_or_basis, *args, masses=None, dynmat=None, **kw):
    """``phonon_modes(scfres; kwargs...)`` (phonon.jl:72-94): ``dict(mass_matrix, frequencies, dynmat, dynmat_cart,
    vectors, vectors_cart)``.  Frequencies in atomic units, ascending, negative for unstable modes; ``vectors_cart[:, i]``
    the Cartesian displacement pattern of mode i (index 3 * atom + direction), ``vectors`` the same in reduced coordinates.
    ``dynmat``: a reduced dynamical matrix computed before (else ``compute_dynmat`` with the remaining arguments)."""
    basis = scfres_or_basis["basis"] if isinstance(scfres_or_basis, dict) else scfres_or_basis
    model = basis.model
    M = mass_matrix(model, masses)
    if dynmat is None:
        dynmat = compute_dynmat(scfres_or_basis, *args, **kw)
    dynmat = np.asarray(dynmat, dtype=float)
    dcart = dynmat_red_to_cart(model.lattice, dynmat)
    freq, vcart = _modes(dcart, M)
    n = len(model.atoms)
    inv_l = np.linalg.inv(model.lattice)
    vred = np.einsum("ij,ajm->aim", inv_l, vcart.reshape(n, 3, -1)).reshape(3 * n, -1)       # vector_cart_to_red
    return dict(mass_matrix=M, frequencies=freq, dynmat=dynmat, dynmat_cart=dcart, vectors=vred, vectors_cart=vcart)
