"""The stress tensor after an SCF (src/postprocess/stresses.jl): sigma = (1 / Omega) dE[(I + eps) L] / d eps at eps = 0 with
the orbital coefficients, occupations and eigenvalues held fixed and the density recomputed from the orbitals, in
Cartesian coordinates (Hartree / bohr^3), symmetrised over ``basis.symmetries``.  The reference differentiates the energy
with dual numbers; here every term's derivative is written out and evaluated by the library's stress kernels
(stress_kernels.hip): Kinetic and AtomicNonlocal per k-block, AtomicLocal and Hartree in one pass over the cube, Xc from
the point-wise kernels plus one reduction.  Ewald and PspCorrection are analytic on the host; Entropy does not depend on
the lattice at fixed occupations.  There is no torch fall-back: a basis without the library raises."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .forces import _check_nlcc
from .hubbard import refuse as refuse_hubbard
from .psp_upf import refuse_upf
from .symmetry import symmetrize_stresses
from .terms import (_DENSITY_THRESHOLD, _GGA_BITS, _LDA_BITS, _SPIN_LDA, local_species_tables, occupied_block,
                    projector_species_tables, stress_ewald, total_density)


# ------------------------------------------------------------------------------------------ Voigt notation
def voigt_stress_to_full(v):
    """stresses.jl:56-60; Voigt order [xx, yy, zz, zy, zx, yx]."""
    v = np.asarray(v, dtype=float)
    return np.array([[v[0], v[5], v[4]], [v[5], v[1], v[3]], [v[4], v[3], v[2]]])


def full_stress_to_voigt(s):
    """stresses.jl:61-66."""
    s = np.asarray(s, dtype=float)
    return np.array([s[0, 0], s[1, 1], s[2, 2], (s[2, 1] + s[1, 2]) / 2, (s[2, 0] + s[0, 2]) / 2, (s[0, 1] + s[1, 0]) / 2])


def voigt_strain_to_full(v):
    """stresses.jl:67-71: the deformation I + eps (the zero vector gives the identity)."""
    v = np.asarray(v, dtype=float)
    return np.array([[1 + v[0], v[5] / 2, v[4] / 2], [v[5] / 2, 1 + v[1], v[3] / 2], [v[4] / 2, v[3] / 2, 1 + v[2]]])


def full_strain_to_voigt(e):
    """stresses.jl:72-77."""
    e = np.asarray(e, dtype=float)
    return np.array([e[0, 0] - 1, e[1, 1] - 1, e[2, 2] - 1, e[2, 1] + e[1, 2], e[2, 0] + e[0, 2], e[0, 1] + e[1, 0]])


# ------------------------------------------------------------------------------------------ device terms
_projector_tables = projector_species_tables      # (the name this module had for it; tests import it from here)


def _check_unsharded(basis):
    from .exchange import refuse
    refuse(basis.model, "the stress tensor (no exact-exchange stress term)")
    if basis.comm_pw.size > 1:
        raise NotImplementedError("stresses of a basis whose plane waves are sharded over comm_pw are not implemented")


def _kinetic_nonlocal(basis, psi, occupation):
    """(sigma_kinetic, sigma_nonlocal): ``dftk_mi_stress_kinetic_nonlocal`` per k-block, partial sums of the k-points of
    this rank reduced over ``comm_kpts`` like the forces."""
    model = basis.model
    T = basis.terms
    have_P = T is not None and T.P is not None
    n_species, rp, nproj, species, positions, col_start = projector_species_tables(model)
    if not have_P:
        n_species, species, col_start = 0, species[:0], col_start[:1]
    n_atoms = len(species)
    Bh = np.asfortranarray(model.recip_lattice, dtype=np.float64)

    def one(ik, psik):
        kpt = basis.kpoints[ik]
        out = np.zeros(12)
        block = occupied_block(basis, ik, psik, occupation)
        if block is None:
            return out
        ps, w = block
        kh = np.ascontiguousarray(kpt.coordinate, dtype=np.float64)
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_stress_kinetic_nonlocal(
            kpt.handle, Bh.ctypes.data, kh.ctypes.data, len(w), ps.data_ptr(), ps.stride(0), w.ctypes.data, n_species,
            rp.ctypes.data, nproj.ctypes.data, n_atoms, species.ctypes.data if n_atoms else None,
            positions.ctypes.data if n_atoms else None, col_start.ctypes.data, out.ctypes.data))
        return out

    parts = basis.run_on_lanes(one, psi)
    tot = np.zeros(12)
    for p in parts:
        tot += p
    if basis.comm_kpts.size > 1:
        tot = np.asarray(basis.comm_kpts.sum_scalars(tot.tolist()))
    vol = model.unit_cell_volume
    return voigt_stress_to_full(tot[:6]) / vol, voigt_stress_to_full(tot[6:]) / vol


def _local_hartree(basis, rho):
    """(sigma_local, sigma_hartree) from one ``dftk_mi_stress_cube`` call."""
    model = basis.model
    par, species, positions = local_species_tables(model)
    n_atoms = len(species) if "AtomicLocal" in model.term_types else 0
    Bh = np.asfortranarray(model.recip_lattice, dtype=np.float64)
    rho_tot = total_density(rho).to(torch.float64).contiguous()
    out = np.zeros(14)
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_stress_cube(basis._cube_handle, Bh.ctypes.data, par.shape[0], par.ctypes.data, n_atoms,
                                             species.ctypes.data, positions.ctypes.data, rho_tot.data_ptr(),
                                             out.ctypes.data))
    vol = model.unit_cell_volume
    eye = np.eye(3)
    return ((voigt_stress_to_full(out[:6]) - out[12] * eye) / vol, (voigt_stress_to_full(out[6:12]) - out[13] * eye) / vol)


def _xc(basis, rho):
    """delta_ab (E_xc - int v_rho rho - 2 int v_sigma sigma) - 2 int v_sigma grad_a rho grad_b rho, all over Omega:
    e / v_rho / v_sigma from the library's point-wise kernels, the sums from ``dftk_mi_stress_xc``."""
    model = basis.model
    lda = sum(_LDA_BITS[f] for f in model.functionals if f in _LDA_BITS)
    gga = sum(_GGA_BITS[f] for f in model.functionals if f in _GGA_BITS)
    unknown = [f for f in model.functionals if f not in _LDA_BITS and f not in _GGA_BITS]
    if unknown:
        raise NotImplementedError(f"XC functionals {unknown}: LDA and PBE are on this path")
    rho = rho.to(torch.float64).contiguous()
    n_spin = 2 if rho.dim() == 4 else 1
    n = rho.numel() // n_spin
    out = np.zeros(8)
    E = 0.0
    if n_spin == 2:
        if any(f not in _SPIN_LDA for f in model.functionals):
            raise NotImplementedError(f"collinear spin: spin-polarised forms exist for {_SPIN_LDA} only, got "
                                      f"{model.functionals}")
        if lda:
            V = torch.empty_like(rho)
            E3 = (C.c_double * 3)()
            basis.pre_call()
            _lib.check(basis.lib.dftk_mi_local_potential_collinear(basis._cube_handle, rho.data_ptr(), None, None, lda,
                                                                   V.data_ptr(), E3))
            E = E3[1]
            _lib.check(basis.lib.dftk_mi_stress_xc(basis.handle, n, 2, rho.data_ptr(), V.data_ptr(), None, None, None,
                                                   out.ctypes.data))
    elif lda or gga:
        vrho = torch.zeros_like(rho)
        if lda:
            E3 = (C.c_double * 3)()
            basis.pre_call()
            _lib.check(basis.lib.dftk_mi_local_potential(basis._cube_handle, rho.data_ptr(), None, None, lda,
                                                         vrho.data_ptr(), E3))
            E = E3[1]
        eg = vsig = grad = None
        if gga:
            # grad rho exactly as the GGA potential takes it (xc_energy_potential): i G multipliers between cube FFTs
            G = basis.G_vectors_cart_cube()
            rho_f = basis.fft(rho)
            grad = torch.stack([basis.irfft(1j * G[..., a] * rho_f) for a in range(3)]).contiguous()
            sigma = (grad * grad).sum(dim=0).contiguous()
            eg, vr, vsig = torch.empty_like(rho), torch.empty_like(rho), torch.empty_like(rho)
            basis.pre_call()
            _lib.check(basis.lib.dftk_mi_xc_gga(basis.handle, n, rho.data_ptr(), sigma.data_ptr(), gga, _DENSITY_THRESHOLD,
                                                eg.data_ptr(), vr.data_ptr(), vsig.data_ptr()))
            vrho = vrho + vr
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_stress_xc(basis.handle, n, 1, rho.data_ptr(), vrho.data_ptr(),
                                               eg.data_ptr() if gga else None, vsig.data_ptr() if gga else None,
                                               grad.data_ptr() if gga else None, out.ctypes.data))
    out *= basis.dvol
    E += out[0]
    vv = voigt_stress_to_full(out[2:8])
    return (np.eye(3) * (E - out[1] - 2 * np.trace(vv)) - 2 * vv) / model.unit_cell_volume


def _device_terms(basis, psi, occupation, rho, names):
    """The device terms among ``names`` with shared passes run once: {name: (3, 3)}."""
    basis._require_gpu()
    _check_unsharded(basis)
    out = {}
    with basis.on_library_stream():
        if "Kinetic" in names or "AtomicNonlocal" in names:
            out["Kinetic"], out["AtomicNonlocal"] = _kinetic_nonlocal(basis, psi, occupation)
        if "AtomicLocal" in names or "Hartree" in names:
            if rho is None:
                raise ValueError("AtomicLocal and Hartree stresses need the density")
            out["AtomicLocal"], out["Hartree"] = _local_hartree(basis, rho)
        if "Xc" in names:
            if rho is None:
                raise ValueError("Xc stresses need the density")
            _check_nlcc(basis.model)
            out["Xc"] = _xc(basis, rho)
    return out


_DEVICE_TERMS = ("Kinetic", "AtomicNonlocal", "AtomicLocal", "Hartree", "Xc")


def _host_term(name, basis):
    model = basis.model
    T = basis.terms
    if name == "Ewald":
        # computed on the first stress call (not at set-up), then kept like F_ewald
        if getattr(T, "S_ewald", None) is None:
            T.S_ewald = stress_ewald(model.lattice, [a.charge_ionic for a in model.atoms], model.positions)
        return T.S_ewald.copy()
    if name == "PspCorrection":
        return -T.E_pspcorr / model.unit_cell_volume * np.eye(3)
    raise NotImplementedError(f"stresses of term {name} are outside the MI355X hot path")


def compute_stresses_term(name, basis, psi, occupation, rho=None):
    """The UNSYMMETRISED (3, 3) Cartesian contribution of the term named ``name`` to the stress tensor, or None for
    Entropy (no lattice dependence at fixed occupations and eigenvalues).  ``rho`` must be the density of ``psi`` and
    ``occupation`` (the definition recomputes it from the orbitals)."""
    if name not in basis.model.term_types:
        raise ValueError(f"term {name} is not part of the model")
    refuse_hubbard(basis.model, "the stress tensor")
    refuse_upf(basis.model, "the stress tensor")
    if name == "Entropy":
        return None
    _check_unsharded(basis)
    if name in _DEVICE_TERMS:
        return _device_terms(basis, psi, occupation, rho, (name,))[name]
    return _host_term(name, basis)


def compute_stresses_cart(basis_or_scfres, psi=None, occupation=None, rho=None):
    """``compute_stresses_cart(scfres)`` / ``compute_stresses_cart(basis, psi, occupation; rho)`` (stresses.jl:30-55): the
    sum over the model's terms, symmetrised over ``basis.symmetries``; (3, 3) float64, Hartree / bohr^3."""
    if isinstance(basis_or_scfres, dict):
        res = basis_or_scfres
        basis, psi, occupation, rho = res["basis"], res["psi"], res["occupation"], res["rho"]
    else:
        basis = basis_or_scfres
    from .model import refuse_meta_gga
    refuse_meta_gga(basis.model, "the stress tensor (compute_stresses_cart; the reference has no meta-GGA stress either)")
    refuse_hubbard(basis.model, "the stress tensor")
    refuse_upf(basis.model, "the stress tensor")
    _check_unsharded(basis)
    names = [n for n in basis.model.term_types if n != "Entropy"]
    dev = _device_terms(basis, psi, occupation, rho, [n for n in names if n in _DEVICE_TERMS])
    total = np.zeros((3, 3))
    for name in names:
        total += dev[name] if name in _DEVICE_TERMS else _host_term(name, basis)
    return symmetrize_stresses(basis, total)
