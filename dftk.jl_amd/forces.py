"""Atomic forces after an SCF (src/postprocess/forces.jl): ``compute_forces`` sums ``compute_forces(term, ...)`` over the
model's terms and returns REDUCED-coordinate forces, one row per atom in ``model.atoms`` order; ``compute_forces_cart``
converts them with covector_red_to_cart, F_cart = inv(lattice') F_red (forces.jl:44-47).

Device terms (the library's force kernels, force_kernels.hip): AtomicLocal (local.jl:142-177, the exact derivative of the
local energy on the cube) and AtomicNonlocal (nonlocal.jl:49-98, one projector product per k-block, symmetrised as the
reference does).  Ewald (ewald.jl:24-31) is analytic on the host.  Kinetic, Hartree, PspCorrection and Entropy have no
explicit position dependence (terms.jl:85).  Xc (xc.jl:200-270) has one through the core densities of a non-linear core
correction alone: the AtomicLocal sum with (rho, ff_loc) replaced by (v_xc, ff_core), through the same kernel; without a
core density (HGH) the term has no forces.  There is no torch fall-back: a basis without the library raises."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .symmetry import symmetrize_forces
from .psp_upf import is_upf, model_has_upf
from .terms import (_local_potential_call, core_form_factor_table, energy_forces_ewald, local_form_factor_table,
                    local_species_tables, model_uses_nlcc, occupied_block, total_density)

# (ExactExchange: a functional of the orbitals alone, no explicit dependence on the positions)
_NO_FORCES = ("Kinetic", "Hartree", "PspCorrection", "Entropy", "ExactExchange")


def _group_order(model):
    """Atoms in species-group order (the order of the projector columns and of the local-term species table)."""
    return [ia for g in model.atom_groups for ia in g]


def _forces_local(basis, rho):
    model = basis.model
    order = _group_order(model)
    Bh = np.asfortranarray(model.recip_lattice, dtype=np.float64)
    rho_tot = total_density(rho).to(torch.float64).contiguous()
    out = np.zeros((len(order), 3))
    if model_has_upf(model):
        # a numeric local part: the form factors of every species as a device table (the one V_loc was built from)
        ff = local_form_factor_table(basis)
        _, species, positions = local_species_tables(model, lambda el: [])
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_forces_local_table(basis._cube_handle, Bh.ctypes.data, ff.shape[0], ff.data_ptr(),
                                                        len(order), species.ctypes.data, positions.ctypes.data,
                                                        rho_tot.data_ptr(), out.ctypes.data))
        F = np.zeros((len(model.atoms), 3))
        F[order] = out
        return F
    par, species, positions = local_species_tables(model)
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_forces_local(basis._cube_handle, Bh.ctypes.data, par.shape[0], par.ctypes.data,
                                              len(order), species.ctypes.data, positions.ctypes.data,
                                              rho_tot.data_ptr(), out.ctypes.data))
    F = np.zeros((len(model.atoms), 3))
    F[order] = out
    return F


def _projector_col_start(model):
    """Column offsets of every atom (group order) in P: groups without projectors own no columns."""
    starts = [0]
    for g in model.atom_groups:
        n = model.atoms[g[0]].psp.count_n_proj()
        for _ in g:
            starts.append(starts[-1] + n)
    return np.asarray(starts, dtype=np.int32)


def _forces_nonlocal(basis, psi, occupation):
    model = basis.model
    n_atoms = len(model.atoms)
    T = basis.terms
    if T is None or T.P is None:
        return np.zeros((n_atoms, 3))
    order = _group_order(model)
    col_start = _projector_col_start(model)

    def one(ik, psik):
        kpt = basis.kpoints[ik]
        out = np.zeros((n_atoms, 3))
        block = occupied_block(basis, ik, psik, occupation)
        if block is None:
            return out
        ps, w = block
        kh = np.ascontiguousarray(kpt.coordinate, dtype=np.float64)
        if getattr(T, "exx_kernel", None) is not None:
            # the projector slot may hold a compressed exchange operator behind P: the nonlocal term alone goes back in
            # (the Hamiltonian block that owns the slot re-binds on its next use)
            from .exchange import bind_projectors
            bind_projectors(basis, ik, None)
            kpt._exx_owner = None
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_forces_nonlocal(kpt.handle, kh.ctypes.data, len(w), ps.data_ptr(), ps.stride(0),
                                                     w.ctypes.data, n_atoms, col_start.ctypes.data, out.ctypes.data))
        return out

    parts = basis.run_on_lanes(one, psi)
    Fg = np.zeros((n_atoms, 3))
    for p in parts:
        Fg += p
    if basis.comm_kpts.size > 1:
        Fg = np.asarray(basis.comm_kpts.sum_scalars(Fg.reshape(-1).tolist())).reshape(n_atoms, 3)
    F = np.zeros((n_atoms, 3))
    F[order] = Fg
    return symmetrize_forces(basis, F)


def _check_nlcc(model):
    """Xc forces come from the core densities of UPF core channels (xc.jl:200-); a pseudopotential that claims a core
    density the library cannot evaluate, or that cannot say (no ``has_core_density``), is refused."""
    for el in model.atoms:
        has = getattr(el.psp, "has_core_density", None)
        if has is None or (has() and not is_upf(el.psp)):
            raise NotImplementedError(f"XC forces with a non-linear core correction ({el.symbol}) are not implemented "
                                      "for this pseudopotential (UPF core channels only)")


def _forces_xc(basis, rho):
    """xc.jl:200-270: F_a = -Re sum_G (-2 pi i G) conj(v_xc(G)) ff_core,s(|G|) e^{-2 pi i G.r_a} / sqrt(Omega), v_xc the
    XC potential alone (averaged over the channels of a collinear model) at rho + rho_core."""
    model = basis.model
    T = basis.terms
    out = _local_potential_call(basis, rho, model.functionals, False, want_potential=True, want_energies=False)
    if out is None:
        raise NotImplementedError(f"XC forces: the functionals {model.functionals} are not evaluated by the library")
    vxc = out["V"]
    for name, s in zip(model.functionals, getattr(model, "functional_scales", ())):
        if s != 1.0:                   # (a hybrid's scaled exchange part, as local_potential_fused takes it out)
            part = _local_potential_call(basis, rho, (name,), False, want_potential=True, want_energies=False)
            vxc.sub_(part["V"], alpha=1.0 - s)
    if vxc.dim() == 4:
        vxc = 0.5 * (vxc[0] + vxc[1])
    return _forces_xc_of_potential(basis, vxc.contiguous())


def _forces_xc_of_potential(basis, vxc):
    """The Xc force sum for a given potential cube: linear in ``vxc`` (refine.refine_forces hands it f_xc d_rho)."""
    model = basis.model
    T = basis.terms
    ff = T.core_ff if getattr(T, "core_ff", None) is not None else core_form_factor_table(basis)
    order = _group_order(model)
    _, species, positions = local_species_tables(model, lambda el: [])
    Bh = np.asfortranarray(model.recip_lattice, dtype=np.float64)
    res = np.zeros((len(order), 3))
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_forces_local_table(basis._cube_handle, Bh.ctypes.data, ff.shape[0], ff.data_ptr(),
                                                    len(order), species.ctypes.data, positions.ctypes.data,
                                                    vxc.data_ptr(), res.ctypes.data))
    F = np.zeros((len(model.atoms), 3))
    F[order] = res
    return symmetrize_forces(basis, F)


def compute_forces_term(name, basis, psi, occupation, rho=None):
    """``compute_forces(term, basis, psi, occupation; rho)`` for the term named ``name``: an (n_atoms, 3) array of
    reduced-coordinate forces, or None for terms without explicit position dependence."""
    model = basis.model
    from .hubbard import refuse as refuse_hubbard
    refuse_hubbard(model, "forces (the Hubbard term has no force yet: the sum of the other terms would be wrong)")
    if name not in model.term_types:
        raise ValueError(f"term {name} is not part of the model")
    if name in _NO_FORCES:
        return None
    if name == "Xc":
        _check_nlcc(model)
        if not model_uses_nlcc(model):
            return None
        if rho is None:
            raise ValueError("Xc forces need the density")
        basis._require_gpu()
        with basis.on_library_stream():
            return _forces_xc(basis, rho)
    if name == "Ewald":
        # computed on the first forces call (not at set-up: instantiate_terms and the SCF are unchanged), then kept
        T = basis.terms
        if getattr(T, "F_ewald", None) is None:
            T.F_ewald = energy_forces_ewald(model.lattice, [a.charge_ionic for a in model.atoms], model.positions)[1]
        return T.F_ewald.copy()
    basis._require_gpu()
    if name == "AtomicLocal":
        if rho is None:
            raise ValueError("AtomicLocal forces need the density")
        with basis.on_library_stream():
            return _forces_local(basis, rho)
    if name == "AtomicNonlocal":
        with basis.on_library_stream():
            return _forces_nonlocal(basis, psi, occupation)
    raise NotImplementedError(f"forces of term {name} are outside the MI355X hot path")


def compute_forces(basis_or_scfres, psi=None, occupation=None, rho=None):
    """``compute_forces(scfres)`` / ``compute_forces(basis, psi, occupation; rho)`` (forces.jl:23-36): the sum over the
    model's terms, (n_atoms, 3) float64 in reduced coordinates, ``model.atoms`` order."""
    if isinstance(basis_or_scfres, dict):
        res = basis_or_scfres
        basis, psi, occupation, rho = res["basis"], res["psi"], res["occupation"], res["rho"]
    else:
        basis = basis_or_scfres
    total = np.zeros((len(basis.model.atoms), 3))
    for name in basis.model.term_types:
        f = compute_forces_term(name, basis, psi, occupation, rho=rho)
        if f is not None:
            total += f
    return total


def forces_red_to_cart(lattice, forces):
    """covector_red_to_cart: F_cart = inv(lattice') F_red for every atom."""
    return np.asarray(forces, dtype=float) @ np.linalg.inv(np.asarray(lattice, dtype=float))


def compute_forces_cart(basis_or_scfres, psi=None, occupation=None, rho=None):
    """``compute_forces_cart`` (forces.jl:44-47): Cartesian forces, (n_atoms, 3)."""
    basis = basis_or_scfres["basis"] if isinstance(basis_or_scfres, dict) else basis_or_scfres
    return forces_red_to_cart(basis.model.lattice, compute_forces(basis_or_scfres, psi, occupation, rho))
