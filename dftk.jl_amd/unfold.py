"""Symmetry operations on orbitals and the unfolding of an irreducible SCF onto the full Monkhorst-Pack mesh (host mirror of
src/symmetry.jl:229-270 and :459-530).

* ``apply_symop(symop, basis, kpoint, psi_k)``: the orbitals of ``kpoint`` carried to S k, one library call
  (``dftk_mi_apply_symop``: a gather over the rows of the output sphere, the phase once per row, all bands in one launch).
* ``unfold_bz(basis)``: the same model, ``Ecut``, FFT grid and Monkhorst-Pack grid without the k-point reduction;
  ``unfold_mapping`` / ``unfold_array`` / ``unfold_bz(scfres)``: every full-mesh k-point takes the data of the irreducible
  point it is the image of; the orbitals are rotated, eigenvalues and occupations copied, energies and Hamiltonian rebuilt.

Supported: Monkhorst-Pack bases (shifted or not), collinear spin, DFT+U and meta-GGA results (``hubbard_n`` and ``tau`` are
carried through).  Refused: ``ExplicitKpoints`` bases (``ValueError``), ``comm_kpts`` / ``comm_pw`` of more than one rank and
exact exchange (``NotImplementedError``).  The unfolded basis keeps its symmetry list, as in the reference.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .model import MonkhorstPack
from .symmetry import SYMMETRY_TOLERANCE, normalize_kpoint_coordinate
from .transfer import _ordered_with_torch


def _refuse(basis, who):
    """What neither function does, decided before any device work."""
    if basis.comm_kpts.size > 1 or basis.comm_pw.size > 1:
        raise NotImplementedError(f"{who}: Brillouin-zone unfolding is not supported over comm_kpts or comm_pw "
                                  "(the reference refuses MPI as well)")
    if getattr(basis.model, "exact_exchange", None) is not None:
        raise NotImplementedError(f"{who}: models with exact exchange are not supported (Gamma point only: nothing to unfold)")


def symop_image(symop, kcoord):
    """``(Sk, kshift)``: S k reduced to [-0.5, 0.5)^3 and the integer vector Sk - S k (symmetry.jl:236-240)."""
    kcoord = np.asarray(kcoord, dtype=float)
    if not np.all((-0.5 <= kcoord) & (kcoord < 0.5)):
        raise ValueError(f"apply_symop: the k-point {kcoord} is not in [-0.5, 0.5)^3")
    Sk_raw = np.asarray(symop.S, dtype=float) @ kcoord
    Sk = normalize_kpoint_coordinate(Sk_raw)
    return Sk, np.rint(Sk - Sk_raw).astype(np.int32)


def apply_symop(symop, basis, kpoint, psi_k, out_kpoint=None, wait=True):
    """``apply_symop(symop, basis, kpoint, psi_k) -> (Skpoint, psi_Sk)`` (symmetry.jl:229-270):
    u_{Sk}(G) = e^{-2 pi i (G + kshift).tau} u_k(S^-1 (G + kshift)), with S k reduced to [-0.5, 0.5)^3 by the integer
    ``kshift``.  The identity returns its inputs.  ``Skpoint`` is the k-point of ``basis`` at S k with the spin of ``kpoint``
    where the basis has one, else a new ``Kpoint``.  ``psi_k``: band-major ``(n_bands, n_G)`` complex128 CUDA block, or one
    orbital ``(n_G,)``.  An operation that is not a symmetry of the discretised sphere raises ``DftkMiError``.
    ``out_kpoint`` (an extension, what ``unfold_array`` uses): a k-point at S k of ANOTHER basis of the same model, ``Ecut``,
    FFT grid and device, returned as ``Skpoint`` -- its k-block receives the rows, none is built; ``wait=False`` leaves the
    host synchronisation after the call to the caller (``basis.post_call`` of the output k-point's basis)."""
    if symop.isone() and out_kpoint is None:
        return kpoint, psi_k
    _refuse(basis, "apply_symop")
    Sk, kshift = symop_image(symop, kpoint.coordinate)
    basis._require_gpu()
    if not (torch.is_tensor(psi_k) and psi_k.is_cuda and psi_k.dtype == torch.complex128 and psi_k.dim() in (1, 2)
            and psi_k.stride(-1) == 1):
        raise TypeError("apply_symop: band-major complex128 CUDA block required (the hot path has no CPU fallback)")
    if psi_k.shape[-1] != kpoint.n_G:
        raise ValueError(f"apply_symop: the block must be (n_bands, {kpoint.n_G})")
    if out_kpoint is not None:
        Skpoint, basis_out = out_kpoint, out_kpoint.basis
        basis_out._require_gpu()
        if (basis_out.device != basis.device or basis_out.fft_size != basis.fft_size or basis_out.Ecut != basis.Ecut
                or Skpoint.spin != kpoint.spin or np.any(np.abs(Skpoint.coordinate - Sk) > SYMMETRY_TOLERANCE)):
            raise ValueError(f"apply_symop: out_kpoint {Skpoint.coordinate} is not the k-point S k = {Sk} of a basis with the "
                             "same cut-off, grid and device")
        if Skpoint.n_G != kpoint.n_G:      # (a symmetry maps the sphere of k onto that of S k, row for row)
            raise RuntimeError(f"apply_symop: the spheres of k = {kpoint.coordinate} and S k = {Sk} differ in size")
    else:
        from .basis import Kpoint
        basis_out = basis
        Skpoint = next((q for q in basis.kpoints
                        if q.spin == kpoint.spin and np.all(np.abs(q.coordinate - Sk) < SYMMETRY_TOLERANCE)), None)
        if Skpoint is None:
            Skpoint = Kpoint(basis, Sk, spin=kpoint.spin, lane=kpoint.lane)
    block = psi_k.reshape(1, -1) if psi_k.dim() == 1 else psi_k
    nb = block.shape[0]
    out = torch.empty((nb, Skpoint.n_G), dtype=torch.complex128, device=block.device)
    invS = np.ascontiguousarray(np.rint(np.linalg.inv(np.asarray(symop.S, dtype=float))).astype(np.int32).ravel(order="F"))
    tau = np.ascontiguousarray(symop.tau, dtype=np.float64)
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_apply_symop(kpoint.handle, Skpoint.handle, invS.ctypes.data, kshift.ctypes.data,
                                             tau.ctypes.data, nb, block.data_ptr(), block.stride(0) if nb > 1 else kpoint.n_G,
                                             out.data_ptr(), out.stride(0) if nb > 1 else Skpoint.n_G))
    # the entry orders the streams of the two k-blocks against each other; torch follows if it runs on one of them
    if wait and not (_ordered_with_torch(basis, kpoint.lane) or _ordered_with_torch(basis_out, Skpoint.lane)):
        basis_out.post_call(Skpoint.lane)
    return Skpoint, (out.reshape(-1) if psi_k.dim() == 1 else out)


def _unfold_basis(basis):
    """``unfold_bz(basis)`` (symmetry.jl:459-472)."""
    from .basis import PlaneWaveBasis
    if not isinstance(getattr(basis, "kgrid", None), MonkhorstPack):
        raise ValueError("unfold_bz: the basis must be constructed from a MonkhorstPack grid (an ExplicitKpoints list has no "
                         "full mesh to unfold onto)")
    _refuse(basis, "unfold_bz")
    if len(basis.symmetries) == 1:
        return basis
    return PlaneWaveBasis(basis.model, basis.Ecut, basis.kgrid, fft_size=basis.fft_size, device=basis.device,
                          use_symmetries_for_kpoint_reduction=False, gamma_real=basis.gamma_real,
                          build_terms=basis.terms is not None, symmetries_respect_rgrid=basis.symmetries_respect_rgrid)


def unfold_mapping(basis_irred, kpt_unfolded):
    """``(ik_irred, symop)``: where in ``basis_irred`` the k-point ``kpt_unfolded`` is handled (symmetry.jl:475-487) -- the
    first irreducible k-point of the same spin and the first symmetry with S k_irred = k_unfolded."""
    k_unfolded = normalize_kpoint_coordinate(kpt_unfolded.coordinate)
    for ik, kpt in enumerate(basis_irred.kpoints):
        if kpt.spin != kpt_unfolded.spin:
            continue
        for symop in basis_irred.symmetries:
            Sk = normalize_kpoint_coordinate(np.asarray(symop.S, dtype=float) @ kpt.coordinate)
            if np.all(np.abs(Sk - k_unfolded) < SYMMETRY_TOLERANCE):
                return ik, symop
    raise ValueError(f"Invalid unfolding of BZ: no irreducible k-point maps onto {kpt_unfolded.coordinate}")


def unfold_array(basis_irred, basis_unfolded, data, is_psi):
    """``unfold_array(basis_irred, basis_unfolded, data, is_psi)`` (symmetry.jl:489-518): one entry per k-point of
    ``basis_unfolded``; orbital blocks are rotated with ``apply_symop``, everything else is copied."""
    if basis_irred is basis_unfolded:
        return data
    _refuse(basis_irred, "unfold_array")
    if len(data) != len(basis_irred.kpoints):
        raise ValueError("unfold_array: one entry per k-point of basis_irred")
    out = []
    for kpt in basis_unfolded.kpoints:
        ik, symop = unfold_mapping(basis_irred, kpt)
        if not is_psi:
            out.append(data[ik].clone() if torch.is_tensor(data[ik]) else np.array(data[ik], copy=True))
            continue
        if np.any(np.abs(normalize_kpoint_coordinate(kpt.coordinate) - kpt.coordinate) > SYMMETRY_TOLERANCE):
            raise ValueError(f"unfold_array: the k-point {kpt.coordinate} of the unfolded basis is not in [-0.5, 0.5)^3")
        # the k-block of the unfolded basis receives the rows: no k-block is built for S k, and the library's check of the
        # pre-images is remembered on it
        _, psi_Sk = apply_symop(symop, basis_irred, basis_irred.kpoints[ik], data[ik], out_kpoint=kpt, wait=False)
        out.append(psi_Sk)
    if is_psi:
        basis_unfolded.post_call()           # one wait for all k-points
    return out


def unfold_bz(basis_or_scfres):
    """``unfold_bz(basis)`` (symmetry.jl:459-472): the basis without the k-point reduction (the basis itself when it has
    no symmetry but the identity).  ``unfold_bz(scfres)`` (:520-530): the SCF result on that basis -- ``basis``, ``psi``,
    ``ham``, ``eigenvalues`` and ``occupation`` replaced, everything else (density, Fermi level, ``hubbard_n``, ``tau``,
    energies ...) carried over; the energies rebuilt from the unfolded orbitals must reproduce the total of the result to
    1.5e-8 relative (sqrt(eps), the reference's ``@assert ... ≈``), else ``RuntimeError``.  The input is not modified."""
    if not isinstance(basis_or_scfres, dict):
        return _unfold_basis(basis_or_scfres)
    from .terms import energy_hamiltonian
    scfres = basis_or_scfres
    basis = scfres["basis"]
    basis_unfolded = _unfold_basis(basis)
    psi = unfold_array(basis, basis_unfolded, scfres["psi"], True)
    eigenvalues = unfold_array(basis, basis_unfolded, scfres["eigenvalues"], False)
    occupation = unfold_array(basis, basis_unfolded, scfres["occupation"], False)
    extra = {key: scfres[key] for key in ("hubbard_n", "tau") if scfres.get(key) is not None}
    energies, ham = energy_hamiltonian(basis_unfolded, psi, occupation, rho=scfres["rho"], eigenvalues=eigenvalues,
                                       eF=scfres.get("eF"), **extra)
    E_ref = float(scfres["energies"].total)
    if not abs(float(energies.total) - E_ref) <= 1.5e-8 * max(abs(float(energies.total)), abs(E_ref)):
        raise RuntimeError(f"unfold_bz: the total energy of the unfolded state, {float(energies.total)!r}, differs from the "
                           f"result's, {E_ref!r}")
    out = dict(scfres)
    out.update(basis=basis_unfolded, psi=psi, ham=ham, eigenvalues=eigenvalues, occupation=occupation)
    return out
