"""Exact exchange at the Gamma point: interaction kernels, the Fock operator, its adaptive compression and its energy.

Reference: src/coulomb.jl (kernels on the Gamma sphere), src/terms/exact_exchange.jl (``VanillaExx``, ``AceExx``,
``compress_exchange``, ``exx_energy_only``), ``ExchangeOperator`` of src/terms/operators.jl:184-210.

The operator itself is ONE library call (``dftk_mi_exx_apply``, csrc/exx_kernels.hip: two pruned transforms per
(occupied orbital, column) pair).  The compressed operator -xi xi' has the shape of the nonlocal term and rides in the
k-block's projector slot: P_ext = [P_nl; xi], D_ext = blockdiag(D, -I) (``bind_projectors``), so that ``dftk_mi_apply_H`` and
the LOBPCG driver apply it without knowing about it.  Orbital blocks are band-major (n_bands, n_G) complex128 tensors.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib


# ---------------------------------------------------------------------------------- interaction kernels (coulomb.jl)
@dataclass(frozen=True)
class ProbeCharge:
    """Gygi-Baldereschi probe-charge value of the G = 0 component (coulomb.jl:309-339); alpha = pi^2 / Ecut."""
    alpha: float | None = None


@dataclass(frozen=True)
class ReplaceSingularity:
    """The G = 0 component set to ``value`` (coulomb.jl:350-363)."""
    value: float = 0.0


@dataclass(frozen=True)
class VoxelAveraged:
    n_quadrature_points: int = 12


@dataclass(frozen=True)
class Coulomb:
    """1 / r (coulomb.jl:57-62)."""
    regularization: object = field(default_factory=ProbeCharge)


@dataclass(frozen=True)
class ShortRangeCoulomb:
    """erfc(mu r) / r (coulomb.jl:68-80); G = 0 value pi / mu^2.  mu in inverse bohr (0.2 / angstrom by default)."""
    mu: float = 0.2 * 0.529177210903


@dataclass(frozen=True)
class LongRangeCoulomb:
    mu: float = 0.2 * 0.529177210903
    regularization: object = field(default_factory=ProbeCharge)


@dataclass(frozen=True)
class SphericallyTruncatedCoulomb:
    """theta(Rcut - r) / r (coulomb.jl:156-172); Rcut = cbrt(3 Omega / 4 pi) unless given; G = 0 value 2 pi Rcut^2."""
    Rcut: float | None = None


@dataclass(frozen=True)
class WignerSeitzTruncatedCoulomb:
    pass


def check_gamma_only(kcoords, n_ranks_kpts=1, n_ranks_pw=1):
    """The refusals of compute_kernel_fourier (coulomb.jl:126-136)."""
    if any(np.any(np.asarray(k, dtype=float) != 0) for k in kcoords) or len(kcoords) != 1:
        raise ValueError("exact exchange (Hartree-Fock, hybrid functionals): only Gamma-point calculations are supported, "
                         f"got the k-points {[list(map(float, k)) for k in kcoords]}")
    if n_ranks_kpts > 1:
        raise ValueError("exact exchange: k-point parallelisation (comm_kpts larger than 1) is not supported")
    if n_ranks_pw > 1:
        raise ValueError("exact exchange: plane-wave sharding (comm_pw larger than 1) is not supported")


def compute_kernel_fourier(kernel, basis) -> torch.Tensor:
    """``compute_kernel_fourier(kernel, basis)`` (coulomb.jl:126-146): the kernel on the Gamma sphere, n_G reals on
    ``basis.device``.  Row 0 of the sphere is G = 0."""
    check_gamma_only(basis.kcoords_global, basis.comm_kpts.size, basis.comm_pw.size)
    kpt = basis.kpoints[0]
    G2 = (kpt.Gplusk_cart.to(torch.float64) ** 2).sum(dim=1)
    if float(G2[0].item()) != 0.0:
        raise ValueError("exact exchange: the first plane wave of the Gamma sphere must be G = 0")
    rest = G2[1:]
    coulomb = 4 * math.pi / rest

    def with_G0(values, v0):
        return torch.cat([torch.tensor([float(v0)], dtype=torch.float64, device=G2.device), values]).contiguous()

    if isinstance(kernel, Coulomb):
        reg = kernel.regularization
        if isinstance(reg, ReplaceSingularity):
            return with_G0(coulomb, reg.value)
        if isinstance(reg, ProbeCharge):
            alpha = math.pi ** 2 / basis.Ecut if reg.alpha is None else float(reg.alpha)
            recip_cell_volume = abs(np.linalg.det(basis.model.recip_lattice))
            integral = 8 * math.pi ** 2 * math.sqrt(math.pi / alpha) / recip_cell_volume
            return with_G0(coulomb, integral - float((coulomb * torch.exp(-alpha * rest)).sum().item()))
        raise NotImplementedError(f"exact exchange: regularization {type(reg).__name__} of the Coulomb kernel is not "
                                  "implemented (ProbeCharge and ReplaceSingularity are)")
    if isinstance(kernel, ShortRangeCoulomb):
        mu = float(kernel.mu)
        return with_G0(-coulomb * torch.expm1(-rest / (4 * mu ** 2)), math.pi / mu ** 2)
    if isinstance(kernel, SphericallyTruncatedCoulomb):
        Rcut = float(np.cbrt(3 * basis.model.unit_cell_volume / (4 * math.pi))) if kernel.Rcut is None else float(kernel.Rcut)
        return with_G0(coulomb * (1 - torch.cos(Rcut * torch.sqrt(rest))), 2 * math.pi * Rcut ** 2)
    raise NotImplementedError(f"exact exchange: interaction kernel {type(kernel).__name__} is not implemented (Coulomb, "
                              "ShortRangeCoulomb and SphericallyTruncatedCoulomb are)")


# ---------------------------------------------------------------------------------- algorithms (exact_exchange.jl:68-103)
@dataclass(frozen=True)
class VanillaExx:
    """The uncompressed operator: every H psi costs n_occ pair transforms per column.  ``mul_`` applies it; the library's
    LOBPCG driver cannot (it knows the projector slot only): diagonalise with ``AceExx``."""


@dataclass(frozen=True)
class AceExx:
    """Adaptively compressed exchange (exact_exchange.jl:99-132), sketched with all orbitals handed in or with the
    occupied ones only."""
    sketch_with_extra_orbitals: bool = True


def n_occupied(occ, occupation_threshold=0.0) -> int:
    """occupied_empty_masks (occupation.jl:242-249): 1 .. the last band with |occupation| above the threshold"""
    idx = np.nonzero(np.abs(np.asarray(occ, dtype=float)) > occupation_threshold)[0]
    return int(idx[-1]) + 1 if len(idx) else 0


def _check_block(name, X, n_G):
    if not (X.is_cuda and X.dtype == torch.complex128 and X.dim() == 2 and X.shape[1] == n_G
            and (X.shape[0] == 0 or (X.stride(1) == 1 and X.stride(0) >= n_G))):
        raise ValueError(f"{name}: a band-major (n_bands, {n_G}) complex128 CUDA block is required")


def apply_exchange(basis, ik, psi_occ, occ, psi, out=None, accumulate=False):
    """``out (+)= Vx psi`` with the exchange operator built from the orbitals ``psi_occ`` with occupations ``occ``
    (apply!(Hpsi, ::ExchangeOperator, psi) between ifft and fft!): one ``dftk_mi_exx_apply`` call."""
    basis._require_gpu()
    T = basis.terms
    if T is None or getattr(T, "exx_kernel", None) is None:
        raise ValueError("apply_exchange: the model of this basis has no ExactExchange term")
    kpt = basis.kpoints[ik]
    _check_block("apply_exchange: psi_occ", psi_occ, kpt.n_G)
    _check_block("apply_exchange: psi", psi, kpt.n_G)
    w = np.ascontiguousarray(np.asarray(occ, dtype=np.float64) / basis.model.filled_occupation)
    if len(w) != psi_occ.shape[0]:
        raise ValueError("apply_exchange: one occupation per row of psi_occ")
    if out is None:
        if accumulate:
            raise ValueError("apply_exchange: accumulate needs out")
        out = torch.empty((psi.shape[0], kpt.n_G), dtype=torch.complex128, device=psi.device)
    _check_block("apply_exchange: out", out, kpt.n_G)
    if out.shape[0] != psi.shape[0]:
        raise ValueError("apply_exchange: out must have the shape of psi")
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_exx_apply(kpt.handle, psi_occ.shape[0], psi_occ.data_ptr(), psi_occ.stride(0) or kpt.n_G,
                                           w.ctypes.data, T.exx_kernel.data_ptr(), psi.shape[0], psi.data_ptr(),
                                           psi.stride(0) or kpt.n_G, out.data_ptr(), out.stride(0) or kpt.n_G,
                                           1 if accumulate else 0))
    basis.post_call(kpt.lane)
    return out


@dataclass
class ExchangeOperator:
    """What a Hamiltonian block keeps of the exchange term: ``xi`` (ACE: n_sketch x n_G, the operator is -xi' xi in
    band-major terms) or the occupied orbitals and their occupations (vanilla)."""
    xi: torch.Tensor | None = None
    psi_occ: torch.Tensor | None = None
    occ: np.ndarray | None = None
    M: np.ndarray | None = None          # diagonal of psi' Vx psi on the sketch (host)


def exchange_energy(basis, ik, psik, occk, occupation_threshold=0.0) -> float:
    """1/2 sum_n occ_n Re <psi_n | Vx psi_n> over the occupied orbitals (the number ``exx_energy_only`` returns)."""
    from .eigen import columnwise_dots
    n_occ = n_occupied(occk, occupation_threshold)
    if n_occ == 0:
        return 0.0
    occ = np.asarray(occk, dtype=float)[:n_occ]
    W = apply_exchange(basis, ik, psik[:n_occ], occ, psik[:n_occ])
    return 0.5 * float(np.dot(occ, np.real(columnwise_dots(basis, psik[:n_occ], W))))


def exx_operator(exxalg, basis, ik, psik, occk, occupation_threshold=0.0):
    """``exx_operator(exxalg, basis, kpt, kernel, psik, occk, mask_occ)`` -> (E_k, ExchangeOperator | None)."""
    n_occ = n_occupied(occk, occupation_threshold)
    if n_occ == 0:
        return 0.0, None
    occ = np.asarray(occk, dtype=float)
    psi_occ = psik[:n_occ]
    if isinstance(exxalg, VanillaExx):
        E = exchange_energy(basis, ik, psik, occk, occupation_threshold)
        return E, ExchangeOperator(psi_occ=psi_occ.contiguous(), occ=occ[:n_occ].copy())
    if not isinstance(exxalg, AceExx):
        raise TypeError(f"exxalg must be VanillaExx() or AceExx(), got {exxalg!r}")
    # compress_exchange (exact_exchange.jl:136-154): W = Vx Psi, M = Psi' W, -M = R' R, xi = W inv(R)
    sketch = psik if exxalg.sketch_with_extra_orbitals else psi_occ
    n_sk, n_G = sketch.shape
    W = apply_exchange(basis, ik, psi_occ, occ[:n_occ], sketch)
    Mt = torch.empty((n_sk, n_sk), dtype=torch.complex128, device=W.device)        # column-major M
    one, zero = _lib.cplx(1.0), _lib.cplx(0.0)
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_zgemm(basis.handle, b"C", n_sk, n_sk, n_G, one, sketch.data_ptr(), sketch.stride(0),
                                       W.data_ptr(), W.stride(0), zero, Mt.data_ptr(), n_sk))
    basis.post_call()
    diag = torch.diagonal(Mt).real.cpu().numpy().copy()
    E = 0.5 * float(np.dot(occ[:n_sk], diag))
    A = (-(Mt + Mt.conj().T) / 2).contiguous()                                     # Hermitian(-M)
    invR = torch.zeros_like(A)
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_potrf_trtri(basis.handle, n_sk, A.data_ptr(), n_sk, invR.data_ptr(), n_sk))
    xi = torch.empty_like(W)
    _lib.check(basis.lib.dftk_mi_zgemm(basis.handle, b"N", n_G, n_sk, n_sk, one, W.data_ptr(), W.stride(0),
                                       invR.data_ptr(), n_sk, zero, xi.data_ptr(), n_G))
    basis.post_call()
    return E, ExchangeOperator(xi=xi, M=diag)


def bind_projectors(basis, ik, xi=None):
    """Make the k-block's projector slot hold [P_nl; xi] with couplings blockdiag(D, -I) (``xi`` None: the nonlocal
    term alone).  The buffer has room for the xi rows: a rebind copies them, not P."""
    kpt, T = basis.kpoints[ik], basis.terms
    P = T.P[ik] if T.P is not None else None
    n_p = 0 if P is None else P.shape[0]
    n_xi = 0 if xi is None else xi.shape[0]
    basis.pre_call()
    if n_xi == 0:
        if n_p == 0:
            _lib.check(basis.lib.dftk_mi_kblock_set_projectors(kpt.handle, 0, None, kpt.n_G, None))
        else:
            _lib.check(basis.lib.dftk_mi_kblock_set_projectors(kpt.handle, n_p, P.data_ptr(), kpt.n_loc,
                                                               kpt._keep["D"].ctypes.data))
        return
    buf = old = kpt._keep.get("exx_P")
    if buf is None or buf.shape[0] < n_p + n_xi:
        # (the library may still read the old buffer: `old` holds it until set_projectors below has synchronised)
        buf = torch.empty((n_p + n_xi, kpt.n_G), dtype=torch.complex128, device=xi.device)
        if n_p:
            buf[:n_p] = P
        kpt._keep["exx_P"] = buf
    buf[n_p:n_p + n_xi] = xi
    D = np.zeros((n_p + n_xi, n_p + n_xi), order="F")
    if n_p:
        D[:n_p, :n_p] = T.D
    D[n_p:, n_p:] = -np.eye(n_xi)
    kpt._keep["exx_D"] = D
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_kblock_set_projectors(kpt.handle, n_p + n_xi, buf.data_ptr(), kpt.n_G, D.ctypes.data))
    del old


def refuse(model, what):
    """Entry points that have no exchange term yet."""
    if getattr(model, "exact_exchange", None) is not None:
        raise NotImplementedError(f"{what} is not implemented for models with exact exchange (Hartree-Fock, hybrid "
                                  "functionals)")
