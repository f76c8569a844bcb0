"""Transfer of orbital blocks and densities between two plane-wave bases of the same lattice (host mirror of
src/transfer.jl:10-178).

* ``transfer_blochwave_kpt`` / ``transfer_blochwave``: one library call per k-point (``dftk_mi_transfer_blochwave``: a gather
  over the rows of the output sphere, all bands in one launch, bit-for-bit reproducible).
* ``transfer_density``: one library call (``dftk_mi_transfer_density``: cube FFT on the input grid, the index blocks of
  ``transfer_mapping``, inverse cube FFT on the output grid).

Orbital blocks are band-major ``(n_bands, n_G)`` complex128 CUDA tensors, densities ``(nz, ny, nx)`` or ``(n_spin, nz, ny, nx)``
real CUDA tensors, as everywhere in this package.  The two bases may differ in ``Ecut`` and FFT grid; they must share the
lattice and the device.  The private index helpers of the two-level LOBPCG start (eigen.py) are a separate, older path.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .symmetry import SYMMETRY_TOLERANCE


def check_same_lattice(basis_in, basis_out, who="transfer"):
    """``@assert basis_in.model.lattice == basis_out.model.lattice`` (transfer.jl:11, :48, :100, :130, :167)."""
    if not np.array_equal(np.asarray(basis_in.model.lattice, dtype=float), np.asarray(basis_out.model.lattice, dtype=float)):
        raise ValueError(f"{who}: the two bases must have the same lattice")


def check_same_kpoints(basis_in, basis_out, who="transfer"):
    """transfer.jl:101-103, :132-134: as many k-points, with equal coordinates."""
    if len(basis_in.kpoints) != len(basis_out.kpoints):
        raise ValueError(f"{who}: the two bases must have the same number of k-points "
                         f"({len(basis_in.kpoints)} and {len(basis_out.kpoints)})")
    for ik, (a, b) in enumerate(zip(basis_in.kpoints, basis_out.kpoints)):
        if not np.array_equal(a.coordinate, b.coordinate) or a.spin != b.spin:
            raise ValueError(f"{who}: k-point {ik} differs between the two bases ({a.coordinate} and {b.coordinate})")


def delta_G(kpt_in, kpt_out):
    """The integer vector ``dG = k_out - k_in`` (transfer.jl:49-51); ``ValueError`` if the two k-points are not equivalent."""
    d = np.asarray(kpt_out.coordinate, dtype=float) - np.asarray(kpt_in.coordinate, dtype=float)
    r = np.round(d)
    if np.any(np.abs(d - r) > SYMMETRY_TOLERANCE):
        raise ValueError(f"transfer_blochwave_kpt: k_out - k_in = {d} is not an integer vector: the k-points {kpt_in.coordinate} "
                         f"and {kpt_out.coordinate} are not equivalent")
    return r.astype(np.int32)


def _refuse_sharded(basis, who):
    if basis.comm_pw.size > 1:
        raise NotImplementedError(f"{who}: a basis whose plane waves are sharded over comm_pw is not supported")


def _ordered_with_torch(basis, lane):
    # torch's current stream IS the stream of this lane of the basis (on_library_stream): no host synchronisation needed
    return basis._same_stream() and lane == 0


def transfer_blochwave_kpt(psik_in, basis_in, kpt_in, basis_out, kpt_out):
    """``transfer_blochwave_kpt(psik_in, basis_in, kpt_in, basis_out, kpt_out)`` (transfer.jl:112-124): the block ``psik_in`` of
    ``kpt_in`` expressed on ``kpt_out``, which must be ``kpt_in`` shifted by an integer vector dG (the Bloch wave is the same,
    its periodic part is multiplied by e^{-i dG x}).  The coefficient of plane wave G moves to the row of ``kpt_out`` that
    carries G - dG; rows without a partner are zero, coefficients without one are dropped (lossy from a larger to a smaller
    basis)."""
    check_same_lattice(basis_in, basis_out, "transfer_blochwave_kpt")
    dG = delta_G(kpt_in, kpt_out)
    _refuse_sharded(basis_in, "transfer_blochwave_kpt")
    _refuse_sharded(basis_out, "transfer_blochwave_kpt")
    basis_in._require_gpu()
    basis_out._require_gpu()
    if basis_in.device != basis_out.device:
        raise ValueError("transfer_blochwave_kpt: the two bases must live on the same device")
    if not (torch.is_tensor(psik_in) and psik_in.is_cuda and psik_in.dtype == torch.complex128 and psik_in.dim() == 2
            and psik_in.stride(1) == 1):
        raise TypeError("transfer_blochwave_kpt: band-major complex128 CUDA block required (the hot path has no CPU fallback)")
    if psik_in.shape[1] != kpt_in.n_G:
        raise ValueError(f"transfer_blochwave_kpt: the block must be (n_bands, {kpt_in.n_G})")
    nb = psik_in.shape[0]
    out = torch.empty((nb, kpt_out.n_G), dtype=torch.complex128, device=psik_in.device)
    if nb == 0:
        return out
    basis_in.pre_call()
    basis_out.pre_call()
    _lib.check(basis_out.lib.dftk_mi_transfer_blochwave(kpt_in.handle, kpt_out.handle, dG.ctypes.data, nb, psik_in.data_ptr(),
                                                        psik_in.stride(0), out.data_ptr(), out.stride(0)))
    # the entry orders the streams of the two bases against each other; torch follows if it runs on one of them
    if not (_ordered_with_torch(basis_in, kpt_in.lane) or _ordered_with_torch(basis_out, kpt_out.lane)):
        basis_out.post_call(kpt_out.lane)
    return out


def transfer_blochwave(psi_in, basis_in, basis_out):
    """``transfer_blochwave(psi_in, basis_in, basis_out)`` (transfer.jl:129-150): every k-block of ``psi_in`` on the k-point of
    ``basis_out`` with the same coordinate."""
    check_same_lattice(basis_in, basis_out, "transfer_blochwave")
    check_same_kpoints(basis_in, basis_out, "transfer_blochwave")
    if len(psi_in) != len(basis_in.kpoints):
        raise ValueError("transfer_blochwave: one block per k-point of basis_in")
    return [transfer_blochwave_kpt(psik, basis_in, kin, basis_out, kout)
            for psik, kin, kout in zip(psi_in, basis_in.kpoints, basis_out.kpoints)]


def transfer_density(rho_in, basis_in, basis_out):
    """``transfer_density(rho_in, basis_in, basis_out)`` (transfer.jl:165-178): the density moved through its Fourier
    coefficients.  ``rho_in``: ``(nz, ny, nx)`` or ``(n_spin, nz, ny, nx)`` on the grid of ``basis_in``; the result has the
    same number of dimensions on the grid of ``basis_out``.  For an even axis of the smaller grid, small -> large -> small
    is not the identity (the unmatched frequency -n/2 is carried along without its partner).
    One deviation from the reference: the index blocks of ``transfer_mapping`` are reproduced exactly, but the inverse
    transform is this package's (complex transform, real part, as ``basis.irfft``), where the reference's half-spectrum
    ``irfft`` reads the x >= 0 half only.  Of an unmatched plane g_x = -n_x/2 (even small n_x) the reference therefore drops
    all and this function keeps the Hermitian half; along y and z, and for every matched frequency, the two agree.  The
    density of orbitals on a sphere inside the grid has nothing on that plane."""
    check_same_lattice(basis_in, basis_out, "transfer_density")
    if not torch.is_tensor(rho_in) or rho_in.dim() not in (3, 4):
        raise ValueError("transfer_density: rho_in must be a three- or four-dimensional real cube")
    nx, ny, nz = basis_in.fft_size
    if tuple(rho_in.shape[-3:]) != (nz, ny, nx):
        raise ValueError(f"transfer_density: rho_in must live on the grid of basis_in, (.., {nz}, {ny}, {nx})")
    n_spin = 1 if rho_in.dim() == 3 else int(rho_in.shape[0])
    if n_spin not in (1, 2):
        raise ValueError("transfer_density: one or two spin components")
    basis_in._require_gpu()
    basis_out._require_gpu()
    if basis_in.device != basis_out.device:
        raise ValueError("transfer_density: the two bases must live on the same device")
    if not rho_in.is_cuda:
        raise TypeError("transfer_density: CUDA tensor required (the hot path has no CPU fallback)")
    rho = rho_in.to(torch.float64).contiguous()
    ox, oy, oz = basis_out.fft_size
    out = torch.empty(((oz, oy, ox) if rho_in.dim() == 3 else (n_spin, oz, oy, ox)), dtype=torch.float64, device=rho.device)
    basis_in.pre_call()
    basis_out.pre_call()
    _lib.check(basis_out.lib.dftk_mi_transfer_density(basis_in._cube_handle, basis_out._cube_handle, n_spin, rho.data_ptr(),
                                                      out.data_ptr()))
    if not (_ordered_with_torch(basis_in, 0) or _ordered_with_torch(basis_out, 0)):
        basis_out.post_call(0)
    return out
