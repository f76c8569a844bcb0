"""The density response of a converged ground state at q = 0 (host mirror of src/response/chi0.jl, src/response/cg.jl,
``compute_drho`` of src/densities.jl:60-108, ``apply_kernel`` of src/terms, ``solve_OmegaPlusK_split`` of
src/response/hessian.jl:266-359).

* ``sternheimer_solver``: one library call per k-point (``dftk_mi_sternheimer``: the reference's Schur split over the extra
  bands and its preconditioned block CG with locking, one host synchronisation per iteration).
* ``apply_chi0_4P`` / ``apply_chi0``: the independent-particle response chi0 dV -- occupation changes on the host, the
  explicit finite-temperature term through the library's ``zgemm``, the Sternheimer solves spread over the basis' lanes,
  ``compute_delta_rho`` through ``dftk_mi_density_response_accumulate``.
* ``apply_kernel``: Hartree + LDA exchange-correlation kernel in one library call (``dftk_mi_apply_kernel``).
* ``solve_OmegaPlusK_split``: the self-consistent response, (1 - chi0 K) d_rho = chi0 dV_ext by the GMRES of mixing.py.

Spellings are ASCII (``chi0`` for the reference's chi_0, ``delta`` / ``d`` for its delta), as ``Chi0Mixing``.  Orbital blocks
are band-major ``(n_bands, n_G)`` complex128 CUDA tensors, as everywhere in this package.  Outside the scope of this layer,
each refused with ``NotImplementedError``: q != 0 (phonons), collinear spin, GGA kernels, a basis sharded over ``comm_pw``,
``compute_chi0`` as a dense matrix and ``solve_OmegaPlusK`` (the CG on the tangent space).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .hamiltonian import DftHamiltonianBlock
from .mixing import gmres, occupation_derivative
from .scf import _smear
from .symmetry import symmetrize_rho
from .terms import _GGA_BITS, _LDA_BITS, total_density

EPS = float(np.finfo(np.float64).eps)
_KERNEL_LDA = ("lda_x", "lda_c_vwn", "lda_c_pw")          # functionals whose f_xc the library has in closed form


# ------------------------------------------------------------------------------------------ pure host functions
def _occ1(kind, x):
    return float(_smear(kind, np.array([float(x)]))[0])


def occupation_divided_difference(kind, em, en, eF, temperature):
    """``(f(em) - f(en)) / (em - en)`` for the occupation function ``f(e) = smearing((e - eF) / T)``, stable for close
    arguments (Smearing.jl:31-56, :94-111): equal arguments give ``f'((e - eF) / T) / T``; at T = 0 (or without smearing) the
    step function, and 0 for equal arguments."""
    x, y = float(em), float(en)
    if temperature == 0 or kind == "none":
        if x == y:
            return 0.0
        fx = 1.0 if x < eF else 0.0
        fy = 1.0 if y < eF else 0.0
        return (fx - fy) / (x - y)
    T = float(temperature)

    def f(z):
        return _occ1(kind, (z - eF) / T)

    def fder(z):
        return float(occupation_derivative(kind, (z - eF) / T)) / T

    def generic():
        # (f(x) - f(y)) / (x - y) is accurate to eps / |x - y|, (f'(x) + f'(y)) / 2 to |x - y|^2
        if abs(x - y) < EPS ** (1 / 3):
            return (fder(x) + fder(y)) / 2
        return (f(x) - f(y)) / (x - y)

    if kind == "fermi_dirac":
        # f(x) - f(y) = f(x) f(y) exp(x) expm1(y - x), symmetrised; the generic form where an exponential would overflow
        big = math.log(np.finfo(np.float64).max / 1e4)
        if x == y or any(abs((a - b) / T) > big for a, b in ((x, y), (x, eF), (y, eF))):
            return generic()
        dxy = f(x) * f(y) * math.exp((x - eF) / T) * math.expm1((y - x) / T)
        dyx = f(x) * f(y) * math.exp((y - eF) / T) * math.expm1((x - y) / T)
        return (dxy - dyx) / 2 / (x - y)
    return generic()


def compute_alpha_mn(fm, fn, ratio):
    """The coefficient alpha_mn of <psi_m|dpsi_n> = alpha_mn <psi_m|dH|psi_n> that minimises alpha_mn^2 + alpha_nm^2 under
    ``fn alpha_mn + fm alpha_nm = ratio`` (chi0.jl:268-287)."""
    if ratio == 0:
        return ratio
    return ratio * fn / (fn * fn + fm * fm)


def is_effective_insulator(basis, eigenvalues, eF, atol=EPS, smearing=None, temperature=None):
    """No band is fractionally occupied to ``atol`` (chi0.jl:289-306); the minimum runs over ``comm_kpts``."""
    smearing = basis.model.smearing if smearing is None else smearing
    temperature = basis.model.temperature if temperature is None else temperature
    if temperature == 0 or smearing == "none":
        return True
    vals = [float(np.min(np.abs(np.asarray(e, dtype=float) - eF))) / temperature for e in eigenvalues if len(e)]
    m = min(vals) if vals else math.inf
    comm = basis.comm_kpts
    if comm.size > 1:
        m = min(float(v) for v in comm.gather_lists(m))
    return _occ1(smearing, m) < atol


def occupied_empty_masks(occupation, occupation_threshold):
    """Per k-point ``(n_occ, n_bands)``: bands ``[0, n_occ)`` get a response, ``[n_occ, n_bands)`` are the extra bands
    (occupation.jl:242-249: everything up to the LAST band above the threshold)."""
    out = []
    for occ in occupation:
        occ = np.asarray(occ, dtype=float)
        above = np.nonzero(np.abs(occ) > occupation_threshold)[0]
        out.append((int(above[-1]) + 1 if len(above) else 0, len(occ)))
    return out


class _Bandtol:
    """Factors by which a density tolerance is multiplied to give the Sternheimer tolerance of every occupied band
    (chi0.jl:560-646, arXiv 2505.02319)."""
    guaranteed = False

    def __init__(self, basis=None, psi=None, occupation=None, occupation_threshold=0.0, bandtol_min=EPS / 2,
                 bandtol_max=math.inf, _factors=None):
        self.bandtol_min, self.bandtol_max = float(bandtol_min), float(bandtol_max)
        self.occupation_threshold = float(occupation_threshold)
        if _factors is not None:
            self.bandtol_factors = _factors
            return
        vol = basis.model.unit_cell_volume
        Ng = int(np.prod(basis.fft_size))
        Nk = len(occupation)
        masks = occupied_empty_masks(occupation, occupation_threshold)
        self.bandtol_factors = []
        for ik, (n_occ, _) in enumerate(masks):
            occ = np.asarray(occupation[ik], dtype=float)[:n_occ]
            if n_occ == 0:
                self.bandtol_factors.append(np.zeros(0))
                continue
            term = self._orbital_term(basis, ik, psi, n_occ)
            self.bandtol_factors.append((math.sqrt(vol / Ng) / math.sqrt(n_occ) / term)
                                        / (2 * occ * Nk * basis.kweights[ik]))

    def _orbital_term(self, basis, ik, psi, n_occ):
        return math.sqrt(n_occ) / math.sqrt(basis.model.unit_cell_volume)      # lower bound of ||F^-1 Phi_k||_{2,inf}

    def scaled(self, alpha):
        return type(self)(occupation_threshold=self.occupation_threshold, bandtol_min=self.bandtol_min,
                          bandtol_max=self.bandtol_max, _factors=[alpha * f for f in self.bandtol_factors])


class BandtolBalanced(_Bandtol):
    """``BandtolBalanced(basis, psi, occupation; occupation_threshold, bandtol_min, bandtol_max)`` (chi0.jl:581-600)."""


class BandtolGuaranteed(_Bandtol):
    """``BandtolGuaranteed`` (chi0.jl:560-579): the orbital term ||F^-1 Phi_k||_{2,inf} is evaluated on the device (the
    density kernel with unit weights gives sum_n |psi_nk(r)|^2)."""
    guaranteed = True

    def _orbital_term(self, basis, ik, psi, n_occ):
        basis._require_gpu()
        kpt = basis.kpoints[ik]
        ps = psi[ik][:n_occ]
        nx, ny, nz = basis.fft_size
        acc = torch.zeros((nz, ny, nx), dtype=torch.float64, device=basis.device)
        w = np.full(n_occ, basis.ifft_normalization ** 2)
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_density_accumulate(kpt.handle, n_occ, ps.data_ptr(), ps.stride(0), w.ctypes.data,
                                                        acc.data_ptr()))
        basis.post_call(kpt.lane)
        return math.sqrt(float(acc.max().item()))


def determine_band_tolerances(alg, density_tol):
    """chi0.jl:663-667: factor * tol per occupied band, clamped to [bandtol_min, bandtol_max]."""
    return [np.clip(np.asarray(f, dtype=float) * density_tol, alg.bandtol_min, alg.bandtol_max)
            for f in alg.bandtol_factors]


# ------------------------------------------------------------------------------------------ checks
def _check_supported(basis, q=None):
    from .model import refuse_meta_gga
    refuse_meta_gga(basis, "the density response (no meta-GGA kernel, no Sternheimer solve with the div-A-grad term)")
    from .exchange import refuse
    refuse(basis.model, "the density response (no exchange kernel term, no Sternheimer solve with the Fock operator)")
    from .hubbard import refuse as refuse_hubbard
    refuse_hubbard(basis.model, "the density response (no Hubbard kernel term)")
    if q is not None and np.any(np.asarray(q, dtype=float) != 0):
        raise NotImplementedError("response at q != 0 (phonons) is not implemented: q = 0 only")
    if basis.model.n_spin_components != 1:
        raise NotImplementedError("response with collinear spin is not implemented")
    if basis.comm_pw.size > 1:
        raise NotImplementedError("response of a basis whose plane waves are sharded over comm_pw is not implemented")
    basis._require_gpu()


def _check_block(name, x, n_rows=None):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.complex128 and x.dim() == 2 and x.stride(1) == 1):
        raise TypeError(f"{name}: band-major complex128 CUDA block required (the hot path has no CPU fallback)")
    if n_rows is not None and x.shape[1] != n_rows:
        raise ValueError(f"{name}: blocks must be (n_bands, {n_rows})")


def compute_chi0(*args, **kwargs):
    raise NotImplementedError("compute_chi0 (chi0 as a dense matrix) is not implemented: use apply_chi0")


def solve_OmegaPlusK(*args, **kwargs):
    raise NotImplementedError("solve_OmegaPlusK (the CG on the tangent space) is not implemented: use "
                              "solve_OmegaPlusK_split")


# ------------------------------------------------------------------------------------------ Sternheimer
def sternheimer_solver(Hk, psik, eps, rhs, psik_extra=None, tol=1e-9, miniter=1, maxiter=100, dpsik0=None, out=None):
    """``sternheimer_solver(Hk, psik, eps, rhs; psik_extra, tol, miniter, maxiter, dpsik0)`` (chi0.jl:115-232): solves
    ``Q (Hk - eps_n) Q dpsi_n = -Q rhs_n`` with Q the projector onto the orthogonal of ``psik``, for all columns at once.
    ``psik`` must diagonalise Hk (``eps`` its eigenvalues), ``psik_extra`` are further Rayleigh-Ritz vectors used for the
    Schur split.  ``tol``: one number or one per column; ``out``: an ``(n_occ, n_G)`` block that takes the result.  Returns
    ``dict(dpsik, n_iter, residual_norms, converged, tol)``."""
    basis = Hk.basis
    _check_supported(basis)
    kpt = Hk.kpoint
    n = kpt.n_G
    _check_block("sternheimer_solver: psik", psik, n)
    _check_block("sternheimer_solver: rhs", rhs, n)
    n_occ = psik.shape[0]
    if rhs.shape[0] != n_occ:
        raise ValueError("sternheimer_solver: one right-hand side per column of psik")
    eps_h = np.ascontiguousarray(np.asarray(eps, dtype=np.float64).reshape(-1))
    if len(eps_h) != n_occ:
        raise ValueError("sternheimer_solver: one eigenvalue per column of psik")
    tol_h = np.ascontiguousarray(np.broadcast_to(np.asarray(tol, dtype=np.float64), (n_occ,)))
    n_extra = 0
    if psik_extra is not None and psik_extra.shape[0] > 0:
        _check_block("sternheimer_solver: psik_extra", psik_extra, n)
        n_extra = psik_extra.shape[0]
    if dpsik0 is not None:
        _check_block("sternheimer_solver: dpsik0", dpsik0, n)
        if dpsik0.shape[0] != n_occ:
            raise ValueError("sternheimer_solver: dpsik0 must have the shape of rhs")
    if out is not None:
        _check_block("sternheimer_solver: out", out, n)
        if out.shape[0] != n_occ:
            raise ValueError("sternheimer_solver: out must have the shape of rhs")
    dpsi = out if out is not None else torch.zeros((n_occ, n), dtype=torch.complex128, device=rhs.device)
    res = np.zeros(n_occ)
    n_iter, conv = C.c_int(0), C.c_int(1)
    if n_occ > 0:
        Hk.bind()
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_sternheimer(
            kpt.handle, n_occ, psik.data_ptr(), psik.stride(0), eps_h.ctypes.data, n_extra,
            psik_extra.data_ptr() if n_extra else None, psik_extra.stride(0) if n_extra else 0, rhs.data_ptr(), rhs.stride(0),
            tol_h.ctypes.data, int(miniter), int(maxiter), dpsik0.data_ptr() if dpsik0 is not None else None,
            dpsik0.stride(0) if dpsik0 is not None else 0, dpsi.data_ptr(), dpsi.stride(0), C.byref(n_iter),
            res.ctypes.data, C.byref(conv)))
        basis.post_call(kpt.lane)
    return dict(dpsik=dpsi, n_iter=int(n_iter.value), residual_norms=res, converged=bool(conv.value), tol=tol_h)


# ------------------------------------------------------------------------------------------ chi0
def compute_delta_occ(basis, psi, eF, eps, dHpsi, dtemperature=0.0):
    """``compute_docc!`` (chi0.jl:314-350): the derivatives of the occupations of the given (occupied) bands and of the Fermi
    level, ``(doccupation, deF)``.  A model with a fixed Fermi level (``model.eF``) keeps it; sums run over ``comm_kpts``."""
    from .exchange import refuse
    refuse(basis.model, "the density response")
    from .eigen import columnwise_dots
    model = basis.model
    T, kind, filled = model.temperature, model.smearing, model.filled_occupation
    docc = [np.zeros(len(e)) for e in eps]
    deF = 0.0
    if is_effective_insulator(basis, eps, eF):
        return docc, deF
    D = 0.0
    fps = []
    for ik, ek in enumerate(eps):
        ek = np.asarray(ek, dtype=float)
        if len(ek) == 0:
            fps.append(np.zeros(0))
            continue
        de = columnwise_dots(basis, psi[ik], dHpsi[ik]).real                     # d eps_nk = <psi_nk|dH|psi_nk>
        ered = (ek - eF) / T
        dered = de / T - ered * dtemperature / T
        fp = filled * occupation_derivative(kind, ered)
        fps.append(fp)
        docc[ik] = fp * dered
        D -= float(np.sum(fp)) * basis.kweights[ik] / T                          # the total DOS at the Fermi level
    comm = basis.comm_kpts
    tot = float(sum(w * float(np.sum(d)) for w, d in zip(basis.kweights, docc)))
    if comm.size > 1:
        D, tot = comm.sum_scalars([D, tot])
    if getattr(model, "eF", None) is None:
        deF = -tot / D
        for ik in range(len(eps)):
            docc[ik] = docc[ik] - fps[ik] * deF / T
    return docc, float(deF)


def _explicit_alpha(model, ek, eF):
    """alpha[m, n] of the explicit (computed-states) contribution to dpsi_n at q = 0 (chi0.jl:398-412); zero diagonal."""
    T, kind, filled = model.temperature, model.smearing, model.filled_occupation
    n = len(ek)
    alpha = np.zeros((n, n))
    if T == 0 or kind == "none":
        f = np.where(np.asarray(ek) < eF, filled, 0.0)      # (the reference evaluates occupation((e - eF) / 0): +-Inf)
    else:
        f = filled * _smear(kind, (np.asarray(ek, dtype=float) - eF) / T)
    for a in range(n):
        for m in range(n):
            if m == a:
                continue
            ratio = filled * occupation_divided_difference(kind, ek[m], ek[a], eF, T)
            alpha[m, a] = compute_alpha_mn(f[m], f[a], ratio)
    return alpha


def apply_chi0_4P(ham, psi, occupation, eF, eigenvalues, dHpsi, dtemperature=0.0, occupation_threshold=1e-6, q=None,
                  bandtolalg=None, tol=1e-9, dpsi0=None, miniter=1, maxiter=100):
    """``apply_chi0_4P`` (chi0.jl:436-503): orbital and occupation changes caused by the Hamiltonian change whose products
    with the orbitals are ``dHpsi``.  ``ham``: the list of ``DftHamiltonianBlock`` of the ground state.  Returns
    ``dict(dpsi, doccupation, deF, n_iter, residual_norms, converged)``; ``dpsi`` and ``doccupation`` are zero for the extra
    bands."""
    basis = ham[0].basis
    _check_supported(basis, q)
    model = basis.model
    masks = occupied_empty_masks(occupation, occupation_threshold)
    if bandtolalg is None:
        bandtolalg = BandtolBalanced(basis, psi, occupation, occupation_threshold=occupation_threshold)
    if bandtolalg.occupation_threshold != occupation_threshold:
        raise ValueError("apply_chi0_4P: bandtolalg was built for another occupation_threshold")
    bandtol = determine_band_tolerances(bandtolalg, tol)
    for ik, (n_occ, _) in enumerate(masks):
        _check_block("apply_chi0_4P: psi", psi[ik], basis.kpoints[ik].n_G)
        _check_block("apply_chi0_4P: dHpsi", dHpsi[ik], basis.kpoints[ik].n_G)
        if dHpsi[ik].shape != psi[ik].shape:
            raise ValueError("apply_chi0_4P: dHpsi must have the shape of psi")
    psi_occ = [psi[ik][:n] for ik, (n, _) in enumerate(masks)]
    psi_extra = [psi[ik][n:nb] for ik, (n, nb) in enumerate(masks)]
    eps_occ = [np.asarray(eigenvalues[ik], dtype=float)[:n] for ik, (n, _) in enumerate(masks)]
    dH_occ = [dHpsi[ik][:n] for ik, (n, _) in enumerate(masks)]

    docc_occ, deF = compute_delta_occ(basis, psi_occ, eF, eps_occ, dH_occ, dtemperature)
    doccupation = [np.zeros(len(o)) for o in occupation]
    for ik, (n, _) in enumerate(masks):
        doccupation[ik][:n] = docc_occ[ik]

    lib = basis.lib
    one, zero = _lib.cplx(1.0), _lib.cplx(0.0)

    def one_k(ik, _):
        kpt = basis.kpoints[ik]
        n_occ, _nb = masks[ik]
        out = torch.zeros_like(dHpsi[ik])
        if n_occ == 0:
            return out, dict(n_iter=0, residual_norms=np.zeros(0), converged=True)
        h = basis.lane_handles[kpt.lane]
        dp = out[:n_occ]
        res = sternheimer_solver(ham[ik], psi_occ[ik], eps_occ[ik], dH_occ[ik], psik_extra=psi_extra[ik], tol=bandtol[ik],
                                 miniter=miniter, maxiter=maxiter, dpsik0=None if dpsi0 is None else dpsi0[ik][:n_occ],
                                 out=dp)
        if model.temperature > 0 and model.smearing != "none":
            # explicit contribution of the computed states: dpsi_k += psi_k (alpha .* (psi_k' dHpsi_k))   (chi0.jl:413-416)
            alpha = _explicit_alpha(model, eps_occ[ik], eF)
            dots = torch.empty((n_occ, n_occ), dtype=torch.complex128, device=out.device)     # dots[n, m] = <psi_m|dH psi_n>
            basis.pre_call()
            _lib.check(lib.dftk_mi_zgemm(h, b"C", n_occ, n_occ, kpt.n_G, one, psi_occ[ik].data_ptr(), psi_occ[ik].stride(0),
                                         dH_occ[ik].data_ptr(), dH_occ[ik].stride(0), zero, dots.data_ptr(), n_occ))
            basis.post_call(kpt.lane)
            dots *= torch.as_tensor(alpha.T.copy(), device=out.device)
            basis.pre_call()
            _lib.check(lib.dftk_mi_zgemm(h, b"N", kpt.n_G, n_occ, n_occ, one, psi_occ[ik].data_ptr(), psi_occ[ik].stride(0),
                                         dots.data_ptr(), n_occ, one, dp.data_ptr(), dp.stride(0)))
            basis.post_call(kpt.lane)
        return out, res

    basis.pre_call()
    parts = basis.run_on_lanes(one_k, list(range(len(masks))))
    dpsi = [p[0] for p in parts]
    converged = all(p[1]["converged"] for p in parts)
    if basis.comm_kpts.size > 1:
        converged = all(bool(c) for c in basis.comm_kpts.gather_lists(converged))
    return dict(dpsi=dpsi, doccupation=doccupation, deF=deF, n_iter=[p[1]["n_iter"] for p in parts],
                residual_norms=[p[1]["residual_norms"] for p in parts], converged=converged)


def compute_delta_rho(basis, psi, dpsi, occupation, doccupation=None, occupation_threshold=0.0, q=None):
    """``compute_drho`` (densities.jl:60-108) at q = 0: the density change for orbital changes ``dpsi`` and occupation
    changes ``doccupation``, accumulated on the device (``dftk_mi_density_response_accumulate``), summed over lanes and
    ``comm_kpts`` and symmetrised as ``compute_density`` does."""
    _check_supported(basis, q)
    nx, ny, nz = basis.fft_size
    drhos = [torch.zeros((nz, ny, nx), dtype=torch.float64, device=basis.device) for _ in range(basis.n_lanes)]
    basis.pre_call()

    def accumulate(ik, kpt):
        occ = np.asarray(occupation[ik], dtype=np.float64)
        docc = np.zeros_like(occ) if doccupation is None else np.asarray(doccupation[ik], dtype=np.float64)
        keep = np.abs(occ) >= occupation_threshold
        scale = basis.kweights[ik] * basis.ifft_normalization ** 2
        wo = np.ascontiguousarray(np.where(keep, occ, 0.0) * scale)
        wd = np.ascontiguousarray(np.where(keep, docc, 0.0) * scale)
        _check_block("compute_delta_rho: psi", psi[ik], kpt.n_G)
        _check_block("compute_delta_rho: dpsi", dpsi[ik], kpt.n_G)
        nb = len(occ)
        if psi[ik].shape[0] < nb or dpsi[ik].shape[0] < nb:
            raise ValueError("compute_delta_rho: one orbital and one orbital change per occupation")
        _lib.check(basis.lib.dftk_mi_density_response_accumulate(kpt.handle, nb, psi[ik].data_ptr(), psi[ik].stride(0),
                                                                 dpsi[ik].data_ptr(), dpsi[ik].stride(0), wo.ctypes.data,
                                                                 wd.ctypes.data, drhos[kpt.lane].data_ptr()))
    basis.run_on_lanes(accumulate, basis.kpoints)
    drho = drhos[0]
    if basis.n_lanes > 1:
        basis.post_call()
        for r in drhos[1:]:
            drho += r
        basis.pre_call()
    if basis.comm_kpts.size > 1:
        basis.comm_kpts.sum_(drho, basis.stream_ptr)
    basis.post_call()
    return symmetrize_rho(basis, drho, do_lowpass=False)


def multiply_psi_by_potential(basis, psi, dV):
    """``dV psi`` for every k-point: the local part of the H apply (``which = 1``) of a temporary block that owns ``dV``.
    The ground-state blocks re-upload their potential on their next ``bind()``."""
    from .exchange import refuse
    refuse(basis.model, "the density response")
    dV = dV.to(torch.float64).contiguous()

    def one(ik, psik):
        blk = DftHamiltonianBlock(basis, basis.kpoints[ik], dV, bind=False)
        return blk.mul_(torch.empty_like(psik), psik, which=1)
    basis.pre_call()
    return basis.run_on_lanes(one, psi)


def apply_chi0(scfres_or_ham, *args, **kwargs):
    """``apply_chi0(scfres, dV; ...)`` / ``apply_chi0(ham, psi, occupation, eF, eigenvalues, dV; ...)`` (chi0.jl:505-557):
    the density change ``chi0 dV`` of the non-interacting system.  Keywords: ``dtemperature``, ``occupation_threshold``,
    ``q`` (must be zero), ``bandtolalg``, ``tol``, ``miniter``, ``maxiter``.  Returns ``dict(drho, norm_dH, dpsi,
    doccupation, deF, n_iter, residual_norms, converged)``."""
    if isinstance(scfres_or_ham, dict):
        res = scfres_or_ham
        (dV,) = args
        kwargs.setdefault("occupation_threshold", res["occupation_threshold"])
        return _apply_chi0(res["ham"], res["psi"], res["occupation"], res["eF"], res["eigenvalues"], dV, **kwargs)
    return _apply_chi0(scfres_or_ham, *args, **kwargs)


def _apply_chi0(ham, psi, occupation, eF, eigenvalues, dV, dtemperature=0.0, occupation_threshold=1e-6, q=None,
                bandtolalg=None, **kw_sternheimer):
    basis = ham[0].basis
    _check_supported(basis, q)
    if not (torch.is_tensor(dV) and dV.is_cuda and dV.dim() == 3):
        raise TypeError("apply_chi0: dV must be a real (nz, ny, nx) CUDA cube")
    with basis.on_library_stream():
        # the perturbation is made to respect the symmetry group of the basis and normalised (rhs of order 1)
        dV = symmetrize_rho(basis, dV.to(torch.float64).contiguous())
        norm_dH = float(torch.linalg.norm(dV).item())
        if norm_dH < EPS:
            basis.sync()
            return dict(drho=torch.zeros_like(dV), norm_dH=norm_dH)
        dV = dV / norm_dH
        if bandtolalg is None:
            bandtolalg = BandtolBalanced(basis, psi, occupation, occupation_threshold=occupation_threshold)
        if bandtolalg.guaranteed:
            bandtolalg = bandtolalg.scaled(1 / norm_dH)
        dHpsi = multiply_psi_by_potential(basis, psi, dV)
        res = apply_chi0_4P(ham, psi, occupation, eF, eigenvalues, dHpsi, dtemperature=dtemperature,
                            occupation_threshold=occupation_threshold, bandtolalg=bandtolalg, **kw_sternheimer)
        drho = compute_delta_rho(basis, psi, res["dpsi"], occupation, res["doccupation"],
                                 occupation_threshold=occupation_threshold)
        drho = drho * norm_dH
        basis.sync()
    return dict(res, drho=drho, norm_dH=norm_dH)


# ------------------------------------------------------------------------------------------ kernel
def apply_kernel(basis, drho, rho=None, RPA=False, q=None):
    """``apply_kernel(basis, drho; rho, RPA)``: dV = v_c * drho + f_xc(rho) drho, the Hartree and (unless ``RPA``) LDA
    exchange-correlation kernels of the model's terms in one library call (``dftk_mi_apply_kernel``)."""
    _check_supported(basis, q)
    T = basis.terms
    if T is None:
        raise ValueError("apply_kernel: the basis was built without terms")
    mask = 0
    if "Xc" in T.names and not RPA:
        for name in basis.model.functionals:
            if name in _KERNEL_LDA:
                mask |= _LDA_BITS[name]
            elif name in _GGA_BITS:
                raise NotImplementedError(f"apply_kernel: the kernel of the GGA functional {name} is not implemented")
            else:
                raise NotImplementedError(f"apply_kernel: the kernel of {name} is not implemented (closed forms exist for "
                                          f"{_KERNEL_LDA})")
        if rho is None:
            raise ValueError("apply_kernel: the exchange-correlation kernel needs the ground-state density rho")
    if not (torch.is_tensor(drho) and drho.is_cuda and drho.dim() == 3):
        raise TypeError("apply_kernel: drho must be a real (nz, ny, nx) CUDA cube")
    drho = drho.to(torch.float64).contiguous()
    rho_t = total_density(rho).to(torch.float64).contiguous() if (mask and rho is not None) else None
    if rho_t is not None and getattr(T, "rho_core", None) is not None:
        # non-linear core correction: f_xc is that of rho + rho_core (xc.jl:245-250); rho_d feeds f_xc alone, the Hartree
        # part acts on drho
        rho_t = rho_t + T.rho_core
    green = T.poisson if "Hartree" in T.names else None
    dV = torch.empty_like(drho)
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_apply_kernel(basis._cube_handle, rho_t.data_ptr() if rho_t is not None else None,
                                              drho.data_ptr(), green.data_ptr() if green is not None else None, mask,
                                              dV.data_ptr()))
    basis.post_call()
    return dV


# ------------------------------------------------------------------------------------------ self-consistent response
def solve_OmegaPlusK_split(scfres, dHextpsi, tol=1e-8, dtemperature=0.0, q=None, maxiter_sternheimer=100, maxiter=100,
                           krylovdim=20, factor_initial=0.1, factor_final=0.1, bandtolalg=None, RPA=False):
    """``solve_OmegaPlusK_split(scfres, dHextpsi; tol, ...)`` (hessian.jl:266-359, q = 0): the self-consistent response to
    an external perturbation given by its products ``dHextpsi`` with the orbitals.  d_rho0 = chi0 dH_ext; d_rho solves
    (1 - chi0 K) d_rho = d_rho0 by GMRES (every application is ``apply_chi0`` of ``apply_kernel``, Sternheimer tolerance
    ``tol / 10``); a final ``apply_chi0_4P`` with the induced potential added gives the orbital response.  Returns
    ``dict(dpsi, drho, dHpsi, dVind, drho0, deigenvalues, doccupation, deF, converged)``."""
    from .eigen import columnwise_dots
    basis = scfres["basis"]
    _check_supported(basis, q)
    ham, psi, occupation = scfres["ham"], scfres["psi"], scfres["occupation"]
    eF, eigenvalues, rho = scfres["eF"], scfres["eigenvalues"], scfres["rho"]
    thr = scfres["occupation_threshold"]
    if bandtolalg is None:
        bandtolalg = BandtolBalanced(basis, psi, occupation, occupation_threshold=thr)
    with basis.on_library_stream():
        res0 = apply_chi0_4P(ham, psi, occupation, eF, eigenvalues, dHextpsi, dtemperature=dtemperature,
                             occupation_threshold=thr, bandtolalg=bandtolalg, tol=tol * factor_initial,
                             maxiter=maxiter_sternheimer)
        drho0 = compute_delta_rho(basis, psi, res0["dpsi"], occupation, res0["doccupation"], occupation_threshold=thr)
        dpsi0 = res0["dpsi"]
        del res0

        def dielectric_adjoint(x):                   # (1 - chi0 K) x
            dV = apply_kernel(basis, x, rho, RPA=RPA)
            chi0dV = _apply_chi0(ham, psi, occupation, eF, eigenvalues, dV, occupation_threshold=thr,
                                 bandtolalg=bandtolalg, tol=tol * factor_final, maxiter=maxiter_sternheimer)["drho"]
            return x - chi0dV

        nrm0 = float(torch.linalg.norm(drho0).item())
        if nrm0 == 0.0:
            drho, ok = torch.zeros_like(drho0), True
        else:
            drho, ok = gmres(dielectric_adjoint, drho0, rtol=0.0, krylovdim=krylovdim, maxiter=maxiter, atol=tol)
        dVind = apply_kernel(basis, drho, rho, RPA=RPA)
        dVpsi = multiply_psi_by_potential(basis, psi, dVind)
        dHtotpsi = [a + b_ for a, b_ in zip(dVpsi, dHextpsi)]
        fin = apply_chi0_4P(ham, psi, occupation, eF, eigenvalues, dHtotpsi, dtemperature=dtemperature,
                            occupation_threshold=thr, bandtolalg=bandtolalg, tol=tol * factor_final,
                            maxiter=maxiter_sternheimer, dpsi0=dpsi0)
        deig = [columnwise_dots(basis, p, d).real for p, d in zip(psi, dHtotpsi)]
        basis.sync()
    return dict(dpsi=fin["dpsi"], drho=drho, dHpsi=dHtotpsi, dVind=dVind, drho0=drho0, deigenvalues=deig,
                doccupation=fin["doccupation"], deF=fin["deF"], converged=bool(ok) and fin["converged"])
