"""Newton's method on the occupied orbitals and the conjugate-gradient solve on their tangent space that it is made of (host
mirror of src/scf/newton.jl:79-158, ``solve_OmegaPlusK`` of src/response/hessian.jl:111-176 and ``cg!`` of
src/response/cg.jl for one right-hand side).

* ``TangentSpace``: what one solve keeps -- rho, the Hamiltonian at psi, Lambda_k = psi_k' H_k psi_k, the mean kinetic
  energies of the Teter-Payne-Allan preconditioner and, with the cache on, psi_n(r) of every band
  (``dftk_mi_orbitals_realspace``).  psi is fixed for the 10-50 iterations of a solve, so an application of K then costs two
  3-D transforms per band (``dftk_mi_tangent_density``, ``dftk_mi_tangent_potential``) where ``refine.apply_K`` pays four.
* ``apply_OmegaPlusK``: P [H d - d Lambda + dV[drho(d)] psi] with d = P dpsi -- one projection in, one out; P is linear and
  idempotent, so this is the operator ``refine.apply_Omega + refine.apply_K``.
* ``solve_OmegaPlusK_cg``: the reference's ``solve_OmegaPlusK``.  The packed-vector updates run behind
  ``dftk_mi_tangent_cg_*`` (csrc/newton_kernels.hip): alpha and beta are formed on the device, the host reads three scalars
  per iteration in one synchronisation.
* ``newton``: the driver.

Spellings are ASCII as in response.py / refine.py.  Orbital blocks are band-major ``(n_bands, n_G)`` complex128 CUDA tensors
in the full-sphere layout (a basis with the Gamma-real switch on included, as in direct_minimization).  Scope: the
intersection of what ``apply_kernel`` and ``direct_minimization`` accept -- spin-unpolarised LDA, HGH or UPF species with or
without non-linear core correction, zero temperature, full occupations, one rank; everything else is refused on
descriptors before any device work.
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np
import torch

from . import _lib
from . import refine as _refine
from .densities import compute_density
from .direct_minimization import check_supported as _dm_check_supported
from .packed import PackedHandle, mean_kin, rayleigh_ritz, sub_product
from .response import _check_block, apply_kernel, compute_delta_rho, multiply_psi_by_potential
from .symmetry import symmetrize_rho
from .terms import energy_hamiltonian

CG_GAMMA, CG_PC, CG_RR = 0, 1, 2          # DFTK_MI_CG_*: the named slots of dftk_mi_tangent_cg_dot
NEGATIVE_CURVATURE = ("newton: the tangent-space CG met <p, (Omega + K) p> <= 0: the Hessian is not positive definite at this "
                      "point.  As the reference warns, the starting point needs to be not too far from the solution "
                      "(converge an SCF or a direct minimisation further first)")


# ------------------------------------------------------------------------------------------ checks
def check_supported(basis, psi=None, who="newton"):
    """The refusals of this module, on descriptors alone (no device work): those of ``refine.check_supported`` (what
    ``apply_kernel`` lacks: ``NotImplementedError``), then those of ``direct_minimization.check_supported`` (a temperature,
    electrons that do not fill the bands, blocks of another shape: ``ValueError``).  Returns the number of bands."""
    _refine.check_supported(basis, who)
    return _dm_check_supported(basis, psi, who=who)


def _check_blocks(basis, who, name, blocks):
    if len(blocks) != len(basis.kpoints):
        raise ValueError(f"{who}: {name} has {len(blocks)} blocks, the basis {len(basis.kpoints)} k-blocks")
    for kpt, x in zip(basis.kpoints, blocks):
        _check_block(f"{who}: {name}", x, kpt.n_G)


# ------------------------------------------------------------------------------------------ tangent space
class TangentSpace:
    """``TangentSpace(basis, psi, occupation, cache_realspace="auto")``: the point that defines the tangent space and what a
    solve keeps there.  ``cache_realspace``: True keeps psi_n(r) of every band on the device (16 bytes per grid point and
    band), False runs the K part through ``compute_delta_rho`` / ``multiply_psi_by_potential``, ``"auto"`` turns the cache on
    when it needs at most half of the free device memory that ``torch.cuda.mem_get_info()`` reports now.  ``rho`` and
    ``ham``: the density and the Hamiltonian of ``psi`` where the caller has them already."""

    def __init__(self, basis, psi, occupation, cache_realspace="auto", rho=None, ham=None):
        check_supported(basis, None, "TangentSpace")
        _refine.check_full_occupation(basis, occupation)
        if cache_realspace not in (True, False, "auto"):
            raise ValueError("TangentSpace: cache_realspace is True, False or 'auto'")
        basis._require_gpu()
        _check_blocks(basis, "TangentSpace", "psi", psi)
        self.basis = basis
        self.psi = [p.contiguous() for p in psi]
        self.occupation = [np.asarray(o, dtype=np.float64) for o in occupation]
        self.rho = compute_density(basis, self.psi, self.occupation) if rho is None else rho
        self.ham = energy_hamiltonian(basis, self.psi, self.occupation, rho=self.rho)[1] if ham is None else ham
        self.Lambda = _refine.rayleigh_coefficients(self.ham, self.psi)
        self.mean_kin = mean_kin(basis, self.psi)
        self.n_apply = 0
        nx, ny, nz = basis.fft_size
        need = sum(p.shape[0] for p in self.psi) * nx * ny * nz * 16
        if cache_realspace == "auto":
            cache_realspace = need <= torch.cuda.mem_get_info(basis.device)[0] // 2
        self.cache_bytes = need if cache_realspace else 0
        self.psi_r = None
        if cache_realspace:
            self.psi_r = [torch.empty((p.shape[0], nz, ny, nx), dtype=torch.complex128, device=basis.device) for p in self.psi]
            basis.pre_call()

            def fill(ik, kpt):
                p = self.psi[ik]
                _lib.check(basis.lib.dftk_mi_orbitals_realspace(kpt.handle, p.shape[0], p.data_ptr(), p.stride(0),
                                                                self.psi_r[ik].data_ptr()))
            basis.run_on_lanes(fill, basis.kpoints)
            basis.post_call()

    # the density change of d, symmetrised and summed over lanes exactly as compute_delta_rho does
    def _delta_rho(self, d):
        basis = self.basis
        if self.psi_r is None:
            return compute_delta_rho(basis, self.psi, d, self.occupation)
        nx, ny, nz = basis.fft_size
        drhos = [torch.zeros((nz, ny, nx), dtype=torch.float64, device=basis.device) for _ in range(basis.n_lanes)]
        basis.pre_call()

        def accumulate(ik, kpt):
            w = np.ascontiguousarray(self.occupation[ik] * (basis.kweights[ik] * basis.ifft_normalization ** 2))
            _lib.check(basis.lib.dftk_mi_tangent_density(kpt.handle, len(w), self.psi_r[ik].data_ptr(), d[ik].data_ptr(),
                                                         d[ik].stride(0), w.ctypes.data, drhos[kpt.lane].data_ptr()))
        basis.run_on_lanes(accumulate, basis.kpoints)
        drho = drhos[0]
        if basis.n_lanes > 1:
            basis.post_call()
            for r in drhos[1:]:
                drho += r
            basis.pre_call()
        basis.post_call()
        return symmetrize_rho(basis, drho, do_lowpass=False)

    def projected_gradient(self):
        """``compute_projected_gradient`` with the Hamiltonian held here: the blocks (1 - psi_k psi_k') H_k psi_k"""
        return [_refine.proj_tangent_kpt_(self.basis, kpt, Hk @ p, p)
                for kpt, Hk, p in zip(self.basis.kpoints, self.ham, self.psi)]

    def project(self, x):
        """P x as new blocks"""
        return _refine.proj_tangent(self.basis, x, self.psi)

    def precondition(self, r):
        """the preconditioner of ``solve_OmegaPlusK``: P T^-1 P r, T the Teter-Payne-Allan form prepared at psi"""
        basis = self.basis
        out = []
        for kpt, t, p, mk in zip(basis.kpoints, self.project(r), self.psi, self.mean_kin):
            y = torch.empty_like(t)
            basis.pre_call()
            _lib.check(basis.lib.dftk_mi_tpa_ldiv(kpt.handle, t.shape[0], t.data_ptr(), t.stride(0), mk.ctypes.data, 1.0,
                                                  y.data_ptr(), y.stride(0)))
            basis.post_call(kpt.lane)
            out.append(_refine.proj_tangent_kpt_(basis, kpt, y, p))
        return out


def apply_OmegaPlusK(ts, dpsi):
    """``(Omega + K) dpsi`` at the point of ``ts``: P [H d - d Lambda + dV[drho(d)] psi] with d = P dpsi, as new blocks."""
    basis = ts.basis
    _check_blocks(basis, "apply_OmegaPlusK", "dpsi", dpsi)
    d = ts.project(dpsi)
    dV = apply_kernel(basis, ts._delta_rho(d), ts.rho)
    out = []
    for kpt, Hk, dk, L in zip(basis.kpoints, ts.ham, d, ts.Lambda):
        Od = Hk @ dk
        out.append(sub_product(basis, kpt, Od, dk, L))
    if ts.psi_r is not None:
        dV = dV.to(torch.float64).contiguous()
        basis.pre_call()

        def add_K(ik, kpt):
            o = out[ik]
            _lib.check(basis.lib.dftk_mi_tangent_potential(kpt.handle, o.shape[0], ts.psi_r[ik].data_ptr(), dV.data_ptr(),
                                                           o.data_ptr(), o.stride(0), 1))
        basis.run_on_lanes(add_K, basis.kpoints)
        basis.post_call()
    else:
        for o, Kd in zip(out, multiply_psi_by_potential(basis, ts.psi, dV)):
            o += Kd
    ts.n_apply += 1
    return [_refine.proj_tangent_kpt_(basis, kpt, o, p) for kpt, o, p in zip(basis.kpoints, out, ts.psi)]


# ------------------------------------------------------------------------------------------ packed-vector CG
class TangentCgNative(PackedHandle):
    """The scalars of ``cg!`` behind the C ABI (``dftk_mi_tangent_cg_*``) for packed vectors shaped like ``shapes``
    (band-major ``(n_bands, n_G)``) with one weight per block."""

    def __init__(self, basis, shapes, weights):
        w = (C.c_double * len(shapes))(*[float(x) for x in weights])
        super().__init__(basis, shapes, "dftk_mi_tangent_cg_create", w)

    def dot(self, slot, a, b):
        self._call("dftk_mi_tangent_cg_dot", int(slot), *self._tables(a, b), post=False)

    def update_xr(self, p, c, x, r):
        self._call("dftk_mi_tangent_cg_update_xr", *self._tables(p, c, x, r))

    def update_p(self, z, p, first=False):
        self._call("dftk_mi_tangent_cg_update_p", *self._tables(z, p), 1 if first else 0)

    def read(self):
        """-> (<r, r>, gamma, <p, c>): the one host synchronisation of an iteration"""
        out = (C.c_double * 3)()
        _lib.check(self.basis.lib.dftk_mi_tangent_cg_read(self.handle, out))
        return float(out[0]), float(out[1]), float(out[2])


def solve_OmegaPlusK_cg(basis, psi, dHext_psi, occupation, tol=1e-10, maxiter=100, miniter=1, callback=None,
                        cache_realspace="auto", tangent_space=None):
    """``solve_OmegaPlusK(basis, psi, dHext_psi, occupation; callback, tol)`` (hessian.jl:111-176): dpsi on the tangent space
    at psi with (Omega + K) dpsi = -P dHext_psi, the sign convention of ``solve_OmegaPlusK_split``, by the preconditioned CG
    of cg.jl in the order of ``cg!`` for one right-hand side (no column locking): inner product sum_k w_k Re <x_k, y_k>,
    preconditioner P T^-1 P with T the Teter-Payne-Allan form prepared at psi, iterates projected after every update.
    ``tangent_space``: a ``TangentSpace`` of (psi, occupation) built earlier.  ``callback(info)`` gets a dict per iteration
    (``n_iter``, ``residual_norms``, ``x``, ``r``, ``converged``, ``stage``, ``basis``).  Returns ``dict(dpsi, converged, tol,
    residual_norms, n_iter, negative_curvature, residual_history, n_apply)``; ``negative_curvature``: the scalars read back
    showed <p, (Omega + K) p> <= 0 and the solve ended there, not converged."""
    who = "solve_OmegaPlusK_cg"
    check_supported(basis, None, who)
    _refine.check_full_occupation(basis, occupation)
    basis._require_gpu()
    _check_blocks(basis, who, "psi", psi)
    for p, occ in zip(psi, occupation):
        if p.shape[0] != len(occ):
            raise ValueError(f"{who}: one occupation per orbital (remove the virtual orbitals with select_occupied_orbitals)")
    _check_blocks(basis, who, "dHext_psi", dHext_psi)
    for p, rhs in zip(psi, dHext_psi):
        if rhs.shape != p.shape:
            raise ValueError(f"{who}: dHext_psi must have the shape of psi")
    tol = float(tol)

    with basis.on_library_stream():
        ts = tangent_space if tangent_space is not None else TangentSpace(basis, psi, occupation, cache_realspace)
        n0 = ts.n_apply
        cg = TangentCgNative(basis, [p.shape for p in ts.psi], basis.kweights)
        try:
            r = [-x for x in ts.project(dHext_psi)]                    # r = b - A 0
            x = [torch.zeros_like(v) for v in r]
            c = ts.precondition(r)
            p = [torch.empty_like(v) for v in r]
            cg.dot(CG_GAMMA, r, c)
            cg.dot(CG_RR, r, r)
            cg.update_p(c, p, first=True)                              # p = c; gamma = <r, c>
            rr, gamma, _ = cg.read()
            history = [math.sqrt(max(rr, 0.0))]
            n_iter, converged, negative = 0, False, False
            while n_iter < maxiter:
                if callback is not None:
                    callback(dict(basis=basis, n_iter=n_iter, x=x, r=r, residual_norms=np.array([history[-1]]),
                                  converged=converged, stage="iterate"))
                n_iter += 1
                if n_iter >= miniter and history[-1] <= tol:
                    converged = True
                    break
                c = apply_OmegaPlusK(ts, p)
                cg.dot(CG_PC, p, c)
                cg.update_xr(p, c, x, r)                               # alpha = gamma / <p, c> on the device
                for kpt, xk, rk, pk in zip(basis.kpoints, x, r, ts.psi):
                    _refine.proj_tangent_kpt_(basis, kpt, xk, pk)
                    _refine.proj_tangent_kpt_(basis, kpt, rk, pk)
                cg.dot(CG_RR, r, r)
                c = ts.precondition(r)
                cg.dot(CG_GAMMA, r, c)
                cg.update_p(c, p)                                      # beta = gamma_new / gamma_old on the device
                for kpt, qk, pk in zip(basis.kpoints, p, ts.psi):
                    _refine.proj_tangent_kpt_(basis, kpt, qk, pk)
                rr, gamma, pc = cg.read()
                history.append(math.sqrt(max(rr, 0.0)) if rr == rr else math.nan)
                if not pc > 0:
                    negative = True
                    break
            basis.sync()
        finally:
            cg.close()
    result = dict(dpsi=x, converged=converged, tol=tol, residual_norms=np.array([history[-1]]), n_iter=n_iter,
                  negative_curvature=negative, residual_history=history, n_apply=ts.n_apply - n0, maxiter=maxiter,
                  stage="finalize")
    if callback is not None:
        callback(dict(result, basis=basis, x=x))
    return result


# ------------------------------------------------------------------------------------------ driver
def newton(basis, psi0, tol=1e-6, tol_cg=None, maxiter=20, callback=None, is_converged=None, seed=None,
           cache_realspace="auto"):
    """``newton(basis, psi0; tol, tol_cg, maxiter, callback, is_converged, seed)`` (newton.jl:79-158).  ``psi0``: the
    occupied orbitals (no virtual ones: ``select_occupied_orbitals``); the start needs to be not too far from the solution.
    Every iteration solves (Omega + K) dpsi = -(projected gradient) to ``tol_cg`` (default ``tol / 100``), takes
    psi_k <- ortho_qr(psi_k + dpsi_k) and builds the new density, energies and Hamiltonian; convergence is
    ``ScfConvergenceDensity(tol)`` on |rho - rho_in| sqrt(dvol).  Returns a dict with the keys of the ``direct_minimization``
    result that post-processing reads, ``algorithm="Newton"``, and per Newton step ``cg_iterations`` and
    ``cg_residual_norms``.  ``RuntimeError`` when a solve meets negative curvature."""
    if psi0 is None:
        raise ValueError("newton: psi0 is required (the occupied orbitals of a start not too far from the solution)")
    n_bands = check_supported(basis, psi0, "newton")
    if cache_realspace not in (True, False, "auto"):
        raise ValueError("newton: cache_realspace is True, False or 'auto'")
    basis._require_gpu()
    from .eigen import ortho_qr
    t0 = time.time()
    filled = basis.model.filled_occupation
    tol_cg = tol / 100 if tol_cg is None else tol_cg
    is_converged = is_converged or (lambda info: info["history_drho"][-1] < tol)       # ScfConvergenceDensity
    occupation = [np.full(n_bands, float(filled)) for _ in basis.kpoints]
    sqrt_dvol = math.sqrt(basis.dvol)
    n_iter, converged = 0, False
    history_Etot, history_drho, cg_iterations, cg_residual_norms = [], [], [], []

    with basis.on_library_stream():
        psi = [p.to(device=basis.device, dtype=torch.complex128).clone().contiguous() for p in psi0]
        rho_in = compute_density(basis, psi, occupation)
        energies, ham = energy_hamiltonian(basis, psi, occupation, rho=rho_in)
        while not converged and n_iter < maxiter:
            n_iter += 1
            # the Newton step psi <- psi + dpsi with (Omega + K) dpsi = -res; density and Hamiltonian of psi are at hand
            ts = TangentSpace(basis, psi, occupation, cache_realspace, rho=rho_in, ham=ham)
            res = ts.projected_gradient()
            sol = solve_OmegaPlusK_cg(basis, psi, res, occupation, tol=tol_cg, tangent_space=ts)
            cg_iterations.append(int(sol["n_iter"]))
            cg_residual_norms.append(float(sol["residual_norms"][0]))
            if sol["negative_curvature"]:
                raise RuntimeError(NEGATIVE_CURVATURE + f" (Newton step {n_iter}, CG iteration {sol['n_iter']})")
            psi = [ortho_qr(basis, p + d) for p, d in zip(psi, sol["dpsi"])]
            del ts, sol

            rho = compute_density(basis, psi, occupation)
            energies, ham = energy_hamiltonian(basis, psi, occupation, rho=rho)
            history_drho.append(float(torch.linalg.norm(rho - rho_in).item()) * sqrt_dvol)
            history_Etot.append(energies.total)
            info = dict(ham=ham, basis=basis, converged=converged, stage="iterate", rho_in=rho_in, rho=rho, n_iter=n_iter,
                        energies=energies, algorithm="Newton", runtime=time.time() - t0, history_drho=history_drho,
                        history_Etot=history_Etot, psi=psi, occupation=occupation, cg_iterations=cg_iterations,
                        cg_residual_norms=cg_residual_norms)
            if callback is not None:
                callback(info)
            converged = bool(is_converged(info))
            rho_in = rho

        eigenvalues, psi_rr = rayleigh_ritz(basis, ham, psi)
        basis.sync()

    result = dict(basis=basis, ham=ham, energies=energies, converged=converged, rho=rho_in, psi=psi_rr,
                  eigenvalues=eigenvalues, occupation=occupation, eF=None, n_bands_converge=n_bands, n_iter=n_iter,
                  history_Etot=history_Etot, history_drho=history_drho, algorithm="Newton", seed=seed,
                  runtime=time.time() - t0, cg_iterations=cg_iterations, cg_residual_norms=cg_residual_norms,
                  stage="finalize")
    if callback is not None:
        callback(result)
    return result
