#!/usr/bin/env python
"""The density response of silicon to a long-wavelength cosine potential dV(r) = A cos(2 pi x) (x the first reduced
coordinate): the bare response chi0 dV of the non-interacting electrons (``apply_chi0``: one Sternheimer solve per
k-point) and the self-consistent one, d_rho = chi0 (dV + K d_rho) with the Hartree + LDA kernel K
(``solve_OmegaPlusK_split``).  Screening shows as the ratio of the two.

    python examples/silicon_response.py            (needs an MI355X; there is no CPU fallback)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402

lattice, atoms, positions = dftk.silicon_cell()
model = dftk.model_DFT(lattice, atoms, positions, functionals=("lda_x", "lda_c_vwn"), symmetries=False)
basis = dftk.PlaneWaveBasis(model, 15, dftk.MonkhorstPack((2, 2, 2)))
print(f"fft_size {basis.fft_size}, {len(basis.kpoints)} k-points")
scfres = dftk.self_consistent_field(basis, tol=1e-9, callback=dftk.ScfDefaultCallback())

nx, ny, nz = basis.fft_size
A = 0.01
x = torch.arange(nx, dtype=torch.float64, device=basis.device) / nx
dV = (A * torch.cos(2 * np.pi * x))[None, None, :].expand(nz, ny, nx).contiguous()

bare = dftk.apply_chi0(scfres, dV, tol=1e-8)
print(f"bare response chi0 dV: max |d_rho| = {float(bare['drho'].abs().max()):.6e}, "
      f"<dV|chi0 dV> = {float((dV * bare['drho']).sum()) * basis.dvol:.6e}")
print(f"    Sternheimer iterations per k-point: {bare['n_iter']}, converged: {bare['converged']}")

dHpsi = dftk.multiply_psi_by_potential(basis, scfres["psi"], dV)
full = dftk.solve_OmegaPlusK_split(scfres, dHpsi, tol=1e-8)
print(f"self-consistent response: max |d_rho| = {float(full['drho'].abs().max()):.6e}, "
      f"<dV|d_rho> = {float((dV * full['drho']).sum()) * basis.dvol:.6e}, converged: {full['converged']}")
print(f"    induced potential: max |dV_ind| = {float(full['dVind'].abs().max()):.6e}")
print(f"    screening <dV|d_rho> / <dV|chi0 dV> = "
      f"{float((dV * full['drho']).sum()) / float((dV * bare['drho']).sum()):.4f}")
for ik, de in enumerate(full["deigenvalues"]):
    print(f"    k-point {ik}: first-order eigenvalues of the occupied bands {np.array2string(de[:4], precision=6)}")
