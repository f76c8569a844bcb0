#!/usr/bin/env python
"""Phonon frequencies of silicon at the Gamma point from density-functional perturbation theory: an LDA SCF, then
``phonon_modes`` -- one self-consistent response (``solve_OmegaPlusK_split``) per displacement of an atom along a reduced
direction, the dynamical matrix from the explicit local / nonlocal / Ewald terms, and the generalised eigenproblem
D_cart v = omega^2 M v.  Three acoustic modes (zero up to the translation invariance the XC grid breaks) and the triply
degenerate optical mode.  The model is built with ``symmetries=False``: a displacement breaks the symmetries.

    python examples/silicon_phonons_gamma.py            (needs an MI355X; there is no CPU fallback)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402

HARTREE_TO_INV_CM = 219474.6313632

lattice, atoms, positions = dftk.silicon_cell()
model = dftk.model_DFT(lattice, atoms, positions, functionals=("lda_x", "lda_c_vwn"), symmetries=False)
basis = dftk.PlaneWaveBasis(model, 15, dftk.MonkhorstPack((2, 2, 2)))
print(f"fft_size {basis.fft_size}, {len(basis.kpoints)} k-points")
scfres = dftk.self_consistent_field(basis, tol=1e-10, callback=dftk.ScfDefaultCallback())

modes = dftk.phonon_modes(scfres, tol=1e-8)
D = modes["dynmat"]
n = len(model.atoms)
M = D.transpose(1, 0, 3, 2).reshape(3 * n, 3 * n)
print(f"dynamical matrix (reduced coordinates): max |D| = {np.abs(D).max():.6f}, max |D - D'| = {np.abs(M - M.T).max():.2e}, "
      f"acoustic sum rule residual {np.abs(D.sum(axis=1)).max():.2e}")
print("masses (electron masses):", np.diag(modes["mass_matrix"])[::3])
print("frequencies (cm^-1):", np.array2string(modes["frequencies"] * HARTREE_TO_INV_CM, precision=2))
