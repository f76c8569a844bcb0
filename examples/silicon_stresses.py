#!/usr/bin/env python
"""The stress tensor of a slightly compressed, twisted silicon cell (the cell of test/stresses.jl of the reference with
a 1.02 instead of a 1.1 twist: integer occupations on a 2x2x2 mesh without a temperature): LDA, Ecut 15, SCF to 1e-8,
then sigma in Voigt order and the pressure.

    python examples/silicon_stresses.py            (needs an MI355X; there is no CPU fallback)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402

_, atoms, positions = dftk.silicon_cell()
a = 10.0                                                               # (equilibrium: 10.26 Bohr)
lattice = a / 2 * np.array([[0, 1, 1.02], [1, 0, 1], [1, 1, 0]])
model = dftk.model_DFT(lattice, atoms, positions, functionals=("lda_x", "lda_c_pw"), symmetries=True)
basis = dftk.PlaneWaveBasis(model, 15, dftk.MonkhorstPack((2, 2, 2)))
print(f"fft_size {basis.fft_size}, {len(basis.symmetries)} symmetries, {len(basis.kpoints)} irreducible k-points")
scfres = dftk.self_consistent_field(basis, tol=1e-8, callback=dftk.ScfDefaultCallback())
sigma = dftk.compute_stresses_cart(scfres)
HARTREE_PER_BOHR3_IN_GPA = 29421.02648438959
print("stress tensor (Hartree / bohr^3), Voigt order xx yy zz zy zx yx:")
print("   ", np.array2string(dftk.full_stress_to_voigt(sigma), precision=8))
for name in model.term_types:
    s = dftk.compute_stresses_term(name, basis, scfres["psi"], scfres["occupation"], rho=scfres["rho"])
    if s is not None:
        print(f"    {name:15s} {np.array2string(dftk.full_stress_to_voigt(s), precision=6)}   (unsymmetrised)")
p = -np.trace(sigma) / 3
print(f"pressure -tr sigma / 3 = {p:.8e} Hartree / bohr^3 = {p * HARTREE_PER_BOHR3_IN_GPA:.3f} GPa")
