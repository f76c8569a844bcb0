#!/usr/bin/env python
"""First-order refinement of a cheap SCF on a larger basis (``refine_scfres``; Cances, Dusson, Kemlin, Levitt, SIAM J. Sci.
Comput. 44 (5), 2022): silicon with one atom displaced, LDA, the Gamma point.  The SCF runs at Ecut 15; its result is lifted
to the basis of Ecut 35 and corrected there by one Schur-split Newton step.  Printed: the errors of the energy, the density
and the forces against the SCF at Ecut 35, before and after the refinement.

    python examples/silicon_refine.py            (needs an MI355X; there is no CPU fallback)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402

lattice, atoms, positions = dftk.silicon_cell(a=2 * 5.131570667152971)
positions = [np.asarray(p, dtype=float).copy() for p in positions]
positions[0] += np.array([-0.022, 0.028, 0.035])            # displaced: the forces do not vanish
model = dftk.model_DFT(lattice, atoms, positions, functionals=("lda_x", "lda_c_pw"))
kgrid = dftk.MonkhorstPack((1, 1, 1))
tol = 1e-10

basis = dftk.PlaneWaveBasis(model, 15, kgrid)
scfres = dftk.self_consistent_field(basis, tol=tol)
basis_ref = dftk.PlaneWaveBasis(model, 35, kgrid)
print(f"Ecut 15: fft_size {basis.fft_size}, {basis.kpoints[0].n_G} plane waves; "
      f"Ecut 35: fft_size {basis_ref.fft_size}, {basis_ref.kpoints[0].n_G} plane waves")

refinement = dftk.refine_scfres(scfres, basis_ref, tol=tol)
energies = dftk.refine_energies(refinement)
E, dE = energies["E"], energies["dE"]
F, dF = dftk.refine_forces(refinement)

scfres_ref = dftk.self_consistent_field(basis_ref, tol=tol)      # the expensive calculation the refinement stands in for
E_ref = scfres_ref["energies"].total
rho_ref = scfres_ref["rho"]
F_ref = dftk.compute_forces(scfres_ref)


def rel(x, ref):
    x, ref = np.asarray(x, dtype=float), np.asarray(ref, dtype=float)
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


print(f"{'':10s} {'Ecut 15':>12s} {'refined':>12s}     (relative error against Ecut 35)")
print(f"{'energy':10s} {abs(E.total - E_ref) / abs(E_ref):12.3e} {abs(E.total + dE.total - E_ref) / abs(E_ref):12.3e}")
print(f"{'density':10s} {rel(refinement.rho.cpu().numpy(), rho_ref.cpu().numpy()):12.3e} "
      f"{rel((refinement.rho + refinement.drho).cpu().numpy(), rho_ref.cpu().numpy()):12.3e}")
print(f"{'forces':10s} {rel(F, F_ref):12.3e} {rel(F + dF, F_ref):12.3e}")
print("dE by term: " + ", ".join(f"{name} {value:+.3e}" for name, value in dE.items()))
