#!/usr/bin/env python
"""Direct minimisation beside the SCF on the silicon example (examples/silicon.py): LDA, Ecut 7, a 4 x 4 x 4 k-mesh reduced by
the crystal's symmetries.  ``direct_minimization`` minimises the energy over the occupied orbitals by preconditioned L-BFGS on
the device (no density mixing, no eigensolver: the route for insulators on which mixing stalls); both solvers must land on
the same ground state.

    python examples/silicon_direct_minimization.py            (needs an MI355X; there is no CPU fallback)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402

lattice, atoms, positions = dftk.silicon_cell()
model = dftk.model_DFT(lattice, atoms, positions, functionals=("lda_x", "lda_c_pw"), symmetries=True)
basis = dftk.PlaneWaveBasis(model, 7, dftk.MonkhorstPack((4, 4, 4)))
tol = 1e-7

scfres = dftk.self_consistent_field(basis, tol=tol / 10)


def show(info):
    if info.get("stage") == "iterate":
        print(f"  DM {info['n_iter']:3d}   E = {info['history_Etot'][-1]:.12f}   |rho_out - rho| = {info['history_drho'][-1]:.2e}")


dmres = dftk.direct_minimization(basis, tol=tol, callback=show)

print(f"SCF: {scfres['n_iter']} steps in {scfres['runtime']:.2f} s, E = {scfres['energies'].total:.10f}")
print(f"DM : {dmres['n_iter']} iterations in {dmres['runtime']:.2f} s, E = {dmres['energies'].total:.10f}, "
      f"{sum(dmres['linesearch_trials'])} energy evaluations in line searches, "
      f"{sum(dmres['history_pairs_kept'])} of {dmres['n_iter']} pairs kept")
print(f"max |rho_DM - rho_SCF| = {float((dmres['rho'] - scfres['rho']).abs().max().item()):.2e}")
for ik, (a, b) in enumerate(zip(dmres["eigenvalues"], scfres["eigenvalues"])):
    print(f"k-point {ik}: max |eigenvalue difference| over the occupied bands = {np.abs(a - np.asarray(b)[:len(a)]).max():.2e}")
print("forces (DM result):")
print(dftk.compute_forces_cart(dmres))
