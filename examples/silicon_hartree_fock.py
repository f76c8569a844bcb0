#!/usr/bin/env python
"""Exact exchange at the Gamma point: Hartree-Fock and the PBE0 hybrid on the two-atom silicon cell, started from the
converged LDA state.  The exchange operator of an SCF step is the adaptively compressed one (``AceExx()``) built from the
previous step's orbitals: two pruned transforms per (occupied orbital, orbital) pair in one library call
(``dftk_mi_exx_apply``), after which the eigensolver applies it as extra rows of the projector matrix.

    python examples/silicon_hartree_fock.py        (needs an MI355X; there is no CPU fallback)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402

lattice, atoms, positions = dftk.silicon_cell()
gamma = dftk.ExplicitKpoints([[0.0, 0.0, 0.0]], [1.0])
Ecut = 10

lda = dftk.PlaneWaveBasis(dftk.model_DFT(lattice, atoms, positions), Ecut, gamma)
print(f"fft_size {lda.fft_size}, {lda.kpoints[0].n_G} plane waves")
start = dftk.self_consistent_field(lda, tol=1e-8)
print(f"LDA   total energy {start['energies'].total:+.10f} Ha in {start['n_iter']} steps")

models = {
    "HF": dftk.model_HF(lattice, atoms, positions),                                   # Coulomb kernel, probe-charge G = 0
    "PBE0": dftk.model_DFT(lattice, atoms, positions, functionals=dftk.PBE0()),       # 0.75 PBE exchange + 0.25 exact
    "HF, short range": dftk.model_HF(lattice, atoms, positions, exx_kernel=dftk.ShortRangeCoulomb(0.2)),
}
for name, model in models.items():
    basis = dftk.PlaneWaveBasis(model, Ecut, gamma, fft_size=lda.fft_size)
    # plain damping: the orbitals that build the exchange operator lag one step behind the density
    res = dftk.self_consistent_field(basis, rho=start["rho"], psi=start["psi"], tol=1e-8, damping=0.4, anderson_m=0)
    E = res["energies"]
    eig = np.asarray(res["eigenvalues"][0])
    print(f"{name:16s} total energy {E.total:+.10f} Ha in {res['n_iter']} steps, exact exchange {E['ExactExchange']:+.8f}, "
          f"gap at Gamma {eig[4] - eig[3]:.4f} Ha")
    print("    " + ", ".join(f"{term} {value:+.6f}" for term, value in E.items()))
    F = dftk.compute_forces_cart(res)
    print(f"    largest force component {np.abs(F).max():.2e} Ha / bohr (zero by symmetry)")
