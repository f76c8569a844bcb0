#!/usr/bin/env python
"""Wannier90 input for the four valence bands of silicon: LDA, Ecut 7, a 4 x 4 x 4 k-mesh reduced by the crystal's symmetries.
The SCF runs on the irreducible wedge; ``write_wannier90_files`` unfolds it onto the full mesh (``unfold_bz``), finds the
finite-difference neighbours (``compute_nnkp``: no wannier90 run needed), and writes ``silicon.win / .nnkp / .eig / .amn /
.mmn`` with Gaussians on the four bond centres as initial guesses.  The spread functional is then evaluated here, without a
minimiser: Omega_I (gauge invariant), and the gauge-dependent part and the centres in the Kohn-Sham gauge the SCF happened
to return and in the projected gauge U_k = A_k (A_k' A_k)^{-1/2} that wannier90 starts from.

    python examples/silicon_wannier.py [output folder]            (needs an MI355X; there is no CPU fallback)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402

folder = sys.argv[1] if len(sys.argv) > 1 else "wannier_silicon"
lattice, atoms, positions = dftk.silicon_cell()
model = dftk.model_DFT(lattice, atoms, positions, functionals=("lda_x", "lda_c_pw"), symmetries=True)
basis = dftk.PlaneWaveBasis(model, 7, dftk.MonkhorstPack((4, 4, 4)))
scfres = dftk.self_consistent_field(basis, tol=1e-8)
print(f"SCF on {len(basis.kpoints)} irreducible k-points: {scfres['n_iter']} steps, E = {scfres['energies'].total:.10f}")

# the atom at (1/8, 1/8, 1/8) is bonded to the atom at -(1/8, 1/8, 1/8) and to its images by the three lattice vectors
bond_centres = [[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]]
projections = [dftk.GaussianWannierProjection(c) for c in bond_centres]
out = dftk.write_wannier90_files(scfres, os.path.join(folder, "silicon"), n_bands=4, n_wannier=4, projections=projections,
                                 num_iter=100)
nnkp, M, A = out["nnkp"], out["M"], out["A"]
print(f"unfolded onto {len(out['scfres']['basis'].kpoints)} k-points, {nnkp['nntot']} neighbours each; files in {folder}/: "
      f"{sorted(os.listdir(folder))}")

lat = np.asarray(lattice, dtype=float)
for name, overlaps in (("Kohn-Sham gauge", M), ("projected gauge", dftk.rotate_mmn(M, dftk.projection_gauge(A), nnkp))):
    s = dftk.wannier_spreads(overlaps, nnkp)
    print(f"{name}: Omega_I = {s['omega_I']:.6f}, Omega_OD = {s['omega_OD']:.6f}, Omega_D = {s['omega_D']:.6f} bohr^2")
    for n, (c, r2) in enumerate(zip(s["centers"], s["spreads"])):
        red = np.linalg.solve(lat, c)
        print(f"    function {n + 1}: centre {np.round(red - np.floor(red + 0.5 - 1e-6), 6) + 0.0} (reduced), spread {r2:.6f} bohr^2")
