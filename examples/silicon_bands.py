#!/usr/bin/env python
"""Band structure and projected density of states of silicon: an LDA SCF on the 2-atom cell (Ecut 15, 4x4x4 mesh) with the
GTH pseudopotential written as a UPF file that carries two pseudo-atomic orbitals, 3S and 3P (Gaussians times r^l: the
generator of the test-suite, tests/pswfc_gen.py); the bands along L - Gamma - X - U | K - Gamma from the converged density
(``compute_bands`` with a ``KPath``), the indirect gap, the s and p weights of the top valence band at Gamma
(``atomic_orbital_projections``) and the projected density of states summed per angular momentum (``compute_pdos``,
``sum_pdos``).  Any norm-conserving UPF version 2 file with a PP_PSWFC block can be given instead.  No plotting:

    python examples/silicon_bands.py [path/to/Si.upf]          (needs an MI355X; there is no CPU fallback)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dftk_jl_amd as dftk  # noqa: E402
import pswfc_gen  # noqa: E402

HARTREE_EV = 27.211386245988

psp = dftk.load_psp(sys.argv[1]) if len(sys.argv) > 1 else pswfc_gen.pswfc_psp(("3S", "3P"))
print("pseudo-atomic orbitals:", [(psp.pswfc_label(i + 1, l), l) for l in range(psp.lmax + 1)
                                  for i in range(psp.count_n_pswfc_radial(l))])
lattice, _, positions = dftk.silicon_cell()
model = dftk.model_DFT(lattice, [dftk.ElementPsp("Si", psp=psp)] * 2, positions, functionals=("lda_x", "lda_c_pw"))
basis = dftk.PlaneWaveBasis(model, 15, dftk.MonkhorstPack((4, 4, 4)).reducible())
scfres = dftk.self_consistent_field(basis, tol=1e-8)
print(f"SCF: {scfres['n_iter']} iterations, total energy {scfres['energies'].total:.8f} Ha")

# fcc path in the reduced coordinates of the primitive cell
points = {"L": [0.5, 0.5, 0.5], "G": [0.0, 0.0, 0.0], "X": [0.5, 0.0, 0.5], "U": [0.625, 0.25, 0.625],
          "K": [0.375, 0.375, 0.75]}
kpath = dftk.KPath(points, [["L", "G", "X", "U"], ["K", "G"]])
bands = dftk.compute_bands(scfres, kpath, n_bands=8, kline_density=15, tol=1e-5)
ki = bands["kinter"]
print(f"{len(ki['kcoords'])} k-points along " + " - ".join(f"{name}@{ki['kdistances'][i]:.3f}" for i, name in ki["labels"]))
eig = np.array(bands["eigenvalues"])
i_v, i_c = int(np.argmax(eig[:, 3])), int(np.argmin(eig[:, 4]))
print(f"valence band maximum {eig[i_v, 3]:.5f} Ha at k = {np.round(ki['kcoords'][i_v], 3)}, conduction band minimum "
      f"{eig[i_c, 4]:.5f} Ha at k = {np.round(ki['kcoords'][i_c], 3)}: indirect gap {(eig[i_c, 4] - eig[i_v, 3]) * HARTREE_EV:.3f} eV, "
      f"direct gap at Gamma {(eig[i_v, 4] - eig[i_v, 3]) * HARTREE_EV:.3f} eV")

# fat bands: weight of every band at Gamma on the s and p orbitals of both atoms
projections, labels = dftk.atomic_orbital_projections(bands["basis"], bands["psi"])
i_gamma = [i for i, name in ki["labels"] if name == "G"][0]
w = projections[i_gamma].cpu().numpy()
s_cols = [j for j, o in enumerate(labels) if o["l"] == 0]
p_cols = [j for j, o in enumerate(labels) if o["l"] == 1]
for n in range(8):
    print(f"band {n + 1} at Gamma: {eig[i_gamma, n]:+.5f} Ha, s weight {w[n, s_cols].sum():.3f}, p weight {w[n, p_cols].sum():.3f}")

# projected density of states on the SCF mesh, Gaussian smearing of 0.01 Ha
eps = np.linspace(eig.min() - 0.05, eig[:, 4].min() + 0.1, 120)
pdos = dftk.compute_pdos(eps, scfres["basis"], scfres["psi"], scfres["eigenvalues"], smearing="gaussian", temperature=0.01)
s_sum = dftk.sum_pdos(pdos, [lambda o: o["l"] == 0])[:, 0]
p_sum = dftk.sum_pdos(pdos, [lambda o: o["l"] == 1])[:, 0]
step = eps[1] - eps[0]
print(f"PDOS integrated up to {eps[-1]:.3f} Ha: s {s_sum.sum() * step:.3f}, p {p_sum.sum() * step:.3f} electrons "
      f"(of {model.n_electrons}); s character peaks at {eps[np.argmax(s_sum)]:+.3f} Ha, p at {eps[np.argmax(p_sum)]:+.3f} Ha")
