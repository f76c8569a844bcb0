#!/usr/bin/env python
"""Silicon with a numeric (UPF) pseudopotential beside the HGH table: the GTH silicon pseudopotential is written as a
UPF 2.0.1 file on a 1141-point logarithmic mesh (the generator of the test-suite, tests/upf_gen.py), read back with
``load_psp(path)``, and LDA silicon (two atoms displaced off symmetry, Ecut 15, unreduced 2x2x2 mesh) is converged with both kinds;
the two total energies and the forces are printed side by side.  Any norm-conserving scalar-relativistic UPF version 2 file
can be given instead.  A third run shows the non-linear core correction: a file with a core density in PP_NLCC (the given
file if it has one, else the generated file with a made-up Gaussian core of charge 2 and decay length 0.45 bohr), with the
share of the Xc term in the forces, and the same file with ``use_nlcc=False``:

    python examples/silicon_upf.py [path/to/Si.upf]          (needs an MI355X; there is no CPU fallback)
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dftk_jl_amd as dftk  # noqa: E402
import upf_gen  # noqa: E402
from dftk_jl_amd.terms import atom_decay_length  # noqa: E402

hgh = dftk.load_psp("Si", "lda")
if len(sys.argv) > 1:
    path = sys.argv[1]
else:
    path = os.path.join(tempfile.mkdtemp(), "Si.gth-lda.upf")
    r = upf_gen.log_mesh(1141, 1e-5, 60.0)
    with open(path, "w") as fh:
        fh.write(upf_gen.write_upf(hgh, r, rhoatom=upf_gen.gaussian_density_real(4.0, atom_decay_length(10, 4), r)))
upf = dftk.load_psp(path)
print(f"{path}: Zion {upf.Zion}, lmax {upf.lmax}, {len(upf.rgrid)} mesh points, "
      f"{[upf.count_n_proj_radial(l) for l in range(upf.lmax + 1)]} projectors per l")

lattice, _, _ = dftk.silicon_cell()
positions = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]
results = {}
for name, psp in (("HGH", hgh), ("UPF", upf)):
    model = dftk.model_DFT(lattice, [dftk.ElementPsp("Si", psp=psp)] * 2, positions, functionals=("lda_x", "lda_c_pw"))
    basis = dftk.PlaneWaveBasis(model, 15, dftk.MonkhorstPack((2, 2, 2)).reducible())
    scfres = dftk.self_consistent_field(basis, tol=1e-9)
    results[name] = (scfres["energies"].total, dftk.compute_forces_cart(scfres))
for name, (E, F) in results.items():
    print(f"{name}: total energy {E:.10f} Ha; forces (Ha / bohr)")
    print("   ", np.array2string(F, precision=8, prefix="    "))
print(f"difference: {results['UPF'][0] - results['HGH'][0]:+.2e} Ha, "
      f"forces {np.max(np.abs(results['UPF'][1] - results['HGH'][1])):.2e} Ha / bohr")

# ---- non-linear core correction: rho_core joins rho in the XC term alone, and brings Xc forces with it
if upf.has_core_density():
    core = upf
else:
    r = upf_gen.log_mesh(1141, 1e-5, 60.0)
    core = dftk.parse_psp_upf(upf_gen.write_upf(hgh, r, rhoatom=upf_gen.gaussian_density_real(4.0, atom_decay_length(10, 4), r),
                                                core_correction=True, nlcc=upf_gen.gaussian_density_real(2.0, 0.45, r)),
                              identifier="Si.gth-lda.core.upf")
for use_nlcc in (True, False):
    model = dftk.model_DFT(lattice, [dftk.ElementPsp("Si", psp=core)] * 2, positions, functionals=("lda_x", "lda_c_pw"),
                           use_nlcc=use_nlcc)
    basis = dftk.PlaneWaveBasis(model, 15, dftk.MonkhorstPack((2, 2, 2)).reducible())
    scfres = dftk.self_consistent_field(basis, tol=1e-9)
    F = dftk.compute_forces(scfres)
    Fxc = dftk.compute_forces_term("Xc", basis, scfres["psi"], scfres["occupation"], rho=scfres["rho"])
    print(f"core density, use_nlcc={use_nlcc}: total energy {scfres['energies'].total:.10f} Ha, E_xc "
          f"{scfres['energies']['Xc']:.10f} Ha; largest force {np.max(np.abs(F)):.3e}, Xc share "
          f"{'none' if Fxc is None else f'{np.max(np.abs(Fxc)):.3e}'} (reduced coordinates)")
