#!/usr/bin/env python
"""Newton's method after a loose SCF on the silicon example (examples/silicon.py): LDA, Ecut 7, a 4 x 4 x 4 k-mesh reduced by
the crystal's symmetries.  The SCF stops at 1e-3; ``newton`` takes its occupied orbitals to 1e-10 in a few second-order steps,
each one conjugate-gradient solve on the tangent space (the tolerances the response, refinement and phonon code wants, where
density mixing crawls).

    python examples/silicon_newton.py            (needs an MI355X; there is no CPU fallback)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402

lattice, atoms, positions = dftk.silicon_cell()
model = dftk.model_DFT(lattice, atoms, positions, functionals=("lda_x", "lda_c_pw"), symmetries=True)
basis = dftk.PlaneWaveBasis(model, 7, dftk.MonkhorstPack((4, 4, 4)))

scfres = dftk.self_consistent_field(basis, tol=1e-3)
print(f"SCF to 1e-3: {scfres['n_iter']} steps in {scfres['runtime']:.2f} s")
for i, (e, d) in enumerate(zip(scfres["history_Etot"], scfres["history_drho"]), start=1):
    print(f"  SCF    {i:3d}   E = {e:.12f}   |rho_out - rho_in| = {d:.2e}")

# Newton works on the occupied orbitals alone: the virtual ones are removed
psi0, _ = dftk.select_occupied_orbitals(basis, scfres["psi"], scfres["occupation"])


def show(info):
    if info.get("stage") == "iterate":
        print(f"  Newton {info['n_iter']:3d}   E = {info['history_Etot'][-1]:.12f}   |rho - rho_in| = {info['history_drho'][-1]:.2e}"
              f"   {info['cg_iterations'][-1]} CG iterations, residual {info['cg_residual_norms'][-1]:.1e}")


res = dftk.newton(basis, psi0, tol=1e-10, callback=show)
print(f"Newton to 1e-10: converged {res['converged']}, {res['n_iter']} steps in {res['runtime']:.2f} s, "
      f"{sum(res['cg_iterations'])} CG iterations, E = {res['energies'].total:.12f}")
print("forces (Newton result):")
print(dftk.compute_forces_cart(res))
