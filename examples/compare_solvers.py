#!/usr/bin/env python
"""Comparison of the DFT solvers on silicon (the reference's examples/compare_solvers.jl): the density-based SCF, the
potential-based SCF with fixed and with adaptive damping, direct minimisation and Newton's method, all to the same tolerance
in the density.  LDA with the HGH pseudopotential, Ecut 5, a 3 x 3 x 3 k-mesh (Newton's method needs the exchange-correlation
kernel, which the library has for LDA).

    python examples/compare_solvers.py            (needs an MI355X; there is no CPU fallback)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402

lattice, atoms, positions = dftk.silicon_cell()
model = dftk.model_DFT(lattice, atoms, positions, functionals=("lda_x", "lda_c_pw"), symmetries=True)
basis = dftk.PlaneWaveBasis(model, 5, dftk.MonkhorstPack((3, 3, 3)))

tol = 1e-6          # convergence we desire in the density

# density-based self-consistent field
scfres_scf = dftk.self_consistent_field(basis, tol=tol)

# potential-based SCF: fixed damping, and the line search with adaptive damping (no damping to choose)
scfres_scfv = dftk.scf_potential_mixing(basis, tol=tol)
scfres_adaptive = dftk.scf_potential_mixing_adaptive(basis, tol=tol)

# direct minimisation
scfres_dm = dftk.direct_minimization(basis, tol=tol)

# Newton: start not too far from the solution -- a very crude SCF first -- and remove the virtual orbitals
scfres_start = dftk.self_consistent_field(basis, tol=0.5)
psi, _ = dftk.select_occupied_orbitals(basis, scfres_start["psi"], scfres_start["occupation"])
scfres_newton = dftk.newton(basis, psi, tol=tol)

runs = [("SCF (density mixing)", scfres_scf), ("SCF (potential mixing)", scfres_scfv),
        ("SCF (potential mixing, adaptive)", scfres_adaptive), ("direct minimisation", scfres_dm), ("Newton", scfres_newton)]
print(f"{'solver':34s} {'iterations':>10s} {'energy':>18s} {'runtime':>9s}")
for name, res in runs:
    print(f"{name:34s} {res['n_iter']:10d} {res['energies'].total:18.10f} {res['runtime']:8.2f}s")
print("accepted dampings of the adaptive run:", [round(float(a), 3) for a in scfres_adaptive["alphas"]],
      "trials per iteration:", scfres_adaptive["n_backtracks"])


def norm(x):
    return float(x.norm().item())


print("|rho_newton - rho_scf|      =", norm(scfres_newton["rho"] - scfres_scf["rho"]))
print("|rho_newton - rho_scfv|     =", norm(scfres_newton["rho"] - scfres_scfv["rho"]))
print("|rho_newton - rho_adaptive| =", norm(scfres_newton["rho"] - scfres_adaptive["rho"]))
print("|rho_newton - rho_dm|       =", norm(scfres_newton["rho"] - scfres_dm["rho"]))
