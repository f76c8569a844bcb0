"""Milliseconds per displacement of ``compute_dynmat`` at q = 0, split into its three parts: the perturbation dH psi
(``dftk_mi_local_potential_displacement`` + the local apply + ``dftk_mi_nonlocal_displacement_apply``; the three directions
of an atom are built together, the figure is a third of that), the self-consistent response (``solve_OmegaPlusK_split``)
and the contractions (``dftk_mi_forces_local`` of d_rho + ``dftk_mi_dynmat_nonlocal`` along (d_psi, d_occupation)); once per
matrix: the explicit Hessians (``dftk_mi_dynmat_local``, ``dftk_mi_dynmat_nonlocal``) and the host Ewald Hessian.  Host clock
around work that ends in a synchronisation of the basis' streams.  Silicon, LDA: the primitive cell on a k-mesh, or with
``--supercell n`` the n^3 supercell at Gamma.

    python tools/dynmat_bench.py [--ecut 15] [--kgrid 2] [--supercell 1] [--atoms 1] [--tol 1e-8] [--out profiles/dynmat_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import phonon  # noqa: E402
from dftk_jl_amd.forces import _forces_local  # noqa: E402
from dftk_jl_amd.terms import dynmat_ewald  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ecut", type=float, default=15.0)
    ap.add_argument("--kgrid", type=int, default=2)
    ap.add_argument("--supercell", type=int, default=1)
    ap.add_argument("--atoms", type=int, default=1, help="atoms whose three displacements are timed (after one warm-up atom)")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    n = args.supercell
    lat, atoms, pos = dftk.silicon_cell((n, n, n))
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"), symmetries=False)
    basis = dftk.PlaneWaveBasis(model, args.ecut, dftk.MonkhorstPack((args.kgrid,) * 3), device="cuda:0")
    t0 = time.time()
    res = dftk.self_consistent_field(basis, tol=1e-10)
    psi, occ, rho = res["psi"], res["occupation"], res["rho"]
    log(f"tools/dynmat_bench.py --ecut {args.ecut} --kgrid {args.kgrid} --supercell {n} --atoms {args.atoms} --tol {args.tol}; "
        f"library {dftk.load_library().dftk_mi_version().decode()}")
    log(f"{len(atoms)} atoms, fft {basis.fft_size}, {len(basis.kpoints)} k-points, n_G {basis.kpoints[0].n_G}, "
        f"{psi[0].shape[0]} bands; SCF {res['n_iter']} steps, {time.time() - t0:.1f} s")

    def timed(fn):
        basis.sync()
        t = time.time()
        out = fn()
        basis.sync()
        return out, (time.time() - t) * 1e3

    def perturbation(s):
        with basis.on_library_stream():
            return phonon._delta_H_psi_atom(basis, psi, s)

    def contract(r):
        with basis.on_library_stream():
            return (_forces_local(basis, r["drho"]),
                    phonon._dynmat_nonlocal(basis, psi, occ, r["dpsi"], r["doccupation"])[0])

    ms = dict(dH=[], response=[], contract=[])
    for s in range(min(max(args.atoms, 1) + 1, len(atoms))):
        dH, t_dH = timed(lambda: perturbation(s))
        for al in range(3):
            r, t_r = timed(lambda: dftk.solve_OmegaPlusK_split(res, dH[al], tol=args.tol))
            _, t_c = timed(lambda: contract(r))
            if s > 0:                       # (atom 0 is the warm-up)
                ms["response"].append(t_r)
                ms["contract"].append(t_c)
        if s > 0:
            ms["dH"].append(t_dH / 3)
    for key, what in (("dH", "dH psi (a third of one atom's three)"), ("response", "solve_OmegaPlusK_split"),
                      ("contract", "forces_local(d_rho) + dynmat_nonlocal(d_psi, d_occ)")):
        v = np.asarray(ms[key])
        if len(v):
            log(f"  per displacement: {what:55s} median {np.median(v):9.2f} ms   min {v.min():9.2f} ms   ({len(v)} samples)")

    def explicit():
        with basis.on_library_stream():
            return phonon._dynmat_local_explicit(basis, rho), phonon._dynmat_nonlocal(basis, psi, occ, hess=True)[1]
    explicit()
    _, t_e = timed(explicit)
    t = time.time()
    dynmat_ewald(model.lattice, [a.charge_ionic for a in model.atoms], model.positions)
    log(f"  once per matrix: explicit local + nonlocal Hessians {t_e:.2f} ms; Ewald Hessian (host numpy) "
        f"{(time.time() - t) * 1e3:.1f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
