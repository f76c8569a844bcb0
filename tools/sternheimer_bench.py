"""The Sternheimer solver (dftk_mi_sternheimer) on one Gamma-only block: silicon_cell((2, 2, 2)) at Ecut 15 by default (16
atoms, 32 occupied bands), general complex block.  The orbitals come from one SCF, the right-hand side is a long-wavelength
cosine potential times the orbitals.  The solver runs a FIXED number of CG iterations (tol = 0, miniter = maxiter = K) for
two values of K; everything reported is the difference between the two runs divided by the difference of K, i.e. per CG
iteration without the set-up and the back-substitution:

  * milliseconds per iteration from HIP events on the library's stream,
  * the share of the H apply in them (profile family 9 of dftk_mi_prof_get, a second pair of runs with the profile on),
  * kernel launches and host synchronisations per iteration (dftk_mi_launch_count).

    python tools/sternheimer_bench.py [--supercell 2] [--ecut 15] [--extra 0] [--k1 5] [--k2 25] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import _lib  # noqa: E402


def counters(lib):
    a, b = C.c_int64(), C.c_int64()
    _lib.check(lib.dftk_mi_launch_count(C.byref(a), C.byref(b)))
    return a.value, b.value


def apply_h_ms(basis):
    ms, work, n = C.c_double(), C.c_double(), C.c_int64()
    _lib.check(basis.lib.dftk_mi_prof_get(basis.handle, 9, C.byref(ms), C.byref(work), C.byref(n)))
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--supercell", type=int, default=2)
    ap.add_argument("--ecut", type=float, default=15.0)
    ap.add_argument("--extra", type=int, default=0, help="extra (unoccupied) bands handed to the Schur split")
    ap.add_argument("--k1", type=int, default=5)
    ap.add_argument("--k2", type=int, default=25)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.supercell
    lat, atoms, pos = dftk.silicon_cell((n, n, n))
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
    basis = dftk.PlaneWaveBasis(model, args.ecut, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0", gamma_real=False)
    res = dftk.self_consistent_field(basis, tol=1e-8)
    kpt, Hk = basis.kpoints[0], res["ham"][0]
    n_occ = int(np.sum(np.asarray(res["occupation"][0]) > 1e-6))
    psi = res["psi"][0]
    n_extra = min(args.extra, psi.shape[0] - n_occ)
    nx, ny, nz = basis.fft_size
    x = torch.arange(nx, device="cuda:0", dtype=torch.float64) / nx
    dV = torch.cos(2 * np.pi * x)[None, None, :].expand(nz, ny, nx).contiguous()
    dV = dV / torch.linalg.norm(dV)
    rhs = dftk.multiply_psi_by_potential(basis, [psi], dV)[0][:n_occ]
    occ, extra = psi[:n_occ], (psi[n_occ:n_occ + n_extra] if n_extra else None)
    eps = np.asarray(res["eigenvalues"][0])[:n_occ]

    def solve(K):
        return dftk.sternheimer_solver(Hk, occ, eps, rhs, psik_extra=extra, tol=0.0, miniter=K, maxiter=K)

    solve(args.k2)                                     # sizes every workspace
    out = {}
    for profile in (0, 1):
        _lib.check(basis.lib.dftk_mi_prof_enable(basis.handle, profile))
        for K in (args.k1, args.k2):
            best = None
            for _ in range(3):
                l0, s0 = counters(basis.lib)
                h0 = apply_h_ms(basis) if profile else 0.0
                with basis.on_library_stream():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    r = solve(K)
                    b.record()
                    b.synchronize()
                assert r["n_iter"] == K
                l1, s1 = counters(basis.lib)
                rec = dict(ms=a.elapsed_time(b), launches=l1 - l0, syncs=s1 - s0,
                           apply_h_ms=(apply_h_ms(basis) - h0) if profile else 0.0)
                if best is None or rec["ms"] < best["ms"]:
                    best = rec
            out[(profile, K)] = best
    _lib.check(basis.lib.dftk_mi_prof_enable(basis.handle, 0))
    dK = args.k2 - args.k1

    def per_iter(profile, key):
        return (out[(profile, args.k2)][key] - out[(profile, args.k1)][key]) / dK
    ms = per_iter(0, "ms")
    share = per_iter(1, "apply_h_ms") / per_iter(1, "ms")
    full = dftk.sternheimer_solver(Hk, occ, eps, rhs, psik_extra=extra, tol=1e-9)
    lines = [
        f"sternheimer_bench: Si {n}x{n}x{n} ({len(atoms)} atoms), Ecut {args.ecut:g}, fft {basis.fft_size}, n_G {kpt.n_G}, "
        f"n_occ {n_occ}, n_extra {n_extra}, n_p {0 if basis.terms.P is None else basis.terms.P[0].shape[0]}",
        f"  per CG iteration (K = {args.k1} -> {args.k2}): {ms:.3f} ms, H apply share {100 * share:.1f} % "
        f"(profile on: {per_iter(1, 'ms'):.3f} ms of which H apply {per_iter(1, 'apply_h_ms'):.3f} ms), "
        f"not H apply {ms * (1 - share):.3f} ms",
        f"  launches per iteration {per_iter(0, 'launches'):.1f}, host synchronisations per iteration {per_iter(0, 'syncs'):.2f}",
        f"  whole call at K = {args.k2}: {out[(0, args.k2)]['ms']:.2f} ms, {out[(0, args.k2)]['launches']} launches, "
        f"{out[(0, args.k2)]['syncs']} host synchronisations",
        f"  solve to tol 1e-9: {full['n_iter']} iterations, converged {full['converged']}, "
        f"largest residual {float(np.max(full['residual_norms'])):.2e}",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
