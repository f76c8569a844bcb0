"""Milliseconds per k-point of the three passes of the Wannier interface on silicon (LDA, 4 x 4 x 4 mesh, Ecut 7 by default,
4 bands, bond-centred Gaussians): the unfolding of an irreducible SCF result (``unfold_array``: one ``dftk_mi_apply_symop``
per full-mesh k-point, its k-block included), the overlaps (``compute_mmn``: one ``dftk_mi_wannier_overlaps`` per k-point
for all its neighbours) and the projections (``compute_amn``: guess columns and one zgemm per k-point).  Wall time around
the whole pass, device idle before and after, best of the repeats, divided by the number of full-mesh k-points; kernel
launches and host synchronisations per k-point beside it.

    python tools/wannier_bench.py [--ecut 7] [--mesh 4] [--bands 4] [--repeats 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import _lib  # noqa: E402


def counters(lib):
    a, b = C.c_int64(), C.c_int64()
    _lib.check(lib.dftk_mi_launch_count(C.byref(a), C.byref(b)))
    return a.value, b.value


def timed(basis, fn, repeats):
    best = None
    for _ in range(repeats + 1):                     # the first run builds the tables the blocks keep
        basis.sync()
        l0, s0 = counters(basis.lib)
        t0 = time.perf_counter()
        out = fn()
        basis.sync()
        ms = 1e3 * (time.perf_counter() - t0)
        l1, s1 = counters(basis.lib)
        if best is None or ms < best[0]:
            best = (ms, l1 - l0, s1 - s0)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ecut", type=float, default=7.0)
    ap.add_argument("--mesh", type=int, default=4)
    ap.add_argument("--bands", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lat, atoms, pos = dftk.silicon_cell()
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_pw"), symmetries=True)
    basis = dftk.PlaneWaveBasis(model, args.ecut, dftk.MonkhorstPack((args.mesh,) * 3))
    scfres = dftk.self_consistent_field(basis, tol=1e-8)
    full = dftk.unfold_bz(basis)
    n_k = len(full.kpoints)
    projections = [dftk.GaussianWannierProjection(c) for c in ([0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5])]
    nnkp = dftk.compute_nnkp(full)
    psi, t_unfold = timed(basis, lambda: dftk.unfold_array(basis, full, scfres["psi"], True), args.repeats)
    _, t_mmn = timed(full, lambda: dftk.compute_mmn(full, psi, nnkp, args.bands), args.repeats)
    _, t_amn = timed(full, lambda: dftk.compute_amn(full, psi, projections, args.bands), args.repeats)
    lines = [f"wannier_bench: Si, Ecut {args.ecut:g}, {args.mesh}^3 mesh: {len(basis.kpoints)} irreducible -> {n_k} k-points, "
             f"n_G about {full.kpoints[0].n_G}, {args.bands} bands, {nnkp['nntot']} neighbours, {len(projections)} projections"]
    for name, (ms, launches, syncs) in (("unfold (apply_symop)", t_unfold), ("Mmn (wannier_overlaps)", t_mmn),
                                        ("Amn (guess columns + zgemm)", t_amn)):
        lines.append(f"  {name}: {ms / n_k:.3f} ms per k-point, {launches / n_k:.1f} launches, {syncs / n_k:.1f} host "
                     f"synchronisations per k-point ({ms:.1f} ms for the pass, host-side work included)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
