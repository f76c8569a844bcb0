"""The exact-exchange apply (dftk_mi_exx_apply) on one Gamma-only block: silicon_cell((2, 2, 2)) at Ecut 15 by default (the
cell of tools/sternheimer_bench.py: fft 54^3, n_G 5961), 32 occupied orbitals applied to 35 columns, i.e. the sketch of one
ACE build.  Random orthonormal orbitals: the cost does not depend on their values.

Reported: milliseconds per call (HIP events on the library's stream, best of three), per (orbital, column) pair, launches
and host synchronisations per call -- beside the time of two pruned transforms per pair (one backward, one forward: stages
A ... E of the local H psi on the same block, tools/fft_bench.py's measurement in the same run), which is what a pair costs
at the least.

    python tools/exx_bench.py [--supercell 2] [--ecut 15] [--occ 32] [--cols 35] [--batch 8] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import _lib  # noqa: E402
import fft_bench  # noqa: E402


def counters(lib):
    a, b = C.c_int64(), C.c_int64()
    _lib.check(lib.dftk_mi_launch_count(C.byref(a), C.byref(b)))
    return a.value, b.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--supercell", type=int, default=2)
    ap.add_argument("--ecut", type=float, default=15.0)
    ap.add_argument("--occ", type=int, default=32)
    ap.add_argument("--cols", type=int, default=35)
    ap.add_argument("--batch", type=int, default=8, help="bands per FFT launch group")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.supercell
    lat, atoms, pos = dftk.silicon_cell((n, n, n))
    basis = dftk.PlaneWaveBasis(dftk.model_HF(lat, atoms, pos), args.ecut, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0")
    kpt = basis.kpoints[0]
    _lib.check(basis.lib.dftk_mi_basis_set_fft_batch(basis.handle, args.batch))
    g = torch.Generator(device="cuda").manual_seed(1)
    psi = dftk.ortho_qr(basis, dftk.random_orbitals(basis, kpt, args.cols, g))
    occ = np.full(args.occ, 2.0)
    out = torch.empty_like(psi)
    dftk.apply_exchange(basis, 0, psi[:args.occ], occ, psi, out=out)          # sizes the workspace
    basis.sync()
    best = None
    for _ in range(3):
        l0, s0 = counters(basis.lib)
        with basis.on_library_stream():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dftk.apply_exchange(basis, 0, psi[:args.occ], occ, psi, out=out)
            b.record()
            b.synchronize()
        l1, s1 = counters(basis.lib)
        rec = dict(ms=a.elapsed_time(b), launches=l1 - l0, syncs=s1 - s0)
        if best is None or rec["ms"] < best["ms"]:
            best = rec
    pairs = args.occ * args.cols
    nb = max(args.batch, 32)
    fft_ms = fft_bench.two_transforms_ms_per_band(fft_bench.stage_times(basis, nb, args.batch), nb)
    lines = [
        f"exx_bench: Si {n}x{n}x{n} ({len(atoms)} atoms), Ecut {args.ecut:g}, fft {basis.fft_size}, n_G {kpt.n_G}, "
        f"{args.occ} occupied x {args.cols} columns = {pairs} pairs, {args.batch} bands per launch group",
        f"  dftk_mi_exx_apply: {best['ms']:.2f} ms per call, {best['ms'] / pairs * 1e3:.2f} us per pair, "
        f"{best['launches']} launches, {best['syncs']} host synchronisations",
        f"  two pruned transforms (stages A ... E of the local H psi): {fft_ms * 1e3:.2f} us per band; "
        f"a pair costs {best['ms'] / pairs / fft_ms:.2f} times that",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
