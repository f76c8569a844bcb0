"""direct_minimization on one Gamma-only cell: silicon_cell((n, n, n)) at Ecut 15 by default, general complex blocks.  The
solver runs a FIXED number of iterations (maxiter = K, a criterion that never holds) for two values of K from the same
random start; what is reported is the difference between the two runs divided by the difference of K, i.e. per iteration
without the set-up and the final Rayleigh-Ritz:

  * milliseconds per DM iteration (wall clock around the call, which ends with a synchronisation),
  * the share of the L-BFGS calls (dftk_mi_lbfgs_direction and dftk_mi_lbfgs_update, HIP events on the library's stream
    around every call) and the energy / gradient evaluations per iteration (line-search trials),
  * kernel launches and host synchronisations per iteration, and those of the L-BFGS calls alone (dftk_mi_launch_count),
  * beside these: one SCF step of the same cell (median of the steps of a short self_consistent_field run).

    python tools/dm_bench.py [--supercell 2] [--ecut 15] [--memory 10] [--k1 4] [--k2 12] [--out FILE]
"""
import argparse
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import _lib  # noqa: E402

dm = importlib.import_module("dftk_jl_amd.direct_minimization")      # (the package attribute of that name is the function)


def counters(lib):
    a, b = C.c_int64(), C.c_int64()
    _lib.check(lib.dftk_mi_launch_count(C.byref(a), C.byref(b)))
    return a.value, b.value


class Probe:
    """HIP events and the library's counters around every L-BFGS call of a run"""

    def __init__(self, lib):
        self.lib, self.pairs, self.launches, self.syncs, self.calls = lib, [], 0, 0, 0

    def wrap(self, fn):
        def inner(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            l0, s0 = counters(self.lib)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            l1, s1 = counters(self.lib)
            self.pairs.append((e0, e1))
            self.launches += l1 - l0
            self.syncs += s1 - s0
            self.calls += 1
            return out
        return inner

    def ms(self):
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.pairs)


def run(basis, K, memory):
    probe = Probe(basis.lib)
    upd, dire = dm.LbfgsNative.update, dm.LbfgsNative.direction
    dm.LbfgsNative.update, dm.LbfgsNative.direction = probe.wrap(upd), probe.wrap(dire)
    try:
        basis.sync()
        l0, s0 = counters(basis.lib)
        t0 = time.perf_counter()
        res = dftk.direct_minimization(basis, maxiter=K, memory=memory, is_converged=lambda info: False, seed=1)
        ms = 1e3 * (time.perf_counter() - t0)
        l1, s1 = counters(basis.lib)
    finally:
        dm.LbfgsNative.update, dm.LbfgsNative.direction = upd, dire
    assert res["n_iter"] == K
    return dict(ms=ms, launches=l1 - l0, syncs=s1 - s0, lbfgs_ms=probe.ms(), lbfgs_launches=probe.launches,
                lbfgs_syncs=probe.syncs, trials=sum(res["linesearch_trials"]), kept=sum(res["history_pairs_kept"]),
                E=res["energies"].total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--supercell", type=int, default=2)
    ap.add_argument("--ecut", type=float, default=15.0)
    ap.add_argument("--memory", type=int, default=10)
    ap.add_argument("--k1", type=int, default=4)
    ap.add_argument("--k2", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.supercell
    lat, atoms, pos = dftk.silicon_cell((n, n, n))
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
    basis = dftk.PlaneWaveBasis(model, args.ecut, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0", gamma_real=False)
    kpt = basis.kpoints[0]
    n_bands = dm.n_bands_full(model)
    run(basis, args.k1, args.memory)                       # sizes every workspace
    best = {}
    for K in (args.k1, args.k2):
        for _ in range(2):
            r = run(basis, K, args.memory)
            if K not in best or r["ms"] < best[K]["ms"]:
                best[K] = r
    dK = args.k2 - args.k1

    def per_iter(key):
        return (best[args.k2][key] - best[args.k1][key]) / dK
    scf = dftk.self_consistent_field(basis, tol=1e-14, maxiter=8)
    scf_ms = 1e3 * float(np.median(scf["timings"][2:]))
    vec_bytes = 16 * kpt.n_G * n_bands
    lines = [
        f"dm_bench: Si {n}x{n}x{n} ({len(atoms)} atoms), Ecut {args.ecut:g}, fft {basis.fft_size}, n_G {kpt.n_G}, "
        f"n_bands {n_bands}, memory {args.memory}: history {(2 * args.memory + 4) * vec_bytes / 2 ** 20:.1f} MiB",
        f"  per DM iteration (K = {args.k1} -> {args.k2}): {per_iter('ms'):.3f} ms with {per_iter('trials'):.2f} energy / "
        f"gradient evaluations; L-BFGS calls {per_iter('lbfgs_ms'):.3f} ms = {100 * per_iter('lbfgs_ms') / per_iter('ms'):.1f} %",
        f"  launches per iteration {per_iter('launches'):.1f} (L-BFGS calls {per_iter('lbfgs_launches'):.1f}), host "
        f"synchronisations per iteration {per_iter('syncs'):.1f} (L-BFGS calls {per_iter('lbfgs_syncs'):.2f})",
        f"  pairs kept {best[args.k2]['kept']} of {args.k2}; E after {args.k2} iterations {best[args.k2]['E']:.8f}",
        f"  one SCF step of the same cell: {scf_ms:.3f} ms (median of steps 3 .. {len(scf['timings'])})",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
