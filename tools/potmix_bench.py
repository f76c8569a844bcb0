"""scf_potential_mixing_adaptive beside the density-mixing SCF on Gamma-only silicon cells: silicon_cell((n, n, n)) at Ecut 15
by default (n = 2: 16 atoms, n = 3: 54 atoms), in the same run on the same basis:

  * milliseconds per ScfStepper step (wall time of step(), which ends with a synchronisation; median without the first two),
  * milliseconds per iteration of the potential-mixing SCF (time between two callbacks; median without the first two) and per
    trial step (the same time over the number of trials; a trial is one diagonalisation, one density, one energy evaluation),
  * the scalar block of a trial step alone: kernel launches and host synchronisations of the one ``dftk_mi_diff_dots`` call
    (dftk_mi_launch_count) and its milliseconds beside those of the torch formulation (DFTK_MI_TORCH_LOCAL=1) of the same
    five scalars, on the arrays of the last two iterations.

    python tools/potmix_bench.py [--supercell 2 3] [--ecut 15] [--iterations 8] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import _lib  # noqa: E402
from dftk_jl_amd import potential_mixing as pm  # noqa: E402


def counters(lib):
    a, b = C.c_int64(), C.c_int64()
    _lib.check(lib.dftk_mi_launch_count(C.byref(a), C.byref(b)))
    return a.value, b.value


def wall_ms(basis, fn, warmup=3, repeats=20):
    """median wall milliseconds of fn(), which ends with a host synchronisation of its own"""
    out = []
    with basis.on_library_stream():
        for i in range(warmup + repeats):
            basis.sync()
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def bench_cell(n, ecut, iterations):
    lat, atoms, pos = dftk.silicon_cell((n, n, n))
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
    basis = dftk.PlaneWaveBasis(model, ecut, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0")
    kpt = basis.kpoints[0]
    lines = [f"potmix_bench: Si {n}x{n}x{n} ({len(atoms)} atoms), Ecut {ecut:g}, fft {basis.fft_size}, n_G {kpt.n_G}"]

    stepper = dftk.ScfStepper(basis, tol=1e-14)
    steps = []
    for _ in range(iterations):
        t0 = time.perf_counter()
        stepper.step()
        steps.append(1e3 * (time.perf_counter() - t0))
    t_step = float(np.median(steps[2:]))
    lines.append(f"  ScfStepper step: {t_step:.2f} ms (steps {['%.1f' % s for s in steps]})")

    for label, curvature in (("kernel", "kernel"), ("secant", "secant")):
        stamps, infos = [], []

        def callback(info):
            basis.sync()
            stamps.append(time.perf_counter())
            if info.get("stage") == "iterate":
                infos.append(info)
        res = dftk.scf_potential_mixing_adaptive(basis, tol=1e-14, maxiter=iterations, callback=callback, curvature=curvature)
        its = [1e3 * (b - a) for a, b in zip(stamps, stamps[1:len(infos)])]        # iteration i + 2: between callbacks i + 1, i + 2
        trials = res["n_backtracks"]
        per_it = float(np.median(its[1:]))
        per_trial = float(sum(its[1:]) / sum(trials[1:len(its)]))
        lines.append(f"  potential mixing, adaptive, curvature {label}: iteration {per_it:.2f} ms, trial {per_trial:.2f} ms "
                     f"(x{per_trial / t_step:.2f} of an ScfStepper step); trials per iteration {trials}, alphas "
                     f"{[round(float(a), 3) for a in res['alphas']]}")

    # the scalar block alone, on the arrays of the last two iterations
    a, b = infos[-2], infos[-1]
    rho, rho_next, P = a["rho"], b["rho"], b["Pinv_dV"]
    pairs = [(a["Vout"], a["Vin"], rho_next, rho), (b["Vin"], a["Vin"], rho_next, rho), (rho_next, rho, b["Vout"], a["Vout"]),
             (P, None, P, None), (rho_next, rho, rho_next, rho)]
    basis.sync()
    l0, s0 = counters(basis.lib)
    with basis.on_library_stream():
        native = pm.diff_dots(basis, pairs)
    l1, s1 = counters(basis.lib)
    t_native = wall_ms(basis, lambda: pm.diff_dots(basis, pairs))
    os.environ["DFTK_MI_TORCH_LOCAL"] = "1"
    try:
        with basis.on_library_stream():
            twin = pm.diff_dots(basis, pairs)
        t_twin = wall_ms(basis, lambda: pm.diff_dots(basis, pairs))
    finally:
        del os.environ["DFTK_MI_TORCH_LOCAL"]
    err = max(abs(x - y) / max(abs(y), 1e-300) for x, y in zip(native, twin))
    lines.append(f"  scalar block of a trial (5 scalars, {rho.numel()} doubles per array): dftk_mi_diff_dots {l1 - l0} launch, "
                 f"{s1 - s0} host synchronisation, {t_native:.3f} ms; torch formulation {t_twin:.3f} ms; largest relative "
                 f"difference {err:.1e}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--supercell", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--ecut", type=float, default=15.0)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n in args.supercell:
        lines += bench_cell(n, args.ecut, args.iterations)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
