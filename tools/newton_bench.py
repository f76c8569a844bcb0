"""newton and its tangent-space CG on Gamma-only silicon cells: silicon_cell((n, n, n)) at Ecut 15 by default, general complex
blocks, at the orbitals of an SCF stopped at 1e-3.  For the real-space cache on and off, on the same inputs in the same run
(the cache-off path is the composition the package had before: compute_delta_rho and multiply_psi_by_potential):

  * milliseconds per (Omega + K) application (HIP events on the library's stream, warm-up, median of the repeats), and of its
    three transform-bearing pieces alone (H d, the density change, dV psi): their sum over the application is the share of
    the calls that run 3-D transforms,
  * milliseconds, kernel launches and host synchronisations per CG iteration: the solver runs a FIXED number of iterations
    (tol = 0) for two values of K; reported is the difference of the two runs divided by the difference of K,
  * Newton steps and CG iterations of newton(tol = 1e-10) from that start, and its wall time.

    python tools/newton_bench.py [--supercell 2 3] [--ecut 15] [--k1 4] [--k2 12] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import _lib  # noqa: E402
from dftk_jl_amd.response import apply_kernel, multiply_psi_by_potential  # noqa: E402


def counters(lib):
    a, b = C.c_int64(), C.c_int64()
    _lib.check(lib.dftk_mi_launch_count(C.byref(a), C.byref(b)))
    return a.value, b.value


def event_ms(basis, fn, warmup=3, repeats=10):
    """median milliseconds of fn() between two events on the library's stream"""
    out = []
    with basis.on_library_stream():
        for i in range(warmup + repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def potential_part(ts, dV):
    basis = ts.basis
    if ts.psi_r is None:
        return multiply_psi_by_potential(basis, ts.psi, dV)
    out = [torch.empty_like(p) for p in ts.psi]
    for kpt, o, pr in zip(basis.kpoints, out, ts.psi_r):
        _lib.check(basis.lib.dftk_mi_tangent_potential(kpt.handle, o.shape[0], pr.data_ptr(), dV.data_ptr(), o.data_ptr(),
                                                       o.stride(0), 0))
    return out


def cg_run(basis, ts, rhs, occ, K):
    basis.sync()
    l0, s0 = counters(basis.lib)
    t0 = time.perf_counter()
    sol = dftk.solve_OmegaPlusK_cg(basis, ts.psi, rhs, occ, tol=0.0, maxiter=K, tangent_space=ts)
    ms = 1e3 * (time.perf_counter() - t0)
    l1, s1 = counters(basis.lib)
    assert sol["n_iter"] == K and not sol["negative_curvature"]
    return dict(ms=ms, launches=l1 - l0, syncs=s1 - s0)


def bench_cell(n, ecut, k1, k2):
    lat, atoms, pos = dftk.silicon_cell((n, n, n))
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
    basis = dftk.PlaneWaveBasis(model, ecut, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0", gamma_real=False)
    kpt = basis.kpoints[0]
    start = dftk.self_consistent_field(basis, tol=1e-3)
    psi, occ = dftk.select_occupied_orbitals(basis, start["psi"], start["occupation"])
    psi = [p.contiguous() for p in psi]
    nb = psi[0].shape[0]
    lines = [f"newton_bench: Si {n}x{n}x{n} ({len(atoms)} atoms), Ecut {ecut:g}, fft {basis.fft_size}, n_G {kpt.n_G}, "
             f"n_bands {nb}; the start is an SCF at 1e-3 ({start['n_iter']} steps)"]
    per = {}
    for cache in (True, False):
        with basis.on_library_stream():
            ts = dftk.TangentSpace(basis, psi, occ, cache_realspace=cache)
            rhs = ts.projected_gradient()
            d = ts.project(rhs)
            dV = apply_kernel(basis, ts._delta_rho(d), ts.rho).contiguous()
            basis.sync()
        t_apply = event_ms(basis, lambda: dftk.apply_OmegaPlusK(ts, d))
        t_H = event_ms(basis, lambda: [Hk @ dk for Hk, dk in zip(ts.ham, d)])
        t_rho = event_ms(basis, lambda: ts._delta_rho(d))
        t_V = event_ms(basis, lambda: potential_part(ts, dV))
        cg_run(basis, ts, rhs, occ, k1)                       # sizes every workspace
        best = {}
        for K in (k1, k2):
            for _ in range(2):
                r = cg_run(basis, ts, rhs, occ, K)
                if K not in best or r["ms"] < best[K]["ms"]:
                    best[K] = r
        # (K iterations begun = K - 1 applications and updates, whatever K: the difference counts whole iterations)
        it = {k: (best[k2][k] - best[k1][k]) / (k2 - k1) for k in ("ms", "launches", "syncs")}
        per[cache] = dict(apply=t_apply, H=t_H, rho=t_rho, V=t_V, **it)
        name = f"cache on ({ts.cache_bytes / 2 ** 20:.0f} MiB)" if cache else "cache off"
        lines.append(f"  {name}: (Omega + K) application {t_apply:.3f} ms; H d {t_H:.3f} ms, density change {t_rho:.3f} ms, "
                     f"dV psi {t_V:.3f} ms = {100 * (t_H + t_rho + t_V) / t_apply:.0f} % in calls that run 3-D transforms; "
                     f"CG iteration {it['ms']:.3f} ms, {it['launches']:.1f} launches, {it['syncs']:.1f} host synchronisations")
        del ts
    lines.append(f"  cache on / off: application x{per[False]['apply'] / per[True]['apply']:.2f}, K part (density change + dV psi) "
                 f"x{(per[False]['rho'] + per[False]['V']) / (per[True]['rho'] + per[True]['V']):.2f}, CG iteration "
                 f"x{per[False]['ms'] / per[True]['ms']:.2f}")
    for cache in (True, False):
        basis.sync()
        t0 = time.perf_counter()
        res = dftk.newton(basis, psi, tol=1e-10, cache_realspace=cache)
        wall = time.perf_counter() - t0
        lines.append(f"  newton to 1e-10, cache {'on' if cache else 'off'}: converged {res['converged']}, {res['n_iter']} steps, CG "
                     f"iterations {res['cg_iterations']}, |rho - rho_in| {['%.1e' % x for x in res['history_drho']]}, {wall:.2f} s")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--supercell", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--ecut", type=float, default=15.0)
    ap.add_argument("--k1", type=int, default=4)
    ap.add_argument("--k2", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for n in args.supercell:
        lines += bench_cell(n, args.ecut, args.k1, args.k2)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
