"""compute_forces on the bench cell (bench.py's default workload: Si 5x5x5 supercell, 250 atoms, 1000 electrons, LDA HGH,
Ecut 30, 192^3, Gamma only): SCF to 1e-6, then a warm-up and ``--calls`` timed compute_forces calls with HIP-event timers
per term, and the TF/s of the forces' projector products (zgemm profile family).  Once on the Gamma-real path, once
with ``gamma_real=False`` (general complex blocks).

    python tools/forces_bench.py [--supercell 5] [--calls 5] [--out profiles/forces_cfg5.txt]
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
from dftk_jl_amd.forces import compute_forces_term  # noqa: E402


def run(n, gamma_real, calls, log):
    lat, atoms, pos = dftk.silicon_cell((n, n, n))
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_pw"))
    basis = dftk.PlaneWaveBasis(model, 30.0, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0",
                                gamma_real=None if gamma_real else False)
    t0 = time.time()
    res = dftk.self_consistent_field(basis, tol=1e-6)
    t_scf = time.time() - t0
    psi, occ, rho = res["psi"], res["occupation"], res["rho"]
    kpt = basis.kpoints[0]
    n_occ = int(np.count_nonzero(np.asarray(occ[0])))
    log(f"\n== {'Gamma-real' if kpt.gamma_real else 'complex'} path: {len(atoms)} atoms, fft {basis.fft_size}, "
        f"n_G {kpt.n_G}, n_p {basis.terms.P[0].shape[0]}, occupied bands {n_occ}; SCF {res['n_iter']} steps, "
        f"{t_scf:.1f} s, E = {res['energies'].total:.10f}")
    terms = [t for t in model.term_types if t in ("AtomicLocal", "AtomicNonlocal", "Ewald")]
    lib, h = basis.lib, basis.handle
    ms = {t: [] for t in terms}
    first_ms = {}
    F = None
    for it in range(calls + 1):
        if it == 1:
            _lib.check(lib.dftk_mi_prof_enable(h, 1))
        parts = {}
        for t in terms:
            with basis.on_library_stream():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                parts[t] = compute_forces_term(t, basis, psi, occ, rho=rho)
                b.record()
                b.synchronize()
            if it > 0:
                ms[t].append(a.elapsed_time(b))
            else:
                first_ms[t] = a.elapsed_time(b)
        Fi = sum(parts.values())
        if F is not None:
            assert np.array_equal(F, Fi), "compute_forces is not bitwise reproducible"
        F = Fi
    g_ms, g_work, g_n = C.c_double(), C.c_double(), C.c_int64()
    _lib.check(lib.dftk_mi_prof_get(h, 0, C.byref(g_ms), C.byref(g_work), C.byref(g_n)))
    _lib.check(lib.dftk_mi_prof_enable(h, 0))
    for t in terms:
        v = np.asarray(ms[t])
        log(f"  {t:15s} median {np.median(v):8.2f} ms   min {v.min():8.2f} ms   ({calls} calls)   first call {first_ms[t]:9.2f} ms")
    if "Ewald" in terms:
        log(f"  Ewald forces are host numpy, computed on the first call of a basis (once per geometry) and kept: "
            f"{first_ms['Ewald']:.1f} ms on the first call, the timed calls return the kept array")
    dev_ms = float(np.median(ms["AtomicLocal"]) + np.median(ms["AtomicNonlocal"]))
    log(f"  device part (AtomicLocal + AtomicNonlocal): {dev_ms:.2f} ms  (target <= 50 ms on the Gamma-real path)")
    if g_n.value:
        log(f"  forces zgemm: {g_n.value // calls} calls per compute_forces, {g_ms.value / calls:.2f} ms, "
            f"{g_work.value / g_ms.value / 1e9:.1f} TF/s (useful flops of the {'REAL' if kpt.gamma_real else 'complex'} product)")
    log(f"  max |F| = {np.max(np.abs(F)):.3e}, |sum F| = {np.abs(F.sum(axis=0)).max():.3e} (reduced)")
    return F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--supercell", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-complex", action="store_true")
    args = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    log(f"tools/forces_bench.py --supercell {args.supercell} --calls {args.calls}; library {dftk.load_library().dftk_mi_version().decode()}")
    Fr = run(args.supercell, True, args.calls, log)
    if not args.no_complex:
        Fc = run(args.supercell, False, args.calls, log)
        log(f"\nmax |F(Gamma-real) - F(complex)| = {np.max(np.abs(Fr - Fc)):.3e} (independent SCFs to 1e-6)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
