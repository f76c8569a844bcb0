"""compute_stresses_cart on the bench cell (bench.py's default workload: Si 5x5x5 supercell, 250 atoms, 1000 electrons, LDA
HGH, Ecut 30, 192^3, Gamma only): SCF to 1e-6, then a warm-up and ``--calls`` timed calls with HIP-event timers per group
of terms (Kinetic + AtomicNonlocal share one entry point, AtomicLocal + Hartree one cube pass), the number and rate of
the projector products (zgemm profile family), the peak extra workspace, and from the same run compute_forces and a
late SCF step (median wall time of the last five steps) for comparison.  Once on the Gamma-real path, once with
``gamma_real=False`` (general complex blocks).

    python tools/stresses_bench.py [--supercell 5] [--calls 5] [--out profiles/stresses_cfg5.txt]
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
from dftk_jl_amd.stresses import _device_terms, full_stress_to_voigt  # noqa: E402

GROUPS = [("Kinetic+AtomicNonlocal", ("Kinetic", "AtomicNonlocal")), ("AtomicLocal+Hartree", ("AtomicLocal", "Hartree")),
          ("Xc", ("Xc",))]


def timed(basis, fn):
    with basis.on_library_stream():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
    return out, a.elapsed_time(b)


def workspace_bytes(kpt, n_p, n_bands, max_atom_cols):
    """the bound stated in stress_kernels.hip, evaluated for this block (bytes)"""
    rows = (kpt.n_G + 1) // 2 if kpt.gamma_real else kpt.n_G
    cc = min(n_p, max(max_atom_cols, (512 << 20) // (6 * rows * 16)))
    cc -= cc % max_atom_cols                                   # whole atoms (one species here)
    per_band = ((rows if kpt.gamma_real else 0) + n_p + 6 * cc) * 16
    cb = max(1, min(n_bands, (512 << 20) // per_band))
    return 6 * rows * cc * 16, per_band * cb, cc, cb


def run(n, gamma_real, calls, log):
    lat, atoms, pos = dftk.silicon_cell((n, n, n))
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_pw"))
    basis = dftk.PlaneWaveBasis(model, 30.0, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0",
                                gamma_real=None if gamma_real else False)
    stamps = []

    def cb(info):
        torch.cuda.synchronize()
        stamps.append(time.time())
    t0 = time.time()
    res = dftk.self_consistent_field(basis, tol=1e-6, callback=cb)
    t_scf = time.time() - t0
    steps = np.diff(np.asarray(stamps))
    late = float(np.median(steps[-5:])) * 1e3 if len(steps) >= 5 else float("nan")
    psi, occ, rho = res["psi"], res["occupation"], res["rho"]
    kpt = basis.kpoints[0]
    n_occ = int(np.count_nonzero(np.asarray(occ[0])))
    n_p = basis.terms.P[0].shape[0]
    log(f"\n== {'Gamma-real' if kpt.gamma_real else 'complex'} path: {len(atoms)} atoms, fft {basis.fft_size}, "
        f"n_G {kpt.n_G}, n_p {n_p}, occupied bands {n_occ}; SCF {res['n_iter']} steps, "
        f"{t_scf:.1f} s, E = {res['energies'].total:.10f}")
    lib, h = basis.lib, basis.handle
    ms = {g: [] for g, _ in GROUPS}
    first_ms = {}
    S = None
    for it in range(calls + 1):
        if it == 1:
            _lib.check(lib.dftk_mi_prof_enable(h, 1))
        parts = {}
        for g, names in GROUPS:
            out, t = timed(basis, lambda: _device_terms(basis, psi, occ, rho, names))
            parts.update(out)
            (ms[g].append(t) if it > 0 else first_ms.__setitem__(g, t))
        Si = sum(parts.values())
        if S is not None:
            assert np.array_equal(S, Si), "the device stress terms are not bitwise reproducible"
        S = Si
    g_ms, g_work, g_n = C.c_double(), C.c_double(), C.c_int64()
    _lib.check(lib.dftk_mi_prof_get(h, 0, C.byref(g_ms), C.byref(g_work), C.byref(g_n)))
    _lib.check(lib.dftk_mi_prof_enable(h, 0))
    for g, _ in GROUPS:
        v = np.asarray(ms[g])
        log(f"  {g:24s} median {np.median(v):8.2f} ms   min {v.min():8.2f} ms   ({calls} calls)   first call {first_ms[g]:9.2f} ms")
    dev_ms = float(sum(np.median(ms[g]) for g, _ in GROUPS))
    log(f"  device part (all five device terms): {dev_ms:.2f} ms")
    if g_n.value:
        log(f"  stress zgemm: {g_n.value // calls} calls per compute_stresses_cart, {g_ms.value / calls:.2f} ms, "
            f"{g_work.value / g_ms.value / 1e9:.1f} TF/s (useful flops of the {'REAL' if kpt.gamma_real else 'complex'} product)")
    w_bytes, band_bytes, cc, cbands = workspace_bytes(kpt, n_p, n_occ, atoms[0].psp.count_n_proj())
    log(f"  nonlocal workspace: derivative projectors {w_bytes / 2**20:.1f} MiB ({cc} columns per chunk, "
        f"{-(-n_p // cc)} chunks) + band panel and products {band_bytes / 2**20:.1f} MiB ({cbands} bands per chunk); "
        f"P itself is {kpt.n_G * n_p * 16 / 2**20:.1f} MiB")
    t0 = time.time()
    Sh = dftk.compute_stresses_term("Ewald", basis, psi, occ, rho=rho)
    log(f"  Ewald stress (host numpy, once per geometry, then kept): {1e3 * (time.time() - t0):.1f} ms on the first call")
    total, t_total = timed(basis, lambda: dftk.compute_stresses_cart(res))
    log(f"  compute_stresses_cart(scfres), everything included: {t_total:.2f} ms")
    # the comparison from the same run: forces (existing code) and a late SCF step
    f_ms = {t: [] for t in ("AtomicLocal", "AtomicNonlocal")}
    for it in range(calls + 1):
        for t in f_ms:
            _, dt = timed(basis, lambda: compute_forces_term(t, basis, psi, occ, rho=rho))
            if it > 0:
                f_ms[t].append(dt)
    f_dev = float(sum(np.median(v) for v in f_ms.values()))
    log(f"  compute_forces device part (AtomicLocal + AtomicNonlocal), same run: {f_dev:.2f} ms -> stresses / forces = "
        f"{dev_ms / f_dev:.2f}")
    log(f"  late SCF step (median wall time of the last five steps): {late:.1f} ms -> stresses / step = {dev_ms / late:.2f}")
    log(f"  sigma (Voigt xx yy zz zy zx yx) = {np.array2string(full_stress_to_voigt(total), precision=8)}, "
        f"pressure -tr sigma / 3 = {-np.trace(total) / 3:.8e} Ha/bohr^3")
    del Sh
    return total


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
    log(f"tools/stresses_bench.py --supercell {args.supercell} --calls {args.calls}; library {dftk.load_library().dftk_mi_version().decode()}")
    Sr = run(args.supercell, True, args.calls, log)
    if not args.no_complex:
        Sc = run(args.supercell, False, args.calls, log)
        log(f"\nmax |sigma(Gamma-real) - sigma(complex)| = {np.max(np.abs(Sr - Sc)):.3e} (independent SCFs to 1e-6)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
