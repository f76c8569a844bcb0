"""Set-up cost of UPF pseudopotentials beside the HGH set-up of the same cell on the same build.

    python tools/upf_setup_bench.py --system si1000     # the 1000-electron silicon cell of bench.py (Gamma, Ecut 30)
    python tools/upf_setup_bench.py --system al         # fcc Al PBE, Ecut 40, 12^3 Monkhorst-Pack mesh (symmetry-reduced)

The UPF file is the cell's GTH pseudopotential written on a 1141-point logarithmic mesh (the size of the GTH files in UPF
form) by tests/upf_gen.py.  Reported, in milliseconds (each timed to a stream synchronisation, second of two runs):
dftk_mi_radial_transform per channel with its rows per second and the share of (q, r) pairs that take the sincos branch of
g_l, the table builders, and the whole basis set-up for both kinds of pseudopotential."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import psp_upf, terms  # noqa: E402
import upf_gen  # noqa: E402


def timed(basis, fn, repeat=2):
    for _ in range(repeat):
        basis.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        basis.sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    return out, 1e3 * dt


def sincos_share(l, q, r):
    """fraction of (q, r) pairs with q r >= the switch point of g_l (kind 1: every pair)"""
    if l is None:
        return 1.0
    q = np.sort(q[q > 0])
    if len(q) == 0:
        return 0.0
    below = np.searchsorted(q, psp_upf.SWITCH_POINTS[l] / r, side="left")      # q values under the switch, per r
    return 1.0 - float(below.sum()) / (len(r) * (len(q) + 0.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", choices=("si1000", "al"), default="si1000")
    ap.add_argument("--mesh", type=int, default=1141)
    args = ap.parse_args()
    r = upf_gen.log_mesh(args.mesh, 1e-5, 60.0)
    if args.system == "si1000":
        hgh = dftk.load_psp("Si", "lda")
        lat, _, pos = dftk.silicon_cell((5, 5, 5))
        sym, fun, kw, ecut, kg = "Si", ("lda_x", "lda_c_pw"), {}, 30.0, dftk.MonkhorstPack((1, 1, 1))
    else:
        hgh = dftk.load_psp("Al", "pbe")
        a = 7.6324708938577865
        lat, pos = a / 2 * np.array([[0, 1, 1.0], [1, 0, 1.0], [1, 1, 0.0]]), [np.zeros(3)]
        sym, fun, ecut, kg = "Al", ("gga_x_pbe", "gga_c_pbe"), 40.0, dftk.MonkhorstPack((12, 12, 12))
        kw = dict(temperature=1e-3, smearing="gaussian", symmetries=True)
    upf = dftk.parse_psp_upf(upf_gen.write_upf(hgh, r, element=sym), identifier=f"{sym}.upf")

    def build(psp):
        t0 = time.perf_counter()
        model = dftk.model_DFT(lat, [dftk.ElementPsp(sym, psp=psp)] * len(pos), pos, functionals=fun, **kw)
        basis = dftk.PlaneWaveBasis(model, ecut, kg, device="cuda:0", coarse_start=False)
        basis.sync()
        torch.cuda.synchronize()
        return basis, 1e3 * (time.perf_counter() - t0)

    build(hgh)                                  # warm-up: library load, first launches
    bh, t_h = build(hgh)
    bu, t_u = build(upf)
    print(f"system {args.system}: fft {bu.fft_size}, {len(bu.kpoints)} k-blocks, n_G {[k.n_G for k in bu.kpoints[:3]]}..., "
          f"mesh {len(r)} points")
    print(f"whole basis set-up: HGH {t_h:.1f} ms, UPF {t_u:.1f} ms (difference {t_u - t_h:+.1f} ms)")
    # ---- the pieces, on the UPF basis
    q_cube = terms._cube_norms(bu)
    rr, wf = upf.local_channel()
    _, t = timed(bu, lambda: terms.radial_transform_abi(bu, 1, 0, rr, wf, upf.Zion, q_cube))
    print(f"radial_transform kind 1 (V_loc), cube {q_cube.numel()} rows: {t:.2f} ms, {q_cube.numel() / t * 1e3:.3g} rows/s, "
          f"sincos share 100 %")
    kpt = bu.kpoints[0]
    q_k = torch.linalg.norm(kpt.Gplusk_cart[kpt.row0:kpt.row1], dim=1).contiguous()
    qh = q_k.cpu().numpy()
    total = 0.0
    for l in range(upf.lmax + 1):
        for i in range(upf.count_n_proj_radial(l)):
            rr, wf = upf.projector_channel(l, i)
            _, t = timed(bu, lambda: terms.radial_transform_abi(bu, 0, l, rr, wf, 0.0, q_k))
            total += t
            print(f"radial_transform kind 0 l={l} i={i + 1}, k-block 0, {q_k.numel()} rows x {len(rr)} points: {t:.3f} ms, "
                  f"{q_k.numel() / t * 1e3:.3g} rows/s, sincos share {100 * sincos_share(l, qh, rr):.1f} %")
    print(f"  all channels of one k-block: {total:.3f} ms; x {len(bu.kpoints)} k-blocks = {total * len(bu.kpoints):.1f} ms")
    _, t = timed(bu, lambda: terms._build_projection_vectors_radial_abi(bu, kpt))
    _, t0 = timed(bh, lambda: terms.build_projection_vectors_abi(bh, bh.kpoints[0]))
    print(f"projectors of k-block 0 (transforms + dftk_mi_build_projectors_radial): {t:.3f} ms; HGH builder: {t0:.3f} ms")

    def vloc_upf():
        bu._ff_local_table = None
        return terms.compute_local_potential(bu)
    _, t = timed(bu, vloc_upf)
    _, t0 = timed(bh, lambda: terms.compute_local_potential(bh))
    print(f"V_loc (transform + dftk_mi_atomic_superposition_table): {t:.2f} ms; HGH: {t0:.2f} ms")
    _, t = timed(bu, lambda: terms._atomic_superposition_table_abi(bu, terms.local_form_factor_table(bu)))
    print(f"  dftk_mi_atomic_superposition_table alone (table kept): {t:.2f} ms")


if __name__ == "__main__":
    main()
