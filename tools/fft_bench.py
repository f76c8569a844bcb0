#!/usr/bin/env python
"""Time the five FFT stages of the local H psi (and the density z-pass) on a BASELINE-sized sphere:
python tools/fft_bench.py [supercell n = 5] [bands = 64] [bands per launch group = 32].  Prints ms per launch and algorithmic TB/s per stage
(HIP events inside the library).  DFTK_MI_ZPASS_CLASSIC=1 selects the LDS-staged z-pass for comparison.
``stage_times(basis, nb, fft_batch)`` is the measurement itself, for other tools (tools/exx_bench.py)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402

NAMES = {1: "A xbwd_scatter", 2: "B ybwd", 3: "C z fused V", 4: "D yfwd", 5: "E xfwd_gather", 6: "density z"}
REPS = 5


def stage_times(basis, nb, fft_batch):
    """{family: (ms, work, launches)} of REPS local H psi + density passes over nb random bands of the basis' first k-block
    (profile on after one warm-up round; the profile is switched off again)"""
    kpt = basis.kpoints[0]
    lib = basis.lib
    check(lib.dftk_mi_basis_set_fft_batch(basis.handle, fft_batch))
    g = torch.Generator(device="cuda").manual_seed(1)
    V = torch.randn(basis.fft_size[::-1], dtype=torch.float64, device="cuda", generator=g)
    H = dftk.DftHamiltonianBlock(basis, kpt, V)
    psi = dftk.random_orbitals(basis, kpt, nb, g)
    out = torch.empty_like(psi)
    rho = torch.zeros(basis.fft_size[::-1], dtype=torch.float64, device="cuda")
    w = np.full(nb, 0.5)
    before = {}
    for rep in range(2):
        if rep == 1:
            check(lib.dftk_mi_prof_enable(basis.handle, 1))
            before = _read(basis)
        for _ in range(REPS):
            H.mul_(out, psi, 3)
            check(lib.dftk_mi_density_accumulate(kpt.handle, nb, psi.data_ptr(), psi.stride(0), w.ctypes.data, rho.data_ptr()))
        basis.sync()
    after = _read(basis)
    check(lib.dftk_mi_prof_enable(basis.handle, 0))
    return {fam: tuple(a - b for a, b in zip(after[fam], before[fam])) for fam in NAMES}


def _read(basis):
    out = {}
    for fam in NAMES:
        ms, work, cnt = C.c_double(), C.c_double(), C.c_int64()
        check(basis.lib.dftk_mi_prof_get(basis.handle, fam, C.byref(ms), C.byref(work), C.byref(cnt)))
        out[fam] = (ms.value, work.value, cnt.value)
    return out


def two_transforms_ms_per_band(times, nb):
    """one pruned backward + one pruned forward transform of a band: stages A ... E of the local H psi"""
    return sum(times[fam][0] for fam in (1, 2, 3, 4, 5)) / (REPS * nb)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    fft_batch = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    lat, atoms, pos = dftk.silicon_cell((n, n, n))
    basis = dftk.PlaneWaveBasis(dftk.model_DFT(lat, atoms, pos), 30, dftk.MonkhorstPack((1, 1, 1)), build_terms=False)
    times = stage_times(basis, nb, fft_batch)
    print(f"fft {basis.fft_size}, n_G {basis.kpoints[0].n_G}, {nb} bands, {fft_batch} bands per launch group, classic={os.environ.get('DFTK_MI_ZPASS_CLASSIC') is not None}")
    for fam, name in NAMES.items():
        ms, work, cnt = times[fam]
        print(f"  {name:16s} {ms / max(cnt, 1) * 1e3:8.1f} us/launch  {work / (ms * 1e-3) / 1e12:6.2f} TB/s  ({cnt} launches)")


if __name__ == "__main__":
    main()
