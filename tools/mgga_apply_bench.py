#!/usr/bin/env python3
"""One dftk_mi_apply_H with and without the tau potential of a meta-GGA on the silicon blocks of
tests/golden/silicon_scan_abinit.json (Ecut 15, 27^3, the four irreducible k-points), 8 and 64 bands.
Per block: 30 warm-up calls, then 7 samples of 100 back-to-back calls each, ended by a synchronisation; the median sample, the
smaller of two alternating passes.  Prints one line, APPLYH {...}, times in microseconds per call."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dftk_jl_amd as dftk  # noqa: E402

gold = json.load(open(os.path.join(ROOT, "tests", "golden", "silicon_scan_abinit.json")))
lat, atoms, pos = dftk.silicon_cell(functional="pbe", a=gold["lattice_constant"])
model = dftk.model_DFT(lat, atoms, pos, functionals=("mgga_x_scan", "mgga_c_scan"), symmetries=True)
basis = dftk.PlaneWaveBasis(model, 15, dftk.ExplicitKpoints(gold["kcoords"], gold["kweights"]), fft_size=(27, 27, 27), device="cuda:0")
rho = dftk.guess_density(basis)
tau = dftk.guess_kinetic_energy_density(basis, rho)
_, ham = dftk.energy_hamiltonian(basis, None, None, rho=rho, tau=tau)
gen = torch.Generator(device="cuda")
gen.manual_seed(1)
out = {}
vts = [H.tau_potential for H in ham]
assert all(v is not None for v in vts)
for nb in (8, 64):
    psis = [dftk.random_orbitals(basis, H.kpoint, nb, gen).contiguous() for H in ham]
    outs = [torch.empty_like(p) for p in psis]
    res = {}
    for label in ("with", "without", "with", "without"):
        for H, vt in zip(ham, vts):
            H.tau_potential = vt if label == "with" else None
            H.bind()
        per = []
        for H, p, o in zip(ham, psis, outs):
            for _ in range(30):
                H.mul_(o, p)
            torch.cuda.synchronize()
            samples = []
            for _ in range(7):
                t0 = time.perf_counter()
                for _ in range(100):
                    H.mul_(o, p)
                basis.sync()
                torch.cuda.synchronize()
                samples.append((time.perf_counter() - t0) / 100)
            per.append(float(np.median(samples)))
        res.setdefault(label, []).append(per)
    w, wo = np.min(np.array(res["with"]), axis=0), np.min(np.array(res["without"]), axis=0)
    out[nb] = dict(n_G=[int(H.n_G) for H in ham], with_us=(w * 1e6).round(1).tolist(), without_us=(wo * 1e6).round(1).tolist(),
                   ratio=(w / wo).round(2).tolist(), ratio_all=float(w.sum() / wo.sum()))
print("APPLYH " + json.dumps(out))
