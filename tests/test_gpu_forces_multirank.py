"""compute_forces on two ranks sharing cuda:0 (host-staged collectives over gloo, as tests/test_gpu_multirank.py):
k-points split over comm_kpts, and one Gamma k-block whose plane waves are sharded over comm_pw (general complex and
real-symmetric half-format blocks).  Each worker runs its SCF, computes the forces on the distributed basis, gathers
psi / occupations / rho on rank 0 and recomputes the forces there on a single-rank basis of the same calculation: the
two must agree to round-off of the different summation orders."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import free_port  # noqa: E402
from test_gpu_multirank import ROOT, _spawn  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COMMON = r'''
import json, os, sys
sys.path.insert(0, os.environ["REPO"])
import numpy as np, torch, torch.distributed as dist
import dftk_jl_amd as dftk
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["PORT"],
                        rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
comm = dftk.KptComm.from_torch()


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))
'''

KPT_WORKER = COMMON + r'''
lat, atoms, _ = dftk.silicon_cell()
pos = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]
model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
KC = [[0, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0]]
KW = [0.25, 0.5, 0.25]
basis = dftk.PlaneWaveBasis(model, 8, dftk.ExplicitKpoints(KC, KW), fft_size=(20, 20, 20), device="cuda:0",
                            comm_kpts=comm)
assert len(basis.kpoints) == (2 if comm.rank == 0 else 1)
res = dftk.self_consistent_field(basis, tol=1e-9)
F = dftk.compute_forces(res)
parts = comm.gather_lists((list(basis.krange_thisproc), [p.cpu().numpy() for p in res["psi"]],
                           [np.asarray(o) for o in res["occupation"]]))
Fs = comm.gather_lists(F.tolist())
if comm.rank == 0:
    parts.sort(key=lambda t: t[0][0])
    psi = [torch.from_numpy(p).to("cuda:0") for _, ps, _ in parts for p in ps]
    occ = [o for _, _, os_ in parts for o in os_]
    ref_basis = dftk.PlaneWaveBasis(model, 8, dftk.ExplicitKpoints(KC, KW), fft_size=(20, 20, 20), device="cuda:0")
    Fref = dftk.compute_forces(ref_basis, psi, occ, rho=res["rho"])
    print("RESULT " + json.dumps({"err": relerr(F, Fref), "ranks_equal": bool(np.array_equal(Fs[0], Fs[1])),
                                  "maxF": float(np.max(np.abs(Fref)))}))
dist.barrier(); dist.destroy_process_group()
'''

PW_WORKER = COMMON + r'''
lat, atoms, pos = dftk.silicon_cell((2, 1, 1))
pos = [np.asarray(p) + (0.004 * np.array([1.0, 2.0, 3.0]) if i == 0 else 0) for i, p in enumerate(pos)]
model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_pw"))
out = {}
for gamma_real in (False, True):
    basis = dftk.PlaneWaveBasis(model, 8, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0", comm_pw=comm,
                                gamma_real=gamma_real)
    kpt = basis.kpoints[0]
    assert kpt.n_loc < kpt.n_G and kpt.gamma_real == gamma_real
    res = dftk.self_consistent_field(basis, tol=1e-9)
    F = dftk.compute_forces(res)
    slabs = comm.gather_lists((kpt.row0, res["psi"][0].cpu().numpy()))
    Fs = comm.gather_lists(F.tolist())
    if comm.rank == 0:
        slabs.sort(key=lambda t: t[0])
        psi = [torch.from_numpy(np.ascontiguousarray(np.concatenate([s for _, s in slabs], axis=1))).to("cuda:0")]
        ref_basis = dftk.PlaneWaveBasis(model, 8, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0",
                                        fft_size=basis.fft_size, gamma_real=gamma_real)
        assert ref_basis.kpoints[0].gamma_real == gamma_real and ref_basis.kpoints[0].n_G == kpt.n_G
        Fref = dftk.compute_forces(ref_basis, psi, res["occupation"], rho=res["rho"])
        out["real" if gamma_real else "complex"] = {"err": relerr(F, Fref), "maxF": float(np.max(np.abs(Fref))),
                                                    "ranks_equal": bool(np.array_equal(Fs[0], Fs[1]))}
if comm.rank == 0:
    print("RESULT " + json.dumps(out))
dist.barrier(); dist.destroy_process_group()
'''


def _run(tmp_path, source):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    script = tmp_path / "worker.py"
    script.write_text(source)
    base = dict(os.environ, WORLD_SIZE="2", PORT=free_port(), REPO=ROOT, MASTER_ADDR="127.0.0.1")
    outs = _spawn([([sys.executable, str(script)], dict(base, RANK=str(r))) for r in range(2)])
    line = [ln for ln in outs[0].splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_kpoint_split_forces_equal_single_rank(tmp_path):
    got = _run(tmp_path, KPT_WORKER)
    assert got["ranks_equal"]
    assert got["maxF"] > 1e-3
    assert got["err"] < 1e-12, got


def test_planewave_sharded_gamma_forces_equal_single_rank(tmp_path):
    got = _run(tmp_path, PW_WORKER)
    for kind in ("complex", "real"):
        assert got[kind]["ranks_equal"], (kind, got)
        assert got[kind]["maxF"] > 1e-4, (kind, got)
        assert got[kind]["err"] < 1e-11, (kind, got)
