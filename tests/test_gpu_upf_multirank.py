"""UPF pseudopotentials on two ranks sharing cuda:0 (host-staged collectives over gloo, as
tests/test_gpu_forces_multirank.py): k-points split over comm_kpts, and one Gamma k-block whose plane waves are sharded over
comm_pw (every rank transforms the channels at the norms of its own row slab).  Each worker converges the distributed SCF
of GTH silicon written as a UPF file, computes the forces, and rank 0 repeats the calculation on a single-rank basis: total
energies to 1e-8 Ha (the tolerance of tests/test_gpu_multirank.py for two converged SCFs), forces to 1e-7."""
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
sys.path.insert(0, os.path.join(os.environ["REPO"], "tests"))
import numpy as np, torch, torch.distributed as dist
import dftk_jl_amd as dftk
import upf_gen
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["PORT"],
                        rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
comm = dftk.KptComm.from_torch()
hgh = dftk.load_psp("Si", "lda")
upf = dftk.parse_psp_upf(upf_gen.write_upf(hgh, upf_gen.uniform_mesh(2001, 30.0)), identifier="si.upf")
Si = dftk.ElementPsp("Si", psp=upf)
'''

KPT_WORKER = COMMON + r'''
lat, _, _ = dftk.silicon_cell()
pos = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]
model = dftk.model_DFT(lat, [Si, Si], pos, functionals=("lda_x", "lda_c_vwn"))
KC = [[0, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0]]
KW = [0.25, 0.5, 0.25]
basis = dftk.PlaneWaveBasis(model, 8, dftk.ExplicitKpoints(KC, KW), fft_size=(20, 20, 20), device="cuda:0",
                            comm_kpts=comm)
assert len(basis.kpoints) == (2 if comm.rank == 0 else 1)
res = dftk.self_consistent_field(basis, tol=1e-10)
F = dftk.compute_forces(res)
Fs = comm.gather_lists(F.tolist())
if comm.rank == 0:
    ref_basis = dftk.PlaneWaveBasis(model, 8, dftk.ExplicitKpoints(KC, KW), fft_size=(20, 20, 20), device="cuda:0")
    ref = dftk.self_consistent_field(ref_basis, tol=1e-10)
    Fref = dftk.compute_forces(ref)
    print("RESULT " + json.dumps({"dE": abs(res["energies"].total - ref["energies"].total),
                                  "dF": float(np.max(np.abs(F - Fref))), "maxF": float(np.max(np.abs(Fref))),
                                  "converged": bool(res["converged"] and ref["converged"]),
                                  "ranks_equal": bool(np.array_equal(Fs[0], Fs[1]))}))
dist.barrier(); dist.destroy_process_group()
'''

PW_WORKER = COMMON + r'''
lat, atoms, pos = dftk.silicon_cell((2, 1, 1))
pos = [np.asarray(p) + (0.004 * np.array([1.0, 2.0, 3.0]) if i == 0 else 0) for i, p in enumerate(pos)]
model = dftk.model_DFT(lat, [Si] * len(pos), pos, functionals=("lda_x", "lda_c_pw"))
out = {}
for gamma_real in (False, True):
    basis = dftk.PlaneWaveBasis(model, 8, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0", comm_pw=comm,
                                gamma_real=gamma_real)
    kpt = basis.kpoints[0]
    assert kpt.n_loc < kpt.n_G and kpt.gamma_real == gamma_real
    res = dftk.self_consistent_field(basis, tol=1e-10)
    F = dftk.compute_forces(res)
    Fs = comm.gather_lists(F.tolist())
    if comm.rank == 0:
        ref_basis = dftk.PlaneWaveBasis(model, 8, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0",
                                        fft_size=basis.fft_size, gamma_real=gamma_real)
        ref = dftk.self_consistent_field(ref_basis, tol=1e-10)
        Fref = dftk.compute_forces(ref)
        out["real" if gamma_real else "complex"] = {
            "dE": abs(res["energies"].total - ref["energies"].total), "dF": float(np.max(np.abs(F - Fref))),
            "maxF": float(np.max(np.abs(Fref))), "converged": bool(res["converged"] and ref["converged"]),
            "ranks_equal": bool(np.array_equal(Fs[0], Fs[1]))}
    dist.barrier()
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


def _check(got):
    assert got["converged"] and got["ranks_equal"], got
    assert got["maxF"] > 1e-4, got
    assert got["dE"] < 1e-8 and got["dF"] < 1e-7, got


def test_upf_kpoints_split_over_two_ranks(tmp_path):
    _check(_run(tmp_path, KPT_WORKER))


def test_upf_planewave_sharded_gamma_block(tmp_path):
    got = _run(tmp_path, PW_WORKER)
    for kind in ("complex", "real"):
        _check(got[kind])
