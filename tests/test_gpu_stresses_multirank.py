"""compute_stresses_cart on two ranks sharing cuda:0 (host-staged collectives over gloo, as
tests/test_gpu_forces_multirank.py): k-points split over comm_kpts -- every rank gets the tensor of the single-rank
calculation, to round-off of the different summation order -- and a basis whose plane waves are sharded over comm_pw is
refused."""
import json
import os
import sys

import pytest

from conftest import free_port  # noqa: E402
from test_gpu_forces_multirank import COMMON  # noqa: E402
from test_gpu_multirank import ROOT, _spawn  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KPT_WORKER = COMMON + r'''
lattice = 5.0 * np.array([[0, 1, 1.02], [1, 0, 1], [1, 1, 0]])
_, atoms, _ = dftk.silicon_cell()
pos = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]
model = dftk.model_DFT(lattice, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
KC = [[0, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0]]
KW = [0.25, 0.5, 0.25]
basis = dftk.PlaneWaveBasis(model, 8, dftk.ExplicitKpoints(KC, KW), fft_size=(20, 20, 20), device="cuda:0",
                            comm_kpts=comm)
assert len(basis.kpoints) == (2 if comm.rank == 0 else 1)
res = dftk.self_consistent_field(basis, tol=1e-9)
S = dftk.compute_stresses_cart(res)
parts = comm.gather_lists((list(basis.krange_thisproc), [p.cpu().numpy() for p in res["psi"]],
                           [np.asarray(o) for o in res["occupation"]]))
Ss = comm.gather_lists(S.tolist())
if comm.rank == 0:
    parts.sort(key=lambda t: t[0][0])
    psi = [torch.from_numpy(p).to("cuda:0") for _, ps, _ in parts for p in ps]
    occ = [o for _, _, os_ in parts for o in os_]
    ref_basis = dftk.PlaneWaveBasis(model, 8, dftk.ExplicitKpoints(KC, KW), fft_size=(20, 20, 20), device="cuda:0")
    Sref = dftk.compute_stresses_cart(ref_basis, psi, occ, rho=res["rho"])
    print("RESULT " + json.dumps({"err": relerr(S, Sref), "ranks_equal": bool(np.array_equal(Ss[0], Ss[1])),
                                  "maxS": float(np.max(np.abs(Sref)))}))
dist.barrier(); dist.destroy_process_group()
'''

PW_WORKER = COMMON + r'''
lat, atoms, pos = dftk.silicon_cell((2, 1, 1))
model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_pw"))
basis = dftk.PlaneWaveBasis(model, 8, dftk.MonkhorstPack((1, 1, 1)), device="cuda:0", comm_pw=comm)
kpt = basis.kpoints[0]
assert kpt.n_loc < kpt.n_G
psi = [torch.zeros((4, kpt.n_loc), dtype=torch.complex128, device="cuda:0")]
occ = [np.full(4, 2.0)]
rho = dftk.guess_density(basis)
refused = {}
for name, call in (("cart", lambda: dftk.compute_stresses_cart(basis, psi, occ, rho=rho)),
                   ("kinetic", lambda: dftk.compute_stresses_term("Kinetic", basis, psi, occ, rho=rho)),
                   ("ewald", lambda: dftk.compute_stresses_term("Ewald", basis, psi, occ, rho=rho))):
    try:
        call()
        refused[name] = "no error"
    except NotImplementedError as e:
        refused[name] = "NotImplementedError: " + str(e)
if comm.rank == 0:
    print("RESULT " + json.dumps(refused))
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


def test_kpoint_split_stresses_equal_single_rank(tmp_path):
    got = _run(tmp_path, KPT_WORKER)
    assert got["ranks_equal"]
    assert got["maxS"] > 1e-4
    assert got["err"] < 1e-12, got


def test_planewave_sharded_basis_is_refused(tmp_path):
    got = _run(tmp_path, PW_WORKER)
    for name, what in got.items():
        assert what.startswith("NotImplementedError") and "comm_pw" in what, (name, what)
