"""The density response on two ranks sharing cuda:0 (host-staged collectives over gloo, as
tests/test_gpu_stresses_multirank.py): k-points split over comm_kpts -- every rank gets the d_rho and the Fermi-level
shift of the single-rank calculation on the same orbitals, to round-off of the different summation order (the Sternheimer
tolerances are clamped to one value: the balanced rule divides by the LOCAL number of k-points, as the reference does) --
and a basis whose plane waves are sharded over comm_pw is refused."""
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
lat, atoms, _ = dftk.silicon_cell()
pos = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]
model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"), temperature=0.03, smearing="fermi_dirac")
KC = [[0, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0]]
KW = [0.25, 0.5, 0.25]
basis = dftk.PlaneWaveBasis(model, 5, dftk.ExplicitKpoints(KC, KW), device="cuda:0", comm_kpts=comm)
assert len(basis.kpoints) == (2 if comm.rank == 0 else 1)
res = dftk.self_consistent_field(basis, tol=1e-8)
nx, ny, nz = basis.fft_size
z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
dV = torch.from_numpy(0.3 * np.cos(2 * np.pi * x + 0.3) + 0.2 * np.cos(2 * np.pi * (y + z) + 1.1)).to("cuda:0")
thr = res["occupation_threshold"]


def fixed(b, psi, occ):
    return dftk.BandtolBalanced(b, psi, occ, occupation_threshold=thr, bandtol_min=1e-10, bandtol_max=1e-10)


out = dftk.apply_chi0(res, dV, bandtolalg=fixed(basis, res["psi"], res["occupation"]))
parts = comm.gather_lists((list(basis.krange_thisproc), [p.cpu().numpy() for p in res["psi"]],
                           [np.asarray(o) for o in res["occupation"]], [np.asarray(e) for e in res["eigenvalues"]]))
outs = comm.gather_lists((out["drho"].cpu().numpy(), out["deF"], bool(out["converged"])))
if comm.rank == 0:
    parts.sort(key=lambda t: t[0][0])
    psi = [torch.from_numpy(p).to("cuda:0") for _, ps, _, _ in parts for p in ps]
    occ = [o for _, _, os_, _ in parts for o in os_]
    eig = [e for _, _, _, es in parts for e in es]
    ref_basis = dftk.PlaneWaveBasis(model, 5, dftk.ExplicitKpoints(KC, KW), fft_size=basis.fft_size, device="cuda:0")
    _, ham = dftk.energy_hamiltonian(ref_basis, None, None, rho=res["rho"], only_hamiltonian=True)
    ref = dftk.apply_chi0(ham, psi, occ, res["eF"], eig, dV, occupation_threshold=thr, bandtolalg=fixed(ref_basis, psi, occ))
    print("RESULT " + json.dumps({"err": relerr(out["drho"].cpu().numpy(), ref["drho"].cpu().numpy()),
                                  "deF": out["deF"], "deF_ref": ref["deF"],
                                  "ranks_equal": bool(np.array_equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]),
                                  "converged": bool(outs[0][2] and outs[1][2] and ref["converged"]),
                                  "max": float(np.max(np.abs(ref["drho"].cpu().numpy())))}))
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
eig = [np.zeros(4)]
rho = dftk.guess_density(basis)
_, ham = dftk.energy_hamiltonian(basis, None, None, rho=rho, only_hamiltonian=True)
refused = {}
for name, call in (("apply_chi0", lambda: dftk.apply_chi0(ham, psi, occ, 0.1, eig, rho)),
                   ("apply_chi0_4P", lambda: dftk.apply_chi0_4P(ham, psi, occ, 0.1, eig, psi)),
                   ("sternheimer_solver", lambda: dftk.sternheimer_solver(ham[0], psi[0], eig[0], psi[0])),
                   ("compute_delta_rho", lambda: dftk.compute_delta_rho(basis, psi, psi, occ)),
                   ("apply_kernel", lambda: dftk.apply_kernel(basis, rho, rho))):
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


def test_kpoint_split_response_equals_single_rank(tmp_path):
    got = _run(tmp_path, KPT_WORKER)
    assert got["converged"] and got["ranks_equal"]
    assert got["max"] > 1e-4 and abs(got["deF_ref"]) > 1e-6
    assert got["err"] < 1e-10, got
    assert abs(got["deF"] - got["deF_ref"]) < 1e-10 * abs(got["deF_ref"]), got


def test_planewave_sharded_basis_is_refused(tmp_path):
    got = _run(tmp_path, PW_WORKER)
    for name, what in got.items():
        assert what.startswith("NotImplementedError") and "comm_pw" in what, (name, what)
