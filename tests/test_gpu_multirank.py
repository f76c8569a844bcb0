"""N > 1 code path on the real hot path with ONE GPU: two ranks share cuda:0 and reduce over gloo
(RCCL refuses two ranks on one device; the collective is the only thing swapped).  Covers what the
driver's multi-GPU bench exercises: k-point distribution, the density all-reduce, the Fermi level
over sharded eigenvalues, summed energies, and bench.py's aggregation over ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import free_port  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KCOORDS = [[0, 0, 0], [0.5, 0, 0], [0.25, 0.25, 0]]
KWEIGHTS = [0.25, 0.5, 0.25]

WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["REPO"])
import numpy as np, torch, torch.distributed as dist
import dftk_jl_amd as dftk
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["PORT"],
                        rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
comm = dftk.KptComm.from_torch()
lat, atoms, pos = dftk.silicon_cell()
model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
kg = dftk.ExplicitKpoints(json.loads(os.environ["KCOORDS"]), json.loads(os.environ["KWEIGHTS"]))
basis = dftk.PlaneWaveBasis(model, 8, kg, fft_size=(20, 20, 20), device="cuda:0", comm_kpts=comm)
assert len(basis.kpoints) == (2 if comm.rank == 0 else 1)          # split_evenly: 3 k-points over 2 ranks
res = dftk.self_consistent_field(basis, tol=1e-9, nbandsalg=dftk.AdaptiveBands(model, n_bands_converge=6))
lam = comm.gather_lists([l[:6].tolist() for l in res["eigenvalues"]])
if comm.rank == 0:
    print("RESULT " + json.dumps({"E": res["energies"].total, "terms": dict(res["energies"]),
                                  "lam": [l for sub in lam for l in sub], "converged": bool(res["converged"]),
                                  "rho_sum": float(res["rho"].sum()) * basis.dvol}))
dist.barrier(); dist.destroy_process_group()
'''


def _spawn(cmds_env, timeout=600.0, grace=10.0):
    """Run the rank processes to completion.  A rank that dies leaves its peers waiting in a collective for ever, so
    the survivors are killed ``grace`` seconds after the first failure (and everybody at ``timeout``): a broken rank
    fails the test in seconds with its output instead of hanging the suite.  Output goes to temporary files (no pipe
    that could fill up while nobody reads it)."""
    import tempfile
    import time
    logs = [tempfile.TemporaryFile(mode="w+") for _ in cmds_env]
    procs = [subprocess.Popen(cmd, env=env, stdout=log, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
             for (cmd, env), log in zip(cmds_env, logs)]
    t0 = time.time()
    first_failure = None
    while any(p.poll() is None for p in procs):
        now = time.time()
        if first_failure is None and any(p.poll() not in (None, 0) for p in procs):
            first_failure = now
        if now - t0 > timeout or (first_failure is not None and now - first_failure > grace):
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.1)
    outs = []
    for p, log in zip(procs, logs):
        p.wait()
        log.seek(0)
        outs.append(log.read())
        log.close()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed (exit {p.returncode}):\n{o[-4000:]}"
    return outs


def test_two_ranks_one_gpu_scf_equals_single_rank(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    port = free_port()
    base = dict(os.environ, WORLD_SIZE="2", PORT=port, REPO=ROOT, MASTER_ADDR="127.0.0.1",
                KCOORDS=json.dumps(KCOORDS), KWEIGHTS=json.dumps(KWEIGHTS))
    outs = _spawn([([sys.executable, str(script)], dict(base, RANK=str(r))) for r in range(2)])
    line = [ln for ln in outs[0].splitlines() if ln.startswith("RESULT ")][-1]
    got = json.loads(line[len("RESULT "):])
    assert got["converged"]
    # the same calculation on one rank
    lat, atoms, pos = dftk.silicon_cell()
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
    basis = dftk.PlaneWaveBasis(model, 8, dftk.ExplicitKpoints(KCOORDS, KWEIGHTS), fft_size=(20, 20, 20))
    ref = dftk.self_consistent_field(basis, tol=1e-9, nbandsalg=dftk.AdaptiveBands(model, n_bands_converge=6))
    assert ref["converged"]
    assert abs(got["E"] - ref["energies"].total) < 1e-8 * 2            # 1e-8 Ha/atom
    for name, v in ref["energies"].items():
        assert abs(got["terms"][name] - v) < 1e-7, name
    np.testing.assert_allclose(np.array(got["lam"]).reshape(3, 6), np.array([l[:6] for l in ref["eigenvalues"]]),
                               atol=1e-7)
    assert abs(got["rho_sum"] - 8.0) < 1e-9


def _run_bench(extra, port_base):
    port = free_port()
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-cpu-baseline"] + extra
    base = dict(os.environ, WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                DFTK_MI_BENCH_BACKEND="gloo", DFTK_MI_BENCH_DEVICE="0")
    outs = _spawn([(cmd, dict(base, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)])
    lines = [ln for ln in outs[0].splitlines() if ln.startswith("{")]
    assert len(lines) == 1, outs[0][-2000:]
    assert not [ln for ln in outs[1].splitlines() if ln.startswith("{")]        # only rank 0 prints
    return json.loads(lines[0])


def test_bench_two_ranks_one_gpu_weak_kpoints():
    """bench.py --mode weak, N = 2 (torch.distributed.run env contract, one k-point per rank, max-over-ranks
    timing, whole-job value) on a tiny cell; both ranks on cuda:0 over gloo; --steps sets the timed SCF steps."""
    out = _run_bench(["--full", "--mode", "weak", "--steps", "2", "--warmup", "1", "--supercell", "1", "--ecut", "10"], 33000)
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["config"]["parallelism"] == "kpt2" and not out["config"]["converged"]
    assert abs(out["value"] - 2 * 2 / (out["ms_per_step"] * 2 / 1e3)) < 1e-6 * out["value"]   # 2 k-blocks x steps / time
    assert out["roofline"]["achieved"] > 0 and np.isfinite(out["config"]["E_total"])


def test_bench_two_ranks_one_gpu_kpoints_strong_equals_single_rank():
    """bench.py --mode kpoints (BASELINE configs[2] class: Al PBE, symmetry-reduced Monkhorst-Pack mesh, LDOS mixing,
    k-points split over the ranks, one density all-reduce per step + one for the LDOS): the 2-rank run does the SAME
    fixed workload as the 1-rank run (strong scaling) and converges to the same energy."""
    args = ["--full", "--mode", "kpoints", "--kgrid", "4", "--ecut", "12", "--warmup", "0", "--tol", "1e-8"]  # (to convergence)
    out = _run_bench(args, 39000)
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["config"]["converged"]
    assert out["config"]["parallelism"] == "kpt2" and "8 k-points (4 on rank 0" in out["config"]["workload"]
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline"] + args
    one = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-2000:]
    ref = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
    assert ref["config"]["converged"] and "8 k-points (8 on rank 0" in ref["config"]["workload"]
    assert abs(out["config"]["E_total"] - ref["config"]["E_total"]) < 1e-8
    assert abs(out["steps"] - ref["steps"]) <= 2
    assert out["config"]["n_matvec"] > 0 and abs(out["config"]["n_matvec"] / ref["config"]["n_matvec"] - 1) < 0.3


def test_bench_two_ranks_one_gpu_gamma_sharded_equals_single_rank():
    """bench.py's DEFAULT N > 1 path: the Gamma-only cell with its plane waves sharded over the ranks (strong
    scaling, whole SCF to convergence); same converged energy and SCF length class as the one-rank run."""
    args = ["--full", "--warmup", "0", "--supercell", "1", "--ecut", "12", "--tol", "1e-8"]     # (no --steps: to convergence)
    out = _run_bench(args, 35000)
    assert out["n_gpus"] == 2 and out["scaling"] == "strong" and out["config"]["converged"]
    assert out["config"]["parallelism"].startswith("pw2") and out["steps"] < 40
    assert out["config"]["orbitals"].startswith("real-symmetric")
    assert out["roofline"]["families_launches"]["collectives"] > 0
    # the library's own communicator saw both ranks; the start-up self-check (one sharded H psi + Gram against the
    # gathered block) ran and passed before the SCF
    assert out["config"]["rccl"]["n_ranks"] == 2 and out["config"]["rccl"]["backend"].startswith("host-staged")
    chk = out["config"]["sharded_self_check"]
    assert chk["gram_hermiticity"] < 1e-10 and chk["gram_vs_gathered"] < 1e-10
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--no-cpu-baseline"] + args
    one = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert one.returncode == 0, one.stdout[-2000:] + one.stderr[-2000:]
    ref = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
    assert ref["config"]["converged"] and ref["n_gpus"] == 1
    assert abs(out["config"]["E_total"] - ref["config"]["E_total"]) < 1e-8 * 2      # 1e-8 Ha / atom
    # (same SCF length class: tol = 1e-8 sits in the round-off tail of the Anderson iteration, where the different
    #  summation orders of the sharded Gram products move the step count by a few)
    assert abs(out["steps"] - ref["steps"]) <= 5


PW_WORKER = r'''
import json, os, sys
sys.path.insert(0, os.environ["REPO"])
import numpy as np, torch, torch.distributed as dist
import dftk_jl_amd as dftk
torch.cuda.set_device(0)
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%s" % os.environ["PORT"],
                        rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
comm = dftk.KptComm.from_torch()
lat, atoms, pos = dftk.silicon_cell((2, 2, 2))
model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_pw"))
basis = dftk.PlaneWaveBasis(model, 8, dftk.MonkhorstPack((1, 1, 1)), fft_size=(40, 40, 40), device="cuda:0", comm_pw=comm)
kpt = basis.kpoints[0]
assert kpt.n_loc < kpt.n_G and comm._abi_kind is not None
assert kpt.gamma_real          # real-symmetric Gamma orbitals also on the sharded block (half-format row slabs)
# (1) H psi and the density of a fixed block, slab by slab
rho0 = dftk.guess_density(basis)
_, ham = dftk.energy_hamiltonian(basis, None, None, rho=rho0)
torch.manual_seed(5)
gen = torch.Generator(device="cuda"); gen.manual_seed(11)
psi = dftk.random_orbitals(basis, kpt, 9, gen)
Hpsi = ham[0] @ psi
occ = [np.array([2.0, 2, 2, 2, 1.5, 0.5, 0, 0, 0])]
rho = dftk.compute_density(basis, [psi], occ)
parts = comm.gather_lists((kpt.row0, psi.cpu().numpy(), Hpsi.cpu().numpy()))
# (2) a whole SCF
res = dftk.self_consistent_field(basis, tol=1e-9)
# (3) the same SCF with a FIXED tight diagonalisation tolerance: every step is then determined to round-off
res_fixed = dftk.self_consistent_field(basis, tol=1e-7, determine_tol=lambda n_iter, hist: 1e-9)
if comm.rank == 0:
    full_psi = np.concatenate([p[1] for p in sorted(parts, key=lambda t: t[0])], axis=1)
    full_H = np.concatenate([p[2] for p in sorted(parts, key=lambda t: t[0])], axis=1)
    np.save(os.environ["OUT"] + "_psi.npy", full_psi); np.save(os.environ["OUT"] + "_H.npy", full_H)
    np.save(os.environ["OUT"] + "_rho.npy", rho.cpu().numpy())
    print("RESULT " + json.dumps({"E": res["energies"].total, "terms": dict(res["energies"]),
                                  "lam": res["eigenvalues"][0].tolist(), "converged": bool(res["converged"]),
                                  "n_iter": res["n_iter"], "n_matvec": res["n_matvec"],
                                  "history_drho_fixed_diagtol": [float(x) for x in res_fixed["history_drho"]],
                                  "rho_sum": float(res["rho"].sum()) * basis.dvol}))
dist.barrier(); dist.destroy_process_group()
'''


def test_planewave_sharded_block_two_ranks_one_gpu(tmp_path):
    """SURVEY section 8e (Gamma-only cells): the plane waves of ONE k-block shard over two ranks as row slabs
    (dftk_mi_kblock_set_shard; here both ranks on cuda:0 with the host-staged communicator over gloo).  H psi and
    the density of a fixed block equal the unsharded ones to round-off; a whole SCF reproduces the single-rank
    energy terms (1e-8 Ha/atom) and eigenvalues."""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    script = tmp_path / "pw_worker.py"
    script.write_text(PW_WORKER)
    port = free_port()
    out_prefix = str(tmp_path / "pw")
    base = dict(os.environ, WORLD_SIZE="2", PORT=port, REPO=ROOT, MASTER_ADDR="127.0.0.1", OUT=out_prefix)
    outs = _spawn([([sys.executable, str(script)], dict(base, RANK=str(r))) for r in range(2)])
    got = json.loads([ln for ln in outs[0].splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert got["converged"]
    lat, atoms, pos = dftk.silicon_cell((2, 2, 2))
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_pw"))
    basis = dftk.PlaneWaveBasis(model, 8, dftk.MonkhorstPack((1, 1, 1)), fft_size=(40, 40, 40))
    rho0 = dftk.guess_density(basis)
    _, ham = dftk.energy_hamiltonian(basis, None, None, rho=rho0)
    psi = torch.from_numpy(np.load(out_prefix + "_psi.npy")).cuda()
    # the slabs of the sharded random block are the rows of the one-rank block drawn from the same generator
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    assert torch.equal(psi, dftk.random_orbitals(basis, basis.kpoints[0], 9, gen))
    Href = (ham[0] @ psi).cpu().numpy()
    Hgot = np.load(out_prefix + "_H.npy")
    assert np.linalg.norm(Hgot - Href) / np.linalg.norm(Href) < 1e-13
    occ = [np.array([2.0, 2, 2, 2, 1.5, 0.5, 0, 0, 0])]
    rho_ref = dftk.compute_density(basis, [psi], occ).cpu().numpy()
    rho_got = np.load(out_prefix + "_rho.npy")
    assert np.linalg.norm(rho_got - rho_ref) / np.linalg.norm(rho_ref) < 1e-13
    ref = dftk.self_consistent_field(basis, tol=1e-9)
    assert ref["converged"]
    n_atoms = 16
    assert abs(got["E"] - ref["energies"].total) < 1e-8 * n_atoms
    for name, v in ref["energies"].items():
        assert abs(got["terms"][name] - v) < 1e-7, name
    nconv = ref["n_bands_converge"]
    np.testing.assert_allclose(np.array(got["lam"])[:nconv], ref["eigenvalues"][0][:nconv], atol=1e-7)
    assert abs(got["rho_sum"] - 64.0) < 1e-8
    # (tol = 1e-9 sits at the round-off floor of the Anderson iteration: the last decade takes a few steps more or
    #  less depending on the summation order of the sharded reductions -- five seeds of the ONE-rank run alone give
    #  33 .. 38 steps; the energies, terms and eigenvalues above are the parity criteria)
    assert abs(got["n_iter"] - ref["n_iter"]) <= 15
    # ... and a TIGHT criterion where one exists.  With the adaptive tolerance a step's output is only determined to
    # diagtol (0.025 on the first steps), so trajectories part at the 1e-4 level from step 1 on and the step count is
    # not a sharp observable.  With a FIXED tight diagonalisation tolerance every SCF step is a deterministic map up to
    # round-off: the sharded run must then walk the SAME density-change history and stop at the same step.
    ref_fixed = dftk.self_consistent_field(basis, tol=1e-7, determine_tol=lambda n_iter, hist: 1e-9)
    h_got, h_ref = got["history_drho_fixed_diagtol"], ref_fixed["history_drho"]
    assert ref_fixed["converged"] and abs(len(h_got) - len(h_ref)) <= 1, (h_got, h_ref)
    # (entries far above the diagonalisation tolerance: below ~1e-5 the 1e-9 eigensolver residuals start to show)
    n_cmp = min(len(h_got), len(h_ref), sum(1 for d in h_ref if d > 1e-5))
    assert n_cmp >= 4
    np.testing.assert_allclose(h_got[:n_cmp], h_ref[:n_cmp], rtol=1e-4)


def test_rccl_c_abi_single_rank_allreduce():
    """dftk_mi_comm_* / dftk_mi_allreduce_sum_f64 (what a Julia shim calls instead of mpi_sum!): the run-time
    RCCL binding, communicator life cycle and an in-place fp64 sum on a one-rank communicator."""
    import ctypes as C
    from dftk_jl_amd._lib import check
    lib = dftk.load_library()
    uid = C.create_string_buffer(128)
    check(lib.dftk_mi_comm_get_unique_id(uid))
    comm = C.c_void_p()
    check(lib.dftk_mi_comm_init_rank(uid.raw, 1, 0, 0, C.byref(comm)))
    x = torch.arange(1 << 20, dtype=torch.float64, device="cuda") * 0.5
    want = x.clone()
    torch.cuda.synchronize()
    check(lib.dftk_mi_allreduce_sum_f64(comm, x.data_ptr(), x.numel(), None))
    torch.cuda.synchronize()
    assert torch.equal(x, want)
    assert lib.dftk_mi_allreduce_sum_f64(comm, None, 4, None) < 0          # invalid argument, reported not crashed
    check(lib.dftk_mi_comm_destroy(comm))


def test_c_consumer_of_the_header_drives_rccl_shard_apply_density_lobpcg():
    """tools/abi_c_check.c (plain C against include/dftk_mi355x.h): unique id -> init_rank -> describe (ncclCommCount)
    -> all-reduce -> zgemm with by-value complex scalars -> set_shard -> apply_H / density / LOBPCG on the slab, each
    compared with the unsharded block inside the program.  One rank here (RCCL wants one device per rank; the same
    binary takes N on a multi-GPU node: `tools/bin/abi_c_check 8`)."""
    import subprocess
    from dftk_jl_amd import _build
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    exe = _build.build_abi_check()
    res = subprocess.run([exe, "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "abi_c_check OK ranks=1" in res.stdout
    n_dev = torch.cuda.device_count()
    if n_dev > 1:
        res = subprocess.run([exe, str(n_dev)], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
        assert f"abi_c_check OK ranks={n_dev}" in res.stdout
