"""bench.py's plain run on a tiny cell: --steps sets the number of timed steps (the SCF converges on the way and goes on
iterating), the JSON line carries the headline and nothing that needs runs of its own, and --dump-outputs writes the last
step's outputs, the same for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--supercell", "1", "--ecut", "10", "--steps", "25", "--warmup", "1"]


def _bench(extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra, capture_output=True, text=True,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_bench_runs_exactly_steps_and_dumps_reproducible_outputs(tmp_path):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    out = _bench(["--dump-outputs", str(tmp_path / "a")])
    c = out["config"]
    assert out["steps"] == 25 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert c["converged"] and c["steps_to_convergence"] < 25 and len(c["step_wall_s"]) == 25
    for k_ in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k_ in out
    assert out["unit"] == "SCF iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert abs(out["ms_per_step"] * out["steps"] / 1e3 - c["scf_wall_s"]) < 2e-3
    assert abs(out["value"] * out["ms_per_step"] / 1e3 - 1.0) < 1e-9
    # lean: nothing of --full
    assert not {"roofline", "cpu_baseline", "amdahl", "random_start_value", "complex_iteration_value"} & set(out)
    assert "parity" not in c and "host_timers_ms_per_step" not in c
    a = _load(tmp_path / "a")
    assert {"rho", "eigenvalues", "occupation", "energies", "density_matrix_sample"} <= set(a)
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64e6
    import dftk_jl_amd as dftk
    lat, atoms, _ = dftk.silicon_cell()
    assert abs(a["rho"].sum() * abs(np.linalg.det(lat)) / a["rho"].size - 4 * len(atoms)) < 1e-8
    assert a["energies"][0] == c["E_total"]
    assert np.isclose(a["occupation"].sum(), 4 * len(atoms), atol=1e-10)
    # same arguments, same inputs: the outputs agree to round-off
    _bench(["--dump-outputs", str(tmp_path / "b")])
    b = _load(tmp_path / "b")
    assert set(b) == set(a)
    for k_ in a:
        np.testing.assert_allclose(b[k_], a[k_], rtol=0, atol=1e-9 * max(1.0, np.abs(a[k_]).max()), err_msg=k_)
