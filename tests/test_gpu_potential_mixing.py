"""``scf_potential_mixing`` / ``scf_potential_mixing_adaptive`` on the device against ``self_consistent_field`` of the same basis.

The first tests are the reference's own (test/scf_compare.jl:56-62, :150-158): silicon, LDA, Ecut 3 on a 9^3 cube with the four
irreducible k-points of the 3 x 3 x 3 mesh, and bcc iron with collinear spin at T = 0.01 (Ecut 11, 13^3, 3 x 3 x 3); the
densities agree with the density-mixing SCF to 10 tol, tol = 1e-7 -- the reference's bound.  The other cells are the displaced
Gamma cells of tests/test_gpu_direct_minimization.py.

The gradient check needs no SCF: with E(alpha) = E(V_in + alpha dV) from ``EVrho`` on a cell without symmetries, the central
difference (E(h) - E(-h)) / 2h and the mean of the model's slopes at +h and -h, <V_out - V_in, rho(h) - rho(-h)> dvol / 2h,
both approach dE/dalpha at second order: their distance at h / 2 is at most 0.3 x the one at h (a quarter, with room for the
next order), down to a floor of 1e-8 / h -- LOBPCG residuals of 1e-10 over a gap of 0.1 leave 1e-9 in the orbitals, which
enters E at first order times |V_out - V_in| = O(1) wherever V_in is not the fixed point; ten times that, over h.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import potential_mixing as pm  # noqa: E402

import nlcc_gen  # noqa: E402
from test_gpu_direct_minimization import DISPLACED, GAMMA, LDA, PBE, TOL, si_basis  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IRON_LATTICE = 2.71176 * np.array([[-1, 1, 1], [1, -1, 1], [1, 1, -1.0]])


def scf(basis, tol, **kw):
    res = dftk.self_consistent_field(basis, tol=tol, **kw)
    assert res["converged"]
    return res


def drho_max(a, b):
    return float((a["rho"] - b["rho"]).abs().max().item())


def report(name, res, ref):
    d = drho_max(res, ref)
    print(f"\n{name}: {res['n_iter']} iterations, trials per iteration {res['n_backtracks']}, alphas "
          f"{[round(a, 3) for a in res['alphas']]}, curvature {res['curvature']}, max|rho - rho_SCF| = {d:.2e} "
          f"(bound {10 * TOL:.0e}), E - E_SCF = {res['energies'].total - ref['energies'].total:.2e}")
    assert res["converged"], (res["n_iter"], res["history_drho"][-3:])
    return d


# ------------------------------------------------------------------------------------------ the reference's tests
@pytest.fixture(scope="module")
def si_kpts():
    basis = si_basis()
    return basis, scf(basis, TOL / 10)


def test_silicon_kerker_fixed_damping(si_kpts):
    basis, ref = si_kpts
    res = dftk.scf_potential_mixing(basis, mixing=dftk.KerkerMixing(), tol=TOL, rho=dftk.guess_density(basis))
    assert report("silicon LDA, Kerker, fixed damping", res, ref) < 10 * TOL
    assert set(res["alphas"]) == {0.8} and set(res["n_backtracks"]) == {1} and res["curvature"] == "kernel"
    # the result reads like an scfres
    assert res["algorithm"] == "SCF" and res["basis"] is basis and res["stage"] == "finalize"
    assert len(res["history_Etot"]) == len(res["history_drho"]) == res["n_iter"] and res["history_drho"][-1] < TOL
    assert len(res["alphas"]) == len(res["n_backtracks"]) == len(res["model_relerrors"]) == res["n_iter"] - 1
    assert len(res["psi"]) == len(res["ham"]) == len(basis.kpoints)
    # the final Hamiltonian is built from the last output potential
    assert torch.equal(dftk.total_local_potential(res["ham"]), res["Vout"])


def test_silicon_simple_mixing_adaptive(si_kpts):
    basis, ref = si_kpts
    res = dftk.scf_potential_mixing_adaptive(basis, mixing=dftk.SimpleMixing(), tol=TOL, rho=dftk.guess_density(basis))
    assert report("silicon LDA, simple mixing, adaptive damping", res, ref) < 10 * TOL
    damping = dftk.AdaptiveDamping()
    assert all(damping.alpha_min <= abs(a) <= damping.alpha_max for a in res["alphas"])
    assert all(1 <= n <= 3 for n in res["n_backtracks"])


@pytest.fixture(scope="module")
def iron():
    Fe = dftk.ElementPsp("Fe", dftk.load_psp("Fe", "lda"))
    model = dftk.model_DFT(IRON_LATTICE, [Fe], [np.zeros(3)], functionals=LDA, temperature=0.01, magnetic_moments=(4.0,),
                           symmetries=True)
    basis = dftk.PlaneWaveBasis(model, 11, dftk.MonkhorstPack((3, 3, 3)), fft_size=(13, 13, 13), device="cuda:0")
    rho0 = dftk.guess_density(basis, (4.0,))
    return basis, rho0, scf(basis, TOL, rho=rho0)


def test_iron_collinear_kerker(iron):
    basis, rho0, ref = iron
    res = dftk.scf_potential_mixing(basis, mixing=dftk.KerkerMixing(), tol=TOL, rho=rho0)
    assert res["rho"].shape == ref["rho"].shape and res["rho"].dim() == 4
    assert report("iron LDA collinear, Kerker", res, ref) < 10 * TOL


def test_iron_collinear_adaptive_from_bad_damping(iron):
    """started deliberately with the very bad damping of 1.5, as the reference does.  (Whether a backtrack happens is printed,
    not asserted: tests/test_potmix_host.py covers backtracking deterministically.)"""
    basis, rho0, ref = iron
    res = dftk.scf_potential_mixing_adaptive(basis, mixing=dftk.SimpleMixing(), tol=TOL, rho=rho0,
                                             damping=dftk.AdaptiveDamping(1.5))
    assert res["curvature"] == "secant"
    assert report("iron LDA collinear, simple mixing, AdaptiveDamping(1.5)", res, ref) < 10 * TOL


# ------------------------------------------------------------------------------------------ model pieces
@pytest.fixture(scope="module")
def gamma_cell():
    """the displaced cell at Gamma with the Gamma-real switch off: the basis, its SCF at tol and at tol / 10"""
    basis = si_basis(**GAMMA, Ecut=7, fft_size=None, positions=DISPLACED, gamma_real=False)
    return basis, scf(basis, TOL), scf(basis, TOL / 10)


@pytest.mark.parametrize("cell", ["gamma", "kpoints"])
def test_energy_gradient_against_central_differences(cell, gamma_cell):
    basis = gamma_cell[0] if cell == "gamma" else si_basis(symmetries=False)
    with basis.on_library_stream():
        rho0 = dftk.guess_density(basis)
        ham0 = dftk.energy_hamiltonian(basis, None, None, rho=rho0, only_hamiltonian=True)[1]
        gen = torch.Generator(device=basis.device)
        gen.manual_seed(5)
        EVrho = pm.make_EVrho(basis, ham0, generator=gen)
        at = dict(EVrho(dftk.total_local_potential(ham0), diagtol=1e-10), dvol=basis.dvol)
        dV = at["Vout"] - at["Vin"]

        def errors(h):
            plus, minus = (dict(EVrho(at["Vin"] + a * dV, diagtol=1e-10, psi=at["psi"]), alpha=a) for a in (h, -h))
            fd = (plus["energies"].total - minus["energies"].total) / (2 * h)
            slope = 0.5 * (pm.quadratic_model_coefficients(at, plus, "secant")[0]
                           + pm.quadratic_model_coefficients(at, minus, "secant")[0])
            return abs(fd - slope), slope, fd
        h = 0.2
        coarse, slope, _ = errors(h)
        fine, slope_fine, fd_fine = errors(h / 2)
        basis.sync()
    floor = 1e-8 / (h / 2)
    print(f"\nenergy gradient ({cell}): slope = {slope_fine:.8e}, central difference = {fd_fine:.8e}; distance {coarse:.2e} at "
          f"h = {h}, {fine:.2e} at h / 2, floor {floor:.1e}")
    assert slope_fine < 0 and abs(slope_fine) > 100 * floor           # the direction descends, well above the floor
    assert fine <= max(0.3 * coarse, floor)


def test_kernel_against_secant_curvature(gamma_cell):
    """<drho, K drho> from ``apply_kernel`` and from V_out(rho + t d) - V_out(rho) differ at third order in t"""
    basis = gamma_cell[0]
    from dftk_jl_amd.terms import local_potential_fused
    nx, ny, nz = basis.fft_size
    with basis.on_library_stream():
        rho = dftk.guess_density(basis)
        x = torch.arange(nx, dtype=torch.float64, device=basis.device) / nx
        y = torch.arange(ny, dtype=torch.float64, device=basis.device) / ny
        d = 0.1 * rho * (torch.cos(2 * np.pi * x)[None, None, :] + 0.5 * torch.sin(2 * np.pi * y)[None, :, None])
        V = local_potential_fused(basis, rho, want_energies=False)["V"]
        P = torch.zeros_like(rho)

        def gap(t):
            rho_t = (rho + t * d).contiguous()
            V_t = local_potential_fused(basis, rho_t, want_energies=False)["V"]
            info = dict(rho=rho, Vin=V, Vout=V, basis=basis)
            nxt = dict(rho=rho_t, Vin=V_t, Vout=V_t, Pinv_dV=P, basis=basis)
            kernel = pm._device_model_sums(basis, "kernel", True)(info, nxt)
            secant = pm._device_model_sums(basis, "secant", True)(info, nxt)
            assert kernel["dot_out"] == secant["dot_out"] == 0.0 and kernel["drho_norm2"] == secant["drho_norm2"] > 0
            return secant["dot_kernel"] - kernel["dot_kernel"], kernel["dot_kernel"]
        g1, k1 = gap(1.0)
        g2, k2 = gap(0.5)
        basis.sync()
    print(f"\ncurvature: <drho, K drho> = {k1:.6e} at t = 1 ({k2:.6e} at t / 2), secant - kernel = {g1:.3e}, {g2:.3e}, ratio "
          f"{g1 / g2:.2f}")
    assert abs(k1 / k2 - 4) < 1e-9 * 4 and k1 > 0
    assert 6 <= g1 / g2 <= 10


def test_hamiltonian_with_total_potential_leaves_the_input_alone(gamma_cell):
    basis, loose, _ = gamma_cell
    ham = loose["ham"]
    psi = loose["psi"][0]
    with basis.on_library_stream():
        before = (ham[0] @ psi).clone()
        pot = ham[0].potential.clone()
        V = dftk.total_local_potential(ham)
        assert V.shape == tuple(reversed(basis.fft_size)) and torch.equal(V, pot)
        other = dftk.hamiltonian_with_total_potential(ham, 2 * V + 0.3)
        shifted = other[0] @ psi
        after = ham[0] @ psi
        basis.sync()
    assert other[0] is not ham[0] and torch.equal(ham[0].potential, pot) and torch.equal(other[0].potential, 2 * V + 0.3)
    assert torch.equal(before, after)                                           # bit-equal H psi
    assert float((shifted - before).abs().max()) > 1e-3
    with pytest.raises(ValueError, match="shape"):
        dftk.hamiltonian_with_total_potential(ham, V[:-1])


# ------------------------------------------------------------------------------------------ other runs at Gamma
def test_pbe_at_gamma():
    basis = si_basis(PBE, **GAMMA, Ecut=7, fft_size=None, positions=DISPLACED)
    res = dftk.scf_potential_mixing_adaptive(basis, tol=TOL)
    assert res["curvature"] == "secant"
    assert report("silicon PBE at Gamma, adaptive", res, scf(basis, TOL / 10)) < 10 * TOL


def test_upf_with_core_correction():
    psp = nlcc_gen.core_psp("Si", "lda", core=True)
    basis = si_basis(("lda_x", "lda_c_vwn"), **GAMMA, Ecut=7, fft_size=None, positions=DISPLACED,
                     atoms=[dftk.ElementPsp("Si", psp=psp)] * 2)
    assert basis.terms.rho_core is not None
    res = dftk.scf_potential_mixing_adaptive(basis, tol=TOL)
    assert res["curvature"] == "kernel"
    assert report("silicon UPF + NLCC at Gamma, adaptive", res, scf(basis, TOL / 10)) < 10 * TOL


@pytest.fixture(scope="module")
def gamma_adaptive(gamma_cell):
    return dftk.scf_potential_mixing_adaptive(gamma_cell[0], tol=TOL, seed=3)


def test_gamma_real_switch_on_against_off(gamma_cell, gamma_adaptive):
    basis_off, loose, tight = gamma_cell
    basis_on = si_basis(**GAMMA, Ecut=7, fft_size=basis_off.fft_size, positions=DISPLACED, gamma_real=True)
    on = dftk.scf_potential_mixing_adaptive(basis_on, tol=TOL)
    assert report("Gamma-real switch on, against the SCF with it off", on, tight) < 10 * TOL
    assert report("Gamma-real switch off", gamma_adaptive, tight) < 10 * TOL


CHILD = r'''
import ctypes, json, os, sys
sys.path.insert(0, os.environ["REPO"])
sys.path.insert(0, os.path.join(os.environ["REPO"], "tests"))
import numpy as np
import dftk_jl_amd as dftk
from test_gpu_direct_minimization import DISPLACED, GAMMA, TOL, si_basis
basis = si_basis(**GAMMA, Ecut=7, fft_size=None, positions=DISPLACED, gamma_real=True)
res = dftk.scf_potential_mixing_adaptive(basis, tol=TOL, damping=dftk.AdaptiveDamping(1.5))
n = ctypes.c_int64()
basis.lib.dftk_mi_ax_reuse_count(ctypes.byref(n))
np.save(os.environ["OUT"], res["rho"].cpu().numpy())
print("RESULT " + json.dumps(dict(n_iter=res["n_iter"], converged=bool(res["converged"]), n_backtracks=res["n_backtracks"],
                                  ax_reuse=n.value)))
'''


def test_kept_lobpcg_state_switched_off_in_a_child(tmp_path):
    """the same run with the A X and the planes a k-block keeps between two LOBPCG calls switched off: the line search hands
    over the orbitals they are valid for, or older ones, for which nothing is promised.  (Both runs take the general LOBPCG
    driver, the one that keeps the A X: the small-block driver this cell would get keeps nothing.)"""
    outs = {}
    for tag, extra in (("kept", {}), ("off", dict(DFTK_MI_AX_REUSE="0", DFTK_MI_PLANES_REUSE="0"))):
        script = tmp_path / "child.py"
        script.write_text(CHILD)
        out = str(tmp_path / f"rho_{tag}.npy")
        env = dict(os.environ, REPO=ROOT, OUT=out, DFTK_MI_LOBPCG_SMALL="0", **extra)
        run = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, env=env, timeout=600)
        assert run.returncode == 0, (tag, run.stdout[-1500:], run.stderr[-3000:])
        line = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        outs[tag] = (json.loads(line[len("RESULT "):]), np.load(out))
    (kept, rho_kept), (off, rho_off) = outs["kept"], outs["off"]
    print(f"\nkept LOBPCG state: on {kept}, off {off}, max|rho_on - rho_off| = {np.abs(rho_kept - rho_off).max():.2e}")
    assert kept["converged"] and off["converged"]
    assert kept["ax_reuse"] > 0 and off["ax_reuse"] == 0
    assert np.abs(rho_kept - rho_off).max() < 10 * TOL
    assert kept["n_iter"] == off["n_iter"]


# ------------------------------------------------------------------------------------------ the run itself
def test_energy_acceptance(gamma_cell):
    """under ScfAcceptImprovingStep the energy of an accepted step never rises by more than max_energy_change, unless the
    residual fell (a step taken because the trials ran out is exempt: it is the last of ``max_backtracks`` trials)"""
    basis = gamma_cell[0]
    seen = []
    res = dftk.scf_potential_mixing_adaptive(basis, tol=TOL, damping=dftk.AdaptiveDamping(1.5), max_backtracks=3,
                                             callback=lambda info: seen.append(info))
    its = [i for i in seen if i["stage"] == "iterate"]
    assert res["converged"] and len(its) == res["n_iter"]
    checked = 0
    for a, b, trials in zip(its, its[1:], res["n_backtracks"]):
        dE = b["energies"].total - a["energies"].total
        fell = b["sums"]["pinv_norm2"] < a["sums"]["pinv_norm2"]
        if trials < 3:
            assert dE < TOL or fell, (dE, trials)
            checked += 1
    print(f"\nenergy acceptance: trials {res['n_backtracks']}, {checked} accepted steps checked")
    assert checked >= 1


def test_result_interoperability(gamma_cell, gamma_adaptive, tmp_path):
    basis, loose, tight = gamma_cell
    res = gamma_adaptive
    f_loose, f_tight = dftk.compute_forces_cart(loose), dftk.compute_forces_cart(tight)
    bound = 10 * float(np.abs(f_loose - f_tight).max())
    err = float(np.abs(dftk.compute_forces_cart(res) - f_tight).max())
    print(f"\nforces: max|F_potmix - F_SCF| = {err:.2e}, bound 10 |F_SCF(tol) - F_SCF(tol / 10)| = {bound:.2e}")
    assert np.abs(f_tight).max() > 1e-3 and err <= bound
    fn = str(tmp_path / "potmix.npz")
    dftk.save_scfres(fn, res, save_psi=True)
    back = dftk.load_scfres(fn, basis)
    assert torch.equal(back["rho"], res["rho"]) and all(torch.equal(p, q) for p, q in zip(back["psi"], res["psi"]))
    assert back["energies"]["total"] == pytest.approx(res["energies"].total, abs=1e-12)
    assert back["algorithm"] == "SCF" and back["n_iter"] == res["n_iter"] and back["converged"]
    bands = dftk.compute_bands(res, dftk.ExplicitKpoints([[0, 0, 0], [0.5, 0, 0]], [0.5, 0.5]), n_bands=5)
    assert np.abs(np.asarray(bands["eigenvalues"][0])[:4] - np.asarray(res["eigenvalues"][0])[:4]).max() < 1e-5


def test_same_seed_same_trajectory_and_nothing_else_changes(gamma_cell, gamma_adaptive):
    basis, _, tight = gamma_cell
    rho0, psi0 = tight["rho"].clone(), [p.clone() for p in tight["psi"]]
    e0, ham_pot = tight["energies"].total, tight["ham"][0].potential.clone()
    before = dftk.energy_hamiltonian(basis, tight["psi"], tight["occupation"], rho=tight["rho"])[0]
    with basis.on_library_stream():
        Hpsi = (tight["ham"][0] @ tight["psi"][0]).clone()
        basis.sync()
    again = dftk.scf_potential_mixing_adaptive(basis, tol=TOL, seed=3)
    other = dftk.scf_potential_mixing_adaptive(basis, tol=TOL, seed=4, maxiter=4)
    a = gamma_adaptive
    assert a["history_Etot"] == again["history_Etot"] and a["history_drho"] == again["history_drho"]        # bitwise
    assert a["alphas"] == again["alphas"] and torch.equal(a["rho"], again["rho"])
    assert a["history_Etot"][:3] != other["history_Etot"][:3]
    assert torch.equal(tight["rho"], rho0) and all(torch.equal(p, q) for p, q in zip(tight["psi"], psi0))
    assert tight["energies"].total == e0 and torch.equal(tight["ham"][0].potential, ham_pot)
    with basis.on_library_stream():
        assert torch.equal(tight["ham"][0] @ tight["psi"][0], Hpsi)
        basis.sync()
    after = dftk.energy_hamiltonian(basis, tight["psi"], tight["occupation"], rho=tight["rho"])[0]
    assert dict(after) == dict(before)


def test_callback_keys(gamma_cell):
    basis = gamma_cell[0]
    seen, lengths = [], []

    def callback(info):
        seen.append(info)
        lengths.append((len(info["history_Etot"]), len(info["history_drho"])))      # (the lists grow in place, as the reference's)
    res = dftk.scf_potential_mixing(basis, damping=0.7, tol=TOL, callback=callback,
                                    is_converged=lambda info: info["n_iter"] >= 3)
    assert res["converged"] and res["n_iter"] == 3 and res["damping_alg"].alpha == 0.7 and res["alphas"] == [0.7, 0.7]
    assert [i["stage"] for i in seen] == ["iterate"] * 3 + ["finalize"] and seen[-1] is res
    for n, i in enumerate(seen[:-1], 1):
        assert i["n_iter"] == n and i["algorithm"] == "SCF" and i["basis"] is basis
        assert isinstance(i["diagonalization"], list) and len(i["diagonalization"]) == 1
        assert "n_iter" in i["diagonalization"][0] and "residual_norms" in i["diagonalization"][0]
        assert (np.isnan(i["alpha"]) if n == 1 else i["alpha"] == 0.7)
        for key in ("ham", "energies", "rho", "rho_in", "Vin", "Vout", "Pinv_dV", "psi", "eigenvalues", "occupation", "eF",
                    "history_Etot", "history_drho", "converged", "runtime", "n_matvec", "sums", "diagtol"):
            assert key in i, key
        assert lengths[n - 1] == (n, n)
    for key in ("alphas", "n_backtracks", "model_relerrors", "history_Etot", "history_drho", "occupation_threshold", "seed",
                "n_bands_converge", "diagonalization", "runtime", "mixing"):
        assert key in res, key


def test_refusals_on_a_device_basis(gamma_cell):
    basis = gamma_cell[0]
    nx, ny, nz = basis.fft_size
    with pytest.raises(ValueError, match="psi has 0 blocks"):
        dftk.scf_potential_mixing(basis, psi=[])
    with pytest.raises(ValueError, match="V must have the shape"):
        dftk.scf_potential_mixing(basis, V=torch.zeros((2, nz, ny, nx), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="max_backtracks"):
        dftk.scf_potential_mixing_adaptive(basis, max_backtracks=0)
    with pytest.raises(ValueError, match="curvature"):
        dftk.scf_potential_mixing(basis, curvature="fd")
    for mixing in (dftk.LdosMixing(), dftk.DielectricMixing(), dftk.HybridMixing()):
        with pytest.raises(NotImplementedError, match="SimpleMixing, KerkerMixing or KerkerDosMixing"):
            dftk.scf_potential_mixing(basis, mixing=mixing)
    with pytest.raises(TypeError, match="damping"):
        dftk.scf_potential_mixing(basis, damping="adaptive")
    pbe = si_basis(PBE, **GAMMA, Ecut=7, fft_size=basis.fft_size, positions=DISPLACED)
    with pytest.raises(NotImplementedError, match="GGA"):
        dftk.scf_potential_mixing_adaptive(pbe, curvature="kernel")
    scan = si_basis(("mgga_x_scan", "mgga_c_scan"), **GAMMA, Ecut=7, fft_size=basis.fft_size, positions=DISPLACED)
    with pytest.raises(NotImplementedError, match="meta-GGA"):
        dftk.scf_potential_mixing(scan)
    hf = dftk.PlaneWaveBasis(dftk.model_HF(*dftk.silicon_cell()), 7, dftk.ExplicitKpoints([[0, 0, 0]], [1.0]),
                             fft_size=basis.fft_size, device="cuda:0")
    with pytest.raises(NotImplementedError, match="exact exchange"):
        dftk.scf_potential_mixing(hf)
