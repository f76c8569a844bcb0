"""Host-side pieces of compute_stresses_cart (no GPU): the Voigt helpers (stresses.jl:56-77), symmetrize_stresses
(symmetry.jl:362-374), the Ewald stress against central differences of the oracle's ``energy_ewald`` on strained
lattices, the PspCorrection stress and the analytic derivative of the HGH local form factor.

Ewald yardstick: sigma_ab = [E((I + eps) L) - E((I - eps) L)] / (2 h Omega), eps = h/2 (e_a e_b' + e_b e_a'), h = 1e-5,
reduced positions fixed.  Its truncation error is O(h^2) (checked against h = 1e-4: 1e-7 relative), its round-off
eps_mach |E| / (h Omega) ~ 1e-11 relative; tolerance 1e-8 of the largest component."""
import numpy as np
import pytest
import torch

import dftk_jl_amd as dftk
from dftk_jl_amd import psp as lpsp
from dftk_jl_amd.stresses import (compute_stresses_term, full_strain_to_voigt, full_stress_to_voigt,
                                  voigt_strain_to_full, voigt_stress_to_full)
from dftk_jl_amd.terms import stress_ewald

from oracle.terms import energy_ewald as oracle_energy_ewald

from test_hgh_channels import SYNTH, synthetic_library_psp

# the sheared seven-atom cell of test_gpu_multispecies.py (Si, X = every HGH channel, C, Fe, H-like local-only)
LATTICE7 = np.array([[7.4, 0.9, -0.6], [0.4, 6.9, 1.1], [-0.7, 0.5, 7.8]])
POSITIONS7 = [np.array(p) for p in ([0.02, 0.03, 0.05], [0.27, 0.21, 0.09], [0.51, 0.46, 0.13], [0.77, 0.69, 0.33],
                                    [0.14, 0.62, 0.58], [0.43, 0.88, 0.71], [0.69, 0.31, 0.86])]
CHARGES7 = [4.0, float(SYNTH["Zion"]), 4.0, 8.0, 1.0, 4.0, float(SYNTH["Zion"])]
TWISTED_SI = 10.0 / 2 * np.array([[0, 1, 1.05], [1, 0, 1], [1, 1, 0]])
SI_POSITIONS = [np.ones(3) / 8, -np.ones(3) / 8]


# ------------------------------------------------------------------------------------------ Voigt helpers
def test_voigt_helpers_round_trip_in_the_reference_order():
    v = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])           # xx, yy, zz, zy, zx, yx
    s = voigt_stress_to_full(v)
    assert np.array_equal(s, np.array([[1.0, 6.0, 5.0], [6.0, 2.0, 4.0], [5.0, 4.0, 3.0]]))
    assert np.array_equal(full_stress_to_voigt(s), v)
    assert np.array_equal(voigt_strain_to_full(np.zeros(6)), np.eye(3))
    e = voigt_strain_to_full(v)
    assert np.array_equal(e, np.array([[2.0, 3.0, 2.5], [3.0, 3.0, 2.0], [2.5, 2.0, 4.0]]))
    assert np.allclose(full_strain_to_voigt(e), v, rtol=0, atol=1e-15)
    # a non-symmetric matrix: the stress helper averages the off-diagonal pairs
    a = np.arange(9.0).reshape(3, 3)
    assert np.array_equal(full_stress_to_voigt(a), [0.0, 4.0, 8.0, 6.0, 4.0, 2.0])
    # the work of a stress against a strain is the plain dot product of the two Voigt vectors
    rng = np.random.default_rng(0)
    sv, ev = rng.standard_normal(6), rng.standard_normal(6)
    assert abs(np.sum(voigt_stress_to_full(sv) * (voigt_strain_to_full(ev) - np.eye(3))) - sv @ ev) < 1e-14
    for name in ("voigt_stress_to_full", "full_stress_to_voigt", "voigt_strain_to_full", "full_strain_to_voigt",
                 "compute_stresses_cart", "compute_stresses_term", "symmetrize_stresses"):
        assert hasattr(dftk, name), name


# ------------------------------------------------------------------------------------------ symmetrize_stresses
def _si_model(symmetries, lattice=None):
    lat, atoms, pos = dftk.silicon_cell()
    return dftk.model_DFT(lat if lattice is None else lattice, atoms, pos, functionals=("lda_x", "lda_c_vwn"),
                          symmetries=symmetries)


def test_symmetrize_stresses():
    rng = np.random.default_rng(4)
    A = rng.standard_normal((3, 3))
    S = A + A.T
    ident = _si_model(False)
    assert len(ident.symmetries) == 1
    assert np.array_equal(dftk.symmetrize_stresses(ident, S, symmetries=ident.symmetries), S)
    fcc = _si_model(True)
    assert len(fcc.symmetries) == 48
    Ss = dftk.symmetrize_stresses(fcc, S, symmetries=fcc.symmetries)
    assert np.max(np.abs(Ss - np.trace(S) / 3 * np.eye(3))) < 1e-13
    assert np.max(np.abs(dftk.symmetrize_stresses(fcc, Ss, symmetries=fcc.symmetries) - Ss)) < 1e-13
    # a twisted cell keeps a subgroup: the result is invariant under every remaining operation and idempotent
    tw = _si_model(True, lattice=TWISTED_SI)
    assert 1 < len(tw.symmetries) < 48
    St = dftk.symmetrize_stresses(tw, S, symmetries=tw.symmetries)
    assert np.max(np.abs(dftk.symmetrize_stresses(tw, St, symmetries=tw.symmetries) - St)) < 1e-13
    assert np.max(np.abs(St - St.T)) < 1e-13 and abs(np.trace(St) - np.trace(S)) < 1e-13
    Linv = np.linalg.inv(TWISTED_SI)
    for op in tw.symmetries:
        Wc = TWISTED_SI @ op.W @ Linv
        assert np.max(np.abs(Wc @ St @ np.linalg.inv(Wc) - St)) < 1e-13


# ------------------------------------------------------------------------------------------ Ewald
def _fd_ewald_stress(lattice, charges, positions, h):
    vol = abs(np.linalg.det(lattice))
    out = np.zeros((3, 3))
    for a in range(3):
        for b in range(a + 1):
            eps = np.zeros((3, 3))
            eps[a, b] += h / 2
            eps[b, a] += h / 2
            Ep = oracle_energy_ewald((np.eye(3) + eps) @ lattice, charges, positions)
            Em = oracle_energy_ewald((np.eye(3) - eps) @ lattice, charges, positions)
            out[a, b] = out[b, a] = (Ep - Em) / (2 * h * vol)
    return out


@pytest.mark.parametrize("system", ["seven_atoms", "twisted_si"])
def test_ewald_stress_matches_finite_differences(system):
    if system == "seven_atoms":
        lat, q, pos = LATTICE7, CHARGES7, POSITIONS7
    else:
        lat, q, pos = TWISTED_SI, [4.0, 4.0], SI_POSITIONS
    S = stress_ewald(lat, q, pos)
    ref = _fd_ewald_stress(lat, q, pos, 1e-5)
    coarse = _fd_ewald_stress(lat, q, pos, 1e-4)
    scale = np.max(np.abs(ref))
    print(system, "max |analytic - fd| / scale =", np.max(np.abs(S - ref)) / scale,
          "fd(1e-4) vs fd(1e-5):", np.max(np.abs(coarse - ref)) / scale)
    assert np.max(np.abs(coarse - ref)) <= 1e-7 * scale            # the yardstick itself
    assert np.max(np.abs(S - ref)) <= 1e-8 * scale, (S, ref)
    assert np.array_equal(S, S.T)


def test_ewald_stress_trace_on_a_cubic_cell():
    """E_ewald scales as 1 / a under a uniform dilation: tr sigma = -E / Omega; cubic symmetry makes sigma isotropic."""
    a = 6.3
    lat = a * np.eye(3)
    pos = [np.zeros(3), np.ones(3) / 2]
    q = [3.0, 5.0]
    S = stress_ewald(lat, q, pos)
    E = oracle_energy_ewald(lat, q, pos)
    assert abs(np.trace(S) + E / a ** 3) <= 1e-12 * abs(E / a ** 3)
    assert np.max(np.abs(S - np.trace(S) / 3 * np.eye(3))) <= 1e-13 * abs(np.trace(S))


# ------------------------------------------------------------------------------------------ PspCorrection, Entropy, errors
def test_psp_correction_stress_and_term_names():
    model = dftk.model_DFT(TWISTED_SI, dftk.silicon_cell()[1], SI_POSITIONS, functionals=("lda_x", "lda_c_vwn"),
                           temperature=0.01)
    basis = dftk.PlaneWaveBasis(model, 5, dftk.MonkhorstPack((1, 1, 1)), device="cpu")
    S = compute_stresses_term("PspCorrection", basis, None, None)
    assert np.array_equal(S, -basis.terms.E_pspcorr / model.unit_cell_volume * np.eye(3))
    assert basis.terms.E_pspcorr != 0
    assert compute_stresses_term("Entropy", basis, None, None) is None
    Se = compute_stresses_term("Ewald", basis, None, None)
    assert np.array_equal(Se, stress_ewald(TWISTED_SI, [4.0, 4.0], SI_POSITIONS))
    with pytest.raises(ValueError):
        compute_stresses_term("Magnetic", basis, None, None)
    with pytest.raises(RuntimeError):          # device terms have no CPU fall-back
        compute_stresses_term("Kinetic", basis, None, None)


# ------------------------------------------------------------------------------------------ local form factor
def _table_psps():
    out = {f"{sym}/{fun}": lpsp.load_psp(sym, fun) for (sym, fun) in lpsp._TABLE}
    out["synthetic"] = synthetic_library_psp()
    return out


@pytest.mark.parametrize("name", sorted(_table_psps()))
def test_local_form_factor_derivative(name):
    """Central differences of eval_psp_local_fourier in p (h = 1e-5: truncation ~ h^2 |ff'''| / 6, round-off
    ~ 1e-16 |ff| / h; both below 1e-8 of the derivative on this range)."""
    psp = _table_psps()[name]
    p = torch.linspace(0.5, 12.0, 400, dtype=torch.float64)
    h = 1e-5
    fd = (lpsp.eval_psp_local_fourier(psp, p + h) - lpsp.eval_psp_local_fourier(psp, p - h)) / (2 * h)
    an = lpsp.eval_psp_local_fourier_derivative(psp, p)
    err = float((an - fd).abs().max())
    scale = float(fd[p > 1.0].abs().max())
    print(name, "max |analytic - fd| =", err, "scale", scale)
    assert float(((an - fd).abs() / (fd.abs() + scale)).max()) <= 1e-8
    assert float(lpsp.eval_psp_local_fourier_derivative(psp, torch.zeros(1, dtype=torch.float64))[0]) == 0.0


# ------------------------------------------------------------------------------------------ the kernels' closed forms
def test_device_closed_forms_against_finite_differences_on_the_host():
    """The __host__ __device__ functions of stress_kernels.hip (HGH radial forms and solid harmonics with their
    derivatives -> the six dP_ab; the local form-factor derivative) through tools/host_stress_check.cpp, which includes
    the kernels' source and runs without a GPU: every tabulated channel against central differences of the strained
    projector, 1e-8 of the channel's largest derivative."""
    import subprocess
    from dftk_jl_amd import _build
    exe = _build.build_host_stress_check()
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout[-3000:], res.stderr[-2000:])
    assert "host_stress_check OK" in res.stdout and "FAILED" not in res.stdout
