"""Host-only pieces of the response layer (dftk.jl_amd/response.py; reference: src/Smearing.jl:31-56,94-111,
src/response/chi0.jl:268-306,560-667): the divided difference of the occupation function, alpha_mn, and the adaptive
Sternheimer tolerances.  No GPU needed."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import dftk_jl_amd as dftk
from dftk_jl_amd.mixing import occupation_derivative
from dftk_jl_amd.scf import _smear

EF, T = 0.21, 0.03
KINDS = ("fermi_dirac", "gaussian")


def f(kind, e):
    return float(_smear(kind, np.array([(e - EF) / T]))[0])


def fprime_over_T(kind, e):
    return float(occupation_derivative(kind, (e - EF) / T)) / T


@pytest.mark.parametrize("kind", KINDS)
def test_divided_difference_of_separated_arguments_is_the_quotient(kind):
    for a, b in ((0.05, 0.30), (0.20, 0.23), (0.215, 0.19), (-0.4, 0.5), (0.21, 0.26)):
        want = (f(kind, a) - f(kind, b)) / (a - b)
        got = dftk.occupation_divided_difference(kind, a, b, EF, T)
        # the quotient itself is accurate to eps / |a - b| relative to the size of f / |a - b|
        assert abs(got - want) <= 1e-13 / abs(a - b) + 1e-12 * abs(want), (kind, a, b, got, want)


@pytest.mark.parametrize("kind", KINDS)
def test_divided_difference_of_equal_arguments_is_the_derivative(kind):
    for e in (0.05, 0.20, 0.21, 0.24, 0.6):
        want = fprime_over_T(kind, e)
        got = dftk.occupation_divided_difference(kind, e, e, EF, T)
        assert got == pytest.approx(want, rel=1e-14, abs=1e-300), (kind, e)


@pytest.mark.parametrize("kind", KINDS)
def test_divided_difference_is_symmetric(kind):
    rng = np.random.default_rng(3)
    for a, b in rng.uniform(0.0, 0.45, size=(20, 2)):
        ab = dftk.occupation_divided_difference(kind, a, b, EF, T)
        ba = dftk.occupation_divided_difference(kind, b, a, EF, T)
        assert ab == pytest.approx(ba, rel=1e-13, abs=1e-300)
        assert ab <= 0.0                                       # the occupation function decreases


@pytest.mark.parametrize("kind", KINDS)
def test_divided_difference_is_continuous_at_equal_arguments(kind):
    for e in (0.15, 0.21, 0.25):
        d = 1e-6 * T
        near = dftk.occupation_divided_difference(kind, e - d / 2, e + d / 2, EF, T)
        limit = fprime_over_T(kind, e)
        # the symmetric quotient differs from f'(e) by f''' d^2 / 24: far below 1e-9 relative at d = 1e-6 T
        assert near == pytest.approx(limit, rel=1e-9)


def test_divided_difference_at_zero_temperature_is_the_step_function():
    dd = dftk.occupation_divided_difference
    for kind in ("none", "fermi_dirac"):
        assert dd(kind, 0.1, 0.1, EF, 0.0) == 0.0
        assert dd(kind, 0.1, 0.15, EF, 0.0) == 0.0                # both occupied
        assert dd(kind, 0.3, 0.35, EF, 0.0) == 0.0                # both empty
        assert dd(kind, 0.1, 0.3, EF, 0.0) == pytest.approx(1 / (0.1 - 0.3))
        assert dd(kind, 0.3, 0.1, EF, 0.0) == pytest.approx(1 / (0.1 - 0.3))


def test_fermi_dirac_divided_difference_survives_huge_arguments():
    got = dftk.occupation_divided_difference("fermi_dirac", 0.0, 40.0, EF, T)      # exp((40 - eF) / T) overflows
    assert got == pytest.approx((1.0 - 0.0) / (0.0 - 40.0), rel=1e-3)
    assert math.isfinite(got)


def test_alpha_mn_satisfies_its_constraint():
    rng = np.random.default_rng(5)
    for fm, fn, ratio in rng.uniform(0.01, 2.0, size=(20, 3)) * np.array([1, 1, -1]):
        amn = dftk.compute_alpha_mn(fm, fn, ratio)
        anm = dftk.compute_alpha_mn(fn, fm, ratio)
        assert fn * amn + fm * anm == pytest.approx(ratio, rel=1e-14)
    assert dftk.compute_alpha_mn(0.3, 1.7, 0.0) == 0.0
    assert dftk.compute_alpha_mn(0.0, 0.0, 0.0) == 0.0              # empty pair: no 0 / 0
    # one empty state: the formula of orthogonal perturbation theory, alpha_mn = ratio / fn
    assert dftk.compute_alpha_mn(0.0, 2.0, -5.0) == pytest.approx(-2.5)


def toy_basis():
    model = SimpleNamespace(unit_cell_volume=250.0)
    return SimpleNamespace(model=model, fft_size=(10, 12, 15), kweights=[0.25, 0.75])


def test_bandtol_balanced_factors_match_the_closed_form():
    basis = toy_basis()
    occ = [np.array([2.0, 2.0, 1.2, 1e-9]), np.array([2.0, 0.4, 0.0, 0.0])]
    alg = dftk.BandtolBalanced(basis, None, occ, occupation_threshold=1e-6)
    vol, Ng, Nk = 250.0, 10 * 12 * 15, 2
    assert [len(fk) for fk in alg.bandtol_factors] == [3, 2]
    for ik, n_occ in enumerate((3, 2)):
        for n in range(n_occ):
            # sqrt(vol / Ng) / sqrt(n_occ) / (sqrt(n_occ) / sqrt(vol)) / (2 f_nk N_k w_k)
            want = math.sqrt(vol / Ng) * math.sqrt(vol) / n_occ / (2 * occ[ik][n] * Nk * basis.kweights[ik])
            assert alg.bandtol_factors[ik][n] == pytest.approx(want, rel=1e-14)
    assert alg.occupation_threshold == 1e-6
    assert dftk.occupied_empty_masks(occ, 1e-6) == [(3, 4), (2, 4)]
    half = alg.scaled(0.5)
    assert half.bandtol_factors[1][1] == pytest.approx(0.5 * alg.bandtol_factors[1][1])


def test_band_tolerances_are_clamped():
    basis = toy_basis()
    occ = [np.array([2.0, 1e-3]), np.array([2.0, 2.0])]
    alg = dftk.BandtolBalanced(basis, None, occ, occupation_threshold=1e-6, bandtol_min=1e-9, bandtol_max=1e-5)
    tols = dftk.determine_band_tolerances(alg, 1e-8)
    raw = [fk * 1e-8 for fk in alg.bandtol_factors]
    assert raw[0][1] > 1e-5 > raw[0][0] > 1e-9                    # the toy numbers exercise the upper clamp ...
    assert tols[0][1] == 1e-5 and tols[0][0] == raw[0][0]
    tiny = dftk.determine_band_tolerances(alg, 1e-16)               # ... and the lower one
    assert all(np.all(t == 1e-9) for t in tiny)
    free = dftk.BandtolBalanced(basis, None, occ, occupation_threshold=1e-6)
    assert free.bandtol_min == np.finfo(float).eps / 2 and free.bandtol_max == math.inf
    fixed = dftk.BandtolBalanced(basis, None, occ, occupation_threshold=1e-6, bandtol_min=1e-10, bandtol_max=1e-10)
    assert all(np.all(t == 1e-10) for t in dftk.determine_band_tolerances(fixed, 1e-8))


def test_effective_insulator_decision():
    comm = SimpleNamespace(size=1)
    basis = SimpleNamespace(model=SimpleNamespace(smearing="fermi_dirac", temperature=T), comm_kpts=comm)
    assert not dftk.is_effective_insulator(basis, [np.array([0.0, 0.2, 0.4])], EF)
    assert dftk.is_effective_insulator(basis, [np.array([-2.0, 3.0])], EF)          # |e - eF| / T > 36: f < eps
    basis0 = SimpleNamespace(model=SimpleNamespace(smearing="none", temperature=0.0), comm_kpts=comm)
    assert dftk.is_effective_insulator(basis0, [np.array([0.2, 0.21])], EF)


def test_out_of_scope_entries_are_refused():
    with pytest.raises(NotImplementedError, match="dense matrix"):
        dftk.compute_chi0()
    with pytest.raises(NotImplementedError, match="tangent space"):
        dftk.solve_OmegaPlusK()
