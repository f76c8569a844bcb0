"""The references of tests/cube_ref.py checked against each other on the CPU, before tests/test_gpu_cube_kernels.py holds the
kernels of ``csrc/cube_kernels.hip`` to them:

* the Fourier-space symmetrisation (``np.longdouble`` and ``np.fft``) equals the real-space average -- an index permutation of
  the grid per operation, no transform -- on band-limited input, for every group; transposing every S changes the result by
  O(1), so the pair distinguishes the index convention;
* with the low-pass on the symmetrisation is idempotent; on all-odd cubes its result is real to rounding; the mean survives;
* the cube lists cover the parities and the second trip of the grid-stride loops; the committed groups have the sizes the
  crystals are known to have and are what the package's ``symmetry_operations`` finds;
* the gradient and the multipliers agree with closed forms.
"""
import os
import re

import numpy as np
import pytest

import cube_ref as R
from cube_ref import LD

EPS = 2.220446049250313e-16
EPS_LD = float(np.finfo(LD).eps)
# a grid that every operation of the group maps onto itself (Si: w = 1/4 steps and rotations that mix the axes; hcp: w_z = 1/2)
COMPATIBLE = {"si_primitive": (12, 12, 12), "hcp": (12, 12, 20), "si_conventional": (12, 12, 12), "si_supercell_222": (12, 12, 12),
              "triclinic_pair": (10, 15, 16), "si_centring": (12, 12, 20)}


@pytest.fixture(scope="module")
def groups():
    assert EPS_LD < 2e-19, "np.longdouble must be the 80-bit extended type"
    return R.load_groups()


def relmax(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_cube_lists_cover_parities_and_the_second_trip():
    assert R.TRIP == 524288
    parities = [tuple(n % 2 for n in c) for c in R.SMALL_CUBES]
    assert (1, 1, 1) in parities and (0, 0, 0) in parities and any(len(set(p)) == 2 for p in parities)
    for c in R.LARGE_CUBES:
        assert np.prod(c) > R.TRIP
    assert [int(np.prod(c)) for c in R.LARGE_CUBES] == [531441, 552960]
    assert {tuple(n % 2 for n in c) for c in R.LARGE_CUBES} == {(1, 1, 1), (0, 0, 0)}


def test_second_trip_constant_is_the_launch_geometry_of_the_kernels():
    """``cube_ref.TRIP`` decides which cubes count as large: it must be what csrc/cube_kernels.hip launches, or a change of
    the grid there would quietly take the second trip out of the GPU tests (or put the small cubes into one)."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dftk.jl_amd", "csrc", "cube_kernels.hip")).read()
    blocks = re.findall(r"const int CUBE_BLOCKS = (\d+);", src)
    assert len(blocks) == 1 and int(blocks[0]) * 256 == R.TRIP
    assert max(int(np.prod(c)) for c in R.SMALL_CUBES) < R.TRIP


def test_group_sizes(groups):
    for name, (n, n_tau) in R.EXPECTED.items():
        g = groups[name]
        assert len(g) == n, name
        if n_tau is not None:
            assert g.n_translated() == n_tau, name
        assert np.array_equal(np.rint(g.tau * 4), g.tau * 4), name          # every tau is a double without rounding
        keys = {(tuple(W.ravel()), tuple(num * (4 // den))) for W, num, den in zip(g.W, g.w_num, g.w_den)}
        assert len(keys) == n, name                                         # no operation twice
    assert len(groups["si_conventional"].pure_translations()) == 4
    assert len(groups["si_supercell_222"].pure_translations()) == 8
    c = groups["si_centring"]
    assert np.all(c.S == np.eye(3, dtype=int)) and c.n_translated() == 3
    t = groups["triclinic_pair"]
    assert sorted(int(W[0, 0]) for W in t.W) == [-1, 1] and not t.tau.any()


@pytest.mark.parametrize("name", ["si_primitive", "hcp", "triclinic_pair"])
def test_committed_groups_are_what_the_package_finds(groups, name):
    """(the three cells whose search takes well under a second; the fixture as a whole comes from ``cube_ref.generate_groups``)"""
    new, old = R.group_from_package(name), groups[name]
    assert np.array_equal(new.W, old.W) and np.array_equal(new.w_num * old.w_den[:, None], old.w_num * new.w_den[:, None])


def test_long_dft_against_numpy_and_round_trip():
    rng = np.random.default_rng(0)
    for shape in [(4, 5, 6), (7, 3, 8)]:
        x = rng.standard_normal(shape)
        c = R.dftn(x)
        assert relmax(c.astype(complex), np.fft.fftn(x)) < 16 * EPS
        assert relmax(R.dftn(c, +1) / x.size, x.astype(R.CLD)) < 64 * EPS_LD


@pytest.mark.parametrize("name", sorted(COMPATIBLE))
def test_fourier_equals_realspace_on_band_limited_input(groups, name):
    g, cube = groups[name], COMPATIBLE[name]
    assert R.grid_compatible(g, cube)
    rho = R.band_limited(np.random.default_rng(1), g.lattice, cube)
    ref = R.symmetrize_realspace(rho, g, cube)
    for lowpass in (0, 1):
        long = R.symmetrize_fourier(rho, g, cube, lowpass)
        double = R.symmetrize_fourier(rho, g, cube, lowpass, precision="double")
        # band_limited leaves coefficients of 1e-16 outside the ball, which the two sides treat differently
        assert relmax(long.real, ref) < 32 * EPS and np.abs(long.imag).max() < 32 * EPS * np.abs(ref).max(), (name, lowpass)
        assert relmax(double.real, ref) < 32 * EPS, (name, lowpass)
    if len(g) > 2 and name != "si_centring":
        # the index convention: S <-> S' (with tau as it is) is another operator
        swapped = R.Group(name, g.lattice, g.W.transpose(0, 2, 1), g.w_num, g.w_den)
        swapped.tau = g.tau
        assert relmax(R.symmetrize_fourier(rho, swapped, cube, 0).real, ref) > 0.1, name


def test_the_centring_group_is_the_translation_average(groups):
    g, cube = groups["si_centring"], (12, 12, 20)
    rho = np.random.default_rng(2).standard_normal(cube[::-1])
    shifts = [[-int(p * n // q) for p, n in zip(num[::-1], cube[::-1])] for num, q in zip(g.w_num, g.w_den)]   # rho(r + w)
    want = sum(np.roll(rho, s, axis=(0, 1, 2)) for s in shifts) / 4
    assert relmax(R.symmetrize_realspace(rho, g, cube).astype(float), want) < 4 * EPS
    assert relmax(want, rho) > 0.1


@pytest.mark.parametrize("cube", R.SMALL_CUBES)
def test_idempotent_with_lowpass_real_on_odd_cubes_and_mean(groups, cube):
    rho = np.random.default_rng(3).standard_normal(cube[::-1]) + 0.3
    for name, g in groups.items():
        once = R.symmetrize_fourier(rho, g, cube, 1)
        twice = R.symmetrize_fourier(once.real, g, cube, 1)
        scale = np.abs(once).max()
        assert np.abs(twice.real - once.real).max() < 64 * EPS_LD * max(len(g), 8) * scale, name
        plain = R.symmetrize_fourier(rho, g, cube, 0)
        if all(n % 2 for n in cube):
            assert np.abs(once.imag).max() < 64 * EPS_LD * scale and np.abs(plain.imag).max() < 64 * EPS_LD * scale, name
        for out in (once, plain):          # the G = 0 entry: every S^-1 0 = 0 is on the grid, the phase is 1
            assert abs(out.real.mean() - rho.astype(LD).mean()) < 64 * EPS_LD * np.abs(rho).max(), name


def test_lowpass_matters_on_the_mixed_cube(groups):
    """on (10, 15, 16) S G leaves the grid for most rotations of Si: the two settings differ by O(1) there"""
    cube = (10, 15, 16)
    rho = np.random.default_rng(4).standard_normal(cube[::-1])
    g = groups["si_primitive"]
    a, b = (R.symmetrize_fourier(rho, g, cube, lp, precision="double").real for lp in (0, 1))
    assert relmax(a, b) > 0.05


@pytest.mark.parametrize("cube", R.SMALL_CUBES)
def test_gradient_reference_against_the_analytic_gradient(cube):
    rng = np.random.default_rng(5)
    G, amp, phi = R.random_modes(rng, cube, 24, corners=True)
    assert np.all(np.abs(G) <= R.paired_max(cube)) and len({tuple(g) for g in G}) == 24
    f, grad = R.trig_polynomial(R.SHEARED, cube, G, amp, phi)
    assert relmax(R.gradient(f, R.SHEARED, cube), grad) < 256 * EPS_LD
    f64, grad64 = R.trig_polynomial(R.SHEARED, cube, G, amp, phi, precision="double")
    assert relmax(f64, f) < 64 * EPS and relmax(grad64, grad) < 64 * EPS
    assert relmax(R.gradient(f64, R.SHEARED, cube, precision="double"), grad) < 64 * EPS


def test_gradient_reference_of_a_pure_nyquist_component_is_zero():
    """the Nyquist entry of an even axis carries G = -n/2 and the real part is taken at the end: i G c (-1)^i is imaginary"""
    for cube, axis in (((12, 12, 20), 0), ((12, 12, 20), 2), ((10, 15, 16), 0), ((10, 15, 16), 2)):
        f = R.nyquist_wave(cube, axis, 0.7)
        assert f.shape == cube[::-1] and set(np.unique(f)) == {-0.7, 0.7}
        assert np.abs(R.gradient(f, R.SHEARED, cube)).max() < 64 * EPS_LD
        assert np.abs(R.gradient(f, R.SHEARED, cube, precision="double")).max() < 64 * EPS


def test_multipliers():
    cube, kTF, eps_r = (10, 15, 16), 0.9, 7.0
    G2 = R.g_squared(R.SHEARED, cube)
    G2l = R.g_squared(R.SHEARED, cube, LD)
    assert relmax(G2l.astype(float), G2) < 8 * EPS and G2.flat[0] == 0.0
    k, d, c = R.kerker_multiplier(G2, cube, kTF), R.dielectric_multiplier(G2, kTF, eps_r), R.chi0_multiplier(G2, kTF, eps_r)
    ny = R.unpaired_nyquist(cube)
    assert ny.sum() == 15 * 16 + 10 * 15 - 15 and k.flat[0] == d.flat[0] == 1.0 and c.flat[0] == 0.0
    assert np.all(k[ny] == 0.0) and np.all((k[~ny] >= 0) & (k[~ny] <= 1.0))
    far = G2 > 1e3 * kTF ** 2
    assert np.all(np.abs(d - 1.0)[far] < 2e-3) and abs(d.flat[1] - (kTF ** 2 + 6 * G2.flat[1]) / (7 * kTF ** 2 + 6 * G2.flat[1])) < 4 * EPS
    assert np.all(c.ravel()[1:] < 0)          # chi0 of the dielectric model is negative
    x = np.random.default_rng(6).standard_normal(cube[::-1]) + 0.3
    for m in (k, d):
        out = R.apply_multiplier(x, m.astype(LD))
        assert abs(out.mean() - x.astype(LD).mean()) < 64 * EPS_LD          # the G = 0 coefficient survives
        assert relmax(R.apply_multiplier(x, m, precision="double"), out) < 32 * EPS
    assert np.abs(np.fft.fftn(R.apply_multiplier(x, k.astype(LD)).astype(float))[ny]).max() < 64 * EPS * x.size
