"""The density-sized passes of ``csrc/cube_kernels.hip`` at the C ABI -- ``dftk_mi_symmetrize_rho``, ``dftk_mi_cube_gradient``,
``dftk_mi_mix_kerker``, ``dftk_mi_mix_dielectric``, ``dftk_mi_chi0_dielectric_apply``, ``dftk_mi_cube_fourier_filter`` -- against
the references of tests/cube_ref.py (checked against each other on the CPU in tests/test_cube_reference.py).  No reference
calls the library, the package's torch twin or ``oracle/``.

Every kernel of the family is a grid-stride loop of 2048 workgroups x 256 threads, so a second trip starts at cube entry
524 288 (``cube_ref.TRIP``).  Cubes: (15, 15, 15) all odd, (12, 12, 20) all even (hcp's tau_z = 1/2 stays on the grid),
(10, 15, 16) mixed (S G leaves the grid for most rotations); (81, 81, 81) and (96, 90, 64), N = 531 441 and 552 960, run
the second trip -- there the entries from ``TRIP`` on are also held to the bound on their own.  Groups
(tests/golden/cube_symmetry_groups.json): primitive Si (48 operations), hcp (24, hexagonal), conventional Si (192, the most
one launch holds), the 2 x 2 x 2 Si supercell (384: two chunks), a triclinic pair (identity + inversion) and the four centring
translations of conventional Si alone (S = I, tau != 0: the identity shortcut must not fire).

Tolerances.  Small cubes: e = max|got - ref| / max|ref| against the ``np.longdouble`` reference (or the transform-free real-space
average / the analytic gradient); the yardstick y is the same error of the float64 NumPy restatement (``np.fft``) of the same
operation; e <= max(8 y, 32 eps): the device FFT and NumPy's differ in factorisation and summation order.  Large cubes:
max|got - ref| <= 1e-12 max|ref| against the float64 restatement, the bound tests/test_gpu_symmetry.py holds the kernel to.
The mean: |mean(out) - mean(in)| <= 16 eps max|in| (the G = 0 coefficient is a sum tree over N <= 2^20 entries, error
<= log2(N) / 2 eps max|in| after the division by N, and passes through the multiplier unchanged).  Linearity of the gradient:
each of the three gradients is within 32 eps of the exact (linear) operator, so their defect is within 32 eps of the three
magnitudes summed.

Measured on an MI355X (worst over the cases of each line; ``pytest -s`` prints every figure):
  symmetrise, small cubes, 6 groups x 3 cubes x low-pass off / on     err <= 12.0 eps (384 operations, 12 x 12 x 20; yardstick
                                                                      17.1 eps), err / bound <= 0.123 (192 operations, 10 x 15 x 16)
  symmetrise, chunk edges (193, 383, 384 reversed, 385 operations)    err <= 12.2 eps, err / bound <= 0.111
  symmetrise against the real-space average                           err <= 8.1 eps, err / bound <= 0.089
  ``symmetrize_rho`` of the 384-operation supercell basis, 20^3       err 19.6 eps (yardstick 32.2 eps), err / bound 0.076
  symmetrise, second trip (81^3, 96 x 90 x 64)                        <= 2.5e-15 max|ref|, its second trip alone <= 3.1e-15
  gradient, small cubes                                               err <= 1.95 eps, err / bound <= 0.061
  gradient, second trip                                               <= 1.1e-15 max|ref|
  gradient of a pure Nyquist component                                (8, 16, 4): 0 on all three axes; elsewhere <= 2.7e-16
                                                                      for a = 0.75 (0.004 of the bound), 0 on the 12-axes
  gradient linearity                                                  defect / bound <= 0.035
  multipliers, (10, 15, 16)                                           err <= 1.80 eps, err / bound <= 0.056
  multipliers, second trip                                            <= 6.1e-16 max|ref|
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check as abi_check  # noqa: E402

import cube_ref as R  # noqa: E402
from test_gpu_kernels import Basis, KBlock, dev  # noqa: E402

EPS = 2.220446049250313e-16
EINVAL = -1               # DFTK_MI_EINVAL (include/dftk_mi355x.h)
NAN = float("nan")
KTF, EPS_R = 0.9, 7.0
GROUP_NAMES = ["si_primitive", "hcp", "si_conventional", "si_supercell_222", "triclinic_pair", "si_centring"]
# grids that every operation of the group maps onto itself: the real-space average exists there
COMPATIBLE = [("si_primitive", (12, 12, 12)), ("si_conventional", (12, 12, 12)), ("si_supercell_222", (12, 12, 12)),
              ("hcp", (12, 12, 20)), ("si_centring", (12, 12, 20)), ("triclinic_pair", (15, 15, 15)),
              ("triclinic_pair", (10, 15, 16))]
GROUPS = R.load_groups()


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


class Cube:
    """a basis and its cube k-block (the "sphere" is the whole cube)"""

    def __init__(self, lib, fft_size, lattice=R.SHEARED):
        nx, ny, nz = fft_size
        self.lib, self.fft_size, self.shape, self.N = lib, tuple(fft_size), (nz, ny, nx), nx * ny * nz
        self.lattice = np.asarray(lattice, dtype=float)
        self.BH = np.asfortranarray(R.recip(self.lattice))          # column-major, as the header asks
        self.bs = Basis(lib, nx, ny, nz, abs(np.linalg.det(self.lattice)))
        self.kb = KBlock(lib, self.bs, np.arange(self.N), np.zeros(self.N))

    def symmetrize_status(self, S_h, tau_h, lowpass, x, out):
        torch.cuda.synchronize()
        st = self.lib.dftk_mi_symmetrize_rho(self.kb.h, len(S_h), S_h.ctypes.data, tau_h.ctypes.data, lowpass, x.data_ptr(),
                                             out.data_ptr())
        self.bs.sync()
        return st

    def symmetrize(self, group, lowpass, rho, inplace=False):
        S_h, tau_h = group.abi()
        x = dev(np.array(rho))
        out = x if inplace else torch.full_like(x, NAN)
        abi_check(self.symmetrize_status(S_h, tau_h, lowpass, x, out))
        return out.cpu().numpy()

    def gradient(self, f):
        fd = dev(np.array(f))
        out = torch.full((3,) + self.shape, NAN, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        abi_check(self.lib.dftk_mi_cube_gradient(self.kb.h, self.BH.ctypes.data, fd.data_ptr(), out.data_ptr()))
        self.bs.sync()
        return out.cpu().numpy()

    def filter(self, entry, x, *args):
        xd = dev(np.array(x))
        out = torch.full(self.shape, NAN, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        abi_check(getattr(self.lib, entry)(self.kb.h, *args, xd.data_ptr(), out.data_ptr()))
        self.bs.sync()
        return out.cpu().numpy()


@pytest.fixture(scope="module")
def cubes(lib):
    made = {}

    def get(fft_size):
        if fft_size not in made:
            made[fft_size] = Cube(lib, fft_size)
        return made[fft_size]
    return get


@functools.lru_cache(maxsize=None)
def random_cube(fft_size, seed=11):
    x = np.random.default_rng(seed).standard_normal(tuple(fft_size)[::-1]) + 0.3
    x.setflags(write=False)
    return x


def maxabs(a):
    return float(np.abs(a).max())


def check_small(tag, got, ref, restated):
    """max(8 x the float64 restatement's own error, 32 eps), relative to max|ref| (module docstring)"""
    assert np.all(np.isfinite(got)), tag
    scale = maxabs(ref)
    err, yard = maxabs(got - ref) / scale, maxabs(restated - ref) / scale
    bound = max(8 * yard, 32 * EPS)
    print(f"\n{tag}: err {err / EPS:.2f} eps, yardstick {yard / EPS:.2f} eps, err / bound = {err / bound:.3f}")
    assert err <= bound, tag


def check_large(tag, got, ref):
    """1e-12 max|ref| on the whole cube, and on the entries of the second trip by themselves"""
    assert np.all(np.isfinite(got)), tag
    lead = got.shape[:-3]
    g, r = got.reshape(lead + (-1,)), np.asarray(ref).reshape(lead + (-1,))
    assert g.shape[-1] > R.TRIP
    err, tail = maxabs(g - r) / maxabs(r), maxabs(g[..., R.TRIP:] - r[..., R.TRIP:]) / maxabs(r[..., R.TRIP:])
    print(f"\n{tag}: err / (1e-12 max|ref|) = {err / 1e-12:.2e}, second trip alone {tail / 1e-12:.2e}")
    assert g[..., R.TRIP:].any() and maxabs(r[..., R.TRIP:]) > 0.01 * maxabs(r), tag
    assert err <= 1e-12 and tail <= 1e-12, tag


# ======================================================================================= dftk_mi_symmetrize_rho
@pytest.mark.parametrize("fft_size", R.SMALL_CUBES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_symmetrize_random_input_against_long_double(cubes, name, fft_size):
    """Every group on every small cube, random (not band-limited) input, low-pass off and on.  n_sym = 192 is one launch,
    n_sym = 384 two chunks; S_h is column-major and not symmetric for Si and hcp, so the transpose of the entry is pinned."""
    group, cube, rho = GROUPS[name], cubes(fft_size), random_cube(fft_size)
    for lowpass in (0, 1):
        ref = R.symmetrize_fourier(rho, group, fft_size, lowpass).real
        restated = R.symmetrize_fourier(rho, group, fft_size, lowpass, precision="double").real
        got = cube.symmetrize(group, lowpass, rho)
        check_small(f"symmetrize {name} {fft_size} lowpass={lowpass}", got, ref, restated)
        assert abs(got.mean() - rho.mean()) <= 16 * EPS * maxabs(rho), (name, lowpass)


@pytest.mark.parametrize("name,fft_size", COMPATIBLE, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_symmetrize_band_limited_input_against_the_realspace_average(cubes, name, fft_size):
    """The reference holds no transform: (1 / n) sum rho(W r + w) as a permutation of the grid per operation."""
    group, cube = GROUPS[name], cubes(fft_size)
    rho = R.band_limited(np.random.default_rng(12), group.lattice, fft_size)
    ref = R.symmetrize_realspace(rho, group, fft_size)
    for lowpass in (0, 1):
        restated = R.symmetrize_fourier(rho, group, fft_size, lowpass, precision="double").real
        check_small(f"symmetrize vs real space {name} {fft_size} lowpass={lowpass}", cube.symmetrize(group, lowpass, rho), ref,
                    restated)


@pytest.mark.parametrize("lowpass", [0, 1])
@pytest.mark.parametrize("fft_size", R.LARGE_CUBES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("name", ["si_primitive", "hcp"])
def test_symmetrize_second_trip(cubes, name, fft_size, lowpass):
    group, rho = GROUPS[name], random_cube(fft_size)
    assert rho.size > R.TRIP
    ref = R.symmetrize_fourier(rho, group, fft_size, lowpass, precision="double").real
    check_large(f"symmetrize {name} {fft_size} lowpass={lowpass}", cubes(fft_size).symmetrize(group, lowpass, rho), ref)


@pytest.mark.parametrize("pick", ["first 193", "first 383", "all 384 reversed", "all 384 and the first again"])
def test_symmetrize_chunk_edges(cubes, pick):
    """More than 192 operations go through in chunks of 192: a second chunk of one operation, of 191, of 192 in another order, and
    a third chunk of one.  On (10, 15, 16) the low-pass of either chunk clears entries the other chunk fills: a cleared entry
    must stay cleared.  (The lists are no groups; the operator is defined for any list.)"""
    full, fft_size = GROUPS["si_supercell_222"], (10, 15, 16)
    sel = {"first 193": np.arange(193), "first 383": np.arange(383), "all 384 reversed": np.arange(384)[::-1],
           "all 384 and the first again": np.r_[np.arange(384), 0]}[pick]
    group, rho = full.subset(sel), random_cube(fft_size)
    G = R.g_cube(fft_size)
    kept = [np.logical_and.reduce([R.index_of(G @ S.T, fft_size)[0] for S in group.S[a:a + 192]]) for a in (0, 192)]
    assert (kept[0] & ~kept[1]).any() or (kept[1] & ~kept[0]).any()          # one chunk clears what the other keeps
    for lowpass in (0, 1):
        ref = R.symmetrize_fourier(rho, group, fft_size, lowpass).real
        restated = R.symmetrize_fourier(rho, group, fft_size, lowpass, precision="double").real
        check_small(f"symmetrize chunks {pick} lowpass={lowpass}", cubes(fft_size).symmetrize(group, lowpass, rho), ref, restated)


def test_symmetrize_centring_translations_alone(cubes):
    """S = I for all four operations, tau != 0 for three: the translation average, not the copy of the identity-only case."""
    group, fft_size = GROUPS["si_centring"], (12, 12, 20)
    rho = random_cube(fft_size)
    shifts = [[-int(p * n // q) for p, n in zip(num[::-1], fft_size[::-1])] for num, q in zip(group.w_num, group.w_den)]
    want = sum(np.roll(rho, s, axis=(0, 1, 2)).astype(R.LD) for s in shifts) / 4          # rho(r + w) averaged
    assert maxabs(want - rho) > 0.1 * maxabs(rho)
    for lowpass in (0, 1):          # (the Nyquist planes are mapped onto themselves by S = I: nothing is cleared)
        got = cubes(fft_size).symmetrize(group, lowpass, rho)
        restated = R.symmetrize_fourier(rho, group, fft_size, lowpass, precision="double").real
        check_small(f"centring lowpass={lowpass}", got, want, restated)
        assert maxabs(got - rho) > 0.1 * maxabs(rho)


def test_symmetrize_table_cache_is_keyed_by_content(lib):
    """The tables stay on the basis between calls, keyed by a hash of their content.  A, then lists of the SAME length with other
    content (A in another order; hcp twice), then A again, on one basis: each result has the bits of the same call on a fresh
    basis.  Likewise one group on two cube sizes, alternating."""
    A = GROUPS["si_primitive"]
    hcp = GROUPS["hcp"]
    seq = [A, A.subset(np.arange(48)[::-1]), A, hcp.subset(np.r_[np.arange(24), np.arange(24)]), A]
    assert {len(g) for g in seq} == {48}
    fft_size = (15, 15, 15)
    rho = random_cube(fft_size)
    shared = Cube(lib, fft_size)
    got = [shared.symmetrize(g, 1, rho) for g in seq]
    fresh = [Cube(lib, fft_size).symmetrize(g, 1, rho) for g in seq]
    for i, (a, b) in enumerate(zip(got, fresh)):
        assert np.array_equal(a, b), i
    assert np.array_equal(got[0], got[2]) and np.array_equal(got[0], got[4])
    assert maxabs(got[3] - got[0]) > 0.01 * maxabs(got[0])                   # hcp's operations are another operator
    assert maxabs(got[1] - got[0]) <= 32 * EPS * maxabs(got[0])              # the same group in another order
    pair = {c: Cube(lib, c) for c in ((15, 15, 15), (12, 12, 20))}
    for c in ((15, 15, 15), (12, 12, 20), (15, 15, 15), (12, 12, 20)):
        assert np.array_equal(pair[c].symmetrize(A, 1, random_cube(c)), Cube(lib, c).symmetrize(A, 1, random_cube(c))), c


@pytest.mark.parametrize("name", ["si_primitive", "si_supercell_222"])
def test_symmetrize_in_place_gives_the_same_bits(cubes, name):
    fft_size = (10, 15, 16)
    rho = random_cube(fft_size)
    for lowpass in (0, 1):
        apart = cubes(fft_size).symmetrize(GROUPS[name], lowpass, rho)
        assert np.array_equal(cubes(fft_size).symmetrize(GROUPS[name], lowpass, rho, inplace=True), apart)


def test_symmetrize_refusals_leave_the_output_alone(cubes):
    fft_size = (15, 15, 15)
    cube, x = cubes(fft_size), dev(np.array(random_cube(fft_size)))
    S_h, tau_h = GROUPS["si_supercell_222"].abi()
    out = torch.full_like(x, 7.25)
    assert cube.symmetrize_status(S_h[:0], tau_h[:0], 1, x, out) == EINVAL            # n_sym = 0
    for n, where in ((1, 0), (48, 47), (384, 200)):                                  # det S = 2, also in the second chunk
        bad = S_h[:n].copy()
        bad[where] = np.diag([2, 1, 1]).ravel()
        assert cube.symmetrize_status(bad, tau_h[:n], 1, x, out) == EINVAL, n
    assert bool((out == 7.25).all())
    assert cube.symmetrize_status(S_h, tau_h, 1, x, out) == 0 and bool(torch.isfinite(out).all())


def test_symmetrize_rho_of_a_supercell_basis_with_384_operations():
    """The Python level: the 2 x 2 x 2 Si supercell with ``symmetries=True`` and an explicit cube keeps all 384 operations, and
    ``symmetrize_rho`` applies them (tau as the package hands it to the library)."""
    fft_size = (20, 20, 20)
    lattice, atoms, positions = dftk.silicon_cell(supercell=(2, 2, 2))
    model = dftk.model_DFT(lattice, atoms, positions, functionals=("lda_x", "lda_c_pw"), symmetries=True)
    basis = dftk.PlaneWaveBasis(model, 5, dftk.MonkhorstPack((1, 1, 1)), fft_size=fft_size)
    assert len(basis.symmetries) == 384 and basis.fft_size == fft_size
    group = R.group_from_ops("basis", lattice, basis.symmetries)
    handed = np.stack([s.tau for s in basis.symmetries])
    assert maxabs(handed - group.tau) <= 2 * EPS
    group.tau = handed
    rho = random_cube(fft_size)
    for lowpass in (False, True):
        got = dftk.symmetrize_rho(basis, torch.from_numpy(rho.copy()).cuda(), do_lowpass=lowpass).cpu().numpy()
        ref = R.symmetrize_fourier(rho, group, fft_size, int(lowpass)).real
        restated = R.symmetrize_fourier(rho, group, fft_size, int(lowpass), precision="double").real
        check_small(f"symmetrize_rho, 384 operations, lowpass={lowpass}", got, ref, restated)


# ======================================================================================= dftk_mi_cube_gradient
@pytest.mark.parametrize("fft_size", R.SMALL_CUBES, ids=lambda c: "x".join(map(str, c)))
def test_gradient_of_a_trigonometric_polynomial_small(cubes, fft_size):
    """sum a_j cos(2 pi G_j.r + phi_j), G_j strictly inside the grid and the eight corners among them, sheared lattice: the
    analytic cartesian gradient in ``np.longdouble``"""
    G, amp, phi = R.random_modes(np.random.default_rng(21), fft_size, 40, corners=True)
    f, grad = R.trig_polynomial(R.SHEARED, fft_size, G, amp, phi)
    f = f.astype(np.float64)
    restated = R.gradient(f, R.SHEARED, fft_size, precision="double")
    check_small(f"gradient {fft_size}", cubes(fft_size).gradient(f), grad, restated)


@pytest.mark.parametrize("fft_size", R.LARGE_CUBES, ids=lambda c: "x".join(map(str, c)))
def test_gradient_of_a_trigonometric_polynomial_second_trip(cubes, fft_size):
    G, amp, phi = R.random_modes(np.random.default_rng(22), fft_size, 300, corners=True)
    f, grad = R.trig_polynomial(R.SHEARED, fft_size, G, amp, phi, precision="double")
    check_large(f"gradient {fft_size}", cubes(fft_size).gradient(f), grad)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gradient_of_a_pure_nyquist_component_is_exactly_zero(cubes, axis):
    """The Nyquist entry of an even axis carries G = -n/2; i G c (-1)^i is imaginary and the real part is taken at the end: no
    gradient (the convention of the reference, pinned on ``cube_ref.gradient`` first).  EXACTLY zero where the transform of
    +-a is exact: on the power-of-two cube (8, 16, 4) every butterfly of the radix 2 / 4 / 8 passes adds or subtracts equal
    numbers and every twiddle factor meets an exact zero, so the only nonzero coefficient is N a at the Nyquist entry, which
    i G turns imaginary.  (A radix-5 butterfly of equal numbers forms a + c1 2a + c2 2a with rounded cos(2 pi / 5),
    cos(4 pi / 5), which is no exact zero: cubes with such axes are in the next test.)"""
    fft_size = (8, 16, 4)
    f = R.nyquist_wave(fft_size, axis, 0.75)
    assert maxabs(R.gradient(f, R.SHEARED, fft_size)) <= 64 * float(np.finfo(R.LD).eps)
    assert maxabs(R.gradient(f, R.SHEARED, fft_size, precision="double")) <= 64 * EPS
    got = cubes(fft_size).gradient(f)
    print(f"\nnyquist {fft_size} axis {axis}: max|grad| = {maxabs(got):.3g}")
    assert not got.any()


@pytest.mark.parametrize("fft_size,axis", [((12, 12, 20), 0), ((12, 12, 20), 1), ((12, 12, 20), 2), ((10, 15, 16), 0),
                                           ((10, 15, 16), 2), ((96, 90, 64), 1)])
def test_gradient_ignores_a_nyquist_component_to_rounding(cubes, fft_size, axis):
    """On axes with factors 3 and 5 the transform of +-a leaks rounding noise into other entries of the Nyquist plane.  Alone, the
    component gives at most 32 eps a max|B G|: the module's floor for a transform pair, through a multiplier of at most that
    modulus.  Beside a trigonometric polynomial it leaves the polynomial's gradient."""
    amp = 0.75
    wave = R.nyquist_wave(fft_size, axis, amp)
    gmax = float(np.sqrt(R.g_squared(R.SHEARED, fft_size).max()))
    assert maxabs(R.gradient(wave, R.SHEARED, fft_size, precision="double")) <= 32 * EPS * amp * gmax
    got = cubes(fft_size).gradient(wave)
    print(f"\nnyquist {fft_size} axis {axis}: max|grad| / (32 eps a max|G|) = {maxabs(got) / (32 * EPS * amp * gmax):.3g}")
    assert maxabs(got) <= 32 * EPS * amp * gmax
    large = np.prod(fft_size) > R.TRIP
    G, a, phi = R.random_modes(np.random.default_rng(25), fft_size, 20)
    f, grad = R.trig_polynomial(R.SHEARED, fft_size, G, a, phi, precision="double" if large else "long")
    f = f.astype(np.float64) + wave
    if large:
        check_large(f"gradient beside nyquist {fft_size} axis {axis}", cubes(fft_size).gradient(f), grad)
    else:
        check_small(f"gradient beside nyquist {fft_size} axis {axis}", cubes(fft_size).gradient(f), grad,
                    R.gradient(f, R.SHEARED, fft_size, precision="double"))


@pytest.mark.parametrize("fft_size", [(10, 15, 16), (96, 90, 64)], ids=lambda c: "x".join(map(str, c)))
def test_gradient_is_linear_to_rounding(cubes, fft_size):
    """the header's promise: grad(a + b) and grad a + grad b differ by rounding only (a smooth, b rough, as rho and rho_core)"""
    G, amp, phi = R.random_modes(np.random.default_rng(23), fft_size, 12)
    a = R.trig_polynomial(R.SHEARED, fft_size, G, amp, phi, precision="double")[0] + 2.0
    b = random_cube(fft_size, seed=24)
    cube = cubes(fft_size)
    ga, gb, gab = cube.gradient(a), cube.gradient(b), cube.gradient(a + b)
    defect, bound = maxabs(gab - (ga + gb)), 32 * EPS * (maxabs(ga) + maxabs(gb) + maxabs(gab))
    print(f"\ngradient linearity {fft_size}: defect / bound = {defect / bound:.3f}")
    assert defect <= bound


# ======================================================================================= the Fourier multipliers
def multiplier_cases(fft_size, dtype):
    """entry -> (multiplier cube, arguments after the k-block, keeps the mean)"""
    G2 = R.g_squared(R.SHEARED, fft_size, dtype)
    BH = np.asfortranarray(R.recip(R.SHEARED))
    stored = np.random.default_rng(31).uniform(0.5, 2.0, tuple(fft_size)[::-1])
    return {"dftk_mi_mix_kerker": (R.kerker_multiplier(G2, fft_size, KTF), (BH.ctypes.data, KTF), True, BH),
            "dftk_mi_mix_dielectric": (R.dielectric_multiplier(G2, KTF, EPS_R), (BH.ctypes.data, KTF, EPS_R), True, BH),
            "dftk_mi_chi0_dielectric_apply": (R.chi0_multiplier(G2, KTF, EPS_R), (BH.ctypes.data, KTF, EPS_R), False, BH),
            "dftk_mi_cube_fourier_filter": (stored.astype(dtype), (dev(stored),), False, BH)}


ENTRIES = ["dftk_mi_mix_kerker", "dftk_mi_mix_dielectric", "dftk_mi_chi0_dielectric_apply", "dftk_mi_cube_fourier_filter"]


def run_filter(cube, entry, args, x):
    args = tuple(a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args)
    return cube.filter(entry, x, *args)


def check_filter_properties(entry, fft_size, got, x, keeps_mean):
    if keeps_mean:          # Kerker: the DC coefficient of dF is copied; dielectric: it is kept
        assert abs(got.mean() - x.mean()) <= 16 * EPS * maxabs(x), entry
    if entry == "dftk_mi_mix_kerker":          # enforce_real!: the unpaired Nyquist entries are zeroed
        ny = R.unpaired_nyquist(fft_size)
        c = np.fft.fftn(got)
        assert ny.any() == any(n % 2 == 0 for n in fft_size), entry
        assert not ny.any() or maxabs(c[ny]) <= 64 * EPS * maxabs(c), entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_filters_small_sheared_cube(cubes, entry):
    fft_size = (10, 15, 16)
    x = random_cube(fft_size)
    mult_long, args, keeps_mean, _keep = multiplier_cases(fft_size, R.LD)[entry]
    mult = multiplier_cases(fft_size, np.float64)[entry][0]
    got = run_filter(cubes(fft_size), entry, args, x)
    check_small(f"{entry} {fft_size}", got, R.apply_multiplier(x, mult_long), R.apply_multiplier(x, mult, precision="double"))
    check_filter_properties(entry, fft_size, got, x, keeps_mean)


@pytest.mark.parametrize("fft_size", R.LARGE_CUBES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("entry", ENTRIES)
def test_filters_second_trip(cubes, entry, fft_size):
    x = random_cube(fft_size)
    mult, args, keeps_mean, _keep = multiplier_cases(fft_size, np.float64)[entry]
    got = run_filter(cubes(fft_size), entry, args, x)
    check_large(f"{entry} {fft_size}", got, R.apply_multiplier(x, mult, precision="double"))
    check_filter_properties(entry, fft_size, got, x, keeps_mean)
