"""The FFT kernels of ``dftk.jl_amd/csrc/fft_kernels.hip`` at every axis length and every z factorisation, at the C ABI.

Reference: a dense DFT in ``numpy.longdouble``, one axis after the other with ``einsum``; the matrices are
exp(+-2 pi i ((j k) mod n) / n) with the integer phase reduced before the division, so no FFT algorithm takes part and
the reference is good to ~1e-19.  Conventions (those of ``test_sphere_fft_roundtrip_and_oracle`` and
``test_apply_H_vs_oracle``): ``ifft_sphere`` = unnormalised exp(+i) of the zero-padded sphere, ``fft_sphere`` =
unnormalised exp(-i) restricted to the sphere, local part = FFT[V IFFT[pad c]] / N on the sphere, density
rho += sum_n w_n |IFFT[pad c_n]|^2; mapping index ix + nx (iy + ny iz), cubes (nz, ny, nx) in C order.

The spheres are synthetic (``synthetic_sphere``): ``dftk_mi_kblock_create`` accepts any strictly ascending mapping, so
every z window -- one plane, no negative planes, no non-negative planes, the whole cube, a window with a hole -- is
reached on cubes like 11 x 3 x nz.

Tolerance: err = |got - ref|_2 / |ref|_2 in long double.  The same data goes through ``numpy.fft`` in fp64, whose error
against the same reference is e_np (2e-16 ... 3.2e-16 for one transform, up to 6e-16 for the local part, which is
two); a case passes if err <= 64 max(e_np, 2.2e-16), 1.4e-14 ... 4e-14.  The factor is a margin over the reference's fp64 twin, not over the code
under test: the hand-written passes use twiddle recurrences (up to 5 steps of w = w w1) and O(p^2) generic prime
butterflies up to p = 61, which may lose a few bits more than pocketfft.  The worst err / e_np observed per family is
recorded in DESIGN.md ("FFT kernels at every axis length").

Memory discipline: every output that a call must fully write is NaN-filled first, every output buffer is a view into
a larger allocation with 1 KiB of sentinel values on both sides, asserted unchanged afterwards (the padding lanes
x >= nx of the z kernels are where a stray store would land)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402

from test_gpu_kernels import Basis, KBlock, dev  # noqa: E402
from test_host_side import largest_prime_factor  # noqa: E402

# the register-resident z kernels are the default from nz = 24 on; with either switch set this file would silently
# test the LDS-pass kernels instead
assert "DFTK_MI_FFT_REG" not in os.environ and "DFTK_MI_FFT_REG_MIN" not in os.environ, \
    "unset DFTK_MI_FFT_REG / DFTK_MI_FFT_REG_MIN: these tests are about the default choice of the z kernels"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD, CLD = np.longdouble, np.clongdouble
assert np.finfo(LD).eps < 1.1e-19, "the reference needs a long double with a 64-bit mantissa"
PI = LD(4) * np.arctan(LD(1))
EPS = 2.2e-16
# err <= FACTOR[family] * max(e_np, EPS); the measured ratios are in DESIGN.md
FACTOR = {"sweep x": 64, "sweep y": 64, "sweep z": 64, "stage C reg": 64, "density reg": 64, "multi": 64}

# the factorisations of REG_SIZES (fft_kernels.hip)
REG_LENGTHS = [24, 27, 30, 32, 36, 40, 45, 48, 50, 54, 60, 64, 72, 80, 90, 96, 100, 108, 120, 128, 144, 150, 160, 180,
               192, 200, 216, 240, 256]


# every length of 1 .. 128 that the planner accepts (prime factors up to 61), and the large ones of the issue
SWEEP_LENGTHS = [n for n in range(1, 129) if largest_prime_factor(n) <= 61] + [144, 150, 160, 169, 180, 192, 200, 216,
                                                                                  240, 243, 245, 250, 256]
N_BLOCKS = 8      # 128 lengths in 8 interleaved blocks of 16: every block has short and long axes


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


# ----------------------------------------------------------------------------------- reference
@functools.lru_cache(maxsize=None)
def dft_matrix(n, sign):
    """W[j, k] = exp(sign 2 pi i ((j k) mod n) / n) in long double (shared by all tests, read-only)"""
    jk = np.outer(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)) % n
    ang = (2 * PI) * jk.astype(LD) / LD(n)
    W = np.empty((n, n), dtype=CLD)
    W.real = np.cos(ang)
    W.imag = sign * np.sin(ang)
    W.setflags(write=False)
    return W


class Sphere:
    """A mapping on an (nx, ny, nz) cube with its long-double reference transforms and their numpy.fft twins in fp64;
    all take and return batches: coefficients (nb, n_G), cubes (nb, nz, ny, nx)."""

    def __init__(self, dims, mapping):
        self.dims = nx, ny, nz = dims
        self.mapping = m = np.asarray(mapping, dtype=np.int64)
        assert np.all(np.diff(m) > 0) and m[0] >= 0 and m[-1] < nx * ny * nz
        self.ix, self.iy, self.iz = m % nx, (m // nx) % ny, m // (nx * ny)
        self.zs = np.unique(self.iz)                     # the sphere's planes: the others are zero / not wanted
        self.zi = np.searchsorted(self.zs, self.iz)
        self.n_G, self.N = len(m), nx * ny * nz

    def window(self):
        """(nzx, z_lo) by the rule of dftk_mi_kblock_create: z_lo = -1 if the planes do not wrap around contiguously"""
        nz, zv = self.dims[2], self.zs
        lo = 0
        while lo < len(zv) and zv[lo] == lo:
            lo += 1
        ok = all(zv[i] == nz - (len(zv) - i) for i in range(lo, len(zv)))
        return len(zv), (lo if ok else -1)

    def ifft(self, c):
        nx, ny, nz = self.dims
        sub = np.zeros((len(c), len(self.zs), ny, nx), dtype=CLD)
        sub[:, self.zi, self.iy, self.ix] = c
        sub = np.einsum("ax,bzyx->bzya", dft_matrix(nx, +1), sub)
        sub = np.einsum("ay,bzyx->bzax", dft_matrix(ny, +1), sub)
        return np.einsum("az,bzyx->bayx", dft_matrix(nz, +1)[:, self.zs], sub)

    def fft(self, cube):
        nx, ny, nz = self.dims
        sub = np.einsum("za,bayx->bzyx", dft_matrix(nz, -1)[self.zs, :], np.asarray(cube).astype(CLD))
        sub = np.einsum("ya,bzax->bzyx", dft_matrix(ny, -1), sub)
        sub = np.einsum("xa,bzya->bzyx", dft_matrix(nx, -1), sub)
        return sub[:, self.zi, self.iy, self.ix]

    def local(self, V, c):
        return self.fft(V.astype(LD)[None] * self.ifft(c)) / LD(self.N)

    def ifft64(self, c):
        nx, ny, nz = self.dims
        pad = np.zeros((len(c), nz, ny, nx), dtype=complex)
        pad[:, self.iz, self.iy, self.ix] = c
        return np.fft.ifftn(pad, axes=(1, 2, 3), norm="forward")

    def fft64(self, cube):
        return np.fft.fftn(cube, axes=(1, 2, 3))[:, self.iz, self.iy, self.ix]

    def local64(self, V, c):
        return self.fft64(V[None] * self.ifft64(c)) / self.N


def synthetic_sphere(nx, ny, nz, z_lo, n_hi, rng, full=False, hole=False, inversion=False):
    """Ascending mapping whose z planes are 0 .. z_lo-1 and nz-n_hi .. nz-1; every plane gets a random non-empty set of y
    rows, every row a random non-empty set of x (about half filled).  full: the whole cube, whatever else is asked.
    hole: one interior plane of the window is removed, so that the planes no longer wrap around contiguously (z_lo = -1
    in the library).  inversion: frequencies strictly below Nyquist on every axis, closed under G -> -G; the whole cube
    is closed under G -> -G as it is and keeps its Nyquist planes, whose self-conjugate entries ``real_symmetric``
    makes real like c(0)."""
    if full:
        return np.arange(nx * ny * nz, dtype=np.int64)
    assert z_lo >= 0 and n_hi >= 0 and 1 <= z_lo + n_hi <= nz
    planes = list(range(z_lo)) + list(range(nz - n_hi, nz))
    if hole:
        assert z_lo >= 3 and not inversion
        planes.remove(1)

    def below_nyquist(n):
        return np.array([i for i in range(n) if 2 * min(i, n - i) < n])

    def some(pool, p):
        pick = pool[rng.random(len(pool)) < p]
        return pick if len(pick) else pool[[rng.integers(len(pool))]]

    xs, ys = (below_nyquist(nx), below_nyquist(ny)) if inversion else (np.arange(nx), np.arange(ny))
    pts = set()
    for z in planes:
        for y in some(ys, 0.6):
            pts.update((int(x), int(y), z) for x in some(xs, 0.5))
    if inversion:
        assert n_hi == z_lo - 1 and all(2 * min(z, nz - z) < nz for z in planes)
        pts |= {((-x) % nx, (-y) % ny, (-z) % nz) for x, y, z in pts}
    return np.array(sorted(x + nx * (y + ny * z) for x, y, z in pts), dtype=np.int64)


def relerr(got, ref):
    d = np.asarray(got).astype(ref.dtype) - ref
    return float(np.sqrt((np.abs(d) ** 2).sum()) / np.sqrt((np.abs(ref) ** 2).sum()))


class Tally:
    """The comparisons of one test: every failing (label) is named, the worst err / e_np is printed."""

    def __init__(self, family):
        self.family, self.bad, self.worst = family, [], (0.0, "")

    def add(self, label, got, got64, ref):
        err, e_np = relerr(got, ref), relerr(got64, ref)
        bound = FACTOR[self.family] * max(e_np, EPS)
        ratio = err / max(e_np, 1e-300)
        if not ratio <= self.worst[0]:
            self.worst = (ratio, f"{label}: err {err:.3e}, e_np {e_np:.3e}")
        if not err <= bound:
            self.bad.append(f"{label}: err {err:.3e} > {bound:.3e} = {FACTOR[self.family]} max(e_np = {e_np:.3e}, {EPS})")

    def finish(self):
        print(f"[{self.family}] worst err / e_np = {self.worst[0]:.2f} ({self.worst[1]})")
        assert not self.bad, "\n".join(self.bad)


# ----------------------------------------------------------------------------------- device side
SENTINEL = -6.02214076e23


class Guarded:
    """An output buffer as a view into a larger allocation with 1 KiB of sentinel values on both sides"""

    def __init__(self, shape, dtype, fill=float("nan")):
        n = int(np.prod(shape))
        self.pad = 1024 // torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((n + 2 * self.pad,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.raw[self.pad:self.pad + n].view(*shape)
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill)))
        else:
            self.t.fill_(complex(fill, fill) if dtype.is_complex else fill)
        torch.cuda.synchronize()      # the library works on its own stream

    def ptr(self):
        return self.t.data_ptr()

    def numpy(self, label):
        raw = self.raw.cpu().numpy()
        assert np.all(raw[:self.pad] == SENTINEL) and np.all(raw[-self.pad:] == SENTINEL), \
            f"{label}: store outside the output buffer"
        return self.t.cpu().numpy()


def run_ifft(lib, bs, kb, c, dims, label):
    nx, ny, nz = dims
    cd_ = dev(c)
    cube = Guarded((nz, ny, nx), torch.complex128)
    check(lib.dftk_mi_ifft_sphere(kb.h, cd_.data_ptr(), cube.ptr()))
    bs.sync()
    return cube.numpy(label)[None]


def run_fft(lib, bs, kb, f, label):
    fd = dev(f)
    out = Guarded((kb.n_G,), torch.complex128)
    check(lib.dftk_mi_fft_sphere(kb.h, fd.data_ptr(), out.ptr()))
    bs.sync()
    return out.numpy(label)[None]


def run_local(lib, bs, kb, V, c, label):
    """dftk_mi_apply_H_parts(which = 1) of the bands c (nb, n_G)"""
    kb.set_potential(V)
    cd_ = dev(c)
    out = Guarded(c.shape, torch.complex128)
    check(lib.dftk_mi_apply_H_parts(kb.h, 1, len(c), cd_.data_ptr(), kb.n_G, out.ptr(), kb.n_G))
    bs.sync()
    return out.numpy(label)


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def plan_status(lib, n):
    nr, rad, pos = C.c_int(), (C.c_int * 32)(), (C.c_int * n)()
    return lib.dftk_mi_fft_plan_host(n, C.byref(nr), rad, pos)


def plan_radices(lib, n):
    nr, rad, pos = C.c_int(), (C.c_int * 32)(), (C.c_int * n)()
    check(lib.dftk_mi_fft_plan_host(n, C.byref(nr), rad, pos))
    return set(rad[:nr.value])


# ----------------------------------------------------------------------------------- A. axis sweep, LDS-pass kernels
def sweep_dims(axis, n):
    # the other two axes small and awkward; nx = 11 pads to nxp = 16
    return {"x": (n, 3, 5), "y": (11, n, 3), "z": (11, 3, n)}[axis]


@pytest.mark.parametrize("block", range(N_BLOCKS))
@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_axis_sweep(lib, axis, block):
    """Stages A, B, z cube modes, D, E (``ifft_sphere`` / ``fft_sphere``) at every plannable axis length, each axis in turn;
    on the z sweep also the local part with 3 bands: ``k_zpass<0>`` for every length without a register instantiation
    (generic primes take the un-fused potential multiply).  Every 8th length additionally with the full-cube mapping."""
    tally = Tally(f"sweep {axis}")
    for n in SWEEP_LENGTHS[block::N_BLOCKS]:
        assert plan_status(lib, n) == 0, f"length {n} not planned"
        dims = nx, ny, nz = sweep_dims(axis, n)
        rng = np.random.default_rng(1000 * "xyz".index(axis) + n)
        bs = Basis(lib, nx, ny, nz)
        cases = [("window", dict())]
        i = SWEEP_LENGTHS.index(n)
        if (i + i // 8) % 8 == 0:        # one length of every 8 consecutive ones, a different block each time
            cases.append(("full", dict(full=True)))
        for name, kw in cases:
            sp = Sphere(dims, synthetic_sphere(nx, ny, nz, nz // 4 + 1, nz // 4, rng, **kw))
            kb = KBlock(lib, bs, sp.mapping, np.zeros(sp.n_G))
            label = f"axis {axis}, n = {n}, {name}"
            c = crandn(rng, 1, sp.n_G)
            tally.add(f"{label}, ifft_sphere", run_ifft(lib, bs, kb, c[0], dims, label), sp.ifft64(c), sp.ifft(c))
            f = crandn(rng, 1, nz, ny, nx)
            tally.add(f"{label}, fft_sphere", run_fft(lib, bs, kb, f[0], label), sp.fft64(f), sp.fft(f))
            if axis == "z":
                V, c3 = rng.standard_normal((nz, ny, nx)), crandn(rng, 3, sp.n_G)
                tally.add(f"{label}, local part", run_local(lib, bs, kb, V, c3, label), sp.local64(V, c3), sp.local(V, c3))
    tally.finish()


def test_unplannable_axis_is_rejected(lib):
    """A prime factor above 61 on any axis: negative status, the "cannot plan" message, and the half-built basis is
    released (the later axes fail after the tables of the earlier ones went to the device)."""
    for n in range(1, 129):
        assert (plan_status(lib, n) == 0) == (n in SWEEP_LENGTHS), n
    for dims in [(67, 8, 8), (8, 67, 8), (8, 8, 67), (8, 8, 2 * 71)]:
        h = C.c_void_p()
        st = lib.dftk_mi_basis_create(*dims, 1.0, 0, C.byref(h))
        assert st < 0 and b"cannot plan" in lib.dftk_mi_last_error(), (dims, st, lib.dftk_mi_last_error())
        assert not h.value
    bs = Basis(lib, 8, 8, 8)      # the library goes on working
    sp = Sphere((8, 8, 8), synthetic_sphere(8, 8, 8, 3, 2, np.random.default_rng(0)))
    kb = KBlock(lib, bs, sp.mapping, np.zeros(sp.n_G))
    c = crandn(np.random.default_rng(1), 1, sp.n_G)
    assert relerr(run_ifft(lib, bs, kb, c[0], (8, 8, 8), "8^3"), sp.ifft(c)) < 64 * EPS


# ----------------------------------------------------------------------------------- B. every factorisation, stage C
def test_reg_sizes_are_the_tested_list():
    """A factorisation added to REG_SIZES without a test fails here."""
    src = open(os.path.join(ROOT, "dftk.jl_amd", "csrc", "fft_kernels.hip")).read()
    body = re.search(r"#define REG_SIZES\(X\)((?:.*\\\n)*.*\n)", src).group(1)
    entries = [tuple(map(int, e)) for e in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)\)", body)]
    assert len(entries) == len(set(e[0] for e in entries)) == body.count("X(")
    assert sorted(e[0] for e in entries) == REG_LENGTHS
    assert all(n == a * b * c * d for n, a, b, c, d in entries)


def reg_windows(N):
    return [("window (N/4+1, N/4)", N // 4 + 1, N // 4, dict()),
            ("window (3, N/2-2)", 3, N // 2 - 2, dict()),
            ("window (1, 0)", 1, 0, dict()),
            ("window (0, 1)", 0, 1, dict()),
            ("full cube", N, 0, dict(full=True)),
            ("window (N/4+1, N/4) with a hole", N // 4 + 1, N // 4, dict(hole=True))]


@pytest.mark.parametrize("N", REG_LENGTHS)
def test_stage_c_every_factorisation(lib, N):
    """``k_zpass_reg`` of every factorisation through ``dftk_mi_apply_H_parts(which = 1)``: cube (11, 3, N) = 6 column
    groups on a grid of 8 (the early exit of the XCD swizzle runs), 3 bands; at 45, 96 and 216 also (17, 4, N) with 5 bands
    = 12 groups, two slots per XCD.  Windows: both kinds of partial window, one plane on either side, the whole cube,
    and a window with a hole, which takes the LDS-pass fall-back on the same axis."""
    tally = Tally("stage C reg")
    for (nx, ny), nb in [((11, 3), 3)] + ([((17, 4), 5)] if N in (45, 96, 216) else []):
        dims = (nx, ny, N)
        rng = np.random.default_rng(N + nx)
        bs = Basis(lib, nx, ny, N)
        V = rng.standard_normal((N, ny, nx))
        for name, z_lo, n_hi, kw in reg_windows(N):
            sp = Sphere(dims, synthetic_sphere(nx, ny, N, z_lo, n_hi, rng, **kw))
            assert sp.window() == (z_lo + n_hi - bool(kw.get("hole")), -1 if kw.get("hole") else z_lo), (name, sp.window())
            kb = KBlock(lib, bs, sp.mapping, np.zeros(sp.n_G))
            c = crandn(rng, nb, sp.n_G)
            label = f"N = {N}, cube ({nx}, {ny}, {N}), {name}"
            tally.add(label, run_local(lib, bs, kb, V, c, label), sp.local64(V, c), sp.local(V, c))
    tally.finish()


# ----------------------------------------------------------------------------------- C. every factorisation, density
def real_symmetric(sp, c):
    """c(-G) = conj c(G) exactly (c(0) and every other self-conjugate entry real)"""
    nx, ny, nz = sp.dims
    lin = (-sp.ix) % nx + nx * ((-sp.iy) % ny + ny * ((-sp.iz) % nz))
    neg = np.searchsorted(sp.mapping, lin)
    assert np.array_equal(sp.mapping[neg], lin), "the sphere is not closed under G -> -G"
    return (c + c[:, neg].conj()) / 2


def density_case(lib, tally, label, sp, entry, c, w, rng, fft_batch=None):
    nx, ny, nz = sp.dims
    bs = Basis(lib, nx, ny, nz)
    if fft_batch:
        check(lib.dftk_mi_basis_set_fft_batch(bs.h, fft_batch))
    kb = KBlock(lib, bs, sp.mapping, np.zeros(sp.n_G))
    acc = np.einsum("b,bzyx->zyx", w.astype(LD), np.abs(sp.ifft(c)) ** 2)
    acc64 = np.einsum("b,bzyx->zyx", w, np.abs(sp.ifft64(c)) ** 2)
    rho0 = rng.uniform(0.5, 1.5, (nz, ny, nx)) * float(acc.mean())          # the call is +=
    cd_ = dev(c)
    rho = Guarded((nz, ny, nx), torch.float64, fill=rho0)
    check(getattr(lib, entry)(kb.h, len(c), cd_.data_ptr(), sp.n_G, w.ctypes.data, rho.ptr()))
    bs.sync()
    tally.add(label, rho.numpy(label), rho0 + acc64, rho0.astype(LD) + acc)


@pytest.mark.parametrize("N", REG_LENGTHS)
def test_density_every_factorisation(lib, N):
    """``k_zdensity_reg`` of every factorisation on cube (11, 3, N), window (N/4+1, N/4) and the whole cube.
    ``dftk_mi_density_accumulate``: launch groups of 2 bands, 5 bands with weights [1.3, 0.5, 0, 0, 0.7] -- the second
    group is all zero and skipped, the third has one band.  ``dftk_mi_density_accumulate_real``: an inversion-symmetric
    sphere, 5 real-symmetric columns with weights [2, 0.3, 0, 1.1, 0.6] -- pairs share a transform (w Re^2 + wim Im^2),
    the odd count leaves the last imaginary slot weightless.  rho is pre-filled: the calls add."""
    tally = Tally("density reg")
    nx, ny = 11, 3
    rng = np.random.default_rng(7 * N)
    for name, kw in [("window (N/4+1, N/4)", dict()), ("full cube", dict(full=True))]:
        sp = Sphere((nx, ny, N), synthetic_sphere(nx, ny, N, N // 4 + 1, N // 4, rng, **kw))
        density_case(lib, tally, f"N = {N}, {name}, density_accumulate", sp, "dftk_mi_density_accumulate",
                     crandn(rng, 5, sp.n_G), np.array([1.3, 0.5, 0.0, 0.0, 0.7]), rng, fft_batch=2)
        sp = Sphere((nx, ny, N), synthetic_sphere(nx, ny, N, N // 4 + 1, N // 4, rng, inversion=True, **kw))
        assert sp.window()[1] >= 0
        density_case(lib, tally, f"N = {N}, {name}, density_accumulate_real", sp, "dftk_mi_density_accumulate_real",
                     real_symmetric(sp, crandn(rng, 5, sp.n_G)), np.array([2.0, 0.3, 0.0, 1.1, 0.6]), rng)
    tally.finish()


# ----------------------------------------------------------------------------------- D. job-table paths
@pytest.mark.parametrize("nz", [45, 64, 216, 20, 21])
def test_density_multi_job_table(lib, nz):
    """``dftk_mi_density_accumulate_multi2`` / ``_multi`` over two k-blocks with different windows on one (12, 3, nz)
    basis (nx = 12 pads to nxp = 16).  The executor builds a job table only if no axis has a generic radix (7 or a prime
    above), so x and y must be 2-3-5-smooth here -- asserted from the plan.  45, 64, 216: register kernels under a job
    table (odd R2 without pitch padding, the square factorisation, R1 != R2 with a radix 6); 20: the lean LDS kernel
    under a job table; 21 = 3 x 7: the one deliberate generic axis, for which the executor returns to one-by-one calls.
    9 + 11 bands = 18 jobs (two bands have no weight at all) on 6 < 1024 columns: two partial cubes and
    ``k_dens_reduce``; 3 + 4 bands = 6 jobs: one group, straight into rho.  Second weights go to a second cube; some
    weights are exactly 0 in one set only."""
    tally = Tally("multi")
    nx, ny = 12, 3
    lean = {2, 3, 4, 5, 6, 8}
    assert plan_radices(lib, nx) <= lean and plan_radices(lib, ny) <= lean, "a generic x or y axis: no job table is built"
    assert (plan_radices(lib, nz) <= lean) == (nz != 21), "only nz = 21 is meant to take the one-by-one fall-back"
    rng = np.random.default_rng(nz)
    bs = Basis(lib, nx, ny, nz)
    spheres = [Sphere((nx, ny, nz), synthetic_sphere(nx, ny, nz, z_lo, n_hi, rng))
               for z_lo, n_hi in [(nz // 4 + 1, nz // 4), (3, nz // 2 - 2)]]
    assert spheres[0].window() != spheres[1].window() and all(sp.window()[1] >= 0 for sp in spheres)
    kbs = [KBlock(lib, bs, sp.mapping, np.zeros(sp.n_G)) for sp in spheres]
    M = [9, 11]
    cs = [crandn(rng, m, sp.n_G) for m, sp in zip(M, spheres)]
    psi = [dev(c) for c in cs]
    dens = [np.abs(sp.ifft(c)) ** 2 for sp, c in zip(spheres, cs)]          # shared by both calls
    dens64 = [np.abs(sp.ifft64(c)) ** 2 for sp, c in zip(spheres, cs)]
    scale = float(np.mean([d.mean() for d in dens]))

    def call(name, nb, wa, wb, single):
        assert len(wa) == len(wb) == sum(nb)
        ref = [sum(np.einsum("b,bzyx->zyx", w[o:o + m].astype(LD), d[:m]) for o, m, d in zip((0, nb[0]), nb, dens))
               for w in (wa, wb)]
        ref64 = [sum(np.einsum("b,bzyx->zyx", w[o:o + m], d[:m]) for o, m, d in zip((0, nb[0]), nb, dens64))
                 for w in (wa, wb)]
        rho0 = [rng.uniform(0.5, 1.5, (nz, ny, nx)) * scale for _ in range(3)]
        rho = [Guarded((nz, ny, nx), torch.float64, fill=r) for r in rho0]
        args = (2, (C.c_void_p * 2)(*[k.h.value for k in kbs]), (C.c_int * 2)(*nb),
                (C.c_void_p * 2)(*[p.data_ptr() for p in psi]), (C.c_int64 * 2)(*[sp.n_G for sp in spheres]))
        check(lib.dftk_mi_density_accumulate_multi2(*args, wa.ctypes.data, rho[0].ptr(), wb.ctypes.data, rho[1].ptr()))
        bs.sync()
        if single:
            check(lib.dftk_mi_density_accumulate_multi(*args, wa.ctypes.data, rho[2].ptr()))
            bs.sync()
        for i, r in ((0, 0), (1, 1)) + (((2, 0),) if single else ()):
            label = f"nz = {nz}, {name}, cube {i}"
            tally.add(label, rho[i].numpy(label), rho0[i] + ref64[r], rho0[i].astype(LD) + ref[r])

    wa, wb = rng.uniform(0.1, 2.0, 20), rng.uniform(0.1, 2.0, 20)
    wa[[1, 5, 9 + 7]] = 0.0
    wb[[3, 5, 9 + 7]] = 0.0
    assert np.count_nonzero((wa != 0) | (wb != 0)) == 18
    call("9 + 11 bands", M, wa, wb, single=False)
    wa, wb = rng.uniform(0.1, 2.0, 7), rng.uniform(0.1, 2.0, 7)
    wa[[1, 5]] = 0.0
    wb[[0, 4, 5]] = 0.0
    call("3 + 4 bands", [3, 4], wa, wb, single=True)
    tally.finish()
