"""References for the density-sized passes of ``csrc/cube_kernels.hip`` (symmetrisation, gradient, Fourier multipliers), written
from the reference project's formulas (symmetry.jl:282-357, mixing.jl:61-72,161-171, chi0models.jl:66-77, xc.jl:356-409) in
NumPy.  Nothing here calls the library, the package's torch twin or ``oracle/``.

Cubes are (nz, ny, nx) arrays, ``fft_size = (nx, ny, nz)``, linear index ix + nx (iy + ny iz); the integer G of an entry is
its FFT-order frequency [0 .. (n-1)/2, -ceil((n-1)/2) .. -1] per axis.

* ``dftn``: the separable DFT with per-axis matrices exp(-+2 pi i (jk mod n) / n) in ``np.clongdouble`` (jk mod n reduced in
  integers, so the angle is exact to one rounding) -- O(N n), for the small cubes -- or ``np.fft`` (``precision="double"``).
* ``symmetrize_fourier``: out(G) = keep(G) / n_sym sum_s [S_s^-1 G on the grid] e^{-2 pi i G.tau_s} in(S_s^-1 G),
  keep(G) = prod_s [S_s G on the grid] with the low-pass on.  tau is taken as the double it is handed (G.tau is exact in
  ``np.longdouble`` and reduced mod 1 before the angle is formed).
* ``symmetrize_realspace``: (1 / n_sym) sum_s rho(W_s r + w_s) as an integer permutation of the grid per operation, summed in
  ``np.longdouble``: no transform at all.  Only for grids that every operation maps onto themselves (``grid_compatible``).
* ``gradient``, ``apply_multiplier`` and the multiplier cubes of Kerker / dielectric mixing and the dielectric chi0 model.
* The space groups of tests/golden/cube_symmetry_groups.json (integer W, rational w), written by ``generate_groups`` with the
  package's own ``symmetry_operations``; tests/test_cube_reference.py regenerates the quick ones and compares.
"""
import itertools
import json
import os

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
PI_LD = LD(4) * np.arctan(LD(1))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cube_symmetry_groups.json")

TRIP = 2048 * 256          # CUBE_BLOCKS workgroups of 256 threads: the second trip of a grid-stride loop starts here
SMALL_CUBES = [(15, 15, 15), (12, 12, 20), (10, 15, 16)]          # all odd; all even; mixed and anisotropic
LARGE_CUBES = [(81, 81, 81), (96, 90, 64)]                        # N = 531 441 and 552 960, both past TRIP

A_SI = 10.26
SI_PRIMITIVE = A_SI / 2 * np.array([[0, 1, 1.0], [1, 0, 1.0], [1, 1, 0.0]])
SHEARED = np.array([[7.4, 0.9, -0.6], [0.4, 6.9, 1.1], [-0.7, 0.5, 7.8]])          # columns, tests/test_gpu_multispecies.py
HCP = np.array([[6.0, -3.0, 0.0], [0.0, 3.0 * np.sqrt(3.0), 0.0], [0.0, 0.0, 9.8]])  # a = 6.0, c = 9.8


# ------------------------------------------------------------------------------------------------------------ grids
def freq(n):
    i = np.arange(n)
    return np.where(i <= (n - 1) // 2, i, i - n)


def g_cube(fft_size):
    """integer G of every cube entry, shape (nz, ny, nx, 3) with the last axis (Gx, Gy, Gz)"""
    nx, ny, nz = fft_size
    gz, gy, gx = np.meshgrid(freq(nz), freq(ny), freq(nx), indexing="ij")
    return np.stack([gx, gy, gz], axis=-1).astype(np.int64)


def index_of(G, fft_size):
    """(on the grid, linear index) of integer vectors G (..., 3); a vector is on the grid when every component lies in
    [-ceil((n-1)/2), floor((n-1)/2)]"""
    ok = np.ones(G.shape[:-1], dtype=bool)
    idx = []
    for a, n in enumerate(fft_size):
        g = G[..., a]
        ok &= (g >= -((n - 1) - (n - 1) // 2)) & (g <= (n - 1) // 2)
        idx.append(np.mod(g, n))
    return ok, idx[0] + fft_size[0] * (idx[1] + fft_size[1] * idx[2])


def recip(lattice):
    return 2 * np.pi * np.linalg.inv(np.asarray(lattice, dtype=float)).T


def unpaired_nyquist(fft_size):
    """entries whose -G partner is not on the grid: the planes n/2 of the even axes"""
    nx, ny, nz = fft_size
    m = np.zeros((nz, ny, nx), dtype=bool)
    for ax, n in enumerate((nz, ny, nx)):
        if n % 2 == 0:
            sl = [slice(None)] * 3
            sl[ax] = n // 2
            m[tuple(sl)] = True
    return m


# ------------------------------------------------------------------------------------------------------------ DFT
def dft_matrix(n, sign):
    jk = np.outer(np.arange(n), np.arange(n)) % n
    ang = (2 * PI_LD) * jk.astype(LD) / LD(n)
    F = np.empty((n, n), dtype=CLD)
    F.real, F.imag = np.cos(ang), sign * np.sin(ang)
    return F


def dftn(x, sign=-1, precision="long"):
    """unnormalised 3-D DFT, e^{sign 2 pi i jk / n} per axis"""
    if precision == "double":
        return np.fft.fftn(x) if sign < 0 else np.fft.ifftn(x) * x.size
    y = np.asarray(x).astype(CLD)
    for ax in range(3):
        y = np.moveaxis(np.tensordot(dft_matrix(y.shape[ax], sign), y, axes=([1], [ax])), 0, ax)
    return y


# ------------------------------------------------------------------------------------------------------------ groups
class Group:
    """W (n, 3, 3) int, w = w_num / w_den (rational, in [0, 1)), S = W', tau = -W^-1 w (a correctly rounded double)"""

    def __init__(self, name, lattice, W, w_num, w_den):
        self.name, self.lattice = name, np.asarray(lattice, dtype=float)
        self.W = np.asarray(W, dtype=np.int64).reshape(-1, 3, 3)
        self.w_num = np.asarray(w_num, dtype=np.int64).reshape(-1, 3)
        self.w_den = np.asarray(w_den, dtype=np.int64).reshape(-1)
        self.S = np.ascontiguousarray(self.W.transpose(0, 2, 1))
        self.w = self.w_num / self.w_den[:, None]
        Winv = np.stack([int_inverse(W) for W in self.W])
        self.tau = -np.einsum("nij,nj->ni", Winv, self.w_num) / self.w_den[:, None] + 0.0      # (+ 0.0: no -0.0)

    def __len__(self):
        return len(self.W)

    def subset(self, sel, name=None):
        sel = np.asarray(sel)
        return Group(name or self.name, self.lattice, self.W[sel], self.w_num[sel], self.w_den[sel])

    def abi(self):
        """S_h (n, 9) int32, each matrix column-major, and tau_h (n, 3) as ``dftk_mi_symmetrize_rho`` takes them"""
        S_h = np.ascontiguousarray(self.S.transpose(0, 2, 1).reshape(-1, 9), dtype=np.int32)
        return S_h, np.ascontiguousarray(self.tau, dtype=np.float64)

    def n_translated(self):
        return int(np.count_nonzero(np.any(self.tau != 0.0, axis=1)))

    def pure_translations(self):
        return np.flatnonzero(np.all(self.W == np.eye(3, dtype=np.int64), axis=(1, 2)))


def int_inverse(M):
    M = np.asarray(M, dtype=np.int64)
    det = int(round(np.linalg.det(M)))
    assert det in (1, -1)
    adj = np.array([[M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1], M[0, 2] * M[2, 1] - M[0, 1] * M[2, 2], M[0, 1] * M[1, 2] - M[0, 2] * M[1, 1]],
                    [M[1, 2] * M[2, 0] - M[1, 0] * M[2, 2], M[0, 0] * M[2, 2] - M[0, 2] * M[2, 0], M[0, 2] * M[1, 0] - M[0, 0] * M[1, 2]],
                    [M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0], M[0, 1] * M[2, 0] - M[0, 0] * M[2, 1], M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]]])
    inv = adj * det
    assert np.array_equal(inv @ M, np.eye(3, dtype=np.int64))
    return inv


CELLS = {          # name -> (lattice, positions); one species each
    "si_primitive": (SI_PRIMITIVE, [np.ones(3) / 8, -np.ones(3) / 8]),
    "hcp": (HCP, [np.array([1 / 3, 2 / 3, 1 / 4]), np.array([2 / 3, 1 / 3, 3 / 4])]),
    "si_conventional": (A_SI * np.eye(3), [np.array(f) + s * np.ones(3) / 8 for f in
                                            ([0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]) for s in (1, -1)]),
    "si_supercell_222": (2 * SI_PRIMITIVE, [(s * np.ones(3) / 8 + np.array([i, j, k])) / 2 for s in (1, -1)
                                            for k in range(2) for j in range(2) for i in range(2)]),
    "triclinic_pair": (SHEARED, [np.array([0.11, 0.23, 0.31]), -np.array([0.11, 0.23, 0.31])]),
}
EXPECTED = {"si_primitive": (48, 36), "hcp": (24, 12), "si_conventional": (192, 180), "si_supercell_222": (384, None),
            "triclinic_pair": (2, 0), "si_centring": (4, 3)}          # (operations, of them with tau != 0)


def group_from_package(name):
    """the operations of one cell of ``CELLS`` from the package's ``symmetry_operations``"""
    from dftk_jl_amd.symmetry import symmetry_operations
    lattice, positions = CELLS[name]
    return group_from_ops(name, lattice, symmetry_operations(lattice, [list(range(len(positions)))], positions))


def group_from_ops(name, lattice, ops):
    """a ``Group`` from the package's ``SymOp`` list (integer W, float w made rational)"""
    from fractions import Fraction
    W, num, den = [], [], []
    for op in ops:
        fr = [Fraction(float(x)).limit_denominator(48) for x in op.w]
        d = int(np.lcm.reduce([f.denominator for f in fr]))
        assert all(abs(float(f) - x) < 1e-9 for f, x in zip(fr, op.w))
        W.append(np.asarray(op.W, dtype=np.int64))
        num.append([int(f * d) % d for f in fr])
        den.append(d)
    return Group(name, lattice, W, num, den)


def generate_groups():
    return {name: group_from_package(name) for name in CELLS}


def write_groups(groups, path=GOLDEN):
    doc = {name: {"lattice": g.lattice.tolist(), "W": g.W.reshape(len(g), 9).tolist(), "w_num": g.w_num.tolist(),
                  "w_den": g.w_den.tolist()} for name, g in groups.items()}
    with open(path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")


def load_groups(path=GOLDEN):
    """the committed groups plus ``si_centring``: the four pure translations of conventional Si (S = I, tau != 0 for three)"""
    with open(path) as fh:
        doc = json.load(fh)
    groups = {name: Group(name, d["lattice"], d["W"], d["w_num"], d["w_den"]) for name, d in doc.items()}
    conv = groups["si_conventional"]
    groups["si_centring"] = conv.subset(conv.pure_translations(), "si_centring")
    return groups


def grid_compatible(group, fft_size):
    """every operation maps the real-space grid onto itself: W_ab n_a / n_b and w_a n_a are integers"""
    n = np.asarray(fft_size, dtype=np.int64)
    rot = np.all((group.W * n[None, :, None]) % n[None, None, :] == 0)
    return bool(rot and np.all((group.w_num * n[None, :]) % group.w_den[:, None] == 0))


# ------------------------------------------------------------------------------------------------------------ inputs
def ball_mask(lattice, fft_size):
    """G with |B G| < R, R the distance from the origin to the nearest plane G_a = floor((n_a - 1) / 2) + 1: a ball that lies
    inside the cube's paired frequencies and that every lattice symmetry maps onto itself"""
    L = np.asarray(lattice, dtype=float)
    R = min(((n - 1) // 2 + 1) * 2 * np.pi / np.linalg.norm(L[:, a]) for a, n in enumerate(fft_size))
    Gc = g_cube(fft_size) @ recip(L).T
    return np.sqrt((Gc ** 2).sum(axis=-1)) < R * (1 - 1e-9)


def band_limited(rng, lattice, fft_size):
    """a real random cube whose Fourier coefficients vanish outside ``ball_mask``"""
    x = rng.standard_normal(tuple(fft_size)[::-1])
    out = np.fft.ifftn(np.where(ball_mask(lattice, fft_size), np.fft.fftn(x), 0.0))
    assert np.abs(out.imag).max() < 1e-13
    return np.ascontiguousarray(out.real)


# ------------------------------------------------------------------------------------------------------------ symmetrisation
def symmetrize_fourier(rho, group, fft_size, lowpass, precision="long"):
    """the COMPLEX result cube (the kernel keeps its real part); ``precision``: "long" or "double" """
    long = precision == "long"
    fft_size = tuple(int(n) for n in fft_size)
    G = g_cube(fft_size)
    flat = dftn(rho, -1, precision).reshape(-1)
    acc = np.zeros(G.shape[:-1], dtype=CLD if long else np.complex128)
    keep = np.ones(G.shape[:-1], dtype=bool)
    axes = [freq(n) for n in fft_size]
    for S, tau in zip(group.S, group.tau):
        ok, lin = index_of(G @ int_inverse(S).T, fft_size)
        term = flat[np.where(ok, lin, 0)]
        if np.any(tau != 0.0):
            if long:
                x = G.astype(LD) @ tau.astype(LD)
                ang = (-2 * PI_LD) * (x - np.rint(x))
                phase = np.empty(x.shape, dtype=CLD)
                phase.real, phase.imag = np.cos(ang), np.sin(ang)
            else:          # the same phase as a product over the axes
                px, py, pz = (np.exp(-2j * np.pi * (g * t)) for g, t in zip(axes, tau))
                phase = pz[:, None, None] * py[None, :, None] * px[None, None, :]
            term = term * phase
        acc += np.where(ok, term, 0.0)
        if lowpass:
            keep &= index_of(G @ S.T, fft_size)[0]
    acc = np.where(keep, acc, 0.0) / len(group)
    return dftn(acc, +1, precision) / acc.size


def symmetrize_realspace(rho, group, fft_size):
    """(1 / n_sym) sum_s rho(W_s r + w_s) on the grid points r = (i / nx, j / ny, k / nz), ``np.longdouble``"""
    assert grid_compatible(group, fft_size)
    nx, ny, nz = fft_size
    n = np.asarray(fft_size, dtype=np.int64)
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    I = np.stack([ix, iy, iz]).reshape(3, -1)
    flat = np.asarray(rho).reshape(-1).astype(LD)
    acc = np.zeros(flat.shape, dtype=LD)
    for W, num, den in zip(group.W, group.w_num, group.w_den):
        assert np.all((num * n) % den == 0)                     # every w . n is an integer
        M = (W * n[:, None]) // n[None, :]
        J = np.mod(M @ I + ((num * n) // den)[:, None], n[:, None])
        acc += flat[J[0] + nx * (J[1] + ny * J[2])]
    return (acc / LD(len(group))).reshape(nz, ny, nx)


# ------------------------------------------------------------------------------------------------------------ gradient, filters
def g_cart(lattice, fft_size, dtype=float):
    """cartesian G of every entry, shape (3, nz, ny, nx)"""
    return np.einsum("ij,...j->i...", recip(lattice).astype(dtype), g_cube(fft_size).astype(dtype))


def gradient(f, lattice, fft_size, precision="long"):
    """Re irfft(i G_a fft(f)), a = x, y, z: shape (3, nz, ny, nx)"""
    dt = LD if precision == "long" else float
    c = dftn(f, -1, precision)
    Gc = g_cart(lattice, fft_size, dt)
    return np.stack([(dftn(c.dtype.type(1j) * Gc[a] * c, +1, precision) / c.size).real for a in range(3)])


def paired_max(fft_size):
    """the largest |G_a| per axis that has its -G partner on the grid (no Nyquist entry)"""
    return np.array([(n - 1) // 2 for n in fft_size])


def random_modes(rng, fft_size, count, corners=False):
    """``count`` distinct nonzero integer G strictly inside the grid, amplitudes and phases; ``corners``: the eight
    (+-hx, +-hy, +-hz) with h = ``paired_max`` among them"""
    h = paired_max(fft_size)
    G = {tuple(int(s * v) for s, v in zip(sg, h)) for sg in itertools.product((-1, 1), repeat=3)} if corners else set()
    while len(G) < count:
        g = tuple(int(rng.integers(-v, v + 1)) for v in h)
        if any(g):
            G.add(g)
    G = np.array(sorted(G), dtype=np.int64)
    return G, rng.uniform(0.5, 1.5, len(G)), rng.uniform(0.0, 2 * np.pi, len(G))


def nyquist_wave(fft_size, axis, amp):
    """amp (-1)^i along the (even) axis 0 = x, 1 = y, 2 = z: the pure Nyquist component of that axis"""
    assert fft_size[axis] % 2 == 0
    shape = [1, 1, 1]
    shape[2 - axis] = fft_size[axis]
    return np.ascontiguousarray(np.broadcast_to(amp * ((-1.0) ** np.arange(fft_size[axis])).reshape(shape), fft_size[::-1]))


def trig_polynomial(lattice, fft_size, G, amp, phi, precision="long"):
    """f = sum_j a_j cos(2 pi G_j.r + phi_j) on the grid r = (ix / nx, iy / ny, iz / nz) and its analytic cartesian gradient
    -sum_j a_j sin(2 pi G_j.r + phi_j) B G_j: (f, grad) of shapes (nz, ny, nx) and (3, nz, ny, nx).  The angle of every axis
    comes from (G i mod n) / n reduced in integers; the sum over j is one contraction per cube."""
    dt, cdt, pi = (LD, CLD, PI_LD) if precision == "long" else (np.float64, np.complex128, np.pi)

    def cis(ang):
        t = np.empty(ang.shape, dtype=cdt)
        t.real, t.imag = np.cos(ang), np.sin(ang)
        return t

    X, Y, Z = (cis(2 * pi * (np.outer(G[:, a], np.arange(n)) % n).astype(dt) / dt(n)) for a, n in enumerate(fft_size))
    T = (np.asarray(amp, dtype=dt) * cis(np.asarray(phi, dtype=dt)))[:, None, None] * Z[:, :, None] * Y[:, None, :]
    Gc = G.astype(dt) @ recip(lattice).astype(dt).T                      # (J, 3)
    f = np.tensordot(T, X, axes=([0], [0])).real
    grad = np.stack([np.tensordot(T * (cdt(1j) * Gc[:, a])[:, None, None], X, axes=([0], [0])).real for a in range(3)])
    return f, grad


def g_squared(lattice, fft_size, dtype=float):
    return (g_cart(lattice, fft_size, dtype) ** 2).sum(axis=0)


def kerker_multiplier(G2, fft_size, kTF):
    """mixing.jl:61-72: G^2 / (kTF^2 + G^2), enforce_real! (unpaired Nyquist entries zeroed), DC copied from dF"""
    m = np.where(unpaired_nyquist(fft_size), 0.0, G2 / (kTF ** 2 + G2))
    m.flat[0] = 1.0
    return m


def dielectric_multiplier(G2, kTF, eps_r):
    """mixing.jl:161-171 with C0 = 1 - eps_r, DC kept"""
    C0 = 1 - eps_r
    m = (kTF ** 2 - C0 * G2) / (eps_r * kTF ** 2 - C0 * G2)
    m.flat[0] = 1.0
    return m


def chi0_multiplier(G2, kTF, eps_r):
    """chi0models.jl:66-77: C0 kTF^2 G^2 / (4 pi (kTF^2 - C0 G^2))"""
    C0 = 1 - eps_r
    pi = PI_LD if G2.dtype == LD else np.pi
    return C0 * kTF ** 2 * G2 / (4 * pi) / (kTF ** 2 - C0 * G2)


def apply_multiplier(f, mult, precision="long"):
    """Re irfft(mult fft(f))"""
    return (dftn(mult * dftn(f, -1, precision), +1, precision) / f.size).real
