"""References for the half-sphere format of csrc/gamma_kernels.hip, written from the definitions in that file's header
comment and evaluated in ``numpy.longdouble`` (64-bit mantissa: good to ~1e-19) or, with ``dtype=np.float64``, as the
float64 twin of the same formula that test_gpu_gamma_kernels.py takes its tolerances from.  Host only: nothing here needs
the library or a GPU; test_gamma_reference.py validates it.

  format      row 0 = x(G = 0) (real, imaginary part exactly 0), row j > 0 = sqrt(2) x(G_j) for one representative G_j of
              every pair {G, -G}; the pairs in ascending order of their first row
  compress    h_j = s_j (x(G_j) + conj x(-G_j)), s_0 = 1/2, s_j = 1/sqrt(2): the scaled real-symmetric part of ANY column
  expand      x(G_j) = h_j / sqrt(2), x(-G_j) = conj(h_j) / sqrt(2), x(0) = Re h_0
  align       x exp(-i phi), phi = atan2(Im s, Re s) / 2, s = sum_G x(G) x(-G): the global phase that maximises the
              real-symmetric part
  apply_H     compress . (local + kinetic + P D P') . expand

Blocks are (rows, columns) arrays as in the other test files; mappings are linear indices ix + nx (iy + ny iz)."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -52


def _ctype(dtype):
    return CLD if dtype is LD else np.complex128


def _isqrt2(dtype):
    return dtype(1) / np.sqrt(dtype(2))


# ------------------------------------------------------------------------------------------ spheres and pair tables
def minus_rows(dims, mapping):
    """row of -G for every row of an ascending, inversion-closed mapping"""
    nx, ny, nz = dims
    m = np.asarray(mapping, dtype=np.int64)
    ix, iy, iz = m % nx, (m // nx) % ny, m // (nx * ny)
    lin = (-ix) % nx + nx * ((-iy) % ny + ny * ((-iz) % nz))
    neg = np.searchsorted(m, lin)
    assert np.all(np.diff(m) > 0) and np.all(neg < len(m)) and np.array_equal(m[neg], lin), "not closed under G -> -G"
    return neg


def pairs(dims, mapping):
    """(g, mg): row of G_j and of -G_j, G = 0 first, one representative (the earlier row) per pair"""
    neg = minus_rows(dims, mapping)
    assert mapping[0] == 0 and np.count_nonzero(neg == np.arange(len(neg))) == 1, "G = 0 is the only self-partner allowed"
    g = np.nonzero(neg >= np.arange(len(neg)))[0]
    return g, neg[g]


def below_nyquist(dims):
    """every point of the cube whose three frequencies lie strictly below Nyquist, ascending"""
    ok = [np.array([2 * min(i, n - i) < n for i in range(n)]) for n in dims]
    keep = ok[2][:, None, None] & ok[1][None, :, None] & ok[0][None, None, :]
    return np.nonzero(keep.reshape(-1))[0].astype(np.int64)


def pair_sphere(dims, n_half, rng, pool=None):
    """Ascending mapping with exactly n_half pair rows: G = 0 and n_half - 1 pairs {G, -G} drawn at random from ``pool``
    (default: everything below Nyquist).  A random draw leaves the two members of a pair anywhere in the mapping."""
    pool = below_nyquist(dims) if pool is None else np.asarray(pool, dtype=np.int64)
    neg = pool[minus_rows(dims, pool)]
    reps = np.nonzero(pool < neg)[0]
    assert pool[0] == 0 and 1 <= n_half <= len(reps) + 1, (n_half, len(reps) + 1)
    pick = rng.choice(len(reps), n_half - 1, replace=False)
    return np.sort(np.concatenate([[0], pool[reps[pick]], neg[reps[pick]]])).astype(np.int64)


def signed_freq(n):
    i = np.arange(n)
    return np.where(2 * i < n, i, i - n)


def even_kinetic(dims, mapping):
    """a kinetic factor that is even in G, distinct per axis, exactly representable: (fx^2 + 2 fy^2 + 3 fz^2) / 8"""
    nx, ny, nz = dims
    m = np.asarray(mapping, dtype=np.int64)
    fx, fy, fz = signed_freq(nx)[m % nx], signed_freq(ny)[(m // nx) % ny], signed_freq(nz)[m // (nx * ny)]
    return (fx * fx + 2.0 * fy * fy + 3.0 * fz * fz) / 8.0


# ------------------------------------------------------------------------------------------ inputs
def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def symmetric_columns(rng, g, mg, n, m):
    """(n, m) float64 columns with x(-G) = conj x(G) and Im x(0) = 0, exactly"""
    z = crandn(rng, len(g), m)
    x = np.zeros((n, m), dtype=complex)
    x[g], x[mg] = z, z.conj()
    x[g[0]] = z[0].real
    return x


def half_columns(rng, n_half, m):
    """a generic half-format block; row 0 is real, as the format says"""
    h = crandn(rng, n_half, m)
    h[0] = h[0].real
    return h


def symmetrise_projectors(P, g, mg):
    """P(-G) = conj P(G) and Im P(0) = 0, exactly"""
    Q = np.array(P, dtype=complex)
    Q[mg] = Q[g].conj()
    Q[g[0]] = Q[g[0]].real
    return Q


def banded_D(rng, col_start, bandwidths):
    """real symmetric, block diagonal over the atoms, banded inside a block (test_nonlocal_band_chunks_at_the_abi)"""
    n_p = int(col_start[-1])
    D = np.zeros((n_p, n_p))
    for a, bw in enumerate(bandwidths):
        c0, c1 = int(col_start[a]), int(col_start[a + 1])
        for i in range(c0, c1):
            for j in range(i, min(c1, i + bw + 1)):
                D[i, j] = D[j, i] = rng.uniform(-2, 2)
    return D


def two_theta(rng, m):
    """2 theta at least 0.8 rad away from +- pi: with the 0.46 rad of aligned_input, arg s keeps 0.3 rad from the branch
    cut of atan2"""
    return rng.uniform(-(np.pi - 0.8), np.pi - 0.8, m)


def aligned_input(rng, g, mg, n, two_theta):
    """x = exp(i theta) S + 0.2 Z per column: S a unit real-symmetric vector, Z a unit complex one.  s = sum x(G) x(-G) is
    exp(2 i theta) plus at most 0.4 + 0.04 in modulus, so it stays well conditioned and its argument within 0.46 rad of
    2 theta."""
    m = len(two_theta)
    S = symmetric_columns(rng, g, mg, n, m)
    S /= np.linalg.norm(S, axis=0)[None, :]
    Z = crandn(rng, n, m)
    Z /= np.linalg.norm(Z, axis=0)[None, :]
    return np.exp(0.5j * np.asarray(two_theta))[None, :] * S + 0.2 * Z


# ------------------------------------------------------------------------------------------ the format
def compress(x, g, mg, dtype=LD):
    x = np.asarray(x).astype(_ctype(dtype))
    h = (x[g] + np.conj(x[mg])) * _isqrt2(dtype)
    h[0] = x[g[0]].real
    return h


def compress_bound(x, g, mg):
    """4 * 2^-52 s_j (|x(G_j)| + |x(-G_j)|): one add, one product with a correctly rounded constant, with room"""
    x = np.asarray(x).astype(CLD)
    s = np.full(len(g), _isqrt2(LD))
    s[0] = LD(1) / 2
    return 4 * LD(U) * s.reshape((-1,) + (1,) * (x.ndim - 1)) * (np.abs(x[g]) + np.abs(x[mg]))


def expand(h, g, mg, n, dtype=LD):
    h = np.asarray(h).astype(_ctype(dtype))
    x = np.zeros((n,) + h.shape[1:], dtype=h.dtype)
    x[g] = h * _isqrt2(dtype)
    x[mg] = np.conj(h) * _isqrt2(dtype)
    x[g[0]] = h[0].real
    return x


def expand_bound(h, g, mg, n):
    """2 * 2^-52 |h_j| / sqrt(2) on both members of a pair (one product with a correctly rounded constant); row G = 0
    is a copy: 0"""
    h = np.asarray(h).astype(CLD)
    b = np.zeros((n,) + h.shape[1:], dtype=LD)
    b[g] = b[mg] = 2 * LD(U) * np.abs(h) * _isqrt2(LD)
    b[g[0]] = 0
    return b


def pair_sum(x, g, mg, dtype=LD):
    """(s, S): s = sum_G x(G) x(-G) = x(0)^2 + 2 sum_{j > 0} x(G_j) x(-G_j) per column and S = sum_G |x(G) x(-G)|;
    the aligned result depends on s through 1 / |s|, so |s| / S is its condition"""
    x = np.asarray(x).astype(_ctype(dtype))
    t = x[g] * x[mg]
    w = np.full(len(g), dtype(2))
    w[0] = 1
    w = w.reshape((-1,) + (1,) * (x.ndim - 1))
    return (w * t).sum(axis=0), (w * np.abs(t)).sum(axis=0)


def align(x, g, mg, dtype=LD):
    x = np.asarray(x).astype(_ctype(dtype))
    s, _ = pair_sum(x, g, mg, dtype)
    phi = np.arctan2(s.imag, s.real) / 2          # (a zero column: atan2(0, 0) = 0)
    rot = np.empty(s.shape, dtype=x.dtype)
    rot.real, rot.imag = np.cos(phi), -np.sin(phi)
    return x * rot[None, ...]


def compress_aligned(x, g, mg, dtype=LD):
    return compress(align(x, g, mg, dtype), g, mg, dtype)


# ------------------------------------------------------------------------------------------ H in the half format
def apply_H(h, g, mg, n, which, local, kin, P, D, dtype=LD):
    """The five steps: expand; to the cube, times V, back, / N, onto the sphere (``local``: (nb, n) -> (nb, n) in the
    precision of ``dtype``); + kin x + P D P' x with the full complex P; compress.  which: bit 0 local, 1 kinetic,
    2 nonlocal."""
    C = _ctype(dtype)
    x = expand(h, g, mg, n, dtype)
    y = np.zeros_like(x)
    if which & 1:
        y = y + np.asarray(local(x.T)).astype(C).T
    if which & 2:
        y = y + np.asarray(kin).astype(dtype)[:, None] * x
    if (which & 4) and P.shape[1] > 0:
        Pc = np.asarray(P).astype(C)
        y = y + Pc @ (np.asarray(D).astype(dtype) @ (Pc.conj().T @ x))
    return compress(y, g, mg, dtype)
