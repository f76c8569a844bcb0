"""The extended-precision references of gamma_ref.py, checked on the host before test_gpu_gamma_kernels.py holds the
kernels of csrc/gamma_kernels.hip to them:

  * the synthetic spheres have exactly the rows they promise, in the order ``dftk_mi_kblock_create`` requires, and
    their pair tables agree with a brute-force search; representatives and partners interleave;
  * the format is what the header comment of gamma_kernels.hip says: expand inverts compress on real-symmetric
    columns, the plain real dot product of two half columns is the full inner product, i times a real field
    compresses to zero;
  * the alignment phase maximises the norm of the compressed column, returns a rotated real field as +- itself, and the
    construction of the GPU file keeps |s| >= 0.5 sum |x(G) x(-G)| and the branch of atan2 out of play;
  * apply_H is compress . H . expand of an explicitly assembled dense matrix, and that operator is real symmetric
    in the 2 n_half real coordinates;
  * the float64 twin of every formula agrees with the long-double one to a few 1e-16: a correct fp64 evaluation sits
    well inside the margins of the GPU file;
  * the inputs exercise what they claim: dropping a rule (sqrt 2, the factor of row 0, the conjugate of the partner,
    the weight 2 of the pair sum) moves a reference by more than 1e-3 of its norm."""
import numpy as np
import pytest

import gamma_ref as gr

LD, CLD = gr.LD, gr.CLD
NHALF = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)      # the list of the GPU file
CUBE = (33, 33, 33)


def rel(a, b):
    a, b = np.asarray(a).astype(CLD), np.asarray(b).astype(CLD)
    return float(np.sqrt((np.abs(a - b) ** 2).sum()) / max(np.sqrt((np.abs(b) ** 2).sum()), LD(1e-300)))


def brute_pairs(dims, mapping):
    nx, ny, nz = dims
    row = {int(v): i for i, v in enumerate(mapping)}
    g, mg = [], []
    for i, v in enumerate(mapping):
        ix, iy, iz = int(v) % nx, (int(v) // nx) % ny, int(v) // (nx * ny)
        p = row[(-ix) % nx + nx * ((-iy) % ny + ny * ((-iz) % nz))]
        if p >= i:
            g.append(i)
            mg.append(p)
    return np.array(g), np.array(mg)


@pytest.mark.parametrize("dims,n_half", [((5, 5, 5), 1), ((5, 5, 5), 63), ((7, 8, 9), 20), ((12, 9, 10), 33),
                                         ((33, 33, 33), 257), ((33, 33, 33), 8193)])
def test_pair_sphere_and_tables(dims, n_half):
    rng = np.random.default_rng(n_half)
    m = gr.pair_sphere(dims, n_half, rng)
    assert len(m) == 2 * n_half - 1 and m[0] == 0 and np.all(np.diff(m) > 0) and m[-1] < np.prod(dims)
    assert np.all(np.isin(m, gr.below_nyquist(dims)))
    g, mg = gr.pairs(dims, m)
    bg, bmg = brute_pairs(dims, m)
    assert np.array_equal(g, bg) and np.array_equal(mg, bmg) and len(g) == n_half and g[0] == mg[0] == 0
    assert np.all(np.diff(g) > 0) and np.all(mg[1:] > g[1:])
    assert np.array_equal(np.sort(np.concatenate([g, mg[1:]])), np.arange(len(m)))
    if n_half >= 20:       # some partner row precedes some representative: g is not a contiguous range
        assert mg[1:].min() < g.max()
    if dims == CUBE and n_half == 257:      # a sparse draw from 17968 pairs: the members of a pair lie far apart
        assert (mg - g).max() > n_half


def test_below_nyquist_is_closed_and_excludes_the_nyquist_planes():
    for dims in [(5, 5, 5), (7, 8, 9), (12, 9, 10), (16, 15, 18)]:
        pts = gr.below_nyquist(dims)
        nx, ny, nz = dims
        assert len(pts) == np.prod([n if n % 2 else n - 1 for n in dims])
        neg = gr.minus_rows(dims, pts)
        assert np.array_equal(np.nonzero(neg == np.arange(len(pts)))[0], [0])
        for n, c in zip(dims, (pts % nx, (pts // nx) % ny, pts // (nx * ny))):
            assert n % 2 or not np.any(c == n // 2)


@pytest.mark.parametrize("n_half", [1, 2, 257, 1025])
def test_format_identities(n_half):
    rng = np.random.default_rng(10 + n_half)
    m = gr.pair_sphere(CUBE, n_half, rng)
    g, mg = gr.pairs(CUBE, m)
    n = len(m)
    X, Y = gr.symmetric_columns(rng, g, mg, n, 3), gr.symmetric_columns(rng, g, mg, n, 3)
    neg = gr.minus_rows(CUBE, m)
    assert np.array_equal(X[neg], X.conj()) and not X[0].imag.any()
    hx, hy = gr.compress(X, g, mg), gr.compress(Y, g, mg)
    assert not hx[0].imag.any()
    assert rel(gr.expand(hx, g, mg, n), X) < 1e-18
    # the plain real dot product of the 2 n_half real numbers is the full inner product
    dot = hx.real.T @ hy.real + hx.imag.T @ hy.imag
    full = X.astype(CLD).conj().T @ Y.astype(CLD)
    assert rel(dot, full) < 1e-17 and float(np.abs(full.imag).max()) < 1e-17 * float(np.abs(full).max())
    # compress is the projection on the real-symmetric part: i times a real field has none
    assert float(np.abs(gr.compress(1j * X, g, mg)).max()) == 0.0
    Z = gr.crandn(rng, n, 2)
    sym = (Z + Z[neg].conj()) / 2
    assert rel(gr.expand(gr.compress(Z, g, mg), g, mg, n), sym.astype(CLD)) < 1e-16
    # expand ignores Im h_0 and writes every row
    h = gr.crandn(rng, n_half, 2)
    x = gr.expand(h, g, mg, n)
    assert np.array_equal(x[0], h[0].real.astype(CLD)) and (n_half == 1 or np.all(np.abs(x[1:]) > 0))
    # the bounds are the ones of the operation count
    assert np.array_equal(gr.expand_bound(h, g, mg, n)[0], np.zeros(2))
    if n_half > 1:
        j = n_half - 1
        want = 4 * LD(gr.U) / np.sqrt(LD(2)) * (np.abs(Z[g[j]].astype(CLD)) + np.abs(Z[mg[j]].astype(CLD)))
        assert np.allclose((gr.compress_bound(Z, g, mg)[j] / want).astype(float), 1.0, rtol=1e-15)
        assert np.allclose((gr.compress_bound(Z, g, mg)[0] / (4 * LD(gr.U) * np.abs(Z[0].astype(CLD)))).astype(float), 1.0,
                           rtol=1e-15)


@pytest.mark.parametrize("n_half", [2, 255, 1025])
def test_alignment_maximises_the_real_symmetric_part(n_half):
    rng = np.random.default_rng(20 + n_half)
    m = gr.pair_sphere(CUBE, n_half, rng)
    g, mg = gr.pairs(CUBE, m)
    n = len(m)
    X = gr.crandn(rng, n, 4)
    best = np.linalg.norm(gr.compress_aligned(X, g, mg).astype(complex), axis=0)
    for phi in np.linspace(0, np.pi, 181):
        other = np.linalg.norm(gr.compress(X * np.exp(-1j * phi), g, mg).astype(complex), axis=0)
        assert np.all(other <= best * (1 + 1e-12))
    # |compress(x e^{-i phi})|^2 = (|x|^2 + Re(e^{-2 i phi} s)) / 2: at the maximum (|x|^2 + |s|) / 2
    s, _ = gr.pair_sum(X, g, mg)
    assert np.allclose(best ** 2, (np.linalg.norm(X, axis=0) ** 2 + np.abs(s).astype(float)) / 2, rtol=1e-13)
    # a real field times any phase comes back as +- itself; a zero column stays zero
    S = gr.symmetric_columns(rng, g, mg, n, 5)
    ph = np.array([0.0, np.pi / 2, 0.3, -2.1, 1.0])
    got = gr.compress_aligned(S * np.exp(1j * ph)[None, :], g, mg)
    base = gr.compress(S, g, mg)
    for c in range(5):
        assert min(rel(got[:, c], base[:, c]), rel(-got[:, c], base[:, c])) < 1e-15
    assert not np.abs(gr.compress_aligned(np.zeros((n, 1), dtype=complex), g, mg)).any()
    # exactly real-symmetric input: s > 0 with a zero imaginary part, phi = 0, nothing is rotated
    s, _ = gr.pair_sum(S, g, mg)
    assert np.all(s.imag == 0) and np.all(s.real > 0)
    assert np.array_equal(gr.compress_aligned(S, g, mg), base)
    s, _ = gr.pair_sum(1j * S, g, mg)
    assert np.all(s.imag == 0) and np.all(s.real < 0)


two_theta = gr.two_theta


@pytest.mark.parametrize("n_half", NHALF)
def test_aligned_inputs_are_well_conditioned(n_half):
    """The condition the GPU file asserts per column, here over 20 seeds: |s| >= 0.5 sum |x(G) x(-G)| with margin, and
    arg s at least 0.3 rad away from +- pi."""
    worst, edge = 1.0, 1.0
    for seed in range(20):
        rng = np.random.default_rng(1000 * n_half + seed)
        m = gr.pair_sphere(CUBE, n_half, rng)
        g, mg = gr.pairs(CUBE, m)
        tt = two_theta(rng, 5)
        x = gr.aligned_input(rng, g, mg, len(m), tt)
        s, S = gr.pair_sum(x, g, mg)
        worst = min(worst, float((np.abs(s) / S).min()))
        edge = min(edge, float((np.pi - np.abs(np.arctan2(s.imag, s.real))).min()))
        assert float(np.abs(np.angle(s.astype(complex) * np.exp(-1j * tt))).max()) < 0.46
    print(f"\nn_half = {n_half}: smallest |s| / sum |x(G) x(-G)| = {worst:.3f}, closest to the branch cut {edge:.3f} rad")
    assert worst >= 0.9 and edge >= 0.3


@pytest.mark.parametrize("n_half", [2, 257, 4097])
def test_float64_twins_sit_at_round_off(n_half):
    rng = np.random.default_rng(30 + n_half)
    m = gr.pair_sphere(CUBE, n_half, rng)
    g, mg = gr.pairs(CUBE, m)
    n = len(m)
    X = gr.aligned_input(rng, g, mg, n, two_theta(rng, 5))
    for fn in (gr.compress, gr.compress_aligned):
        ref, twin = fn(X, g, mg), fn(X, g, mg, dtype=np.float64)
        assert ref.dtype == CLD and twin.dtype == np.complex128
        for c in range(5):
            assert rel(twin[:, c], ref[:, c]) < 8 * gr.U
    h = gr.half_columns(rng, n_half, 3)
    assert rel(gr.expand(h, g, mg, n, dtype=np.float64), gr.expand(h, g, mg, n)) < 2 * gr.U


def dense_local(dims, mapping, V):
    """the (n, n) matrix of c -> FFT[V IFFT[pad c]] / N on the sphere, column by column with numpy.fft"""
    nx, ny, nz = dims
    m = np.asarray(mapping)
    L = np.zeros((len(m), len(m)), dtype=complex)
    for c in range(len(m)):
        pad = np.zeros(nx * ny * nz, dtype=complex)
        pad[m[c]] = 1.0
        cube = np.fft.ifftn(pad.reshape(nz, ny, nx), norm="forward")
        L[:, c] = (np.fft.fftn(V * cube) / (nx * ny * nz)).reshape(-1)[m]
    return L


def local64(dims, mapping, V):
    nx, ny, nz = dims
    m = np.asarray(mapping)

    def f(c):
        pad = np.zeros((len(c), nx * ny * nz), dtype=complex)
        pad[:, m] = c
        cube = np.fft.ifftn(pad.reshape(-1, nz, ny, nx), axes=(1, 2, 3), norm="forward")
        return np.fft.fftn(V[None] * cube, axes=(1, 2, 3)).reshape(len(c), -1)[:, m] / (nx * ny * nz)
    return f


@pytest.mark.parametrize("dims,n_half", [((5, 5, 5), 1), ((5, 5, 5), 30), ((7, 8, 9), 41)])
def test_apply_H_is_the_compressed_dense_operator(dims, n_half):
    rng = np.random.default_rng(40 + n_half)
    m = gr.pair_sphere(dims, n_half, rng)
    g, mg = gr.pairs(dims, m)
    n = len(m)
    nx, ny, nz = dims
    V = rng.standard_normal((nz, ny, nx))
    kin = gr.even_kinetic(dims, m)
    assert np.array_equal(kin[g], kin[mg]) and (n_half == 1 or len(np.unique(kin)) > 1)
    col_start = [0, 4, 4, 13]
    P = gr.symmetrise_projectors(gr.crandn(rng, n, 13), g, mg)
    neg = gr.minus_rows(dims, m)
    assert np.array_equal(P[neg], P.conj())
    D = gr.banded_D(rng, col_start, (1, 0, 2))
    assert np.array_equal(D, D.T) and not D[:4, 4:].any() and D[4, 6] != 0 and D[4, 7] == 0
    parts = {1: dense_local(dims, m, V), 2: np.diag(kin).astype(complex), 4: P @ D @ P.conj().T}
    # the half format as a real-linear map on the 2 n_half real coordinates (row 0 has one)
    E = np.zeros((n, 2 * n_half), dtype=complex)
    for j in range(n_half):
        for part, unit in ((0, 1.0), (1, 1j)):
            e = np.zeros((n_half, 1), dtype=complex)
            e[j] = unit
            E[:, 2 * j + part] = gr.expand(e, g, mg, n, dtype=np.float64)[:, 0]
    h = gr.half_columns(rng, n_half, 3)
    hr = np.stack([h.real, h.imag], axis=1).reshape(2 * n_half, 3)
    loc = local64(dims, m, V)
    for which in range(1, 8):
        Hd = sum(parts[b] for b in (1, 2, 4) if which & b)
        assert np.linalg.norm(Hd - Hd.conj().T) <= 1e-13 * np.linalg.norm(Hd)
        full = gr.compress(Hd @ (E @ hr), g, mg, dtype=np.float64)
        twin = gr.apply_H(h, g, mg, n, which, loc, kin, P, D, dtype=np.float64)
        assert rel(twin, full) < 1e-13, which
        assert not twin[0].imag.any()
        # the restricted operator is real symmetric: R = E' Hd E has no imaginary part and R = R'
        R = E.conj().T @ Hd @ E
        assert np.abs(R.imag).max() <= 1e-13 * np.abs(R).max() and np.abs(R - R.T).max() <= 1e-13 * np.abs(R).max()
        # long double with the same float64 local part: the other four steps agree to round-off
        ld = gr.apply_H(h, g, mg, n, which, loc, kin, P, D)
        assert ld.dtype == CLD and rel(twin, ld) < 1e-14, which


def test_the_inputs_notice_a_dropped_rule():
    rng = np.random.default_rng(5)
    m = gr.pair_sphere(CUBE, 257, rng)
    g, mg = gr.pairs(CUBE, m)
    n = len(m)
    X = gr.crandn(rng, n, 2)
    ref = gr.compress(X, g, mg)
    wrong = {"0.5 for sqrt(1/2)": (X[g] + X[mg].conj()) * 0.5,
             "row 0 scaled like the others": np.concatenate([(X[g[:1]].real * np.sqrt(2)), ref[1:].astype(complex)]),
             "no conjugate on the partner": np.concatenate([ref[:1].astype(complex), (X[g] + X[mg])[1:] / np.sqrt(2)])}
    for name, w in wrong.items():
        assert rel(w, ref) > 1e-3, name
    h = gr.half_columns(rng, 257, 2)
    x = gr.expand(h, g, mg, n)
    flipped = x.copy()
    flipped[mg[1:]] = np.conj(flipped[mg[1:]])
    assert rel(flipped, x) > 1e-3
    # the weight 2 of the pair sum counts against row 0 only: a small sphere, generic columns
    m = gr.pair_sphere((5, 5, 5), 3, rng)
    g, mg = gr.pairs((5, 5, 5), m)
    Xa = gr.crandn(rng, len(m), 4)
    s, _ = gr.pair_sum(Xa, g, mg)
    s1 = (Xa[g] * Xa[mg]).sum(axis=0)                    # weight 1 for every pair
    good, bad = gr.compress_aligned(Xa, g, mg), gr.compress(Xa * np.exp(-0.5j * np.angle(s1))[None, :], g, mg)
    assert rel(bad, good) > 1e-3, (np.angle(s.astype(complex)), np.angle(s1))
