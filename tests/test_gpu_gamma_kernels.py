"""The format kernels of csrc/gamma_kernels.hip (pair tables, compress, compress_aligned, expand, pack / unpack around the
FFT pipeline, the half-format projectors) at the C ABI, on the tile, trip and pair edges, against the long-double
references of gamma_ref.py (validated on the host by test_gamma_reference.py).  No reference comes from a device call.

Shapes, and why each is there
  pair tables   synthetic inversion-closed mappings drawn pair by pair (gamma_ref.pair_sphere): representatives and
                partners interleave, a sparse draw leaves the two members of a pair thousands of rows apart; n_G = 1;
                count only (both tables null); one table null; a missing partner, a Nyquist self-partner and
                mapping[0] != 0, each with its own message.
  compress /    subsets of the 33^3 cube (all axes odd: no Nyquist plane, 17969 pairs) with n_half = 1, 2 (row 0 alone,
  expand /      one pair), 255 / 256 / 257 (one 256-thread stride of a workgroup), 1023 / 1024 / 1025 (GR_ROWS = 1024 pairs
  aligned       per workgroup: the second workgroup starts at 1025), 4095 / 4096 / 4097 (GRA_NT * GR_UNR = 4096 pairs per
                trip of the one-workgroup-per-column aligned kernel: the second trip starts at 4097), 8193 (third trip,
                ninth workgroup); m = 1, 3, 5 columns; both leading dimensions = rows + 7 with NaN in the input padding;
                outputs NaN-filled where they must be written, sentinel-filled everywhere else and between 1 KiB guards;
                every call made twice (bitwise equal); m = 0.
  apply_H       cubes (5, 5, 5), (7, 8, 9), (12, 9, 10), (16, 15, 18) (every axis parity), on each a sparse sphere
                (n_half in the tens, thinned from synthetic_sphere(..., inversion=True)) and the fullest one (everything
                strictly below Nyquist; on (5, 5, 5) the whole cube), on (5, 5, 5) also {0}; a generic real V, an even
                kinetic factor, three "atoms" of 4 / 0 / 9 projector columns symmetrised exactly, banded D blocks;
                1, 2, 3 and 2 * 32 + 1 = 65 bands at the default FFT batch (33 pairs: two launch groups, the last pair
                odd), 2 and 3 bands at FFT batch 1; which = 1 .. 7; ld_psi = ld_Hpsi = n_half + 7; one spare column after
                the last band on both sides (NaN in psi, sentinel in H psi).
  projectors    n_half = 513 (three 256-row workgroups of k_gr_gather_P), n_p = 13; the perturbed entry is the partner of
                the LAST pair of the LAST column (third workgroup), the NaN sits in a partner row of the middle workgroup.

Bounds, and where each comes from (none is measured on the kernels)
  compress      |got_j - ref_j| <= 4 * 2^-52 s_j (|x(G_j)| + |x(-G_j)|), s_0 = 1/2, s_j = 1/sqrt 2: one add and one product
                with a correctly rounded constant are 3 * 2^-53 at most; Im got_0 == 0 exactly.
  expand        |got - ref| <= 2 * 2^-52 |h_j| / sqrt 2 on both members (one product with a rounded constant: 2 * 2^-53);
                row G = 0 == (Re h_0, 0) exactly; every row written.
  round trip    expand . compress of real-symmetric columns: the sum of the two bounds.
  aligned       per column |got - ref|_2 / |ref|_2 <= 64 max(e64, 2.2e-16), e64 the error of the float64 NumPy evaluation
                of the same formula -- the rule of test_gpu_fft_axes.py: a margin over the reference's fp64 twin (the device
                sums 1024 partials in a tree, NumPy pairwise; device atan2 / sincos may lose a bit more).  The inputs
                x = exp(i theta) S + 0.2 Z keep |s| >= 0.5 sum |x(G) x(-G)| (asserted per column; >= 0.93 over 20 seeds in
                test_gamma_reference.py) and arg s 0.3 rad from the branch cut of atan2.
  branches      zero column: zeros; real-symmetric column: bitwise dftk_mi_gamma_compress; i times a real-symmetric
                column: +- the plain compression of the unrotated column within the compress bound + 2^-52 |x|_2 (the
                rotation by cos(pi/2) = 6.1e-17, sin = 1 adds less than 1.7e-16 |x|_2 to an entry).
  apply_H,      |got - ref|_2 / |ref|_2 <= 64 max(e_np, 2.2e-16) over the block, e_np the error of the float64 twin of the
  projectors    five reference steps built on numpy.fft (Tally of test_gpu_fft_axes.py); Im out_0 == 0 exactly.
  pair packing  H of bands (a, b) alone == the same two columns of a 3-band call, bitwise, for which = 1, 2, 3: pack /
                unpack run one workgroup column per pair (blockIdx.y = pair), every FFT stage one workgroup per (band,
                column group or plane) -- the band count of a launch only places workgroups -- and k_kinetic is
                element-wise.  Not claimed for which & 4: the K split of the two projector products is chosen by a cost
                model from the shape (n_p x n_bands x n_half), so 2 and 3 bands may sum in different orders.
  refusals      1e-10 max|P| is the library's threshold: 1e-13 max|P| passes, 1e-8 max|P| and NaN do not.

Largest measured err / bound on MI355X (every test prints its own figures; nothing was found wrong):
    compress      0.283   n_half = 257                      (exact at n_half = 1)
    expand        0.400   n_half = 8193
    round trip    0.185   n_half = 8193
    aligned       0.011   n_half = 257; worst err / e64 = 2.20 at n_half = 2 (err 1.06e-16), 0.92 .. 1.52 elsewhere
    i * real      0.049   n_half = 255
    apply_H       0.039   which = 1 on (5, 5, 5); worst err / e_np = 20.3 on the sphere {0}, which = 6, one band (err 1.7e-16,
                          the twin's own error is 8.5e-18 there), 6.7 for which = 1 on {0}, at most 1.98 on the larger cubes
    projectors    0.020   worst err / e_np = 1.31

One-line changes of gamma_kernels.hip (none moves a load or store out of its buffer: the spare psi column is what the
sixth reads), each built in a copy outside the repository and run against this file alone, and the tests they fail:
    GR_ISQRT2 -> 0.5 in k_gr_compress              compress_and_expand_on_the_tile_edges[2 .. 8193],
                                                   compress_aligned_exact_branches[2 .. 8193] (the bitwise twin)
    row-0 factor 0.5 -> GR_ISQRT2, k_gr_compress   the same two tests at every n_half, 1 included
    the same in k_gr_compress_aligned              compress_aligned_against_its_definition and _exact_branches, every n_half
    the same in k_gr_unpack                        apply_H_against_the_dense_long_double_operator, all four cubes
    sign of Im stored to x[im] in k_gr_expand      compress_and_expand_on_the_tile_edges[2 .. 8193]
    weight 2.0 -> 1.0 in the aligned sum           compress_aligned_against_its_definition[2 .. 8193]
    step GRA_NT * GR_UNR -> GRA_NT, reduction      compress_aligned_against_its_definition[1025, 4095, 4096, 4097, 8193]
    pass only                                      (rows from 1024 on are counted more than once)
    has_b forced true for the loads of k_gr_pack   apply_H_against_the_dense_long_double_operator, all four cubes, and
                                                   projectors_accepted_and_refused (the NaN of the spare column comes out)
    1e-10 -> 1e-6 in gr_projectors                 projectors_accepted_and_refused (1e-8 max|P| is accepted)
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402

import gamma_ref as gr  # noqa: E402
import test_gpu_fft_axes as fa  # noqa: E402
from test_gpu_fft_axes import Guarded, SENTINEL, Sphere, Tally, synthetic_sphere  # noqa: E402
from test_gpu_gamma_real import pair_tables  # noqa: E402
from test_gpu_kernels import Basis, KBlock, dev  # noqa: E402

LD, CLD = np.longdouble, np.clongdouble
assert np.finfo(LD).eps < 1.1e-19, "the reference needs a long double with a 64-bit mantissa"
U = 2.0 ** -52
EPS = 2.2e-16
FACTOR = 64          # err <= FACTOR max(e64, EPS): the margin over the float64 twin of the reference
EINVAL = -1          # DFTK_MI_EINVAL
PAD = 7
CUBE = (33, 33, 33)
NHALF = (1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8193)
COLUMNS = (1, 3, 5)
NAN = complex(float("nan"), float("nan"))
MARK = complex(SENTINEL, SENTINEL)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def cube33(lib):
    return Basis(lib, *CUBE)


class BoundTally(Tally):
    """Tally of test_gpu_fft_axes.py (err <= 64 max(e_np, 2.2e-16)) that also prints the largest err / bound"""

    def __init__(self, family):
        fa.FACTOR.setdefault(family, FACTOR)
        super().__init__(family)
        self.tightest = 0.0

    def add(self, label, got, got64, ref):
        super().add(label, got, got64, ref)
        self.tightest = max(self.tightest, fa.relerr(got, ref) / (FACTOR * max(fa.relerr(got64, ref), EPS)))

    def finish(self):
        print(f"[{self.family}] worst err / bound = {self.tightest:.4f}")
        super().finish()


def tally(family):
    return BoundTally(family)


# ------------------------------------------------------------------------------------------ buffers
def in_buffer(block, ld, spare=0):
    """(rows, m) -> device (m + spare, ld), NaN wherever the call has no business reading"""
    rows, m = block.shape
    buf = np.full((m + spare, ld), NAN)
    buf[:m, :rows] = block.T
    return dev(buf)


def out_buffer(rows, m, ld, spare=0):
    """(m + spare, ld) between guards: NaN where the call must write, the sentinel in the padding rows and spare columns"""
    fill = np.full((m + spare, ld), MARK)
    fill[:m, :rows] = NAN
    return Guarded(fill.shape, torch.complex128, fill=fill)


def take(out, rows, m, label, written=True):
    """the (rows, m) result; every entry outside it still holds the sentinel, bit for bit"""
    raw = out.numpy(label)
    outside = np.ones(raw.shape, dtype=bool)
    outside[:m, :rows] = False
    assert np.all(raw.real[outside] == SENTINEL) and np.all(raw.imag[outside] == SENTINEL), \
        f"{label}: store into the padding rows or past the last column"
    got = raw[:m, :rows].T.copy()
    if written:
        assert not np.isnan(got.real).any() and not np.isnan(got.imag).any(), f"{label}: rows left unwritten or NaN read"
    else:
        assert np.isnan(got.real).all() and np.isnan(got.imag).all(), f"{label}: a call with nothing to do wrote"
    return got


def worst_ratio(err, bound):
    """max err / bound; where the bound is 0 the error must be 0"""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    assert np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def col_rel(got, ref):
    d = np.asarray(got).astype(CLD) - ref
    return (np.sqrt((np.abs(d) ** 2).sum(axis=0)) / np.sqrt((np.abs(ref) ** 2).sum(axis=0))).astype(float)


# ------------------------------------------------------------------------------------------ 1. pair tables
def tables_host(lib, dims, mapping, want_tables=True):
    m = np.ascontiguousarray(mapping, dtype=np.int64)
    cnt = C.c_int64(-1)
    rows = np.full((len(m) + 1) // 2 + 1, -7, dtype=np.int32)
    prt = np.full_like(rows, -7)
    st = lib.dftk_mi_gamma_tables_host(*dims, len(m), m.ctypes.data, C.byref(cnt),
                                       rows.ctypes.data if want_tables else None, prt.ctypes.data if want_tables else None)
    return st, cnt.value, rows, prt


@pytest.mark.parametrize("dims,n_half", [((33, 33, 33), 257), ((33, 33, 33), 8193), ((7, 8, 9), 31), ((12, 9, 10), 2),
                                         ((16, 15, 18), 1913), ((5, 5, 5), 63)])
def test_pair_tables_on_synthetic_mappings(lib, dims, n_half):
    rng = np.random.default_rng(100 + n_half)
    m = gr.pair_sphere(dims, n_half, rng)
    g, mg = pair_tables(dims, m)
    assert len(g) == n_half and np.array_equal(g, gr.pairs(dims, m)[0]) and np.array_equal(mg, gr.pairs(dims, m)[1])
    if n_half > 2:
        assert mg[1:].min() < g.max(), "representatives and partners are meant to interleave"
    if n_half == 257:
        assert (mg - g).max() > 257, "a sparse draw is meant to leave the members of a pair far apart"
    st, cnt, rows, prt = tables_host(lib, dims, m)
    assert st == 0 and cnt == n_half
    assert np.array_equal(rows[:n_half], g) and np.array_equal(prt[:n_half], mg) and rows[0] == prt[0] == 0
    assert np.all(rows[n_half:] == -7) and np.all(prt[n_half:] == -7)
    st, cnt, rows, prt = tables_host(lib, dims, m, want_tables=False)
    assert st == 0 and cnt == n_half and np.all(rows == -7)


def test_pair_tables_single_row_and_refusals(lib):
    st, cnt, rows, prt = tables_host(lib, (5, 5, 5), [0])
    assert st == 0 and cnt == 1 and rows[0] == prt[0] == 0
    st, cnt, _, _ = tables_host(lib, (5, 5, 5), [0], want_tables=False)
    assert st == 0 and cnt == 1
    # exactly one table
    m = np.ascontiguousarray(gr.pair_sphere((7, 8, 9), 12, np.random.default_rng(1)))
    cnt, tab = C.c_int64(-1), np.full(13, -7, dtype=np.int32)
    assert lib.dftk_mi_gamma_tables_host(7, 8, 9, len(m), m.ctypes.data, C.byref(cnt), tab.ctypes.data, None) == EINVAL
    assert lib.dftk_mi_gamma_tables_host(7, 8, 9, len(m), m.ctypes.data, C.byref(cnt), None, tab.ctypes.data) == EINVAL
    assert cnt.value == -1 and np.all(tab == -7)
    # a missing partner
    g, mg = gr.pairs((7, 8, 9), m)
    st, cnt, _, _ = tables_host(lib, (7, 8, 9), np.delete(m, mg[5]))
    assert st == EINVAL and cnt == -1 and b"no -G partner" in lib.dftk_mi_last_error()
    # a Nyquist point is its own partner (x = 4 of 8, y = z = 0), with and without other pairs around it
    for nyq in ([0, 4], [0, 1, 4, 7]):
        st, cnt, _, _ = tables_host(lib, (8, 7, 9), nyq)
        assert st == EINVAL and cnt == -1 and b"its own inversion partner" in lib.dftk_mi_last_error()
    # G = 0 must come first
    st, cnt, _, _ = tables_host(lib, (7, 8, 9), m[1:])
    assert st == EINVAL and cnt == -1 and b"G = 0 as its first entry" in lib.dftk_mi_last_error()
    # and the entry goes on working
    assert tables_host(lib, (7, 8, 9), m)[:2] == (0, 12)


# ------------------------------------------------------------------------------------------ 2. the format kernels
@functools.lru_cache(maxsize=None)
def sphere33(n_half):
    m = gr.pair_sphere(CUBE, n_half, np.random.default_rng(7000 + n_half))
    g, mg = gr.pairs(CUBE, m)
    for a in (m, g, mg):
        a.setflags(write=False)
    return m, g, mg


class HalfBlock:
    """A Gamma-real k-block on a synthetic sphere; ``run`` makes one ABI call twice with padded, poisoned buffers"""

    def __init__(self, lib, bs, dims, mapping, kin=None):
        self.lib, self.bs = lib, bs
        self.g, self.mg = gr.pairs(dims, mapping)
        self.n, self.nh = len(mapping), len(self.g)
        self.kb = KBlock(lib, bs, mapping, np.zeros(self.n) if kin is None else kin)
        check(lib.dftk_mi_kblock_set_gamma_real(self.kb.h, 1))
        nh = C.c_int64()
        check(lib.dftk_mi_gamma_half_size(self.kb.h, C.byref(nh)))
        assert nh.value == self.nh

    def run(self, entry, block, rows_out, label, m=None):
        rows_in = block.shape[0]
        m = block.shape[1] if m is None else m
        src = in_buffer(block, rows_in + PAD)
        outs = []
        for _ in range(2):
            out = out_buffer(rows_out, block.shape[1], rows_out + PAD)
            check(getattr(self.lib, entry)(self.kb.h, m, src.data_ptr(), rows_in + PAD, out.ptr(), rows_out + PAD))
            self.bs.sync()
            outs.append(take(out, rows_out, block.shape[1], f"{label}, {entry}", written=m > 0))
        assert outs[0].tobytes() == outs[1].tobytes(), f"{label}, {entry}: two calls differ"
        return outs[0]


@pytest.mark.parametrize("n_half", NHALF)
def test_compress_and_expand_on_the_tile_edges(lib, cube33, n_half):
    m33, g, mg = sphere33(n_half)
    blk = HalfBlock(lib, cube33, CUBE, m33)
    n, nh = blk.n, blk.nh
    assert nh == n_half and n == 2 * n_half - 1
    rng = np.random.default_rng(n_half)
    worst = {"compress": 0.0, "expand": 0.0, "round trip": 0.0}
    for m in COLUMNS:
        label = f"n_half = {n_half}, m = {m}"
        # compress of arbitrary complex columns
        X = gr.crandn(rng, n, m)
        got = blk.run("dftk_mi_gamma_compress", X, nh, label)
        err = np.abs(got.astype(CLD) - gr.compress(X, g, mg))
        r = worst_ratio(err, gr.compress_bound(X, g, mg))
        worst["compress"] = max(worst["compress"], r)
        assert r <= 1.0, f"{label}: compress err / bound = {r:.3f}"
        assert np.all(got[0].imag == 0), f"{label}: Im of row 0 after compress"
        # expand of a generic half block, Im h_0 != 0 on purpose
        h = gr.crandn(rng, nh, m)
        assert np.all(h[0].imag != 0)
        x = blk.run("dftk_mi_gamma_expand", h, n, label)
        r = worst_ratio(np.abs(x.astype(CLD) - gr.expand(h, g, mg, n)), gr.expand_bound(h, g, mg, n))
        worst["expand"] = max(worst["expand"], r)
        assert r <= 1.0, f"{label}: expand err / bound = {r:.3f}"
        assert np.array_equal(x[0].real, h[0].real) and np.all(x[0].imag == 0), f"{label}: row G = 0 after expand"
        # expand . compress on real-symmetric columns
        S = gr.symmetric_columns(rng, g, mg, n, m)
        back = blk.run("dftk_mi_gamma_expand", blk.run("dftk_mi_gamma_compress", S, nh, label), n, label)
        cb = gr.compress_bound(S, g, mg)
        both = gr.expand_bound(gr.compress(S, g, mg), g, mg, n)
        both[g] += cb
        both[mg[1:]] += cb[1:]
        r = worst_ratio(np.abs(back.astype(CLD) - S.astype(CLD)), both)
        worst["round trip"] = max(worst["round trip"], r)
        assert r <= 1.0, f"{label}: round trip err / bound = {r:.3f}"
    print(f"\n[format] n_half = {n_half}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    # m = 0: status 0, nothing written
    for entry, rows_in, rows_out in (("dftk_mi_gamma_compress", n, nh), ("dftk_mi_gamma_compress_aligned", n, nh),
                                     ("dftk_mi_gamma_expand", nh, n)):
        blk.run(entry, gr.crandn(rng, rows_in, 1), rows_out, f"n_half = {n_half}, m = 0", m=0)


@pytest.mark.parametrize("n_half", NHALF)
def test_compress_aligned_against_its_definition(lib, cube33, n_half):
    m33, g, mg = sphere33(n_half)
    blk = HalfBlock(lib, cube33, CUBE, m33)
    n, nh = blk.n, blk.nh
    rng = np.random.default_rng(50 + n_half)
    worst, bad, tight = (0.0, ""), [], 0.0
    for m in COLUMNS:
        X = gr.aligned_input(rng, g, mg, n, gr.two_theta(rng, m))
        s, S = gr.pair_sum(X, g, mg)
        assert np.all(np.abs(s) >= 0.5 * S), "the input leaves 1 / |s| badly conditioned"
        assert np.all(np.pi - np.abs(np.arctan2(s.imag, s.real)) >= 0.3), "arg s too close to the branch cut of atan2"
        got = blk.run("dftk_mi_gamma_compress_aligned", X, nh, f"n_half = {n_half}, m = {m}")
        ref = gr.compress_aligned(X, g, mg)
        err, e64 = col_rel(got, ref), col_rel(gr.compress_aligned(X, g, mg, dtype=np.float64), ref)
        for c in range(m):
            tight = max(tight, err[c] / (FACTOR * max(e64[c], EPS)))
            if err[c] / max(e64[c], 1e-300) > worst[0]:
                worst = (err[c] / max(e64[c], 1e-300), f"m = {m}, column {c}: err {err[c]:.3e}, e64 {e64[c]:.3e}")
            if not err[c] <= FACTOR * max(e64[c], EPS):
                bad.append(f"n_half = {n_half}, m = {m}, column {c}: err {err[c]:.3e} > {FACTOR} max(e64 = {e64[c]:.3e}, {EPS})")
    print(f"\n[aligned] n_half = {n_half}: worst err / bound = {tight:.4f}, worst err / e64 = {worst[0]:.2f} ({worst[1]})")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n_half", NHALF)
def test_compress_aligned_exact_branches(lib, cube33, n_half):
    """One 3-column call: a zero column (s == 0), a real-symmetric one (ti == 0, tr > 0), i times a real-symmetric one
    (ti == 0, tr < 0: phi = pi / 2)."""
    m33, g, mg = sphere33(n_half)
    blk = HalfBlock(lib, cube33, CUBE, m33)
    n, nh = blk.n, blk.nh
    rng = np.random.default_rng(90 + n_half)
    S = gr.symmetric_columns(rng, g, mg, n, 2)
    X = np.stack([np.zeros(n, dtype=complex), S[:, 0], 1j * S[:, 1]], axis=1)
    assert np.array_equal(X[:, 2].real, -S[:, 1].imag) and np.array_equal(X[:, 2].imag, S[:, 1].real)
    label = f"n_half = {n_half}, branches"
    got = blk.run("dftk_mi_gamma_compress_aligned", X, nh, label)
    plain = blk.run("dftk_mi_gamma_compress", S, nh, label)
    assert not got[:, 0].real.any() and not got[:, 0].imag.any(), f"{label}: the zero column"
    assert got[:, 1].tobytes() == plain[:, 0].tobytes(), f"{label}: a real-symmetric column is not compressed bit for bit"
    ref = gr.compress(S[:, 1:], g, mg)[:, 0]
    bound = gr.compress_bound(S[:, 1:], g, mg)[:, 0] + LD(U) * LD(np.linalg.norm(S[:, 1]))
    r = min(worst_ratio(np.abs(got[:, 2].astype(CLD) - ref), bound), worst_ratio(np.abs(got[:, 2].astype(CLD) + ref), bound))
    print(f"\n[branches] n_half = {n_half}: i * real column, err / bound = {r:.3f}")
    assert r <= 1.0, f"{label}: i times a real field is not +- its plain compression: err / bound = {r:.3f}"
    assert np.all(got[0].imag == 0)


# ------------------------------------------------------------------------------------------ 3. H in the half format
H_CUBES = [(5, 5, 5), (7, 8, 9), (12, 9, 10), (16, 15, 18)]
COL_START = [0, 4, 4, 13]            # three "atoms" of 4, 0 and 9 projector columns
N_P = 13
DEFAULT_FFT_BATCH = 32               # dftk_mi_basis_create
BAND_RUNS = [(None, 1), (None, 2), (None, 3), (None, 2 * DEFAULT_FFT_BATCH + 1), (1, 2), (1, 3)]     # (fft batch, bands)
NB_MAX = 2 * DEFAULT_FFT_BATCH + 1


def h_spheres(dims):
    nx, ny, nz = dims
    rng = np.random.default_rng(sum(dims))
    loose = np.union1d([0], synthetic_sphere(nx, ny, nz, 2, 1, rng, inversion=True))
    out = [("sparse", gr.pair_sphere(dims, min(24, (len(loose) + 1) // 2), rng, pool=loose)),
           ("fullest", gr.below_nyquist(dims))]
    if dims == (5, 5, 5):
        assert np.array_equal(out[1][1], synthetic_sphere(nx, ny, nz, 1, 0, rng, full=True))
        out.append(("{0}", np.zeros(1, dtype=np.int64)))
    assert 10 <= (len(out[0][1]) + 1) // 2 < 100
    return out


class HCase:
    """One sphere with V, kin, P, D bound, and the references of all NB_MAX bands: long double per part (the parts add),
    the float64 twin per ``which``."""

    def __init__(self, lib, bs, dims, mapping, rng):
        nx, ny, nz = dims
        self.sp = sp = Sphere(dims, mapping)
        self.kin = 0.25 + gr.even_kinetic(dims, mapping)
        self.blk = blk = HalfBlock(lib, bs, dims, mapping, self.kin)
        g, mg, n = blk.g, blk.mg, blk.n
        assert np.array_equal(self.kin[g], self.kin[mg])
        self.V = V = rng.standard_normal((nz, ny, nx))
        self.P = gr.symmetrise_projectors(gr.crandn(rng, n, N_P), g, mg)
        self.D = gr.banded_D(rng, COL_START, (1, 0, 2))
        blk.kb.set_potential(V)
        blk.kb.set_projectors(self.P, self.D)
        self.h = gr.half_columns(rng, blk.nh, NB_MAX)
        args = (self.kin, self.P, self.D)
        self.part = {b: gr.apply_H(self.h, g, mg, n, b, lambda c: sp.local(V, c), *args) for b in (1, 2, 4)}
        self.twin = {w: gr.apply_H(self.h, g, mg, n, w, lambda c: sp.local64(V, c), *args, dtype=np.float64)
                     for w in range(1, 8)}

    def ref(self, which):
        return sum(self.part[b] for b in (1, 2, 4) if which & b)

    def call(self, which, nb, label):
        """bands 0 .. nb-1; one spare column on both sides: NaN behind psi, the sentinel behind H psi"""
        blk = self.blk
        ld = blk.nh + PAD
        src = in_buffer(self.h[:, :nb], ld, spare=1)
        out = out_buffer(blk.nh, nb, ld, spare=1)
        check(blk.lib.dftk_mi_gamma_apply_H(blk.kb.h, which, nb, src.data_ptr(), ld, out.ptr(), ld))
        blk.bs.sync()
        got = take(out, blk.nh, nb, label)
        assert np.all(got[0].imag == 0), f"{label}: Im of row 0"
        return got


@pytest.mark.parametrize("dims", H_CUBES, ids=lambda d: "x".join(map(str, d)))
def test_apply_H_against_the_dense_long_double_operator(lib, dims):
    rng = np.random.default_rng(1000 + sum(dims))
    tallies = {w: tally(f"gamma apply_H which = {w}") for w in range(1, 8)}
    for name, mapping in h_spheres(dims):
        bs = Basis(lib, *dims)
        case = HCase(lib, bs, dims, mapping, rng)
        alone = {}
        for batch, nb in BAND_RUNS:
            if batch is not None:
                check(lib.dftk_mi_basis_set_fft_batch(bs.h, batch))
            for which in range(1, 8):
                label = f"{dims}, {name} (n_half = {case.blk.nh}), fft batch {batch or DEFAULT_FFT_BATCH}, {nb} bands, which = {which}"
                got = case.call(which, nb, label)
                tallies[which].add(label, got, case.twin[which][:, :nb], case.ref(which)[:, :nb])
                # bands (0, 1) alone and as the first pair of three: the same bits (see the module docstring)
                if which <= 3 and nb == 2:
                    alone[batch, which] = got
                if which <= 3 and nb == 3:
                    assert got[:, :2].tobytes() == alone[batch, which].tobytes(), f"{label}: the first pair differs from the 2-band call"
    for w in range(1, 8):
        tallies[w].finish()


# ------------------------------------------------------------------------------------------ 4. half-format projectors
def test_projectors_accepted_and_refused(lib, cube33):
    n_half, nb = 513, 3
    m33, g, mg = sphere33(n_half)
    blk = HalfBlock(lib, cube33, CUBE, m33)
    n, nh = blk.n, blk.nh
    assert -(-nh // 256) == 3
    rng = np.random.default_rng(513)
    P = gr.symmetrise_projectors(gr.crandn(rng, n, N_P), g, mg)
    D = gr.banded_D(rng, COL_START, (1, 0, 2))
    h = gr.half_columns(rng, nh, nb)
    ref = gr.apply_H(h, g, mg, n, 4, None, None, P, D)
    twin = gr.apply_H(h, g, mg, n, 4, None, None, P, D, dtype=np.float64)
    top = np.abs(P).max()
    ld = nh + PAD
    t = tally("gamma projectors")

    def apply(Pdev, label):
        blk.kb.set_projectors(Pdev, D)
        src = in_buffer(h, ld, spare=1)
        out = out_buffer(nh, nb, ld, spare=1)
        st = lib.dftk_mi_gamma_apply_H(blk.kb.h, 4, nb, src.data_ptr(), ld, out.ptr(), ld)
        blk.bs.sync()
        return st, out

    def accepted(Pdev, label):
        st, out = apply(Pdev, label)
        assert st == 0, (label, lib.dftk_mi_last_error())
        got = take(out, nh, nb, label)
        assert np.all(got[0].imag == 0)
        t.add(label, got, twin, ref)

    def perturbed(row, col, delta):
        Q = P.copy()
        Q[row, col] += delta
        return Q

    last = (mg[-1], N_P - 1)          # the partner entry of the last pair of the last column: third workgroup
    accepted(P, "symmetric P")
    accepted(perturbed(*last, 1e-13 * top), "partner entry off by 1e-13 max|P|")
    nan_partner, nan_rep = P.copy(), P.copy()
    nan_partner[mg[300], 5] = float("nan")          # second workgroup; only the asymmetry measure sees it
    nan_rep[g[300], 5] = float("nan")
    refused = [("partner entry off by 1e-8 max|P|", perturbed(*last, 1e-8 * top)),
               ("Im P[0, c] = 1e-8 max|P|", perturbed(0, 7, 1e-8j * top)),
               ("NaN in a partner row", nan_partner), ("NaN in a representative row", nan_rep)]
    for label, Q in refused:
        st, out = apply(Q, label)
        assert st == EINVAL and b"real-symmetric" in lib.dftk_mi_last_error(), (label, st, lib.dftk_mi_last_error())
        accepted(P, f"symmetric P bound again after: {label}")
    t.finish()
