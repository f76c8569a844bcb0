"""``dftk_mi_diff_dots`` (csrc/potmix_kernels.hip) at the C ABI: out[p] = sum_i (a_p[i] - b_p[i]) (c_p[i] - d_p[i]).

Reference: the same sums in ``numpy.longdouble`` (64-bit mantissa, pairwise ``np.sum``), written here.

Bound, from the operation count of the reduction.  Every operand difference is one rounding (none where b / d is null), the
product at most one (none where the compiler contracts it into the accumulation), so a term enters its accumulator with at
most 3 roundings.  It then passes through at most
    m = ceil(n / (128 * 256))   additions of the serial chain of its thread (grid-stride loop of the 128 x 256 grid),
    6                           additions of the shuffle tree of its wave,
    4                           additions of the four wave partials of its block,
    128                         additions of the host sum over the block partials,
k = m + 141 roundings in all, hence |out - exact| <= gamma_k sum_i |(a - b)(c - d)| with gamma_k = k eps / (1 - k eps).  The
reference's own error is below 40 eps_ld of the same sum (two differences, a product and a pairwise sum of at most 2^17 terms
in long double), which is added.  The achieved fraction of the bound is printed (``pytest -s``).

Every operand lives inside a buffer with NaN on both sides of it (5 doubles before, 7 after: the pointers are 8-byte aligned
only), so that a read outside [0, n) turns the result into NaN.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402

from test_gpu_kernels import Basis  # noqa: E402

EPS = 2.220446049250313e-16
EINVAL = -1               # DFTK_MI_EINVAL (include/dftk_mi355x.h)
LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
GRID = 128 * 256
SIZES = [1, 255, 256, 257, GRID - 1, GRID, GRID + 1, 2 * 9 ** 3]
PAD_L, PAD_R = 5, 7


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert EPS_LD < 1.1e-19, "the reference needs the 80-bit long double"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs(lib):
    return Basis(lib, 8, 8, 8)


class Guarded:
    """a host array and its device copy between two NaN fences"""

    def __init__(self, host):
        self.host = np.ascontiguousarray(host, dtype=np.float64)
        buf = np.full(PAD_L + len(self.host) + PAD_R, np.nan)
        buf[PAD_L:PAD_L + len(self.host)] = self.host
        self.buf = torch.from_numpy(buf).cuda()
        self.ptr = self.buf.data_ptr() + 8 * PAD_L


def mixed(rng, n):
    """magnitudes from 1e-8 to 1e8, both signs"""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, 8, n) * rng.uniform(1.0, 2.0, n)


def table(ops):
    return (C.c_void_p * len(ops))(*[(o.ptr if o is not None else None) for o in ops])


def call(lib, bs, n, pairs, handle=True, fill=math.nan):
    out = (C.c_double * 8)(*([fill] * 8))
    st = lib.dftk_mi_diff_dots(bs.h if handle else None, n, len(pairs), *[table([q[j] for q in pairs]) for j in range(4)], out)
    return st, list(out)


def reference(pairs):
    """(sum, sum of |terms|) per pair in long double"""
    out = []
    for a, b, c, d in pairs:
        left = a.host.astype(LD) - (b.host.astype(LD) if b is not None else LD(0))
        right = c.host.astype(LD) - (d.host.astype(LD) if d is not None else LD(0))
        out.append((np.sum(left * right), np.sum(np.abs(left * right))))
    return out


def check_against_reference(lib, bs, n, pairs, label):
    st, out = call(lib, bs, n, pairs)
    assert st == 0
    k = math.ceil(n / GRID) + 141
    gamma = k * EPS / (1 - k * EPS)
    worst = 0.0
    for p, (ref, mag) in enumerate(reference(pairs)):
        err = abs(float(LD(out[p]) - ref))
        bound = (gamma + 40 * EPS_LD) * float(mag)
        assert math.isfinite(out[p]), (label, p)
        assert err <= bound, (label, p, err, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    assert all(math.isnan(v) for v in out[len(pairs):])               # nothing behind n_pairs is written
    print(f"\ndiff_dots {label} n={n} pairs={len(pairs)}: worst err / bound = {worst:.3f} (k = {k})")
    return out


def operand_pool(rng, n, count=6):
    return [Guarded(mixed(rng, n)) for _ in range(count)]


def make_pairs(rng, pool, n_pairs):
    """pairs over a small pool: pointers repeat within and across pairs, b / d are null in every combination, pair 0 is a
    squared norm of a difference and the last pair one of a plain array"""
    pairs = []
    for p in range(n_pairs):
        a, b, c, d = (pool[i] for i in rng.integers(0, len(pool), 4))
        if p % 4 == 1:
            b = None
        elif p % 4 == 2:
            d = None
        elif p % 4 == 3:
            b = d = None
        pairs.append((a, b, c, d))
    pairs[0] = (pool[0], pool[1], pool[0], pool[1])
    if n_pairs > 1:
        pairs[-1] = (pool[2], None, pool[2], None)
    return pairs


@pytest.mark.parametrize("n_pairs", [1, 5, 8])
@pytest.mark.parametrize("n", SIZES)
def test_diff_dots_against_longdouble(lib, bs, n, n_pairs):
    rng = np.random.default_rng(100 * n + n_pairs)
    pool = operand_pool(rng, n)
    check_against_reference(lib, bs, n, make_pairs(rng, pool, n_pairs), "mixed magnitudes")


@pytest.mark.parametrize("n", [257, GRID + 1])
def test_diff_dots_cancelling_differences(lib, bs, n):
    """the shape of the driver's call: differences that are 1e-9 of their operands, drho in four of the five pairs"""
    rng = np.random.default_rng(n)
    Vin, rho = Guarded(1e2 * rng.standard_normal(n)), Guarded(1.0 + rng.uniform(0, 1, n))
    Vout = Guarded(Vin.host + 1e-7 * rng.standard_normal(n))
    Vnext = Guarded(Vin.host + 1e-7 * rng.standard_normal(n))
    rho_next = Guarded(rho.host + 1e-9 * rng.standard_normal(n))
    Vout_next = Guarded(Vout.host + 1e-7 * rng.standard_normal(n))
    P = Guarded(1e-7 * rng.standard_normal(n))
    pairs = [(Vout, Vin, rho_next, rho), (Vnext, Vin, rho_next, rho), (rho_next, rho, Vout_next, Vout), (P, None, P, None),
             (rho_next, rho, rho_next, rho)]
    out = check_against_reference(lib, bs, n, pairs, "driver call")
    assert out[3] > 0 and out[4] > 0


def test_diff_dots_nullable_positions(lib, bs):
    """b / d null per entry in every combination, and as whole tables"""
    n = 1000
    rng = np.random.default_rng(7)
    a, b, c, d = operand_pool(rng, n, 4)
    for bb in (b, None):
        for dd in (d, None):
            check_against_reference(lib, bs, n, [(a, bb, c, dd)], f"null b={bb is None} d={dd is None}")
    ref = reference([(a, None, c, None), (c, None, a, None)])
    for tables in ((table([a, c]), None, table([c, a]), None), (table([a, c]), table([None, None]), table([c, a]), None)):
        out = (C.c_double * 2)(math.nan, math.nan)
        assert lib.dftk_mi_diff_dots(bs.h, n, 2, *tables, out) == 0
        for p in range(2):
            assert abs(float(LD(out[p]) - ref[p][0])) <= 142 * EPS * float(ref[p][1])
        assert out[0] == out[1]                     # the product commutes bit for bit


def test_diff_dots_repeated_pointers(lib, bs):
    """an operand that repeats an earlier one is copied, not read again: the results equal those of distinct copies bit for
    bit, whatever the position of the repeat"""
    n = GRID + 77
    rng = np.random.default_rng(11)
    x, y, z = operand_pool(rng, n, 3)
    x2, y2 = Guarded(x.host), Guarded(y.host)
    shared = [(x, y, z, None), (z, None, x, y), (x, y, x, y), (y, x, x, y), (x, None, x, y)]
    copies = [(x, y, z, None), (z, None, x2, y2), (x2, y2, x, y), (y, x, x2, y2), (x2, None, x, y2)]
    out_s = check_against_reference(lib, bs, n, shared, "repeated pointers")
    st, out_c = call(lib, bs, n, copies)
    assert st == 0 and out_s[:5] == out_c[:5]
    assert out_s[0] == out_s[1] and out_s[2] == -out_s[3]


def counts(lib):
    a, b = C.c_int64(), C.c_int64()
    assert lib.dftk_mi_launch_count(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def test_diff_dots_one_launch_one_sync_repeatable(lib, bs):
    n = 2 * 9 ** 3
    rng = np.random.default_rng(13)
    pool = operand_pool(rng, n)
    pairs = make_pairs(rng, pool, 5)
    bs.sync()
    l0, s0 = counts(lib)
    st, first = call(lib, bs, n, pairs)
    l1, s1 = counts(lib)
    assert st == 0 and (l1 - l0, s1 - s0) == (1, 1)
    for _ in range(3):
        st, again = call(lib, bs, n, pairs)
        assert st == 0 and again[:5] == first[:5]


def test_diff_dots_error_returns(lib, bs):
    n = 300
    rng = np.random.default_rng(17)
    a, b, c, d = operand_pool(rng, n, 4)
    good = [(a, b, c, d), (c, None, a, None)]
    sentinel = 12345.678

    def untouched(st_out):
        st, out = st_out
        return st == EINVAL and all(v == sentinel for v in out)
    assert untouched(call(lib, bs, n, good, handle=False, fill=sentinel))
    assert untouched(call(lib, bs, 0, good, fill=sentinel))
    assert untouched(call(lib, bs, -5, good, fill=sentinel))
    assert untouched(call(lib, bs, n, [(None, b, c, d)], fill=sentinel))
    assert untouched(call(lib, bs, n, [(a, b, None, d)], fill=sentinel))
    assert untouched(call(lib, bs, n, good + [(a, b, None, None)], fill=sentinel))
    tabs = [table([q[j] for q in good]) for j in range(4)]
    for n_pairs in (0, -1, 9):
        out = (C.c_double * 8)(*([sentinel] * 8))
        assert lib.dftk_mi_diff_dots(bs.h, n, n_pairs, *tabs, out) == EINVAL and all(v == sentinel for v in out)
    out = (C.c_double * 8)(*([sentinel] * 8))
    assert lib.dftk_mi_diff_dots(bs.h, n, 2, None, tabs[1], tabs[2], tabs[3], out) == EINVAL
    assert lib.dftk_mi_diff_dots(bs.h, n, 2, tabs[0], tabs[1], None, tabs[3], out) == EINVAL
    assert all(v == sentinel for v in out)
    assert lib.dftk_mi_diff_dots(bs.h, n, 2, *tabs, None) == EINVAL
    # and the call still works afterwards
    st, out = call(lib, bs, n, good)
    assert st == 0 and all(math.isfinite(v) for v in out[:2])
