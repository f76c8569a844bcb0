"""REAL `UPPER` 'C' products (the Gram matrices of the Cholesky-QR chain) at the ABI, on the sizes where a tile that the
diagonal crosses is partial (n = 1, 63), exactly one tile (64, 128), straddles two row panels (65, 127, 129, 192, 259) or meets
the shifted last tile row / column and the compact live-tile launch (503, 1006), for k = 1 000 and 4 099 complex rows (the
second one odd: the last k-chunk and its last k-tile are ragged).

What is checked, per (n, k) and once more with a leading dimension larger than n:
  * flag against no flag: every entry with i <= j equals the unflagged REAL product of the same operands BIT FOR BIT, on the
    same device.  The unflagged launch shares the kernel but neither the live-tile grid nor the tile test of the reduce
    pass, so this measures the flag.  n = 1006 is the one size where the two launches cut k into different chunks (7
    against 4; asserted: no other size may take this branch), so their results can only agree to twice the absolute
    bound.  There the flagged result is compared bit for bit with something that does not depend on the unflagged plan
    of that shape: the sum, in the reduce pass's order, of the unflagged products over each of the flagged launch's own
    chunks, each from a launch wide enough never to split k (`chunk_sum`);
  * entries below the diagonal are either untouched (NaN from the fill) or, inside a live tile, the unflagged value;
  * the padding rows of a wider leading dimension and two sentinel areas around the output come back unchanged;
  * absolute: the upper triangle against a long-double product to 64 max(e_np, 2.2e-16) relative (the bound of
    tests/test_gpu_fft_axes.py), e_np = the error of the fp64 NumPy product against the same reference.

NumPy multiplies long doubles at ~0.2 GFlop/s (no BLAS), and the full upper triangle of the widest case would take a
minute.  The reference is therefore computed ONCE per k, for the widest operands -- the narrower cases use its leading
columns, their operands being leading columns -- and on ROWS sampled so that every tile of every launch is hit in each of
its four 32-row wave groups: rows 128 p + 32 w + {0, 15, 31} of every row panel p, and the last three rows (the shifted
last tile row).  Every column j >= i of such a row is compared.  The bit-for-bit comparison above covers every entry.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check, cplx  # noqa: E402

GEMM_UPPER, GEMM_REAL = 1, 8
SIZES = [1, 63, 64, 65, 127, 128, 129, 192, 259, 503, 1006]
KS = [1000, 4099]
NMAX = max(SIZES)
BLK = 128
LD = np.longdouble


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def handle(lib):
    h = C.c_void_p()
    check(lib.dftk_mi_basis_create(8, 8, 8, 1.0, 0, C.byref(h)))
    yield h
    lib.dftk_mi_basis_destroy(h)


_operands = {}


def operands(k):
    """(A, B) as k x NMAX complex blocks (host) and their device copies (column-major: one column per torch row)."""
    if k not in _operands:
        rng = np.random.default_rng(k)
        A = rng.standard_normal((k, NMAX)) + 1j * rng.standard_normal((k, NMAX))
        B = rng.standard_normal((k, NMAX)) + 1j * rng.standard_normal((k, NMAX))
        _operands[k] = (A, B, torch.from_numpy(np.ascontiguousarray(A.T)).cuda(),
                        torch.from_numpy(np.ascontiguousarray(B.T)).cuda())
    return _operands[k]


ROWS = np.array(sorted({128 * p + 32 * w + o for p in range((NMAX + 127) // 128) for w in range(4) for o in (0, 15, 31)
                        if 128 * p + 32 * w + o < NMAX} | {NMAX - 3, NMAX - 2, NMAX - 1}))

_reference = {}


def reference(k):
    """(ref, e_np): rows ROWS of Re(A^H B) = Ar'Br + Ai'Bi in long double (summed over k in slabs that stay in cache), and
    the relative error of the fp64 NumPy product on the entries j >= i of those rows."""
    if k not in _reference:
        A, B, _, _ = operands(k)
        S64 = np.ascontiguousarray(np.concatenate([A.real, A.imag])[:, ROWS].T)       # len(ROWS) x 2k
        T64 = np.concatenate([B.real, B.imag])                                        # 2k x NMAX
        S, T = S64.astype(LD), T64.astype(LD)
        ref = np.zeros((len(ROWS), NMAX), dtype=LD)
        for c0 in range(0, 2 * k, 256):
            ref += np.ascontiguousarray(S[:, c0:c0 + 256]) @ T[c0:c0 + 256]
        upper = np.arange(NMAX)[None, :] >= ROWS[:, None]
        d = ((S64 @ T64).astype(LD) - ref)[upper]
        _reference[k] = (ref, float(np.sqrt(np.sum(d * d) / np.sum(ref[upper] ** 2))))
    return _reference[k]


def run(lib, h, n, k, ldc, flags):
    """C (ldc x n, NaN-filled, between two sentinel areas) = Re(A[:, :n]^H B[:, :n]) with `flags`; returns the n x n result,
    the padding rows and the two sentinel areas as they came back."""
    _, _, Ad, Bd = operands(k)
    guard = 4096
    buf = torch.full((guard + ldc * n + guard,), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
    buf[:guard] = 1.25 - 2.5j
    buf[guard + ldc * n:] = -3.5 + 0.75j
    out = buf[guard:guard + ldc * n]
    check(lib.dftk_mi_zgemm_ex(h, b"C", n, n, k, cplx(1.0), Ad.data_ptr(), k, Bd.data_ptr(), k, cplx(0.0),
                               out.data_ptr(), ldc, flags))
    check(lib.dftk_mi_basis_sync(h))
    host = buf.cpu().numpy()
    Cm = host[guard:guard + ldc * n].reshape(n, ldc).T          # Cm[i, j]
    return Cm[:n, :], Cm[n:, :], host[:guard], host[guard + ldc * n:]


def same_k_chunks(lib, n, k):
    """Do the flagged and the unflagged product sum every entry over the same k chunks?  (dftk_mi_zgemm_plan_host: split
    count and chunk length of the interior and of the border launch.)  True for every size here but n = 1006, where the
    72 live tiles of the flagged launch take 7 chunks and the 128 tiles of the full one 4."""
    plans = []
    for flags in (GEMM_REAL, GEMM_REAL | GEMM_UPPER):
        out = (C.c_int * 12)()
        check(lib.dftk_mi_zgemm_plan_host(b"C", n, n, k, flags, out))
        plans.append((out[5], out[6], out[8], out[9]))
    return plans[0] == plans[1]


def chunk_sum(lib, h, k, n):
    """What the flagged launch must store where it cuts k into other chunks than the unflagged one: for every chunk z of ITS
    plan the unflagged REAL product over that chunk alone, summed over z in order from 0.0 as the reduce pass does.  The
    chunk products must come from launches that do not split k themselves, whatever the plan of the n x n product is: the
    operands are repeated side by side to 2 n x 2048 columns, 16 x 32 = 512 tiles -- as many as workgroups are resident, the
    size from which the plan never splits (asserted).  An entry's k order does not depend on where its tile sits."""
    _, _, Ad, Bd = operands(k)
    out = (C.c_int * 12)()
    check(lib.dftk_mi_zgemm_plan_host(b"C", n, n, k, GEMM_REAL | GEMM_UPPER, out))
    ns, kc = out[5], out[6]
    assert ns > 1 and out[3] == 0 and out[4] == 0            # split interior launch, no border launch
    m2, n2 = 2 * n, 2048
    A2 = torch.cat([Ad[:n], Ad[:n]]).contiguous()            # column-major k x 2 n
    B2 = torch.cat([Bd[:n], Bd[:n], Bd[:n]])[:n2].contiguous()
    total = np.zeros((n, n))
    for z in range(ns):
        k0, kz = z * kc, min(kc, k - z * kc)
        check(lib.dftk_mi_zgemm_plan_host(b"C", m2, n2, kz, GEMM_REAL, out))
        assert out[5] == 1 and out[3] == 0 and out[4] == 0, "the chunk product must not split k itself"
        Cz = torch.full((n2, m2), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
        check(lib.dftk_mi_zgemm_ex(h, b"C", m2, n2, kz, cplx(1.0), A2.data_ptr() + 16 * k0, k, B2.data_ptr() + 16 * k0, k,
                                   cplx(0.0), Cz.data_ptr(), m2, GEMM_REAL))
        check(lib.dftk_mi_basis_sync(h))
        part = Cz[:n, :n].cpu().numpy().T
        assert not part.imag.any()
        total = total + part.real
    return total


CASES = [(n, k, n) for k in KS for n in SIZES] + [(259, 4099, 259 + 37), (503, 1000, 512)]


@pytest.mark.parametrize("n,k,ldc", CASES)
def test_real_upper_gram_equals_the_unflagged_product(lib, handle, n, k, ldc):
    full, pad_f, g0_f, g1_f = run(lib, handle, n, k, ldc, GEMM_REAL)
    up, pad, g0, g1 = run(lib, handle, n, k, ldc, GEMM_REAL | GEMM_UPPER)
    for g, want in ((g0, 1.25 - 2.5j), (g1, -3.5 + 0.75j), (g0_f, 1.25 - 2.5j), (g1_f, -3.5 + 0.75j)):
        assert np.all(g == want), "sentinel area overwritten"
    assert np.all(np.isnan(pad.real)) and np.all(np.isnan(pad.imag)) and np.all(np.isnan(pad_f.real)) \
        and np.all(np.isnan(pad_f.imag)), "padding rows written"
    assert np.all(np.isfinite(full.real)) and not full.imag.any()
    ref, e_np = reference(k)
    bound = 64.0 * max(e_np, 2.2e-16)
    iu = np.triu_indices(n)
    il = np.tril_indices(n, -1)
    lower = up[il]
    untouched = np.isnan(lower.real) | np.isnan(lower.imag)      # (a written entry is finite in both parts)
    same = same_k_chunks(lib, n, k)
    assert same == (n != 1006), "the sizes whose two launches share their k chunks are pinned: every one but n = 1006"
    if same:
        assert np.array_equal(up[iu], full[iu]), "an entry at or above the diagonal differs from the unflagged product"
        assert np.all(untouched | (lower == full[il])), "an entry below the diagonal is neither untouched nor the product"
    else:
        # n = 1006: the two launches cut k into different chunks (the plan fills the chip with the tiles each of them runs), so
        # their sums differ in the order of the chunk partials: both lie within `bound` of the exact product, hence within
        # 2 bound of each other ...
        d = np.linalg.norm(up[iu] - full[iu]) / np.linalg.norm(full[iu])
        print(f"n={n} k={k}: different k chunks with and without the flag, relative difference {d:.3e}")
        assert d <= 2.0 * bound
        # ... and BIT FOR BIT the flagged result is the fixed-order sum of its own chunks' unflagged products
        emu = chunk_sum(lib, handle, k, n)
        assert np.array_equal(up[iu].real, emu[iu]) and not up[iu].imag.any(), \
            "an entry at or above the diagonal differs from the sum of the unflagged products of the flagged launch's k chunks"
        assert np.all(untouched | (lower.real == emu[il])), "an entry below the diagonal is neither untouched nor that sum"
    # absolute accuracy of the upper triangle
    rows = ROWS[ROWS < n]
    sel = np.arange(n)[None, :] >= rows[:, None]
    r = ref[:len(rows), :n][sel]
    got = up.real[rows, :].astype(LD)[sel]
    err = float(np.sqrt(np.sum((got - r) ** 2) / np.sum(r * r)))
    print(f"n={n} k={k} ldc={ldc}: error against long double {err:.3e} (NumPy fp64 {e_np:.3e}, bound {bound:.3e})")
    assert err <= bound
