"""The batched kernels of dftk.jl_amd/csrc/batch_kernels.hip, operation by operation, against high-precision references.

``dftk_mi_batch_replay`` runs a table of device operations as the fibers of one batched call: every row goes through the
internal entry point the LOBPCG drivers call, is recorded, merged position by position with the rows of the other fibers
and executed by ONE launch per kind (``batch_exec_group``).  ``test_gpu_kbatch.py`` sees these kernels only through a
whole LOBPCG, which converges past a wrong product; here each kernel is compared with NumPy in ``longdouble``.

Rules of every case: buffers have ``ld`` > rows and one column more than the operation uses, all of it NaN-poisoned, and
what the contract leaves alone must be bitwise unchanged afterwards; ``dftk_mi_batch_stats`` must show that the merged
path ran (``merged_launches`` > 0) and that exactly the rows sent to a fall-back on purpose ran one by one.  Cases whose
operations have a one-by-one form run a second time with ``DFTK_MI_KBATCH_SEQUENTIAL=1`` under the same bounds.

Bounds (u = 2^-53; the references are exact to ~2^-64):
  bitwise      copies, gathers, fills, sub-identity, add-diag, hermitise, conjugate-transpose, host <-> device copies
  element-wise |got - ref| <= 4 u (|a| + |lam x|) for a - lam x, <= 4 u |ref| without a subtraction: three roundings,
               fused or not
  reductions   |got - ref| <= (n + 8) u sum |terms| (for a square-rooted result: the same on its square).  The norms that
               RESIDUAL / TPA return are sums over the block the kernel has just written, so their reference is taken
               from the returned block (which has its own element-wise check)
  products     |C - C_ref| <= 4 (k + 4) u (|alpha| |op(A)|' |B| + |beta| |C0|) entrywise
  POTRF / HEEV / ORTHO: the assertions of test_potrf_trtri, test_heev and test_fused_ortho_kernel; POTRF's two norm
               estimates equal max|diag| + sqrt(sum |offdiag|^2) of the returned factor to (n^2 + 8) u.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check, cplx, dftk_mi_batch_op  # noqa: E402

from test_gpu_kernels import Basis, KBlock, make_oracle_basis  # noqa: E402

U = 2.0 ** -53
EPS = 2 * U
LD, CLD = np.longdouble, np.clongdouble
(ZGEMM, COLRED, RESIDUAL, TPA, SCALE, COPY, FILL0, SUBID, GATHER, ADDDIAG, HERMIT, CTRANS, H2D, D2H, POTRF,
 HEEV) = range(16)
APPLYD, ORTHO = 18, 19
UPPER, B_UPPER, REAL = 1, 2, 8
NUM_NONFINITE, NUM_CHOLESKY = 1, 2
NANC = complex(np.nan, np.nan)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs(lib):
    return Basis(lib, 8, 8, 8)


@pytest.fixture(params=["merged", "one-by-one"])
def mode(request, monkeypatch):
    """The second run of a case: every recorded row through its original entry point (read per scheduling round)."""
    if request.param == "one-by-one":
        monkeypatch.setenv("DFTK_MI_KBATCH_SEQUENTIAL", "1")
    else:
        monkeypatch.delenv("DFTK_MI_KBATCH_SEQUENTIAL", raising=False)
    return request.param


@pytest.fixture
def merged(monkeypatch):
    monkeypatch.delenv("DFTK_MI_KBATCH_SEQUENTIAL", raising=False)
    return "merged"


def L(a):
    a = np.asarray(a)
    return a.astype(CLD if np.iscomplexobj(a) else LD)


def block(rng, n, m):
    return rng.standard_normal((n, m)) + 1j * rng.standard_normal((n, m))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


class Mat:
    """A column-major rows x cols matrix (complex or double) inside a NaN-poisoned device buffer with ld = rows + pad and
    one column more.  ``a`` None: the window itself is poisoned as well (an output that must not be read)."""

    def __init__(self, a=None, shape=None, dtype=np.complex128, pad=3):
        if a is not None:
            a = np.asarray(a)
            a = a[:, None] if a.ndim == 1 else a
            shape, dtype = a.shape, a.dtype
        self.rows, self.cols = shape
        self.ld = self.rows + pad
        h = np.empty((self.cols + 1, self.ld), dtype=dtype)
        h.fill(NANC if np.iscomplexobj(h) else np.nan)
        if a is not None:
            h[:self.cols, :self.rows] = a.T
        self.before = h
        self.t = torch.from_numpy(h.copy()).cuda()
        self.ptr = self.t.data_ptr()

    def fetch(self):
        self.after = self.t.cpu().numpy()
        return self.after[:self.cols, :self.rows].T.copy()

    def rest_untouched(self, written=None):
        """Padding rows, the extra column and the unwritten part of the window (``written``: rows x cols mask, default
        all) are bitwise what they were."""
        keep = np.ones(self.before.shape, dtype=bool)
        w = np.ones((self.rows, self.cols), dtype=bool) if written is None else np.broadcast_to(written, (self.rows, self.cols))
        keep[:self.cols, :self.rows] = ~w.T
        a = bits(self.after).reshape(self.before.shape + (-1,))
        b = bits(self.before).reshape(self.before.shape + (-1,))
        return np.array_equal(a[keep], b[keep])


def stats(lib):
    v = [C.c_int64() for _ in range(4)]
    check(lib.dftk_mi_batch_stats(*[C.byref(x) for x in v]))
    return dict(zip(("rounds", "ops", "merged_launches", "sequential_ops"), (x.value for x in v)))


class Table:
    def __init__(self, n_fibers):
        self.n_fibers, self.rows, self.keep = n_fibers, [], []

    def add(self, typ, fiber, **kw):
        r = dftk_mi_batch_op()
        r.type, r.fiber = typ, fiber
        for k, v in kw.items():
            if isinstance(v, Mat):
                self.keep.append(v)
                v = v.ptr
            elif isinstance(v, torch.Tensor):
                self.keep.append(v)
                v = v.data_ptr()
            elif isinstance(v, np.ndarray):
                self.keep.append(v)
                v = v.ctypes.data
            elif k in ("alpha", "beta"):
                v = cplx(v)
            elif k == "trans":
                v = ord(v)
            setattr(r, k, v)
        self.rows.append(r)
        return len(self.rows) - 1

    def call(self, lib, bs):
        self.arr = (dftk_mi_batch_op * len(self.rows))(*self.rows)
        return lib.dftk_mi_batch_replay(bs.h, self.n_fibers, len(self.rows), self.arr)

    def run(self, lib, bs, mode, fallback=0):
        """One replay call; returns the statuses of the rows.  ``fallback``: rows sent to a one-by-one group on purpose."""
        check(self.call(lib, bs))
        st = stats(lib)
        assert st["ops"] == len(self.rows), st
        if mode == "merged":
            assert st["merged_launches"] > 0 and st["sequential_ops"] == fallback, st
        else:
            assert st["merged_launches"] == 0 and st["sequential_ops"] == st["ops"], st
        return [r.status for r in self.arr]


def witness(tab, fiber):
    """A small copy that merges in any table: keeps merged_launches > 0 in the cases whose other rows fall back."""
    src = Mat(np.arange(6, dtype=complex).reshape(3, 2) * (1 - 2j))
    dst = Mat(shape=(3, 2))
    tab.add(COPY, fiber, n=3, m=2, A=src, lda=src.ld, C=dst, ldc=dst.ld)

    def verify():
        assert same_bits(dst.fetch(), src.fetch()) and dst.rest_untouched()
    return verify


# ------------------------------------------------------------------------------------------------- products
@functools.lru_cache(maxsize=None)
def gemm_ref(trans, m, n, k, flags, alpha, beta, seed):
    """Operands and the longdouble reference of one product (computed once, shared by both runs of a case)."""
    rng = np.random.default_rng(seed)
    A = block(rng, k, m) if trans == "C" else block(rng, m, k)
    B = block(rng, k, n)
    C0 = block(rng, m, n) if beta != 0 else None
    opA = A.conj().T if trans == "C" else A
    Bm = np.triu(B) if flags & B_UPPER else B
    if flags & REAL and trans == "N":
        Bm = Bm.real + 0j
    prod = L(opA) @ L(Bm)
    if flags & REAL and trans == "C":
        prod = prod.real + CLD(0)
    ref = CLD(alpha) * prod
    bound = abs(alpha) * (np.abs(opA) @ np.abs(Bm))
    if C0 is not None:
        ref = ref + CLD(beta) * L(C0)
        bound = bound + abs(beta) * np.abs(C0)
    return A, B, C0, ref, 4 * (k + 4) * U * bound


class Gemm:
    def __init__(self, tab, fiber, trans, m, n, k, flags=0, alpha=1.0, beta=0.0, seed=0, join_next=0, sync_after=0,
                 poison_B=True):
        self.trans, self.m, self.n, self.k, self.flags = trans, m, n, k, flags
        A, B, C0, self.ref, self.bound = gemm_ref(trans, m, n, k, flags, alpha, beta, seed + 1000 * fiber)
        if flags & B_UPPER:      # k_b_gemm_n never reads the strict lower triangle of B; zgemm() itself asks for zeros there
            B = B.copy()
            B[np.tril_indices(k, -1, n)] = np.nan if poison_B else 0.0
        self.A, self.B = Mat(A), Mat(B)
        self.C = Mat(C0) if C0 is not None else Mat(shape=(m, n))
        tab.add(ZGEMM, fiber, trans=trans, gm=m, gn=n, gk=k, alpha=alpha, beta=beta, A=self.A, lda=self.A.ld, B=self.B,
                ldb=self.B.ld, C=self.C, ldc=self.C.ld, flags=flags, join_next=join_next, sync_after=sync_after)

    def verify(self, mode, tile=16):
        """Returns the worst |error| / bound.  UPPER: the merged kernel computes the 16 x 16 tiles that are not strictly
        below the diagonal and leaves the others bitwise alone; the one-by-one product has wider tiles, so there the
        upper triangle is held to the bound and every other entry is either computed or untouched."""
        got = self.C.fetch()
        err = np.abs(L(got) - self.ref)
        i, j = np.indices(got.shape)
        what = (self.trans, self.m, self.n, self.k, self.flags, mode)
        if not self.flags & UPPER:
            must = np.ones(got.shape, dtype=bool)
            assert self.C.rest_untouched(), what
        elif mode == "merged":
            must = (i // tile) <= (j // tile)
            assert self.C.rest_untouched(written=must), what      # tiles strictly below the diagonal: bitwise the fill
        else:
            must = i <= j
            assert self.C.rest_untouched(), what
            same = bits(got).reshape(got.shape + (2,)) == bits(self.C.before[:self.n, :self.m].T).reshape(got.shape + (2,))
            assert np.all((err <= self.bound) | same.all(axis=-1)), what
        assert np.all(err[must] <= self.bound[must]), (what, float(np.nanmax(err[must] / self.bound[must])))
        return float(np.max(err[must] / self.bound[must]))


AL, BE = 0.7 - 0.2j, -0.3 + 0.5j


def test_products_conjugate_transposed(lib, bs, mode):
    """k_b_gemm_c and its split-K reduce: position 0 is ONE launch of ten items whose longest k (8200) sets nsplit = 32,
    so the items of k = 1 .. 257 run mostly empty chunks; position 1 is one launch with every k <= 256 (unsplit).
    UPPER at m = n = 16, 40, 96 in both; beta = 0 items have a NaN-filled C, the others complex alpha and beta."""
    split = [(1, 1, 1, 0, 1.0, 0.0), (15, 17, 63, 0, AL, BE), (16, 16, 64, UPPER, 1.0, 0.0), (17, 33, 65, 0, AL, BE),
             (33, 15, 256, 0, AL, 0.0), (96, 96, 257, UPPER, 1.0, 0.0), (40, 40, 1350, UPPER, AL, BE),
             (96, 1, 4653, 0, AL, BE), (16, 33, 8200, 0, 1.0, 0.0), (1, 96, 1350, 0, AL, BE)]
    unsplit = [(96, 96, 256, UPPER, AL, BE), (40, 40, 65, UPPER, 1.0, 0.0), (16, 16, 1, UPPER, AL, 0.0), (1, 1, 63, 0, AL, BE),
               (15, 96, 64, 0, 1.0, 0.0), (33, 17, 256, 0, AL, BE), (17, 1, 65, 0, 1.0, 0.0), (96, 15, 1, 0, AL, BE),
               (16, 33, 63, 0, AL, BE), (1, 16, 256, 0, 1.0, 0.0)]
    tab = Table(len(split))
    items = [[Gemm(tab, f, "C", *g, seed=p) for f, g in enumerate(group)] for p, group in enumerate((split, unsplit))]
    tab.run(lib, bs, mode)
    for name, group in zip(("split", "unsplit"), items):
        print(f"k_b_gemm_c {name} ({mode}): worst error / bound per item",
              np.array2string(np.array([it.verify(mode) for it in group]), precision=3))


def test_products_plain(lib, bs, mode):
    """k_b_gemm_n (one thread per row, 8 columns per workgroup, k <= 128): rows 1 .. 4653 against a grid sized by the
    longest, B_UPPER with NaN below the diagonal of B at n = k = 7, 8, 9, 24, the joined pair X = Y c, AX = AY c of the
    Rayleigh-Ritz update, and two A^H B items in the same launch group.  The one-by-one run has zeros below the diagonal of
    B instead: zgemm()'s contract is B[k][j] = 0 for k > j, and inside its last 64-column tile it does read them (as
    test_zgemm_upper_triangular_B says); the drivers pass the inv(R) of dense_potrf_trtri, which has them."""
    plain = [(1, 1, 1, 0, 1.0, 0.0), (255, 7, 7, B_UPPER, AL, BE), (256, 8, 8, B_UPPER, 1.0, 0.0), (257, 9, 9, B_UPPER, AL, BE),
             (1350, 24, 24, B_UPPER, 1.0, 0.0), (4653, 24, 128, 0, AL, BE), (257, 512, 8, 0, AL, 0.0), (1350, 9, 24, 0, AL, BE),
             (255, 1, 128, 0, 1.0, 0.0)]
    tab = Table(len(plain) + 3)
    items = [Gemm(tab, f, "N", *g, poison_B=(mode == "merged")) for f, g in enumerate(plain)]
    f = len(plain)
    items.append(Gemm(tab, f, "N", 1350, 7, 24, alpha=1.0, beta=0.0, seed=1, join_next=1))    # X = Y c
    items.append(Gemm(tab, f, "N", 1350, 7, 24, alpha=1.0, beta=0.0, seed=2))                 # AX = AY c, same launch
    items.append(Gemm(tab, f + 1, "C", 17, 24, 1350, 0, AL, BE))
    items.append(Gemm(tab, f + 2, "C", 24, 24, 257, UPPER, 1.0, 0.0))
    tab.run(lib, bs, mode)
    if mode == "merged":
        assert stats(lib)["merged_launches"] == 1      # A B and A^H B items are ONE group; the joined row rides on position 0
    print(f"k_b_gemm_n ({mode}): worst error / bound per item", np.array2string(np.array([it.verify(mode) for it in items]), precision=3))


@pytest.mark.parametrize("kind", ["m97", "real", "k129", "n513"])
def test_products_outside_the_batched_kernels(lib, bs, mode, kind):
    """One item outside a batched kernel's range sends its WHOLE launch group to the one-by-one path, which must be as
    right as the merged one: m = 97 (> 96), DFTK_MI_GEMM_REAL, k = 129 (> 128) and n = 513 (> 512) of A B."""
    tab = Table(2)
    if kind == "m97":
        items = [Gemm(tab, 0, "C", 97, 5, 300, 0, AL, BE), Gemm(tab, 1, "C", 16, 17, 300, 0, AL, BE)]
    elif kind == "real":
        items = [Gemm(tab, 0, "C", 16, 16, 300, REAL, 0.7, 0.0), Gemm(tab, 1, "C", 16, 17, 300, 0, AL, BE)]
    elif kind == "k129":
        items = [Gemm(tab, 0, "N", 300, 9, 129, 0, AL, BE), Gemm(tab, 1, "N", 257, 8, 24, 0, AL, BE)]
    else:
        items = [Gemm(tab, 0, "N", 40, 513, 8, 0, AL, 0.0), Gemm(tab, 1, "N", 257, 8, 24, 0, AL, BE)]
    wit = witness(tab, 0)
    tab.run(lib, bs, mode, fallback=2)
    print(f"fall-back {kind} ({mode}): worst error / bound", [it.verify("one-by-one") for it in items])
    if kind == "real":
        assert not items[0].C.fetch().imag.any()
    wit()


# ------------------------------------------------------------------------------------------------- column kernels
# 1024 | 1025: the last full and the first partial pass of a 256-thread workgroup with four rows per thread; 8191 | 8192 |
# 8193: the one-by-one form switches to 1024 threads from 8192 rows on, 8193 is its one-row tail
COL_SHAPES = [(1, 1), (255, 7), (256, 24), (257, 1), (1350, 7), (4653, 24), (1024, 3), (1025, 3), (8191, 2), (8192, 2),
              (8193, 3)]


@functools.lru_cache(maxsize=None)
def col_data(n, m):
    rng = np.random.default_rng(17 * n + m)
    return dict(X=block(rng, n, m), Y=block(rng, n, m), w=rng.random(n) + 0.1, kin=3.0 * rng.random(n) + 0.05,
                lam=rng.standard_normal(m), mk=rng.random(m) + 0.5, den=rng.random(m) + 0.5)


def colred_ref(mode, d):
    """(reference, sum |terms|) of k_col_reduce's modes in longdouble; mode 0 is compared on its square."""
    x, y, w = L(d["X"]), L(d["Y"]), L(d["w"])[:, None]
    if mode in (0, 3):
        t = x.real ** 2 + x.imag ** 2
        return t.sum(axis=0), t.sum(axis=0)
    if mode == 1:
        return (x.real * y.real + x.imag * y.imag).sum(axis=0), (np.abs(x.real * y.real) + np.abs(x.imag * y.imag)).sum(axis=0)
    if mode == 4:
        return (x.real * y.imag - x.imag * y.real).sum(axis=0), (np.abs(x.real * y.imag) + np.abs(x.imag * y.real)).sum(axis=0)
    t = w * (x.real ** 2 + x.imag ** 2)
    return t.sum(axis=0), t.sum(axis=0)


def sumsq(a):
    a = L(a)
    return (a.real ** 2 + a.imag ** 2).sum(axis=0)


def reduction_ok(got, ref, terms, n, squared=False):
    g = L(got) ** 2 if squared else L(got)
    err, bound = np.abs(g - ref), (n + 8) * U * terms
    assert np.all(err <= bound), (got, ref, float(np.max(err / bound)))
    return float(np.max(err / bound))


def column_table(shapes):
    """One fiber per shape: COLRED in its five modes (a different one per fiber at every position), RESIDUAL with and
    without the kinetic sums, TPA in its three forms.  Returns the table and, per fiber, its data and output buffers."""
    tab = Table(len(shapes))
    per = []
    for f, (n, m) in enumerate(shapes):
        d = col_data(n, m)
        X, Y, w, kin = Mat(d["X"]), Mat(d["Y"]), Mat(d["w"]), Mat(d["kin"])
        lam, mk = Mat(d["lam"]), Mat(d["mk"])
        o = dict(d=d, n=n, m=m, X=X, red=[])
        for p in range(5):
            md = (p + f) % 5
            out = Mat(shape=(m, 1), dtype=np.float64)
            tab.add(COLRED, f, mode=md, n=n, m=m, A=X, lda=X.ld, B=Y if md in (1, 4) else None, ldb=Y.ld,
                    W=w if md == 2 else None, C=out)
            o["red"].append((md, out))
        for key, with_kin in (("res_kin", True), ("res", False)):
            R, nr = Mat(shape=(n, m)), Mat(shape=(m, 1), dtype=np.float64)
            E, F = Mat(shape=(m, 1), dtype=np.float64), Mat(shape=(m, 1), dtype=np.float64)
            tab.add(RESIDUAL, f, n=n, m=m, A=Y, lda=Y.ld, B=X, ldb=X.ld, W=lam, C=R, ldc=R.ld, D=nr,
                    W2=kin if with_kin else None, E=E, F=F if with_kin else None)
            o[key] = (R, nr, E, F)
        for key, k_, mk_, s0 in (("tpa_mk", kin, mk, 0.0), ("tpa_shift", kin, None, 0.7), ("tpa_copy", None, None, 0.0)):
            dst, nr = Mat(shape=(n, m)), Mat(shape=(m, 1), dtype=np.float64)
            tab.add(TPA, f, n=n, m=m, A=Y, lda=Y.ld, C=dst, ldc=dst.ld, W=k_, W2=mk_, D=nr, s0=s0)
            o[key] = (dst, nr)
        per.append(o)
    return tab, per


def test_column_kernels(lib, bs, mode):
    """k_b_colred (modes 0-4, a different one per fiber at every position), k_b_residual with and without the kinetic
    sums, k_b_tpa in its three forms: n = 1 .. 8193 rows and m = 1 .. 24 columns in every launch, whose grid is sized by
    the widest item.  One by one, the rows of 8192 and 8193 run the 1024-thread forms of the same bodies."""
    tab, per = column_table(COL_SHAPES)
    tab.run(lib, bs, mode)
    worst = {}

    def note(key, r):
        worst[key] = max(worst.get(key, 0.0), r)

    for o in per:
        d, n, m = o["d"], o["n"], o["m"]
        for md, out in o["red"]:
            ref, terms = colred_ref(md, d)
            note(f"colred{md}", reduction_ok(out.fetch()[:, 0], ref, terms, n, squared=(md == 0)))
            assert out.rest_untouched()
        lam = L(d["lam"])[None, :]
        for key in ("res_kin", "res"):
            R, nr, E, F = o[key]
            got = R.fetch()
            ref = L(d["Y"]) - lam * L(d["X"])
            bound = 4 * U * (np.abs(d["Y"]) + np.abs(d["lam"])[None, :] * np.abs(d["X"]))
            err = np.abs(L(got) - ref)
            assert np.all(err <= bound), (key, n, m)
            note(key, float(np.max(err / bound)))
            note(key + " norms", reduction_ok(nr.fetch()[:, 0], sumsq(got), sumsq(got), n, squared=True))
            assert R.rest_untouched() and nr.rest_untouched()
            if key == "res_kin":
                x2 = L(d["X"]).real ** 2 + L(d["X"]).imag ** 2
                tk = (L(d["kin"])[:, None] * x2).sum(axis=0)
                note("res mean_kin", reduction_ok(E.fetch()[:, 0], tk, tk, n))
                note("res <x,x>", reduction_ok(F.fetch()[:, 0], x2.sum(axis=0), x2.sum(axis=0), n))
                assert E.rest_untouched() and F.rest_untouched()
            else:      # without kin neither sum is written
                E.fetch(), F.fetch()
                assert E.rest_untouched(written=False) and F.rest_untouched(written=False)
        kin = L(d["kin"])[:, None]
        for key, fac in (("tpa_mk", L(d["mk"])[None, :] / (L(d["mk"])[None, :] + kin)), ("tpa_shift", 1 / (kin + LD(0.7))),
                         ("tpa_copy", None)):
            dst, nr = o[key]
            got = dst.fetch()
            if fac is None:
                assert same_bits(got, d["Y"]), (key, n, m)
            else:
                ref = L(d["Y"]) * fac
                err, bound = np.abs(L(got) - ref), 4 * U * np.abs(ref)
                assert np.all(err <= bound), (key, n, m)
                note(key, float(np.max(err / bound)))
            note(key + " norms", reduction_ok(nr.fetch()[:, 0], sumsq(got), sumsq(got), n, squared=True))
            assert dst.rest_untouched() and nr.rest_untouched()
    print(f"column kernels ({mode}): worst error / bound", {k: round(v, 3) for k, v in worst.items()})


def test_column_kernels_merged_equals_one_by_one(lib, bs, monkeypatch):
    """One device body per operation (csrc/ew_device.h): below 8192 rows the merged launch and the original entry point
    both run it with 256 threads per column, so every output of COLRED / RESIDUAL / TPA -- reductions, R, dst, norms, E,
    F -- is the same bits either way.  (From 8192 rows on the entry point takes 1024 threads: another, equally fixed,
    summation tree; those items are held to the bounds of test_column_kernels only.)"""
    shapes = [(1024, 3), (1025, 3), (8191, 2), (8192, 2), (8193, 3), (257, 1), (1350, 7), (4653, 24)]

    def outputs(mode):
        tab, per = column_table(shapes)
        tab.run(lib, bs, mode)
        res = []
        for o in per:
            mats = [out for _, out in o["red"]] + list(o["res_kin"]) + list(o["res"][:2]) + list(o["tpa_mk"])
            mats += list(o["tpa_shift"]) + list(o["tpa_copy"])
            res.append([mt.fetch() for mt in mats])
        return res

    monkeypatch.delenv("DFTK_MI_KBATCH_SEQUENTIAL", raising=False)
    merged_out = outputs("merged")
    monkeypatch.setenv("DFTK_MI_KBATCH_SEQUENTIAL", "1")
    single_out = outputs("one-by-one")
    names = [f"colred@{p}" for p in range(5)] + ["res_kin R", "res_kin norms", "res_kin E", "res_kin F", "res R", "res norms",
                                                 "tpa_mk dst", "tpa_mk norms", "tpa_shift dst", "tpa_shift norms",
                                                 "tpa_copy dst", "tpa_copy norms"]
    compared = 0
    for (n, m), a, b in zip(shapes, merged_out, single_out):
        if n >= 8192:
            continue
        assert len(a) == len(b) == len(names)
        for name, x, y in zip(names, a, b):
            assert same_bits(x, y), (name, n, m)
            compared += 1
    assert compared == 6 * len(names)


def test_residual_with_device_rayleigh_quotients(lib, bs, merged):
    """The small-block driver's RESIDUAL: lam[c] = W[c] / W3[c] formed inside k_b_residual (batched form only)."""
    shapes = [(1, 1), (257, 7), (4653, 24)]
    tab = Table(len(shapes))
    per = []
    for f, (n, m) in enumerate(shapes):
        d = col_data(n, m)
        X, Y, num, den, kin = Mat(d["X"]), Mat(d["Y"]), Mat(d["lam"]), Mat(d["den"]), Mat(d["kin"])
        R, nr = Mat(shape=(n, m)), Mat(shape=(m, 1), dtype=np.float64)
        E, F = Mat(shape=(m, 1), dtype=np.float64), Mat(shape=(m, 1), dtype=np.float64)
        tab.add(RESIDUAL, f, n=n, m=m, A=Y, lda=Y.ld, B=X, ldb=X.ld, W=num, W3=den, C=R, ldc=R.ld, D=nr, W2=kin, E=E, F=F)
        per.append((d, n, R, nr, E, F))
    tab.run(lib, bs, merged)
    for d, n, R, nr, E, F in per:
        lam = (L(d["lam"]) / L(d["den"]))[None, :]
        got = R.fetch()
        err = np.abs(L(got) - (L(d["Y"]) - lam * L(d["X"])))
        assert np.all(err <= 4 * U * (np.abs(d["Y"]) + np.abs(lam.astype(float)) * np.abs(d["X"])))
        reduction_ok(nr.fetch()[:, 0], sumsq(got), sumsq(got), n, squared=True)
        x2 = L(d["X"]).real ** 2 + L(d["X"]).imag ** 2
        tk = (L(d["kin"])[:, None] * x2).sum(axis=0)
        reduction_ok(E.fetch()[:, 0], tk, tk, n)
        reduction_ok(F.fetch()[:, 0], x2.sum(axis=0), x2.sum(axis=0), n)
        assert R.rest_untouched() and nr.rest_untouched() and E.rest_untouched() and F.rest_untouched()


# ------------------------------------------------------------------------------------------------- element-wise kernels
def test_elementwise_kernels(lib, bs, mode):
    """k_b_rows (scale, copy, gather, fill) and k_b_small (sub-identity, add-diag, hermitise, conjugate-transpose) with
    m = 1, 5, 24, 64 and n = 1 | 4653 mixed in every launch.  Everything but the scaling is bitwise."""
    shapes = [(1, 1), (4653, 5), (1, 24), (4653, 64)]
    fills16 = [16, 16 * 5, 16 * 4653, 16 * 1000]
    fills8 = [8, 8 * 3, 8 * (2 * 4653 + 1), 8 * 77]
    tab = Table(len(shapes))
    per = []
    for f, (n, m) in enumerate(shapes):
        rng = np.random.default_rng(100 + f)
        o = dict(n=n, m=m)
        s = rng.random(m) + 0.5
        X0 = block(rng, n, m)
        o["s"], o["X0"] = s, X0
        sv = Mat(s)
        for key, inv in (("scale", 0), ("unscale", 1)):
            Xd = Mat(X0)
            tab.add(SCALE, f, n=n, m=m, C=Xd, ldc=Xd.ld, W=sv, flags=inv)
            o[key] = Xd
        src = Mat(block(rng, n, m + 2))
        o["src"] = src
        o["copy"] = Mat(shape=(n, m))
        tab.add(COPY, f, n=n, m=m, A=src, lda=src.ld, C=o["copy"], ldc=o["copy"].ld)
        perm = rng.integers(0, m + 2, m).astype(np.int32)
        perm[-1] = perm[0]                                       # a repeat
        o["perm"], o["gather"] = perm, Mat(shape=(n, m))
        tab.add(GATHER, f, n=n, m=m, A=src, lda=src.ld, W=torch.from_numpy(perm).cuda(), C=o["gather"], ldc=o["gather"].ld)
        o["fills"] = []
        for nbytes in (fills16[f], fills8[f]):
            buf = Mat(shape=(nbytes // 8, 1), dtype=np.float64, pad=5)
            tab.add(FILL0, f, C=buf, bytes=nbytes)
            o["fills"].append(buf)
        rows, i0 = m + 1, 3                                      # i0 + m > rows: the row clip matters
        o["sub0"] = block(rng, rows, m)
        o["sub"] = Mat(o["sub0"])
        tab.add(SUBID, f, n=rows, m=m, C=o["sub"], ldc=o["sub"].ld, i0=i0)
        o["sq0"] = block(rng, m, m)
        o["add"] = Mat(o["sq0"])
        tab.add(ADDDIAG, f, m=m, C=o["add"], ldc=o["add"].ld, s0=0.375 + f)
        low = o["sq0"].copy()
        low[np.tril_indices(m, -1)] = NANC                        # overwritten from the upper triangle, never read
        o["herm"] = Mat(low)
        tab.add(HERMIT, f, m=m, C=o["herm"], ldc=o["herm"].ld)
        o["ct_src"], o["ct"] = Mat(o["sq0"]), Mat(shape=(m, m))
        tab.add(CTRANS, f, m=m, A=o["ct_src"], lda=o["ct_src"].ld, C=o["ct"], ldc=o["ct"].ld)
        per.append(o)
    tab.run(lib, bs, mode)
    worst = 0.0
    for f, o in enumerate(per):
        n, m, what = o["n"], o["m"], (o["n"], o["m"], mode)
        for key, fac in (("scale", L(o["s"])), ("unscale", 1 / L(o["s"]))):
            ref = L(o["X0"]) * fac[None, :]
            err, bound = np.abs(L(o[key].fetch()) - ref), 4 * U * np.abs(ref)
            assert np.all(err <= bound) and o[key].rest_untouched(), (key, what)
            worst = max(worst, float(np.max(err / bound)))
        src = o["src"].fetch()
        assert same_bits(o["copy"].fetch(), src[:, :m]) and o["copy"].rest_untouched(), what
        assert same_bits(o["gather"].fetch(), src[:, o["perm"]]) and o["gather"].rest_untouched(), what
        for buf in o["fills"]:
            assert same_bits(buf.fetch(), np.zeros((buf.rows, 1))) and buf.rest_untouched(), (what, buf.rows)
        exp = o["sub0"].copy()
        a = np.arange(m)
        a = a[3 + a < m + 1]
        exp[3 + a, a] -= 1.0
        wr = np.zeros(exp.shape, dtype=bool)
        wr[3 + a, a] = True
        assert same_bits(o["sub"].fetch(), exp) and o["sub"].rest_untouched(written=wr), what
        exp = o["sq0"].copy()
        exp[np.diag_indices(m)] += 0.375 + f
        assert same_bits(o["add"].fetch(), exp) and o["add"].rest_untouched(written=np.eye(m, dtype=bool)), what
        up = np.triu(o["sq0"], 1)
        exp = up + up.conj().T + np.diag(np.diag(o["sq0"]).real)
        got = o["herm"].fetch()
        assert np.array_equal(got, exp) and np.array_equal(got, got.conj().T) and o["herm"].rest_untouched(), what
        assert same_bits(o["ct"].fetch(), o["sq0"].conj().T.copy()) and o["ct"].rest_untouched(), what
    print(f"scaling ({mode}): worst error / bound {worst:.3f}")


def test_fill_of_odd_size_falls_back(lib, bs, mode):
    """A fill that is no multiple of 8 bytes has no batched form: its group runs one by one and zeroes exactly `bytes`."""
    tab = Table(2)
    a = torch.full((40,), 0xAB, dtype=torch.uint8, device="cuda")
    b = torch.full((40,), 0xAB, dtype=torch.uint8, device="cuda")
    tab.add(FILL0, 0, C=a, bytes=12)
    tab.add(FILL0, 1, C=b, bytes=16)
    wit = witness(tab, 1)
    tab.run(lib, bs, mode, fallback=2)
    for t, nb in ((a, 12), (b, 16)):
        h = t.cpu().numpy()
        assert not h[:nb].any() and np.all(h[nb:] == 0xAB)
    wit()


# ------------------------------------------------------------------------------------------------- copies
def _h2d(tab, fiber, nbytes, rng):
    src = rng.integers(0, 256, nbytes, dtype=np.uint8)
    dst = torch.full((nbytes + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    tab.add(H2D, fiber, C=dst, host=src, bytes=nbytes)

    def verify():
        h = dst.cpu().numpy()
        assert np.array_equal(h[:nbytes], src) and np.all(h[nbytes:] == 0xAB), nbytes
    return verify


def _d2h(tab, fiber, nbytes, rng, wait=0):
    src = torch.from_numpy(rng.integers(0, 256, nbytes, dtype=np.uint8)).cuda()
    dst = np.full(nbytes + 16, 0xCD, dtype=np.uint8)
    tab.add(D2H, fiber, A=src, host=dst, bytes=nbytes, flags=wait)

    def verify():
        assert np.array_equal(dst[:nbytes], src.cpu().numpy()) and np.all(dst[nbytes:] == 0xCD), nbytes
    return verify


def test_host_device_copies(lib, bs, mode):
    """k_b_copy_words: payloads of 4, 12 and 100 bytes read straight from the pinned table, a group above 16 KiB that is
    staged with a copy, and results of 4 B, 12 B and 1 MiB through the mapped result slots and their host fix-ups."""
    rng = np.random.default_rng(4)
    tab = Table(3)
    checks = [_h2d(tab, f, nb, rng) for f, nb in enumerate((4, 12, 100))]
    checks += [_h2d(tab, f, 8000, rng) for f in range(3)]
    checks += [_d2h(tab, f, nb, rng, wait=int(f == 0)) for f, nb in enumerate((4, 12, 1 << 20))]
    tab.run(lib, bs, mode)
    for c in checks:
        c()


def test_copies_outside_the_batched_form(lib, bs, mode):
    """Three results of 3 MiB exceed the 8 MiB of result slots: the group takes the one-by-one copies (no slot, no fix-up
    that could overwrite them later) and delivers the right bytes; so do payloads that are no whole 4-byte words."""
    rng = np.random.default_rng(5)
    tab = Table(3)
    checks = [_d2h(tab, f, 3 << 20, rng) for f in range(3)]
    checks += [_h2d(tab, f, nb, rng) for f, nb in enumerate((5, 8, 4))]        # position 1: one payload of 5 bytes
    checks += [_d2h(tab, 1, 6, rng), _d2h(tab, 2, 8, rng)]                      # position 2: one result of 6 bytes
    wit = witness(tab, 0)
    tab.run(lib, bs, mode, fallback=8)
    for c in checks:
        c()
    wit()


# ------------------------------------------------------------------------------------------------- banded D of the projectors
def test_apply_D_of_different_blocks(lib, mode):
    """k_b_apply_D: Y = D X with the banded real D of three k-blocks that differ in n_p, bandwidth and band count."""
    ob = make_oracle_basis(5, (15, 15, 15), terms=("Kinetic",))
    kpt = ob.kpoints[0]
    basis = Basis(lib, 15, 15, 15, ob.model.unit_cell_volume)
    rng = np.random.default_rng(8)
    tab = Table(3)
    per = []
    for f, (n_p, bw, nb) in enumerate([(4, 0, 1), (18, 2, 3), (40, 5, 7)]):
        kb = KBlock(lib, basis, kpt.mapping, np.zeros(len(kpt.mapping)))
        D = rng.standard_normal((n_p, n_p))
        D = np.triu(np.tril(D + D.T, bw), -bw)
        kb.set_projectors(block(rng, len(kpt.mapping), n_p), D)
        X = block(rng, n_p, nb)
        Xd, Yd = Mat(X, pad=0), Mat(shape=(n_p, nb), pad=0)
        tab.add(APPLYD, f, kb=kb.h.value, m=nb, A=Xd, C=Yd)
        per.append((kb, D, X, Xd, Yd, bw))
    basis.sync()
    tab.run(lib, basis, mode)
    for kb, D, X, Xd, Yd, bw in per:
        err = np.abs(L(Yd.fetch()) - L(D) @ L(X))
        bound = 4 * (2 * bw + 1 + 4) * U * (np.abs(D) @ np.abs(X))
        assert np.all(err <= bound) and Yd.rest_untouched(), (D.shape, float(np.max(err / bound)))


# ------------------------------------------------------------------------------------------------- Cholesky
@functools.lru_cache(maxsize=None)
def gram(n):
    """Complex Gram matrix for odd n, real symmetric for even n (as test_potrf_trtri)."""
    rng = np.random.default_rng(n)
    X = rng.standard_normal((3 * n + 5, n)) + (1j if n % 2 else 0) * rng.standard_normal((3 * n + 5, n))
    return (X.conj().T @ X).astype(complex)


class Potrf:
    def __init__(self, tab, fiber, n, O=None):
        self.n, self.O = n, gram(n) if O is None else O
        A = self.O.copy()
        A[np.tril_indices(n, -1)] = NANC       # the strict lower triangle is loaded, must not matter and must stay
        self.A, self.I = Mat(A), Mat(shape=(n, n))
        self.est = np.full(3, -7.0)
        self.row = tab.add(POTRF, fiber, m=n, C=self.A, ldc=self.A.ld, D=self.I, ldb=self.I.ld, host=self.est)

    def verify(self):
        n, O = self.n, self.O
        got, invR = self.A.fetch(), self.I.fetch()
        R = np.triu(got)
        relerr = np.linalg.norm(R.conj().T @ R - O) / np.linalg.norm(O)
        assert relerr < 1e-13, (n, relerr)
        assert np.linalg.norm(invR @ R - np.eye(n)) < 1e-10 * np.linalg.cond(R), n
        assert not np.tril(invR, -1).any(), n
        assert self.A.rest_untouched(written=np.triu(np.ones((n, n), dtype=bool))), n      # NaNs below the diagonal stayed
        assert self.I.rest_untouched(), n
        for est, T in zip(self.est[:2], (R, np.triu(invR))):
            ref = np.abs(L(np.diag(T))).max() + np.sqrt(sumsq(np.triu(T, 1)).sum())
            assert abs(LD(est) - ref) <= (n * n + 8) * U * ref, (n, est, ref)
        assert self.est[2] == -7.0


def test_potrf_groups(lib, bs, mode):
    """k_b_potrf: orders 1 .. 32 in one launch (one wave per matrix), then 5 .. 64 in one (256 threads; the order-5 matrix
    under the pitch of the order-64 one)."""
    groups = [(1, 2, 7, 16, 24, 31, 32), (5, 33, 48, 63, 64)]
    tab = Table(7)
    items = [Potrf(tab, f, n) for g in groups for f, n in enumerate(g)]
    status = tab.run(lib, bs, mode)
    assert not any(status), status
    if mode == "merged":
        assert stats(lib)["merged_launches"] == 2
    for it in items:
        it.verify()


def test_potrf_reports_failures_per_item(lib, bs, mode):
    """An indefinite and a NaN matrix among good ones: DFTK_MI_NUM_CHOLESKY for those rows only, the neighbours right."""
    tab = Table(4)
    bad = gram(16) - 2 * np.trace(gram(16)).real / 16 * np.eye(16)
    nan = gram(24).copy()
    nan[3, 5] = np.nan
    items = [Potrf(tab, 0, 7), Potrf(tab, 1, 16, bad), Potrf(tab, 2, 24, nan), Potrf(tab, 3, 31)]
    status = tab.run(lib, bs, mode)
    assert status == [0, NUM_CHOLESKY, NUM_CHOLESKY, 0], status
    items[0].verify()
    items[3].verify()
    for it in items[1:3]:
        it.A.fetch(), it.I.fetch()
        assert it.A.rest_untouched(written=np.triu(np.ones((it.n, it.n), dtype=bool))) and it.I.rest_untouched()


def test_dense_orders_above_64_fall_back(lib, bs, mode):
    """n = 65 has no batched factorisation / eigensolver: both groups run one by one."""
    tab = Table(2)
    items = [Potrf(tab, 0, 65), Potrf(tab, 1, 8)]
    heevs = [Heev(tab, 0, 65, "random"), Heev(tab, 1, 8, "random")]
    wit = witness(tab, 0)
    status = tab.run(lib, bs, mode, fallback=4)
    assert not any(status), status
    for it in items + heevs:
        it.verify()
    wit()


# ------------------------------------------------------------------------------------------------- Hermitian eigensolver
@functools.lru_cache(maxsize=None)
def heev_matrix(n, kind):
    rng = np.random.default_rng(1000 + n)
    X = block(rng, n, n)
    A = (X + X.conj().T) / 2
    if kind == "diagonal":          # unsorted: no sweep at all
        A = np.diag(rng.standard_normal(n)).astype(complex)
    elif kind == "degenerate":      # three eigenvalues with large multiplicities (test_heev)
        Q = np.linalg.qr(X)[0]
        A = (Q * rng.choice([-1.0, 0.0, 2.0], n)[None, :]) @ Q.conj().T
        A = (A + A.conj().T) / 2
    elif kind == "real":
        A = A.real + 0j
    elif kind == "ritz":            # Rayleigh-Ritz-like: sorted diagonal + weak coupling
        A = np.diag(np.sort(rng.standard_normal(n))) + 1e-3 * A
    elif kind == "tiny":
        A = A * 1e-150
    elif kind == "huge":
        A = A * 1e150
    elif kind == "nan":
        A = A.copy()
        A[0, n - 1] = A[n - 1, 0] = np.nan
    return A


class Heev:
    def __init__(self, tab, fiber, n, kind, device_values=False):
        self.n, self.kind, self.Ah = n, kind, heev_matrix(n, kind)
        self.A, self.V = Mat(self.Ah), Mat(shape=(n, n))
        self.W = np.full(n + 1, -7.0)
        self.E = Mat(shape=(n, 1), dtype=np.float64) if device_values else None
        self.row = tab.add(HEEV, fiber, m=n, C=self.A, ldc=self.A.ld, D=self.V, ldb=self.V.ld, host=self.W, E=self.E)

    def verify(self):
        """test_heev's assertions; for the matrices scaled by 1e+-150 `scale` is the spectrum's own size instead of
        max(|w|, 1), so that a lost spectrum cannot pass."""
        n, A, W, V = self.n, self.Ah, self.W[:self.n], self.V.fetch()
        what = (n, self.kind)
        self.A.fetch()
        assert self.A.rest_untouched(written=True) and self.V.rest_untouched() and self.W[n] == -7.0, what
        wref = np.linalg.eigvalsh(A)
        scale = np.abs(wref).max() if self.kind in ("tiny", "huge") else max(np.abs(wref).max(), 1.0)
        assert np.abs(W - wref).max() < 1e-12 * scale, (what, np.abs(W - wref).max() / scale)
        assert np.linalg.norm(V.conj().T @ V - np.eye(n)) < max(1e-12, 5e-14 * n), what
        s = 1.0 / scale if self.kind in ("tiny", "huge") else 1.0       # (the residual itself, formed without overflow)
        assert np.linalg.norm((A * s) @ V - V * (W * s)[None, :]) < 1e-11 * (scale * s) * np.sqrt(n), what
        if self.E is not None:
            assert same_bits(self.E.fetch()[:, 0], W) and self.E.rest_untouched(), what


HEEV_GROUPS = [[(10, "random"), (9, "diagonal"), (6, "degenerate"), (3, "real"), (2, "ritz"), (10, "tiny"), (9, "huge"),
                (1, "random")],
               [(64, "random"), (63, "diagonal"), (33, "degenerate"), (24, "real"), (19, "ritz"), (18, "tiny"),
                (11, "huge"), (7, "random")]]


def test_heev_groups(lib, bs, mode):
    """k_b_heev: orders 1 .. 10 in one launch (one wave per matrix), 7 .. 64 in another (256 threads; odd orders padded
    by a decoupled diagonal entry), each with a random, a diagonal, a degenerate, a real symmetric, a Rayleigh-Ritz-like
    and two badly scaled matrices."""
    tab = Table(8)
    items = [Heev(tab, f, n, kind) for g in HEEV_GROUPS for f, (n, kind) in enumerate(g)]
    status = tab.run(lib, bs, mode)
    assert not any(status), [(it.n, it.kind, s) for it, s in zip(items, status) if s]
    if mode == "merged":
        assert stats(lib)["merged_launches"] == 2
    for it in items:
        it.verify()


def test_heev_reports_a_non_finite_item_alone(lib, bs, mode):
    tab = Table(4)
    items = [Heev(tab, 0, 9, "random"), Heev(tab, 1, 19, "nan"), Heev(tab, 2, 24, "ritz"), Heev(tab, 3, 6, "random")]
    status = tab.run(lib, bs, mode)
    assert status == [0, NUM_NONFINITE, 0, 0], status
    for it in (items[0], items[2], items[3]):
        it.verify()
    assert np.all(items[1].W == -7.0)


def test_heev_device_eigenvalues(lib, bs, merged):
    """HEEV with E: the device copy the residual pass of the same round reads equals the host eigenvalues bitwise; the
    status of a non-finite item arrives in the table with the fiber's next synchronisation."""
    tab = Table(5)
    items = [Heev(tab, f, n, kind, device_values=True)
             for f, (n, kind) in enumerate([(7, "random"), (24, "ritz"), (19, "degenerate"), (64, "real"), (11, "nan")])]
    status = tab.run(lib, bs, merged)
    assert status == [0, 0, 0, 0, NUM_NONFINITE], status
    for it in items[:4]:
        it.verify()


# ------------------------------------------------------------------------------------------------- fused orthogonalisation
class Ortho:
    def __init__(self, tab, fiber, n, m, ny, cond, kind="good"):
        rng = np.random.default_rng(n + m + ny)
        self.n, self.m, self.ny, self.cond, self.kind = n, m, ny, cond, kind
        Y = np.linalg.qr(block(rng, n, max(ny, 1)))[0][:, :ny]
        X = block(rng, n, m) @ (np.linalg.qr(block(rng, m, m))[0] * np.geomspace(1.0, 1.0 / cond, m)) @ np.linalg.qr(block(rng, m, m))[0]
        if ny:
            X = X + 0.5 * Y @ block(rng, ny, m)
        if kind in ("in_span", "nan"):
            X[:, m // 2] = Y @ block(rng, ny, 1)[:, 0]       # drop_small! would re-randomise this column: status 1
        if kind == "nan":
            X[5, 1] = np.nan
        self.Xh, self.Yh = X, Y
        self.X, self.Y = Mat(X), Mat(Y) if ny else None
        self.res = np.full(5, -7.0)
        self.row = tab.add(ORTHO, fiber, n=n, m=m, k=ny, C=self.X, ldc=self.X.ld, A=self.Y, lda=self.Y.ld if ny else 0,
                           s0=2 * EPS, host=self.res)

    def verify(self, status):
        n, m, ny, cond, X, Y = self.n, self.m, self.ny, self.cond, self.Xh, self.Yh
        what = (n, m, ny, cond, self.kind, self.res)
        Q = self.X.fetch()
        assert self.X.rest_untouched() and self.res[4] == -7.0, what
        expect = {"good": 0, "in_span": 1, "nan": 2}[self.kind]
        assert self.res[0] == expect and status == expect, what
        if expect:
            return
        assert np.linalg.norm(Q.conj().T @ Q - np.eye(m)) < 50 * EPS * m, what
        ref = X - Y @ (Y.conj().T @ X) if ny else X
        if ny:
            assert np.linalg.norm(Y.conj().T @ Q) < 10 * EPS * np.sqrt(n), what
        out = ref - Q @ (Q.conj().T @ ref)
        assert np.linalg.norm(out) < (1e-13 * cond + 1e-12) * np.linalg.norm(ref), (what, np.linalg.norm(out) / np.linalg.norm(ref))


def test_ortho_in_mixed_groups(lib, bs, merged):
    """The fused kernel is chosen by the LONGEST item of a launch and then runs the shorter ones: 300 .. 2048 rows under
    the register-resident variant of 4 x 512 rows (with one item whose column lies inside span(Y) and one non-finite
    item: results 1 and 2 for those alone), then 997 and 2049 rows under the streaming kernel."""
    first = [(300, 1, 3, 1.0), (512, 6, 16, 1e2), (513, 8, 0, 1e4), (725, 6, 3, 1e6), (1350, 8, 0, 1e9), (2047, 6, 16, 1e3),
             (2048, 1, 0, 1.0)]
    tab = Table(len(first) + 2)
    items = [Ortho(tab, f, *a) for f, a in enumerate(first)]
    items.append(Ortho(tab, 7, 900, 4, 6, 1.0, "in_span"))
    items.append(Ortho(tab, 8, 900, 4, 6, 1.0, "nan"))
    items += [Ortho(tab, 0, 997, 1, 3, 1.0), Ortho(tab, 1, 2049, 8, 16, 1e3)]
    status = tab.run(lib, bs, merged)
    assert stats(lib)["merged_launches"] == 2
    for it in items:
        it.verify(status[it.row])


# ------------------------------------------------------------------------------------------------- a dependent chain
def test_cholesky_qr_chain_per_fiber(lib, bs, mode):
    """Cholesky-QR per fiber: G = X^H X (UPPER) -> copy -> hermitise -> copy -> add-diag -> copy -> Cholesky + inverse ->
    Q = X inv(R) (B_UPPER) -> column norms, with a different shape per fiber and one fiber that synchronises in the middle:
    position-by-position merging must keep every fiber's own order.  Every intermediate has its own buffer."""
    shapes = [(257, 5), (1350, 8), (4653, 24), (300, 1)]
    shift = 1e-3
    tab = Table(len(shapes))
    per = []
    for f, (n, m) in enumerate(shapes):
        g = Gemm(tab, f, "C", m, m, n, UPPER, 1.0, 0.0, seed=77)
        tab.rows[-1].B, tab.rows[-1].ldb = g.A.ptr, g.A.ld               # X^H X: both operands are X
        X = g.A
        G2, G3, G4, Iv = Mat(shape=(m, m)), Mat(shape=(m, m)), Mat(shape=(m, m)), Mat(shape=(m, m))
        Q, nr = Mat(shape=(n, m)), Mat(shape=(m, 1), dtype=np.float64)
        est = np.zeros(2)
        tab.add(COPY, f, n=m, m=m, A=g.C, lda=g.C.ld, C=G2, ldc=G2.ld)
        tab.add(HERMIT, f, m=m, C=G2, ldc=G2.ld, sync_after=int(f == 1))
        tab.add(COPY, f, n=m, m=m, A=G2, lda=G2.ld, C=G3, ldc=G3.ld)
        tab.add(ADDDIAG, f, m=m, C=G3, ldc=G3.ld, s0=shift)
        tab.add(COPY, f, n=m, m=m, A=G3, lda=G3.ld, C=G4, ldc=G4.ld)
        tab.add(POTRF, f, m=m, C=G4, ldc=G4.ld, D=Iv, ldb=Iv.ld, host=est)
        tab.add(ZGEMM, f, trans="N", gm=n, gn=m, gk=m, alpha=1.0, beta=0.0, A=X, lda=X.ld, B=Iv, ldb=Iv.ld, C=Q, ldc=Q.ld,
                flags=B_UPPER)
        tab.add(COLRED, f, mode=0, n=n, m=m, A=Q, lda=Q.ld, C=nr)
        per.append((n, m, g, G2, G3, G4, Iv, Q, nr))
    status = tab.run(lib, bs, mode)
    assert not any(status), status
    for n, m, g, G2, G3, G4, Iv, Q, nr in per:
        Xh = g.A.fetch()
        # G: the reference of gemm_ref was formed with an independent B; redo it for B = X
        G1 = g.C.fetch()
        ref = L(Xh).conj().T @ L(Xh)
        bound = 4 * (n + 4) * U * (np.abs(Xh).T @ np.abs(Xh))
        iu = np.triu_indices(m)
        assert np.all(np.abs(L(G1) - ref)[iu] <= bound[iu]), (n, m)
        up = np.triu(G1, 1)
        herm = up + up.conj().T + np.diag(np.diag(G1).real)
        assert np.array_equal(G2.fetch(), herm) and G2.rest_untouched(), (n, m)
        shifted = herm.copy()
        shifted[np.diag_indices(m)] += shift
        assert same_bits(G3.fetch(), shifted) and G3.rest_untouched(), (n, m)
        R, invR = np.triu(G4.fetch()), Iv.fetch()
        assert np.array_equal(np.tril(G4.fetch(), -1), np.tril(shifted, -1)), (n, m)        # the copy's lower triangle stays
        assert np.linalg.norm(R.conj().T @ R - shifted) < 1e-13 * np.linalg.norm(shifted), (n, m)
        assert np.linalg.norm(invR @ R - np.eye(m)) < 1e-10 * np.linalg.cond(R) and not np.tril(invR, -1).any(), (n, m)
        Qh = Q.fetch()
        err = np.abs(L(Qh) - L(Xh) @ L(np.triu(invR)))
        assert np.all(err <= 4 * (m + 4) * U * (np.abs(Xh) @ np.abs(np.triu(invR)))) and Q.rest_untouched(), (n, m)
        reduction_ok(nr.fetch()[:, 0], sumsq(Qh), sumsq(Qh), n, squared=True)
        assert nr.rest_untouched()
        assert np.linalg.norm(Qh.conj().T @ Qh - np.eye(m)) < 1e-2, (n, m)      # (the shift 1e-3 on a Gram matrix of order n)


# ------------------------------------------------------------------------------------------------- malformed tables
def test_malformed_tables_are_refused_before_anything_runs(lib, bs, merged):
    src, dst = Mat(np.ones((3, 2), dtype=complex)), Mat(shape=(3, 2))
    good = dict(n=3, m=2, A=src, lda=src.ld, C=dst, ldc=dst.ld)

    def refused(n_fibers, *rows):
        tab = Table(n_fibers)
        tab.add(COPY, 0, **good)
        for typ, fiber, kw in rows:
            tab.add(typ, fiber, **kw)
        assert tab.call(lib, bs) == -1
        dst.fetch()
        assert dst.rest_untouched(written=False)         # the well-formed first row has not run either

    refused(1, (COPY, 1, good))                                            # fiber out of range
    refused(1, (COPY, -1, good))
    refused(1, (16, 0, good))                                              # APPLYH is not replayed
    refused(1, (99, 0, good))
    refused(1, (COPY, 0, dict(good, lda=2)))                               # ld < rows
    refused(1, (COPY, 0, dict(good, C=None)))
    refused(1, (COPY, 0, dict(good, m=0)))
    refused(1, (COPY, 0, dict(good, join_next=1)))                         # nothing to join
    refused(1, (COPY, 0, dict(good, join_next=1)), (HERMIT, 0, dict(m=2, C=dst, ldc=dst.ld)))
    refused(1, (ZGEMM, 0, dict(trans="T", gm=2, gn=2, gk=3, A=src, lda=src.ld, B=src, ldb=src.ld, C=dst, ldc=dst.ld)))
    refused(1, (ZGEMM, 0, dict(trans="C", gm=2, gn=2, gk=3, A=src, lda=src.ld, B=src, ldb=src.ld, C=dst, ldc=dst.ld, flags=16)))
    refused(1, (COLRED, 0, dict(mode=5, n=3, m=2, A=src, lda=src.ld, C=dst)))
    refused(1, (ORTHO, 0, dict(n=3, m=9, k=0, C=dst, ldc=dst.ld, host=np.zeros(4))))
    refused(1, (POTRF, 0, dict(m=2, C=dst, ldc=dst.ld, D=dst, ldb=dst.ld)))   # no host array for the norm estimates
    assert lib.dftk_mi_batch_replay(bs.h, 0, 0, None) == -1
