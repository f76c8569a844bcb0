"""The optimiser of direct_minimization at the C ABI (csrc/dm_kernels.hip; ctypes, device memory from torch) against the
longdouble twin of tests/dm_twin.py.

Shapes.  A work item of the kernels is DM_CH = 1024 rows of one column, walked by 256 threads (four waves of 64): the rows are
1 (one lane), 63 / 64 / 65 (the wave), 255 / 256 / 257 (the workgroup), 1023 / 1024 / 1025 (the item: the last forces a
second, one-row item) and 4097 (five items per column); 1, 3, 4 and 33 columns; 1, 2 and 3 blocks of unequal rows and
columns behind one grid; memory 1 and 3; the direction with 0 pairs, 1 pair, a full history and after wrap-around
(memory + 2 updates); every block has a leading dimension above its rows and NaN in the padding; both middle steps (the
Teter-Payne-Allan form on k-blocks of an 18^3 cube -- the lowest plane waves of the silicon cell, as many as the block has
rows -- and NULL).

Bound, the project's convention: the device result may differ from the longdouble twin by
max(64 x the error of the SAME recursion in float64 NumPy against the longdouble one, n eps scale), where the second term is
the floor for cases in which the float64 twin happens to round like the reference: n = 2 k + 2 sequential steps of the
recursion with k pairs, scale = the largest entry of any intermediate vector of the longdouble run (those before the middle
step divided by the smallest scale_b, through which their rounding reaches the result).  <s, y> of an update: 64 eps sum |Re(conj(s) y)| (at most
4 sequential additions per thread, a wave tree, 4 wave sums, then the block partials in order).

The refusal "inside a batched multi-k call" cannot be reached through the ABI (``dftk_mi_batch_replay`` takes enumerated
operations only); the other refusals are all here.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402

import dm_twin as twin  # noqa: E402
import refine_twin  # noqa: E402
from test_gpu_kernels import Basis, KBlock, LATTICE, dev  # noqa: E402

EPS = 2.0 ** -52
EINVAL = -1                           # DFTK_MI_EINVAL
FFT = (18, 18, 18)
ROWS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
COLS = [1, 3, 4, 33]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs(lib):
    return Basis(lib, *FFT, 1.0)


_KB = {}


def kblock(lib, bs, n_rows):
    """the n_rows plane waves of lowest kinetic energy of the silicon cell on the 18^3 cube, as a k-block; once per size"""
    if n_rows not in _KB:
        nx, ny, nz = FFT
        G = refine_twin.G_of_mapping(np.arange(nx * ny * nz, dtype=np.int64), FFT).astype(float)
        B = 2 * np.pi * np.linalg.inv(np.asarray(LATTICE, dtype=float).T)
        kin_all = 0.5 * np.sum((G @ B.T) ** 2, axis=1)
        mapping = np.sort(np.argsort(kin_all, kind="stable")[:n_rows]).astype(np.int64)
        _KB[n_rows] = (KBlock(lib, bs, mapping, kin_all[mapping]), kin_all[mapping])
    return _KB[n_rows]


def block_shapes(rows, cols, n_blocks):
    return [(rows, cols), (rows // 2 + 1, cols + 2), (rows + 7, max(1, cols - 1))][:n_blocks]


def padded(A, pad):
    """(n_rows, n_cols) host block -> band-major device tensor with leading dimension n_rows + pad, NaN in the padding"""
    n, m = A.shape
    buf = np.full((m, n + pad), complex(np.nan, np.nan))
    buf[:, :n] = A.T
    return dev(buf)


def unpad(t, n):
    h = t.cpu().numpy()
    assert np.isnan(h[:, n:]).all()                      # the padding is untouched
    return h[:, :n].T.copy()


class Acc:
    def __init__(self, lib, bs, shapes, memory):
        self.lib, self.shapes, self.n = lib, shapes, len(shapes)
        self.h = C.c_void_p()
        rows = (C.c_int64 * self.n)(*[r for r, _ in shapes])
        cols = (C.c_int * self.n)(*[c for _, c in shapes])
        check(lib.dftk_mi_lbfgs_create(bs.h, self.n, rows, cols, memory, C.byref(self.h)))

    def tables(self, blocks):
        return ((C.c_void_p * self.n)(*[b.data_ptr() for b in blocks]), (C.c_int64 * self.n)(*[b.stride(0) for b in blocks]))

    def update(self, x, g):
        xp, xl = self.tables(x)
        gp, gl = self.tables(g)
        sy, kept = C.c_double(-7.0), C.c_int(-7)
        check(self.lib.dftk_mi_lbfgs_update(self.h, xp, xl, gp, gl, C.byref(sy), C.byref(kept)))
        return sy.value, kept.value

    def direction(self, g, scale, d, kbs=None, mks=None):
        gp, gl = self.tables(g)
        dp, dl = self.tables(d)
        sc = (C.c_double * self.n)(*scale)
        kb = (C.c_void_p * self.n)(*[k.h.value for k in kbs]) if kbs else None
        keep = [np.ascontiguousarray(m, dtype=np.float64) for m in mks] if kbs else []
        mk = (C.c_void_p * self.n)(*[m.ctypes.data for m in keep]) if kbs else None
        return self.lib.dftk_mi_lbfgs_direction(self.h, gp, gl, kb, mk, sc, dp, dl)

    @property
    def history(self):
        return self.lib.dftk_mi_lbfgs_history(self.h)

    def close(self):
        if self.h:
            check(self.lib.dftk_mi_lbfgs_destroy(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def counts(lib):
    a, b = C.c_int64(), C.c_int64()
    check(lib.dftk_mi_launch_count(C.byref(a), C.byref(b)))
    return a.value, b.value


def crandn(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def points(rng, shapes, n):
    """n points and the gradients of a convex function there (a diagonal in [0.5, 2] plus a rank-one term per block): every
    pair has <s, y> > 0"""
    diag = [0.5 + 1.5 * rng.random(s) for s in shapes]
    u = [crandn(rng, s) / np.sqrt(s[0] * s[1]) for s in shapes]
    out = []
    for _ in range(n):
        x = [crandn(rng, s) for s in shapes]
        t = twin.dot(u, x)
        out.append((x, [d * a + t * v for d, a, v in zip(diag, x, u)]))
    return out


def run_case(lib, bs, rows, cols, n_blocks, memory, use_kb, report):
    shapes = block_shapes(rows, cols, n_blocks)
    rng = np.random.default_rng(1000 * rows + 10 * cols + 3 * n_blocks + memory)
    pts = points(rng, shapes, memory + 3)
    scale = [0.25, 0.5, 1.5][:n_blocks]
    kbs = kin = mks = None
    if use_kb:
        pairs = [kblock(lib, bs, r) for r, _ in shapes]
        kbs, kin = [p[0] for p in pairs], [p[1] for p in pairs]
        mks = [0.3 + 2.0 * rng.random(c) for _, c in shapes]
    acc = Acc(lib, bs, shapes, memory)
    ref, f64 = twin.LbfgsTwin(memory), twin.LbfgsTwin(memory, real=np.float64)
    check_at = {1: 0, 2: 1, memory + 1: memory, memory + 3: memory}       # updates done -> pairs held
    try:
        for n_upd, (x, g) in enumerate(pts, start=1):
            xd = [padded(a, 3 + b) for b, a in enumerate(x)]
            gd = [padded(a, 5 + b) for b, a in enumerate(g)]
            torch.cuda.synchronize()
            sy, kept = acc.update(xd, gd)
            sy_ref, kept_ref = ref.update(x, g)
            sy_64, _ = f64.update(x, g)
            assert kept == int(kept_ref) and acc.history == len(ref.pairs) == min(n_upd - 1, memory)
            if n_upd > 1:
                s, y, _ = ref.pairs[-1]
                floor = 64 * EPS * float(sum(np.abs(a.real * b.real + a.imag * b.imag).sum() for a, b in zip(s, y)))
                bound = max(64 * abs(sy_64 - sy_ref), floor)
                report["sy"] = max(report.get("sy", 0.0), abs(sy - sy_ref) / bound)
                assert abs(sy - sy_ref) <= bound, (n_upd, sy, sy_ref, bound)
            else:
                assert sy == 0.0
            if n_upd not in check_at:
                continue
            k = check_at[n_upd]
            assert acc.history == k
            q = [crandn(rng, s) for s in shapes]
            qd = [padded(a, 2 + b) for b, a in enumerate(q)]
            q_before = [t.clone() for t in qd]
            dd = [padded(np.zeros(s, dtype=complex), 4 + b) for b, s in enumerate(shapes)]
            torch.cuda.synchronize()
            check(acc.direction(qd, scale, dd, kbs, mks))
            bs.sync()
            got = [unpad(t, s[0]) for t, s in zip(dd, shapes)]
            for a, b in zip(qd, q_before):                                  # g is not modified (NaN padding included)
                assert torch.equal(torch.view_as_real(a).view(torch.int64), torch.view_as_real(b).view(torch.int64))
            want = ref.direction(q, scale, kin, mks)
            w64 = f64.direction(q, scale, kin, mks)
            err = max(float(np.abs(a - b).max()) for a, b in zip(got, want))
            e64 = max(float(np.abs(a.astype(twin.CLD) - b).max()) for a, b in zip(w64, want))
            floor = (2 * k + 2) * EPS * max(ref.peak_q / min(scale), ref.peak_r)
            bound = max(64 * e64, floor)
            report["d"] = max(report.get("d", 0.0), err / bound)
            report["worst"] = max(report.get("worst", 0.0), err / max(float(np.abs(a).max()) for a in want))
            assert err <= bound, (rows, cols, n_blocks, memory, use_kb, k, err, bound)
    finally:
        acc.close()


@pytest.mark.parametrize("rows", ROWS)
def test_direction_and_update_against_the_longdouble_twin(lib, bs, rows):
    """every (columns, memory, middle step) for this row count, the number of blocks cycling 1, 2, 3 through them; within a
    run the direction is checked at 0 pairs, 1 pair, a full history and after wrap-around"""
    report, i = {}, ROWS.index(rows)
    for cols in COLS:
        for memory in (1, 3):
            for use_kb in (False, True):
                run_case(lib, bs, rows, cols, 1 + i % 3, memory, use_kb, report)
                i += 1
    print(f"\nlbfgs rows {rows}: direction err / bound up to {report['d']:.3g} (relative error up to {report['worst']:.2e}), "
          f"<s, y> err / bound up to {report['sy']:.3g}")


def test_every_block_count_at_the_item_edge(lib, bs):
    """1, 2 and 3 blocks at 1025 rows (two items per column) with 33 columns, both memories and both middle steps"""
    report = {}
    for n_blocks in (1, 2, 3):
        for memory in (1, 3):
            for use_kb in (False, True):
                run_case(lib, bs, 1025, 33, n_blocks, memory, use_kb, report)
    print(f"\nlbfgs 1025 x 33, 1 .. 3 blocks: direction err / bound up to {report['d']:.3g}")


def test_empty_history_is_the_preconditioner(lib, bs):
    """with no pair held the result is -tpa_ldiv(g) / scale to 2 ulp (one more rounding: the division), and two calls are
    bitwise equal"""
    rng = np.random.default_rng(3)
    shapes = block_shapes(1025, 4, 3)
    scale = [0.25, 1.0 / 3.0, 1.5]
    pairs = [kblock(lib, bs, r) for r, _ in shapes]
    mks = [0.3 + 2.0 * rng.random(c) for _, c in shapes]
    q = [crandn(rng, s) for s in shapes]
    qd = [padded(a, 1 + b) for b, a in enumerate(q)]
    acc = Acc(lib, bs, shapes, 2)
    d1 = [padded(np.zeros(s, dtype=complex), 2) for s in shapes]
    d2 = [padded(np.zeros(s, dtype=complex), 2) for s in shapes]
    torch.cuda.synchronize()
    check(acc.direction(qd, scale, d1, [p[0] for p in pairs], mks))
    check(acc.direction(qd, scale, d2, [p[0] for p in pairs], mks))
    bs.sync()
    for (kb, _), s, sc, mk, t_q, t1, t2 in zip(pairs, shapes, scale, mks, qd, d1, d2):
        y = torch.full_like(t_q, complex(np.nan, np.nan))
        check(lib.dftk_mi_tpa_ldiv(kb.h, s[1], t_q.data_ptr(), t_q.stride(0), mk.ctypes.data, 1.0, y.data_ptr(), y.stride(0)))
        bs.sync()
        want = -unpad(y, s[0]) / sc
        got = unpad(t1, s[0])
        assert (np.abs(got.real - want.real) <= 2 * np.spacing(np.abs(want.real))).all()
        assert (np.abs(got.imag - want.imag) <= 2 * np.spacing(np.abs(want.imag))).all()
        assert np.array_equal(got, unpad(t2, s[0]))
    acc.close()


def test_two_calls_are_bitwise_equal_and_leave_the_history_alone(lib, bs):
    rng = np.random.default_rng(4)
    shapes = block_shapes(4097, 3, 2)
    acc = Acc(lib, bs, shapes, 3)
    for x, g in points(rng, shapes, 5):
        acc.update([padded(a, 1) for a in x], [padded(a, 2) for a in g])
    assert acc.history == 3
    q = [padded(crandn(rng, s), 3) for s in shapes]
    out = []
    for _ in range(3):
        d = [padded(np.zeros(s, dtype=complex), 1) for s in shapes]
        torch.cuda.synchronize()
        check(acc.direction(q, [0.5, 2.0], d))
        bs.sync()
        out.append([unpad(t, s[0]) for t, s in zip(d, shapes)])
    for other in out[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(out[0], other))
    assert acc.history == 3
    acc.close()


def test_pairs_without_positive_curvature_are_dropped(lib, bs):
    rng = np.random.default_rng(5)
    shapes = block_shapes(257, 3, 2)
    acc = Acc(lib, bs, shapes, 2)
    pts = points(rng, shapes, 3)
    for x, g in pts:
        acc.update([dev(a.T.copy()) for a in x], [dev(a.T.copy()) for a in g])
    assert acc.history == 2
    q = [dev(crandn(rng, s).T.copy()) for s in shapes]

    def direction():
        d = [torch.zeros_like(t) for t in q]
        torch.cuda.synchronize()
        check(acc.direction(q, [1.0, 1.0], d))
        bs.sync()
        return [t.cpu().numpy() for t in d]
    before = direction()
    x, g = pts[-1]
    x2, g2 = [a + 0.1 for a in x], [a - 0.3 for a in g]                 # s = 0.1, y = -0.3 everywhere: <s, y> < 0
    sy, kept = acc.update([dev(a.T.copy()) for a in x2], [dev(a.T.copy()) for a in g2])
    assert sy < 0 and kept == 0 and acc.history == 2
    x2 = [a + 0.1 for a in x2]                                          # the same gradient again: y = 0, <s, y> = 0
    sy, kept = acc.update([dev(a.T.copy()) for a in x2], [dev(a.T.copy()) for a in g2])
    assert sy == 0.0 and kept == 0 and acc.history == 2
    x2 = [a + 0.1 for a in x2]
    bad = [a.copy() for a in g]
    bad[0][0, 0] = np.inf
    sy, kept = acc.update([dev(a.T.copy()) for a in x2], [dev(a.T.copy()) for a in bad])
    assert kept == 0 and acc.history == 2 and not np.isfinite(sy)
    after = direction()                                    # a full history survives rejected candidates bit for bit
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    check(lib.dftk_mi_lbfgs_reset(acc.h))
    assert acc.history == 0
    assert acc.update([dev(a.T.copy()) for a in x], [dev(a.T.copy()) for a in g]) == (0.0, 0)     # stores only
    acc.close()


def test_launches_and_synchronisations(lib, bs):
    """the direction: no host synchronisation, 2 k + 1 launches whatever the number of blocks; an update: exactly one
    synchronisation (none for the first, which only stores)"""
    rng = np.random.default_rng(6)
    launches = {}
    for n_blocks in (1, 3):
        shapes = block_shapes(1025, 4, n_blocks)
        acc = Acc(lib, bs, shapes, 3)
        pts = points(rng, shapes, 4)
        for i, (x, g) in enumerate(pts):
            xd, gd = [dev(a.T.copy()) for a in x], [dev(a.T.copy()) for a in g]
            torch.cuda.synchronize()
            bs.sync()
            l0, s0 = counts(lib)
            acc.update(xd, gd)
            l1, s1 = counts(lib)
            assert (l1 - l0, s1 - s0) == (1, 0 if i == 0 else 1)
        q = [dev(crandn(rng, s).T.copy()) for s in shapes]
        d = [torch.zeros_like(t) for t in q]
        torch.cuda.synchronize()
        bs.sync()
        l0, s0 = counts(lib)
        check(acc.direction(q, [1.0] * n_blocks, d))
        l1, s1 = counts(lib)
        bs.sync()
        assert s1 - s0 == 0
        launches[n_blocks] = l1 - l0
        acc.close()
    assert launches[1] == launches[3] == 2 * 3 + 1


def test_more_items_than_workgroups(lib, bs):
    """Blocks of 1025 x 400 and 2049 x 90 (NaN-padded): 800 + 270 = 1070 work items behind the 1024 workgroups of a launch, so
    46 workgroups walk two items (``it += gridDim.x``) and the partial buffers are full (four partials per thread when the
    next launch sums them).  Memory 2, three updates (two pairs) and a direction with the preconditioner on, against the
    longdouble twin under the bounds of ``run_case``: the two-item walk adds <= 4 sequential additions per thread to an inner
    product, which the 64 in front of both bounds covers (4 + 4 per thread, a wave tree of 6, the wave sums 2, then the
    partials: under 32 roundings on the device)."""
    shapes, memory, scale = [(1025, 400), (2049, 90)], 2, [0.25, 1.5]
    assert sum(c * -(-r // 1024) for r, c in shapes) == 1070
    rng = np.random.default_rng(7)
    pairs = [kblock(lib, bs, r) for r, _ in shapes]
    kbs, kin = [p[0] for p in pairs], [p[1] for p in pairs]
    mks = [0.3 + 2.0 * rng.random(c) for _, c in shapes]
    acc = Acc(lib, bs, shapes, memory)
    ref, f64 = twin.LbfgsTwin(memory), twin.LbfgsTwin(memory, real=np.float64)
    try:
        for n_upd, (x, g) in enumerate(points(rng, shapes, 3), start=1):
            xd = [padded(a, 3 + b) for b, a in enumerate(x)]
            gd = [padded(a, 5 + b) for b, a in enumerate(g)]
            torch.cuda.synchronize()
            sy, kept = acc.update(xd, gd)
            sy_ref, kept_ref = ref.update(x, g)
            sy_64, _ = f64.update(x, g)
            assert kept == int(kept_ref) and acc.history == len(ref.pairs) == n_upd - 1
            if n_upd > 1:
                s, y, _ = ref.pairs[-1]
                floor = 64 * EPS * float(sum(np.abs(a.real * b.real + a.imag * b.imag).sum() for a, b in zip(s, y)))
                bound = max(64 * abs(sy_64 - sy_ref), floor)
                print(f"\nlbfgs 1070 items: <s, y> err / bound {abs(sy - sy_ref) / bound:.3g}", end="")
                assert abs(sy - sy_ref) <= bound, (n_upd, sy, sy_ref, bound)
        q = [crandn(rng, s) for s in shapes]
        qd = [padded(a, 2 + b) for b, a in enumerate(q)]
        dd = [padded(np.zeros(s, dtype=complex), 4 + b) for b, s in enumerate(shapes)]
        torch.cuda.synchronize()
        check(acc.direction(qd, scale, dd, kbs, mks))
        bs.sync()
        got = [unpad(t, s[0]) for t, s in zip(dd, shapes)]
        want = ref.direction(q, scale, kin, mks)
        w64 = f64.direction(q, scale, kin, mks)
        err = max(float(np.abs(a - b).max()) for a, b in zip(got, want))
        e64 = max(float(np.abs(a.astype(twin.CLD) - b).max()) for a, b in zip(w64, want))
        bound = max(64 * e64, (2 * memory + 2) * EPS * max(ref.peak_q / min(scale), ref.peak_r))
        print(f"\nlbfgs 1070 items: direction err / bound {err / bound:.3g}")
        assert err <= bound, (err, bound)
    finally:
        acc.close()


def test_ring_wraps_with_copies_still_queued(lib, bs):
    """five ``direction`` calls in a row, five different g and mean kinetic energies, nothing waited for in between: the two
    parameter buffers are each reused while earlier copies may still be queued.  Every d equals, bit for bit, the d of the
    same call made alone (the stream idle before and after)."""
    shapes, scale = [(1025, 3), (513, 5)], [0.25, 1.5]
    rng = np.random.default_rng(8)
    kbs = [kblock(lib, bs, r)[0] for r, _ in shapes]
    acc = Acc(lib, bs, shapes, 2)
    try:
        for x, g in points(rng, shapes, 3):
            acc.update([padded(a, 1) for a in x], [padded(a, 2) for a in g])
        assert acc.history == 2
        calls = [([padded(crandn(rng, s), 1 + b) for b, s in enumerate(shapes)], [0.3 + 2.0 * rng.random(c) for _, c in shapes])
                 for _ in range(5)]
        fresh = lambda: [padded(np.zeros(s, dtype=complex), 2 + b) for b, s in enumerate(shapes)]     # noqa: E731
        row = [fresh() for _ in calls]
        torch.cuda.synchronize()
        bs.sync()
        for (q, mk), d in zip(calls, row):
            check(acc.direction(q, scale, d, kbs, mk))
        bs.sync()
        for (q, mk), d in zip(calls, row):
            alone = fresh()
            torch.cuda.synchronize()
            check(acc.direction(q, scale, alone, kbs, mk))
            bs.sync()
            for a, b, s in zip(d, alone, shapes):
                u, v = unpad(a, s[0]), unpad(b, s[0])
                assert np.isfinite(u).all() and np.array_equal(u.view(np.float64).view(np.int64), v.view(np.float64).view(np.int64))
        assert len({unpad(d[0], shapes[0][0]).tobytes() for d in row}) == 5       # the five calls are different calls
    finally:
        acc.close()


# ------------------------------------------------------------------------------------------ the tangent projection
@pytest.mark.parametrize("n,m", [(1, 1), (65, 3), (1025, 4), (4097, 33)])
def test_stiefel_project_tangent(lib, bs, n, m):
    rng = np.random.default_rng(n + m)
    x = twin.polar_retract(crandn(rng, (n, m)))
    g = crandn(rng, (n, m))
    xd, gd = padded(x, 3), padded(g, 6)
    torch.cuda.synchronize()
    check(lib.dftk_mi_stiefel_project_tangent(bs.h, n, m, xd.data_ptr(), n + 3, gd.data_ptr(), n + 6))
    bs.sync()
    once = unpad(gd, n)
    want = twin.project_tangent(g.astype(twin.CLD), x.astype(twin.CLD))
    # the zgemm's bound: x'g is a sum of n products, the update one of m
    gemm = 8 * (n + m) * EPS * float(np.abs(x).max() * np.abs(g).max() + np.abs(g).max())
    err = float(np.abs(once - want).max())
    skew = float(np.abs(x.conj().T @ once + once.conj().T @ x).max())
    check(lib.dftk_mi_stiefel_project_tangent(bs.h, n, m, xd.data_ptr(), n + 3, gd.data_ptr(), n + 6))
    bs.sync()
    twice = float(np.abs(unpad(gd, n) - once).max())
    print(f"\nproject_tangent {n} x {m}: err {err:.2e}, |x'g + g'x| {skew:.2e}, twice - once {twice:.2e}, bound {gemm:.2e}")
    assert err <= gemm and skew <= gemm and twice <= gemm
    assert np.array_equal(unpad(xd, n), x)


# ------------------------------------------------------------------------------------------ refusals, lifetimes
def test_einval_leaves_the_outputs_untouched(lib, bs):
    one_r, one_c = (C.c_int64 * 1)(64), (C.c_int * 1)(2)
    h = C.c_void_p(0x5A5A)
    for args in ((bs.h, 0, one_r, one_c, 2), (bs.h, 1, one_r, one_c, 0), (bs.h, 1, (C.c_int64 * 1)(0), one_c, 2),
                 (bs.h, 1, one_r, (C.c_int * 1)(0), 2), (None, 1, one_r, one_c, 2)):
        assert lib.dftk_mi_lbfgs_create(*args, C.byref(h)) == EINVAL and h.value == 0x5A5A
    shapes = block_shapes(64, 2, 2)
    kb_ok = [kblock(lib, bs, r)[0] for r, _ in shapes]
    kb_bad = [kblock(lib, bs, 65)[0], kb_ok[1]]
    acc = Acc(lib, bs, shapes, 2)
    rng = np.random.default_rng(8)
    x = [padded(crandn(rng, s), 2) for s in shapes]
    g = [padded(crandn(rng, s), 2) for s in shapes]
    acc.update(x, g)
    sy, kept = C.c_double(-7.0), C.c_int(-7)
    xp, xl = acc.tables(x)
    gp, gl = acc.tables(g)
    short = (C.c_int64 * 2)(shapes[0][0], shapes[1][0] - 1)
    null = (C.c_void_p * 2)(x[0].data_ptr(), None)
    for a in ((xp, short, gp, gl), (xp, xl, gp, short), (null, xl, gp, gl), (xp, xl, null, gl)):
        assert lib.dftk_mi_lbfgs_update(acc.h, *a, C.byref(sy), C.byref(kept)) == EINVAL
        assert (sy.value, kept.value, acc.history) == (-7.0, -7, 0)
    poison = complex(7.0, -7.0)
    d = [torch.full_like(t, poison) for t in g]
    dp, dl = acc.tables(d)
    sc, bad_sc = (C.c_double * 2)(1.0, 1.0), (C.c_double * 2)(1.0, 0.0)
    mk = [np.ones(c) for _, c in shapes]
    mkp = (C.c_void_p * 2)(*[m.ctypes.data for m in mk])
    kbp = (C.c_void_p * 2)(*[k.h.value for k in kb_ok])
    kbp_bad = (C.c_void_p * 2)(*[k.h.value for k in kb_bad])
    for a in ((gp, short, None, None, sc, dp, dl), (gp, gl, None, None, sc, dp, short), (gp, gl, None, None, bad_sc, dp, dl),
              (gp, gl, kbp_bad, mkp, sc, dp, dl), (gp, gl, kbp, None, sc, dp, dl), (gp, gl, None, None, sc, gp, gl),
              (null, gl, None, None, sc, dp, dl)):
        assert lib.dftk_mi_lbfgs_direction(acc.h, *a) == EINVAL
    bs.sync()
    assert all(bool((t == poison).all()) for t in d)
    assert lib.dftk_mi_lbfgs_direction(acc.h, gp, gl, kbp, mkp, sc, dp, dl) == 0       # the valid call goes through
    bs.sync()
    assert all(bool(torch.isfinite(torch.view_as_real(t)[:, :s[0]]).all()) for t, s in zip(d, shapes))
    # the tangent projection
    t = torch.full((2, 66), poison, dtype=torch.complex128, device="cuda")
    for a in ((0, 2, x[0].data_ptr(), 66, t.data_ptr(), 66), (64, 0, x[0].data_ptr(), 66, t.data_ptr(), 66),
              (64, 2, x[0].data_ptr(), 63, t.data_ptr(), 66), (64, 2, x[0].data_ptr(), 66, t.data_ptr(), 63),
              (64, 2, t.data_ptr(), 66, t.data_ptr(), 66), (64, 2, None, 66, t.data_ptr(), 66)):
        assert lib.dftk_mi_stiefel_project_tangent(bs.h, *a) == EINVAL
    bs.sync()
    assert bool((t == poison).all())
    acc.close()


def live(lib):
    n, b = C.c_int64(), C.c_int64()
    check(lib.dftk_mi_device_buffers_live(C.byref(n), C.byref(b)))
    return n.value, b.value


def test_destroy_releases_every_buffer(lib, bs):
    """``dftk_mi_device_buffers_live`` is process-wide: handles of earlier tests that the interpreter has not collected yet
    are collected first, and the collector is off between the readings, so that only this handle moves the count"""
    import gc
    shapes = block_shapes(1025, 3, 2)
    per_vec = sum(r * c for r, c in shapes) * 16
    gc.collect()
    gc.disable()
    try:
        n0, b0 = live(lib)
        acc = Acc(lib, bs, shapes, 2)
        n1, b1 = live(lib)
        assert n1 > n0 and b1 - b0 >= (2 * 2 + 4) * per_vec          # memory + 1 slots of (s, y), x_prev, g_prev
        rng = np.random.default_rng(9)
        for x, g in points(rng, shapes, 4):                          # no call allocates after creation
            acc.update([dev(a.T.copy()) for a in x], [dev(a.T.copy()) for a in g])
        q = [dev(crandn(rng, s).T.copy()) for s in shapes]
        d = [torch.zeros_like(t) for t in q]
        torch.cuda.synchronize()
        check(acc.direction(q, [1.0, 1.0], d))
        bs.sync()
        assert live(lib) == (n1, b1)
        acc.close()
        assert live(lib) == (n0, b0)
    finally:
        gc.enable()
