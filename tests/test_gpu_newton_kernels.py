"""The entries of csrc/newton_kernels.hip at the C ABI (ctypes, device memory from torch).

A. ``dftk_mi_orbitals_realspace``, ``dftk_mi_tangent_density``, ``dftk_mi_tangent_potential`` against a longdouble separable
   dense DFT written here (three small matrices per cube; the cubes are small).  Cubes with axes mixed from 8, 9, 12, 15
   (8: radix 8 / 4.2, 9 = 3.3, 12 = 4.3, 15 = 5.3; all three axes different, so swapped strides change the result); Gamma
   and the generic k-point [1/3, 0.1, -0.25]; 1, 3 and 65 bands (65 = 2 x 32 + 1 = 8 x 8 + 1: full launch groups and a ragged last one of one band);
   every block with a leading dimension above n_G and NaN in the padding; weights with zeros (for 65 bands also bands 32 .. 63: whole
   launch groups, which are skipped); ``accumulate`` 0 and 1; a Gamma-real block.
   Bound, the project's convention: 64 x the error of the float64 NumPy twin of the same formula (the same dense DFT in
   float64) against the longdouble values, measured here and printed; 64 eps max|ref| if that error is 0.  The existing
   ``dftk_mi_density_response_accumulate`` (w_docc = 0) and the ``which = 1`` apply of a block with dV bound must meet the
   same bound on the same inputs.
B. ``dftk_mi_tangent_cg_*`` against the longdouble twin of tests/newton_twin.py: rows 1, 63 / 64 / 65 (the wave), 1023 /
   1025 (the work item of 1024 rows: the last forces a second, one-row item), 4097 (five items per column); 1, 3, 33
   columns; 1 to 3 blocks of unequal rows, columns and weights behind one grid, every block padded with NaN; three chained
   iterations on the device.  Every call is compared with the twin applied to the vectors the device had before that call, so
   each bound is that of ONE operation, from its operation count (written beside the assertion).

The refusal "inside a batched multi-k call" cannot be reached through the ABI (``dftk_mi_batch_replay`` takes enumerated
operations only); the other refusals are all here.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import ALLREDUCE_FN, check  # noqa: E402

import newton_twin as twin  # noqa: E402
from test_gpu_kernels import Basis, KBlock, dev, make_oracle_basis  # noqa: E402

EPS = 2.0 ** -52
EINVAL = -1                           # DFTK_MI_EINVAL
LD = np.longdouble
CLD = np.clongdouble
ECUT = 2.5                            # the sphere of every k-point fits the smallest axis (8: |G| <= 3)
CUBES = [(8, 9, 12), (15, 12, 9), (9, 15, 8), (12, 8, 15)]
BANDS = [1, 3, 65]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


def counts(lib):
    a, b = C.c_int64(), C.c_int64()
    check(lib.dftk_mi_launch_count(C.byref(a), C.byref(b)))
    return a.value, b.value


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


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


def bits(t):
    return torch.view_as_real(t).contiguous().view(torch.int64) if t.is_complex() else t.contiguous().view(torch.int64)


# =========================================================================================== A: the transform side
_PI = LD("3.14159265358979323846264338327950288419716939937510")


def dft_matrix(n, sign, real):
    """W[x, i] = exp(sign 2 pi i x i / n); the angle is reduced exactly in integers before it is scaled"""
    k = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    if real is LD:
        ang = 2 * _PI * k.astype(LD) / LD(n)
        return (np.cos(ang) + 1j * sign * np.sin(ang)).astype(CLD)
    ang = 2 * np.pi * k.astype(np.float64) / n
    return np.cos(ang) + 1j * sign * np.sin(ang)


def transform(cubes, fft_size, sign, real):
    """the unnormalised 3-D DFT of (nb, nz, ny, nx) cubes with exp(sign 2 pi i ...), axis by axis with dense matrices"""
    nx, ny, nz = fft_size
    t = np.einsum("xm,bklm->bklx", dft_matrix(nx, sign, real), cubes)
    t = np.einsum("yl,bklx->bkyx", dft_matrix(ny, sign, real), t)
    return np.einsum("zk,bkyx->bzyx", dft_matrix(nz, sign, real), t)


def formulas(fft_size, mapping, psi, dpsi, w, drho0, dV, out0, real):
    """the three quantities in the precision ``real``: psi_n(r); drho0 + sum_n w_n 2 Re[conj psi_n(r) dpsi_n(r)]; the sphere
    rows of FFT(dV psi_n(r)) / N, alone and added to out0"""
    nx, ny, nz = fft_size
    N = nx * ny * nz
    ct = CLD if real is LD else np.complex128

    def cubes_of(c):
        full = np.zeros((c.shape[1], N), dtype=ct)
        full[:, mapping] = c.T.astype(ct)
        return transform(full.reshape(-1, nz, ny, nx), fft_size, +1, real)
    pr, dr = cubes_of(psi), cubes_of(dpsi)
    drho = drho0.astype(real)
    for n in range(psi.shape[1]):                  # ascending bands, as the kernel sums them
        drho = drho + real(w[n]) * 2 * (pr[n].real * dr[n].real + pr[n].imag * dr[n].imag)
    prod = dV.astype(real)[None] * pr
    coef = (transform(prod, fft_size, -1, real).reshape(-1, N)[:, mapping] / real(N)).T
    return pr, drho, coef, out0.astype(ct) + coef


def bound_of(f64, ref, what):
    err = float(np.abs(f64.astype(CLD if np.iscomplexobj(ref) else LD) - ref).max())
    b = 64 * err if err > 0 else 64 * EPS * float(np.abs(ref).max())
    assert b > 0, what
    return b, err


_BASES = {}


def device_block(lib, fft_size, ik):
    if (fft_size, ik) not in _BASES:
        ob = make_oracle_basis(ECUT, fft_size, terms=("Kinetic",))
        if fft_size not in _BASES:
            _BASES[fft_size] = Basis(lib, *fft_size, ob.model.unit_cell_volume)
        kpt = ob.kpoints[ik]
        G = np.stack([kpt.mapping % fft_size[0], (kpt.mapping // fft_size[0]) % fft_size[1],
                      kpt.mapping // (fft_size[0] * fft_size[1])], axis=1)
        for a in range(3):                         # no Nyquist point: every |G_a| <= (n_a - 1) // 2
            g = np.where(G[:, a] > fft_size[a] // 2, G[:, a] - fft_size[a], G[:, a])
            assert np.abs(g).max() <= (fft_size[a] - 1) // 2
        _BASES[(fft_size, ik)] = (_BASES[fft_size], KBlock(lib, _BASES[fft_size], kpt.mapping, np.zeros(len(kpt.mapping))),
                                  np.asarray(kpt.mapping))
    return _BASES[(fft_size, ik)]


def weights_for(nb, rng):
    w = 0.2 + rng.random(nb)
    if nb == 3:
        w[1] = 0.0                                 # a dead band inside a live group
    if nb == 65:
        w[32:64] = 0.0                             # whole launch groups (one of 32 bands, four of 8): skipped
        w[5] = 0.0
    return w * np.where(np.arange(nb) % 4 == 3, -1.0, 1.0)


def run_transform_case(lib, fft_size, ik, nb, gamma_real=False):
    bs, kb, mapping = device_block(lib, fft_size, ik)
    nx, ny, nz = fft_size
    n = len(mapping)
    rng = np.random.default_rng(1000 * nx + 100 * nz + 10 * nb + ik)
    psi, dpsi, out0 = crandn(rng, n, nb), crandn(rng, n, nb), crandn(rng, n, nb)
    w = weights_for(nb, rng)
    drho0, dV = rng.standard_normal((nz, ny, nx)), rng.standard_normal((nz, ny, nx))
    ref = formulas(fft_size, mapping, psi, dpsi, w, drho0, dV, out0, LD)
    f64 = formulas(fft_size, mapping, psi, dpsi, w, drho0, dV, out0, np.float64)
    names = ("psi_r", "drho", "dV psi", "out0 + dV psi")
    bounds = [bound_of(a, b, k) for a, b, k in zip(f64, ref, names)]
    if gamma_real:
        check(lib.dftk_mi_kblock_set_gamma_real(kb.h, 1))
    try:
        pd, dd = padded(psi, 5), padded(dpsi, 9)
        psi_r = torch.full((nb, nz, ny, nx), float("nan"), dtype=torch.complex128, device="cuda")
        drho = dev(drho0)
        dVd = dev(dV)
        o_new, o_acc = padded(np.full((n, nb), complex(np.nan, np.nan)), 3), padded(out0, 7)
        wh = np.ascontiguousarray(w)

        def calls(psi_r, drho, o_new, o_acc):
            check(lib.dftk_mi_orbitals_realspace(kb.h, nb, pd.data_ptr(), n + 5, psi_r.data_ptr()))
            check(lib.dftk_mi_tangent_density(kb.h, nb, psi_r.data_ptr(), dd.data_ptr(), n + 9, wh.ctypes.data, drho.data_ptr()))
            check(lib.dftk_mi_tangent_potential(kb.h, nb, psi_r.data_ptr(), dVd.data_ptr(), o_new.data_ptr(), n + 3, 0))
            check(lib.dftk_mi_tangent_potential(kb.h, nb, psi_r.data_ptr(), dVd.data_ptr(), o_acc.data_ptr(), n + 7, 1))
        torch.cuda.synchronize()
        calls(psi_r, drho, o_new, o_acc)           # (the first call may grow the workspace)
        bs.sync()
        again = [torch.full_like(psi_r, float("nan")), dev(drho0), padded(np.full((n, nb), complex(np.nan, np.nan)), 3),
                 padded(out0, 7)]
        torch.cuda.synchronize()
        l0, s0 = counts(lib)
        calls(*again)
        l1, s1 = counts(lib)
        assert s1 == s0 and l1 > l0                # asynchronous: no host synchronisation in any of the three entries
        bs.sync()
        for a, b in zip((psi_r, drho, o_new, o_acc), again):             # two calls: bitwise identical
            assert torch.equal(bits(a), bits(b))
        got = (psi_r.cpu().numpy(), drho.cpu().numpy(), unpad(o_new, n), unpad(o_acc, n))
        # the existing entries on the same inputs
        old_drho = dev(drho0)
        zeros = np.zeros(nb)
        check(lib.dftk_mi_density_response_accumulate(kb.h, nb, pd.data_ptr(), n + 5, dd.data_ptr(), n + 9, wh.ctypes.data,
                                                      zeros.ctypes.data, old_drho.data_ptr()))
        bs.sync()
        kb.set_potential(dV)
        old_apply = kb.apply(psi, which=1)
        check(lib.dftk_mi_kblock_set_potential(kb.h, None))
        bs.sync()
    finally:
        if gamma_real:
            check(lib.dftk_mi_kblock_set_gamma_real(kb.h, 0))
    report = {}
    for name, g, r, (bound, err64) in zip(names, got, ref, bounds):
        err = float(np.abs(g - r).max())
        report[name] = (err, err64, bound)
        assert np.isfinite(g).all() and err <= bound, (name, fft_size, ik, nb, err, err64, bound)
    for name, g, r, (bound, _) in (("density_response_accumulate", old_drho.cpu().numpy(), ref[1], bounds[1]),
                                   ("apply_H_parts(which = 1)", old_apply, ref[2], bounds[2])):
        err = float(np.abs(g - r).max())
        report[name] = (err, None, bound)
        assert err <= bound, (name, fft_size, ik, nb, err, bound)
    print(f"\n{fft_size} k{ik} {nb} bands: " + ", ".join(f"{k}: err {v[0]:.2e} (float64 twin {v[1] if v[1] is None else format(v[1], '.2e')}, "
                                                           f"bound {v[2]:.2e})" for k, v in report.items()))


@pytest.mark.parametrize("nb", BANDS)
@pytest.mark.parametrize("ik", [0, 1])
@pytest.mark.parametrize("fft_size", CUBES)
def test_transform_entries_against_the_longdouble_dft(lib, fft_size, ik, nb):
    run_transform_case(lib, fft_size, ik, nb)


def test_transform_entries_on_a_gamma_real_block(lib):
    """accepted and served in the complex full-sphere layout: general complex vectors, the same numbers as with the switch off"""
    run_transform_case(lib, (9, 15, 8), 0, 3, gamma_real=True)


def test_transform_entries_refuse_and_write_nothing(lib):
    fft_size = (8, 9, 12)
    bs, kb, mapping = device_block(lib, fft_size, 1)
    nx, ny, nz = fft_size
    n, nb = len(mapping), 3
    rng = np.random.default_rng(3)
    pd, dd = padded(crandn(rng, n, nb), 0), padded(crandn(rng, n, nb), 0)
    w = np.ones(nb)
    dVd = dev(rng.standard_normal((nz, ny, nx)))
    cube = torch.full((nb, nz, ny, nx), float("nan"), dtype=torch.complex128, device="cuda")
    drho = torch.full((nz, ny, nx), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((nb, n), float("nan"), dtype=torch.complex128, device="cuda")
    psi_r = torch.zeros((nb, nz, ny, nx), dtype=torch.complex128, device="cuda")
    before = [t.clone() for t in (cube, drho, out)]

    def three(k, m, ld, word):
        for st in (lib.dftk_mi_orbitals_realspace(k, m, pd.data_ptr(), ld, cube.data_ptr()),
                   lib.dftk_mi_tangent_density(k, m, psi_r.data_ptr(), dd.data_ptr(), ld, w.ctypes.data, drho.data_ptr()),
                   lib.dftk_mi_tangent_potential(k, m, psi_r.data_ptr(), dVd.data_ptr(), out.data_ptr(), ld, 0)):
            assert st == EINVAL and word in lib.dftk_mi_last_error().decode(), (word, lib.dftk_mi_last_error())
    three(kb.h, nb, n - 1, "leading dimension")
    three(kb.h, -1, n, "negative")
    three(None, nb, n, "null")
    assert lib.dftk_mi_orbitals_realspace(kb.h, nb, None, n, cube.data_ptr()) == EINVAL
    assert lib.dftk_mi_tangent_density(kb.h, nb, psi_r.data_ptr(), dd.data_ptr(), n, None, drho.data_ptr()) == EINVAL
    assert lib.dftk_mi_tangent_density(kb.h, nb, psi_r.data_ptr(), dd.data_ptr(), n, w.ctypes.data, None) == EINVAL
    assert lib.dftk_mi_tangent_potential(kb.h, nb, psi_r.data_ptr(), None, out.data_ptr(), n, 0) == EINVAL
    # a block sharded over two ranks (the communicator is never used: the call is refused before any work)
    kb2 = KBlock(lib, bs, mapping, np.zeros(n))
    cb = ALLREDUCE_FN(lambda user, data, count: 0)
    comm = C.c_void_p()
    check(lib.dftk_mi_comm_create_host(2, 0, 0, cb, None, None, C.byref(comm)))
    rows = np.array([0, n // 2, n], dtype=np.int64)
    check(lib.dftk_mi_kblock_set_shard(kb2.h, comm, rows.ctypes.data))
    three(kb2.h, nb, n, "sharded")
    check(lib.dftk_mi_kblock_set_shard(kb2.h, None, None))
    check(lib.dftk_mi_comm_destroy(comm))
    # n_bands = 0: a no-op
    check(lib.dftk_mi_orbitals_realspace(kb.h, 0, None, 0, None))
    check(lib.dftk_mi_tangent_density(kb.h, 0, None, None, 0, None, None))
    check(lib.dftk_mi_tangent_potential(kb.h, 0, None, None, None, 0, 1))
    bs.sync()
    for t, t0 in zip((cube, drho, out), before):
        assert torch.equal(bits(t), bits(t0))      # no refused call wrote anything


# =========================================================================================== B: the CG pieces
ROWS = [1, 63, 64, 65, 1023, 1025, 4097]
COLS = [1, 3, 33]


def block_shapes(rows, cols, n_blocks):
    return [(rows, cols), (rows // 2 + 1, cols + 2), (rows + 7, max(1, cols - 1))][:n_blocks]


class Cg:
    def __init__(self, lib, bs, shapes, weights):
        self.lib, self.shapes, self.n = lib, shapes, len(shapes)
        self.h = C.c_void_p()
        rows = (C.c_int64 * self.n)(*[r for r, _ in shapes])
        cols = (C.c_int * self.n)(*[c for _, c in shapes])
        w = (C.c_double * self.n)(*weights)
        check(lib.dftk_mi_tangent_cg_create(bs.h, self.n, rows, cols, w, C.byref(self.h)))

    def tables(self, blocks):
        return ((C.c_void_p * self.n)(*[b.data_ptr() for b in blocks]), (C.c_int64 * self.n)(*[b.stride(0) for b in blocks]))

    def dot(self, slot, a, b):
        return self.lib.dftk_mi_tangent_cg_dot(self.h, slot, *self.tables(a), *self.tables(b))

    def update_xr(self, p, c, x, r):
        return self.lib.dftk_mi_tangent_cg_update_xr(self.h, *self.tables(p), *self.tables(c), *self.tables(x), *self.tables(r))

    def update_p(self, z, p, first=0):
        return self.lib.dftk_mi_tangent_cg_update_p(self.h, *self.tables(z), *self.tables(p), first)

    def read(self):
        out = (C.c_double * 3)(-7.0, -7.0, -7.0)
        check(self.lib.dftk_mi_tangent_cg_read(self.h, out))
        return [float(v) for v in out]

    def close(self):
        if self.h:
            check(self.lib.dftk_mi_tangent_cg_destroy(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def abs_terms(a, b, w):
    """sum_b w_b sum |Re a Re b| + |Im a Im b|: what the rounding of an inner product scales with"""
    return float(sum(abs(wb) * (np.abs(x.real * y.real) + np.abs(x.imag * y.imag)).sum() for x, y, wb in zip(a, b, w)))


def vmax(v):
    return max(float(np.abs(np.asarray(b, dtype=complex)).max()) for b in v)


def vdiff(a, b):
    return max(float(np.abs(np.asarray(x).astype(CLD) - np.asarray(y).astype(CLD)).max()) for x, y in zip(a, b))


def run_cg_case(lib, bs, rows, cols, n_blocks, shapes=None, n_steps=3):
    shapes = shapes or block_shapes(rows, cols, n_blocks)
    w = [0.25, 0.5, 1.5][:n_blocks]
    rng = np.random.default_rng(1000 * rows + 10 * cols + n_blocks)
    rnd = lambda: [crandn(rng, r, c) for r, c in shapes]                               # noqa: E731
    host = dict(x=rnd(), r=rnd(), z0=rnd())
    steps = [dict(c=rnd(), z=rnd()) for _ in range(n_steps)]
    worst = {}

    def note(key, err, bound):
        worst[key] = max(worst.get(key, 0.0), err / bound)
        assert err <= bound, (key, rows, cols, n_blocks, err, bound)

    def run():
        cg = Cg(lib, bs, shapes, w)
        log = []
        try:
            up = lambda v, pad: [padded(a, pad + b) for b, a in enumerate(v)]          # noqa: E731
            down = lambda v: [unpad(t, s[0]) for t, s in zip(v, shapes)]                 # noqa: E731
            x, r, z0 = up(host["x"], 3), up(host["r"], 5), up(host["z0"], 2)
            p = [padded(np.full(s, complex(np.nan, np.nan)), 4 + b) for b, s in enumerate(shapes)]
            torch.cuda.synchronize()
            l0, s0 = counts(lib)
            check(cg.dot(twin.GAMMA, r, z0))
            check(cg.dot(twin.RR, r, r))
            check(cg.update_p(z0, p, 1))
            l1, s1 = counts(lib)
            assert s1 == s0 and l1 == l0 + 3           # one launch each, no host synchronisation
            rd = cg.read()
            l2, s2 = counts(lib)
            assert s2 == s1 + 1 and l2 == l1 + 1       # exactly one host synchronisation per read
            log.append(dict(kind="init", read=rd, p=down(p)))
            for st in steps:
                c, z = up(st["c"], 1), up(st["z"], 6)
                before = dict(p=down(p), x=down(x), r=down(r))
                torch.cuda.synchronize()
                l0, s0 = counts(lib)
                check(cg.dot(twin.PC, p, c))
                check(cg.update_xr(p, c, x, r))
                check(cg.dot(twin.RR, r, r))
                check(cg.dot(twin.GAMMA, r, z))
                l1, s1 = counts(lib)
                assert s1 == s0 and l1 == l0 + 4
                bs.sync()
                mid = dict(x=down(x), r=down(r))
                torch.cuda.synchronize()
                l0, s0 = counts(lib)
                check(cg.update_p(z, p))
                l1, s1 = counts(lib)
                assert s1 == s0 and l1 == l0 + 1
                rd = cg.read()
                assert counts(lib)[1] == s1 + 1
                log.append(dict(kind="step", before=before, mid=mid, p=down(p), read=rd))
        finally:
            cg.close()
        return log

    log = run()
    # ---- the start: p = z0 bit for bit, <r, r> and gamma = <r, z0>
    assert all(np.array_equal(a, b) for a, b in zip(log[0]["p"], host["z0"]))
    ref = twin.CgScalars(w)
    g = ref.dot(twin.GAMMA, host["r"], host["z0"])
    rr = ref.dot(twin.RR, host["r"], host["r"])
    ref.update_p(host["z0"], None, first=True)
    # an inner product: <= 4 sequential additions of two products per thread and item, a wave tree (6), four wave sums (2), a
    # few items per workgroup, then <= 4 sequential additions and the same trees over the partials: under 32 roundings, each at
    # most eps times the sum of the absolute terms; 64 eps sum |terms| with the weight's rounding
    dg = 64 * EPS * abs_terms(host["r"], host["z0"], w)
    drr = 64 * EPS * abs_terms(host["r"], host["r"], w)
    note("rr", abs(log[0]["read"][0] - float(rr)), drr)
    note("gamma", abs(log[0]["read"][1] - float(g)), dg)
    assert log[0]["read"][2] == 0.0                    # <p, c> has not been formed yet: the slot is zero from creation
    gamma_dev, gamma_ref, dgamma = log[0]["read"][1], g, dg
    p_prev = host["z0"]
    for st, got in zip(steps, log[1:]):
        b = got["before"]
        assert all(np.array_equal(a, c) for a, c in zip(b["p"], p_prev))
        s = twin.CgScalars(w)
        s.gamma = gamma_ref
        pc = s.dot(twin.PC, b["p"], st["c"])
        x_ref, r_ref = s.update_xr(b["p"], st["c"], b["x"], b["r"])
        dpc = 64 * EPS * abs_terms(b["p"], st["c"], w)
        # alpha = gamma / <p, c>: the relative errors of both sums add, one more rounding for the quotient; x + alpha p and
        # r - alpha c are one fused multiply-add each (one rounding of the result)
        dalpha = abs(float(s.alpha)) * (dgamma / abs(float(gamma_ref)) + dpc / abs(float(pc)) + 2 * EPS)
        note("x", vdiff(got["mid"]["x"], x_ref), dalpha * vmax(b["p"]) + 2 * EPS * vmax(x_ref))
        note("r", vdiff(got["mid"]["r"], r_ref), dalpha * vmax(st["c"]) + 2 * EPS * vmax(r_ref))
        # the sums that follow are taken over the DEVICE's r
        r_dev = got["mid"]["r"]
        rr = s.dot(twin.RR, r_dev, r_dev)
        g_next = s.dot(twin.GAMMA, r_dev, st["z"])
        dg_next = 64 * EPS * abs_terms(r_dev, st["z"], w)
        p_ref = s.update_p(st["z"], b["p"])
        # beta = gamma_next / gamma: as alpha; z + beta p is one fused multiply-add
        dbeta = abs(float(s.beta)) * (dg_next / abs(float(g_next)) + dgamma / abs(float(gamma_ref)) + 2 * EPS)
        note("p", vdiff(got["p"], p_ref), dbeta * vmax(b["p"]) + 2 * EPS * vmax(p_ref))
        note("rr", abs(got["read"][0] - float(rr)), 64 * EPS * abs_terms(r_dev, r_dev, w))
        note("gamma", abs(got["read"][1] - float(g_next)), dg_next)
        note("pc", abs(got["read"][2] - float(pc)), dpc)
        gamma_ref, dgamma, p_prev = g_next, dg_next, got["p"]
    # ---- two runs: bitwise identical
    log2 = run()
    for a, b in zip(log, log2):
        assert a["read"] == b["read"] and all(np.array_equal(u, v) for u, v in zip(a["p"], b["p"]))
        if a["kind"] == "step":
            assert all(np.array_equal(u, v) for k in ("x", "r") for u, v in zip(a["mid"][k], b["mid"][k]))
    return worst


@pytest.fixture(scope="module")
def bs(lib):
    return Basis(lib, 8, 9, 12, 1.0)


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_cg_pieces_against_the_longdouble_twin(lib, bs, rows, cols):
    worst = {}
    for n_blocks in (1, 2, 3):
        for k, v in run_cg_case(lib, bs, rows, cols, n_blocks).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f"\ntangent CG {rows} x {cols}, 1-3 blocks: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_cg_pieces_with_more_items_than_workgroups(lib, bs):
    """Blocks of 1025 x 400 and 2049 x 90 (NaN-padded): 800 + 270 = 1070 work items behind the 1024 workgroups of a launch, so
    46 workgroups walk two items (``it += gridDim.x``) and every partial buffer is full: ``sum_partials`` adds four partials
    per thread.  ``dot`` into all three slots, ``update_xr``, ``update_p`` and ``read`` for one iteration against the
    longdouble twin, under the bounds of ``run_cg_case``.  Their operation count at this shape: a term of an inner product
    passes its product and the sum of the two products (2 roundings), <= 4 sequential additions per thread and item, the
    weight, <= 2 additions over the items of the workgroup, the wave tree and the four wave sums (6 + 2), then <= 4
    sequential additions over the 1024 partials and the same trees (4 + 6 + 2): 29 roundings, each at most eps times the sum
    of the absolute terms -- within the 64 eps sum |terms| asserted there."""
    shapes = [(1025, 400), (2049, 90)]
    assert sum(c * -(-r // 1024) for r, c in shapes) == 1070
    worst = run_cg_case(lib, bs, 1025, 400, 2, shapes=shapes, n_steps=1)
    print("\ntangent CG, 1070 items on 1024 workgroups: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_cg_ring_wraps_with_copies_still_queued(lib, bs):
    """2 x 8 + 1 = 17 ``dot`` calls into slot RR with 17 different operand pairs and no ``read`` between them: the ring of
    eight parameter buffers wraps twice while copies may still be queued.  17 launches; the only host synchronisations are
    waits the ring itself counted, and the first eight calls find their buffer free: at most 17 - 8.  The value read
    afterwards equals, bit for bit, the one of the 17th dot issued alone on a fresh handle: no call saw the block table of
    another."""
    shapes, w = [(1025, 3), (513, 5)], [0.25, 1.5]
    rng = np.random.default_rng(17)
    vec = lambda pad: [padded(crandn(rng, r, c), pad + b) for b, (r, c) in enumerate(shapes)]     # noqa: E731
    operands = [(vec(1), vec(2)) for _ in range(17)]
    cg, fresh = Cg(lib, bs, shapes, w), Cg(lib, bs, shapes, w)
    try:
        torch.cuda.synchronize()
        bs.sync()
        l0, s0 = counts(lib)
        for a, b in operands:
            check(cg.dot(twin.RR, a, b))
        l1, s1 = counts(lib)
        assert l1 - l0 == 17 and 0 <= s1 - s0 <= 17 - 8, (l1 - l0, s1 - s0)
        got = cg.read()
        check(fresh.dot(twin.RR, *operands[-1]))
        want = fresh.read()
        assert np.float64(got[0]).view(np.int64) == np.float64(want[0]).view(np.int64), (got, want)
        assert got[1:] == [0.0, 0.0] and np.isfinite(got[0]) and got[0] != 0.0
        ref = twin.CgScalars(w).dot(twin.RR, *[[unpad(t, s[0]) for t, s in zip(v, shapes)] for v in operands[-1]])
        bound = 64 * EPS * abs_terms(*[[unpad(t, s[0]) for t, s in zip(v, shapes)] for v in operands[-1]], w)
        assert abs(got[0] - float(ref)) <= bound       # ... and it is the 17th inner product (the bound of run_cg_case)
    finally:
        cg.close()
        fresh.close()


def test_cg_refusals_leave_everything_untouched(lib, bs):
    shapes = block_shapes(65, 3, 2)
    rng = np.random.default_rng(9)
    h = C.c_void_p()
    rows = (C.c_int64 * 2)(65, 33)
    cols = (C.c_int * 2)(3, 5)
    w = (C.c_double * 2)(0.5, 0.5)
    assert lib.dftk_mi_tangent_cg_create(bs.h, 0, rows, cols, w, C.byref(h)) == EINVAL
    assert lib.dftk_mi_tangent_cg_create(bs.h, 2, (C.c_int64 * 2)(65, 0), cols, w, C.byref(h)) == EINVAL
    assert lib.dftk_mi_tangent_cg_create(bs.h, 2, rows, (C.c_int * 2)(3, 0), w, C.byref(h)) == EINVAL
    assert lib.dftk_mi_tangent_cg_create(bs.h, 2, rows, cols, None, C.byref(h)) == EINVAL
    assert lib.dftk_mi_tangent_cg_create(None, 2, rows, cols, w, C.byref(h)) == EINVAL
    assert not h.value
    cg = Cg(lib, bs, shapes, [0.5, 0.5])
    try:
        vec = lambda: [padded(crandn(rng, r, c), 2) for r, c in shapes]                 # noqa: E731
        p, c, x, r = vec(), vec(), vec(), vec()
        check(cg.dot(twin.GAMMA, r, c))
        check(cg.update_p(c, p, 1))
        check(cg.dot(twin.PC, p, c))
        check(cg.dot(twin.RR, r, r))
        good = cg.read()
        keep = [t.clone() for v in (p, c, x, r) for t in v]
        short = [x[0], x[1][:, :shapes[1][0] - 1].contiguous()]                          # a leading dimension below the rows
        assert cg.dot(twin.RR, short, r) == EINVAL and "does not match" in lib.dftk_mi_last_error().decode()
        assert cg.dot(twin.RR, r, short) == EINVAL
        assert cg.dot(3, r, r) == EINVAL and cg.dot(-1, r, r) == EINVAL
        assert cg.update_xr(p, c, short, r) == EINVAL and cg.update_xr(p, c, x, short) == EINVAL
        assert cg.update_xr(short, c, x, r) == EINVAL and cg.update_xr(p, short, x, r) == EINVAL
        assert cg.update_p(short, p) == EINVAL and cg.update_p(c, short) == EINVAL
        null = (C.c_void_p * 2)(x[0].data_ptr(), None)
        lds = (C.c_int64 * 2)(x[0].stride(0), x[1].stride(0))
        assert lib.dftk_mi_tangent_cg_dot(cg.h, twin.RR, null, lds, *cg.tables(r)) == EINVAL
        assert lib.dftk_mi_tangent_cg_dot(cg.h, twin.RR, None, lds, *cg.tables(r)) == EINVAL
        assert lib.dftk_mi_tangent_cg_read(cg.h, None) == EINVAL and lib.dftk_mi_tangent_cg_read(None, (C.c_double * 3)()) == EINVAL
        assert cg.read() == good                       # no refused call changed a slot
        for a, b in zip([t for v in (p, c, x, r) for t in v], keep):
            assert torch.equal(bits(a), bits(b))       # ... or a vector (NaN padding included)
    finally:
        cg.close()
    assert lib.dftk_mi_tangent_cg_destroy(None) == 0
