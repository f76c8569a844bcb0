"""The UPF entry points at the C ABI (ctypes, device memory from torch): dftk_mi_radial_transform against 50-digit sums of
the same weighted integrand, dftk_mi_build_projectors_radial, dftk_mi_atomic_superposition_table and
dftk_mi_forces_local_table against the HGH entries (tables filled from the closed forms) and the NumPy twin of
tests/upf_gen.py.

Bounds.  Radial transform: 8 x max(E_ref, 4 x 2^-52) x scale, E_ref = the twin's own error against the same 50-digit
values (measured on the CPU, printed), scale = 4 pi sum_i |wf_i| r_i^l max|g_l| for kind 0.  Kind 1 is the difference of
two terms that are each rounded relative to their own size, so its scale is 4 pi (sum_i |wf_i| r_i + Zion / q^2
exp(-q^2 / 4)) per q; where the exact value exceeds the largest double (q = 1e-300: -Zion / q^2) the result must be -inf.
Nothing in a bound is measured on the device."""
import ctypes as C
import math

import mpmath as mp
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import psp as psp_mod  # noqa: E402
from dftk_jl_amd import psp_upf  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402

import upf_gen  # noqa: E402

EINVAL = -1
DEV = "cuda:0"
EPS = 2.0 ** -52
mp.mp.dps = 50
RMAX = 40.0
ZION = 4.0


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs(lib):
    from test_gpu_kernels import Basis
    return Basis(lib, 6, 5, 4, 1.0)


# ------------------------------------------------------------------------------------------------ radial transform
def _mesh(kind, n):
    if n == 1:
        return np.array([0.7])
    return upf_gen.log_mesh(n, 1e-5, RMAX) if kind == "log" else upf_gen.uniform_mesh(n, RMAX)


def _wf(r):
    # a weighted integrand with sign changes and the decay of a projector; positive "weights" that vary from point to point
    return (0.5 + 0.25 * (np.arange(len(r)) % 3)) * r * r * np.exp(-0.5 * (r / 3.0) ** 2) * np.cos(3.0 * r + 0.3)


def _distinct_q(mode, rmax):
    qs = [0.0, 1e-300, 5e-16, 1e-8]
    if mode < 4:
        xs = psp_upf.SWITCH_POINTS[mode]
        qs += [np.nextafter(xs, 0.0) / rmax, np.nextafter(xs, 10.0) / rmax, 0.999 * xs / rmax, 1.001 * xs / rmax]
    return np.array(qs + [1.0, 10.0, 60.0])


def _mp_g(l, x):
    """j_l(x) / x^l at 50 digits: the series below 1, the closed form (extra digits for its cancellation) above"""
    if x < 1:
        t = mp.mpf(1) / [1, 3, 15, 105][l]
        h = -x * x / 2
        s, k = mp.mpf(0), 0
        while k == 0 or abs(t) > mp.mpf(10) ** -60:
            s += t
            t *= h / ((k + 1) * (2 * l + 2 * k + 3))
            k += 1
        return s
    with mp.workdps(70):
        sn, cs = mp.sin(x), mp.cos(x)
        if l == 0:
            return sn / x
        if l == 1:
            return (sn - x * cs) / x ** 3
        if l == 2:
            return ((3 - x * x) * sn - 3 * x * cs) / x ** 5
        return ((15 - 6 * x * x) * sn - (15 - x * x) * x * cs) / x ** 7


_REF_CACHE = {}


def _reference(mode, r, wf, q):
    """(50-digit values as mpf, scale per q) for every distinct q, computed once per (mode, mesh)"""
    key = (mode, len(r), float(r[-1]), float(r[0]))
    if key not in _REF_CACHE:
        rm = [mp.mpf(float(v)) for v in r]
        wm = [mp.mpf(float(v)) for v in wf]
        vals, scales = [], []
        for qj in q:
            qm = mp.mpf(float(qj))
            if mode < 4:
                wr = [w * x ** mode for w, x in zip(wm, rm)]
                vals.append(4 * mp.pi * mp.fsum(w * _mp_g(mode, qm * x) for w, x in zip(wr, rm)))
                scales.append(4 * math.pi * float(np.sum(np.abs(wf) * r ** mode)) / [1, 3, 15, 105][mode])
            elif qj == 0:
                vals.append(mp.mpf(0))
                scales.append(0.0)
            else:
                vals.append(4 * mp.pi * (mp.fsum(w * mp.sin(qm * x) for w, x in zip(wm, rm)) / qm
                                         - ZION / qm ** 2 * mp.exp(-qm * qm / 4)))
                scales.append(float(4 * mp.pi * (mp.fsum(abs(w) * x for w, x in zip(wm, rm))
                                                 + ZION / qm ** 2 * mp.exp(-qm * qm / 4))))
        _REF_CACHE[key] = (vals, scales)
    return _REF_CACHE[key]


def _call(lib, bs, kind, l, r, wf, q, out=None):
    r = np.ascontiguousarray(r, dtype=np.float64)
    wf = np.ascontiguousarray(wf, dtype=np.float64)
    qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float64)).to(DEV)
    out = torch.full((len(q),), float("nan"), dtype=torch.float64, device=DEV) if out is None else out
    torch.cuda.synchronize()
    check(lib.dftk_mi_radial_transform(bs.h, kind, l, len(r), r.ctypes.data, wf.ctypes.data, ZION, len(q),
                                       qd.data_ptr(), out.data_ptr()))
    bs.sync()
    return out.cpu().numpy()


def _check_transform(lib, bs, mode, mesh, n_r, n_q):
    r = _mesh(mesh, n_r)
    wf = _wf(r)
    qd = _distinct_q(mode, float(r[-1]))
    vals, scales = _reference(mode, r, wf, qd)
    idx = np.arange(n_q) % len(qd)
    q = qd[idx]
    kind, l = (1, 0) if mode == 4 else (0, mode)
    got = _call(lib, bs, kind, l, r, wf, q)
    again = _call(lib, bs, kind, l, r, wf, q)
    assert not np.any(np.isnan(got)), "output entries left unwritten"
    assert np.array_equal(got, again), "two calls differ"
    twin = (upf_gen.twin_local(r, wf, ZION, qd) if mode == 4 else upf_gen.twin_hankel(r, wf, l, qd))
    big = 1.7976931348623157e308
    worst = 0.0
    for j, (v, sc) in enumerate(zip(vals, scales)):
        mine = got[idx == j]
        if len(mine) == 0:
            continue
        assert np.all(mine == mine[0]), "lanes with the same q disagree"
        if abs(v) > big:
            assert mine[0] == -np.inf and mode == 4, (qd[j], mine[0])
            continue
        if mode == 4 and qd[j] == 0:
            assert mine[0] == 0.0 and not np.signbit(mine[0])
            continue
        e_ref = float(abs(mp.mpf(float(twin[j])) - v)) / sc if sc > 0 else 0.0
        err = float(abs(mp.mpf(float(mine[0])) - v))
        bound = 8 * max(e_ref, 4 * EPS) * sc
        worst = max(worst, err / sc / EPS if sc > 0 else 0.0)
        print(f"mode {mode} {mesh} n_r={n_r} q={qd[j]:.3g}: E_ref {e_ref / EPS:.2f} eps, device {err / sc / EPS if sc else 0:.2f} eps")
        assert err <= bound, (mode, mesh, n_r, qd[j], err, bound)
    return worst


def _n_r_list(lib):
    tile = lib.dftk_mi_radial_tile()
    assert tile >= 64
    return [1, 4, 5, 6, 7, tile - 1, tile, tile + 1, 1141]


@pytest.mark.parametrize("mesh", ["log", "uniform"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_radial_transform_mesh_lengths(lib, bs, mode, mesh):
    for n_r in _n_r_list(lib):
        _check_transform(lib, bs, mode, mesh, n_r, 257)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_radial_transform_q_counts(lib, bs, mode):
    tile = lib.dftk_mi_radial_tile()
    for n_q in (1, 255, 256, 257, 1000):
        _check_transform(lib, bs, mode, "log", tile + 1, n_q)
        _check_transform(lib, bs, mode, "uniform", 7, n_q)


def test_radial_transform_arguments(lib, bs):
    r = _mesh("log", 8)
    wf = _wf(r)
    q = torch.ones(4, dtype=torch.float64, device=DEV)
    out = torch.empty(4, dtype=torch.float64, device=DEV)
    args = lambda **kw: [kw.get("b", bs.h), kw.get("kind", 0), kw.get("l", 0), kw.get("n_r", 8),  # noqa: E731
                         kw.get("r", r.ctypes.data), kw.get("wf", wf.ctypes.data), ZION, 4, kw.get("q", q.data_ptr()),
                         kw.get("out", out.data_ptr())]
    assert lib.dftk_mi_radial_transform(*args()) == 0
    bs.sync()
    for bad in (dict(l=4), dict(l=-1), dict(n_r=0), dict(kind=2), dict(r=None), dict(wf=None), dict(q=None),
                dict(out=None), dict(b=None)):
        assert lib.dftk_mi_radial_transform(*args(**bad)) == EINVAL, bad
    assert lib.dftk_mi_radial_transform(*args(kind=1, l=7)) == 0        # kind 1 ignores l
    bs.sync()


# ------------------------------------------------------------------------------------------------ projectors
LATTICE = np.array([[7.3, 0.5, -0.3], [0.4, 6.6, 0.8], [-0.6, 0.7, 7.9]]).T
KPT = np.array([0.13, -0.2, 0.31])
FFT_SMALL = (6, 5, 4)
PSP_A = dftk.load_psp("Si", "lda")                                                       # l = 0: 2, l = 1: 1
PSP_B = psp_mod._psp(5, 0.5, [-4.0, 0.6], [0.5, 0.5, 0.45, 0.4], [[], [], [[0.3]], [[-0.2]]], "test-df")   # l = 2: 1, l = 3: 1
ATOMS = [(0, np.array([0.07, 0.11, 0.05])), (0, np.array([0.43, 0.52, 0.38])), (1, np.array([0.71, 0.26, 0.83]))]


class ProjCell:
    def __init__(self, lib):
        from test_gpu_kernels import Basis
        self.lib = lib
        self.recip = 2 * math.pi * np.linalg.inv(LATTICE.T)
        self.vol = abs(np.linalg.det(LATTICE))
        self.B = np.asfortranarray(self.recip, dtype=np.float64)
        self.bs = Basis(lib, *FFT_SMALL, self.vol)
        G, _ = upf_gen.cube_G(*FFT_SMALL)
        q = (G + KPT[None, :]) @ self.recip.T
        keep = np.nonzero(0.5 * np.sum(q * q, axis=1) <= 2.6)[0]
        self.G = G[keep]
        self.n = len(keep)
        assert 24 <= self.n <= 100, self.n
        self.qn = np.linalg.norm(q[keep], axis=1)
        self.species = np.array([a[0] for a in ATOMS], dtype=np.int32)
        self.pos = np.ascontiguousarray(np.array([a[1] for a in ATOMS]))
        self.rp = np.zeros((2, 4))
        self.nproj = np.zeros((2, 4), dtype=np.int32)
        self.first = np.zeros((2, 4), dtype=np.int32)
        self.chan = []                                   # (psp, l, i)
        for s, psp in enumerate((PSP_A, PSP_B)):
            for l in range(psp.lmax + 1):
                self.rp[s, l], self.nproj[s, l], self.first[s, l] = psp.rp[l], psp.h[l].shape[0], len(self.chan)
                self.chan += [(psp, l, i) for i in range(1, psp.h[l].shape[0] + 1)]
        self.n_p = 2 * (2 + 3) + (5 + 7)

    def closed(self, c, qn):
        psp, l, i = self.chan[c]
        return psp_mod.eval_psp_projector_fourier(psp, i, l, torch.from_numpy(np.ascontiguousarray(qn))).numpy()

    def hgh(self, rows=slice(None)):
        G32 = torch.from_numpy(np.ascontiguousarray(self.G[rows], dtype=np.int32)).to(DEV)
        n = G32.shape[0]
        n_p = C.c_int()
        P = torch.empty((self.n_p, n), dtype=torch.complex128, device=DEV)
        check(self.lib.dftk_mi_build_projectors_hgh(self.bs.h, n, G32.data_ptr(), self.B.ctypes.data, KPT.ctypes.data,
                                                    self.vol, 2, self.rp.ctypes.data, self.nproj.ctypes.data, 3,
                                                    self.species.ctypes.data, self.pos.ctypes.data, P.data_ptr(), n,
                                                    C.byref(n_p)))
        self.bs.sync()
        assert n_p.value == self.n_p
        return P.cpu().numpy().T

    def radial(self, R, rows=slice(None), ldP=None, query=False):
        G32 = torch.from_numpy(np.ascontiguousarray(self.G[rows], dtype=np.int32)).to(DEV)
        n = G32.shape[0]
        ldP = n if ldP is None else ldP
        Rd = torch.from_numpy(np.ascontiguousarray(R)).to(DEV)
        n_p = C.c_int()
        P = torch.full((self.n_p, ldP), float("nan"), dtype=torch.complex128, device=DEV)
        torch.cuda.synchronize()
        check(self.lib.dftk_mi_build_projectors_radial(self.bs.h, n, G32.data_ptr(), self.B.ctypes.data, KPT.ctypes.data,
                                                       self.vol, 2, Rd.data_ptr(), R.shape[1], self.first.ctypes.data,
                                                       self.nproj.ctypes.data, 3, self.species.ctypes.data,
                                                       self.pos.ctypes.data, None if query else P.data_ptr(), ldP,
                                                       C.byref(n_p)))
        self.bs.sync()
        assert n_p.value == self.n_p
        return P.cpu().numpy().T


@pytest.fixture(scope="module")
def pc(lib):
    return ProjCell(lib)


def _ulp4(got, want):
    """every column within 4 ulp of its largest entry (real and imaginary parts)"""
    for c in range(want.shape[1]):
        big = np.max(np.abs(np.concatenate([want[:, c].real, want[:, c].imag])))
        d = np.max(np.abs(np.concatenate([(got[:, c] - want[:, c]).real, (got[:, c] - want[:, c]).imag])))
        assert d <= 4 * np.spacing(big), (c, d / np.spacing(big))


def test_projectors_radial_closed_form_table(pc):
    R = np.stack([pc.closed(c, pc.qn) for c in range(len(pc.chan))])
    want = pc.hgh()
    got = pc.radial(R)
    assert got.shape == (pc.n, pc.n_p) and not np.any(np.isnan(got))
    _ulp4(got, want)
    # the twin: layout, (-i)^l, solid harmonics, phases
    species = [[[(lambda qn, c=pc.first[s, l] + i: pc.closed(c, qn)) for i in range(pc.nproj[s, l])] for l in range(4)]
               for s in range(2)]
    twin = upf_gen.twin_projectors(pc.G, KPT, pc.recip, pc.vol, species, ATOMS)
    for c in range(pc.n_p):
        assert np.max(np.abs(got[:, c] - twin[:, c])) <= 64 * EPS * np.max(np.abs(twin[:, c])), c
    # a slab of rows, a padded leading dimension, the column count query
    rows = slice(5, pc.n - 3)
    slab = pc.radial(R[:, rows], rows=rows, ldP=pc.n + 9)
    assert np.array_equal(slab[:pc.n - 8], got[rows])
    assert np.all(np.isnan(slab[pc.n - 8:]))             # the padding is not written
    _ulp4(slab[:pc.n - 8], pc.hgh(rows))
    pc.radial(R, query=True)


def test_projectors_radial_from_device_transform(lib, pc):
    """species A from a generated UPF file: channels by dftk_mi_radial_transform at the rows' |q|, P against the twin with
    its own Hankel sums of the same file"""
    u = dftk.parse_psp_upf(upf_gen.write_upf(PSP_A, upf_gen.log_mesh(400), cutoff_index=[400, 380, 391]))
    tw = upf_gen.twin_channels(u)
    q = pc.qn
    R = np.stack([pc.closed(c, q) for c in range(len(pc.chan))])
    twinR = {}
    for c, (psp, l, i) in enumerate(pc.chan):
        if psp is PSP_A:
            r, wf = u.projector_channel(l, i - 1)
            R[c] = _call(lib, pc.bs, 0, l, r, wf, q)
            twinR[c] = upf_gen.twin_hankel(*tw[(l, i - 1)], l, q)
            # E_quad of this coarse mesh is not the point here: same sums, different summation order and Bessel code
            assert np.max(np.abs(R[c] - twinR[c])) <= 1e-12 * np.max(np.abs(twinR[c])), c
    got = pc.radial(R)
    species = [[[(lambda qn, c=pc.first[s, l] + i: twinR.get(c, None) if c in twinR else pc.closed(c, qn))
                 for i in range(pc.nproj[s, l])] for l in range(4)] for s in range(2)]
    twin = upf_gen.twin_projectors(pc.G, KPT, pc.recip, pc.vol, species, ATOMS)
    for c in range(pc.n_p):
        assert np.max(np.abs(got[:, c] - twin[:, c])) <= 1e-12 * np.max(np.abs(twin[:, c])), c


# ------------------------------------------------------------------------------------------------ cube entries
def _local_ff(psp, qn):
    return psp_mod.eval_psp_local_fourier(psp, torch.from_numpy(np.ascontiguousarray(qn))).numpy()


class CubeCell:
    def __init__(self, lib, shape):
        from test_gpu_kernels import Basis, KBlock
        self.lib, self.shape = lib, shape
        nx, ny, nz = shape
        self.N = nx * ny * nz
        self.recip = 2 * math.pi * np.linalg.inv(LATTICE.T)
        self.vol = abs(np.linalg.det(LATTICE))
        self.B = np.asfortranarray(self.recip, dtype=np.float64)
        self.bs = Basis(lib, nx, ny, nz, self.vol)
        self.cube = KBlock(lib, self.bs, np.arange(self.N), np.zeros(self.N))
        G, _ = upf_gen.cube_G(nx, ny, nz)
        self.qn = np.linalg.norm(G @ self.recip.T, axis=1)
        self.species = np.array([a[0] for a in ATOMS], dtype=np.int32)
        self.pos = np.ascontiguousarray(np.array([a[1] for a in ATOMS]))
        self.par = np.zeros((2, 8))
        for s, psp in enumerate((PSP_A, PSP_B)):
            self.par[s, :6] = [psp.rloc, psp.Zion] + list(psp.cloc)[:4]
        self.ff = np.stack([_local_ff(PSP_A, self.qn), _local_ff(PSP_B, self.qn)])
        self.ffd = torch.from_numpy(self.ff).to(DEV)
        rng = np.random.default_rng(7)
        # a smooth positive density: decaying random Fourier coefficients
        c = (rng.standard_normal((nz, ny, nx)) + 1j * rng.standard_normal((nz, ny, nx))) * np.exp(
            -0.35 * self.qn.reshape(nz, ny, nx) ** 2)
        self.rho = 1.5 + np.fft.ifftn(c).real * self.N * 0.02
        self.rhod = torch.from_numpy(np.ascontiguousarray(self.rho)).to(DEV)

    def superposition(self, table, coef=None):
        out = torch.full((self.N,), float("nan"), dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        if table:
            coef = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
            check(self.lib.dftk_mi_atomic_superposition_table(self.cube.h, self.B.ctypes.data, 2, self.ffd.data_ptr(), 3,
                                                              self.species.ctypes.data, self.pos.ctypes.data,
                                                              None if coef is None else coef.ctypes.data,
                                                              out.data_ptr()))
        else:
            check(self.lib.dftk_mi_atomic_superposition(self.cube.h, 0, self.B.ctypes.data, 2, self.par.ctypes.data, 3,
                                                        self.species.ctypes.data, self.pos.ctypes.data, out.data_ptr()))
        self.bs.sync()
        return out.cpu().numpy()

    def forces(self, table):
        out = np.full((3, 3), np.nan)
        torch.cuda.synchronize()
        if table:
            check(self.lib.dftk_mi_forces_local_table(self.cube.h, self.B.ctypes.data, 2, self.ffd.data_ptr(), 3,
                                                      self.species.ctypes.data, self.pos.ctypes.data,
                                                      self.rhod.data_ptr(), out.ctypes.data))
        else:
            check(self.lib.dftk_mi_forces_local(self.cube.h, self.B.ctypes.data, 2, self.par.ctypes.data, 3,
                                                self.species.ctypes.data, self.pos.ctypes.data, self.rhod.data_ptr(),
                                                out.ctypes.data))
        return out


@pytest.fixture(scope="module", params=[(6, 5, 4), (15, 16, 25)], ids=["6x5x4", "15x16x25"])
def cc(lib, request):
    return CubeCell(lib, request.param)


def test_superposition_table(cc):
    want = cc.superposition(False)
    got = cc.superposition(True)
    assert not np.any(np.isnan(got))
    assert np.max(np.abs(got - want)) <= 4 * np.spacing(np.max(np.abs(want)))
    nx, ny, nz = cc.shape
    twin = upf_gen.twin_superposition(cc.shape, cc.recip, cc.vol,
                                      [lambda q: _local_ff(PSP_A, q), lambda q: _local_ff(PSP_B, q)], ATOMS)
    assert np.max(np.abs(got.reshape(nz, ny, nx) - twin)) <= 1e-12 * np.max(np.abs(twin))
    # one amplitude per atom (the coefficients of the spin-density guess): all ones change nothing, others scale the
    # atom's term -- the twin with every atom a species of its own
    assert np.array_equal(cc.superposition(True, coef=[1.0, 1.0, 1.0]), got)
    coef = [0.5, -1.25, 2.0]
    ffs = [lambda q, c=c, psp=psp: c * _local_ff(psp, q) for c, psp in zip(coef, (PSP_A, PSP_A, PSP_B))]
    twin = upf_gen.twin_superposition(cc.shape, cc.recip, cc.vol, ffs, [(i, pos) for i, (_, pos) in enumerate(ATOMS)])
    got = cc.superposition(True, coef=coef)
    assert not np.any(np.isnan(got))
    assert np.max(np.abs(got.reshape(nz, ny, nx) - twin)) <= 1e-12 * np.max(np.abs(twin))


def test_forces_local_table(cc):
    want = cc.forces(False)
    got = cc.forces(True)
    assert not np.any(np.isnan(got))
    assert np.max(np.abs(got - want)) <= 4 * np.spacing(np.max(np.abs(want)))
    # no atoms: nothing to do, whatever the other arguments hold
    assert cc.lib.dftk_mi_forces_local_table(cc.cube.h, cc.B.ctypes.data, 2, None, 0, None, None, cc.rhod.data_ptr(),
                                             None) == 0
    # central differences of the twin's local energy.  E(u) = Re sum_G A_G e^{-2 pi i G.(r_a + u e_alpha)} with
    # A_G = ff_s(G) conj(R_G) / N (unpaired Nyquist entries dropped), so |E'''| <= M3 = sum_G |2 pi G_alpha|^3 |A_G|: the step
    # balances the truncation h^2 M3 / 6 against the round-off eps |E| / h, and the bound is twice their sum
    nx, ny, nz = cc.shape
    G, ok = upf_gen.cube_G(nx, ny, nz)
    Rg = np.fft.fftn(cc.rho).reshape(-1)
    ffs = [lambda q: _local_ff(PSP_A, q), lambda q: _local_ff(PSP_B, q)]

    def energy(atoms):
        return upf_gen.twin_local_energy(cc.shape, cc.recip, cc.vol, ffs, atoms, cc.rho)

    # the size of the terms the energy is summed from (its round-off, transforms included: a few eps of this)
    E0 = 8 * float(np.sum(np.abs(upf_gen.twin_superposition(cc.shape, cc.recip, cc.vol, ffs, ATOMS) * cc.rho))
                   * cc.vol / cc.N)
    for a, (s, pos) in enumerate(ATOMS):
        A = np.abs(np.where(ok, cc.ff[s] * np.conj(Rg) / cc.N, 0.0))
        for al in range(3):
            M3 = float(np.sum(np.abs(2 * math.pi * G[:, al]) ** 3 * A))
            h = (3 * EPS * E0 / M3) ** (1 / 3)
            moved = lambda d: [(sp, p + d * np.eye(3)[al]) if i == a else (sp, p)  # noqa: E731
                               for i, (sp, p) in enumerate(ATOMS)]
            fd = -(energy(moved(h)) - energy(moved(-h))) / (2 * h)
            bound = 2 * (h * h * M3 / 6 + EPS * E0 / h)
            print(f"atom {a} alpha {al}: F {got[a, al]:.12e}, FD {fd:.12e}, h {h:.1e}, bound {bound:.1e}")
            assert abs(got[a, al] - fd) <= bound, (a, al, got[a, al], fd, bound)
