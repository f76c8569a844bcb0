"""The three response entry points of include/dftk_mi355x.h at the C ABI (ctypes, device memory from torch), on the shapes
where their device code takes another path than on the 18^3 cell of test_gpu_response.py:

A. ``dftk_mi_density_response_accumulate`` against NumPy FFTs: non-cubic grids (nx, ny, nz and the padded nxp all different),
   nz > 32 (more than one accumulator per thread), every z radix plan including the generic prime factor, several launch
   groups (b0 > 0), fft_batch = 1, skipped all-zero groups, leading dimensions above n_G with NaN padding.
B. ``dftk_mi_sternheimer`` against the dense solve x* = -sum_{m >= n_occ} V_m <V_m|rhs> / (E_m - eps) of eigh(H.to_dense()):
   n_G = 1153 (two row blocks and all four unroll lanes of the CG kernels, three H - eps batches with their own shifts),
   five different leading dimensions, a k-block without potential (the shift as a pass of its own), locking with an active
   range strictly inside the block, miniter beyond convergence, start vectors, a right-hand side inside the occupied span.
C. ``dftk_mi_apply_kernel``: f_xc point by point against 60-digit mpmath second derivatives of rho eps(rho) from 1e-12 to
   1e4, and the Hartree part on non-cubic grids against numpy.fft.

All bounds are derived, none is measured on the device: 1e-12 is this suite's bound for FFT identities (RTOL of
test_gpu_kernels.py); the Sternheimer error bound is |A^-1 rho| <= |rho| / gap on the complement of the occupied space.
Every assertion of B uses quantities recomputed on the host from the dense H, never a number the solver reports as its own
bound.  The iteration counts are compared with a NumPy restatement of the same preconditioned CG (``host_cg``): in exact
arithmetic the two agree, in floating point a residual close to the tolerance moves the count by a few iterations.

Out of reach: the grid-stride loop behind RESP_MAX_ROW_BLOCKS = 2048 row blocks of 1024 rows needs n_G above two million,
far beyond any dense reference; it is not tested here.
"""
import ctypes as C

import mpmath
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402

from oracle import energy_hamiltonian  # noqa: E402

from test_gpu_kernels import Basis, KBlock, dev, make_oracle_basis  # noqa: E402

RTOL = 1e-12                 # FFT identities, as in test_gpu_kernels.py
EINVAL = -1                  # DFTK_MI_EINVAL
MARGIN = 1e-3                # relative slack between a recomputed and a reported residual norm (test_gpu_response.py)
MAXITER = 100
SENTINEL = 7.0 + 3.0j
KGEN = 1                     # index of the generic k-point [1/3, 0.1, -0.25] in make_oracle_basis; 0 is Gamma


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


def padded(A, ld, fill=complex(np.nan, np.nan)):
    """the columns of the host matrix A (n x m) as a band-major device block of leading dimension ld, padding rows = fill"""
    n, m = A.shape
    buf = np.full((m, ld), fill, dtype=complex)
    buf[:, :n] = A.T
    return dev(buf)


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# =========================================================================================== A: density response
def cube_of(obasis, kpt, c):
    """unnormalised BFFT of the sphere coefficients c on the (nz, ny, nx) grid"""
    nx, ny, nz = obasis.fft_size
    cube = np.zeros(nx * ny * nz, dtype=complex)
    cube[kpt.mapping] = c
    return np.fft.ifftn(cube.reshape(nz, ny, nx)) * (nx * ny * nz)


def drho_reference(obasis, kpt, psi, dpsi, wo, wd, drho0):
    ref = drho0.copy()
    for b in range(psi.shape[1]):
        p, d = cube_of(obasis, kpt, psi[:, b]), cube_of(obasis, kpt, dpsi[:, b])
        ref += 2.0 * wo[b] * np.real(np.conj(p) * d) + wd[b] * np.abs(p) ** 2
    return ref


def accumulate(lib, bs, kb, psi, dpsi, wo, wd, drho0, pad_psi=5, pad_dpsi=9):
    n, nb = psi.shape
    pd, dd = padded(psi, n + pad_psi), padded(dpsi, n + pad_dpsi)
    out = dev(drho0)
    wo, wd = np.ascontiguousarray(wo, dtype=np.float64), np.ascontiguousarray(wd, dtype=np.float64)
    torch.cuda.synchronize()
    check(lib.dftk_mi_density_response_accumulate(kb.h, nb, pd.data_ptr(), n + pad_psi, dd.data_ptr(), n + pad_dpsi,
                                                  wo.ctypes.data, wd.ctypes.data, out.data_ptr()))
    bs.sync()
    return out.cpu().numpy()


def response_case(lib, Ecut, fft_size, nb, wo, wd, fft_batch=None, repeat=False):
    """both k-points of one grid: device against NumPy; returns the worst max|got - ref| / max|ref - drho0|"""
    obasis = make_oracle_basis(Ecut, fft_size, terms=("Kinetic",))
    nx, ny, nz = fft_size
    bs = Basis(lib, nx, ny, nz, obasis.model.unit_cell_volume)
    if fft_batch is not None:
        check(lib.dftk_mi_basis_set_fft_batch(bs.h, fft_batch))
    rng = np.random.default_rng(1000 * nx + 10 * nz + nb)
    worst = 0.0
    for kpt in obasis.kpoints:
        n = len(kpt.mapping)
        kb = KBlock(lib, bs, kpt.mapping, np.zeros(n))
        psi, dpsi = crandn(rng, n, nb), crandn(rng, n, nb)
        drho0 = rng.standard_normal((nz, ny, nx))              # the call accumulates
        got = accumulate(lib, bs, kb, psi, dpsi, wo, wd, drho0)
        ref = drho_reference(obasis, kpt, psi, dpsi, wo, wd, drho0)
        assert np.isfinite(got).all()                          # the NaN padding rows did not leak
        scale = np.abs(ref - drho0).max()
        assert scale > 1.0
        err = np.abs(got - ref).max() / scale
        worst = max(worst, err)
        assert err <= RTOL, (fft_size, n, nb, err)
        if repeat:
            assert np.array_equal(accumulate(lib, bs, kb, psi, dpsi, wo, wd, drho0), got)
    return worst


# z sizes: 20 = 5.4, 33 = 3.11 (generic prime, nz > 32), 40 = 8.5 (nz > 32), 21 = 3.7 (generic prime), 27 = 3.3.3,
# 24 = 3.8, 25 = 5.5, 36 = 6.6, 16 = 8.2
RESPONSE_GRIDS = [(6, (33, 16, 20)), (6, (16, 20, 33)), (20, (32, 36, 40)), (10, (21, 21, 21)), (12, (24, 25, 27)),
                  (8, (20, 25, 24)), (7, (18, 20, 25)), (9, (24, 20, 36)), (5, (16, 15, 16))]


@pytest.mark.parametrize("Ecut,fft_size", RESPONSE_GRIDS)
def test_density_response_on_every_grid(lib, Ecut, fft_size):
    """Code paths of k_zdensity_response: (33,16,20) has nx = 33 = 4 x-tiles of FFT_L = 8 plus one column (nxp = 40: the
    ``x < nx`` guard and the ``y * nxp + x`` read of T2 differ from ``y * nx + x``) and three different sizes, so swapped
    strides in ``drho[(z * ny + y) * nx + x]`` change the result; (16,20,33) has nz = 33: accumulator k = 1 live for z = 32
    only; (32,36,40) fills k = 1 for z = 32 .. 39; (21,21,21) and (16,20,33) instantiate the GEN = true z plan; the other
    grids end their z plans with 3, 8, 5, 6 and 2 as the list of test_apply_H_vs_oracle does.  Both k-points (Gamma and a
    generic one) on each grid; ld_psi != ld_dpsi > n_G with NaN padding; drho prefilled.
    Measured on the MI355X: worst max|got - ref| / max|ref - drho0| over the grids 8.5e-16 (bound 1e-12)."""
    wo = np.array([1.0, 0.6, -0.3])
    wd = np.array([0.25, -0.7, 0.4])
    worst = response_case(lib, Ecut, fft_size, 3, wo, wd)
    print(f"\ndensity response {fft_size}: worst rel max err {worst:.3e}")


# (nb, fft_batch, wo, wd): the response group is fft_batch / 2 bands (two scratch slots per band)
GROUP_CASES = {
    # groups (0,1) (2,3) (4,5) (6): band 1 has wo = 0 and a negative wd, group (2,3) is all zero and skipped, band 4 has
    # wd = 0, band 5 is a dead band inside a live group, the last group starts at b0 = 6 with one band
    "7 bands, batch 4": (7, 4, [1.0, 0.0, 0.0, 0.0, 0.7, 0.0, 2.0], [0.5, -0.8, 0.0, 0.0, 0.0, 0.0, -0.4]),
    # fft_batch = 1: one band per group; band 2 is a skipped group, band 1 takes the single-transform path (wo = 0)
    "5 bands, batch 1": (5, 1, [1.0, 0.0, 0.0, 0.5, 0.3], [0.0, -0.6, 0.0, 0.2, 0.0]),
    # default batch 32: groups of 16 + 1, the second group reads psi, dpsi, wo and wd at b0 = 16
    "17 bands, default batch": (17, None,
                                [1.0, 0.9, 0.0, 0.0, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 1.1, 1.2, 1.3, 1.4, 1.7],
                                [0.0, 0.3, -0.5, 0.0, 0.1, 0.0, 0.2, -0.2, 0.3, 0.0, 0.4, 0.0, -0.1, 0.0, 0.5, 0.6, -0.9]),
}


@pytest.mark.parametrize("case", list(GROUP_CASES))
@pytest.mark.parametrize("Ecut,fft_size", [(6, (33, 16, 20)), (20, (32, 36, 40))])
def test_density_response_band_groups_and_weights(lib, Ecut, fft_size, case):
    """Code paths of launch_density_response: a second and later launch group (``psi + b0 * ldpsi``, ``dpsi + b0 * lddpsi``,
    ``wo_d + b0``, ``wd_d + b0`` with b0 > 0, the slot offset nbb of the second stage A / B pair differing between groups), the
    skipped all-zero group, fft_batch = 1, and in the kernel the ``w2 == 0 && w1 == 0`` and ``w2 == 0`` branches.  One of
    the grids has nz = 40 > 32.  Two identical calls give bitwise identical results (one writer per drho entry)."""
    nb, batch, wo, wd = GROUP_CASES[case]
    worst = response_case(lib, Ecut, fft_size, nb, np.array(wo), np.array(wd), fft_batch=batch, repeat=True)
    print(f"\ndensity response {fft_size}, {case}: worst rel max err {worst:.3e}")


def test_density_response_edges(lib):
    """n_bands = 0 leaves drho bit-identical; a leading dimension below n_G is refused."""
    fft_size = (16, 15, 16)
    obasis = make_oracle_basis(5, fft_size, terms=("Kinetic",))
    nx, ny, nz = fft_size
    bs = Basis(lib, nx, ny, nz, obasis.model.unit_cell_volume)
    kpt = obasis.kpoints[KGEN]
    n = len(kpt.mapping)
    kb = KBlock(lib, bs, kpt.mapping, np.zeros(n))
    rng = np.random.default_rng(5)
    psi, dpsi = crandn(rng, n, 2), crandn(rng, n, 2)
    drho0 = rng.standard_normal((nz, ny, nx))
    w = np.ones(2)
    pd, dd, out = padded(psi, n), padded(dpsi, n), dev(drho0)
    torch.cuda.synchronize()
    check(lib.dftk_mi_density_response_accumulate(kb.h, 0, pd.data_ptr(), n, dd.data_ptr(), n, w.ctypes.data,
                                                  w.ctypes.data, out.data_ptr()))
    bs.sync()
    assert np.array_equal(out.cpu().numpy(), drho0)
    for ld_psi, ld_dpsi in ((n - 1, n), (n, n - 1)):
        assert lib.dftk_mi_density_response_accumulate(kb.h, 2, pd.data_ptr(), ld_psi, dd.data_ptr(), ld_dpsi,
                                                       w.ctypes.data, w.ctypes.data, out.data_ptr()) == EINVAL
    bs.sync()
    assert np.array_equal(out.cpu().numpy(), drho0)


# =========================================================================================== B: Sternheimer
class System:
    """One k-block on the device with its dense H, spectrum (E, V) and kinetic energies on the host."""

    def __init__(self, lib, Ecut, fft_size, ik, fft_batch=None, kinetic_only=False):
        terms = ("Kinetic",) if kinetic_only else ("Kinetic", "AtomicLocal", "AtomicNonlocal")
        obasis = make_oracle_basis(Ecut, fft_size, terms=terms)
        _, ham = energy_hamiltonian(obasis, None, None)
        H, kpt = ham[ik], obasis.kpoints[ik]
        nx, ny, nz = fft_size
        self.lib = lib
        self.bs = Basis(lib, nx, ny, nz, obasis.model.unit_cell_volume)
        if fft_batch is not None:
            check(lib.dftk_mi_basis_set_fft_batch(self.bs.h, fft_batch))
        self.kb = KBlock(lib, self.bs, kpt.mapping, H.kinetic)
        self.n = H.n_G
        self.kin = np.asarray(H.kinetic, dtype=np.float64)
        if kinetic_only:       # no potential bound, no projectors: H = diag(kin), its eigenvectors are unit vectors
            order = np.argsort(self.kin, kind="stable")
            self.Hd = np.diag(self.kin).astype(complex)
            self.E, self.V = self.kin[order], np.eye(self.n, dtype=complex)[:, order]
        else:
            self.kb.set_projectors(H.P, H.D)
            self.kb.set_potential(H.potential)
            Hd = H.to_dense()
            assert np.abs(Hd - Hd.conj().T).max() < 1e-12
            self.Hd = (Hd + Hd.conj().T) / 2
            self.E, self.V = np.linalg.eigh(self.Hd)

    def exact(self, n_occ, rhs):
        """x*_c = -sum_{m >= n_occ} V_m <V_m|rhs_c> / (E_m - eps_c)"""
        Vc, Ec = self.V[:, n_occ:], self.E[n_occ:]
        return -Vc @ ((Vc.conj().T @ rhs) / (Ec[:, None] - self.E[None, :n_occ]))

    def residual(self, n_occ, x, rhs):
        """rho_c = Q ((H - eps_c) x_c + rhs_c), Q = 1 - psi_occ psi_occ'"""
        P = self.V[:, :n_occ]
        Y = self.Hd @ x - x * self.E[None, :n_occ] + rhs
        return Y - P @ (P.conj().T @ Y)

    def extra_bands(self, n_occ, n_extra, seed):
        """n_extra Rayleigh-Ritz vectors orthogonal to the occupied space that are NOT eigenvectors"""
        rng = np.random.default_rng(seed)
        V, E, n = self.V, self.E, self.n
        rest = n - n_occ - n_extra
        X = V[:, n_occ:n_occ + n_extra] + 0.1 / np.sqrt(rest) * (V[:, n_occ + n_extra:] @ crandn(rng, rest, n_extra))
        X -= V[:, :n_occ] @ (V[:, :n_occ].conj().T @ X)
        Q, _ = np.linalg.qr(X)
        Hm = Q.conj().T @ ((V * E) @ (V.conj().T @ Q))
        e, U = np.linalg.eigh((Hm + Hm.conj().T) / 2)
        assert np.abs(e - E[n_occ:n_occ + n_extra]).max() > 1e-7
        return Q @ U

    def unit_rhs(self, n_occ, seed):
        rhs = crandn(np.random.default_rng(seed), self.n, n_occ)
        return rhs / np.linalg.norm(rhs, axis=0)


def host_cg(s, n_occ, rhs, tol, extra=None, miniter=1, maxiter=MAXITER, x0=None):
    """The solver's algorithm restated with dense NumPy algebra (Schur split over the extra bands, R-projected block CG with
    the TPA preconditioner of the first occupied column's mean kinetic energy, locking on a contiguous active range).
    Returns (x, n_iter, converged): the yardstick for the iteration counts."""
    P, eps = s.V[:, :n_occ], s.E[:n_occ]
    Phi = P if extra is None else np.concatenate([P, extra], axis=1)

    def R(Y):
        return Y - Phi @ (Phi.conj().T @ Y)

    if extra is not None:
        HPe = s.Hd @ extra
        ee = np.real(np.sum(extra.conj() * HPe, axis=0))

    def A(Y, cols):
        Y = R(Y)
        Z = s.Hd @ Y - Y * eps[None, cols]
        if extra is not None:
            Z -= HPe @ ((HPe.conj().T @ Y) / (ee[:, None] - eps[None, cols]))
        return R(Z)

    mk = float(np.real(np.vdot(P[:, 0], s.kin * P[:, 0])))

    def prec(Y):
        return R((mk / (mk + s.kin))[:, None] * R(Y))

    b = -(rhs - P @ (P.conj().T @ rhs))
    r = b.copy()
    if extra is not None:
        r = b - HPe @ ((extra.conj().T @ b) / (ee[:, None] - eps[None, :]))
    r = R(r)
    x = np.zeros_like(r)
    if x0 is not None:
        x = R(x0)
        r = r - A(x, slice(0, n_occ))
    c = prec(r)
    gam = np.real(np.sum(r.conj() * c, axis=0))
    p = c.copy()
    res = np.linalg.norm(r, axis=0)
    n_iter, converged = 0, False

    def ratio(a, d):
        return np.where(d != 0, a / np.where(d != 0, d, 1.0), 0.0)

    while n_iter < maxiter:
        n_iter += 1
        active = np.nonzero(~(res <= tol))[0]
        if n_iter >= miniter and len(active) == 0:
            converged = True
            break
        cols = slice(0, n_occ) if len(active) == 0 else slice(active[0], active[-1] + 1)
        Ap = A(p[:, cols], cols)
        alpha = ratio(gam[cols], np.real(np.sum(p[:, cols].conj() * Ap, axis=0)))
        x[:, cols] = R(x[:, cols] + p[:, cols] * alpha)
        r[:, cols] = R(r[:, cols] - Ap * alpha)
        res[cols] = np.linalg.norm(r[:, cols], axis=0)
        c = prec(r[:, cols])
        gnew = np.real(np.sum(r[:, cols].conj() * c, axis=0))
        p[:, cols] = R(c + p[:, cols] * ratio(gnew, gam[cols]))
        gam[cols] = gnew
    if extra is not None:
        x = x + extra @ ((extra.conj().T @ (b - (s.Hd @ x - x * eps[None, :]))) / (ee[:, None] - eps[None, :]))
    return x, n_iter, converged


def solve(s, n_occ, rhs, tol, extra=None, dpsi0=None, miniter=1, maxiter=MAXITER, pads=(0, 0, 0, 0, 0)):
    """one dftk_mi_sternheimer call; pads = what ld_occ, ld_extra, ld_rhs, ld_dpsi0, ld_dpsi exceed n_G by.  The input
    padding is NaN, the output block is prefilled with SENTINEL."""
    lib, n = s.lib, s.n
    ld_occ, ld_extra, ld_rhs, ld_dpsi0, ld_dpsi = (n + p for p in pads)
    occ_d = padded(s.V[:, :n_occ], ld_occ)
    rhs_d = padded(rhs, ld_rhs)
    ext_d = padded(extra, ld_extra) if extra is not None else None
    x0_d = padded(dpsi0, ld_dpsi0) if dpsi0 is not None else None
    out = torch.full((n_occ, ld_dpsi), SENTINEL, dtype=torch.complex128, device="cuda")
    eps = np.ascontiguousarray(s.E[:n_occ], dtype=np.float64)
    tol_h = np.ascontiguousarray(np.broadcast_to(np.asarray(tol, dtype=np.float64), (n_occ,)))
    res = np.full(n_occ, np.nan)
    n_iter, conv = C.c_int(-1), C.c_int(-1)
    torch.cuda.synchronize()
    st = lib.dftk_mi_sternheimer(s.kb.h, n_occ, occ_d.data_ptr(), ld_occ, eps.ctypes.data,
                                 0 if extra is None else extra.shape[1], ext_d.data_ptr() if extra is not None else None,
                                 ld_extra if extra is not None else 0, rhs_d.data_ptr(), ld_rhs, tol_h.ctypes.data, miniter,
                                 maxiter, x0_d.data_ptr() if dpsi0 is not None else None,
                                 ld_dpsi0 if dpsi0 is not None else 0, out.data_ptr(), ld_dpsi, C.byref(n_iter),
                                 res.ctypes.data, C.byref(conv))
    s.bs.sync()
    raw = out.cpu().numpy()
    return dict(status=st, x=raw[:, :n].T.copy(), padding=raw[:, n:], n_iter=n_iter.value, converged=conv.value,
                residual_norms=res, tol=tol_h)


def check_solution(s, n_occ, rhs, out, label, xstar=None):
    """Assertions 1-4 of the module docstring on host-recomputed quantities; returns the worst error / bound of 4."""
    assert out["status"] == 0, s.lib.dftk_mi_last_error()
    assert out["converged"] == 1, (label, out["n_iter"], out["residual_norms"])
    x, tol = out["x"], out["tol"]
    P = s.V[:, :n_occ]
    xstar = s.exact(n_occ, rhs) if xstar is None else xstar
    # the reference solves the equation: its own residual is rounding
    assert np.linalg.norm(s.residual(n_occ, xstar, rhs), axis=0).max() < 1e-12
    assert np.isfinite(x).all()
    ortho = np.abs(P.conj().T @ x).max()
    assert ortho < 1e-12, (label, ortho)                                                   # 1
    true = np.linalg.norm(s.residual(n_occ, x, rhs), axis=0)
    assert np.all(true <= tol * (1 + MARGIN) + 1e-13), (label, true, tol)                  # 2
    rep = out["residual_norms"]
    assert np.all(np.abs(true - rep) <= MARGIN * rep + 1e-13), (label, true, rep)          # 3
    gap = s.E[n_occ] - s.E[:n_occ]
    err = np.linalg.norm(x - xstar, axis=0)
    bound = tol * (1 + MARGIN) / gap + 1e-12 * np.linalg.norm(xstar, axis=0)
    ratio = float((err / bound).max())
    print(f"\n{label}: n_G {s.n}, n_iter {out['n_iter']}, |psi_occ' x| {ortho:.2e}, residuals {true}, "
          f"worst error / bound {ratio:.3e}")
    assert np.all(err <= bound), (label, err, bound)                                       # 4
    return ratio


def check_iterations(n_iter, n_ref, label):
    """Same algorithm, same inputs: equal counts in exact arithmetic.  Rounding moves a residual across its tolerance one
    iteration earlier or later, and over some hundred iterations the two histories drift apart by a few more."""
    print(f"{label}: device iterations {n_iter}, NumPy restatement {n_ref}")
    assert abs(n_iter - n_ref) <= max(2, n_ref // 10), (label, n_iter, n_ref)


@pytest.fixture(scope="module")
def big(lib):
    """Ecut 20, fft (36,40,32), generic k: n_G = 1153; fft_batch 3, so 7 columns of H - eps go in batches 3, 3, 1"""
    s = System(lib, 20, (36, 40, 32), KGEN, fft_batch=3)
    assert s.n > 1024
    return s


@pytest.fixture(scope="module")
def mid(lib):
    """Ecut 12, fft (24,25,27): n_G = 536 at the generic k; [Gamma, generic k]"""
    return [System(lib, 12, (24, 25, 27), ik) for ik in (0, KGEN)]


@pytest.mark.parametrize("n_extra", [0, 5])
def test_sternheimer_two_row_blocks_and_shift_batches(big, n_extra):
    """Code paths: n_G = 1153 > 1024 = RESP_NT * RESP_UNR puts a second row block and lanes u = 1, 2, 3 (with the ``i < n``
    tail in the second block) of k_update_xr, k_update_p and k_axpby to work; 7 columns with fft_batch = 3 reach
    ``shift_d + b0`` at b0 = 3 and 6 in launch_local_apply with a different eps per column.  With 5 extra bands that are not
    eigenvectors the Schur split and the back-substitution run at this size too; the exact answer is the same x*.
    E8 - E7 = 0.035 Ha; tol 1e-10 on unit right-hand sides is met well within maxiter = 100.
    Measured on the MI355X: error / bound of assertion 4: 0.18 without, 0.09 with extra bands; the worst of the
    file is 0.26 (test_sternheimer_rhs_inside_the_occupied_span).  Device and NumPy iteration counts: 34 / 34 and 26 / 26."""
    s, n_occ = big, 7
    assert s.E[n_occ] - s.E[n_occ - 1] > 0.03
    rhs = s.unit_rhs(n_occ, 21)
    extra = s.extra_bands(n_occ, n_extra, 22) if n_extra else None
    out = solve(s, n_occ, rhs, 1e-10, extra=extra)
    check_solution(s, n_occ, rhs, out, f"n_G 1153, {n_extra} extra bands")
    _, n_ref, conv = host_cg(s, n_occ, rhs, np.full(n_occ, 1e-10), extra=extra)
    assert conv
    check_iterations(out["n_iter"], n_ref, f"n_G 1153, {n_extra} extra bands")


@pytest.mark.parametrize("ik,n_occ", [(0, 4), (1, 7)])
def test_sternheimer_five_leading_dimensions(mid, ik, n_occ):
    """Code paths: ld_occ, ld_extra, ld_rhs, ld_dpsi0 and ld_dpsi pairwise different and above n_G (every ew_copy / zgemm
    that touches a caller's block takes its own leading dimension); NaN in the padding of every input; the padding of the
    output keeps its prefill.  n_occ = 4 at Gamma (bands 2-4 degenerate), 7 at the generic k; 3 extra bands; a random
    start vector that is not orthogonal to the occupied space."""
    s = mid[ik]
    rhs = s.unit_rhs(n_occ, 31 + ik)
    extra = s.extra_bands(n_occ, 3, 32 + ik)
    x0 = 0.1 * crandn(np.random.default_rng(33 + ik), s.n, n_occ)
    out = solve(s, n_occ, rhs, 1e-10, extra=extra, dpsi0=x0, pads=(3, 5, 8, 11, 13))
    check_solution(s, n_occ, rhs, out, f"five leading dimensions, k-point {ik}")
    assert out["padding"].shape == (n_occ, 13) and np.all(out["padding"] == SENTINEL)
    _, n_ref, conv = host_cg(s, n_occ, rhs, np.full(n_occ, 1e-10), extra=extra, x0=x0)
    assert conv
    check_iterations(out["n_iter"], n_ref, f"five leading dimensions, k-point {ik}")


def test_sternheimer_kinetic_only_block(lib):
    """Code path: no potential bound and no projectors, so Solver::apply_H_minus_eps takes its ``else`` branch: the kinetic
    pass, then the shift as a resp_axpby pass with the per-column factors read from the device.  H = diag(kin) on the
    sphere of Ecut 6, fft (33,16,20) at the generic k; the occupied columns are the unit vectors of the lowest kinetic
    energies."""
    s = System(lib, 6, (33, 16, 20), KGEN, fft_batch=2, kinetic_only=True)
    n_occ = 5
    while s.E[n_occ] - s.E[n_occ - 1] < 1e-2:
        n_occ += 1
    assert n_occ <= 8 and s.E[n_occ] - s.E[n_occ - 1] >= 1e-2          # the next kinetic value is not degenerate
    rhs = s.unit_rhs(n_occ, 41)
    out = solve(s, n_occ, rhs, 1e-10)
    check_solution(s, n_occ, rhs, out, f"kinetic only, n_occ {n_occ}")
    _, n_ref, conv = host_cg(s, n_occ, rhs, np.full(n_occ, 1e-10))
    assert conv
    check_iterations(out["n_iter"], n_ref, "kinetic only")


def test_sternheimer_locking_inside_the_block(mid):
    """Code path: tolerances [1e-4, 1e-4, 1e-11, 1e-4, 1e-11, 1e-4, 1e-4]: columns 0, 1, 5, 6 converge first and are locked,
    the active range becomes [2, 4] (lo > 0, hi < n_occ - 1: the ``+ lo`` offsets of every block and scalar array) and holds
    the converged column 3, which is iterated on.  Every column meets assertions 2 and 4 for its own tolerance."""
    s, n_occ = mid[1], 7
    tol = np.array([1e-4, 1e-4, 1e-11, 1e-4, 1e-11, 1e-4, 1e-4])
    rhs = s.unit_rhs(n_occ, 51)
    out = solve(s, n_occ, rhs, tol)
    check_solution(s, n_occ, rhs, out, "locking")
    rep = out["residual_norms"]
    # locked columns stop where they met 1e-4; column 3 went on with its neighbours far below its own tolerance
    assert rep[[0, 1, 5, 6]].max() > 1e-9 and rep[3] < 1e-2 * rep[[0, 1, 5, 6]].max()
    _, n_ref, conv = host_cg(s, n_occ, rhs, tol)
    assert conv
    check_iterations(out["n_iter"], n_ref, "locking")


def test_sternheimer_miniter_beyond_convergence(mid):
    """Code path: tol = 1e-2 with miniter = 6.  The start vector x* + 1e-4 d (unit columns d) leaves a residual of at most
    1e-4 |H - eps| < 1e-2, so every column passes the first check and iterations 1 .. 5 run on the whole block through the
    ``lo < 0`` branch (lo = 0, hi = n_occ - 1) before the sixth ends the loop.  n_iter == 6, converged, all four assertions
    hold."""
    s, n_occ = mid[1], 7
    rhs = s.unit_rhs(n_occ, 61)
    x0 = s.exact(n_occ, rhs) + 1e-4 * s.unit_rhs(n_occ, 62)
    assert np.linalg.norm(s.residual(n_occ, x0, rhs), axis=0).max() < 0.5e-2
    _, n_ref, conv = host_cg(s, n_occ, rhs, np.full(n_occ, 1e-2), x0=x0)
    assert conv and n_ref == 1                                           # without miniter the first check ends it
    out = solve(s, n_occ, rhs, 1e-2, dpsi0=x0, miniter=6)
    assert out["n_iter"] == 6
    check_solution(s, n_occ, rhs, out, "miniter 6")


def test_sternheimer_start_vectors(mid):
    """dpsi0 = x* passes the first convergence check (n_iter == 1), and so does x* + psi_occ c: the start vector is projected
    (x = R dpsi0) before the residual r -= A x is formed."""
    s, n_occ = mid[1], 7
    rhs = s.unit_rhs(n_occ, 71)
    xstar = s.exact(n_occ, rhs)
    out = solve(s, n_occ, rhs, 1e-10, dpsi0=xstar)
    assert out["n_iter"] == 1
    check_solution(s, n_occ, rhs, out, "start vector x*")
    c = crandn(np.random.default_rng(72), n_occ, n_occ)
    out = solve(s, n_occ, rhs, 1e-10, dpsi0=xstar + s.V[:, :n_occ] @ c)
    assert out["n_iter"] == 1
    check_solution(s, n_occ, rhs, out, "start vector x* + psi_occ c")


def test_sternheimer_rhs_inside_the_occupied_span(mid):
    """Code path: safe_ratio.  Column 2 of rhs is a combination of psi_occ (Q rhs = rounding), column 4 is exactly zero
    (gamma = <p, c> = 0: alpha and beta are 0 / 0 without the guard).  Both sit inside the active range of their
    neighbours.  Status 0, not NUM_NONFINITE; those columns of dpsi are finite and below 1e-12; the others are the exact
    solution as if the two were not there."""
    s, n_occ = mid[1], 7
    rhs = s.unit_rhs(n_occ, 81)
    rhs[:, 2] = s.V[:, :n_occ] @ crandn(np.random.default_rng(82), n_occ)
    rhs[:, 2] /= np.linalg.norm(rhs[:, 2])
    rhs[:, 4] = 0.0
    out = solve(s, n_occ, rhs, 1e-10)
    assert out["status"] == 0, s.lib.dftk_mi_last_error()
    assert np.isfinite(out["x"]).all() and np.isfinite(out["residual_norms"]).all()
    assert np.linalg.norm(out["x"][:, [2, 4]], axis=0).max() < 1e-12
    check_solution(s, n_occ, rhs, out, "rhs inside the occupied span")


def test_sternheimer_refusals(mid):
    """Code path: the argument checks of the entry point.  More columns than plane waves, ld_rhs or ld_dpsi below n_G and a
    null tol return DFTK_MI_EINVAL and write nothing; n_occ = 0 returns 0 with *n_iter = 0 and *converged = 1."""
    s = mid[0]
    lib, n = s.lib, s.n
    n_occ = 4
    blk = padded(s.V[:, :n_occ], n)
    eps = np.ascontiguousarray(s.E[:n_occ])
    tol = np.full(n_occ, 1e-8)
    res = np.zeros(n_occ)

    def call(n_occ=n_occ, n_extra=0, extra=None, ld_rhs=n, ld_dpsi=n, tol_p=tol.ctypes.data):
        it, cv = C.c_int(-1), C.c_int(-1)
        st = lib.dftk_mi_sternheimer(s.kb.h, n_occ, blk.data_ptr(), n, eps.ctypes.data, n_extra, extra, n, blk.data_ptr(),
                                     ld_rhs, tol_p, 1, 10, None, 0, blk.data_ptr(), ld_dpsi, C.byref(it), res.ctypes.data,
                                     C.byref(cv))
        return st, it.value, cv.value

    assert call(n_extra=n - n_occ + 1, extra=blk.data_ptr())[0] == EINVAL      # n_occ + n_extra > n_G
    assert call(ld_rhs=n - 1)[0] == EINVAL
    assert call(ld_dpsi=n - 1)[0] == EINVAL
    assert call(tol_p=None)[0] == EINVAL
    assert call(n_occ=0) == (0, 0, 1)                                          # nothing to solve: converged at once
    s.bs.sync()
    assert np.array_equal(blk.cpu().numpy()[:, :n].T, s.V[:, :n_occ])          # no refused call wrote anything


# =========================================================================================== C: apply_kernel
FUNCTIONALS = {1: "lda_x", 2: "lda_c_vwn", 4: "lda_c_pw"}


def mp_eps(mask):
    """eps_xc(rho) of one functional in mpmath, from the constants in the comments and bodies of xc_kernels.hip"""
    mpf, pi = mpmath.mpf, mpmath.pi

    def rs_of(rho):
        return mpmath.cbrt(3 / (4 * pi * rho))

    if mask == 1:
        return lambda rho: -mpf(3) / 4 * mpmath.cbrt(3 / pi) * mpmath.cbrt(rho)
    if mask == 2:
        A, b, c, x0 = mpf("0.0310907"), mpf("3.72744"), mpf("12.9352"), mpf("-0.10498")

        def vwn(rho):
            x = mpmath.sqrt(rs_of(rho))
            X, X0 = x * x + b * x + c, x0 * x0 + b * x0 + c
            Q = mpmath.sqrt(4 * c - b * b)
            at = mpmath.atan(Q / (2 * x + b))
            return A * (mpmath.log(x * x / X) + 2 * b / Q * at
                        - b * x0 / X0 * (mpmath.log((x - x0) ** 2 / X) + 2 * (b + 2 * x0) / Q * at))
        return vwn
    a, a1 = mpf("0.031091"), mpf("0.21370")
    b1, b2, b3, b4 = mpf("7.5957"), mpf("3.5876"), mpf("1.6382"), mpf("0.49294")

    def pw(rho):
        rs = rs_of(rho)
        sq = mpmath.sqrt(rs)
        den = 2 * a * (b1 * sq + b2 * rs + b3 * rs * sq + b4 * rs * rs)
        return -2 * a * (1 + a1 * rs) * mpmath.log(1 + 1 / den)
    return pw


N_SPECIAL = 3
FXC_GRID = (8, 9, 10)


def build_fxc_table():
    """rho (720 values: a log grid from 1e-12 to 1e4, then 0, -1e-3 and 1e-301) and f_xc = d^2 (rho eps) / d rho^2 per
    functional at 60 digits, rounded to double"""
    n = FXC_GRID[0] * FXC_GRID[1] * FXC_GRID[2]
    rho = np.concatenate([np.logspace(-12, 4, n - N_SPECIAL), [0.0, -1e-3, 1e-301]])
    ref = {}
    with mpmath.workdps(60):
        for mask in FUNCTIONALS:
            eps = mp_eps(mask)
            ref[mask] = np.array([float(mpmath.diff(lambda r: r * eps(r), mpmath.mpf(float(v)), 2))
                                  for v in rho[:-N_SPECIAL]] + [0.0] * N_SPECIAL)
    return rho, ref


@pytest.fixture(scope="module")
def fxc_table():
    return build_fxc_table()


def cube_block(lib, nx, ny, nz):
    bs = Basis(lib, nx, ny, nz)
    N = nx * ny * nz
    return bs, KBlock(lib, bs, np.arange(N), np.zeros(N))


def apply_kernel(lib, bs, kb, rho, drho, green, mask):
    rho_d = dev(rho) if rho is not None else None
    drho_d = dev(drho)
    green_d = dev(green) if green is not None else None
    out = torch.full_like(drho_d, float("nan"))
    torch.cuda.synchronize()
    check(lib.dftk_mi_apply_kernel(kb.h, rho_d.data_ptr() if rho is not None else None, drho_d.data_ptr(),
                                   green_d.data_ptr() if green is not None else None, mask, out.data_ptr()))
    bs.sync()
    return out.cpu().numpy()


def test_fxc_pointwise_against_mpmath(lib, fxc_table):
    """drho = 1, no Green's function: dV is f_xc(rho) itself, on an 8 x 9 x 10 cube.  Relative 1e-12 per point from
    rho = 1e-12 to 1e4 for lda_x, lda_c_vwn and lda_c_pw (the closed forms cancel: 2/3 d1 - rs/3 d2, log1p(1 / den); a
    double-precision evaluation of the same forms on the host is within 4.8e-14 of the 60-digit reference, 1e-12 leaves 20
    times that for the device's cbrt, log and log1p); rho = 0, -1e-3 and 1e-301 give exactly 0; masks 3, 5, 7 are the sums.
    Measured on the MI355X, worst relative error: lda_x 4.2e-16 (rho = 1.6e-10), lda_c_vwn 7.5e-14 (rho = 1.8e-12), lda_c_pw
    1.6e-15 (rho = 4.8e-6)."""
    rho, ref = fxc_table
    nx, ny, nz = FXC_GRID
    bs, kb = cube_block(lib, nx, ny, nz)
    ones = np.ones_like(rho)
    got = {m: apply_kernel(lib, bs, kb, rho, ones, None, m) for m in (1, 2, 4, 3, 5, 7)}
    live = slice(0, len(rho) - N_SPECIAL)
    for m, name in FUNCTIONALS.items():
        assert np.all(ref[m][live] < 0)
        rel = np.abs(got[m][live] - ref[m][live]) / np.abs(ref[m][live])
        worst = int(np.argmax(rel))
        print(f"\nf_xc {name}: worst relative error {rel[worst]:.3e} at rho = {rho[worst]:.3e}")
        assert np.all(got[m][-N_SPECIAL:] == 0.0)
        assert rel.max() <= RTOL, (name, rho[worst], rel[worst])
    ulp = np.finfo(np.float64).eps
    for m in (3, 5, 7):
        parts = [k for k in FUNCTIONALS if m & k]
        total = sum(got[k] for k in parts)
        assert np.all(got[m][-N_SPECIAL:] == 0.0)
        assert np.all(np.abs(got[m] - total) <= 4 * ulp * np.abs(total))           # one rounding per addition
        exact = sum(ref[k] for k in parts)
        assert np.all(np.abs(got[m][live] - exact[live]) <= RTOL * np.abs(exact[live]))
    # refusals: an unknown functional bit, a functional without a density
    d = dev(ones)
    out = torch.zeros_like(d)
    assert lib.dftk_mi_apply_kernel(kb.h, d.data_ptr(), d.data_ptr(), None, 8, out.data_ptr()) == EINVAL
    assert lib.dftk_mi_apply_kernel(kb.h, None, d.data_ptr(), None, 1, out.data_ptr()) == EINVAL


@pytest.mark.parametrize("fft_size", [(15, 16, 25), (33, 16, 20)])
def test_hartree_and_fxc_on_non_cubic_grids(lib, fxc_table, fft_size):
    """Code path: the two cube FFTs of apply_kernel_lda with three different sizes (nx = 33 pads to nxp = 40; z plans 5.5 and
    5.4).  A random zero-mean drho and a random positive multiplier with green[0] = 0 against
    Re ifftn(green fftn(drho)); then mask 7 adds f_xc(rho) drho, rho drawn from the pointwise test's table (1e-2 .. 10) so
    that its 60-digit reference is reused."""
    nx, ny, nz = fft_size
    bs, kb = cube_block(lib, nx, ny, nz)
    rng = np.random.default_rng(nx + nz)
    drho = rng.standard_normal((nz, ny, nx))
    drho -= drho.mean()
    green = rng.uniform(0.1, 1.0, (nz, ny, nx))
    green[0, 0, 0] = 0.0
    ref_h = np.fft.ifftn(green * np.fft.fftn(drho)).real
    got_h = apply_kernel(lib, bs, kb, None, drho, green, 0)
    err_h = np.abs(got_h - ref_h).max() / np.abs(ref_h).max()
    table_rho, table_f = fxc_table
    pick = np.nonzero((table_rho >= 1e-2) & (table_rho <= 10.0))[0]
    idx = rng.choice(pick, size=(nz, ny, nx))
    rho = table_rho[idx]
    ref = ref_h + sum(table_f[m][idx] for m in FUNCTIONALS) * drho
    got = apply_kernel(lib, bs, kb, rho, drho, green, 7)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"\napply_kernel {fft_size}: Hartree rel max err {err_h:.3e}, Hartree + f_xc {err:.3e}")
    assert np.abs(ref - ref_h).max() > 0.1 * np.abs(ref_h).max()              # the XC part is not negligible here
    assert err_h <= RTOL
    assert err <= RTOL
