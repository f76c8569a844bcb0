"""The point-wise exchange-correlation kernels of csrc/xc_kernels.hip at the C ABI against the 60-digit fixtures
tests/golden/xc_mp_*.json (tools/make_golden_xc.py), over the whole density range: 1e-30 ... 1e5, reduced gradients from
0 to 100, polarisations up to +-1, and the values next to every guard and floor of the kernels.

Entry points: ``dftk_mi_xc_gga`` (k_gga: dual-number PBE), ``dftk_mi_local_potential`` (k_xc_sum: lda_x, lda_c_vwn,
lda_c_pw with hand-derived first derivatives, lda_xc_teter93), ``dftk_mi_local_potential_collinear`` (k_xc_sum_spin) and
``dftk_mi_apply_kernel`` (k_fxc_sum: hand-derived second derivatives).  V_loc and the Poisson multiplier are NULL, so that
nothing but the point-wise pass runs, on a 15 x 16 x 25 cube (6000 points: 23 blocks and a partial one).

Error measure and bounds are those of tests/test_xc_reference.py: errors scaled by the LDA-exchange quantity of the same
density, bound = 8 x max(E_REF, 4 x 2^-52) per functional, quantity and decade, E_REF being the error of the NumPy forms of
oracle/terms.py against the same fixtures (measured on the CPU; nothing here is measured on the device).  A mask of
several functionals is held to the sum of its parts' bounds.  Energies are only available as a sum over the cube: they are
taken decade by decade (all other points 0), against the fixture's sum, within the sum of the per-point bounds -- the
device's reduction adds fewer roundings over the at most 44 non-zero terms than the floor of 32 ulp per term leaves.
No grid point is skipped or masked: points at or below a threshold are asserted to give exactly 0.0 in every output, every
output buffer starts as NaN and must be written everywhere.

Every test prints the kernel's largest scaled error per decade (``pytest -s``); DESIGN.md section 3.6.1 records them.
"""
import ctypes as C
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check as abi_check  # noqa: E402

import test_xc_reference as R  # noqa: E402
from test_gpu_kernels import Basis, KBlock, dev  # noqa: E402

CUBE = (15, 16, 25)
N = CUBE[0] * CUBE[1] * CUBE[2]
DVOL = 1.0 / N                     # Basis(...) has unit volume
XC_PASS = 1024 * 256               # XC_BLOCKS x 256 threads: one pass of the grid-stride loops of xc_kernels.hip
EINVAL = -1
LDA_BITS = {1: "lda_x", 2: "lda_c_vwn", 4: "lda_c_pw", 32: "lda_xc_teter93"}
GGA_MASKS = {8: "gga_x_pbe", 16: "gga_c_pbe", 24: "gga_xc_pbe"}
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def cube(lib):
    bs = Basis(lib, *CUBE)
    return bs, KBlock(lib, bs, np.arange(N), np.zeros(N))


@pytest.fixture(scope="module")
def lda():
    return R.load_lda()


@pytest.fixture(scope="module")
def gga():
    return R.load_gga()


@pytest.fixture(scope="module")
def spin():
    return R.load_spin()


def nan_like(n):
    return torch.full((n,), NAN, dtype=torch.float64, device="cuda")


def within(keys, got, refs, scale, dec, label):
    """|got - sum refs| <= sum_k 8 max(E_REF_k, FLOOR) scale at every point; returns the scaled errors"""
    ref = sum(refs)
    bound = sum(R.bound_of(k, dec, R.MARGIN) for k in keys)
    err = R.scaled_error(got, ref, scale)
    bad = np.flatnonzero(~(np.abs(got - ref) <= bound * scale))
    assert bad.size == 0, (f"{label} {keys}: {bad.size} points above the bound; worst scaled error {err[bad].max():.3e} "
                           f"(bound {bound[bad][np.argmax(err[bad])]:.3e}) at index {bad[np.argmax(err[bad])]}: "
                           f"kernel {got[bad[np.argmax(err[bad])]]!r}, reference {ref[bad[np.argmax(err[bad])]]!r}")
    return err


def report(key, err, dec):
    print("XCMAX " + json.dumps({"key": list(key), "max": {str(d): v for d, v in R.decade_maxima(err, dec).items()}}))


def spread(k):
    """k distinct cube positions spread over the blocks of the launch"""
    idx = (np.arange(k) * 131 + 7) % N
    assert len(set(idx.tolist())) == k
    return idx


# ================================================================================================ dftk_mi_xc_gga
def xc_gga(lib, bs, rho, sigma, mask, threshold, pad=8):
    """(e, vrho, vsigma) of n points; the output buffers carry ``pad`` further NaNs that must survive the call"""
    n = len(rho)
    rd, sd = dev(rho), dev(sigma)
    out = [nan_like(n + pad) for _ in range(3)]
    torch.cuda.synchronize()
    abi_check(lib.dftk_mi_xc_gga(bs.h, n, rd.data_ptr(), sd.data_ptr(), mask, threshold, *(o.data_ptr() for o in out)))
    bs.sync()
    res = [o.cpu().numpy() for o in out]
    assert all(np.all(np.isnan(r[n:])) for r in res), "written past n"
    return [r[:n] for r in res]


@pytest.mark.parametrize("mask", sorted(GGA_MASKS))
def test_gga_pointwise_against_mpmath(lib, cube, gga, mask):
    """e, de/drho, de/dsigma of PBE exchange (8), correlation (16) and both (24) point by point, rho from 1e-28 to 1e4 and
    s in {0, 1e-6, 1e-3, 0.1, 1, 3, 10, 100} (sigma = 0 at finite rho included), tiled five times over 6000 points, then
    rho < 0 and rho = 0.  Threshold 1e-30: the whole grid.  Threshold 1e-12 (the production value): exact zeros up to and
    including rho = 1e-12 itself, everything else bit for bit as before.  n = 1, 255, 257 and n = 263160 (more than one
    pass of 262144 threads: the grid-stride loop wraps) reproduce the same bits."""
    bs, _ = cube
    fun = GGA_MASKS[mask]
    ng = len(gga.rho)
    tiles = 5
    rho, sigma = np.zeros(N), np.zeros(N)
    rho[:tiles * ng], sigma[:tiles * ng] = np.tile(gga.rho, tiles), np.tile(gga.sigma, tiles)
    rho[tiles * ng:tiles * ng + 3] = [-1e-3, -1e-40, 0.0]
    sigma[tiles * ng:tiles * ng + 3] = [1.0, 0.0, 1e-6]
    full = xc_gga(lib, bs, rho, sigma, mask, 1e-30)
    assert all(np.all(np.isfinite(o)) for o in full)
    for name, o in zip(("e", "vrho", "vsigma"), full):
        assert np.all(o[tiles * ng:] == 0.0), name
        for t in range(1, tiles):
            assert np.array_equal(o[t * ng:(t + 1) * ng], o[:ng]), (name, t)
        err = within([("gga", fun, name)], o[:ng], [gga.ref[fun][name]], R.scale_of(name, gga.rho, gga.sigma), gga.dec,
                     f"dftk_mi_xc_gga mask {mask}")
        report(("gga", fun, name), err, gga.dec)
    # the production threshold
    cut = xc_gga(lib, bs, rho, sigma, mask, 1e-12)
    dead = rho <= 1e-12
    assert np.any(rho == 1e-12) and np.any(dead & (rho > 0)) and np.any(~dead)
    for name, o, c in zip(("e", "vrho", "vsigma"), full, cut):
        assert np.all(c[dead] == 0.0), name
        assert np.array_equal(c[~dead], o[~dead]), name
    # short calls, and one that wraps the grid-stride loop
    for n in (1, 255, 257):
        short = xc_gga(lib, bs, rho[:n], sigma[:n], mask, 1e-30)
        assert all(np.array_equal(s, o[:n]) for s, o in zip(short, full)), n
    reps = XC_PASS // ng + 1
    assert reps * ng > XC_PASS
    long = xc_gga(lib, bs, np.tile(gga.rho, reps), np.tile(gga.sigma, reps), mask, 1e-30)
    for name, o, l in zip(("e", "vrho", "vsigma"), full, long):
        assert np.array_equal(l.reshape(reps, ng), np.broadcast_to(o[:ng], (reps, ng))), name
    # refusals
    rd = dev(rho)
    out = nan_like(N)
    for bad_mask in (0, 1, 8 | 32, 24 | 4):
        assert lib.dftk_mi_xc_gga(bs.h, N, rd.data_ptr(), rd.data_ptr(), bad_mask, 1e-12, out.data_ptr(), out.data_ptr(),
                                  out.data_ptr()) == EINVAL
    bs.sync()
    assert np.all(np.isnan(out.cpu().numpy()))


# ================================================================================================ dftk_mi_local_potential
def local_potential(lib, cube, rho, mask):
    bs, kb = cube
    rd = dev(rho)
    V = nan_like(N)
    E = (C.c_double * 3)(NAN, NAN, NAN)
    torch.cuda.synchronize()
    abi_check(lib.dftk_mi_local_potential(kb.h, rd.data_ptr(), None, None, mask, V.data_ptr(), E))
    bs.sync()
    return V.cpu().numpy(), list(E)


def parts_of(mask):
    return [name for bit, name in LDA_BITS.items() if mask & bit]


@pytest.mark.parametrize("mask", [1, 2, 4, 32, 1 | 4])
def test_lda_potential_and_energy_against_mpmath(lib, cube, lda, mask):
    """V_out = v_xc point by point over rho = 1e-30 ... 1e5 plus 1e-300 (1 + 2^-52) (just above the rho > 1e-300 guard) and
    2e-20, 2.0000001e-20, 4e-20, 4.0000001e-20 (around the floor of the Teter path), tiled over the cube as often as it
    fits, the rest 0.  E_xc decade by decade.  rho in {0, -1e-9, 1e-320, 1e-301} gives e = v = 0."""
    parts = parts_of(mask)
    ng = len(lda.rho)
    tiles = N // ng
    rho = np.zeros(N)
    rho[:tiles * ng] = np.tile(lda.rho, tiles)
    V, E = local_potential(lib, cube, rho, mask)
    assert np.all(np.isfinite(V)) and E[0] == 0.0 and E[2] == 0.0 and math.isfinite(E[1])
    assert np.all(V[tiles * ng:] == 0.0)
    for t in range(1, tiles):
        assert np.array_equal(V[t * ng:(t + 1) * ng], V[:ng]), t
    err = within([("lda", p, "v") for p in parts], V[:ng], [lda.ref[p]["v"] for p in parts], R.scale_of("v", lda.rho),
                 lda.dec, f"dftk_mi_local_potential mask {mask}")
    if len(parts) == 1:
        report(("lda", parts[0], "v"), err, lda.dec)
    if mask == 32:                                        # the collinear floor: rho / 2 + rho / 2 <= 2e-20
        assert np.any(lda.rho == 2e-20) and np.all(V[:ng][lda.rho <= 2e-20] == 0.0)
        assert np.all(V[:ng][lda.rho > 2e-20] < 0.0)
    # energies: one call per decade
    e_err = {}
    for d in np.unique(lda.dec):
        sel = np.flatnonzero(lda.dec == d)
        rho_d = np.zeros(N)
        rho_d[spread(len(sel))] = lda.rho[sel]
        _, Ed = local_potential(lib, cube, rho_d, mask)
        ref = math.fsum(float(lda.ref[p]["e"][i]) for p in parts for i in sel) * DVOL
        scale = R.scale_of("e", lda.rho[sel])
        bound = float(np.sum(sum(R.bound_of(("lda", p, "e"), lda.dec[sel], R.MARGIN) for p in parts) * scale)) * DVOL
        assert abs(Ed[1] - ref) <= bound, (mask, int(d), Ed[1], ref, bound)
        total = float(np.sum(scale)) * DVOL
        e_err[int(d)] = 0.0 if Ed[1] == ref else (abs(Ed[1] - ref) / total if total > 0 else math.inf)
    if len(parts) == 1:
        print("XCMAX " + json.dumps({"key": ["lda", parts[0], "E_xc"], "max": {str(d): v for d, v in e_err.items()}}))
    # the guards
    rho_g = np.zeros(N)
    rho_g[spread(4)] = [0.0, -1e-9, 1e-320, 1e-301]
    Vg, Eg = local_potential(lib, cube, rho_g, mask)
    assert np.all(Vg == 0.0) and Eg == [0.0, 0.0, 0.0]


def test_lda_potential_refuses_other_bits(lib, cube):
    bs, kb = cube
    rd = dev(np.ones(N))
    V = nan_like(N)
    E = (C.c_double * 3)(7.0, 7.0, 7.0)
    for bad_mask in (8, 16, 64, 1 | 8):
        assert lib.dftk_mi_local_potential(kb.h, rd.data_ptr(), None, None, bad_mask, V.data_ptr(), E) == EINVAL
    bs.sync()
    assert np.all(np.isnan(V.cpu().numpy())) and list(E) == [7.0, 7.0, 7.0]


# ================================================================================================ ..._collinear
def collinear(lib, cube, up, dn, mask):
    bs, kb = cube
    rd = dev(np.stack([up, dn]))
    V = nan_like(2 * N)
    E = (C.c_double * 3)(NAN, NAN, NAN)
    torch.cuda.synchronize()
    abi_check(lib.dftk_mi_local_potential_collinear(kb.h, rd.data_ptr(), None, None, mask, V.data_ptr(), E))
    bs.sync()
    V = V.cpu().numpy()
    return V[:N], V[N:], list(E)


@pytest.mark.parametrize("mask", [1, 4, 32, 1 | 4])
def test_collinear_potential_and_energy_against_mpmath(lib, cube, spin, mask):
    """V_up, V_down point by point over rho_t = 1e-18 ... 1e4 and zeta in {0, +-1e-8, +-0.3, +-0.9, +-(1 - 1e-10), +-1}
    (zeta = +-1: a channel that is exactly 0), tiled six times.  A channel that is slightly negative, at the floor 1e-20 or below
    it gives the bits of the channel at 0 (all are evaluated at 1e-20).  rho_up + rho_down <= 2e-20 gives exact zeros.
    Exchanging the cubes exchanges V_up and V_down bit for bit.  E_xc decade by decade."""
    parts = parts_of(mask)
    ng = len(spin.rho)
    tiles = N // ng
    up, dn = np.zeros(N), np.zeros(N)
    up[:tiles * ng], dn[:tiles * ng] = np.tile(spin.up, tiles), np.tile(spin.dn, tiles)
    # edge points behind the tiles: fully polarised grid points with the empty channel replaced, in both orders
    polarised = np.flatnonzero((spin.dn == 0.0) & np.isin(spin.rho, [1e-18, 1e-3, 1e3]))
    assert len(polarised) == 3
    pos = tiles * ng
    twins = []
    for i in polarised:
        for empty in (-1e-25, 1e-20, 5e-21):
            up[pos], dn[pos] = spin.up[i], empty
            up[pos + 1], dn[pos + 1] = empty, spin.up[i]
            twins.append((pos, i))
            pos += 2
    below = [(1e-20, 1e-20), (5e-21, 1e-20), (-1.0, 1e-21), (2e-20, -3e-20), (0.0, 2e-20), (0.0, 0.0)]
    for a, b in below:
        up[pos], dn[pos] = a, b
        pos += 1
    assert pos < N
    Vu, Vd, E = collinear(lib, cube, up, dn, mask)
    assert np.all(np.isfinite(Vu)) and np.all(np.isfinite(Vd)) and E[0] == 0.0 and E[2] == 0.0 and math.isfinite(E[1])
    assert np.all(Vu[pos - len(below):] == 0.0) and np.all(Vd[pos - len(below):] == 0.0)
    for t in range(1, tiles):
        assert np.array_equal(Vu[t * ng:(t + 1) * ng], Vu[:ng]) and np.array_equal(Vd[t * ng:(t + 1) * ng], Vd[:ng]), t
    for p, i in twins:
        assert Vu[p] == Vu[i] and Vd[p] == Vd[i], (p, i)
        assert Vu[p + 1] == Vd[i] and Vd[p + 1] == Vu[i], (p, i)
    for q, V in (("vup", Vu), ("vdn", Vd)):
        err = within([("spin", p, q) for p in parts], V[:ng], [spin.ref[p][q] for p in parts], R.scale_of(q, spin.rho),
                     spin.dec, f"dftk_mi_local_potential_collinear mask {mask}")
        if len(parts) == 1:
            report(("spin", parts[0], q), err, spin.dec)
    # swap symmetry
    Su, Sd, _ = collinear(lib, cube, dn, up, mask)
    assert np.array_equal(Su, Vd) and np.array_equal(Sd, Vu)
    # energies: one call per decade
    e_err = {}
    for d in np.unique(spin.dec):
        sel = np.flatnonzero(spin.dec == d)
        up_d, dn_d = np.zeros(N), np.zeros(N)
        where = spread(len(sel))
        up_d[where], dn_d[where] = spin.up[sel], spin.dn[sel]
        _, _, Ed = collinear(lib, cube, up_d, dn_d, mask)
        ref = math.fsum(float(spin.ref[p]["e"][i]) for p in parts for i in sel) * DVOL
        scale = R.scale_of("e", spin.rho[sel])
        bound = float(np.sum(sum(R.bound_of(("spin", p, "e"), spin.dec[sel], R.MARGIN) for p in parts) * scale)) * DVOL
        assert abs(Ed[1] - ref) <= bound, (mask, int(d), Ed[1], ref, bound)
        e_err[int(d)] = abs(Ed[1] - ref) / (float(np.sum(scale)) * DVOL)
    if len(parts) == 1:
        print("XCMAX " + json.dumps({"key": ["spin", parts[0], "E_xc"], "max": {str(d): v for d, v in e_err.items()}}))


def test_collinear_refuses_unpolarised_only_forms(lib, cube):
    """lda_c_vwn (2) and the GGA bits (8, 16) have no spin-polarised form in the library: DFTK_MI_EINVAL, nothing written"""
    bs, kb = cube
    rd = dev(np.ones(2 * N))
    V = nan_like(2 * N)
    E = (C.c_double * 3)(7.0, 7.0, 7.0)
    for bad_mask in (2, 8, 16, 24, 1 | 2, 4 | 8, 64):
        assert lib.dftk_mi_local_potential_collinear(kb.h, rd.data_ptr(), None, None, bad_mask, V.data_ptr(), E) == EINVAL
    bs.sync()
    assert np.all(np.isnan(V.cpu().numpy())) and list(E) == [7.0, 7.0, 7.0]


# ================================================================================================ dftk_mi_apply_kernel
def apply_kernel(lib, cube, rho, drho, mask):
    bs, kb = cube
    rd, dd = dev(rho), dev(drho)
    out = nan_like(N)
    torch.cuda.synchronize()
    abi_check(lib.dftk_mi_apply_kernel(kb.h, rd.data_ptr(), dd.data_ptr(), None, mask, out.data_ptr()))
    bs.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("mask", [1, 2, 4, 7])
def test_fxc_against_mpmath(lib, cube, lda, mask):
    """With drho = 1, dV is f_xc = d2e/drho2 itself: against the 60-digit second derivative from 1e-30 to 1e5 and just
    above the guard, 1e-300 (1 + 2^-52).  With a sign-alternating drho of magnitudes 1e-10 ... 1e3, dV = f_xc drho: the same
    bound times |drho|, and bit for bit the product of the first result with drho.  rho <= 1e-300 gives 0."""
    parts = parts_of(mask)
    ng = len(lda.rho)
    tiles = N // ng
    rho = np.zeros(N)
    rho[:tiles * ng] = np.tile(lda.rho, tiles)
    rho[tiles * ng:tiles * ng + 4] = [1e-300, -1.0, 1e-301, 1e-320]
    f = apply_kernel(lib, cube, rho, np.ones(N), mask)
    assert np.all(np.isfinite(f)) and np.all(f[tiles * ng:] == 0.0)
    for t in range(1, tiles):
        assert np.array_equal(f[t * ng:(t + 1) * ng], f[:ng]), t
    scale = R.scale_of("f", lda.rho)
    err = within([("lda", p, "f") for p in parts], f[:ng], [lda.ref[p]["f"] for p in parts], scale, lda.dec,
                 f"dftk_mi_apply_kernel mask {mask}")
    if len(parts) == 1:
        report(("lda", parts[0], "f"), err, lda.dec)
    drho = np.where(np.arange(N) % 2 == 0, 1.0, -1.0) * 10.0 ** (np.arange(N) % 14 - 10.0)
    assert drho.min() < -999.0 and np.abs(drho).min() < 1.1e-10 and drho.max() > 99.0
    dV = apply_kernel(lib, cube, rho, drho, mask)
    assert np.array_equal(dV, f * drho)
    within([("lda", p, "f") for p in parts], dV[:ng], [lda.ref[p]["f"] * drho[:ng] for p in parts],
           scale * np.abs(drho[:ng]), lda.dec, f"dftk_mi_apply_kernel mask {mask}, alternating drho")


def test_apply_kernel_refuses_other_bits(lib, cube):
    bs, kb = cube
    d = dev(np.ones(N))
    out = nan_like(N)
    for bad_mask in (8, 16, 32, 1 | 32, 64):
        assert lib.dftk_mi_apply_kernel(kb.h, d.data_ptr(), d.data_ptr(), None, bad_mask, out.data_ptr()) == EINVAL
    bs.sync()
    assert np.all(np.isnan(out.cpu().numpy()))
