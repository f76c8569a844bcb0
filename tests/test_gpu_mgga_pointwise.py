"""The point-wise SCAN kernel of csrc/xc_kernels.hip (k_mgga: dual numbers with the slots d/d rho, d/d sigma, d/d tau) at the
C ABI, ``dftk_mi_xc_mgga``, against the 60-digit fixtures tests/golden/mgga_mp_*.json (tools/make_golden_xc.py).

Grid, error measure and bounds are those of tests/test_mgga_reference.py: rho = 1e-10 ... 1e3, s from 0 to 10, alpha from 0 to
100 with alpha = 1 and tau = 0 (alpha < 0) included; errors scaled by the LDA-exchange quantity of the same density, bound =
8 x max(E_REF, 4 x 2^-52) per functional, quantity and decade, E_REF being the error of the NumPy restatement
tests/mgga_ref.py against the same fixtures (measured on the CPU; nothing here is measured on the device).  The mask of both
functionals is held to the sum of its parts' bounds.  No grid point is skipped or masked: points at or below the threshold
are asserted to give exactly 0.0 in every output, every output buffer starts as NaN and must be written everywhere.

Every test prints the kernel's largest scaled error per decade (``pytest -s``).
"""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check as abi_check  # noqa: E402

import test_mgga_reference as R  # noqa: E402
from test_gpu_kernels import Basis, dev  # noqa: E402

XC_PASS = 1024 * 256               # XC_BLOCKS x 256 threads: one pass of the grid-stride loops of xc_kernels.hip
EINVAL = -1
MASKS = {64: "mgga_x_scan", 128: "mgga_c_scan", 192: "mgga_xc_scan"}
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs(lib):
    return Basis(lib, 15, 16, 25)


@pytest.fixture(scope="module")
def mgga():
    return R.load_mgga()


def nan_like(n):
    return torch.full((n,), NAN, dtype=torch.float64, device="cuda")


def xc_mgga(lib, bs, rho, sigma, tau, mask, threshold, pad=8):
    """(e, vrho, vsigma, vtau) of n points; the output buffers carry ``pad`` further NaNs that must survive the call"""
    n = len(rho)
    rd, sd, td = dev(rho), dev(sigma), dev(tau)
    out = [nan_like(n + pad) for _ in range(4)]
    torch.cuda.synchronize()
    abi_check(lib.dftk_mi_xc_mgga(bs.h, n, rd.data_ptr(), sd.data_ptr(), td.data_ptr(), mask, threshold,
                                  *(o.data_ptr() for o in out)))
    bs.sync()
    res = [o.cpu().numpy() for o in out]
    assert all(np.all(np.isnan(r[n:])) for r in res), "written past n"
    return [r[:n] for r in res]


@pytest.mark.parametrize("mask", sorted(MASKS))
def test_mgga_pointwise_against_mpmath(lib, bs, mgga, mask):
    """e, de/drho, de/dsigma, de/dtau of SCAN exchange (64), correlation (128) and both (192) point by point on the whole
    grid (sigma = 0, alpha = 1 as the grid rounds it, alpha < 0 included), tiled three times, then rho < 0, rho = 0 and live
    edge points (sigma = tau = 0; sigma far above 8 rho tau; a denormal-small tau).  Threshold 1e-30: the whole grid.
    Threshold 1e-8: exact zeros up to and including rho = 1e-8 itself, everything else bit for bit as before.  n = 1, 255,
    257 and one n above 262144 (the grid-stride loop wraps) reproduce the same bits."""
    fun = MASKS[mask]
    parts = ("mgga_x_scan", "mgga_c_scan") if mask == 192 else (fun,)
    ng = len(mgga.rho)
    tiles = 3
    extra = [(-1e-3, 1.0, 1.0), (-1e-40, 0.0, 0.0), (0.0, 1e-6, 1e-6), (1.0, 0.0, 0.0), (1.0, 0.0, float(R.gold.tau_unif(1.0))),
             (1.0, 1e3, 0.0), (1e-3, 0.0, 1e-300)]
    rho = np.concatenate([np.tile(mgga.rho, tiles), [x[0] for x in extra]])
    sigma = np.concatenate([np.tile(mgga.sigma, tiles), [x[1] for x in extra]])
    tau = np.concatenate([np.tile(mgga.tau, tiles), [x[2] for x in extra]])
    full = xc_mgga(lib, bs, rho, sigma, tau, mask, 1e-30)
    assert all(np.all(np.isfinite(o)) for o in full)
    for name, o in zip(R.QUANTITIES, full):
        assert np.all(o[tiles * ng:tiles * ng + 3] == 0.0), name          # rho <= 0
        for t in range(1, tiles):
            assert np.array_equal(o[t * ng:(t + 1) * ng], o[:ng]), (name, t)
        ref = sum(mgga.ref[p][name] for p in parts)
        scale = R.scale_of(name, mgga)
        bound = sum(R.bound_of((p, name), mgga.dec, R.MARGIN) for p in parts)
        err = R.scaled_error(o[:ng], ref, scale)
        print("XCMAX " + json.dumps({"key": [fun, name], "max": {str(d): v for d, v in R.decade_maxima(err, mgga.dec).items()}}))
        bad = np.flatnonzero(~(np.abs(o[:ng] - ref) <= bound * scale))
        assert bad.size == 0, (f"dftk_mi_xc_mgga mask {mask} {name}: {bad.size} points above the bound; worst scaled error "
                               f"{err[bad].max():.3e} (bound {bound[bad][np.argmax(err[bad])]:.3e}) at index "
                               f"{bad[np.argmax(err[bad])]}: kernel {o[bad[np.argmax(err[bad])]]!r}, "
                               f"reference {ref[bad[np.argmax(err[bad])]]!r}")
    e = full[0]
    assert np.all(e[tiles * ng + 3:] != 0.0)                              # the live edge points: finite (above), not skipped
    # the production-like threshold
    cut = xc_mgga(lib, bs, rho, sigma, tau, mask, 1e-8)
    dead = rho <= 1e-8
    assert np.any(rho == 1e-8) and np.any(dead & (rho > 0)) and np.any(~dead)
    for name, o, c in zip(R.QUANTITIES, full, cut):
        assert np.all(c[dead] == 0.0), name
        assert np.array_equal(c[~dead], o[~dead]), name
    # short calls, and one that wraps the grid-stride loop
    for n in (1, 255, 257):
        short = xc_mgga(lib, bs, rho[:n], sigma[:n], tau[:n], mask, 1e-30)
        assert all(np.array_equal(s, o[:n]) for s, o in zip(short, full)), n
    reps = XC_PASS // ng + 1
    assert reps * ng > XC_PASS
    long = xc_mgga(lib, bs, np.tile(mgga.rho, reps), np.tile(mgga.sigma, reps), np.tile(mgga.tau, reps), mask, 1e-30)
    for name, o, l in zip(R.QUANTITIES, full, long):
        assert np.array_equal(l.reshape(reps, ng), np.broadcast_to(o[:ng], (reps, ng))), name


def test_mgga_alpha_one_exactly_and_underflowing_gx(lib, bs):
    """alpha = 1 exactly: with sigma = 0, alpha = tau / tau_unif(rho).  The kernel's tau_unif may differ from the host's t in
    the last bit, so tau = t (1 - 2^-52), t, t (1 + 2^-52) are all passed: whichever the kernel sees as alpha = 1, as just below
    or as just above, the switching functions and their slopes are zero in double precision (exp(-1e15)), and what is left of
    v_tau is the exchange's 2 w dw/dalpha with w = b2 (1 - alpha) = 3e-17: |v_tau| tau_unif <= 1e-14 |e| covers it.
    g_x: at s = 3e-5 (a1 / p^(1/4) > 708) and at sigma = 0 the kernel takes g_x = 1 with zero derivatives: finite values, and
    v_sigma at s = 3e-5 equals the one at sigma = 0 to 1e-6 relative (the forms are smooth in p there)."""
    rho = np.array([0.3, 0.3, 0.3, 2.0, 2.0])
    t = R.gold.tau_unif(rho)
    tau = t * np.array([1 - 2.0 ** -52, 1.0, 1 + 2.0 ** -52, 1.0, 1.0])
    sigma = np.array([0.0, 0.0, 0.0, 0.0, (3e-5) ** 2 * float(R.gold.sigma_unit(2.0))])
    for mask in (64, 128, 192):
        e, vr, vs, vt = xc_mgga(lib, bs, rho, sigma, tau, mask, 1e-12)
        assert all(np.all(np.isfinite(o)) for o in (e, vr, vs, vt))
        assert np.all(np.abs(vt[:4]) * t[:4] <= 1e-14 * np.abs(e[:4]))
        assert np.all(e < 0)
        assert abs(vs[4] - vs[3]) <= 1e-6 * abs(vs[3]) and vs[3] != 0.0


def test_mgga_refusals_write_nothing(lib, bs):
    """masks 0, 8, 64 | 8 and 256 return EINVAL and write nothing; so does a missing operand"""
    n = 600
    d = dev(np.ones(n))
    out = nan_like(n)
    p = out.data_ptr()
    for bad_mask in (0, 8, 64 | 8, 256, 192 | 1, 64 | 256):
        assert lib.dftk_mi_xc_mgga(bs.h, n, d.data_ptr(), d.data_ptr(), d.data_ptr(), bad_mask, 1e-12, p, p, p, p) == EINVAL
    assert lib.dftk_mi_xc_mgga(bs.h, n, d.data_ptr(), d.data_ptr(), None, 192, 1e-12, p, p, p, p) == EINVAL
    assert lib.dftk_mi_xc_mgga(bs.h, n, d.data_ptr(), d.data_ptr(), d.data_ptr(), 192, 1e-12, p, p, p, None) == EINVAL
    bs.sync()
    assert np.all(np.isnan(out.cpu().numpy()))
    # the other point-wise entry keeps refusing the new bits
    for bad_mask in (64, 128, 192, 8 | 64):
        assert lib.dftk_mi_xc_gga(bs.h, n, d.data_ptr(), d.data_ptr(), bad_mask, 1e-12, p, p, p) == EINVAL
    bs.sync()
    assert np.all(np.isnan(out.cpu().numpy()))
