"""The spin-polarised PBE kernel of csrc/xc_kernels.hip (k_gga_spin) at the C ABI, ``dftk_mi_xc_gga_spin``, against the
60-digit fixtures tests/golden/xc_spingga_mp_*.json (tools/make_golden_xc_spin_gga.py): rho = 1e-18 ... 1e4, zeta up to +-1,
s in {0, 1e-3, 1, 10}, sigma_ud of both signs, on the 15 x 16 x 25 cube of tests/test_gpu_xc_pointwise.py (6000 points: 23
blocks and a partial one).

Error measure and bounds are those of tests/test_xc_spin_gga_reference.py: errors scaled by the LDA-exchange quantity of the
same total density, bound = 8 x max(E_REF, 4 x 2^-52) per functional, quantity and decade, E_REF being the error of the NumPy
restatement in that file against the same fixtures (measured on the CPU; nothing here is measured on the device).  Both
bits together are held to the sum of the two bounds.  The decades of E_REF are dominated by their fully polarised points, so
the points with |zeta| <= 0.9 are held to the bound from E_REF_INNER (the same measurement over those points) as well.  No
point is skipped; every output starts as NaN with padding that must survive.

The test prints the kernel's largest scaled error per decade (``pytest -s``); DESIGN.md section 3.6.1 records them.
"""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check as abi_check  # noqa: E402

import test_xc_reference as R  # noqa: E402
import test_xc_spin_gga_reference as S  # noqa: E402
from test_gpu_kernels import Basis, dev  # noqa: E402

CUBE = (15, 16, 25)
N = CUBE[0] * CUBE[1] * CUBE[2]
EINVAL = -1
MASKS = {8: "gga_x_pbe", 16: "gga_c_pbe", 24: "gga_xc_pbe"}
NAN = float("nan")
PAD = 8


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs(lib):
    return Basis(lib, *CUBE)


@pytest.fixture(scope="module")
def sg():
    return S.load_spingga()


def xc_gga_spin(lib, bs, up, dn, suu, sud, sdd, mask, threshold):
    """the six outputs of n points as a dict; the three output buffers carry PAD further NaNs that must survive the call"""
    n = len(up)
    rd, sd = dev(np.concatenate([up, dn])), dev(np.concatenate([suu, sud, sdd]))
    out = [torch.full((k * n + PAD,), NAN, dtype=torch.float64, device="cuda") for k in (1, 2, 3)]
    torch.cuda.synchronize()
    abi_check(lib.dftk_mi_xc_gga_spin(bs.h, n, rd.data_ptr(), sd.data_ptr(), mask, threshold, *(o.data_ptr() for o in out)))
    bs.sync()
    e, vr, vs = (o.cpu().numpy() for o in out)
    assert all(np.all(np.isnan(a[k * n:])) for a, k in ((e, 1), (vr, 2), (vs, 3))), "written past n"
    return {"e": e[:n], "vup": vr[:n], "vdn": vr[n:2 * n], "vsuu": vs[:n], "vsud": vs[n:2 * n], "vsdd": vs[2 * n:3 * n]}


def on_cube(sg):
    """the grid tiled over the cube as often as it fits, then the edge points; returns the five inputs and the edge offset"""
    ng = len(sg.rho)
    tiles = N // ng
    arr = {k: np.zeros(N) for k in ("up", "dn", "suu", "sud", "sdd")}
    for k in arr:
        arr[k][:tiles * ng] = np.tile(getattr(sg, k), tiles)
    return arr, ng, tiles


@pytest.mark.parametrize("mask", sorted(MASKS))
def test_spin_gga_pointwise_against_mpmath(lib, bs, sg, mask):
    """e, de/drho_up, de/drho_down, de/dsigma_uu, de/dsigma_ud, de/dsigma_dd of PBE exchange (8), correlation (16) and both (24)
    at every grid point, tiled over the cube.  Exchange has de/dsigma_ud = 0 exactly; correlation has de/dsigma_uu =
    de/dsigma_dd = de/dsigma_ud / 2 bit for bit.  Short calls (n = 1, 255, 257) reproduce the same bits."""
    fun = MASKS[mask]
    parts = sgold_parts(mask)
    arr, ng, tiles = on_cube(sg)
    out = xc_gga_spin(lib, bs, arr["up"], arr["dn"], arr["suu"], arr["sud"], arr["sdd"], mask, 1e-30)
    inner = S.inner_points(sg)
    for q in S.OUTPUTS:
        o = out[q]
        assert np.all(np.isfinite(o)), q
        assert np.all(o[tiles * ng:] == 0.0), q
        for t in range(1, tiles):
            assert np.array_equal(o[t * ng:(t + 1) * ng], o[:ng]), (q, t)
        got, ref, scale = o[:ng], sg.ref[fun][q], S.scale_of(q, sg)
        err = R.scaled_error(got, ref, scale)
        print("XCMAX " + json.dumps({"key": ["spingga", fun, q], "max": {str(d): v for d, v in R.decade_maxima(err, sg.dec).items()},
                                      "inner": {str(d): v for d, v in R.decade_maxima(err[inner], sg.dec[inner]).items()}}))
        for only_inner in (False, True):
            bound = sum(S.bound_of((p, q), sg.dec, S.MARGIN, only_inner) for p in parts)
            bad = np.flatnonzero(~(np.abs(got - ref) <= bound * scale) & (inner | (not only_inner)))
            assert bad.size == 0, (f"mask {mask} {q} (inner {only_inner}): {bad.size} points above the bound; worst scaled error "
                                   f"{err[bad].max():.3e} (bound {bound[bad][np.argmax(err[bad])]:.3e}) at index "
                                   f"{bad[np.argmax(err[bad])]}: kernel {got[bad[np.argmax(err[bad])]]!r}, reference "
                                   f"{ref[bad[np.argmax(err[bad])]]!r}")
    if mask == 8:
        assert np.all(out["vsud"] == 0.0)
    if mask == 16:
        assert np.array_equal(out["vsuu"], out["vsdd"]) and np.array_equal(2.0 * out["vsuu"], out["vsud"])
    for n in (1, 255, 257):
        short = xc_gga_spin(lib, bs, *(arr[k][:n] for k in ("up", "dn", "suu", "sud", "sdd")), mask, 1e-30)
        assert all(np.array_equal(short[q], out[q][:n]) for q in S.OUTPUTS), n


def sgold_parts(mask):
    return [name for bit, name in ((8, "gga_x_pbe"), (16, "gga_c_pbe")) if mask & bit]


@pytest.mark.parametrize("mask", sorted(MASKS))
def test_exchanging_the_channels_exchanges_the_outputs(lib, bs, sg, mask):
    """(rho_up, sigma_uu) <-> (rho_down, sigma_dd): de/drho_up <-> de/drho_down and de/dsigma_uu <-> de/dsigma_dd bit for bit,
    e and de/dsigma_ud unchanged to the bit."""
    arr, _, _ = on_cube(sg)
    a = xc_gga_spin(lib, bs, arr["up"], arr["dn"], arr["suu"], arr["sud"], arr["sdd"], mask, 1e-12)
    b = xc_gga_spin(lib, bs, arr["dn"], arr["up"], arr["sdd"], arr["sud"], arr["suu"], mask, 1e-12)
    assert np.any(a["vup"] != a["vdn"])
    for qa, qb in (("e", "e"), ("vsud", "vsud"), ("vup", "vdn"), ("vdn", "vup"), ("vsuu", "vsdd"), ("vsdd", "vsuu")):
        assert np.array_equal(a[qa], b[qb]), (qa, qb)


@pytest.mark.parametrize("mask", sorted(MASKS))
def test_floors_and_threshold(lib, bs, sg, mask):
    """A channel that is slightly negative, at the floor 1e-20 or below it gives the bits of the channel at 0 (all are evaluated
    at 1e-20).  rho_up + rho_down <= max(threshold, 2e-20) gives exact zeros in all six outputs -- at the threshold itself too --
    and everything above it is bit for bit what the call with a tiny threshold gives.  Negative sigma_uu, sigma_dd and sigma_tot
    are evaluated at 0."""
    arr, ng, tiles = on_cube(sg)
    keys = ("up", "dn", "suu", "sud", "sdd")
    pos = tiles * ng
    polarised = np.flatnonzero((sg.dn == 0.0) & np.isin(sg.rho, [1e-18, 1e-3, 1e3]) & (sg.s == 1.0) & (sg.cos == 1.0))
    assert len(polarised) == 3
    twins = []
    for i in polarised:
        for empty in (-1e-25, 1e-20, 5e-21):
            for k in keys:
                arr[k][pos] = getattr(sg, k)[i]
            arr["dn"][pos] = empty
            twins.append((pos, i))
            pos += 1
    neg = pos                                   # negative sigma against sigma = 0
    for vals in ((1e-3, 2e-3, -1e-9, 0.0, -1e-9), (1e-3, 2e-3, 0.0, 0.0, 0.0), (1e-3, 2e-3, 1e-9, -2e-9, 1e-9),
                 (1e-3, 2e-3, 1e-9, -1e-9, 1e-9)):
        for k, v in zip(keys, vals):
            arr[k][pos] = v
        pos += 1
    below = [(1e-20, 1e-20), (5e-21, 1e-20), (-1.0, 1e-21), (2e-20, -3e-20), (0.0, 2e-20), (0.0, 0.0)]
    first_below = pos
    for a, b in below:
        arr["up"][pos], arr["dn"][pos], arr["suu"][pos], arr["sud"][pos], arr["sdd"][pos] = a, b, 1e-40, 1e-41, 1e-40
        pos += 1
    assert pos < N
    full = xc_gga_spin(lib, bs, *(arr[k] for k in keys), mask, 1e-30)
    for q in S.OUTPUTS:
        o = full[q]
        assert np.all(np.isfinite(o)) and np.all(o[first_below:] == 0.0), q
        for p, i in twins:
            assert o[p] == o[i], (q, p, i)
        assert o[neg] == o[neg + 1], q          # sigma_uu = sigma_dd = -1e-9 -> 0
    if mask & 16:                               # sigma_tot = -2e-9 is evaluated at 0: as sigma_tot = 0 (correlation only)
        c_neg = xc_gga_spin(lib, bs, *(arr[k][neg + 2:neg + 4] for k in keys), 16, 1e-30)
        assert all(c_neg[q][0] == c_neg[q][1] for q in S.OUTPUTS)
    cut = xc_gga_spin(lib, bs, *(arr[k] for k in keys), mask, 1e-12)
    tot = arr["up"] + arr["dn"]
    dead = tot <= 1e-12
    assert np.any(tot == 1e-12) and np.any(dead & (tot > 2e-20)) and np.any(~dead)
    for q in S.OUTPUTS:
        assert np.all(cut[q][dead] == 0.0), q
        assert np.array_equal(cut[q][~dead], full[q][~dead]), q


def test_refusals_write_nothing(lib, bs):
    rd = dev(np.ones(3 * N))
    out = torch.full((3 * N,), NAN, dtype=torch.float64, device="cuda")
    for bad_mask in (2, 64, 8 | 2, 0, 1, 8 | 32):
        assert lib.dftk_mi_xc_gga_spin(bs.h, N, rd.data_ptr(), rd.data_ptr(), bad_mask, 1e-12, out.data_ptr(), out.data_ptr(),
                                       out.data_ptr()) == EINVAL
    bs.sync()
    assert np.all(np.isnan(out.cpu().numpy()))
