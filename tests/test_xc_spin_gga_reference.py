"""The spin-polarised PBE forms against a 60-digit reference (host side).

tests/golden/xc_spingga_mp_*.json hold e, de/drho_up, de/dsigma_uu, de/dsigma_ud of the polarised gga_x_pbe and gga_c_pbe,
computed by tools/make_golden_xc_spin_gga.py in mpmath from the energy densities alone (every derivative is ``mpmath.diff``):
rho = 1e-18 ... 1e4 by decade, zeta in {0, +-0.3, +-0.9, +-(1 - 1e-6), +-1}, s in {0, 1e-3, 1, 10}, the gradient split between the
channels at two angles.  de/drho_down and de/dsigma_dd of a point are de/drho_up and de/dsigma_uu of the point with the channels
exchanged, which is on the grid.

This file also holds the double-precision restatement of the forms (``pointwise``: NumPy, derivatives by the complex step) that
the device tests compare against and build their pipeline twin from.  It is written for any NumPy float type, so that the
twin can measure its own rounding against long double.

Error measure and bounds are those of tests/test_xc_reference.py: every error is scaled by the LDA-exchange quantity of the
same total density (e: e_x(rho), v: v_x(rho), v_sigma: e_x(rho) / max(sigma, (2 k_F rho)^2) with sigma = s^2 (2 k_F rho)^2 of the
grid point) and bounded by ``margin * max(E_REF, FLOOR)`` per functional, quantity and decade.  E_REF below is the largest
scaled error of ``pointwise`` in float64 against the fixtures (``python tests/test_xc_spin_gga_reference.py`` prints the
table); nothing in it comes from a kernel.  The decades are dominated by their fully polarised points: phi^3 and the
spin-scaled exchange of a channel at the floor 1e-20 have derivatives that exceed the scale by up to (rho / 1e-20)^(4/3),
with a relative error of a few ulp.  E_REF_INNER is the same measurement over the points with |zeta| <= 0.9 alone; those
points are held to both bounds, so that a fully polarised point cannot excuse an error next to it.

What is here: the restatement against the fixtures; both tables against what the restatement shows now; the two identities
of the generator on the fixtures themselves (zeta = 0 with equal gradients against the existing xc_mp_gga_* fixtures, equal
as doubles; zeta = +-1 against 1/2 e_x0(2 rho, 4 sigma)); every 97th point regenerated (skipped without mpmath).
"""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_golden_xc_spin_gga", os.path.join(ROOT, "tools", "make_golden_xc_spin_gga.py"))
sgold = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sgold)
gold = sgold.gold

import test_xc_reference as R  # noqa: E402

FLOOR = R.FLOOR
MARGIN_TWIN = 4            # the restatement against its own recorded error (another libm may round differently)
MARGIN = 8                 # the kernels (tests/test_gpu_xc_spin_gga.py)
OUTPUTS = ("e", "vup", "vdn", "vsuu", "vsud", "vsdd")
SPIN_FLOOR = 1e-20

# E_REF[(functional, quantity)] = {decade of rho: largest scaled error of ``pointwise`` (float64) against the fixtures},
# rounded up to two digits; decades that are not listed are at or below FLOOR = 8.9e-16.
E_REF = {
    ('gga_x_pbe', 'vsuu'): {
        -18: 2.8e-12, -17: 9.0e-11, -16: 1.3e-09, -15: 2.8e-08, -14: 6.0e-07, -13: 1.3e-05, -12: 2.8e-04, -11: 6.0e-03,
        -10: 1.3e-01, -9: 2.8e+00, -8: 6.0e+01, -7: 1.3e+03, -6: 2.8e+04, -5: 6.0e+05, -4: 1.3e+07, -3: 2.8e+08, -2:
        6.0e+09, -1: 1.3e+11, 0: 2.8e+12, 1: 6.0e+13, 2: 1.3e+15, 3: 6.0e+17},
    ('gga_x_pbe', 'vsdd'): {
        -18: 2.8e-12, -17: 9.0e-11, -16: 1.3e-09, -15: 2.8e-08, -14: 6.0e-07, -13: 1.3e-05, -12: 2.8e-04, -11: 6.0e-03,
        -10: 1.3e-01, -9: 2.8e+00, -8: 6.0e+01, -7: 1.3e+03, -6: 2.8e+04, -5: 6.0e+05, -4: 1.3e+07, -3: 2.8e+08, -2:
        6.0e+09, -1: 1.3e+11, 0: 2.8e+12, 1: 6.0e+13, 2: 1.3e+15, 3: 6.0e+17},
    ('gga_c_pbe', 'vup'): {
        -18: 1.2e-15, -17: 1.8e-15, -16: 6.9e-15, -15: 8.3e-15, -14: 1.6e-14, -13: 8.5e-14, -12: 6.7e-14, -11: 1.3e-13,
        -10: 3.6e-13, -9: 8.4e-13, -8: 3.0e-12, -7: 5.1e-12, -6: 6.6e-12, -5: 9.8e-12, -4: 1.4e-11, -3: 3.3e-11, -2:
        3.5e-11, -1: 4.1e-11, 0: 4.0e-11, 1: 5.5e-11, 2: 1.8e-10, 3: 4.6e-10},
    ('gga_c_pbe', 'vdn'): {
        -18: 1.2e-15, -17: 1.8e-15, -16: 6.9e-15, -15: 8.3e-15, -14: 1.6e-14, -13: 8.5e-14, -12: 6.7e-14, -11: 1.3e-13,
        -10: 3.6e-13, -9: 8.4e-13, -8: 3.0e-12, -7: 5.1e-12, -6: 6.6e-12, -5: 9.8e-12, -4: 1.4e-11, -3: 3.3e-11, -2:
        3.5e-11, -1: 4.1e-11, 0: 4.0e-11, 1: 5.5e-11, 2: 1.8e-10, 3: 4.6e-10},
    ('gga_c_pbe', 'vsuu'): {
        -16: 1.1e-15, -13: 1.4e-15},
    ('gga_c_pbe', 'vsud'): {
        -18: 1.3e-15, -16: 2.1e-15, -15: 1.4e-15, -14: 1.6e-15, -13: 2.7e-15, -12: 1.7e-15, -11: 1.6e-15, -10: 1.4e-15,
        -8: 1.8e-15, -5: 1.3e-15},
    ('gga_c_pbe', 'vsdd'): {
        -16: 1.1e-15, -13: 1.4e-15},
}
# the same over the points with |zeta| <= 0.9 only: a second, tighter bound that the polarised points do not dominate
E_REF_INNER = {
    ('gga_x_pbe', 'vsuu'): {
        -18: 3.5e-15, -17: 2.4e-15, -16: 1.6e-15, -15: 1.1e-15, -14: 1.5e-15, -13: 3.9e-15, -12: 1.3e-15, -11: 1.8e-15,
        -10: 1.2e-15, -9: 3.2e-15, -8: 1.1e-15, -7: 1.5e-15, -6: 2.0e-15, -5: 1.4e-15, -4: 5.3e-15, -3: 1.2e-15, -2:
        1.6e-15, -1: 3.3e-15, 0: 4.4e-15, 1: 2.0e-15, 3: 3.6e-15},
    ('gga_x_pbe', 'vsdd'): {
        -18: 3.5e-15, -17: 2.4e-15, -16: 1.6e-15, -15: 1.1e-15, -14: 1.5e-15, -13: 3.9e-15, -12: 1.3e-15, -11: 1.8e-15,
        -10: 1.2e-15, -9: 3.2e-15, -8: 1.1e-15, -7: 1.5e-15, -6: 2.0e-15, -5: 1.4e-15, -4: 5.3e-15, -3: 1.2e-15, -2:
        1.6e-15, -1: 3.3e-15, 0: 4.4e-15, 1: 2.0e-15, 3: 3.6e-15},
    ('gga_c_pbe', 'vup'): {
        -16: 1.3e-15, -11: 2.1e-15, -10: 1.0e-15, -7: 9.5e-16, -6: 1.2e-15},
    ('gga_c_pbe', 'vdn'): {
        -16: 1.3e-15, -11: 2.1e-15, -10: 1.0e-15, -7: 9.5e-16, -6: 1.2e-15},
    ('gga_c_pbe', 'vsuu'): {
        -16: 1.1e-15, -13: 1.4e-15},
    ('gga_c_pbe', 'vsud'): {
        -18: 1.3e-15, -16: 2.1e-15, -15: 1.4e-15, -14: 1.6e-15, -13: 2.7e-15, -12: 1.7e-15, -11: 1.6e-15, -10: 1.4e-15,
        -8: 1.8e-15, -5: 1.3e-15},
    ('gga_c_pbe', 'vsdd'): {
        -16: 1.1e-15, -13: 1.4e-15},
}


# ------------------------------------------------------------------------------------------------ the forms (NumPy)
# The elementary functions of a complex-step argument x + i h: the real libm function of x, and h times its derivative.
# (NumPy's own complex log1p takes log|1 + z| for the real part and a complex power has no cbrt: at rs = 1e6 both lose the
# digits that the real functions keep.  h is 1e-20 of x, so the terms of order h^2 that this drops are below 1e-40.)
def _lift(x, f, df):
    return f + 1j * (x.imag * df) if np.iscomplexobj(x) else f


def _cbrt(x):
    r = np.cbrt(x.real)
    return _lift(x, r, r / (3.0 * x.real))


def _sqrt(x):
    r = np.sqrt(x.real)
    return _lift(x, r, 0.5 / r)


def _log1p(x):
    return _lift(x, np.log1p(x.real), 1.0 / (1.0 + x.real))


def _expm1(x):
    e = np.expm1(x.real)
    return _lift(x, e, e + 1.0)


def _e_x0(rho, sigma):
    """unpolarised gga_x_pbe"""
    kappa, mu, cx = 0.8040, 0.2195149727645171, -0.73855876638202240588
    kf = _cbrt(3.0 * math.pi ** 2 * rho)
    s2 = sigma / (4.0 * (kf * kf * rho * rho))
    return cx * (rho * _cbrt(rho)) * ((1.0 + kappa) - kappa * kappa / (kappa + mu * s2))


def _e_x_channel(r, s):
    """one channel of the spin-scaling relation: 1/2 e_x0(2 rho_s, 4 sigma_ss)"""
    return 0.5 * _e_x0(2.0 * r, 4.0 * s)


def _pw92(rs, sq, A, a1, b1, b2, b3, b4):
    den = 2.0 * A * (b1 * sq + b2 * rs + b3 * (rs * sq) + b4 * (rs * rs))
    return -2.0 * A * (1.0 + a1 * rs) * _log1p(1.0 / den)


def _e_c(ra, rb, st):
    """polarised gga_c_pbe as a function of the two densities and sigma_tot"""
    beta, gamma = 0.06672455060314922, 0.031090690869654895
    rt = ra + rb
    xa, xb = 2.0 * (ra / rt), 2.0 * (rb / rt)
    ca, cb = _cbrt(xa), _cbrt(xb)
    fz = (xa * ca + xb * cb - 2.0) / (2.5198420997897464 - 2.0)
    phi = 0.5 * (ca * ca + cb * cb)
    z = (ra - rb) / rt
    z4 = (z * z) * (z * z)
    rs = _cbrt((3.0 / (4.0 * math.pi)) / rt)
    sq = _sqrt(rs)
    e0 = _pw92(rs, sq, 0.0310907, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294)
    e1 = _pw92(rs, sq, 0.01554535, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517)
    mac = _pw92(rs, sq, 0.0168869, 0.11125, 10.357, 3.6231, 0.88026, 0.49671)
    eps = e0 - mac * fz * (1.0 - z4) / 1.709920934161365617563962776245 + (e1 - e0) * (fz * z4)
    phi3 = phi * phi * phi
    kf = _cbrt(3.0 * math.pi ** 2 * rt)
    t2 = (math.pi / 16.0) * (st / (phi * phi * (kf * rt * rt)))
    A = (beta / gamma) / _expm1(-eps / (gamma * phi3))
    f1 = t2 + A * (t2 * t2)
    return rt * (eps + gamma * phi3 * _log1p((beta / gamma) * (f1 / (1.0 + A * f1))))


def _complex_step(f, args, k, scale):
    """d f / d args[k] by the complex step (relative step 1e-20: the truncation error is 1e-40 of the value)"""
    ctype = np.result_type(args[0].dtype, np.complex64)
    h = 1e-20 * scale
    z = [a.astype(ctype) for a in args]
    z[k] = z[k] + 1j * h
    return f(*z).imag / h


def pointwise(names, up, dn, suu, sud, sdd, threshold=0.0):
    """e and its five derivatives for the functionals ``names`` in the float type of the arguments, with the floors of
    ``dftk_mi_xc_gga_spin``: channels at max(rho_s, 1e-20), derivatives with respect to the clamped variables, zeros where
    rho_up + rho_down <= max(threshold, 2e-20), sigma_uu, sigma_dd, sigma_tot at max(., 0)."""
    ft = up.dtype.type
    alive = up + dn > max(threshold, 2 * SPIN_FLOOR)
    ra, rb = np.maximum(up, ft(SPIN_FLOOR)), np.maximum(dn, ft(SPIN_FLOOR))
    puu, pdd = np.maximum(suu, 0), np.maximum(sdd, 0)
    st = np.maximum((suu + sdd) + 2 * sud, 0)
    unit = gold.sigma_unit(ra + rb).astype(up.dtype)       # the step of a sigma derivative: 1e-20 of max(sigma, (2 k_F rho)^2)
    out = {q: np.zeros_like(up) for q in OUTPUTS}
    with np.errstate(all="ignore"):
        if "gga_x_pbe" in names:
            for r, s, qv, qs in ((ra, puu, "vup", "vsuu"), (rb, pdd, "vdn", "vsdd")):
                out["e"] += _e_x_channel(r, s)
                out[qv] += _complex_step(_e_x_channel, (r, s), 0, r)
                out[qs] += _complex_step(_e_x_channel, (r, s), 1, np.maximum(s, gold.sigma_unit(r).astype(up.dtype)))
        if "gga_c_pbe" in names:
            out["e"] += _e_c(ra, rb, st)
            out["vup"] += _complex_step(_e_c, (ra, rb, st), 0, ra)
            out["vdn"] += _complex_step(_e_c, (ra, rb, st), 1, rb)
            w = _complex_step(_e_c, (ra, rb, st), 2, np.maximum(st, unit))
            out["vsuu"] += w
            out["vsud"] += 2 * w
            out["vsdd"] += w
    return {q: np.where(alive, v, 0) for q, v in out.items()}


# ------------------------------------------------------------------------------------------------ fixtures as arrays
class Family:
    pass


def load_spingga():
    F = Family()
    F.ref = {}
    for fun in sgold.FUNCTIONALS:
        F.ref[fun] = {}
        for q in sgold.QUANTITIES:
            fx = sgold.load_fixture(fun, q)
            F.grid = fx["grid"]
            F.ref[fun][q] = np.array(fx["values"][q])
    F.mirror = sgold.mirror_index(F.grid)
    for fun in sgold.FUNCTIONALS:                     # exchanging the channels: zeta -> -zeta is on the grid
        F.ref[fun]["vdn"] = F.ref[fun]["vup"][F.mirror]
        F.ref[fun]["vsdd"] = F.ref[fun]["vsuu"][F.mirror]
    F.ref["gga_xc_pbe"] = {q: F.ref["gga_x_pbe"][q] + F.ref["gga_c_pbe"][q] for q in OUTPUTS}
    for k, v in sgold.spin_gga_grid(F.grid).items():
        setattr(F, k, v)
    F.sigma = (F.s * F.s) * gold.sigma_unit(F.rho)
    return F


@pytest.fixture(scope="module")
def sg():
    return load_spingga()


def scale_of(quantity, F):
    return R.scale_of("vsigma" if quantity.startswith("vs") else ("e" if quantity == "e" else "v"), F.rho, F.sigma)


def bound_of(key, dec, margin, inner=False):
    table = (E_REF_INNER if inner else E_REF).get(key, {})
    return margin * np.array([max(table.get(int(d), 0.0), FLOOR) for d in dec])


def inner_points(F):
    """the points of E_REF_INNER: |zeta| <= 0.9"""
    return np.abs(F.zeta) <= 0.9


def twin_all(F):
    """{(functional, quantity): (values, reference, scale, decade)} of the float64 restatement on the grid"""
    out = {}
    for fun in sgold.FUNCTIONALS:
        val = pointwise((fun,), F.up, F.dn, F.suu, F.sud, F.sdd)
        for q in OUTPUTS:
            out[(fun, q)] = (val[q], F.ref[fun][q], scale_of(q, F), F.dec)
    return out


# ------------------------------------------------------------------------------------------------ tests
def test_restatement_against_the_fixtures(sg):
    """``pointwise`` in double precision within 4 x max(E_REF, FLOOR) of the 60-digit values: every functional, quantity and
    grid point."""
    sel = inner_points(sg)
    for key, (val, ref, scale, dec) in twin_all(sg).items():
        assert np.all(np.isfinite(val)), key
        err = R.scaled_error(val, ref, scale)
        for inner in (False, True):
            ok = np.abs(val - ref) <= bound_of(key, dec, MARGIN_TWIN, inner) * scale
            bad = np.flatnonzero(~ok & (sel | (not inner)))
            assert bad.size == 0, (key, inner, bad.size, float(err[bad].max()), int(bad[np.argmax(err[bad])]))


def test_e_ref_table_is_the_restatements_error(sg):
    """No listed entry is more than four times what the restatement shows now (a table inflated to let a kernel pass would
    fail here)."""
    sel = inner_points(sg)
    assert E_REF and E_REF_INNER, "a table is empty"
    for tables, pts in ((E_REF, np.ones_like(sel)), (E_REF_INNER, sel)):
        measured = {key: R.decade_maxima(R.scaled_error(val, ref, scale)[pts], dec[pts])
                    for key, (val, ref, scale, dec) in twin_all(sg).items()}
        for key, table in tables.items():
            for d, listed in table.items():
                assert listed > FLOOR, (key, d)
                assert listed <= 4 * max(measured[key][d], FLOOR), (key, d, listed, measured[key][d])


def test_unpolarised_limit_is_the_unpolarised_fixture(sg):
    """zeta = 0 with grad rho_up = grad rho_down: the polarised forms are gga_x_pbe / gga_c_pbe of the existing fixtures at
    (rho, sigma) -- e and de/drho_up = de/drho; correlation: de/dsigma_uu = de/dsigma, de/dsigma_ud = 2 de/dsigma; exchange:
    de/dsigma_uu = 2 de/dsigma (the spin-scaling relation), de/dsigma_ud = 0.  Equal as doubles."""
    gga = R.load_gga()
    sel = np.flatnonzero((sg.zeta == 0.0) & (sg.cos == 1.0))
    assert len(sel) == len(np.unique(sg.rho)) * len(sg.grid["s"])
    where = {(r, s): i for i, (r, s) in enumerate(zip(gga.rho, gga.sigma))}
    idx = np.array([where[(r, s)] for r, s in zip(sg.rho[sel], sg.sigma[sel])])
    assert np.array_equal(sg.suu[sel] + 2 * sg.sud[sel] + sg.sdd[sel], gga.sigma[idx])
    for fun, k_uu, k_ud in (("gga_x_pbe", 2.0, 0.0), ("gga_c_pbe", 1.0, 2.0)):
        assert np.array_equal(sg.ref[fun]["e"][sel], gga.ref[fun]["e"][idx]), fun
        assert np.array_equal(sg.ref[fun]["vup"][sel], gga.ref[fun]["vrho"][idx]), fun
        assert np.array_equal(sg.ref[fun]["vdn"][sel], gga.ref[fun]["vrho"][idx]), fun
        assert np.array_equal(sg.ref[fun]["vsuu"][sel], k_uu * gga.ref[fun]["vsigma"][idx]), fun
        assert np.array_equal(sg.ref[fun]["vsud"][sel], k_ud * gga.ref[fun]["vsigma"][idx]), fun
    assert np.all(sg.ref["gga_x_pbe"]["vsud"] == 0.0)


def test_full_polarisation_is_the_scaled_unpolarised_exchange(sg):
    """zeta = +-1: e_x = 1/2 e_x0(2 rho, 4 sigma) of the filled channel plus the floor term 1/2 e_x0(2e-20, 0) of the empty one.
    2 rho is not on the grid of the unpolarised fixtures, so e_x0 is evaluated here: in mpmath by the existing tool's form
    (equal as doubles), and the two signs of zeta give the same bits."""
    mpmath = pytest.importorskip("mpmath")
    mp = gold._mp()
    up1 = np.flatnonzero(sg.zeta == 1.0)
    dn1 = np.flatnonzero(sg.zeta == -1.0)
    e = sg.ref["gga_x_pbe"]["e"]
    assert len(up1) and np.array_equal(e[up1], e[dn1]) and np.array_equal(sg.mirror[up1], dn1)
    for i in up1[::5]:
        want = gold.e_gga_x_pbe(mp, 2 * mp.mpf(float(sg.up[i])), 4 * mp.mpf(float(sg.suu[i]))) / 2 + \
            gold.e_gga_x_pbe(mp, 2 * mp.mpf(SPIN_FLOOR), mp.mpf(0)) / 2
        assert e[i] == float(want), i
    assert mpmath is not None


def test_fixtures_match_the_generator(sg):
    pytest.importorskip("mpmath")
    pts = list(range(0, len(sg.rho), 97))
    for fun in sgold.FUNCTIONALS:
        for i in pts:
            got = sgold.ref_spin_gga(fun, *(float(getattr(sg, k)[i]) for k in ("up", "dn", "suu", "sud", "sdd")))
            assert all(got[q] == sg.ref[fun][q][i] for q in OUTPUTS), (fun, i)


def test_fixture_files_are_small():
    names = [n for n in os.listdir(gold.GOLDEN) if n.startswith("xc_spingga_mp_")]
    assert len(names) == len(sgold.FUNCTIONALS) * len(sgold.QUANTITIES)
    assert all(os.path.getsize(os.path.join(gold.GOLDEN, n)) <= sgold.MAX_BYTES for n in names)


# ------------------------------------------------------------------------------------------------ measuring E_REF
def measure_e_ref(inner):
    table = {}
    F = load_spingga()
    pts = inner_points(F) if inner else np.ones(len(F.rho), dtype=bool)
    for key, (val, ref, scale, dec) in twin_all(F).items():
        rows = {}
        for d, err in R.decade_maxima(R.scaled_error(val, ref, scale)[pts], dec[pts]).items():
            if err > FLOOR:
                mag = 10.0 ** (math.floor(math.log10(err)) - 1)
                rows[d] = float(f"{math.ceil(err / mag) * mag:.1e}")
        if rows:
            table[key] = rows
    return table


if __name__ == "__main__":
    import textwrap
    for name, inner in (("E_REF", False), ("E_REF_INNER", True)):
        print(name + " = {")
        for key, rows in measure_e_ref(inner).items():
            body = ", ".join(f"{d}: {v:.1e}" for d, v in rows.items())
            print(f"    {key!r}: {{")
            print(textwrap.fill(body, 120, initial_indent=" " * 8, subsequent_indent=" " * 8) + "},")
        print("}")
    sys.exit(0)
