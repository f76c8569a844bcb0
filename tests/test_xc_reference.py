"""The point-wise exchange-correlation forms against a 60-digit reference over the whole density range (host side).

tests/golden/xc_mp_*.json hold e, v, f_xc, v_sigma, v_up, v_down of every functional the library evaluates, computed by
tools/make_golden_xc.py in mpmath from the energy densities alone (every derivative is ``mpmath.diff``), on log grids
from the vacuum decades (1e-30) to 1e5, reduced gradients s from 0 to 100 and polarisations up to zeta = +-1.  The three
implementations of these forms (the kernels, the torch twins of dftk_jl_amd/terms.py, oracle/terms.py) were typed from the
same derivations; the fixtures were not.

Error measure (absolute and plain relative tolerances are both wrong across 35 decades: the VWN form cancels as rs grows):
every error is scaled by the LDA-exchange quantity of the same total density,
    e: |de| / |e_x(rho)|      v, v_up, v_down, v_rho: |dv| / |v_x(rho)|      f_xc: |df| / |f_x(rho)|
    v_sigma: |dv_sigma| max(sigma, (2 k_F rho)^2) / |e_x(rho)|
and asserted as |d| <= bound * scale, so that a scale that underflows (e_x(1e-300) = 0) asks for an exact result.

Bounds: per functional, quantity and decade of rho, ``margin * max(E_REF, FLOOR)``.  E_REF is the largest scaled error in
that decade of the double-precision NumPy forms of oracle/terms.py against the fixtures, measured on the CPU
(``python tests/test_xc_reference.py`` prints the table) and listed below where it exceeds FLOOR = 4 * 2^-52.  Nothing in
it comes from a kernel.  The oracle itself is held to margin 4 of its own recorded error (another libm may round
differently); the torch twins and the kernels (tests/test_gpu_xc_pointwise.py) to margin 8: the device's cbrt, log1p, expm1
and atan are specified to a couple of ulp against under 1 ulp for the host's, and dual numbers or autograd order the
operations differently under the same condition number.  The margin is a judgement, not a derivation.

What is here:
* the oracle forms, including the new ``lda_fxc``, against the fixtures.  On the parent commit this failed in two regimes:
  the GGA de/dsigma for rho < 1e-8 (a complex step of 1e-30 is not small against sigma ~ 4e-31 at rho = 1e-12) and the
  collinear PW92 for rho_t < 1e-6 (log(1 + x) for log1p(x)).
* the torch twins (``_lda_x``, ``_lda_c_vwn``, ``_lda_c_pw`` and the PBE energy densities under autograd) on CPU tensors:
  they need no library.  The package has no twin of lda_xc_teter93 or of the collinear forms.
* fixtures against generator: every 7th point regenerated and compared for equality (skipped without mpmath).
* the reference against itself: e_spin(rho/2, rho/2) = e_unpol(rho), v_up = v at zeta = 0, PBE at s = 0 is
  lda_x + PW92mod with a finite v_sigma.
No grid point is skipped, masked or filtered anywhere.
"""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location("make_golden_xc", os.path.join(ROOT, "tools", "make_golden_xc.py"))
gold = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gold)

from oracle import terms as oterms  # noqa: E402

FLOOR = 4 * 2.0 ** -52
MARGIN_ORACLE = 4
MARGIN = 8                       # torch twins and kernels
GGA_ALL = ("gga_x_pbe", "gga_c_pbe", "gga_xc_pbe")     # the last one: both bits together, reference = sum of the two
CX = -0.75 * (3 / math.pi) ** (1 / 3)

# E_REF[(family, functional, quantity)] = {decade of rho: largest scaled error of oracle/terms.py against the fixtures},
# rounded up to two digits; decades that are not listed are at or below FLOOR = 8.9e-16.  Decade -300 is the single point
# 1e-300 (1 + 2^-52) next to the rho > 1e-300 guard.
E_REF = {
    ('lda', 'lda_c_vwn', 'e'): {
        -30: 6.2e-08, -29: 3.7e-08, -28: 2.9e-09, -27: 5.2e-09, -26: 1.2e-09, -25: 6.3e-10, -24: 1.7e-10, -23: 1.6e-10,
        -22: 3.3e-11, -21: 4.8e-11, -20: 2.9e-11, -19: 5.2e-12, -18: 8.2e-12, -17: 1.5e-12, -16: 1.1e-12, -15: 3.2e-13,
        -14: 7.8e-14, -13: 3.7e-14, -12: 1.9e-14, -11: 1.3e-14, -10: 8.6e-15, -9: 2.9e-15, -8: 2.4e-15},
    ('lda', 'lda_c_vwn', 'v'): {
        -300: 2.1e+82, -30: 5.4e-08, -29: 3.6e-08, -28: 1.8e-09, -27: 4.4e-09, -26: 4.2e-10, -25: 8.6e-10, -24: 1.8e-10,
        -23: 1.9e-10, -22: 3.9e-11, -21: 5.2e-11, -20: 3.0e-11, -19: 5.9e-12, -18: 8.0e-12, -17: 1.5e-12, -16: 9.7e-13,
        -15: 2.2e-13, -14: 5.9e-14, -13: 5.8e-14, -12: 2.1e-14, -11: 1.7e-14, -10: 1.0e-14, -9: 3.0e-15, -8: 2.5e-15},
    ('lda', 'lda_c_vwn', 'f'): {
        -300: 2.8e+82, -30: 3.2e-08, -29: 2.4e-08, -28: 9.0e-09, -27: 8.1e-09, -26: 1.2e-09, -25: 1.4e-09, -24: 5.1e-10,
        -23: 2.9e-10, -22: 1.1e-10, -21: 1.4e-11, -20: 2.1e-11, -19: 7.2e-12, -18: 6.0e-12, -17: 2.2e-12, -16: 8.5e-13,
        -15: 8.3e-14, -14: 2.2e-13, -13: 2.0e-13, -12: 5.8e-14, -11: 2.8e-14, -10: 1.5e-14, -9: 7.1e-15, -8: 2.1e-15},
    ('lda', 'lda_c_pw', 'f'): {
        -28: 1.1e-15, -26: 9.0e-16, -25: 1.2e-15, -24: 1.2e-15, -22: 1.4e-15, -21: 1.3e-15, -20: 1.3e-15, -11: 9.4e-16,
        -7: 9.6e-16},
    ('lda', 'lda_xc_teter93', 'e'): {
        -19: 1.1e-15, -15: 1.2e-15, -13: 9.0e-16},
    ('lda', 'lda_xc_teter93', 'v'): {
        -20: 9.5e-16, -19: 1.4e-15, -16: 1.1e-15, -15: 1.7e-15, -14: 1.1e-15, -13: 1.5e-15, -10: 1.3e-15, -7: 1.2e-15,
        -6: 1.5e-15},
    ('gga', 'gga_x_pbe', 'e'): {
        -28: 8.7e-15, -27: 8.4e-15, -26: 8.1e-15, -25: 7.8e-15, -24: 7.5e-15, -23: 7.1e-15, -22: 6.8e-15, -21: 6.5e-15,
        -20: 6.2e-15, -19: 5.7e-15, -18: 5.8e-15, -17: 5.6e-15, -16: 5.0e-15, -15: 4.5e-15, -14: 4.5e-15, -13: 4.1e-15,
        -12: 4.1e-15, -11: 3.4e-15, -10: 3.1e-15, -9: 2.8e-15, -8: 2.7e-15, -7: 2.3e-15, -6: 1.9e-15, -5: 1.7e-15, -4:
        1.2e-15, -3: 1.2e-15, 2: 1.2e-15, 3: 1.3e-15},
    ('gga', 'gga_x_pbe', 'vrho'): {
        -28: 1.4e-14, -27: 8.0e-15, -26: 1.5e-14, -25: 2.2e-14, -24: 1.5e-14, -23: 2.3e-14, -22: 1.7e-14, -21: 2.2e-14,
        -20: 8.2e-15, -19: 1.3e-14, -18: 7.1e-15, -17: 1.3e-14, -16: 1.7e-14, -15: 1.2e-14, -14: 8.3e-15, -13: 2.5e-15,
        -12: 8.7e-15, -11: 1.3e-14, -10: 3.6e-15, -9: 4.3e-15, -8: 7.8e-15, -7: 5.6e-15, -6: 3.2e-15, -4: 4.0e-15, -3:
        1.6e-15, -2: 2.1e-15, -1: 1.3e-15, 1: 1.1e-15, 2: 2.9e-15, 3: 2.1e-15},
    ('gga', 'gga_x_pbe', 'vsigma'): {
        -28: 1.6e-15, -27: 1.3e-15, -26: 1.7e-15, -25: 2.2e-15, -24: 1.7e-15, -23: 2.4e-15, -22: 1.8e-15, -21: 2.2e-15,
        -20: 1.5e-15, -19: 1.6e-15, -18: 1.4e-15, -17: 1.6e-15, -16: 1.8e-15, -15: 1.4e-15, -14: 1.2e-15, -12: 1.3e-15,
        -11: 1.5e-15},
    ('gga', 'gga_c_pbe', 'e'): {
        -28: 1.7e-15, -27: 1.5e-15, -26: 1.4e-15, -25: 1.6e-15, -24: 1.3e-15, -23: 1.2e-15, -22: 1.3e-15, -21: 1.3e-15,
        -20: 1.2e-15, -19: 9.2e-16, -18: 1.2e-15, -17: 1.1e-15, -14: 9.0e-16},
    ('gga', 'gga_c_pbe', 'vrho'): {
        -28: 3.4e-15, -27: 2.8e-15, -26: 2.2e-15, -25: 4.2e-15, -24: 2.2e-15, -23: 4.2e-15, -22: 5.4e-15, -21: 1.5e-15,
        -20: 1.4e-15, -19: 2.0e-15, -18: 9.7e-16, -17: 2.4e-15, -16: 3.0e-15, -15: 1.6e-15, -14: 2.2e-15, -12: 1.7e-15,
        -11: 1.6e-15, -10: 1.1e-15, -8: 1.2e-15},
    ('gga', 'gga_c_pbe', 'vsigma'): {
        -28: 1.1e-15, -27: 9.5e-16, -26: 9.9e-16, -25: 1.5e-15, -23: 1.5e-15, -22: 1.8e-15, -17: 9.5e-16, -16: 1.2e-15},
    ('gga', 'gga_xc_pbe', 'e'): {
        -28: 9.0e-15, -27: 8.4e-15, -26: 8.1e-15, -25: 7.9e-15, -24: 7.6e-15, -23: 7.3e-15, -22: 7.1e-15, -21: 6.5e-15,
        -20: 6.2e-15, -19: 5.7e-15, -18: 5.5e-15, -17: 5.6e-15, -16: 5.3e-15, -15: 4.5e-15, -14: 4.3e-15, -13: 4.2e-15,
        -12: 3.8e-15, -11: 3.4e-15, -10: 3.1e-15, -9: 2.8e-15, -8: 2.7e-15, -7: 2.4e-15, -6: 1.9e-15, -5: 1.7e-15, -4:
        1.2e-15, -3: 1.2e-15, 2: 1.2e-15, 3: 1.3e-15},
    ('gga', 'gga_xc_pbe', 'vrho'): {
        -28: 1.4e-14, -27: 8.6e-15, -26: 1.4e-14, -25: 2.2e-14, -24: 1.5e-14, -23: 2.4e-14, -22: 1.7e-14, -21: 2.3e-14,
        -20: 8.2e-15, -19: 1.3e-14, -18: 6.8e-15, -17: 1.3e-14, -16: 1.7e-14, -15: 1.3e-14, -14: 8.3e-15, -13: 2.7e-15,
        -12: 9.0e-15, -11: 1.2e-14, -10: 3.6e-15, -9: 4.5e-15, -8: 7.4e-15, -7: 5.7e-15, -6: 3.2e-15, -4: 4.3e-15, -3:
        1.7e-15, -2: 2.1e-15, -1: 1.3e-15, 0: 9.2e-16, 1: 1.1e-15, 2: 2.9e-15, 3: 2.1e-15},
    ('gga', 'gga_xc_pbe', 'vsigma'): {
        -28: 1.7e-15, -27: 1.1e-15, -26: 1.8e-15, -25: 2.5e-15, -24: 1.8e-15, -23: 2.6e-15, -22: 2.0e-15, -21: 2.4e-15,
        -20: 1.3e-15, -19: 1.7e-15, -18: 1.1e-15, -17: 1.6e-15, -16: 2.0e-15, -15: 1.5e-15, -14: 1.1e-15, -12: 1.2e-15,
        -11: 1.5e-15, -8: 9.5e-16},
    ('spin', 'lda_x', 'e'): {
        -18: 8.5e-15, -17: 9.0e-15, -16: 1.2e-14, -15: 1.1e-14, -14: 7.8e-15, -13: 6.1e-15, -12: 6.0e-15, -11: 8.7e-15,
        -10: 3.7e-15, -9: 3.6e-15, -8: 5.4e-15, -7: 5.3e-15, -6: 4.2e-15, -5: 2.5e-15, -4: 2.8e-15, -3: 1.7e-15, -2:
        1.7e-15, 1: 9.0e-16, 2: 2.2e-15, 3: 2.4e-15},
    ('spin', 'lda_x', 'vup'): {
        -18: 9.1e-15, -17: 9.2e-15, -16: 1.2e-14, -15: 1.2e-14, -14: 7.6e-15, -13: 6.9e-15, -12: 6.8e-15, -11: 8.9e-15,
        -10: 4.2e-15, -9: 4.5e-15, -8: 5.4e-15, -7: 5.6e-15, -6: 4.1e-15, -5: 2.3e-15, -4: 2.9e-15, -3: 1.9e-15, -2:
        1.6e-15, 1: 1.1e-15, 2: 2.0e-15, 3: 2.5e-15},
    ('spin', 'lda_x', 'vdn'): {
        -18: 9.1e-15, -17: 9.2e-15, -16: 1.2e-14, -15: 1.2e-14, -14: 7.6e-15, -13: 6.9e-15, -12: 6.8e-15, -11: 8.9e-15,
        -10: 4.2e-15, -9: 4.5e-15, -8: 5.4e-15, -7: 5.6e-15, -6: 4.1e-15, -5: 2.3e-15, -4: 2.9e-15, -3: 1.9e-15, -2:
        1.6e-15, 1: 1.1e-15, 2: 2.0e-15, 3: 2.5e-15},
    ('spin', 'lda_c_pw', 'e'): {
        -18: 1.2e-15, -17: 1.6e-15, -16: 1.0e-15, -14: 1.3e-15, -13: 9.0e-16, -12: 1.2e-15, -11: 1.1e-15},
    ('spin', 'lda_c_pw', 'vup'): {
        -18: 3.1e-15, -17: 5.6e-15, -16: 6.9e-15, -15: 4.7e-15, -14: 4.5e-15, -13: 4.7e-15, -12: 5.6e-15, -11: 2.6e-15,
        -10: 4.9e-15, -9: 2.6e-15, -8: 3.4e-15, -7: 2.6e-15, -6: 2.6e-15, -5: 1.5e-15, -3: 1.2e-15},
    ('spin', 'lda_c_pw', 'vdn'): {
        -18: 3.1e-15, -17: 5.6e-15, -16: 6.9e-15, -15: 4.7e-15, -14: 4.5e-15, -13: 4.7e-15, -12: 5.6e-15, -11: 2.6e-15,
        -10: 4.9e-15, -9: 2.6e-15, -8: 3.4e-15, -7: 2.6e-15, -6: 2.6e-15, -5: 1.5e-15, -3: 1.2e-15},
    ('spin', 'lda_xc_teter93', 'e'): {
        -18: 3.9e-15, -17: 3.2e-15, -16: 2.8e-15, -15: 1.9e-15, -14: 2.2e-15, -13: 2.3e-15, -12: 2.4e-15, -11: 2.3e-15,
        -10: 1.5e-15, -9: 1.6e-15, -8: 1.4e-15, -7: 1.3e-15, -6: 1.8e-15},
    ('spin', 'lda_xc_teter93', 'vup'): {
        -18: 3.2e-15, -17: 4.0e-15, -16: 5.2e-15, -15: 3.7e-15, -14: 2.9e-15, -13: 3.6e-15, -12: 3.1e-15, -11: 2.4e-15,
        -10: 1.9e-15, -9: 2.3e-15, -8: 2.9e-15, -7: 1.5e-15, -6: 2.3e-15, -5: 1.2e-15},
    ('spin', 'lda_xc_teter93', 'vdn'): {
        -18: 3.2e-15, -17: 4.0e-15, -16: 5.2e-15, -15: 3.7e-15, -14: 2.9e-15, -13: 3.6e-15, -12: 3.1e-15, -11: 2.4e-15,
        -10: 1.9e-15, -9: 2.3e-15, -8: 2.9e-15, -7: 1.5e-15, -6: 2.3e-15, -5: 1.2e-15},
}


def e_x(rho):
    return np.abs(CX * rho * np.cbrt(rho))


def v_x(rho):
    return np.abs(4 / 3 * CX * np.cbrt(rho))


def f_x(rho):
    return np.abs(4 / 9 * CX / np.cbrt(rho) ** 2)


def scale_of(quantity, rho, sigma=None):
    """the scale of one quantity at total density rho (arrays)"""
    if quantity == "e":
        return e_x(rho)
    if quantity == "f":
        return f_x(rho)
    if quantity == "vsigma":
        return e_x(rho) / np.maximum(sigma, gold.sigma_unit(rho))
    return v_x(rho)


def bound_of(key, dec, margin):
    """margin * max(E_REF, FLOOR) per point, from the decade of each point"""
    table = E_REF.get(key, {})
    return margin * np.array([max(table.get(int(d), 0.0), FLOOR) for d in dec])


def scaled_error(got, ref, scale):
    """|got - ref| / scale; 0 where both agree exactly, inf where the scale has underflowed and they do not"""
    d = np.abs(np.asarray(got) - np.asarray(ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0.0, 0.0, np.where(scale > 0, d / scale, np.inf))


def decade_maxima(err, dec):
    return {int(d): float(err[dec == d].max()) for d in np.unique(dec)}


def check(key, got, ref, scale, dec, margin, label=""):
    """assert |got - ref| <= margin * max(E_REF, FLOOR) * scale at every point; returns the per-decade maxima"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), (label, key)
    err = scaled_error(got, ref, scale)
    bound = bound_of(key, dec, margin)
    bad = np.flatnonzero(~(np.abs(got - ref) <= bound * scale))
    assert bad.size == 0, (f"{label} {key}: {bad.size} points above margin {margin}; worst scaled error "
                           f"{err[bad].max():.3e} against {bound[bad][np.argmax(err[bad])]:.3e} at index "
                           f"{bad[np.argmax(err[bad])]}")
    return decade_maxima(err, dec)


# ------------------------------------------------------------------------------------------------ fixtures as arrays
class Family:
    pass


def load_lda():
    F = Family()
    F.ref = {}
    for fun, quantities in gold.LDA_FUNCTIONALS.items():
        fx = gold.load_fixture("lda", fun)
        F.grid = fx["grid"]
        F.ref[fun] = {q: np.array(fx["values"][q]) for q in quantities}
    F.rho, F.dec = gold.rho_grid(F.grid)
    return F


def load_gga():
    F = Family()
    F.ref = {}
    for fun in gold.GGA_FUNCTIONALS:
        F.ref[fun] = {}
        for q in ("e", "vrho", "vsigma"):
            fx = gold.load_fixture("gga", fun, q)
            F.grid = fx["grid"]
            F.ref[fun][q] = np.array(fx["values"][q])
    # both bits together: the sum of the two stored references (one more rounding, 2^-53 of the larger part)
    F.ref["gga_xc_pbe"] = {q: F.ref["gga_x_pbe"][q] + F.ref["gga_c_pbe"][q] for q in ("e", "vrho", "vsigma")}
    F.rho, F.sigma, F.dec = gold.gga_grid(F.grid)
    return F


def load_spin():
    F = Family()
    F.ref = {}
    for fun in gold.SPIN_FUNCTIONALS:
        F.ref[fun] = {}
        for q in gold.SPIN_QUANTITIES:
            fx = gold.load_fixture("spin", fun, q)
            F.grid = fx["grid"]
            F.ref[fun][q] = np.array(fx["values"][q])
    # v_down(rho_t, zeta) = v_up(rho_t, -zeta): the zeta list holds both signs (the generator check below recomputes v_down)
    zeta = F.grid["zeta"]
    mirror = [zeta.index(-z) for z in zeta]
    even, n_even = gold.spin_even_index(F.grid)          # e is stored for zeta >= 0 only
    for fun in gold.SPIN_FUNCTIONALS:
        F.ref[fun]["e"] = F.ref[fun]["e"].reshape(-1, n_even)[:, even].ravel()
        F.ref[fun]["vdn"] = F.ref[fun]["vup"].reshape(-1, len(zeta))[:, mirror].ravel()
    F.up, F.dn, F.rho, F.dec = gold.spin_grid(F.grid)
    return F


@pytest.fixture(scope="module")
def lda():
    return load_lda()


@pytest.fixture(scope="module")
def gga():
    return load_gga()


@pytest.fixture(scope="module")
def spin():
    return load_spin()


# ------------------------------------------------------------------------------------------------ the oracle's forms
def oracle_lda(fun, rho):
    e, v = oterms._FUNCTIONALS[fun](rho)
    out = {"e": e, "v": v}
    if "f" in gold.LDA_FUNCTIONALS[fun]:
        out["f"] = oterms.lda_fxc(fun, rho)
    return out


def oracle_gga(fun, rho, sigma):
    names = ("gga_x_pbe", "gga_c_pbe") if fun == "gga_xc_pbe" else (fun,)
    parts = [oterms._gga_terms(oterms._GGA_FUNCTIONALS[n], rho, sigma) for n in names]
    return dict(zip(("e", "vrho", "vsigma"), (sum(p[i] for p in parts) for i in range(3))))


class _SpinModel:
    def __init__(self, fun):
        self.functionals = (fun,)


class _SpinBasis:
    dvol = 1.0

    def __init__(self, fun):
        self.model = _SpinModel(fun)


def oracle_spin(fun, up, dn):
    """e per point by the functional's energy density with the clamp, v by ``xc_energy_potential_spin`` itself"""
    _, v = oterms.xc_energy_potential_spin(_SpinBasis(fun), np.stack([up, dn]))
    e = oterms._SPIN_FUNCTIONALS[fun](np.maximum(up, oterms._SPIN_FLOOR), np.maximum(dn, oterms._SPIN_FLOOR))
    return {"e": np.where(up + dn <= 2 * oterms._SPIN_FLOOR, 0.0, e), "vup": v[0], "vdn": v[1]}


def oracle_all(lda, gga, spin):
    """{(family, functional, quantity): (values, reference, scale, decade)} of every oracle form on every grid"""
    out = {}
    with np.errstate(all="ignore"):
        for fun in gold.LDA_FUNCTIONALS:
            for q, val in oracle_lda(fun, lda.rho).items():
                out[("lda", fun, q)] = (val, lda.ref[fun][q], scale_of(q, lda.rho), lda.dec)
        for fun in GGA_ALL:
            for q, val in oracle_gga(fun, gga.rho, gga.sigma).items():
                out[("gga", fun, q)] = (val, gga.ref[fun][q], scale_of(q, gga.rho, gga.sigma), gga.dec)
        for fun in gold.SPIN_FUNCTIONALS:
            for q, val in oracle_spin(fun, spin.up, spin.dn).items():
                out[("spin", fun, q)] = (val, spin.ref[fun][q], scale_of(q, spin.rho), spin.dec)
    return out


def test_oracle_forms_against_the_fixtures(lda, gga, spin):
    """oracle/terms.py in double precision within 4 x max(E_REF, FLOOR) of the 60-digit values, every functional, quantity
    and grid point; ``lda_fxc`` included."""
    for key, (val, ref, scale, dec) in oracle_all(lda, gga, spin).items():
        check(key, val, ref, scale, dec, MARGIN_ORACLE, "oracle")


def test_e_ref_table_is_the_oracles_error(lda, gga, spin):
    """The table the bounds come from is a record of the oracle's error and of nothing else: no listed entry is more than
    four times what the oracle shows now (an entry inflated to let a kernel pass would fail here)."""
    measured = {key: decade_maxima(scaled_error(val, ref, scale), dec)
                for key, (val, ref, scale, dec) in oracle_all(lda, gga, spin).items()}
    for key, table in E_REF.items():
        for d, listed in table.items():
            assert listed > FLOOR, (key, d)
            assert listed <= 4 * max(measured[key][d], FLOOR), (key, d, listed, measured[key][d])


# ------------------------------------------------------------------------------------------------ the torch twins
def test_torch_twins_against_the_fixtures(lda, gga):
    torch = pytest.importorskip("torch")
    from dftk_jl_amd import terms as dterms
    rho = torch.from_numpy(lda.rho)
    for fun in ("lda_x", "lda_c_vwn", "lda_c_pw"):
        e, v = dterms._FUNCTIONALS[fun](rho)
        check(("lda", fun, "e"), e.numpy(), lda.ref[fun]["e"], scale_of("e", lda.rho), lda.dec, MARGIN, "twin")
        check(("lda", fun, "v"), v.numpy(), lda.ref[fun]["v"], scale_of("v", lda.rho), lda.dec, MARGIN, "twin")
    for fun in GGA_ALL:
        names = ("gga_x_pbe", "gga_c_pbe") if fun == "gga_xc_pbe" else (fun,)
        r = torch.from_numpy(gga.rho).requires_grad_(True)
        s = torch.from_numpy(gga.sigma).requires_grad_(True)
        e = sum(dterms._GGA_FUNCTIONALS[n](r, s) for n in names)
        vr, vs = torch.autograd.grad(e.sum(), (r, s))
        for q, val in (("e", e.detach()), ("vrho", vr), ("vsigma", vs)):
            check(("gga", fun, q), val.numpy(), gga.ref[fun][q], scale_of(q, gga.rho, gga.sigma), gga.dec, MARGIN, "twin")


# ------------------------------------------------------------------------------------------------ fixture = generator
def test_fixtures_match_the_generator(lda, gga, spin):
    pytest.importorskip("mpmath")
    for fun, quantities in gold.LDA_FUNCTIONALS.items():
        for i in range(0, len(lda.rho), 7):
            got = gold.ref_lda(fun, float(lda.rho[i]))
            assert all(got[q] == lda.ref[fun][q][i] for q in quantities), (fun, i)
    for fun in gold.GGA_FUNCTIONALS:
        for i in range(0, len(gga.rho), 7):
            got = gold.ref_gga(fun, float(gga.rho[i]), float(gga.sigma[i]))
            assert all(got[q] == gga.ref[fun][q][i] for q in got), (fun, i)
    for i in range(0, len(gga.rho), 7):                  # the derived reference of both bits together
        got = gold.ref_gga("gga_xc_pbe", float(gga.rho[i]), float(gga.sigma[i]))
        for q in got:
            parts = abs(gga.ref["gga_x_pbe"][q][i]) + abs(gga.ref["gga_c_pbe"][q][i])
            assert abs(got[q] - gga.ref["gga_xc_pbe"][q][i]) <= 2.0 ** -52 * parts, (q, i)
    for fun in gold.SPIN_FUNCTIONALS:
        for i in range(0, len(spin.rho), 7):
            got = gold.ref_spin(fun, float(spin.up[i]), float(spin.dn[i]))
            assert all(got[q] == spin.ref[fun][q][i] for q in got), (fun, i)
    for fun in gold.SPIN_FUNCTIONALS:                    # v_up = v_down at zeta = 0, at every density (v_down is not stored)
        for i in np.flatnonzero(spin.up == spin.dn):
            assert gold.ref_spin(fun, float(spin.up[i]), float(spin.dn[i]))["vdn"] == spin.ref[fun]["vup"][i], (fun, i)
    # PBE correlation at s = 0 is PW92 with libxc's modified a = 0.0310907 (the fixtures hold the original PW92 only)
    mp = gold._mp()
    i_s0 = np.flatnonzero(gga.sigma == 0.0)[::7]
    for i in i_s0:
        pw_mod = float(gold._diff(mp, lambda r: r * gold._pw92_G(mp, gold._rs(mp, r), "eps0_mod"), float(gga.rho[i]), 0, 1.0))
        assert gga.ref["gga_c_pbe"]["e"][i] == pw_mod


def test_fixture_files_are_small():
    names = [n for n in os.listdir(gold.GOLDEN) if n.startswith("xc_mp_")]
    assert len(names) == 16
    assert all(os.path.getsize(os.path.join(gold.GOLDEN, n)) <= gold.MAX_BYTES for n in names)


# ------------------------------------------------------------------------------------------------ the reference itself
def _index_in(rho_small, rho_big):
    idx = np.searchsorted(rho_big, rho_small)
    assert np.array_equal(rho_big[idx], rho_small)
    return idx


def test_reference_is_consistent_with_itself(lda, gga, spin):
    n_main = len(lda.rho) - len(lda.grid["extra_hex"])            # the sorted log grid, before the extra values
    zeta = np.array(spin.grid["zeta"])
    nz = len(zeta)
    # zeta = 0: the collinear forms are the unpolarised ones, and the two channels see the same potential
    z0 = np.flatnonzero(np.tile(zeta, len(spin.rho) // nz) == 0.0)
    idx = _index_in(spin.rho[z0], lda.rho[:n_main])
    for fun in gold.SPIN_FUNCTIONALS:
        assert np.array_equal(spin.ref[fun]["e"][z0], lda.ref[fun]["e"][idx]), fun
        assert np.array_equal(spin.ref[fun]["vup"][z0], lda.ref[fun]["v"][idx]), fun
    # (zeta -> -zeta exchanges the channels: the fixtures are stored that way, test_fixtures_match_the_generator checks it)
    # s = 0: PBE exchange is lda_x; PBE correlation is PW92mod, 1.0e-5 away from PW92 (a = 0.0310907 against 0.031091);
    # de/dsigma is finite and has the sign of the gradient correction (exchange lowers, correlation raises the energy)
    s0 = np.flatnonzero(gga.sigma == 0.0)
    idx = _index_in(gga.rho[s0], lda.rho[:n_main])
    assert np.array_equal(gga.ref["gga_x_pbe"]["e"][s0], lda.ref["lda_x"]["e"][idx])
    assert np.array_equal(gga.ref["gga_x_pbe"]["vrho"][s0], lda.ref["lda_x"]["v"][idx])
    pw = lda.ref["lda_c_pw"]["e"][idx]
    assert np.all(np.abs(gga.ref["gga_c_pbe"]["e"][s0] - pw) <= 2e-5 * np.abs(pw))
    assert np.all(np.isfinite(gga.ref["gga_x_pbe"]["vsigma"][s0])) and np.all(gga.ref["gga_x_pbe"]["vsigma"][s0] < 0)
    assert np.all(np.isfinite(gga.ref["gga_c_pbe"]["vsigma"][s0])) and np.all(gga.ref["gga_c_pbe"]["vsigma"][s0] > 0)
    # the unpolarised Teter form shares the threshold of the collinear one
    dead = lda.rho <= 2e-20
    assert dead.sum() > 40
    assert np.all(lda.ref["lda_xc_teter93"]["e"][dead] == 0.0) and np.all(lda.ref["lda_xc_teter93"]["v"][dead] == 0.0)
    assert np.all(lda.ref["lda_xc_teter93"]["e"][~dead] < 0.0)


# ------------------------------------------------------------------------------------------------ measuring E_REF
def measure_e_ref():
    """{key: {decade: error}} of the oracle, entries above FLOOR only, rounded up to two digits"""
    table = {}
    for key, (val, ref, scale, dec) in oracle_all(load_lda(), load_gga(), load_spin()).items():
        rows = {}
        for d, err in decade_maxima(scaled_error(val, ref, scale), dec).items():
            if err > FLOOR:
                mag = 10.0 ** (math.floor(math.log10(err)) - 1)
                rows[d] = float(f"{math.ceil(err / mag) * mag:.1e}")
        if rows:
            table[key] = rows
    return table


if __name__ == "__main__":
    import textwrap
    print("E_REF = {")
    for key, rows in measure_e_ref().items():
        body = ", ".join(f"{d}: {v:.1e}" for d, v in rows.items())
        print(f"    {key!r}: {{")
        print(textwrap.fill(body, 120, initial_indent=" " * 8, subsequent_indent=" " * 8) + "},")
    print("}")
    sys.exit(0)
