"""The point-wise SCAN forms (mgga_x_scan, mgga_c_scan) against a 60-digit reference (host side).

tests/golden/mgga_mp_*.json hold e, de/drho, de/dsigma, de/dtau of the two functionals, computed by tools/make_golden_xc.py in
mpmath from the energy densities alone (every derivative is ``mpmath.diff``) on the grid
    rho = 1e-10 ... 1e3 by decades,  s in {0, 1e-3, 0.1, 1, 3, 10},
    tau = tau_W + alpha tau_unif with alpha in {0, 0.1, 0.5, 0.9, 0.99, 1, 1.01, 1.1, 2, 10, 100}, and tau = 0
(1008 points; tau = 0 gives alpha = -5/3 s^2 < 0).  (The fixtures do not carry the ``xc_mp_`` prefix of the LDA / GGA ones:
tests/test_xc_reference.py counts the files of that prefix.)

Error measure: that of tests/test_xc_reference.py, every error scaled by the LDA-exchange quantity of the same density,
    e: |de| / |e_x(rho)|     vrho: |dv| / |v_x(rho)|     vsigma: |dv_sigma| max(sigma, (2 k_F rho)^2) / |e_x(rho)|
    vtau: |dv_tau| max(tau, tau_unif) / |e_x(rho)|
and asserted as |d| <= bound * scale.

Bounds: per functional, quantity and decade of rho, ``margin * max(E_REF, FLOOR)``.  E_REF is the largest scaled error in that
decade of the double-precision NumPy restatement tests/mgga_ref.py against the fixtures, measured on the CPU
(``python tests/test_mgga_reference.py`` prints the table) and listed below where it exceeds FLOOR = 4 * 2^-52.  Nothing in it
comes from a kernel.  The restatement is held to margin 4 of its own recorded error, the kernel
(tests/test_gpu_mgga_pointwise.py) to margin 8, for the reasons given in tests/test_xc_reference.py.  The largest entries
(a few 1e-14) are those of s = 10, alpha = 0.9: tau_W = 167 tau_unif there, the scales of v_sigma and v_tau grow with it, and
the switching function is steep.  Both the restatement and the kernel take the difference tau - tau_W with the rounding error
of the quotient sigma / (8 rho) removed (an error-free product in float64 here, one fma there); without that the same points show 1e-12,
and by how much depends on the luck of one rounding per decade.
No grid point is skipped, masked or filtered anywhere.
"""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
_spec = importlib.util.spec_from_file_location("make_golden_xc", os.path.join(ROOT, "tools", "make_golden_xc.py"))
gold = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gold)

import mgga_ref  # noqa: E402

FLOOR = 4 * 2.0 ** -52
MARGIN_RESTATEMENT = 4
MARGIN = 8                       # kernels
QUANTITIES = gold.MGGA_QUANTITIES
MGGA_ALL = ("mgga_x_scan", "mgga_c_scan", "mgga_xc_scan")   # the last one: both bits together, reference = sum of the two
CX = -0.75 * (3 / math.pi) ** (1 / 3)

# E_REF[(functional, quantity)] = {decade of rho: largest scaled error of tests/mgga_ref.py against the fixtures}, rounded up
# to two digits; decades that are not listed are at or below FLOOR = 8.9e-16.
E_REF = {
    ('mgga_x_scan', 'vrho'): {
        -10: 2.0e-14, -9: 6.2e-15, -8: 1.4e-14, -7: 1.2e-14, -6: 8.5e-15, -5: 1.4e-14, -4: 7.3e-15, -3: 9.1e-15, -2:
        1.3e-14, -1: 2.1e-14, 0: 1.1e-14, 1: 6.7e-15, 2: 2.6e-14},
    ('mgga_x_scan', 'vsigma'): {
        -10: 2.7e-14, -9: 7.5e-15, -8: 1.7e-14, -7: 1.6e-14, -6: 9.1e-15, -5: 1.9e-14, -4: 6.9e-15, -3: 1.2e-14, -2:
        1.5e-14, -1: 2.9e-14, 0: 1.2e-14, 1: 9.1e-15, 2: 3.5e-14},
    ('mgga_x_scan', 'vtau'): {
        -10: 2.8e-14, -9: 9.3e-15, -8: 1.8e-14, -7: 1.6e-14, -6: 8.7e-15, -5: 2.0e-14, -4: 1.1e-14, -3: 7.2e-15, -2:
        1.5e-14, -1: 2.9e-14, 0: 1.2e-14, 1: 9.8e-15, 2: 3.5e-14},
    ('mgga_c_scan', 'vrho'): {
        -10: 3.5e-14, -9: 5.3e-15, -8: 2.0e-14, -7: 1.5e-14, -6: 2.9e-15, -5: 8.6e-15, -4: 9.2e-16, -3: 2.6e-15, -2:
        5.0e-15, -1: 9.5e-16, 0: 2.7e-15, 1: 9.7e-16},
    ('mgga_c_scan', 'vsigma'): {
        -10: 4.8e-14, -9: 5.0e-15, -8: 2.7e-14, -7: 2.0e-14, -6: 1.9e-15, -5: 1.2e-14, -4: 1.4e-15, -3: 3.7e-15, -2:
        7.2e-15, -1: 1.3e-15, 0: 3.6e-15, 1: 1.4e-15, 2: 1.9e-15},
    ('mgga_c_scan', 'vtau'): {
        -10: 4.7e-14, -9: 4.7e-15, -8: 3.0e-14, -7: 2.0e-14, -6: 2.9e-15, -5: 1.2e-14, -4: 1.3e-15, -3: 4.1e-15, -2:
        7.1e-15, -1: 1.3e-15, 0: 3.6e-15, 1: 1.4e-15},
    ('mgga_xc_scan', 'vrho'): {
        -10: 1.6e-14, -9: 8.9e-15, -8: 3.3e-14, -7: 9.2e-15, -6: 5.7e-15, -5: 1.4e-14, -4: 7.3e-15, -3: 1.2e-14, -2:
        1.7e-14, -1: 2.0e-14, 0: 8.2e-15, 1: 5.1e-15, 2: 2.6e-14},
    ('mgga_xc_scan', 'vsigma'): {
        -10: 2.2e-14, -9: 1.3e-14, -8: 4.4e-14, -7: 1.3e-14, -6: 9.1e-15, -5: 1.3e-14, -4: 6.9e-15, -3: 1.5e-14, -2:
        1.5e-14, -1: 2.8e-14, 0: 9.0e-15, 1: 6.1e-15, 2: 3.5e-14},
    ('mgga_xc_scan', 'vtau'): {
        -10: 2.0e-14, -9: 1.2e-14, -8: 4.8e-14, -7: 1.1e-14, -6: 8.7e-15, -5: 1.4e-14, -4: 1.2e-14, -3: 7.3e-15, -2:
        1.6e-14, -1: 2.8e-14, 0: 1.1e-14, 1: 9.8e-15, 2: 3.5e-14},
}


def e_x(rho):
    return np.abs(CX * rho * np.cbrt(rho))


def v_x(rho):
    return np.abs(4 / 3 * CX * np.cbrt(rho))


def scale_of(quantity, F):
    """the scale of one quantity on the points of F (arrays)"""
    if quantity == "e":
        return e_x(F.rho)
    if quantity == "vsigma":
        return e_x(F.rho) / np.maximum(F.sigma, gold.sigma_unit(F.rho))
    if quantity == "vtau":
        return e_x(F.rho) / np.maximum(F.tau, gold.tau_unif(F.rho))
    return v_x(F.rho)


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
    """assert |got - ref| <= margin * max(E_REF, FLOOR) * scale at every point; returns the scaled errors"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and np.all(np.isfinite(got)), (label, key)
    err = scaled_error(got, ref, scale)
    bound = bound_of(key, dec, margin)
    bad = np.flatnonzero(~(np.abs(got - ref) <= bound * scale))
    assert bad.size == 0, (f"{label} {key}: {bad.size} points above margin {margin}; worst scaled error "
                           f"{err[bad].max():.3e} against {bound[bad][np.argmax(err[bad])]:.3e} at index "
                           f"{bad[np.argmax(err[bad])]}: got {got[bad[np.argmax(err[bad])]]!r}, "
                           f"reference {ref[bad[np.argmax(err[bad])]]!r}")
    return err


class Family:
    pass


def load_mgga():
    F = Family()
    F.ref = {}
    for fun in gold.MGGA_FUNCTIONALS:
        F.ref[fun] = {}
        for q in QUANTITIES:
            fx = gold.load_mgga_fixture(fun, q)
            F.grid = fx["grid"]
            F.ref[fun][q] = np.array(fx["values"][q])
    # both bits together: the sum of the two stored references (one more rounding, 2^-53 of the larger part)
    F.ref["mgga_xc_scan"] = {q: F.ref["mgga_x_scan"][q] + F.ref["mgga_c_scan"][q] for q in QUANTITIES}
    F.rho, F.sigma, F.tau, F.dec = gold.mgga_grid(F.grid)
    F.n_s, F.n_t = len(F.grid["s"]), len(F.grid["alpha"]) + 1
    return F


@pytest.fixture(scope="module")
def mgga():
    return load_mgga()


def restatement_all(F):
    """{(functional, quantity): (values, reference, scale, decade)} of tests/mgga_ref.py on the grid"""
    out = {}
    for fun in MGGA_ALL:
        for q, val in mgga_ref.scan(fun, F.rho, F.sigma, F.tau).items():
            out[(fun, q)] = (val, F.ref[fun][q], scale_of(q, F), F.dec)
    return out


def test_grid_is_the_one_asked_for(mgga):
    assert mgga.grid == gold.MGGA_GRID and len(mgga.rho) == 14 * 6 * 12 == 1008
    assert mgga.rho.min() == 1e-10 and mgga.rho.max() == 1e3 and np.all(mgga.tau >= 0)
    assert np.sum(mgga.tau == 0.0) == 14 * 6 + 14             # tau = 0 at every (rho, s), and alpha = 0 at s = 0
    assert np.sum(mgga.sigma == 0.0) == 14 * 12


def test_restatement_against_the_fixtures(mgga):
    """tests/mgga_ref.py in double precision within 4 x max(E_REF, FLOOR) of the 60-digit values, every functional, quantity
    and grid point."""
    for key, (val, ref, scale, dec) in restatement_all(mgga).items():
        check(key, val, ref, scale, dec, MARGIN_RESTATEMENT, "restatement")


def test_e_ref_table_is_the_restatements_error(mgga):
    """The table the bounds come from is a record of the restatement's error and of nothing else: no listed entry is more
    than four times what the restatement shows now (an entry inflated to let a kernel pass would fail here)."""
    measured = {key: decade_maxima(scaled_error(val, ref, scale), dec)
                for key, (val, ref, scale, dec) in restatement_all(mgga).items()}
    assert set(E_REF) <= set(measured)
    for key, table in E_REF.items():
        for d, listed in table.items():
            assert listed > FLOOR, (key, d)
            assert listed <= 4 * max(measured[key][d], FLOOR), (key, d, listed, measured[key][d])


def test_fixtures_match_the_generator(mgga):
    pytest.importorskip("mpmath")
    for fun in gold.MGGA_FUNCTIONALS:
        for i in range(0, len(mgga.rho), 7):
            got = gold.ref_mgga(fun, float(mgga.rho[i]), float(mgga.sigma[i]), float(mgga.tau[i]))
            assert all(got[q] == mgga.ref[fun][q][i] for q in QUANTITIES), (fun, i)


def test_fixture_files_are_small():
    names = [n for n in os.listdir(gold.GOLDEN) if n.startswith("mgga_mp_")]
    assert len(names) == 8
    assert all(os.path.getsize(os.path.join(gold.GOLDEN, n)) <= gold.MAX_BYTES for n in names)


def test_reference_is_consistent_with_itself(mgga):
    """Limits that the constants must reproduce, on the fixtures alone.
    * s = 0, alpha = 1 (the uniform gas): SCAN exchange is lda_x, SCAN correlation is PW92mod = gga_c_pbe at s = 0; the
      switching functions vanish with zero slope there, so v_tau = 0.
    * s = 0, alpha = 0: F_x = h0 g_x = 1.174; correlation is eps_LDA0 alone.
    * e_x < 0 and e_c <= 0 everywhere; v_tau >= 0 wherever the switch moves (both energies rise from alpha = 0 to 1)."""
    s0a1 = np.flatnonzero((mgga.sigma == 0.0) & (np.arange(len(mgga.rho)) % mgga.n_t == mgga.grid["alpha"].index(1.0)))
    assert len(s0a1) == 14
    gga_e = np.array(gold.load_fixture("gga", "gga_c_pbe", "e")["values"]["e"])
    g_rho, g_sigma, _ = gold.gga_grid(gold.load_fixture("gga", "gga_c_pbe", "e")["grid"])
    lda = np.array(gold.load_fixture("lda", "lda_x")["values"]["e"])
    l_rho, _ = gold.rho_grid(gold.load_fixture("lda", "lda_x")["grid"])
    for i in s0a1:
        x_lda = lda[np.flatnonzero(l_rho == mgga.rho[i])[0]]
        c_pbe = gga_e[np.flatnonzero((g_rho == mgga.rho[i]) & (g_sigma == 0.0))[0]]
        # tau = tau_unif is rounded, alpha = 1 + O(2^-52): the switch is exp(-1e15) there, the rest moves by a few ulp
        assert abs(mgga.ref["mgga_x_scan"]["e"][i] - x_lda) <= 1e-14 * abs(x_lda)
        assert abs(mgga.ref["mgga_c_scan"]["e"][i] - c_pbe) <= 1e-14 * abs(c_pbe)
        assert abs(mgga.ref["mgga_c_scan"]["vtau"][i]) * gold.tau_unif(mgga.rho[i]) <= 1e-14 * abs(c_pbe)
    s0a0 = np.flatnonzero((mgga.sigma == 0.0) & (mgga.tau == 0.0))
    assert len(s0a0) == 28
    ex = CX * mgga.rho[s0a0] * np.cbrt(mgga.rho[s0a0])
    assert np.all(np.abs(mgga.ref["mgga_x_scan"]["e"][s0a0] - 1.174 * ex) <= 1e-14 * np.abs(ex))
    rs = np.cbrt(3 / (4 * math.pi * mgga.rho[s0a0]))
    e0 = -0.0285764 / (1 + 0.0889 * np.sqrt(rs) + 0.125541 * rs) * mgga.rho[s0a0]
    assert np.all(np.abs(mgga.ref["mgga_c_scan"]["e"][s0a0] - e0) <= 1e-14 * np.abs(e0))
    assert np.all(mgga.ref["mgga_x_scan"]["e"] < 0) and np.all(mgga.ref["mgga_c_scan"]["e"] <= 0)
    assert np.all(np.isfinite(mgga.ref["mgga_xc_scan"][q]).all() for q in QUANTITIES)


# ------------------------------------------------------------------------------------------------ measuring E_REF
def measure_e_ref():
    """{key: {decade: error}} of the restatement, entries above FLOOR only, rounded up to two digits"""
    table = {}
    for key, (val, ref, scale, dec) in restatement_all(load_mgga()).items():
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
