#!/usr/bin/env python3
"""Multiprecision reference of the point-wise exchange-correlation forms: writes tests/golden/xc_mp_*.json and, for the
meta-GGA forms, tests/golden/mgga_mp_*.json.

Only the energy density per volume e of each functional is written down here, from its paper (or the libxc
definition of the same form), with every constant parsed from a decimal string:

  lda_x           Dirac / Slater exchange, e = -3/4 (3/pi)^(1/3) rho^(4/3); spin-scaling relation for two channels
  lda_c_vwn       Vosko, Wilk, Nusair, Can. J. Phys. 58, 1200 (1980), eq. (4.4), paramagnetic fit to Ceperley-Alder ("VWN5")
  lda_c_pw        Perdew, Wang, PRB 45, 13244 (1992), eq. (10) with table I, spin interpolation eq. (8), f''(0) = 1.709921
  lda_xc_teter93  Goedecker, Teter, Hutter, PRB 54, 1703 (1996), appendix: Pade fit with coefficients linear in f(zeta)
  gga_x_pbe       Perdew, Burke, Ernzerhof, PRL 77, 3865 (1996), eq. (14), kappa = 0.8040, mu = 0.2195149727645171
  gga_c_pbe       ibid. eqs. (7), (8) on lda_c_pw_mod (a = 0.0310907), unpolarised (phi = 1)
  mgga_x_scan     Sun, Ruzsinszky, Perdew, PRL 115, 036402 (2015), eq. (2) with the supplement's constants, unpolarised
  mgga_c_scan     ibid. eq. (3) at zeta = 0 (phi = d_x = G_c = 1) on lda_c_pw_mod

Every derivative is a numerical one (``mpmath.diff``, central differences in 800+ bit arithmetic): v = de/drho,
v_sigma = de/dsigma, v_up, v_down, f_xc = d2e/drho2.  No hand-derived formula appears in this file.  Results are good to
60 digits (``mp.dps = 60``) and stored as 17-digit doubles; the guard bits cover the 50 digits that the VWN form cancels
at rho = 1e-300 and the digits a difference quotient loses.  log(1 + x) and exp(x) - 1 of the papers are written log1p(x)
and expm1(x): at rho = 1e-300 the PW92 argument is 1e-198, beyond any guard precision worth paying for.

Semantics of the collinear forms (those of ``dftk_mi_local_potential_collinear`` and of oracle/terms.py): each channel is
evaluated at max(rho_s, 1e-20), the derivative is taken with respect to that clamped variable, and everything is zero
when rho_up + rho_down <= 2e-20.  The unpolarised lda_xc_teter93 is the collinear form at rho_up = rho_down = rho / 2, so
it is zero for rho <= 2e-20 as well.  The other unpolarised forms are the plain functions of rho > 0.

Semantics of the meta-GGA forms (those of ``dftk_mi_xc_mgga``): e(rho, sigma, tau) with alpha = (tau - tau_W) / tau_unif and
no clamp of sigma against 8 rho tau; the switching function is the one of the paper, f(1) = 0; the exchange factor
g_x = 1 - exp(-a1 / p^(1/4)) is 1 for p <= 0, the limit from the right (all its derivatives vanish there).  The kernel
replaces g_x by 1 where the exponential underflows a double, which these values do not distinguish.

The grid helpers at the top need NumPy only; tests/test_xc_reference.py and tests/test_gpu_xc_pointwise.py rebuild the
inputs of a fixture from its "grid" entry with them.  Running this file rewrites the fixtures byte for byte.
"""
import json
import math
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "tests", "golden")
MAX_BYTES = 37108                      # the largest fixture tests/golden held before these
SPIN_FLOOR = 1e-20

# Mantissas as decimal strings: float("3.2e-7") is correctly rounded everywhere, 10 ** (k / 4) need not be.
M4 = ["1", "1.8", "3.2", "5.6"]
LDA_GRID = {"decades": [-30, 5], "mantissas": M4,
            "extra_hex": [float.hex(v) for v in (1e-300 * (1 + 2.0 ** -52), 2e-20, 2.0000001e-20, 4e-20, 4.0000001e-20)]}
GGA_GRID = {"decades": [-28, 4], "mantissas": M4, "s": [0.0, 1e-6, 1e-3, 0.1, 1.0, 3.0, 10.0, 100.0]}
SPIN_GRID = {"decades": [-18, 4], "mantissas": M4,
             "zeta": [0.0, 1e-8, -1e-8, 0.3, -0.3, 0.9, -0.9, 1 - 1e-10, -(1 - 1e-10), 1.0, -1.0]}

LDA_FUNCTIONALS = {"lda_x": ("e", "v", "f"), "lda_c_vwn": ("e", "v", "f"), "lda_c_pw": ("e", "v", "f"),
                   "lda_xc_teter93": ("e", "v")}
GGA_FUNCTIONALS = ("gga_x_pbe", "gga_c_pbe")        # both bits together: the sum of the two, no fixture of its own
# The zeta list holds both signs: v_down(zeta) = v_up(-zeta) has no fixture of its own, and e, even in zeta, is stored
# for zeta >= 0 only.  tests/test_xc_reference.py rebuilds both and has the generator recompute them at sampled points.
SPIN_QUANTITIES = ("e", "vup")
SPIN_FUNCTIONALS = ("lda_x", "lda_c_pw", "lda_xc_teter93")


# ------------------------------------------------------------------------------------------------ grids (NumPy only)
def rho_grid(grid):
    """(rho, decade): mantissa x 10^d for d in [lo, hi), then 10^hi (counted in decade hi - 1), then the extra values"""
    lo, hi = grid["decades"]
    rho = [float(f"{m}e{d}") for d in range(lo, hi) for m in grid["mantissas"]] + [float(f"1e{hi}")]
    dec = [d for d in range(lo, hi) for _ in grid["mantissas"]] + [hi - 1]
    for hx in grid.get("extra_hex", ()):
        rho.append(float.fromhex(hx))
        dec.append(math.floor(math.log10(rho[-1])))
    return np.array(rho), np.array(dec)


def sigma_unit(rho):
    """(2 k_F rho)^2, the sigma of reduced gradient s = 1"""
    return (2.0 * np.cbrt(3.0 * math.pi ** 2 * rho) * rho) ** 2


def gga_grid(grid):
    """(rho, sigma, decade), flat, index = i_rho * n_s + i_s, sigma = s^2 (2 k_F rho)^2"""
    rho, dec = rho_grid(grid)
    s = np.array(grid["s"])
    sigma = (s * s)[None, :] * sigma_unit(rho)[:, None]
    return np.repeat(rho, len(s)), sigma.ravel(), np.repeat(dec, len(s))


def spin_grid(grid):
    """(rho_up, rho_down, rho_total, decade), flat, index = i_rho * n_zeta + i_zeta"""
    rho, dec = rho_grid(grid)
    z = np.array(grid["zeta"])
    up = 0.5 * rho[:, None] * (1.0 + z)[None, :]
    dn = 0.5 * rho[:, None] * (1.0 - z)[None, :]
    return up.ravel(), dn.ravel(), np.repeat(rho, len(z)), np.repeat(dec, len(z))


def spin_even_index(grid):
    """(index of |zeta| among the zeta >= 0 of the list, for every zeta of the list; number of zeta >= 0)"""
    nonneg = [z for z in grid["zeta"] if z >= 0]
    return [nonneg.index(abs(z)) for z in grid["zeta"]], len(nonneg)


MGGA_GRID = {"decades": [-10, 3], "mantissas": ["1"], "s": [0.0, 1e-3, 0.1, 1.0, 3.0, 10.0],
             "alpha": [0.0, 0.1, 0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 2.0, 10.0, 100.0], "tau_zero": True}
MGGA_FUNCTIONALS = ("mgga_x_scan", "mgga_c_scan")   # both bits together: the sum of the two, no fixture of its own
MGGA_QUANTITIES = ("e", "vrho", "vsigma", "vtau")


def tau_unif(rho):
    """(3/10) (3 pi^2)^(2/3) rho^(5/3), the kinetic energy density of the uniform gas"""
    return 0.3 * np.cbrt(3.0 * math.pi ** 2) ** 2 * rho * np.cbrt(rho) ** 2


def mgga_grid(grid):
    """(rho, sigma, tau, decade), flat, index = (i_rho * n_s + i_s) * n_t + i_t; tau = tau_W + alpha tau_unif with
    tau_W = sigma / (8 rho) for every alpha of the list, then tau = 0"""
    rho, dec = rho_grid(grid)
    s = np.array(grid["s"])
    n_t = len(grid["alpha"]) + (1 if grid["tau_zero"] else 0)
    sigma = ((s * s)[None, :] * sigma_unit(rho)[:, None]).ravel()
    rho_s = np.repeat(rho, len(s))
    tau = np.zeros((len(rho_s), n_t))
    tau[:, :len(grid["alpha"])] = (sigma / (8.0 * rho_s))[:, None] + np.array(grid["alpha"])[None, :] * tau_unif(rho_s)[:, None]
    return np.repeat(rho_s, n_t), np.repeat(sigma, n_t), tau.ravel(), np.repeat(np.repeat(dec, len(s)), n_t)


def mgga_fixture_path(functional, quantity):
    return os.path.normpath(os.path.join(GOLDEN, f"mgga_mp_{functional}_{quantity}.json"))


def load_mgga_fixture(functional, quantity):
    with open(mgga_fixture_path(functional, quantity)) as fh:
        return json.load(fh)


def fixture_path(family, functional, quantity=None):
    name = f"xc_mp_{family}_{functional}" + (f"_{quantity}" if quantity else "") + ".json"
    return os.path.normpath(os.path.join(GOLDEN, name))


def load_fixture(family, functional, quantity=None):
    with open(fixture_path(family, functional, quantity)) as fh:
        return json.load(fh)


# ------------------------------------------------------------------------------------------------ the functionals (mpmath)
DPS = 60
GUARD_BITS = 128          # diff: h = 2^-(prec + GUARD_BITS) x scale, working precision (prec + 2 GUARD_BITS) (n + 1) bits


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def _rs(mp, rho):
    return mp.cbrt(3 / (4 * mp.pi * rho))


def e_lda_x(mp, rho):
    return -mp.mpf(3) / 4 * mp.cbrt(3 / mp.pi) * rho * mp.cbrt(rho)


def e_lda_c_vwn(mp, rho):
    A, b, c, x0 = mp.mpf("0.0310907"), mp.mpf("3.72744"), mp.mpf("12.9352"), mp.mpf("-0.10498")
    x = mp.sqrt(_rs(mp, rho))

    def X(y):
        return y * y + b * y + c
    Q = mp.sqrt(4 * c - b * b)
    at = mp.atan(Q / (2 * x + b))
    eps = A * (mp.log(x * x / X(x)) + 2 * b / Q * at
               - b * x0 / X(x0) * (mp.log((x - x0) ** 2 / X(x)) + 2 * (b + 2 * x0) / Q * at))
    return rho * eps


PW92 = {   # table I of Perdew, Wang 1992: A, alpha1, beta1 .. beta4 (p = 1)
    "eps0": ("0.031091", "0.21370", "7.5957", "3.5876", "1.6382", "0.49294"),
    "eps1": ("0.015545", "0.20548", "14.1189", "6.1977", "3.3662", "0.62517"),
    "-alpha_c": ("0.016887", "0.11125", "10.357", "3.6231", "0.88026", "0.49671"),
    "eps0_mod": ("0.0310907", "0.21370", "7.5957", "3.5876", "1.6382", "0.49294"),      # libxc lda_c_pw_mod
}


def _pw92_G(mp, rs, which):
    A, a1, b1, b2, b3, b4 = (mp.mpf(s) for s in PW92[which])
    # log1p, expm1: at rho = 1e-300 the argument is 1e-198, which no affordable guard precision keeps next to 1
    return -2 * A * (1 + a1 * rs) * mp.log1p(1 / (2 * A * (b1 * mp.sqrt(rs) + b2 * rs + b3 * rs ** mp.mpf("1.5") + b4 * rs ** 2)))


def e_lda_c_pw(mp, rho):
    return rho * _pw92_G(mp, _rs(mp, rho), "eps0")


def _fzeta(mp, up, dn):
    rt = up + dn
    p = mp.mpf(4) / 3
    return ((2 * up / rt) ** p + (2 * dn / rt) ** p - 2) / (2 ** p - 2)


def e_spin_lda_x(mp, up, dn):
    return (e_lda_x(mp, 2 * up) + e_lda_x(mp, 2 * dn)) / 2


def e_spin_lda_c_pw(mp, up, dn):
    rt = up + dn
    zeta, fz, rs = (up - dn) / rt, _fzeta(mp, up, dn), _rs(mp, rt)
    e0, e1, alpha_c = _pw92_G(mp, rs, "eps0"), _pw92_G(mp, rs, "eps1"), -_pw92_G(mp, rs, "-alpha_c")
    return rt * (e0 + alpha_c * fz / mp.mpf("1.709921") * (1 - zeta ** 4) + (e1 - e0) * fz * zeta ** 4)


TETER = {"a": ("0.4581652932831429", "2.217058676663745", "0.7405551735357053", "0.01968227878617998"),
         "da": ("0.119086804055547", "0.6157402568883345", "0.1574201515892867", "0.003532336663397157"),
         "b": ("1.0", "4.504130959426697", "1.110667363742916", "0.02359291751427506"),
         "db": ("0.0", "0.2673612973836267", "0.2052004607777787", "0.004200005045691381")}


def e_spin_lda_xc_teter93(mp, up, dn):
    rt = up + dn
    fz, rs = _fzeta(mp, up, dn), _rs(mp, rt)
    num = sum((mp.mpf(TETER["a"][i]) + mp.mpf(TETER["da"][i]) * fz) * rs ** i for i in range(4))
    den = sum((mp.mpf(TETER["b"][i]) + mp.mpf(TETER["db"][i]) * fz) * rs ** (i + 1) for i in range(4))
    return -rt * num / den


def e_gga_x_pbe(mp, rho, sigma):
    kappa, mu = mp.mpf("0.8040"), mp.mpf("0.2195149727645171")
    kf = mp.cbrt(3 * mp.pi ** 2 * rho)
    s2 = sigma / (2 * kf * rho) ** 2
    return e_lda_x(mp, rho) * (1 + kappa - kappa / (1 + mu * s2 / kappa))


def e_gga_c_pbe(mp, rho, sigma):
    beta, gamma = mp.mpf("0.06672455060314922"), (1 - mp.log(2)) / mp.pi ** 2
    eps = _pw92_G(mp, _rs(mp, rho), "eps0_mod")
    kf = mp.cbrt(3 * mp.pi ** 2 * rho)
    ks = mp.sqrt(4 * kf / mp.pi)
    t2 = sigma / (2 * ks * rho) ** 2
    A = beta / gamma / mp.expm1(-eps / gamma)
    H = gamma * mp.log1p(beta / gamma * t2 * (1 + A * t2) / (1 + A * t2 + A * A * t2 * t2))
    return rho * (eps + H)


def e_gga_xc_pbe(mp, rho, sigma):
    return e_gga_x_pbe(mp, rho, sigma) + e_gga_c_pbe(mp, rho, sigma)


def _scan_common(mp, rho, sigma, tau):
    """(p, alpha) = (s^2, (tau - tau_W) / tau_unif)"""
    kf = mp.cbrt(3 * mp.pi ** 2 * rho)
    p = sigma / (2 * kf * rho) ** 2
    t_unif = mp.mpf(3) / 10 * kf ** 2 * rho
    return p, (tau - sigma / (8 * rho)) / t_unif


def _scan_switch(mp, alpha, c1, c2, d):
    if alpha < 1:
        return mp.exp(-mp.mpf(c1) * alpha / (1 - alpha))
    if alpha == 1:
        return mp.mpf(0)
    return -mp.mpf(d) * mp.exp(mp.mpf(c2) / (1 - alpha))


def e_mgga_x_scan(mp, rho, sigma, tau):
    p, alpha = _scan_common(mp, rho, sigma, tau)
    k1, h0, a1, mu = mp.mpf("0.065"), mp.mpf("1.174"), mp.mpf("4.9479"), mp.mpf(10) / 81
    b2 = mp.sqrt(mp.mpf(5913) / 405000)
    b1 = mp.mpf(511) / 13500 / (2 * b2)
    b3 = mp.mpf("0.5")
    b4 = mu * mu / k1 - mp.mpf(1606) / 18225 - b1 * b1
    oma = 1 - alpha
    y = mu * p + b4 * p * p * mp.exp(-b4 * p / mu) + (b1 * p + b2 * oma * mp.exp(-b3 * oma * oma)) ** 2
    h1 = 1 + k1 - k1 / (1 + y / k1)
    gx = 1 - mp.exp(-a1 / mp.sqrt(mp.sqrt(p))) if p > 0 else mp.mpf(1)
    fx = _scan_switch(mp, alpha, "0.667", "0.8", "1.24")
    return e_lda_x(mp, rho) * (h1 + fx * (h0 - h1)) * gx


def e_mgga_c_scan(mp, rho, sigma, tau):
    p, alpha = _scan_common(mp, rho, sigma, tau)
    rs = _rs(mp, rho)
    gamma = (1 - mp.log(2)) / mp.pi ** 2
    b1c, b2c, b3c, chi = mp.mpf("0.0285764"), mp.mpf("0.0889"), mp.mpf("0.125541"), mp.mpf("0.12802585262625815")
    eps = _pw92_G(mp, rs, "eps0_mod")
    beta = mp.mpf("0.066725") * (1 + mp.mpf("0.1") * rs) / (1 + mp.mpf("0.1778") * rs)
    kf = mp.cbrt(3 * mp.pi ** 2 * rho)
    t2 = mp.pi * sigma / (16 * kf * rho * rho)
    w1 = mp.expm1(-eps / gamma)
    A = beta / (gamma * w1)
    eps1 = eps + gamma * mp.log1p(w1 * (1 - 1 / mp.sqrt(mp.sqrt(1 + 4 * A * t2))))
    e0 = -b1c / (1 + b2c * mp.sqrt(rs) + b3c * rs)
    w0 = mp.expm1(-e0 / b1c)
    eps0 = e0 + b1c * mp.log1p(w0 * (1 - 1 / mp.sqrt(mp.sqrt(1 + 4 * chi * p))))
    fc = _scan_switch(mp, alpha, "0.64", "1.5", "0.7")
    return rho * (eps1 + fc * (eps0 - eps1))


E_MGGA = {"mgga_x_scan": e_mgga_x_scan, "mgga_c_scan": e_mgga_c_scan}
E_UNPOL = {"lda_x": e_lda_x, "lda_c_vwn": e_lda_c_vwn, "lda_c_pw": e_lda_c_pw}
E_SPIN = {"lda_x": e_spin_lda_x, "lda_c_pw": e_spin_lda_c_pw, "lda_xc_teter93": e_spin_lda_xc_teter93}
E_GGA = {"gga_x_pbe": e_gga_x_pbe, "gga_c_pbe": e_gga_c_pbe, "gga_xc_pbe": e_gga_xc_pbe}


def _diff(mp, f, x, n, scale):
    """d^n f / dx^n at x by central differences with steps of 2^-(prec + GUARD_BITS) x scale"""
    if n == 0:
        with mp.workprec(mp.mp.prec + 2 * GUARD_BITS):
            return +f(mp.mpf(x))
    h = mp.ldexp(mp.mpf(scale), -(mp.mp.prec + GUARD_BITS))
    return mp.diff(f, mp.mpf(x), n, h=h, addprec=GUARD_BITS)


def ref_lda(functional, rho):
    """{"e", "v"[, "f"]} at one density (a double)"""
    mp = _mp()
    if functional == "lda_xc_teter93":
        if rho <= 2 * SPIN_FLOOR:
            return {"e": 0.0, "v": 0.0}

        def e(r):
            return e_spin_lda_xc_teter93(mp, r / 2, r / 2)
    else:
        def e(r):
            return E_UNPOL[functional](mp, r)
    return {q: float(_diff(mp, e, rho, n, rho)) for q, n in zip(LDA_FUNCTIONALS[functional], (0, 1, 2))}


def ref_gga(functional, rho, sigma):
    """{"e", "vrho", "vsigma"} at one point (doubles)"""
    mp = _mp()
    fun = E_GGA[functional]
    r, sg = mp.mpf(rho), mp.mpf(sigma)
    return {"e": float(_diff(mp, lambda x: fun(mp, x, sg), rho, 0, rho)),
            "vrho": float(_diff(mp, lambda x: fun(mp, x, sg), rho, 1, rho)),
            "vsigma": float(_diff(mp, lambda x: fun(mp, r, x), sigma, 1, max(sigma, float(sigma_unit(rho)))))}


def ref_mgga(functional, rho, sigma, tau):
    """{"e", "vrho", "vsigma", "vtau"} at one point (doubles)"""
    mp = _mp()
    fun = E_MGGA[functional]
    r, sg, tu = mp.mpf(rho), mp.mpf(sigma), mp.mpf(tau)
    return {"e": float(_diff(mp, lambda x: fun(mp, x, sg, tu), rho, 0, rho)),
            "vrho": float(_diff(mp, lambda x: fun(mp, x, sg, tu), rho, 1, rho)),
            "vsigma": float(_diff(mp, lambda x: fun(mp, r, x, tu), sigma, 1, max(sigma, float(sigma_unit(rho))))),
            "vtau": float(_diff(mp, lambda x: fun(mp, r, sg, x), tau, 1, max(tau, float(tau_unif(rho)))))}


def ref_spin(functional, up, dn):
    """{"e", "vup", "vdn"} at one point (doubles), with the clamp and the threshold of the module docstring"""
    mp = _mp()
    if up + dn <= 2 * SPIN_FLOOR:
        return {"e": 0.0, "vup": 0.0, "vdn": 0.0}
    fun = E_SPIN[functional]
    a, b = max(up, SPIN_FLOOR), max(dn, SPIN_FLOOR)
    ma, mb = mp.mpf(a), mp.mpf(b)
    return {"e": float(_diff(mp, lambda x: fun(mp, x, mb), a, 0, a)),
            "vup": float(_diff(mp, lambda x: fun(mp, x, mb), a, 1, a)),
            "vdn": float(_diff(mp, lambda x: fun(mp, ma, x), b, 1, b))}


# ------------------------------------------------------------------------------------------------ writing
def _dump(path, head, values):
    lines = ["{"]
    for k, v in head.items():
        lines.append(f' "{k}": {json.dumps(v)},')
    lines.append(' "values": {')
    items = list(values.items())
    for j, (q, arr) in enumerate(items):
        body = ",".join("%.17g" % x for x in arr)
        lines.append(f'  "{q}": [{body}]' + ("," if j + 1 < len(items) else ""))
    lines += [" }", "}", ""]
    text = "\n".join(lines)
    assert len(text.encode()) <= MAX_BYTES, (path, len(text))
    with open(path, "w") as fh:
        fh.write(text)
    print(f"{os.path.relpath(path)}: {len(text)} bytes")


def main_mgga():
    head = {"generator": "tools/make_golden_xc.py", "mp_dps": DPS}
    rho, sigma, tau, _ = mgga_grid(MGGA_GRID)
    for fun in MGGA_FUNCTIONALS:
        rows = [ref_mgga(fun, float(r), float(s), float(t)) for r, s, t in zip(rho, sigma, tau)]
        for q in MGGA_QUANTITIES:
            _dump(mgga_fixture_path(fun, q), dict(head, family="mgga", functional=fun, grid=MGGA_GRID), {q: [row[q] for row in rows]})


def main():
    if sys.argv[1:] == ["mgga"]:        # the meta-GGA fixtures alone
        return main_mgga()
    head = {"generator": "tools/make_golden_xc.py", "mp_dps": DPS}
    rho, _ = rho_grid(LDA_GRID)
    for fun, quantities in LDA_FUNCTIONALS.items():
        rows = [ref_lda(fun, float(r)) for r in rho]
        _dump(fixture_path("lda", fun), dict(head, family="lda", functional=fun, grid=LDA_GRID),
              {q: [row[q] for row in rows] for q in quantities})
    rho, sigma, _ = gga_grid(GGA_GRID)
    for fun in GGA_FUNCTIONALS:
        rows = [ref_gga(fun, float(r), float(s)) for r, s in zip(rho, sigma)]
        for q in ("e", "vrho", "vsigma"):       # one file per quantity: three together exceed the size limit
            _dump(fixture_path("gga", fun, q), dict(head, family="gga", functional=fun, grid=GGA_GRID), {q: [row[q] for row in rows]})
    up, dn, _, _ = spin_grid(SPIN_GRID)
    for fun in SPIN_FUNCTIONALS:
        rows = [ref_spin(fun, float(a), float(b)) for a, b in zip(up, dn)]
        zeta = SPIN_GRID["zeta"] * (len(rows) // len(SPIN_GRID["zeta"]))
        values = {"e": [row["e"] for row, z in zip(rows, zeta) if z >= 0], "vup": [row["vup"] for row in rows]}
        for q in SPIN_QUANTITIES:
            _dump(fixture_path("spin", fun, q), dict(head, family="spin", functional=fun, grid=SPIN_GRID), {q: values[q]})
    main_mgga()


if __name__ == "__main__":
    sys.exit(main())
