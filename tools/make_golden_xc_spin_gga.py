#!/usr/bin/env python3
"""Multiprecision reference of the spin-polarised PBE forms: writes tests/golden/xc_spingga_mp_*.json.

As tools/make_golden_xc.py (whose helpers and unpolarised forms are imported, and which stays as it is): only the energy
density per volume e(rho_up, rho_down, sigma_uu, sigma_ud, sigma_dd) is written down, from the published definitions
(libxc's polarised gga_x_pbe and gga_c_pbe), every constant parsed from a decimal string, and every derivative is
``mpmath.diff`` at 60 digits:

  gga_x_pbe   spin-scaling relation e_x = 1/2 [e_x0(2 rho_up, 4 sigma_uu) + e_x0(2 rho_down, 4 sigma_dd)] on the
              unpolarised form of make_golden_xc.py (Perdew, Burke, Ernzerhof 1996, eq. (14); Oliver, Perdew 1979)
  gga_c_pbe   e_c = rho [eps_c(rs, zeta) + H(rs, zeta, t)], PBE eqs. (7), (8) with phi = ((1 + zeta)^(2/3) + (1 - zeta)^(2/3)) / 2,
              t^2 = pi sigma_tot / (16 phi^2 k_F rho^2), sigma_tot = sigma_uu + 2 sigma_ud + sigma_dd, and eps_c the PW92
              interpolation (eq. (8) of Perdew, Wang 1992) with libxc's lda_c_pw_mod parameters: A = 0.0310907, 0.01554535,
              0.0168869 and f''(0) = 1.709920934161365617563962776245

Semantics (those of ``dftk_mi_xc_gga_spin``): each channel enters as max(rho_s, 1e-20), derivatives are taken with respect to
the clamped variable, everything is zero when rho_up + rho_down <= 2e-20.

Grid: rho_total = 1e-18 ... 1e4 by decade, zeta in {0, +-0.3, +-0.9, +-(1 - 1e-6), +-1}, reduced gradient s in {0, 1e-3, 1, 10}
of the total density with parallel gradients, sigma = s^2 (2 k_F rho)^2.  The gradient is split as grad rho_s = (rho_s / rho)
g e_s with the two unit vectors at cos = 1 (parallel: sigma_ud > 0, sigma_tot = sigma) and cos = -1/2 (sigma_ud < 0);
s = 0 is stored once.  Quantities: e, vup = de/drho_up, vsuu = de/dsigma_uu, vsud = de/dsigma_ud; de/drho_down and de/dsigma_dd
are the values at the point with the channels exchanged (zeta -> -zeta), which is on the grid.

Two identities are asserted here at 50 digits before anything is written: at zeta = 0 with parallel gradients the forms
are e_gga_x_pbe / e_gga_c_pbe of make_golden_xc.py at (rho, sigma); at zeta = +-1 exchange is 1/2 e_x0(2 rho, 4 sigma) of the
filled channel (plus the floor term 1/2 e_x0(2e-20, 0) of the empty one).  Running this file rewrites the fixtures byte for
byte.
"""
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_xc", os.path.join(_HERE, "make_golden_xc.py"))
gold = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gold)

MAX_BYTES = gold.MAX_BYTES
SPIN_FLOOR = gold.SPIN_FLOOR
GRID = {"decades": [-18, 4], "mantissas": ["1"],
        "zeta": [0.0, 0.3, -0.3, 0.9, -0.9, 1 - 1e-6, -(1 - 1e-6), 1.0, -1.0],
        "s": [0.0, 1e-3, 1.0, 10.0], "cos": [1.0, -0.5]}
FUNCTIONALS = ("gga_x_pbe", "gga_c_pbe")
QUANTITIES = ("e", "vup", "vsuu", "vsud")
PW92_MOD = {   # libxc lda_c_pw_mod: A, alpha1, beta1 .. beta4
    "eps0": ("0.0310907", "0.21370", "7.5957", "3.5876", "1.6382", "0.49294"),
    "eps1": ("0.01554535", "0.20548", "14.1189", "6.1977", "3.3662", "0.62517"),
    "-alpha_c": ("0.0168869", "0.11125", "10.357", "3.6231", "0.88026", "0.49671"),
}
FZ20 = "1.709920934161365617563962776245"


# ------------------------------------------------------------------------------------------------ grid (NumPy only)
def spin_gga_grid(grid):
    """dict of flat arrays up, dn, suu, sud, sdd, rho, dec, zeta, s, cos; index = (i_rho, i_zeta, j) with j running over
    s = 0 once and then (s, cos) for s > 0"""
    rho, dec = gold.rho_grid(grid)
    sc = [(s, c) for s in grid["s"] for c in (grid["cos"] if s > 0 else grid["cos"][:1])]
    out = {k: [] for k in ("up", "dn", "suu", "sud", "sdd", "rho", "dec", "zeta", "s", "cos")}
    unit = gold.sigma_unit(rho)
    for r, d, u in zip(rho, dec, unit):
        for z in grid["zeta"]:
            for s, c in sc:
                sig = (s * s) * u
                wa, wb = 0.5 * (1.0 + z), 0.5 * (1.0 - z)
                for k, v in zip(out, (r * wa, r * wb, sig * (wa * wa), c * sig * (wa * wb), sig * (wb * wb), r, d, z, s, c)):
                    out[k].append(v)
    return {k: np.array(v) for k, v in out.items()}


def mirror_index(grid):
    """index of the point with the two channels exchanged (zeta -> -zeta, same rho, s, cos), for every grid point"""
    zeta = grid["zeta"]
    nz = len(zeta)
    per = 1 + (len(grid["s"]) - 1) * len(grid["cos"])
    n_rho = len(gold.rho_grid(grid)[0])
    idx = np.arange(n_rho * nz * per).reshape(n_rho, nz, per)
    return idx[:, [zeta.index(-z) for z in zeta], :].ravel()


def fixture_path(functional, quantity):
    return os.path.normpath(os.path.join(gold.GOLDEN, f"xc_spingga_mp_{functional}_{quantity}.json"))


def load_fixture(functional, quantity):
    import json
    with open(fixture_path(functional, quantity)) as fh:
        return json.load(fh)


# ------------------------------------------------------------------------------------------------ the functionals (mpmath)
def _pw92_mod_G(mp, rs, which):
    A, a1, b1, b2, b3, b4 = (mp.mpf(s) for s in PW92_MOD[which])
    return -2 * A * (1 + a1 * rs) * mp.log1p(1 / (2 * A * (b1 * mp.sqrt(rs) + b2 * rs + b3 * rs ** mp.mpf("1.5") + b4 * rs ** 2)))


def e_spin_gga_x_pbe(mp, up, dn, suu, sud, sdd):
    return (gold.e_gga_x_pbe(mp, 2 * up, 4 * suu) + gold.e_gga_x_pbe(mp, 2 * dn, 4 * sdd)) / 2


def e_spin_gga_c_pbe(mp, up, dn, suu, sud, sdd):
    beta, gamma = mp.mpf("0.06672455060314922"), (1 - mp.log(2)) / mp.pi ** 2
    rt = up + dn
    zeta, fz, rs = (up - dn) / rt, gold._fzeta(mp, up, dn), gold._rs(mp, rt)
    e0, e1, alpha_c = _pw92_mod_G(mp, rs, "eps0"), _pw92_mod_G(mp, rs, "eps1"), -_pw92_mod_G(mp, rs, "-alpha_c")
    eps = e0 + alpha_c * fz / mp.mpf(FZ20) * (1 - zeta ** 4) + (e1 - e0) * fz * zeta ** 4
    p = mp.mpf(2) / 3
    phi = ((1 + zeta) ** p + (1 - zeta) ** p) / 2
    kf = mp.cbrt(3 * mp.pi ** 2 * rt)
    t2 = mp.pi * (suu + 2 * sud + sdd) / (16 * phi ** 2 * kf * rt ** 2)
    A = beta / gamma / mp.expm1(-eps / (gamma * phi ** 3))
    H = gamma * phi ** 3 * mp.log1p(beta / gamma * (t2 + A * t2 ** 2) / (1 + A * t2 + A ** 2 * t2 ** 2))
    return rt * (eps + H)


E_SPIN_GGA = {"gga_x_pbe": e_spin_gga_x_pbe, "gga_c_pbe": e_spin_gga_c_pbe}


def ref_spin_gga(functional, up, dn, suu, sud, sdd):
    """{"e", "vup", "vdn", "vsuu", "vsud", "vsdd"} at one point (doubles), with the clamp and the threshold of the docstring"""
    mp = gold._mp()
    names = ("e", "vup", "vdn", "vsuu", "vsud", "vsdd")
    if up + dn <= 2 * SPIN_FLOOR:
        return dict.fromkeys(names, 0.0)
    fun = E_SPIN_GGA[functional]
    x0 = [max(up, SPIN_FLOOR), max(dn, SPIN_FLOOR), suu, sud, sdd]
    unit = float(gold.sigma_unit(up + dn))
    scales = [x0[0], x0[1]] + [max(abs(v), unit) for v in x0[2:]]

    def along(k):
        def f(x):
            args = [mp.mpf(v) for v in x0]
            args[k] = x
            return fun(mp, *args)
        return f
    out = {"e": float(gold._diff(mp, along(0), x0[0], 0, scales[0]))}
    for k, name in enumerate(names[1:]):
        out[name] = float(gold._diff(mp, along(k), x0[k], 1, scales[k]))
    return out


def check_identities(grid):
    """the two identities of the module docstring, at 50 digits, at every rho of the grid and s in {0, 1, 10}"""
    mp = gold._mp()
    tol = mp.mpf(10) ** -50
    rho, _ = gold.rho_grid(grid)
    for r in rho:
        r = mp.mpf(float(r))
        for s in (0.0, 1.0, 10.0):
            sig = mp.mpf(s * s) * (2 * mp.cbrt(3 * mp.pi ** 2 * r) * r) ** 2
            for fun in FUNCTIONALS:           # zeta = 0, grad rho_up = grad rho_down = grad rho / 2
                a = E_SPIN_GGA[fun](mp, r / 2, r / 2, sig / 4, sig / 4, sig / 4)
                b = gold.E_GGA[fun](mp, r, sig)
                assert abs(a - b) <= tol * abs(b), (fun, r, s)
            fl = mp.mpf(SPIN_FLOOR)           # zeta = +-1: the empty channel sits at the floor with no gradient
            want = gold.e_gga_x_pbe(mp, 2 * r, 4 * sig) / 2 + gold.e_gga_x_pbe(mp, 2 * fl, mp.mpf(0)) / 2
            for a in (e_spin_gga_x_pbe(mp, r, fl, sig, 0, 0), e_spin_gga_x_pbe(mp, fl, r, 0, 0, sig)):
                assert abs(a - want) <= tol * abs(want), (r, s)


def main():
    check_identities(GRID)
    head = {"generator": "tools/make_golden_xc_spin_gga.py", "mp_dps": gold.DPS}
    g = spin_gga_grid(GRID)
    for fun in FUNCTIONALS:
        rows = [ref_spin_gga(fun, *(float(g[k][i]) for k in ("up", "dn", "suu", "sud", "sdd"))) for i in range(len(g["up"]))]
        for q in QUANTITIES:
            path = fixture_path(fun, q)
            gold._dump(path, dict(head, family="spingga", functional=fun, grid=GRID), {q: [row[q] for row in rows]})
            assert os.path.getsize(path) <= MAX_BYTES


if __name__ == "__main__":
    sys.exit(main())
