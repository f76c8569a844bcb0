"""Double-precision NumPy restatement of the point-wise SCAN forms (mgga_x_scan, mgga_c_scan; Sun, Ruzsinszky, Perdew,
PRL 115, 036402 (2015)), unpolarised: e(rho, sigma, tau) per volume and its three first derivatives.

The derivatives are carried by a forward-mode dual number over arrays (a value and the slots d/d rho, d/d sigma, d/d tau), so
that what is written down is the energy density alone, as in tools/make_golden_xc.py.  This file is the CPU yardstick of
tests/test_mgga_reference.py: its own error against the 60-digit fixtures defines E_REF there.  It is a test helper, no
part of the package and none of the oracle.

Semantics: those of ``dftk_mi_xc_mgga``.  alpha = (tau - sigma / (8 rho)) / tau_unif without a clamp; the switching function
is 0 with zero slope at alpha = 1; g_x = 1 with zero derivatives where exp(-a1 / p^(1/4)) underflows (sigma = 0 included).
"""
import math

import numpy as np


class Dual:
    """value v and derivative slots d (3, n), every slot through the same operations"""

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def const(c, like):
        return Dual(np.full_like(like.v, c), np.zeros_like(like.d))

    @staticmethod
    def seed(x, slot):
        d = np.zeros((3, len(x)))
        d[slot] = 1.0
        return Dual(np.array(x, dtype=float), d)

    def _lift(self, o):
        return o if isinstance(o, Dual) else Dual.const(o, self)

    def __add__(self, o):
        o = self._lift(o)
        return Dual(self.v + o.v, self.d + o.d)

    __radd__ = __add__

    def __neg__(self):
        return Dual(-self.v, -self.d)

    def __sub__(self, o):
        o = self._lift(o)
        return Dual(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return self._lift(o) - self

    def __mul__(self, o):
        if not isinstance(o, Dual):
            return Dual(o * self.v, o * self.d)
        return Dual(self.v * o.v, self.d * o.v + self.v * o.d)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._lift(o)
        q = self.v / o.v
        return Dual(q, (self.d - q * o.d) / o.v)

    def __rtruediv__(self, o):
        return self._lift(o) / self

    def chain(self, f, df):
        return Dual(f, df * self.d)


def dsqrt(a):
    r = np.sqrt(a.v)
    return a.chain(r, 0.5 / r)


def dcbrt(a):
    r = np.cbrt(a.v)
    return a.chain(r, r / (3.0 * a.v))


def dexp(a):
    e = np.exp(a.v)
    return a.chain(e, e)


def dexpm1(a):
    e = np.expm1(a.v)
    return a.chain(e, e + 1.0)


def dlog1p(a):
    return a.chain(np.log1p(a.v), 1.0 / (1.0 + a.v))


def where(cond, a, b):
    return Dual(np.where(cond, a.v, b.v), np.where(cond[None, :], a.d, b.d))


def inv_root4(a):
    return 1.0 / dsqrt(dsqrt(a))


def pw92_mod(rs):
    A, a1, b1, b2, b3, b4 = 0.0310907, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294
    sq = dsqrt(rs)
    den = 2.0 * A * (b1 * sq + b2 * rs + b3 * (rs * sq) + b4 * (rs * rs))
    return (-2.0 * A) * ((1.0 + a1 * rs) * dlog1p(1.0 / den))


def switch(alpha, c1, c2, d):
    """exp(-c1 alpha / (1 - alpha)) below 1, -d exp(c2 / (1 - alpha)) above, 0 at 1; each branch is evaluated where it
    applies only (the other one overflows there)"""
    oma = 1.0 - alpha
    below, above = alpha.v < 1.0, alpha.v > 1.0
    safe = Dual(np.where(alpha.v == 1.0, 0.5, oma.v), oma.d)
    lo = dexp((-c1) * (alpha / safe))
    hi = (-d) * dexp(c2 / safe)
    lo = Dual(np.where(below, lo.v, 0.0), np.where(below[None, :], lo.d, 0.0))
    hi = Dual(np.where(above, hi.v, 0.0), np.where(above[None, :], hi.d, 0.0))
    return lo + hi


def two_product(a, b):
    """(p, e) with p = fl(a b) and a b = p + e exactly (Veltkamp splitting, Dekker's product): what one fma gives"""
    def split(x):
        c = 134217729.0 * x                      # 2^27 + 1
        hi = c - (c - x)
        return hi, x - hi
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def variables(rho, sigma, tau):
    kf = dcbrt(3.0 * math.pi ** 2 * rho)
    kf2r = kf * kf * rho
    p = sigma / (4.0 * (kf2r * rho))
    # tau - tau_W cancels (tau_W = 167 tau_unif at s = 10) under a switching function that is steep in alpha: the value of the
    # difference takes the rounding error of the quotient tau_W = sigma / (8 rho) back in, in float64 throughout (the
    # remainder sigma - tau_W 8 rho from an error-free product; the slots are those of the plain expression)
    num = tau - sigma / (8.0 * rho)
    r8 = 8.0 * rho.v
    tw = sigma.v / r8
    prod, err = two_product(tw, r8)
    num.v = (tau.v - tw) - ((sigma.v - prod) - err) / r8
    alpha = num / (0.3 * kf2r)
    return p, alpha


def e_x_scan(rho, sigma, tau):
    cx = -0.75 * (3.0 / math.pi) ** (1.0 / 3.0)
    k1, h0, a1, mu = 0.065, 1.174, 4.9479, 10.0 / 81.0
    b2 = math.sqrt(5913.0 / 405000.0)
    b1 = (511.0 / 13500.0) / (2.0 * b2)
    b3 = 0.5
    b4 = mu * mu / k1 - 1606.0 / 18225.0 - b1 * b1
    p, alpha = variables(rho, sigma, tau)
    oma = 1.0 - alpha
    w = b1 * p + b2 * (oma * dexp((-b3) * (oma * oma)))
    y = mu * p + b4 * ((p * p) * dexp((-b4 / mu) * p)) + w * w
    h1 = (1.0 + k1) - (k1 * k1) / (k1 + y)
    live = a1 / np.sqrt(np.sqrt(np.where(p.v > 0, p.v, 0.0))) <= 708.0
    p_safe = Dual(np.where(live, p.v, 1.0), p.d)
    gx = where(live, 1.0 - dexp((-a1) * inv_root4(p_safe)), Dual.const(1.0, p))
    fx = switch(alpha, 0.667, 0.8, 1.24)
    return cx * (rho * dcbrt(rho)) * ((h1 + fx * (h0 - h1)) * gx)


def e_c_scan(rho, sigma, tau):
    gamma = (1.0 - math.log(2.0)) / math.pi ** 2
    b1c, b2c, b3c, chi = 0.0285764, 0.0889, 0.125541, 0.12802585262625815
    p, alpha = variables(rho, sigma, tau)
    rs = dcbrt((3.0 / (4.0 * math.pi)) / rho)
    eps = pw92_mod(rs)
    beta = 0.066725 * ((1.0 + 0.1 * rs) / (1.0 + 0.1778 * rs))
    kf = dcbrt(3.0 * math.pi ** 2 * rho)
    t2 = (math.pi / 16.0) * (sigma / (kf * rho * rho))
    w1 = dexpm1((-1.0 / gamma) * eps)
    A = beta / (gamma * w1)
    eps1 = eps + gamma * dlog1p(w1 * (1.0 - inv_root4(1.0 + 4.0 * (A * t2))))
    e0 = (-b1c) / (1.0 + (b2c * dsqrt(rs) + b3c * rs))
    w0 = dexpm1((-1.0 / b1c) * e0)
    eps0 = e0 + b1c * dlog1p(w0 * (1.0 - inv_root4(1.0 + (4.0 * chi) * p)))
    fc = switch(alpha, 0.64, 1.5, 0.7)
    return rho * (eps1 + fc * (eps0 - eps1))


FORMS = {"mgga_x_scan": e_x_scan, "mgga_c_scan": e_c_scan}


def scan(functional, rho, sigma, tau):
    """{"e", "vrho", "vsigma", "vtau"} of one functional (or of "mgga_xc_scan", both) at arrays of points with rho > 0"""
    names = ("mgga_x_scan", "mgga_c_scan") if functional == "mgga_xc_scan" else (functional,)
    r, s, t = Dual.seed(rho, 0), Dual.seed(sigma, 1), Dual.seed(tau, 2)
    with np.errstate(all="ignore"):
        tot = FORMS[names[0]](r, s, t)
        for n in names[1:]:
            tot = tot + FORMS[n](r, s, t)
    return {"e": tot.v, "vrho": tot.d[0], "vsigma": tot.d[1], "vtau": tot.d[2]}
