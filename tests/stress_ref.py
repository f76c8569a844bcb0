"""Extended-precision references of the three entries of csrc/stress_kernels.hip, and the inputs of the tests that use them
(test_stress_reference.py on the host, test_gpu_stress_kernels.py at the C ABI).  Plain module, not collected.

Nothing here restates the kernels' hand-derived derivative formulas.  Every tensor is the derivative of an ENERGY
EXPRESSION on the strained lattice, as the reference's ForwardDiff pass takes it (src/postprocess/stresses.jl):

    q_eps = (I + eps)^-1 B (G + k),   Omega_eps = Omega det(I + eps),   eps = t / 2 (e_a e_b' + e_b e_a'),

coefficients, weights, structure factors (reduced coordinates) held fixed, d / dt at t = 0 in the Voigt order xx, yy, zz,
zy, zx, yx.  The derivative is taken twice, independently:

  * with dual numbers (``Dual``: a + b t, t^2 = 0) over ``np.longdouble`` arrays -- exact up to rounding, the VALUE;
  * with central differences of the same function at t = +-3.2e-2 ... +-2e-3 and a Richardson table of four extrapolation
    levels.  The ERROR ESTIMATE of an output is the larger of |dual - Richardson| and the difference of the last two levels.
    (Steps four times those first tried, 8e-3 ... 5e-4: the rounding of a central difference grows like eps / h and reached
    1e-15 S at h = 5e-4 on the two-row sphere; the truncation error of the larger steps is part of the estimate.)

All arithmetic is ``np.longdouble`` / ``np.clongdouble`` (64-bit mantissa here); constants come from longdouble arithmetic
(pi from a 35-digit string, square roots by ``np.sqrt`` of a longdouble), never from ``math``.  ``dtype=np.float64`` runs the
same code in double precision (the "room under the tolerance" check).  The forms are those of PspHgh.jl:110-124 (local),
PspHgh.jl:140-164 (projectors, divided by p^l) and spherical_harmonics.jl:31-66 (real solid harmonics); oracle/psp.py has the
same forms in float64 and serves as a cross-check (test_stress_reference.py), it cannot be reused: it casts to ``float``.

Every function also returns S, the sum of the ABSOLUTE values of the terms behind each output -- the scale of every
tolerance, so that cancellation in a sum cannot hide an error:
  kinetic   S_t = sum_G sum_n |w_n| |psi_n(G)|^2 |d (q_eps^2 / 2) / dt|
  nonlocal  S_t = 2 sum_n |w_n| sum_ij |p_i| |D_ij| |T_j|,   p = P' psi,  T = d (P_eps' psi) / dt  (the dual part)
  cube      S_t = sum_G sum_s |c_s(G) d ff_s / dt|,  sum_G |d (2 pi |rho|^2 / q_eps^2) / dt|;  energies: sum of |terms|
  xc        S   = sum_i |product_i|
"""
import math

import numpy as np
import scipy.fft as sfft

from oracle import psp as opsp
from oracle.terms import build_projection_coefficients_psp

LD = np.longdouble
_PI35 = "3.1415926535897932384626433832795029"
VOIGT = ((0, 0), (1, 1), (2, 2), (2, 1), (2, 0), (1, 0))
H0, LEVELS = 3.2e-2, 4                                  # Richardson: h = H0 / 2^k, k = 0 .. LEVELS


# ------------------------------------------------------------------------------------------ dual numbers
class Dual:
    """a + b t with t^2 = 0; a and b are arrays (or scalars) of one dtype, real or complex."""
    __slots__ = ("a", "b")
    __array_ufunc__ = None                              # ndarray (op) Dual defers to the reflected method below

    def __init__(self, a, b):
        self.a, self.b = a, b

    def __add__(self, o):
        return Dual(self.a + o.a, self.b + o.b) if isinstance(o, Dual) else Dual(self.a + o, self.b)
    __radd__ = __add__

    def __neg__(self):
        return Dual(-self.a, -self.b)

    def __sub__(self, o):
        return self + (-o)

    def __rsub__(self, o):
        return (-self) + o

    def __mul__(self, o):
        if isinstance(o, Dual):
            return Dual(self.a * o.a, self.a * o.b + self.b * o.a)
        return Dual(self.a * o, self.b * o)
    __rmul__ = __mul__

    def __truediv__(self, o):
        if isinstance(o, Dual):
            return Dual(self.a / o.a, (self.b * o.a - self.a * o.b) / (o.a * o.a))
        return Dual(self.a / o, self.b / o)

    def __rtruediv__(self, o):
        return Dual(o / self.a, -(o * self.b) / (self.a * self.a))


def _lin(fn, x):
    """a linear map applied to both parts"""
    return Dual(fn(x.a), fn(x.b)) if isinstance(x, Dual) else fn(x)


def _exp(x):
    if isinstance(x, Dual):
        e = np.exp(x.a)
        return Dual(e, e * x.b)
    return np.exp(x)


def _sqrt(x):
    if isinstance(x, Dual):
        s = np.sqrt(x.a)
        return Dual(s, x.b / (s + s))
    return np.sqrt(x)


def _val(x):
    return x.a if isinstance(x, Dual) else x


# ------------------------------------------------------------------------------------------ constants, strain
class Consts:
    def __init__(self, dtype):
        self.dt = dtype
        self.cdt = np.result_type(dtype, np.complex64)
        self.pi = dtype(LD(_PI35))
        self.sqrt_pi = np.sqrt(self.pi)
        self.pi54 = self.pi * np.sqrt(self.sqrt_pi)          # pi^(5/4)
        self.half = dtype(1) / dtype(2)

    def num(self, x):
        return self.dt(x)

    def sqrt(self, x):
        return np.sqrt(self.dt(x))

    def arr(self, x):
        return np.asarray(x, dtype=np.float64).astype(self.dt)


def _strain(c, t, a, b):
    """I + t / 2 (e_a e_b' + e_b e_a'); t a number of the dtype or the dual unit"""
    A = [[c.num(1) if i == j else c.num(0) for j in range(3)] for i in range(3)]
    h = t * c.half
    A[a][b] = A[a][b] + h
    A[b][a] = A[b][a] + h
    return A


def _inv3(A):
    def cof(i, j):
        return (A[(i + 1) % 3][(j + 1) % 3] * A[(i + 2) % 3][(j + 2) % 3]
                - A[(i + 1) % 3][(j + 2) % 3] * A[(i + 2) % 3][(j + 1) % 3])
    det = A[0][0] * cof(0, 0) + A[0][1] * cof(0, 1) + A[0][2] * cof(0, 2)
    return [[cof(j, i) / det for j in range(3)] for i in range(3)], det


def _strained_q(c, A, q0):
    """q_eps = (I + eps)^-1 q0 as three columns, and det(I + eps)"""
    Ai, det = _inv3(A)
    return [Ai[i][0] * q0[:, 0] + Ai[i][1] * q0[:, 1] + Ai[i][2] * q0[:, 2] for i in range(3)], det


def _richardson(f, c):
    """d f(t) / dt at 0 by central differences and LEVELS extrapolations; (value, |last level - the one before|)"""
    T = []
    for k in range(LEVELS + 1):
        h = c.num(H0) / c.num(2 ** k)
        row = [(f(h) - f(-h)) / (h + h)]
        for j in range(1, k + 1):
            row.append(row[j - 1] + (row[j - 1] - T[k - 1][j - 1]) / c.num(4 ** j - 1))
        T.append(row)
    return T[-1][-1], np.abs(T[-1][-1] - T[-1][-2])


def _derivatives(c, energies, n_out, estimate):
    """``energies(A)`` -> list of n_out scalars (numbers or Dual).  Returns the (6, n_out) derivatives by dual numbers and
    their error estimates against the Richardson table (zeros when ``estimate`` is off)."""
    val = np.zeros((6, n_out), dtype=c.dt)
    err = np.zeros((6, n_out), dtype=c.dt)
    for t, (a, b) in enumerate(VOIGT):
        val[t] = [x.b for x in energies(_strain(c, Dual(c.num(0), c.num(1)), a, b))]
        if estimate:
            r, e = _richardson(lambda h: np.array(energies(_strain(c, h, a, b)), dtype=c.dt), c)
            err[t] = np.maximum(e, np.abs(r - val[t]))
    return val, err


# ------------------------------------------------------------------------------------------ HGH forms
def _radial(c, l, i, rp, t2):
    """eval_psp_projector_fourier divided by p^l (PspHgh.jl:140-164), t2 = (p r_l)^2"""
    common = c.num(4) * c.pi54 * np.sqrt(c.num(2 ** (l + 1)) * rp * rp * rp) * _exp(t2 * (-c.half))
    n = c.num
    if (l, i) == (0, 1):
        return common
    if (l, i) == (0, 2):
        return common * (n(2) / c.sqrt(15)) * (n(3) - t2)
    if (l, i) == (0, 3):
        return common * (n(4) / (n(3) * c.sqrt(105))) * (n(15) - n(10) * t2 + t2 * t2)
    if (l, i) == (1, 1):
        return common * (rp / c.sqrt(3))
    if (l, i) == (1, 2):
        return common * (n(2) * rp / c.sqrt(105)) * (n(5) - t2)
    if (l, i) == (1, 3):
        return common * (n(4) * rp / (n(3) * c.sqrt(1155))) * (n(35) - n(14) * t2 + t2 * t2)
    if (l, i) == (2, 1):
        return common * (rp * rp / c.sqrt(15))
    if (l, i) == (2, 2):
        return common * (n(2) * rp * rp / (n(3) * c.sqrt(105))) * (n(7) - t2)
    if (l, i) == (3, 1):
        return common * (rp * rp * rp / c.sqrt(105))
    raise NotImplementedError((l, i))


def _solid(c, l, m, x, y, z):
    """r^l Y_lm, real form (spherical_harmonics.jl:31-66)"""
    n = c.num

    def k(num, den):                                     # sqrt(num / (den pi))
        return np.sqrt(n(num) / (n(den) * c.pi))
    if l == 0:
        return k(1, 4) + x * n(0)
    if l == 1:
        return k(3, 4) * {-1: y, 0: z, 1: x}[m]
    if l == 2:
        return {-2: lambda: k(15, 4) * (x * y), -1: lambda: k(15, 4) * (y * z),
                0: lambda: k(5, 16) * (n(2) * z * z - x * x - y * y), 1: lambda: k(15, 4) * (x * z),
                2: lambda: k(15, 16) * (x * x - y * y)}[m]()
    if l == 3:
        return {-3: lambda: k(35, 32) * ((n(3) * x * x - y * y) * y), -2: lambda: k(105, 4) * (x * y * z),
                -1: lambda: k(21, 32) * (y * (n(4) * z * z - x * x - y * y)),
                0: lambda: k(7, 16) * (z * (n(2) * z * z - n(3) * x * x - n(3) * y * y)),
                1: lambda: k(21, 32) * (x * (n(4) * z * z - x * x - y * y)), 2: lambda: k(105, 16) * ((x * x - y * y) * z),
                3: lambda: k(35, 32) * ((x * x - n(3) * y * y) * x)}[m]()
    raise NotImplementedError((l, m))


def _local_ff(c, psp, t2):
    """eval_psp_local_fourier (PspHgh.jl:110-124), t2 = (p rloc)^2 > 0, all four c_i"""
    n = c.num
    rloc, Z = n(psp.rloc), n(psp.Zion)
    cl = [n(v) for v in psp.cloc]
    t4 = t2 * t2
    P = (cl[0] + cl[1] * (n(3) - t2) + cl[2] * (n(15) - n(10) * t2 + t4)
         + cl[3] * (n(105) - n(105) * t2 + n(21) * t4 - t4 * t2))
    return (n(4) * c.pi * rloc * rloc) * ((t2 * P) * (np.sqrt(c.pi / n(2)) * rloc) - Z) * _exp(t2 * (-c.half)) / t2


def _phase(c, p, r):
    """exp(-2 pi i p . r); p: (n, 3) of the dtype, r: three float64 numbers"""
    arg = p[:, 0] * c.num(r[0]) + p[:, 1] * c.num(r[1]) + p[:, 2] * c.num(r[2])
    arg = (arg - np.round(arg)) * (c.num(2) * c.pi)
    return (np.cos(arg) - 1j * np.sin(arg)).astype(c.cdt)


def projector_columns(psp):
    """(l, m, i) of one atom's columns, i fastest (nonlocal.jl:205-244, list_projector_columns)"""
    return [(l, m, i) for l in range(psp.lmax + 1) for m in range(-l, l + 1)
            for i in range(1, psp.count_n_proj_radial(l) + 1)]


# ------------------------------------------------------------------------------------------ kinetic + nonlocal
def pair_rows(G):
    """rows (g, mg) of one representative per {G, -G} of an inversion-symmetric sphere, first occurrence, G = 0 first"""
    row = {tuple(v): i for i, v in enumerate(np.asarray(G).tolist())}
    partner = np.array([row[tuple(-x for x in v)] for v in np.asarray(G).tolist()])
    g = np.nonzero(partner >= np.arange(len(partner)))[0]
    assert tuple(np.asarray(G)[g[0]]) == (0, 0, 0)
    return g, partner[g]


def kinetic_nonlocal(recip, vol, kpt, G, psi, w, atoms, dtype=LD, estimate=True, bra_fixed=False, half=None,
                     ket_l_shift=0):
    """Reference of dftk_mi_stress_kinetic_nonlocal.  recip: (3, 3) float64 reciprocal lattice (q = recip @ (G + k)),
    G: (n_G, 3) integers, psi: (n_G, nb) complex128, w: (nb,), atoms: [(psp, reduced position)] in column order.

    Returns dict(value, S, err: (12,) -- kinetic 0..5, nonlocal 6..11; E: (kinetic, nonlocal) at eps = 0, the energies when
    none of the options below is set).

    ``bra_fixed``: the nonlocal function is 2 Re sum w (P_0' psi)' D (P_eps' psi) -- the same derivative (D is symmetric), but
    an alteration of the strained projector alone does not cancel.  The three alterations below act on that projector:
    ``half``: None, or the rule of the half format for an inversion-symmetric sphere and real-symmetric psi -- "rule" sums
    over one row per pair with the weights 1 (row 0, real part) and sqrt 2, "no_sqrt2" leaves the sqrt 2 out, "no_row0"
    treats row 0 like every other row; ``ket_l_shift``: (-i)^(l + shift) for l >= 2."""
    c = Consts(dtype)
    n_G, nb = psi.shape
    B = c.arr(recip)
    p = np.asarray(G, dtype=np.float64).astype(dtype) + c.arr(kpt)[None, :]
    q0 = np.stack([p[:, 0] * B[i, 0] + p[:, 1] * B[i, 1] + p[:, 2] * B[i, 2] for i in range(3)], axis=1)
    psi_x = np.asarray(psi).astype(c.cdt)
    w_x = c.arr(w)
    dens = (np.abs(psi_x) ** 2) @ w_x                                   # sum_n w_n |psi_n(G)|^2
    dens_abs = (np.abs(psi_x) ** 2) @ np.abs(w_x)
    inv_sqrt_vol = c.num(1) / np.sqrt(c.num(vol))
    species = []                                                         # distinct psps in order of appearance
    for psp, _ in atoms:
        if not any(psp is s for s in species):
            species.append(psp)
    phases = [_phase(c, p, r) for _, r in atoms]
    Ds = [c.arr(build_projection_coefficients_psp(psp)) for psp, _ in atoms]
    if half is not None:
        g, mg = pair_rows(G)
        s2 = c.sqrt(2)
        psi_h = (psi_x[g] + np.conj(psi_x[mg])) / c.num(2) * s2           # the half format of psi (to_half)
        psi_h[0] = psi_x[g[0]].real
        scale = np.full(len(g), s2, dtype=dtype)
        if half != "no_row0":
            scale[0] = c.num(1)
        if half == "no_sqrt2":
            scale[:] = c.num(1)

    def project(F, ls, ph, altered):
        """(n_G, nc) real amplitudes, l per column, the atom's phase -> (nc, nb) projections P' psi"""
        shift = np.where(ls >= 2, ket_l_shift, 0) if altered else 0
        U = ph[:, None] * np.array([1, -1j, -1, 1j], dtype=c.cdt)[(ls + shift) % 4][None, :]   # (-i)^l e^{-2 pi i (G + k) r}
        P = U * F
        if half is None or not altered:
            return np.conj(P).T @ psi_x
        Ph = P[g] * scale[:, None]
        if half != "no_row0":
            Ph[0] = Ph[0].real
        return (Ph.real.T @ psi_h.real + Ph.imag.T @ psi_h.imag).astype(c.cdt)

    def projections(A, altered):
        """P_eps' psi per atom, each (nc, nb), numbers or Dual; ``altered``: with ``half`` and ``ket_l_shift``"""
        q, det = _strained_q(c, A, q0)
        q2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
        norm = inv_sqrt_vol / _sqrt(det)
        forms = []
        for psp in species:
            cols = projector_columns(psp)
            f = [_radial(c, l, i, c.num(psp.rp[l]), q2 * (c.num(psp.rp[l]) * c.num(psp.rp[l])))
                 * _solid(c, l, m, q[0], q[1], q[2]) * norm for l, m, i in cols]
            forms.append((np.array([l for l, _, _ in cols]), f))
        out = []
        for (psp, _), ph in zip(atoms, phases):
            ls, f = forms[[s is psp for s in species].index(True)]
            Fa = np.stack([_val(x) for x in f], axis=1)
            if isinstance(f[0], Dual):
                Fb = np.stack([x.b for x in f], axis=1)
                out.append(Dual(project(Fa, ls, ph, altered), project(Fb, ls, ph, altered)))
            else:
                out.append(project(Fa, ls, ph, altered))
        return q2, out

    assert bra_fixed or (half is None and ket_l_shift == 0)
    ident = _strain(c, c.num(0), 0, 0)
    _, p0 = projections(ident, False)

    def energies(A):
        q2, pk = projections(A, True)
        e_kin = _lin(lambda x: (x * dens).sum(), q2 * c.half)
        e_nl = c.num(0)
        for a, D in enumerate(Ds):
            prod = _lin(np.conj, p0[a] if bra_fixed else pk[a]) * _lin(lambda x: D @ x, pk[a])
            e = _lin(lambda x: (x.real @ w_x).sum(), prod)
            e_nl = e_nl + (e + e if bra_fixed else e)
        return [e_kin, e_nl]

    val, err = _derivatives(c, energies, 2, estimate)
    # S: the absolute sums, from the dual parts of the UNALTERED function
    S = np.zeros((6, 2), dtype=dtype)
    for t, (a, b) in enumerate(VOIGT):
        q2, pk = projections(_strain(c, Dual(c.num(0), c.num(1)), a, b), False)
        S[t, 0] = (np.abs(q2.b * c.half) * dens_abs).sum()
        for a_i, D in enumerate(Ds):
            S[t, 1] += c.num(2) * ((np.abs(pk[a_i].a) * (np.abs(D) @ np.abs(pk[a_i].b))) @ np.abs(w_x)).sum()
    e0 = energies(ident)
    return dict(value=np.concatenate([val[:, 0], val[:, 1]]), S=np.concatenate([S[:, 0], S[:, 1]]),
                err=np.concatenate([err[:, 0], err[:, 1]]), E=(e0[0], e0[1]))


# ------------------------------------------------------------------------------------------ cube terms
def signed_freq(n):
    """G_axis(n) (src/fft.jl:24-31)"""
    i = np.arange(n)
    return np.where(i <= (n - 1) // 2, i, i - n)


def cube(recip, vol, fft_size, rho, groups, dtype=LD, estimate=True, keep_nyquist=False, keep_g0=False):
    """Reference of dftk_mi_stress_cube.  rho: (nz, ny, nx) float64 total density, groups: [(psp, [reduced positions])] in
    species-group order.  rho(G) = DFT(rho) sqrt(Omega) / N in the dtype; c_s(G) = Re[conj rho(G) S_s(G)] / sqrt(Omega) fixed;
    F(eps) = sum_G sum_s c_s ff_s(|q_eps|), H(eps) = 1/2 sum_G 4 pi |rho(G)|^2 / |q_eps|^2; G = 0 and the unpaired Nyquist
    entries left out unless ``keep_g0`` / ``keep_nyquist``.  Returns dict(value, S, err: (14,)) in the entry's order: dF (6),
    dH (6), F(0), H(0)."""
    c = Consts(dtype)
    nx, ny, nz = fft_size
    rho_G = sfft.fftn(np.asarray(rho, dtype=np.float64).reshape(nz, ny, nx).astype(dtype))
    assert rho_G.dtype == c.cdt, rho_G.dtype                          # the transform ran in the dtype, not in double
    rho_G = rho_G * (np.sqrt(c.num(vol)) / c.num(nx * ny * nz))
    fz, fy, fx = np.meshgrid(signed_freq(nz), signed_freq(ny), signed_freq(nx), indexing="ij")
    keep = np.ones((nz, ny, nx), dtype=bool)
    if not keep_nyquist:
        for n, f in ((nx, fx), (ny, fy), (nz, fz)):
            if n % 2 == 0:
                keep &= f != -(n // 2)
    if not keep_g0:
        keep[0, 0, 0] = False
    p = np.stack([fx[keep], fy[keep], fz[keep]], axis=1).astype(np.float64).astype(dtype)
    rg = rho_G[keep]
    B = c.arr(recip)
    q0 = np.stack([p[:, 0] * B[i, 0] + p[:, 1] * B[i, 1] + p[:, 2] * B[i, 2] for i in range(3)], axis=1)
    inv_sqrt_vol = c.num(1) / np.sqrt(c.num(vol))
    cs = []
    for _, positions in groups:
        S_s = sum(_phase(c, p, r) for r in positions)
        cs.append((np.conj(rg) * S_s).real * inv_sqrt_vol)
    hart = (c.num(2) * c.pi) * (rg.real * rg.real + rg.imag * rg.imag)

    def terms(A):
        q, _ = _strained_q(c, A, q0)
        q2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2]
        f = [cs_s * _local_ff(c, psp, q2 * (c.num(psp.rloc) * c.num(psp.rloc))) for cs_s, (psp, _) in zip(cs, groups)]
        return f, hart / q2

    def energies(A):
        f, h = terms(A)
        F = (A[0][0] + A[1][1] + A[2][2] + A[2][1] + A[2][0] + A[1][0]) * c.num(0)      # zero, dual when A is
        for f_s in f:
            F = F + _lin(np.sum, f_s)
        return [F, _lin(np.sum, h)]

    with np.errstate(all="ignore" if keep_g0 else "warn"):
        val, err = _derivatives(c, energies, 2, estimate)
        S = np.zeros((6, 2), dtype=dtype)
        for t, (a, b) in enumerate(VOIGT):
            f, h = terms(_strain(c, Dual(c.num(0), c.num(1)), a, b))
            S[t, 0] = sum(np.abs(f_s.b).sum() for f_s in f)
            S[t, 1] = np.abs(h.b).sum()
        f, h = terms(_strain(c, c.num(0), 0, 0))
    e = [sum((f_s.sum() for f_s in f), c.num(0)), h.sum()]
    Se = [sum((np.abs(f_s).sum() for f_s in f), c.num(0)), np.abs(h).sum()]
    return dict(value=np.concatenate([val[:, 0], val[:, 1], e]).astype(dtype),
                S=np.concatenate([S[:, 0], S[:, 1], Se]).astype(dtype),
                err=np.concatenate([err[:, 0], err[:, 1], [0, 0]]).astype(dtype))


# ------------------------------------------------------------------------------------------ exchange-correlation
def _exact_sum(P):
    """math.fsum of longdouble products: each is split into a double and the double of the rest, the sum of those is exact"""
    hi = P.astype(np.float64)
    lo = (P - hi.astype(LD)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


def xc(n_spin, rho, vrho, e=None, vsigma=None, grad=None):
    """Reference of dftk_mi_stress_xc: (value, S), each (8,) float64.  rho / vrho: (n_spin, n), grad: (3, n)."""
    rho, vrho = np.asarray(rho, dtype=LD).reshape(n_spin, -1), np.asarray(vrho, dtype=LD).reshape(n_spin, -1)
    value, S = np.zeros(8), np.zeros(8)
    if e is not None:
        value[0], S[0] = _exact_sum(np.asarray(e, dtype=LD)), _exact_sum(np.abs(np.asarray(e, dtype=LD)))
    prod = (rho * vrho).reshape(-1)
    value[1], S[1] = _exact_sum(prod), _exact_sum(np.abs(prod))
    if vsigma is not None:
        vs, g = np.asarray(vsigma, dtype=LD), np.asarray(grad, dtype=LD).reshape(3, -1)
        for t, (a, b) in enumerate(VOIGT):
            prod = vs * g[a] * g[b]
            value[2 + t], S[2 + t] = _exact_sum(prod), _exact_sum(np.abs(prod))
    return value, S


# ------------------------------------------------------------------------------------------ the inputs of the tests
# the sheared lattice, the k-point and the positions of test_gpu_multispecies.py
LATTICE = np.array([[7.4, 0.9, -0.6], [0.4, 6.9, 1.1], [-0.7, 0.5, 7.8]])
KPT = np.array([0.23, -0.31, 0.17])
POS = {"Si": [0.02, 0.03, 0.05], "X1": [0.27, 0.21, 0.09], "Fe": [0.77, 0.69, 0.33], "X2": [0.69, 0.31, 0.86]}
NL_FFT, NL_ECUT = (15, 16, 18), 10.0                 # the cube only decodes G; the Ecut sphere holds > 513 rows
NG_COMPLEX = (1, 255, 256, 257, 513)
NHALF_GAMMA = (1, 2, 128, 129, 257)
NBANDS = (1, 3, 6)
WEIGHTS = np.array([0.9, 0.0, 1.3, 0.25, 2.0, 0.6])   # (one weight exactly 0 from three bands on)
CUBES = [(5, 5, 5), (7, 8, 9), (16, 16, 16), (15, 16, 18), (12, 9, 10), (41, 40, 42)]
ATOM_SETS = ("none", "one", "three")
XC_N = (1, 255, 256, 257, 262144, 262145, 524288 + 77)
XC_VARIANTS = ("lda", "gga", "spin")


def cube_id(fft_size):
    return "x".join(str(n) for n in fft_size)


def lattice_tables():
    from oracle.basis import compute_recip_lattice, compute_unit_cell_volume
    return compute_recip_lattice(LATTICE), float(compute_unit_cell_volume(LATTICE))


_PSPS = {}


def psps():
    """X: the synthetic species with every tabulated channel and all four c_i (test_hgh_channels.py); Fe: empty cloc"""
    if not _PSPS:
        from test_hgh_channels import synthetic_oracle_psp
        _PSPS.update(X=synthetic_oracle_psp(), Fe=opsp.load_psp_hgh("Fe", "lda"), Si=opsp.load_psp_hgh("Si", "lda"))
    return _PSPS


def nonlocal_atoms():
    """[(psp, position)] in group order: X twice (29 columns each), Fe (14), Si (5)"""
    s = psps()
    return [(s["X"], POS["X1"]), (s["X"], POS["X2"]), (s["Fe"], POS["Fe"]), (s["Si"], POS["Si"])]


def cube_groups(name):
    s = psps()
    return {"none": [], "one": [(s["X"], [POS["X1"]])],
            "three": [(s["X"], [POS["X1"], POS["X2"]]), (s["Fe"], [POS["Fe"]]), (s["Si"], [POS["Si"]])]}[name]


def _ecut_sphere(kpt):
    recip, _ = lattice_tables()
    nx, ny, nz = NL_FFT
    fz, fy, fx = np.meshgrid(signed_freq(nz), signed_freq(ny), signed_freq(nx), indexing="ij")
    G = np.stack([fx.ravel(), fy.ravel(), fz.ravel()], axis=1)
    q = (G + np.asarray(kpt)[None, :]) @ recip.T
    mapping = np.nonzero(0.5 * np.sum(q * q, axis=1) <= NL_ECUT)[0]
    assert all(np.abs(G[mapping][:, d]).max() <= (NL_FFT[d] - 1) // 2 for d in range(3))     # the sphere fits the cube
    return mapping, G[mapping]


def complex_sphere(n_G):
    """(mapping, G): n_G rows of the Ecut sphere at KPT, in ascending mapping order"""
    mapping, G = _ecut_sphere(KPT)
    rows = np.sort(np.random.default_rng(100 + n_G).choice(len(mapping), n_G, replace=False))
    return mapping[rows], G[rows]


def gamma_sphere(n_half):
    """(mapping, G): G = 0 and n_half - 1 pairs {G, -G} of the Ecut sphere at Gamma, in ascending mapping order"""
    mapping, G = _ecut_sphere(np.zeros(3))
    g, mg = pair_rows(G)
    pick = np.random.default_rng(200 + n_half).choice(np.arange(1, len(g)), n_half - 1, replace=False)
    rows = np.sort(np.concatenate([g[:1], g[pick], mg[pick]]))
    return mapping[rows], G[rows]


def orbitals(G, nb, gamma):
    """(n_G, nb) random orbitals; ``gamma``: real-symmetric columns built from a random half (from_half)"""
    rng = np.random.default_rng(300 + 10 * len(G) + nb)
    if not gamma:
        return rng.standard_normal((len(G), nb)) + 1j * rng.standard_normal((len(G), nb))
    g, mg = pair_rows(G)
    h = rng.standard_normal((len(g), nb)) + 1j * rng.standard_normal((len(g), nb))
    x = np.zeros((len(G), nb), dtype=complex)
    x[g] = h / np.sqrt(2.0)
    x[mg] = np.conj(h) / np.sqrt(2.0)
    x[g[0]] = h[0].real
    return x


_CACHE = {}


def nonlocal_case(n, nb, gamma, **kw):
    """(mapping, G, psi, w, reference) of one case of the GPU file; references are computed once per process"""
    key = (n, nb, gamma, tuple(sorted(kw.items())))
    if key not in _CACHE:
        mapping, G = gamma_sphere(n) if gamma else complex_sphere(n)
        psi = orbitals(G, nb, gamma)
        w = WEIGHTS[:nb].copy()
        recip, vol = lattice_tables()
        ref = kinetic_nonlocal(recip, vol, np.zeros(3) if gamma else KPT, G, psi, w, nonlocal_atoms(), **kw)
        _CACHE[key] = (mapping, G, psi, w, ref)
    return _CACHE[key]


def density(fft_size):
    """(nz, ny, nx): a positive random field, a large constant, and cos(pi i) on every even axis (a large Nyquist amplitude)"""
    nx, ny, nz = fft_size
    # (the seed is one at which no component of a tensor happens to cancel below 1e-3 S, test_stress_reference.py)
    rho = 1.0 + 0.1 * np.random.default_rng(1000 + sum(fft_size)).random((nz, ny, nx))
    for axis, n in ((2, nx), (1, ny), (0, nz)):
        if n % 2 == 0:
            shape = [1, 1, 1]
            shape[axis] = n
            rho = rho + 0.3 * np.cos(np.pi * np.arange(n)).reshape(shape)
    return rho


def cube_case(fft_size, atom_set, **kw):
    key = (tuple(fft_size), atom_set, tuple(sorted(kw.items())))
    if key not in _CACHE:
        recip, vol = lattice_tables()
        rho = density(fft_size)
        _CACHE[key] = (rho, cube(recip, vol, fft_size, rho, cube_groups(atom_set), **kw))
    return _CACHE[key]


def xc_inputs(n, variant):
    """dict(n_spin, rho, vrho, e, vsigma, grad) of signed random numbers"""
    rng = np.random.default_rng(n % 100003 + len(variant))
    n_spin = 2 if variant == "spin" else 1
    d = dict(n_spin=n_spin, rho=rng.standard_normal((n_spin, n)), vrho=rng.standard_normal((n_spin, n)), e=None,
             vsigma=None, grad=None)
    if variant == "gga":
        d.update(e=rng.standard_normal(n), vsigma=rng.standard_normal(n), grad=rng.standard_normal((3, n)))
    return d
