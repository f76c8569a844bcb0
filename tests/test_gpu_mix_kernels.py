"""``csrc/mix_kernels.hip`` at the C ABI: ``dftk_mi_step_sums``, the Anderson accumulator (``dftk_mi_anderson_*``) and
``dftk_mi_chi0_mix``, plus the four Fourier-multiplier entries of ``cube_kernels.hip``, against references written HERE in
NumPy / mpmath from the formulas of the reference project (anderson.jl:81-130, mixing.jl:61-72,161-171,261-290,
chi0models.jl:21-77, hartree.jl:68-81).  No reference calls the library, the torch twins or ``oracle/``.

A. Reductions.  mpmath sums at 50 digits; |sum - ref| <= (ceil(n / 32768) + 15) eps sum|terms|: the first term is the serial
   chain of one thread of the 128 x 256 grid, the 15 covers the wave tree, the block sum and the host sum of 128 partials.

B. Anderson is a pure function of the (x, Pf) pairs it was fed, so the pairs are PRESCRIBED (no fixed-point iteration): every
   drop decision sits far from its threshold (the reference asserts the distance) and cond(M) is the reference's own.  The
   reference keeps its own history lists in ``np.longdouble``.  Up to 6 columns (every case with a drop) it forms M, M'M and
   M'Pf in ``np.longdouble`` and solves the normal equations with mpmath at 50 digits through the eigen-decomposition
   (minimum-norm solution; cond(M) from the square roots of the eigenvalues).  mpmath needs 0.3 s and more per 31 x 31
   problem and a long-double M'M 25 ms, so longer histories keep <r_i, r_j> in ``np.longdouble`` from step to step and
   take a float64 solve with four refinements whose residuals are ``np.longdouble``, cond(M) from the float64 eigenvalues
   of M'M (relative error cond(M)^2 eps); one more step of such a run goes down both paths, which must agree to 1e-17.
   Accelerated step: |xn_gpu - xn_ref| <= 64 kappa^2 eps S, kappa = cond(M) after the drops,
   S = sum_k |beta_k| |x_k + alpha r_k| + |1 - sum beta| |x + alpha Pf| (kappa^2: the library solves through the Gram
   matrix; 64: margin over the 31-term sums).  kappa and the achieved ratio are printed (``pytest -s``).

C. ``dftk_mi_chi0_mix`` against the DENSE operator (<= 240 x 240) on the cubes 6 x 5 x 4 and 5 x 3 x 7 of a sheared
   fcc x (2, 1, 1) cell, assembled column by column from NumPy FFTs, x -> C (x - chi0 (vc sum_comp x - mean)); the solution
   from a dense least-squares solve refined once in ``np.longdouble``; sigma_max / sigma_min from the SVD on the zero-mean
   subspace.  With tol = max(1e-12, reltol |b|), b = dF - mean, for every solve that reports convergence:
   |b - A (x_gpu - dc)| <= tol + delta, delta = (steps + 1) Nt eps (sigma_max |x| + |b|) (the rounding gap between the
   Givens estimate and the true residual), |x_gpu - x_ref| <= (tol + delta) / sigma_min, |mean x_gpu - mean dF| <=
   4 eps max|dF|, and n_applies within 1 of the applications of a plain NumPy GMRES (modified Gram-Schmidt twice, one
   true residual per cycle).  Every branch-named case first asserts from that NumPy GMRES that its inputs reach the branch.

D. The multiplier entries: |out - ref| <= 64 eps max|m| |x|; Kerker and the dielectric mixing keep the mean.

DESIGN.md section 3.9.1 records the printed figures.
"""
import ctypes as C
import math

import mpmath as mp
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check as abi_check  # noqa: E402

from test_gpu_kernels import Basis, KBlock, dev  # noqa: E402

EPS = 2.220446049250313e-16
EINVAL = -1               # DFTK_MI_EINVAL (include/dftk_mi355x.h)
NONFINITE = 1             # DFTK_MI_NUM_NONFINITE
NAN = float("nan")
LD = np.longdouble
mp.mp.dps = 50


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs8(lib):
    return Basis(lib, 8, 8, 8)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _norm(v):
    v = np.asarray(v, dtype=LD).reshape(-1)
    return float(np.sqrt(v @ v))


def _mpf(v):
    """an ``np.longdouble`` as an mpf, exactly"""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(LD(v) - LD(hi)))


# ======================================================================================= A. dftk_mi_step_sums
def step_sums(lib, bs, n, a, b, c, handle=True):
    out = (C.c_double * 2)(NAN, NAN)
    st = lib.dftk_mi_step_sums(bs.h if handle else None, n, _ptr(a), _ptr(b), _ptr(c), out)
    return st, out[0], out[1]


@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 32767, 32768, 32769, 100003])
def test_step_sums_against_mpmath(lib, bs8, n):
    """Cancellation matters: a, b = 1e3 + unit noise (sum|a b| ~ 1e6 n), c = a + 1e-6 noise (the differences are 1e-9 of the
    operands).  n below, at and above one wave, one block and the whole 128 x 256 grid (idle blocks, loops that wrap), and a
    prime."""
    rng = np.random.default_rng(1000 + n)
    a = 1e3 + rng.standard_normal(n)
    b = 1e3 + rng.standard_normal(n)
    c = a + 1e-6 * rng.standard_normal(n)
    st, s0, s1 = step_sums(lib, bs8, n, dev(a), dev(b), dev(c))
    assert st == 0
    ref0 = mp.fdot(a.tolist(), b.tolist())
    ref1 = mp.fsum([mp.mpf(x) - mp.mpf(y) for x, y in zip(a.tolist(), c.tolist())], squared=True)
    abs0 = mp.fdot(np.abs(a).tolist(), np.abs(b).tolist())
    k = math.ceil(n / 32768) + 15
    e0, e1 = float(abs(mp.mpf(s0) - ref0)), float(abs(mp.mpf(s1) - ref1))
    print(f"\nstep_sums n={n}: err/(eps sum|ab|) = {e0 / (EPS * float(abs0)):.2f}, err/(eps sum d^2) = "
          f"{e1 / (EPS * float(ref1)):.2f}, allowed {k}")
    assert e0 <= k * EPS * float(abs0)
    assert e1 <= k * EPS * float(ref1)


def test_step_sums_argument_checks(lib, bs8):
    rng = np.random.default_rng(5)
    a, b, c = (dev(1e3 + rng.standard_normal(257)) for _ in range(3))
    st, s0, s1 = step_sums(lib, bs8, 257, a, None, c)
    assert st == 0 and s0 == 0.0 and s1 > 0.0
    st, s0, s1 = step_sums(lib, bs8, 257, a, b, None)
    assert st == 0 and s1 == 0.0 and s0 > 0.0
    assert step_sums(lib, bs8, 257, a, None, None)[0] == EINVAL
    assert step_sums(lib, bs8, 0, a, b, c)[0] == EINVAL
    assert step_sums(lib, bs8, 257, a, b, c, handle=False)[0] == EINVAL


# ======================================================================================= B. Anderson acceleration
def _eig_solve_mp(G, c):
    """minimum-norm solution of G beta = -c and the singular values of M (G = M'M), mpmath at 50 digits"""
    k = len(c)
    Gm = mp.matrix(k, k)
    for i in range(k):
        for j in range(k):
            Gm[i, j] = _mpf(G[i, j])
    if k > 6:            # (the cross-check of a long, well-conditioned history: eigenvectors of 31 x 31 cost seconds)
        E = mp.eigsy(Gm, eigvals_only=True)
        sol = mp.lu_solve(Gm, mp.matrix([_mpf(v) for v in c]))
        E, Q, beta = [E[i] for i in range(k)], None, [-sol[i] for i in range(k)]
    else:
        E, Q = mp.eigsy(Gm)
        E = [E[i] for i in range(k)]
        beta = [mp.mpf(0)] * k
    cut = mp.mpf(EPS) * k * max(E)
    for e in range(k if Q is not None else 0):
        if not E[e] > cut:
            continue
        qc = mp.fsum(Q[i, e] * _mpf(c[i]) for i in range(k))
        for i in range(k):
            beta[i] -= Q[i, e] * qc / E[e]
    return np.array([LD(float(v)) + LD(float(v - mp.mpf(float(v)))) for v in beta]), \
        np.sqrt(np.maximum(np.array([float(v) for v in E]), 0.0))


def _refined_solve(G, c):
    """the same for more than 6 well-conditioned columns: float64 solve, residuals in ``np.longdouble``; cond(M) from the
    float64 eigenvalues of G (relative error cond(M)^2 eps)"""
    G64 = G.astype(np.float64)
    beta = np.zeros(len(c), dtype=LD)
    for _ in range(4):
        beta = beta + np.linalg.solve(G64, (-c - G @ beta).astype(np.float64)).astype(LD)
    return beta, np.sqrt(np.maximum(np.linalg.eigvalsh(G64), 0.0))


class RefAnderson:
    """anderson.jl:36-130 with its own history lists.  Up to 6 columns (every case with a drop) M is formed explicitly and
    the problem goes to mpmath; longer histories keep <r_i, r_j> in ``np.longdouble`` from step to step (M'M at O(n m) instead
    of O(n m^2) per step) and take the refined float64 solve -- ``force_mp`` sends such a step down the first path."""

    def __init__(self, m, maxcond, errorfactor):
        self.m, self.maxcond, self.errorfactor = m, maxcond, errorfactor
        self.xs, self.rs, self.errors = [], [], []
        self.gram = np.zeros((0, 0), dtype=LD)
        self.margin = math.inf        # smallest factor between a tested quantity and its threshold

    def _delete(self, i):
        for lst in (self.xs, self.rs, self.errors):
            lst.pop(i)
        self.gram = np.delete(np.delete(self.gram, i, axis=0), i, axis=1)

    def _push(self, x, pf):
        row = np.array([r @ pf for r in self.rs] + [pf @ pf], dtype=LD)
        k = len(self.rs)
        g = np.zeros((k + 1, k + 1), dtype=LD)
        g[:k, :k] = self.gram
        g[k, :] = g[:, k] = row
        self.gram = g
        self.xs.append(x)
        self.rs.append(pf)
        self.errors.append(_norm(pf))
        if len(self.xs) > self.m:
            self._delete(0)

    def _near(self, value, threshold):
        if value > 0 and threshold > 0 and math.isfinite(value):
            self.margin = min(self.margin, max(value / threshold, threshold / value))

    def _problem(self, pf, explicit):
        if explicit:
            M = np.stack(self.rs, axis=1) - pf[:, None]          # M_ij = (Pf x_j)_i - (Pf x_n)_i
            return _eig_solve_mp(M.T @ M, M.T @ pf)
        rp = np.array([r @ pf for r in self.rs], dtype=LD)
        pp = pf @ pf
        return _refined_solve(self.gram - rp[:, None] - rp[None, :] + pp, rp - pp)

    def __call__(self, x, alpha, pf, force_mp=False):
        x, pf = np.asarray(x, dtype=LD), np.asarray(pf, dtype=LD)
        plain = x + LD(alpha) * pf
        info = dict(accelerated=False, dropped_error=[], dropped_cond=[], kappa=1.0, S=_norm(plain), cond_seen=[])
        if self.m == 0 or self.errorfactor <= 1 or self.maxcond <= 1:
            return plain, info
        if not self.xs:
            self._push(x, pf)
            return plain, info
        min_error = min(self.errors + [_norm(pf)])
        for e in self.errors[:-1]:
            self._near(e, self.errorfactor * min_error)
        drop = [i for i, e in enumerate(self.errors[:-1]) if e > self.errorfactor * min_error]
        for i in reversed(drop):
            self._delete(i)
        info["dropped_error"] = drop
        while True:
            k = len(self.rs)
            beta, sv = self._problem(pf, k <= 6 or force_mp)
            cond = sv.max() / sv.min() if sv.min() > 0 else math.inf
            info["cond_seen"].append(cond)
            if k > 1:
                self._near(cond, self.maxcond)
            if k > 1 and cond > self.maxcond:
                idrop = int(np.argmax(self.errors[:-1]))          # findmax: the first of the largest
                others = [e for j, e in enumerate(self.errors[:-1]) if j != idrop]
                if others:
                    self._near(self.errors[idrop], max(others))
                self._delete(idrop)
                info["dropped_cond"].append(idrop)
                continue
            break
        xn = plain.copy()
        S = abs(1.0 - float(beta.sum())) * _norm(plain)
        for b_i, x_i, r_i in zip(beta, self.xs, self.rs):
            xn += b_i * (x_i - x + LD(alpha) * (r_i - pf))
            S += abs(float(b_i)) * _norm(x_i + LD(alpha) * r_i)
        info.update(accelerated=True, kappa=cond if math.isfinite(cond) else 1.0, S=S, beta=beta)
        self._push(x, pf)
        return xn, info


class Acc:
    """a ``dftk_mi_anderson`` accumulator"""

    def __init__(self, lib, bs, n, m, maxcond=1e6, errorfactor=1e5):
        self.lib, self.bs, self.n = lib, bs, n
        self.h = C.c_void_p()
        abi_check(lib.dftk_mi_anderson_create(bs.h, n, m, maxcond, errorfactor, C.byref(self.h)))

    def step(self, x, alpha, pf):
        xd, pd = dev(x), dev(pf)
        xn = torch.full_like(xd, NAN)
        nh = C.c_int(-7)
        st = self.lib.dftk_mi_anderson_step(self.h, xd.data_ptr(), alpha, pd.data_ptr(), xn.data_ptr(), C.byref(nh))
        self.bs.sync()
        return st, xn.cpu().numpy(), nh.value

    def history(self):
        return self.lib.dftk_mi_anderson_history(self.h)

    def reset(self):
        return self.lib.dftk_mi_anderson_reset(self.h)

    def __del__(self):
        try:
            self.lib.dftk_mi_anderson_destroy(self.h)
        except Exception:
            pass


def _check_step(acc, ref, x, alpha, pf, tag, stats):
    """one step on both sides: same history count, iterate within the bound of the module docstring"""
    st, got, nh = acc.step(x, alpha, pf)
    want, info = ref(x, alpha, pf)
    assert st == 0, tag
    assert nh == len(ref.xs) == acc.history(), (tag, nh, len(ref.xs))
    assert np.all(np.isfinite(got)), tag
    err = _norm(got.astype(LD) - want)
    if info["accelerated"]:
        bound = 64.0 * info["kappa"] ** 2 * EPS * info["S"]
    else:
        bound = 4.0 * EPS * (_norm(x) + abs(alpha) * _norm(pf))
    stats.append((info["kappa"], err / bound))
    assert err <= bound, (tag, err, bound, info["kappa"])
    return info


def _report(name, stats):
    k = max(s[0] for s in stats)
    print(f"\nanderson {name}: {len(stats)} steps, max cond(M) = {k:.3g}, max err / bound = {max(s[1] for s in stats):.3g}")


def _pairs(rng, n, count):
    return [(rng.standard_normal(n), rng.standard_normal(n)) for _ in range(count)]


@pytest.mark.parametrize("n,m", [(257, 5), (4099, 31), (33000, 3)])
def test_anderson_rollover_and_table_capacity(lib, bs8, n, m):
    """3 m + 4 random pairs with both drop rules out of reach: the history fills (m = 31: every entry of the pointer table),
    then the oldest entry leaves at every step and its slot is taken again (m = 3: on every step)."""
    rng = np.random.default_rng(n + m)
    acc, ref, stats = Acc(lib, bs8, n, m, 1e300, 1e300), RefAnderson(m, 1e300, 1e300), []
    for it, (x, pf) in enumerate(_pairs(rng, n, 3 * m + 4)):
        info = _check_step(acc, ref, x, 0.7, pf, (n, m, it), stats)
        assert acc.history() == min(it + 1, m)
        assert not info["dropped_error"] and not info["dropped_cond"]
    if m > 6:
        # the refined float64 solve of the long histories against mpmath, on the problem of one more step
        x, pf = _pairs(rng, n, 1)[0]
        twin = RefAnderson(m, 1e300, 1e300)
        twin.xs, twin.rs, twin.errors, twin.gram = list(ref.xs), list(ref.rs), list(ref.errors), ref.gram.copy()
        fast, fi = ref(x, 0.7, pf)
        slow, si = twin(x, 0.7, pf, force_mp=True)
        assert _norm(fast - slow) <= 1e-17 * fi["S"] and abs(fi["kappa"] - si["kappa"]) <= 1e-12 * si["kappa"]
    _report(f"rollover n={n} m={m}", stats)


def test_anderson_create_refuses_more_than_the_table_holds(lib, bs8):
    h = C.c_void_p()
    assert lib.dftk_mi_anderson_create(bs8.h, 257, 32, 1e6, 1e5, C.byref(h)) == EINVAL
    assert lib.dftk_mi_anderson_create(bs8.h, 257, -1, 1e6, 1e5, C.byref(h)) == EINVAL
    assert lib.dftk_mi_anderson_create(bs8.h, 0, 5, 1e6, 1e5, C.byref(h)) == EINVAL
    assert lib.dftk_mi_anderson_create(None, 257, 5, 1e6, 1e5, C.byref(h)) == EINVAL


def _unit(rng, n):
    v = rng.standard_normal(n)
    return v / np.linalg.norm(v)


def test_anderson_errorfactor_drop(lib, bs8):
    """Residual norms 1, 1e3, 1, 1, 1e-3 with errorfactor = 1e2: the 1e3 entry leaves at the fourth step (not at the third,
    where it is the newest), both remaining old entries at the fifth, the last entry of norm 1 at the sixth; the later pairs
    take the freed slots."""
    n, m = 1031, 6
    rng = np.random.default_rng(21)
    acc, ref, stats = Acc(lib, bs8, n, m, 1e300, 1e2), RefAnderson(m, 1e300, 1e2), []
    dropped, hist = [], []
    for it, scale in enumerate([1.0, 1e3, 1.0, 1.0, 1e-3, 2e-3, 5e-4, 1e-3]):
        info = _check_step(acc, ref, rng.standard_normal(n), 0.7, scale * _unit(rng, n), ("errorfactor", it), stats)
        dropped.append(info["dropped_error"])
        hist.append(acc.history())
        assert not info["dropped_cond"]
    assert dropped == [[], [], [], [1], [0, 1], [0], [], []]
    assert hist == [1, 2, 3, 3, 2, 2, 3, 4]
    assert ref.margin >= 2.0
    _report("errorfactor", stats)


def test_anderson_maxcond_drop(lib, bs8):
    """maxcond = 1e4.  At the fifth step the columns of M for the entries a and b are parallel to 1e-7: b = p + (a - p) / 4 +
    1e-7 d with p the fifth residual, so cond(M) ~ 1e8.  The errors are 64 (z), 16 (a), 4 (b), 2 (c), 1 (p): z leaves, the
    condition number stays, a leaves; b and c (the newest) stay.  Three more pairs follow."""
    n, m = 1031, 6
    rng = np.random.default_rng(22)
    acc, ref, stats = Acc(lib, bs8, n, m, 1e4, 1e300), RefAnderson(m, 1e4, 1e300), []
    p = _unit(rng, n)
    z, a, c = 64.0 * _unit(rng, n), 16.0 * _unit(rng, n), 2.0 * _unit(rng, n)
    b = p + 0.25 * (a - p) + 1e-7 * _unit(rng, n)
    dropped = []
    for it, pf in enumerate([z, a, b, c, p, _unit(rng, n), 0.5 * _unit(rng, n), 0.25 * _unit(rng, n)]):
        info = _check_step(acc, ref, rng.standard_normal(n), 0.7, pf, ("maxcond", it), stats)
        dropped.append(info["dropped_cond"])
        assert not info["dropped_error"]
        if it == 4:
            assert info["cond_seen"][0] > 1e6 and info["cond_seen"][1] > 1e6 and info["cond_seen"][2] < 1e2
    assert dropped == [[], [], [], [], [0, 0], [], [], []]
    assert ref.margin >= 2.0
    _report("maxcond", stats)


def test_anderson_singular_problem(lib, bs8):
    """The same pair twice: M = 0, one column (nothing to drop); the minimum-norm solution is beta = 0, the plain step."""
    n = 1031
    rng = np.random.default_rng(23)
    acc, ref = Acc(lib, bs8, n, 4), RefAnderson(4, 1e6, 1e5)
    x, pf = _pairs(rng, n, 1)[0]
    for it in range(2):
        st, got, nh = acc.step(x, 0.7, pf)
        want, info = ref(x, 0.7, pf)
        assert st == 0 and nh == len(ref.xs) == it + 1
        assert np.all(np.isfinite(got))
        assert _norm(got.astype(LD) - (x.astype(LD) + LD(0.7) * pf)) <= 4 * EPS * (_norm(x) + 0.7 * _norm(pf))
        assert _norm(want - (x.astype(LD) + LD(0.7) * pf)) == 0.0


def test_anderson_zero_residual(lib, bs8):
    """Pf = 0 after two ordinary steps: every older entry with a nonzero error is dropped (errorfactor x 0), the newest stays
    and gets beta = 0."""
    n = 1031
    rng = np.random.default_rng(24)
    acc, ref, stats = Acc(lib, bs8, n, 4), RefAnderson(4, 1e6, 1e5), []
    for it, (x, pf) in enumerate(_pairs(rng, n, 2)):
        _check_step(acc, ref, x, 0.7, pf, ("zero", it), stats)
    x = rng.standard_normal(n)
    info = _check_step(acc, ref, x, 0.7, np.zeros(n), ("zero", 2), stats)
    assert info["dropped_error"] == [0] and acc.history() == 2
    x, pf = _pairs(rng, n, 1)[0]
    _check_step(acc, ref, x, 0.7, pf, ("zero", 3), stats)


def test_anderson_nonfinite_input_leaves_the_history_alone(lib, bs8):
    n = 1031
    rng = np.random.default_rng(25)
    acc, ref, stats = Acc(lib, bs8, n, 4), RefAnderson(4, 1e6, 1e5), []
    for it, (x, pf) in enumerate(_pairs(rng, n, 2)):
        _check_step(acc, ref, x, 0.7, pf, ("nan", it), stats)
    x, pf = _pairs(rng, n, 1)[0]
    pf[517] = NAN
    st, _, _ = acc.step(x, 0.7, pf)
    assert st == NONFINITE and acc.history() == 2
    for it, (x, pf) in enumerate(_pairs(rng, n, 2)):
        _check_step(acc, ref, x, 0.7, pf, ("nan", 2 + it), stats)      # the reference never saw the bad pair


def test_anderson_reset(lib, bs8):
    n, m = 1031, 4
    rng = np.random.default_rng(26)
    acc, ref, stats = Acc(lib, bs8, n, m), RefAnderson(m, 1e6, 1e5), []
    for it, (x, pf) in enumerate(_pairs(rng, n, m + 1)):
        _check_step(acc, ref, x, 0.7, pf, ("reset", it), stats)
    assert acc.reset() == 0 and acc.history() == 0
    ref = RefAnderson(m, 1e6, 1e5)
    for it, (x, pf) in enumerate(_pairs(rng, n, m + 3)):
        info = _check_step(acc, ref, x, 0.7, pf, ("after reset", it), stats)
        assert info["accelerated"] == (it > 0)
    _report("reset", stats)


@pytest.mark.parametrize("m,maxcond,errorfactor", [(0, 1e6, 1e5), (5, 1e6, 1.0), (5, 1e6, 0.5), (5, 1.0, 1e5), (5, 0.5, 1e5)])
def test_anderson_disabled_is_plain_damping(lib, bs8, m, maxcond, errorfactor):
    """anderson.jl:82: m = 0, errorfactor <= 1 or maxcond <= 1 switch the acceleration off -- the plain damped step at EVERY
    call and no history."""
    n = 1031
    rng = np.random.default_rng(27)
    acc, ref, stats = Acc(lib, bs8, n, m, maxcond, errorfactor), RefAnderson(m, maxcond, errorfactor), []
    for it, (x, pf) in enumerate(_pairs(rng, n, 4)):
        info = _check_step(acc, ref, x, 0.7, pf, ("disabled", it), stats)
        assert not info["accelerated"] and acc.history() == 0


def test_anderson_argument_checks(lib, bs8):
    n = 257
    acc = Acc(lib, bs8, n, 3)
    x, pf, xn = (dev(np.ones(n)) for _ in range(3))
    step = lib.dftk_mi_anderson_step
    assert step(acc.h, x.data_ptr(), 0.5, pf.data_ptr(), x.data_ptr(), None) == EINVAL
    assert step(acc.h, x.data_ptr(), 0.5, pf.data_ptr(), pf.data_ptr(), None) == EINVAL
    assert step(acc.h, None, 0.5, pf.data_ptr(), xn.data_ptr(), None) == EINVAL
    assert step(acc.h, x.data_ptr(), 0.5, None, xn.data_ptr(), None) == EINVAL
    assert step(acc.h, x.data_ptr(), 0.5, pf.data_ptr(), None, None) == EINVAL
    assert step(None, x.data_ptr(), 0.5, pf.data_ptr(), xn.data_ptr(), None) == EINVAL
    assert lib.dftk_mi_anderson_reset(None) == EINVAL
    assert lib.dftk_mi_anderson_history(None) == -1
    assert acc.history() == 0
    assert step(acc.h, x.data_ptr(), 0.5, pf.data_ptr(), xn.data_ptr(), None) == 0      # n_history may be NULL
    bs8.sync()
    assert acc.history() == 1 and np.array_equal(xn.cpu().numpy(), np.full(n, 1.5))


# ======================================================================================= C. dftk_mi_chi0_mix
A_LAT = 7.65
LATTICE = A_LAT / 2 * np.array([[0.0, 1, 1], [1, 0, 1], [1, 1, 0]]).T @ np.diag([2.0, 1.0, 1.0])
RECIP = 2 * np.pi * np.linalg.inv(LATTICE).T
BH = np.asfortranarray(RECIP)
VOL = abs(np.linalg.det(LATTICE))
CUBES = {"even": (6, 5, 4), "odd": (5, 3, 7)}
KTF, EPS_R = 0.9, 7.0
RELTOL_TWICE = 1e-10      # two channels on the even cube: the reference GMRES needs 18 steps (16 at 1e-9)


class Cube:
    """a basis, its cube k-block and the multiplier cubes in (nz, ny, nx) order"""

    def __init__(self, lib, shape):
        nx, ny, nz = shape
        self.shape, self.N = (nz, ny, nx), nx * ny * nz
        self.dvol = VOL / self.N
        self.bs = Basis(lib, nx, ny, nz, VOL)
        self.kb = KBlock(lib, self.bs, np.arange(self.N), np.zeros(self.N))
        gz, gy, gx = np.meshgrid(np.fft.fftfreq(nz) * nz, np.fft.fftfreq(ny) * ny, np.fft.fftfreq(nx) * nx, indexing="ij")
        Gc = np.einsum("ij,j...->i...", RECIP, np.stack([gx, gy, gz]))
        self.G2 = (Gc ** 2).sum(axis=0)
        with np.errstate(divide="ignore"):
            self.poisson = np.where(self.G2 > 0, 4 * np.pi / self.G2, 0.0)          # hartree.jl:68-81
        self.poisson_d = dev(self.poisson)
        self.nyquist = np.zeros(self.shape, dtype=bool)                           # entries without a -G partner
        for ax, n_ax in enumerate((nz, ny, nx)):
            if n_ax % 2 == 0:
                idx = [slice(None)] * 3
                idx[ax] = n_ax // 2
                self.nyquist[tuple(idx)] = True
        self.cache = {}

    def chi0_dielectric(self, kTF=KTF, eps_r=EPS_R):                               # chi0models.jl:66-77
        C0 = 1 - eps_r
        return C0 * kTF ** 2 * self.G2 / (4 * np.pi) / (kTF ** 2 - C0 * self.G2)

    def filt(self, mult, f):
        return np.real(np.fft.ifftn(mult * np.fft.fftn(f)))


@pytest.fixture(scope="module")
def cubes(lib):
    return {name: Cube(lib, shape) for name, shape in CUBES.items()}


def make_ldos(cube, n_comp, scale, seed=1):
    return scale * np.random.default_rng(seed).uniform(0.1, 1.0, (n_comp,) + cube.shape)


def make_dF(cube, n_comp, seed=2):
    return np.random.default_rng(seed).standard_normal((n_comp,) + cube.shape)


def apply_operator(cube, x, ldos, poisson, dielectric):
    """mixing.jl:269-279 for one vector of shape (n_comp, nz, ny, nx)"""
    dV = cube.filt(poisson, x.sum(axis=0)) if poisson is not None else np.zeros(cube.shape)
    dV = dV - dV.mean()
    out = x.copy()
    if ldos is not None:                                                          # chi0models.jl:36-40, alpha = -1
        tdos = ldos.sum() * cube.dvol
        deF = (ldos * dV[None]).sum() * cube.dvol
        out -= -ldos * dV[None] + ldos * deF / tdos
    if dielectric is not None:
        out -= cube.filt(cube.chi0_dielectric(*dielectric), dV)[None]
    return out - out.mean()


class Dense:
    """the dense operator of one case, its reference solve and its singular values"""

    def __init__(self, cube, n_comp, ldos, poisson, dielectric):
        self.Nt = Nt = cube.N * n_comp
        self.shape = (n_comp,) + cube.shape
        A = np.empty((Nt, Nt))
        for j in range(Nt):
            e = np.zeros(Nt)
            e[j] = 1.0
            A[:, j] = apply_operator(cube, e.reshape(self.shape), ldos, poisson, dielectric).reshape(-1)
        self.A, self.A_ld = A, A.astype(LD)
        P = np.eye(Nt) - 1.0 / Nt
        U, sv, Vt = np.linalg.svd(P @ A @ P)
        self.smax, self.smin = sv[0], sv[Nt - 2]          # sv[Nt - 1] ~ 0: the constants
        self.pinv = (Vt[:Nt - 1].T / sv[:Nt - 1]) @ U[:, :Nt - 1].T       # least squares on the zero-mean subspace

    def solve(self, dF):
        f = dF.reshape(-1).astype(LD)
        dc = f.sum() / LD(self.Nt)
        b = f - dc
        x = (self.pinv @ b.astype(np.float64)).astype(LD)
        x = x + (self.pinv @ (b - self.A_ld @ x).astype(np.float64)).astype(LD)          # one refinement
        return x, b, dc


def numpy_gmres(A, b, tol, krylovdim, maxiter):
    """plain restarted GMRES, zero start, modified Gram-Schmidt twice, the true residual once per cycle; returns x, the Krylov
    steps per cycle, the operator applications (steps + true residuals) and whether |b - A x| <= tol"""
    n = len(b)
    x = np.zeros(n)
    r, beta = b.copy(), np.linalg.norm(b)
    steps, applies = [], 0
    for _ in range(maxiter):
        if beta <= tol:
            break
        V = np.zeros((krylovdim + 1, n))
        H = np.zeros((krylovdim + 1, krylovdim))
        V[0] = r / beta
        k_used = 0
        for k in range(krylovdim):
            w = A @ V[k]
            applies += 1
            for _pass in range(2):
                for i in range(k + 1):
                    h = V[i] @ w
                    w -= h * V[i]
                    H[i, k] += h
            H[k + 1, k] = np.linalg.norm(w)
            k_used = k + 1
            e1 = np.zeros(k_used + 1)
            e1[0] = beta
            y, res = np.linalg.lstsq(H[:k_used + 1, :k_used], e1, rcond=None)[:2]
            est = np.linalg.norm(e1 - H[:k_used + 1, :k_used] @ y)
            if est <= tol or H[k + 1, k] == 0.0:
                break
            V[k + 1] = w / H[k + 1, k]
        steps.append(k_used)
        x = x + y @ V[:k_used]
        r = b - A @ x
        applies += 1
        beta = np.linalg.norm(r)
    return x, steps, applies, beta <= tol


def chi0_mix(lib, cube, n_comp, dF, ldos=None, poisson=True, dielectric=None, reltol=1e-9, krylovdim=30, maxiter=100,
             lattice=True, inplace=False, kb=None):
    """the library call; ``dielectric``: (kTF, eps_r) or None.  Returns status, d_rho, n_applies, converged."""
    fd = dev(dF)
    out = fd if inplace else torch.full_like(fd, NAN)
    ld = dev(ldos) if ldos is not None else None
    n_app, conv = C.c_int(-7), C.c_int(-7)
    kTF, eps_r = dielectric if dielectric is not None else (0.0, 1.0)
    torch.cuda.synchronize()
    st = lib.dftk_mi_chi0_mix((kb or cube.kb).h, n_comp, BH.ctypes.data if lattice else None,
                              cube.poisson_d.data_ptr() if poisson else None, _ptr(ld), cube.dvol,
                              1 if dielectric is not None else 0, kTF, eps_r, _ptr(fd), reltol, krylovdim, maxiter, _ptr(out),
                              C.byref(n_app), C.byref(conv))
    cube.bs.sync()
    return st, out.cpu().numpy(), n_app.value, conv.value


def dense_case(cube, n_comp, scale, dielectric=None, with_ldos=True, poisson=True):
    key = (n_comp, scale, dielectric, with_ldos, poisson)
    if key not in cube.cache:
        ldos = make_ldos(cube, n_comp, scale) if with_ldos else None
        cube.cache[key] = (ldos, Dense(cube, n_comp, ldos, cube.poisson if poisson else None, dielectric))
    return cube.cache[key]


def check_solve(lib, cube, n_comp, scale, reltol, krylovdim=30, maxiter=100, dielectric=None, with_ldos=True, inplace=False,
                tag="", reach=None):
    """one converged solve against the dense operator: residual, error, mean, applications (module docstring); ``reach``: what
    the Krylov steps per cycle of the NumPy GMRES must satisfy for the case to reach its branch, asserted before the call"""
    ldos, D = dense_case(cube, n_comp, scale, dielectric, with_ldos)
    dF = make_dF(cube, n_comp)
    x_ref, b, dc = D.solve(dF)
    nb = _norm(b)
    tol = max(1e-12, reltol * nb)
    _, steps, ref_applies, ref_ok = numpy_gmres(D.A, b.astype(np.float64), tol, krylovdim, maxiter)
    assert ref_ok and (reach is None or reach(steps)), steps
    st, got, n_app, conv = chi0_mix(lib, cube, n_comp, dF, ldos, True, dielectric, reltol, krylovdim, maxiter, inplace=inplace)
    assert st == 0 and conv == 1
    x = got.reshape(-1).astype(LD) - dc
    delta = (sum(steps) + 1) * D.Nt * EPS * (D.smax * _norm(x) + nb)
    res = _norm(b - D.A_ld @ x)
    err = _norm(x - x_ref)
    print(f"\nchi0_mix {tag}: Nt={D.Nt} reference steps {sum(steps)} in {len(steps)} cycle(s), applies ref {ref_applies} / "
          f"library {n_app}; tol={tol:.3g} delta={delta:.3g} residual={res:.3g} error={err:.3g} "
          f"sigma=[{D.smin:.3g}, {D.smax:.3g}]")
    assert res <= tol + delta
    assert err <= (tol + delta) / D.smin
    assert abs(float(got.astype(LD).sum() / LD(D.Nt) - dc)) <= 4 * EPS * np.abs(dF).max()
    assert abs(n_app - ref_applies) <= 1
    return got, steps, n_app


def fourier_filter(lib, cube, mult, f):
    out = torch.full(cube.shape, NAN, dtype=torch.float64, device="cuda")
    md, fd = dev(mult), dev(f)
    abi_check(lib.dftk_mi_cube_fourier_filter(cube.kb.h, md.data_ptr(), fd.data_ptr(), out.data_ptr()))
    cube.bs.sync()
    return out.cpu().numpy()


def test_chi0_mix_krylov_buffer_grows_once(lib, cubes):
    check_solve(lib, cubes["even"], 1, 0.2, 1e-9, tag="growth once",
                reach=lambda steps: len(steps) == 1 and 9 <= steps[0] <= 15)           # past 8 vectors, not past 16


def test_chi0_mix_krylov_buffer_grows_twice_and_the_workspace_still_serves(lib, cubes):
    """Two spin channels with their own LDOS (both see the total density's dV); the buffer grows at k = 7 and k = 15 and
    replaces the basis' workspace, which the next cube entry of the same basis must find usable."""
    cube = cubes["even"]
    check_solve(lib, cube, 2, 0.2, RELTOL_TWICE, tag="growth twice", reach=lambda steps: len(steps) == 1 and steps[0] >= 17)
    f = make_dF(cube, 1, seed=9)[0]
    out = fourier_filter(lib, cube, cube.poisson, f)
    assert _norm(out - cube.filt(cube.poisson, f)) <= 64 * EPS * cube.poisson.max() * _norm(f)


def test_chi0_mix_restarts(lib, cubes):
    check_solve(lib, cubes["even"], 2, 0.2, RELTOL_TWICE, krylovdim=3, tag="restarts",
                reach=lambda steps: len(steps) > 3 and all(s == 3 for s in steps[:-1]))


@pytest.mark.parametrize("name", ["even", "odd"])
def test_chi0_mix_hybrid(lib, cubes, name):
    check_solve(lib, cubes[name], 1, 0.2, 1e-9, dielectric=(KTF, EPS_R), tag=f"hybrid {name}")


@pytest.mark.parametrize("name", ["even", "odd"])
def test_chi0_mix_dielectric_only(lib, cubes, name):
    check_solve(lib, cubes[name], 1, 0.2, 1e-9, dielectric=(KTF, EPS_R), with_ldos=False, tag=f"dielectric only {name}")


def test_chi0_mix_all_odd_cube_ldos(lib, cubes):
    check_solve(lib, cubes["odd"], 2, 0.2, 1e-9, tag="odd, two channels")


def test_chi0_mix_physical_ldos_ends_within_eight_vectors(lib, cubes):
    """scale 0.02 is what a physical LDOS looks like: the solve ends at the boundary of the first buffer, where the exit
    trusts the Givens estimate."""
    check_solve(lib, cubes["even"], 1, 0.02, 1e-11, tag="physical", reach=lambda steps: steps in ([7], [8]))


def test_chi0_mix_default_tolerance(lib, cubes):
    check_solve(lib, cubes["even"], 1, 0.2, 1e-2, tag="reltol 1e-2", reach=lambda steps: sum(steps) <= 5)


def test_chi0_mix_aliased_output(lib, cubes):
    cube = cubes["even"]
    ldos, _ = dense_case(cube, 1, 0.2)
    dF = make_dF(cube, 1)
    a = chi0_mix(lib, cube, 1, dF, ldos)
    b = chi0_mix(lib, cube, 1, dF, ldos, inplace=True)
    assert a[0] == b[0] == 0 and a[2:] == b[2:] and np.array_equal(a[1], b[1])
    check_solve(lib, cube, 1, 0.2, 1e-9, inplace=True, tag="in place")
    dead = 1e-9 * np.random.default_rng(3).uniform(0.0, 1.0, (1,) + cube.shape)
    st, out, n_app, conv = chi0_mix(lib, cube, 1, dF, dead, inplace=True)
    assert st == 0 and n_app == 0 and conv == 1 and np.array_equal(out, dF)


def test_chi0_mix_krylovdim_boundaries(lib, cubes):
    cube = cubes["even"]
    ldos, _ = dense_case(cube, 1, 0.2)
    dF = make_dF(cube, 1)
    base = chi0_mix(lib, cube, 1, dF, ldos, krylovdim=30)
    top = chi0_mix(lib, cube, 1, dF, ldos, krylovdim=31)
    assert top[0] == 0 and top[3] == 1 and np.array_equal(top[1], base[1])     # the same single cycle
    assert chi0_mix(lib, cube, 1, dF, ldos, krylovdim=32)[0] == EINVAL
    assert chi0_mix(lib, cube, 1, dF, ldos, krylovdim=0)[0] == EINVAL
    assert chi0_mix(lib, cube, 1, dF, ldos, maxiter=0)[0] == EINVAL


def test_chi0_mix_maxiter_exhausted(lib, cubes):
    """krylovdim = 2, maxiter = 1: two Krylov steps and the true residual, not converged; the iterate is the minimiser of
    |b - A x| over span{b, A b}."""
    cube = cubes["even"]
    ldos, D = dense_case(cube, 1, 0.2)
    dF = make_dF(cube, 1)
    _, b, dc = D.solve(dF)
    _, steps, _, ref_ok = numpy_gmres(D.A, b.astype(np.float64), 1e-9 * _norm(b), 2, 1)
    assert steps == [2] and not ref_ok
    st, got, n_app, conv = chi0_mix(lib, cube, 1, dF, ldos, reltol=1e-9, krylovdim=2, maxiter=1)
    assert st == 0 and conv == 0 and n_app == 3
    K = np.stack([b, D.A_ld @ b], axis=1)
    AK = (D.A_ld @ K).astype(np.float64)
    y = np.linalg.lstsq(AK, b.astype(np.float64), rcond=None)[0]
    y = y + np.linalg.lstsq(AK, (b - D.A_ld @ (K @ y.astype(LD))).astype(np.float64), rcond=None)[0]
    x_min = K @ y.astype(LD)
    x = got.reshape(-1).astype(LD) - dc
    bound = 64 * EPS * np.linalg.cond(AK) * _norm(x)
    print(f"\nchi0_mix maxiter: |x - x_min| = {_norm(x - x_min):.3g}, bound {bound:.3g}, cond = {np.linalg.cond(AK):.3g}")
    assert _norm(x - x_min) <= bound


def test_chi0_mix_no_term_alive_is_simple_mixing(lib, cubes):
    cube = cubes["even"]
    dF = make_dF(cube, 1)
    dead = 1e-9 * np.random.default_rng(3).uniform(0.0, 1.0, (1,) + cube.shape)
    assert np.abs(dead).max() < math.sqrt(EPS)
    for ldos, diel in ((None, (KTF, 1.0)), (dead, None), (dead, (KTF, 1.0))):
        st, out, n_app, conv = chi0_mix(lib, cube, 1, dF, ldos, dielectric=diel)
        assert st == 0 and n_app == 0 and conv == 1 and np.array_equal(out, dF)
    assert chi0_mix(lib, cube, 1, dF, None, dielectric=(KTF, EPS_R), lattice=False)[0] == EINVAL


@pytest.mark.parametrize("name", ["even", "odd"])
def test_chi0_mix_dead_ldos_beside_the_dielectric_model(lib, cubes, name):
    cube = cubes[name]
    dF = make_dF(cube, 1)
    dead = 1e-9 * np.random.default_rng(3).uniform(0.0, 1.0, (1,) + cube.shape)
    alone = chi0_mix(lib, cube, 1, dF, None, dielectric=(KTF, EPS_R))
    both = chi0_mix(lib, cube, 1, dF, dead, dielectric=(KTF, EPS_R))
    assert alone[0] == both[0] == 0 and alone[2:] == both[2:] and alone[2] > 0 and np.array_equal(alone[1], both[1])


def test_chi0_mix_without_hartree_kernel(lib, cubes):
    """poisson_d = NULL with an LDOS: dV = 0, the operator is the centring, one application."""
    cube = cubes["even"]
    ldos, _ = dense_case(cube, 1, 0.2)
    dF = make_dF(cube, 1)
    st, out, n_app, conv = chi0_mix(lib, cube, 1, dF, ldos, poisson=False)
    assert st == 0 and conv == 1 and n_app == 1
    assert _norm(out - dF) <= 8 * EPS * _norm(dF)


def test_chi0_mix_refusals_leave_no_state(lib, cubes):
    cube = cubes["even"]
    ldos, _ = dense_case(cube, 1, 0.2)
    dF = make_dF(cube, 1)
    before = chi0_mix(lib, cube, 1, dF, ldos)
    bad = dF.copy()
    bad[0, 1, 2, 3] = NAN
    assert chi0_mix(lib, cube, 1, bad, ldos)[0] == NONFINITE
    assert chi0_mix(lib, cube, 3, dF, ldos)[0] == EINVAL
    assert chi0_mix(lib, cube, 1, dF, ldos, reltol=0.0)[0] == EINVAL
    fd, out = dev(dF), dev(dF)
    n_app, conv = C.c_int(), C.c_int()
    for f_ptr, o_ptr in ((None, out.data_ptr()), (fd.data_ptr(), None)):
        assert lib.dftk_mi_chi0_mix(cube.kb.h, 1, BH.ctypes.data, cube.poisson_d.data_ptr(), None, cube.dvol, 1, KTF, EPS_R,
                                    f_ptr, 1e-9, 30, 100, o_ptr, C.byref(n_app), C.byref(conv)) == EINVAL
    short = KBlock(lib, cube.bs, np.arange(cube.N - 1), np.zeros(cube.N - 1))
    assert chi0_mix(lib, cube, 1, dF, ldos, kb=short)[0] == EINVAL
    after = chi0_mix(lib, cube, 1, dF, ldos)
    assert after[0] == 0 and after[2:] == before[2:] and np.array_equal(after[1], before[1])


# ======================================================================================= D. the multiplier entries
@pytest.mark.parametrize("name", ["even", "odd"])
def test_fourier_multiplier_entries_against_numpy(lib, cubes, name):
    """mixing.jl:61-72 (Kerker, with the enforce_real! mask), :161-171 (dielectric), chi0models.jl:66-77 and a stored
    multiplier cube, on cubes where no axis has another's length."""
    cube = cubes[name]
    x = make_dF(cube, 1, seed=12)[0] + 0.3
    xd = dev(x)
    G2 = cube.G2
    C0 = 1 - EPS_R
    kerker = np.where(cube.nyquist, 0.0, G2 / (KTF ** 2 + G2))
    diel = (KTF ** 2 - C0 * G2) / (EPS_R * KTF ** 2 - C0 * G2)
    kerker.flat[0] = diel.flat[0] = 1.0
    stored = np.random.default_rng(13).uniform(0.5, 2.0, cube.shape)

    def run(entry, *args):
        out = torch.full(cube.shape, NAN, dtype=torch.float64, device="cuda")
        abi_check(getattr(lib, entry)(cube.kb.h, *args, xd.data_ptr(), out.data_ptr()))
        cube.bs.sync()
        return out.cpu().numpy()

    sd = dev(stored)
    cases = [("dftk_mi_mix_kerker", kerker, run("dftk_mi_mix_kerker", BH.ctypes.data, KTF), True),
             ("dftk_mi_mix_dielectric", diel, run("dftk_mi_mix_dielectric", BH.ctypes.data, KTF, EPS_R), True),
             ("dftk_mi_chi0_dielectric_apply", cube.chi0_dielectric(),
              run("dftk_mi_chi0_dielectric_apply", BH.ctypes.data, KTF, EPS_R), False),
             ("dftk_mi_cube_fourier_filter", stored, run("dftk_mi_cube_fourier_filter", sd.data_ptr()), False),
             ("dftk_mi_cube_fourier_filter", cube.poisson, fourier_filter(lib, cube, cube.poisson, x), False)]
    for entry, mult, got, keeps_mean in cases:
        err, bound = _norm(got - cube.filt(mult, x)), 64 * EPS * np.abs(mult).max() * _norm(x)
        print(f"\n{entry} {name}: err / bound = {err / bound:.3g}")
        assert err <= bound, entry
        if keeps_mean:
            assert abs(got.mean() - x.mean()) <= 4 * EPS * np.abs(x).max(), entry
