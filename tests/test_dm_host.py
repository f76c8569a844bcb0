"""Host-only tests of direct minimisation (no device):

* the twin of the kernels (tests/dm_twin.py): with memory >= history its two-loop recursion gives the direction of the
  explicit BFGS recursion H <- (I - rho s y') H (I - rho y s') + rho s s' started from the preconditioner -- the reference
  of tests/test_gpu_dm_kernels.py is itself right; a bounded memory keeps the newest pairs; a pair with <s, y> <= 0 is
  dropped;
* tangent projection, polar retraction, the twin and the package's ``backtracking`` together on a dense Stiefel problem:
  min tr(X'AX) reaches the sum of the lowest eigenvalues;
* ``backtracking`` on closed-form phi, branch by branch;
* every refusal of ``direct_minimization`` on descriptor-only bases (``device="cpu"``), raised before any device work.
"""
import math

import numpy as np
import pytest

import dftk_jl_amd as dftk
from dftk_jl_amd import KptComm
from dftk_jl_amd.direct_minimization import backtracking, check_supported
import dm_twin as twin

torch = pytest.importorskip("torch")


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ------------------------------------------------------------------------------------------ the twin
def quadratic_history(rng, shapes, n_pairs):
    """points and gradients of a convex quadratic on the packed vectors: every pair has <s, y> > 0"""
    n = sum(2 * r * c for r, c in shapes)
    M = rng.standard_normal((n, n))
    A = M @ M.T / n + np.eye(n)

    def unflatten(v):
        out, at = [], 0
        for r, c in shapes:
            re, im = v[at:at + r * c], v[at + r * c:at + 2 * r * c]
            out.append((re + 1j * im).reshape(r, c))
            at += 2 * r * c
        return out
    xs = [rng.standard_normal(n) for _ in range(n_pairs + 1)]
    return [(unflatten(x), unflatten(A @ x)) for x in xs]


@pytest.mark.parametrize("precond", [False, True])
def test_two_loop_equals_the_explicit_bfgs_recursion(precond):
    rng = np.random.default_rng(5)
    shapes = [(5, 2), (3, 1), (4, 3)]
    hist = quadratic_history(rng, shapes, 4)
    scale = [0.25, 0.5, 0.25]
    kin = [rng.random(r) * 3 for r, _ in shapes] if precond else None
    mk = [rng.random(c) + 0.5 for _, c in shapes] if precond else None
    tw = twin.LbfgsTwin(memory=6)
    for x, g in hist:
        tw.update(x, g)
    assert len(tw.pairs) == 4
    g = [crandn(rng, r, c) for r, c in shapes]
    d = twin.flatten(tw.direction(g, scale, kin, mk))
    ones = [np.ones(s, dtype=complex) for s in shapes]
    H0 = twin.flatten(twin.middle(twin.cast(ones, twin.LD), [twin.LD(s) for s in scale],
                                  None if kin is None else [k.astype(twin.LD) for k in kin],
                                  None if mk is None else [m.astype(twin.LD) for m in mk])).real
    # (flatten puts the imaginary parts of the all-ones blocks -- zeros -- behind the real ones: H0 acts on both alike)
    H0 = np.concatenate([np.tile(h[:len(h) // 2], 2) for h in np.split(H0, np.cumsum([2 * r * c for r, c in shapes])[:-1])])
    pairs = [(twin.flatten(s).astype(twin.LD), twin.flatten(y).astype(twin.LD)) for s, y, _ in tw.pairs]
    ref = twin.explicit_bfgs_direction(pairs, H0, twin.flatten(g).astype(twin.LD))
    err = float(np.abs(d - ref).max() / np.abs(ref).max())
    assert err < 1e-15, err                     # longdouble on both sides: a few of its ulps (2^-63)
    # with an empty history the direction is the middle step, negated
    tw.reset()
    d0 = tw.direction(g, scale, kin, mk)
    want = twin.middle(twin.cast(g, twin.LD), [twin.LD(s) for s in scale],
                       None if kin is None else [k.astype(twin.LD) for k in kin],
                       None if mk is None else [m.astype(twin.LD) for m in mk])
    assert all(np.array_equal(a, -b) for a, b in zip(d0, want))


def test_bounded_memory_keeps_the_newest_pairs_and_drops_bad_ones():
    rng = np.random.default_rng(6)
    shapes = [(4, 2)]
    hist = quadratic_history(rng, shapes, 5)
    full, short = twin.LbfgsTwin(memory=2), twin.LbfgsTwin(memory=8)
    for x, g in hist:
        full.update(x, g)
    for x, g in hist[-3:]:
        short.update(x, g)
    g = [crandn(rng, 4, 2)]
    assert np.array_equal(full.direction(g, [1.0])[0], short.direction(g, [1.0])[0])
    # the same step with the gradient difference reversed: <s, y> < 0, dropped, history unchanged
    x, gr = hist[-1]
    x2 = [x[0] + 0.1]
    g2 = [gr[0] - 0.3]
    sy, kept = full.update(x2, g2)
    assert sy < 0 and not kept and len(full.pairs) == 2
    sy, kept = full.update(x2, g2)             # a zero step: <s, y> = 0
    assert sy == 0 and not kept and len(full.pairs) == 2


def test_stiefel_minimisation_reaches_the_lowest_eigenvalues():
    rng = np.random.default_rng(7)
    n, m = 24, 3
    M = crandn(rng, n, n)
    A = (M + M.conj().T) / 2 + np.diag(np.arange(n))
    lam = np.linalg.eigvalsh(A)
    x = twin.polar_retract(crandn(rng, n, m))
    X = twin.project_tangent(crandn(rng, n, m), x)
    assert np.abs(x.conj().T @ X + X.conj().T @ x).max() < 1e-14           # tangent: x'X is skew-Hermitian
    assert np.abs(twin.project_tangent(X, x) - X).max() < 1e-14            # idempotent
    assert np.abs(x.conj().T @ x - np.eye(m)).max() < 1e-14

    def fg(x):
        return float(np.trace(x.conj().T @ A @ x).real), twin.project_tangent(2 * A @ x, x)

    tw = twin.LbfgsTwin(memory=10, real=np.float64)
    f, g = fg(x)
    tw.update([x], [g])
    for it in range(200):
        d = twin.project_tangent(tw.direction([g], [1.0])[0], x)
        dphi0 = float(twin.dot([g], [d]))
        if not dphi0 < 0:
            tw.reset()
            tw.update([x], [g])
            d = twin.project_tangent(tw.direction([g], [1.0])[0], x)
            dphi0 = float(twin.dot([g], [d]))
        alpha, f, _ = backtracking(lambda a: fg(twin.polar_retract(x + a * d))[0], f, dphi0)
        x = twin.polar_retract(x + alpha * d)
        f, g = fg(x)
        tw.update([x], [g])
        if np.linalg.norm(g) < 1e-6:           # (the energy error is second order in it)
            break
    assert abs(f - lam[:m].sum()) < 1e-10, (f, lam[:m].sum(), it)


# ------------------------------------------------------------------------------------------ the line search
def test_backtracking_accepts_the_first_step():
    calls = []

    def phi(a):
        calls.append(a)
        return (a - 1.0) ** 2 - 1.0
    assert backtracking(phi, 0.0, -2.0) == (1.0, -1.0, 1) and calls == [1.0]
    # the Armijo bound itself: equality is accepted
    assert backtracking(lambda a: 1.0 - 1e-4 * a, 1.0, -1.0)[2] == 1


def test_backtracking_quadratic_step_lands_on_the_minimiser_of_a_parabola():
    alpha, f, trials = backtracking(lambda a: (a - 0.3) ** 2, 0.09, -0.6)
    assert trials == 2 and abs(alpha - 0.3) < 1e-15 and f == (alpha - 0.3) ** 2


def test_backtracking_cubic_steps():
    # a cubic: the model through the last two trials is exact, the third trial is its minimiser (inside the clip range)
    def phi(a):
        return -a + 20 * a ** 2 + 100 * a ** 3
    seen = []
    alpha, f, trials = backtracking(lambda a: (seen.append(a), phi(a))[1], 0.0, -1.0)
    assert trials == 3 and seen[:2] == [1.0, 0.1]                # (the parabola's minimiser 1 / 240, clipped to 0.1)
    assert abs(alpha - (-40 + math.sqrt(2800)) / 600) < 1e-12    # (the coefficients come from differences of trial values)
    # a steep parabola: every interpolated step is its minimiser 0.005, clipped from below to a tenth of the last trial
    seen = []
    alpha, f, trials = backtracking(lambda a: (seen.append(a), -a + 100 * a * a)[1], 0.0, -1.0)
    assert np.allclose(seen, [1.0, 0.1, 0.01, 0.005], rtol=1e-12, atol=0) and trials == 4 and alpha == seen[-1]


def test_backtracking_halves_on_non_finite_values_and_gives_up_after_the_cap():
    seen = []

    def phi(a):
        seen.append(a)
        return math.inf if a > 0.3 else (a - 0.3) ** 2
    alpha, f, trials = backtracking(phi, 0.09, -0.6)
    assert seen == [1.0, 0.5, 0.25] and alpha == 0.25 and trials == 3
    assert backtracking(lambda a: math.nan if a > 0.9 else -a, 0.0, -1.0)[0] == 0.5
    seen = []
    with pytest.raises(RuntimeError, match="50 trials"):
        backtracking(lambda a: (seen.append(a), 1.0)[1], 0.0, -1.0)
    assert len(seen) == 50 and all(0.1 * a <= b <= 0.5 * a for a, b in zip(seen, seen[1:]))


# ------------------------------------------------------------------------------------------ refusals, descriptors only
def cpu_basis(Ecut=5, functionals=("lda_x", "lda_c_pw"), kgrid=None, atoms=None, positions=None, **kw):
    lat, hgh, pos = dftk.silicon_cell()
    basis_kw = {k: kw.pop(k) for k in list(kw) if k in ("comm_pw", "comm_kpts")}
    model = dftk.model_DFT(lat, atoms or hgh, positions or pos, functionals=functionals, **kw)
    return dftk.PlaneWaveBasis(model, Ecut, kgrid or dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu", build_terms=False,
                               **basis_kw)


def test_direct_minimization_refusals_on_descriptors():
    base = cpu_basis()
    with pytest.raises(ValueError, match="temperature"):
        dftk.direct_minimization(cpu_basis(temperature=0.01))
    for rows in (3, 6):
        psi = [torch.zeros((rows, k.n_G), dtype=torch.complex128) for k in base.kpoints]
        with pytest.raises(ValueError, match="n_bands"):
            dftk.direct_minimization(base, psi=psi)
    with pytest.raises(ValueError, match="blocks"):
        dftk.direct_minimization(base, psi=[])
    Al = dftk.ElementPsp("Al", dftk.load_psp("Al", "lda"))
    odd = cpu_basis(atoms=[Al], positions=[np.zeros(3)])
    assert odd.model.n_electrons == 3
    with pytest.raises(ValueError, match="do not fill"):
        dftk.direct_minimization(odd)
    with pytest.raises(NotImplementedError, match="exact exchange"):
        dftk.direct_minimization(dftk.PlaneWaveBasis(dftk.model_HF(*dftk.silicon_cell()), 5,
                                                     dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu", build_terms=False))
    import hubbard_gen
    Si = dftk.ElementPsp("Si", psp=hubbard_gen.hubbard_psp())
    hub = cpu_basis(atoms=[Si, Si], extra_terms=[dftk.Hubbard((dftk.OrbitalManifold("Si", "3P"), 0.1))])
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.direct_minimization(hub)
    with pytest.raises(NotImplementedError, match="comm_pw"):
        dftk.direct_minimization(cpu_basis(comm_pw=KptComm(0, 2)))
    with pytest.raises(NotImplementedError, match="comm_kpts"):
        dftk.direct_minimization(cpu_basis(kgrid=dftk.MonkhorstPack((2, 1, 1)), comm_kpts=KptComm(0, 2)))
    with pytest.raises(ValueError, match="memory"):
        dftk.direct_minimization(base, memory=0)
    # in scope (collinear spin and PBE included), but descriptor-only: refused at the first device call, after every check
    assert check_supported(base) == 4
    assert check_supported(cpu_basis(magnetic_moments=[1.0, 1.0])) == 4
    assert check_supported(cpu_basis(functionals=("gga_x_pbe", "gga_c_pbe"))) == 4
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dftk.direct_minimization(base)
