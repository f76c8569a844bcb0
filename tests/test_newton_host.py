"""Host-only tests of Newton's method and its tangent-space CG (no device):

* the twin of the kernels (tests/newton_twin.py) on a dense symmetric positive definite operator restricted to a subspace,
  against ``numpy.linalg.solve`` of the projected system -- the reference of tests/test_gpu_newton_kernels.py is itself right;
* the twin cut into the pieces of the C ABI (``CgScalars``) against the recursion in one piece;
* ``apply_Omega_dense`` + ``apply_K_dense`` of tests/refine_twin.py driven by the twin's CG with the projected
  Teter-Payne-Allan preconditioner and the k-weighted inner product, against ``solve_OmegaPlusK_dense`` of the same file;
* the ``negative_curvature`` branch on an indefinite operator;
* every refusal of ``newton``, ``solve_OmegaPlusK_cg`` and ``TangentSpace`` on descriptor-only bases (``device="cpu"``), raised
  before any device work; ``solve_OmegaPlusK()`` itself still refuses by name.
"""
import numpy as np
import pytest

import dftk_jl_amd as dftk
from dftk_jl_amd import KptComm
from dftk_jl_amd.newton import check_supported
import newton_twin as twin
import refine_twin

torch = pytest.importorskip("torch")


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ------------------------------------------------------------------------------------------ the twin
def subspace_problem(rng, shapes, n_out=2):
    """a dense SPD operator on the packed vectors (as real vectors of both parts), a projector P onto the complement of
    ``n_out`` random directions, a diagonal preconditioner and a right-hand side"""
    n = sum(2 * r * c for r, c in shapes)
    M = rng.standard_normal((n, n))
    A = M @ M.T / n + np.diag(np.linspace(1.0, 30.0, n))
    Q = np.linalg.qr(rng.standard_normal((n, n_out)))[0]
    P = np.eye(n) - Q @ Q.T

    def flat(v):
        return np.concatenate([np.concatenate([np.asarray(b).real.reshape(-1), np.asarray(b).imag.reshape(-1)]) for b in v])

    def unflat(x):
        out, at = [], 0
        for r, c in shapes:
            m = r * c
            out.append((x[at:at + m] + 1j * x[at + m:at + 2 * m]).reshape(r, c))
            at += 2 * m
        return out
    return A, P, flat, unflat


@pytest.mark.parametrize("real", [twin.LD, np.float64])
def test_twin_cg_solves_the_projected_system(real):
    rng = np.random.default_rng(11)
    shapes = [(7, 2), (5, 3)]
    A, P, flat, unflat = subspace_problem(rng, shapes)
    # unit weights: the inner product is the Euclidean one of the flattened vectors, in which P A P is symmetric
    w = [1.0, 1.0]
    dinv = 1.0 / np.diag(A)
    b = unflat(P @ rng.standard_normal(A.shape[0]))
    res = twin.cg(lambda v: unflat(P @ (A @ (P @ flat(v)))), b, w, precon=lambda v: unflat(P @ (dinv * (P @ flat(v)))),
                  proj=lambda v: unflat(P @ flat(v)), tol=1e-13, maxiter=200, real=real)
    assert res["converged"] and not res["negative_curvature"] and res["n_iter"] < 80
    # the projected system: x in the range of P with P A P x = b, i.e. (P A P + (1 - P)) x = b
    want = np.linalg.solve(P @ A @ P + (np.eye(A.shape[0]) - P), flat(b))
    got = flat(res["x"]).astype(float)
    assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()
    assert np.abs((np.eye(A.shape[0]) - P) @ got).max() < 1e-13            # the iterate stayed in the range of P
    assert res["residual_norms"][-1] <= 1e-13 and len(res["residual_norms"]) == res["n_iter"]


def test_weighted_inner_product_and_the_pieces_of_the_abi():
    """with unequal weights w_b a block-diagonal operator is self-adjoint in <., .>_w; the recursion cut into dot /
    update_xr / update_p / read reproduces the one-piece recursion number by number"""
    rng = np.random.default_rng(12)
    shapes = [(9, 2), (6, 1), (4, 3)]
    w = [0.2, 0.5, 0.3]
    ops = []
    for r, c in shapes:
        M = crandn(rng, r, r)
        ops.append(M @ M.conj().T / r + np.diag(np.linspace(1, 4, r)))
    apply_A = lambda v: [H @ np.asarray(x) for H, x in zip(ops, v)]                       # noqa: E731
    pre = lambda v: [np.asarray(x) / np.diag(H).real[:, None] for H, x in zip(ops, v)]    # noqa: E731
    b = [crandn(rng, r, c) for r, c in shapes]
    x, y = [crandn(rng, r, c) for r, c in shapes], [crandn(rng, r, c) for r, c in shapes]
    assert abs(twin.wdot(x, apply_A(y), w) - twin.wdot(apply_A(x), y, w)) < 1e-14 * abs(twin.wdot(x, apply_A(y), w)) + 1e-15
    for real in (twin.LD, np.float64):
        one = twin.cg(apply_A, b, w, precon=pre, tol=1e-12, real=real)
        two = twin.cg_in_pieces(apply_A, b, w, precon=pre, tol=1e-12, real=real)
        assert one["converged"] and two["converged"] and one["n_iter"] == two["n_iter"]
        assert all(np.array_equal(a, c) for a, c in zip(one["x"], two["x"]))
        assert [float(v) for v in one["residual_norms"]] == [float(v) for v in two["residual_norms"]]
    want = [np.linalg.solve(H, rhs) for H, rhs in zip(ops, b)]
    assert max(np.abs(np.asarray(a, dtype=complex) - c).max() for a, c in zip(one["x"], want)) < 1e-11
    # miniter: a converged start (b = 0) still begins `miniter` iterations before it may stop
    zero = [np.zeros(s, dtype=complex) for s in shapes]
    assert twin.cg(apply_A, zero, w, tol=1e-12)["n_iter"] == 1


def test_negative_curvature_ends_the_twin_solve():
    rng = np.random.default_rng(13)
    n = 12
    H = np.diag(np.concatenate([[-2.0], np.linspace(1, 3, n - 1)])).astype(complex)
    b = [crandn(rng, n, 1)]
    for run in (twin.cg, twin.cg_in_pieces):
        res = run(lambda v: [H @ np.asarray(v[0])], b, [1.0], tol=1e-12, maxiter=50)
        assert res["negative_curvature"] and not res["converged"] and res["n_iter"] < 50
    # a definite operator of the same size never raises the flag
    res = twin.cg(lambda v: [np.abs(H) @ np.asarray(v[0])], b, [1.0], tol=1e-12, maxiter=50)
    assert res["converged"] and not res["negative_curvature"]


# ------------------------------------------------------------------------------------------ (Omega + K) of the dense twin
def synthetic_side(rng):
    """two "k-points" on a 6 x 5 x 7 grid: spheres of the lowest plane waves, H_k = kinetic + a small Hermitian matrix, a
    weak negative f_xc, the Hartree kernel of a cubic cell; psi_k = the two lowest eigenvectors of H_k, so that Omega has
    the gaps of H_k as eigenvalues and Omega + K is positive definite"""
    fft = (6, 5, 7)
    L = 6.0
    recip = 2 * np.pi / L * np.eye(3)
    G_all = refine_twin.G_of_mapping(np.arange(np.prod(fft)), fft).astype(float)
    side = dict(fft_size=fft, volume=L ** 3, recip=recip, weights=[0.25, 0.75], mappings=[], H=[], kin=[],
                fxc=-0.05 * (1.0 + rng.random((fft[2], fft[1], fft[0]))))
    psi = []
    for kc, n_G in (((0.0, 0.0, 0.0), 27), ((0.25, 0.0, 0.1), 23)):
        kin_all = 0.5 * np.sum(((G_all + np.array(kc)) @ recip.T) ** 2, axis=1)
        mapping = np.sort(np.argsort(kin_all, kind="stable")[:n_G])
        kin = kin_all[mapping]
        M = crandn(rng, n_G, n_G)
        H = np.diag(kin) + 0.05 * (M + M.conj().T)
        side["mappings"].append(mapping)
        side["kin"].append(kin)
        side["H"].append(H)
        psi.append(np.linalg.eigh(H)[1][:, :2])
    return side, psi


def test_twin_cg_on_the_dense_hessian_against_the_dense_solve():
    rng = np.random.default_rng(14)
    side, psi = synthetic_side(rng)
    occ = [np.full(2, 2.0)] * 2
    w = side["weights"]
    P = [refine_twin.proj_perp(p) for p in psi]
    mean_kin = [np.sum(k[:, None] * np.abs(p) ** 2, axis=0) for k, p in zip(side["kin"], psi)]

    def op(d):
        return [a + b for a, b in zip(refine_twin.apply_Omega_dense(side, d, psi), refine_twin.apply_K_dense(side, d, psi, occ))]

    def proj(v):
        return [Pk @ np.asarray(x, dtype=complex) for Pk, x in zip(P, v)]

    def precon(v):          # P T^-1 P with the Teter-Payne-Allan form mean_kin / (mean_kin + kin) per column
        return proj([mk[None, :] / (mk[None, :] + k[:, None]) * x for mk, k, x in zip(mean_kin, side["kin"], proj(v))])

    # Omega + K is self-adjoint with respect to the k-weighted inner product (and not the unweighted one: K couples the blocks)
    x, y = proj([crandn(rng, *p.shape) for p in psi]), proj([crandn(rng, *p.shape) for p in psi])
    sym = abs(twin.wdot(x, op(y), w, np.float64) - twin.wdot(op(x), y, w, np.float64))
    assert sym < 1e-13 * abs(twin.wdot(x, op(y), w, np.float64))
    rhs = [crandn(rng, *p.shape) for p in psi]
    res = twin.cg(op, [-v for v in proj(rhs)], w, precon=precon, proj=proj, tol=1e-13, maxiter=200, real=np.float64)
    assert res["converged"] and not res["negative_curvature"]
    want = refine_twin.solve_OmegaPlusK_dense(side, psi, rhs, occ)
    err = max(np.abs(a - b).max() for a, b in zip(res["x"], want)) / max(np.abs(b).max() for b in want)
    assert err < 1e-10, err
    # ... and the answer solves the equation it is defined by
    back = op(res["x"])
    assert max(np.abs(a + b).max() for a, b in zip(back, proj(rhs))) < 1e-11


# ------------------------------------------------------------------------------------------ refusals, descriptors only
def cpu_basis(Ecut=5, functionals=("lda_x", "lda_c_pw"), kgrid=None, atoms=None, positions=None, **kw):
    lat, hgh, pos = dftk.silicon_cell()
    basis_kw = {k: kw.pop(k) for k in list(kw) if k in ("comm_pw", "comm_kpts")}
    model = dftk.model_DFT(lat, atoms or hgh, positions or pos, functionals=functionals, **kw)
    return dftk.PlaneWaveBasis(model, Ecut, kgrid or dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu", build_terms=False,
                               **basis_kw)


def blocks(basis, rows=4):
    return [torch.zeros((rows, k.n_G), dtype=torch.complex128) for k in basis.kpoints]


def refused_cases():
    import hubbard_gen
    Si = dftk.ElementPsp("Si", psp=hubbard_gen.hubbard_psp())
    Al = dftk.ElementPsp("Al", dftk.load_psp("Al", "lda"))
    hf = dftk.PlaneWaveBasis(dftk.model_HF(*dftk.silicon_cell()), 5, dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu",
                             build_terms=False)
    return [
        (cpu_basis(functionals=("gga_x_pbe", "gga_c_pbe")), NotImplementedError, "GGA"),
        (cpu_basis(functionals=("mgga_x_scan", "mgga_c_scan")), NotImplementedError, "meta-GGA"),
        (cpu_basis(magnetic_moments=[1.0, 1.0]), NotImplementedError, "collinear spin"),
        (hf, NotImplementedError, "exact exchange"),
        (cpu_basis(atoms=[Si, Si], extra_terms=[dftk.Hubbard((dftk.OrbitalManifold("Si", "3P"), 0.1))]),
         NotImplementedError, "Hubbard"),
        (cpu_basis(comm_pw=KptComm(0, 2)), NotImplementedError, "comm_pw"),
        (cpu_basis(kgrid=dftk.MonkhorstPack((2, 1, 1)), comm_kpts=KptComm(0, 2)), NotImplementedError, "comm_kpts"),
        (cpu_basis(temperature=0.01), ValueError, "temperature"),
        (cpu_basis(atoms=[Al], positions=[np.zeros(3)]), ValueError, "do not fill"),
    ]


def test_refusals_on_descriptors():
    occ4 = lambda b: [np.full(4, 2.0) for _ in b.kpoints]            # noqa: E731
    for basis, exc, word in refused_cases():
        with pytest.raises(exc, match=word):
            dftk.newton(basis, blocks(basis))
        with pytest.raises(exc, match=word):
            dftk.solve_OmegaPlusK_cg(basis, blocks(basis), blocks(basis), occ4(basis))
        with pytest.raises(exc, match=word):
            dftk.TangentSpace(basis, blocks(basis), occ4(basis))
    base = cpu_basis()
    for rows in (3, 6):
        with pytest.raises(ValueError, match="select_occupied_orbitals"):
            dftk.newton(base, blocks(base, rows))
    with pytest.raises(ValueError, match="blocks"):
        dftk.newton(base, [])
    with pytest.raises(ValueError, match="psi0"):
        dftk.newton(base, None)
    with pytest.raises(ValueError, match="cache_realspace"):
        dftk.newton(base, blocks(base), cache_realspace="yes")
    partial = [np.array([2.0, 2.0, 2.0, 1.0])]
    with pytest.raises(ValueError, match="full occupation"):
        dftk.solve_OmegaPlusK_cg(base, blocks(base), blocks(base), partial)
    with pytest.raises(ValueError, match="full occupation"):
        dftk.TangentSpace(base, blocks(base), partial)
    # in scope, but descriptor-only: refused at the first device call, after every check
    assert check_supported(base, blocks(base)) == 4
    for call in (lambda: dftk.newton(base, blocks(base)),
                 lambda: dftk.solve_OmegaPlusK_cg(base, blocks(base), blocks(base), occ4(base)),
                 lambda: dftk.TangentSpace(base, blocks(base), occ4(base))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_solve_OmegaPlusK_itself_still_refuses():
    with pytest.raises(NotImplementedError, match="solve_OmegaPlusK_split"):
        dftk.solve_OmegaPlusK()
    for name in ("newton", "solve_OmegaPlusK_cg", "TangentSpace", "apply_OmegaPlusK"):
        assert callable(getattr(dftk, name))
