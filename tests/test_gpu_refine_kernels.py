"""``dftk_mi_refinement_metric_solve`` at the C ABI (ctypes, device memory from torch) against the dense solve of
tests/refine_twin.py.

Shapes: the element-wise kernels of the solver work on row tiles of EW_ROWS = 1024 rows of one column (ew_device.h; the CG
kernels of response_kernels.hip on RESP_NT * RESP_UNR = 1024 rows as well), so the blocks have 1023, 1024 and 1025 rows
(one row fewer than, exactly as many as, and one row more than the tile: the last forces a second, one-row tile); 1, 4 and
33 columns; leading dimensions above the rows with NaN padding on all three blocks.  The orbitals are orthonormal random
columns, the right-hand side has a component along them that the solve must project out.

Bound: the comparison is against a direct dense solve and the CG stops at 100 ulp, so the error is that of the attainable
accuracy of CG in fp64, some eps * condition number; METRIC_MEASURED is the largest relative error
max_c |x_c - x_c*| / |x_c*| seen on the MI355X over all shapes, the assertion ten times it and never more than 1e-10.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402

import refine_twin as twin  # noqa: E402
from test_gpu_kernels import Basis, KBlock, LATTICE, dev  # noqa: E402

ROW_TILE = 1024                       # EW_ROWS of ew_device.h
METRIC_MEASURED = 1.8e-14             # 1.2e-15 (1 column), 2.0e-15 (4), 1.7e-14 (33 columns), 4 to 9 CG passes
METRIC_BOUND = min(10 * METRIC_MEASURED, 1e-10)
TOL = 100 * 2.0 ** -52                # the reference's 100 eps
FFT = (12, 12, 12)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


_CASES = {}


def case(lib, n_rows, n_cols):
    """the n_rows plane waves of lowest kinetic energy of the silicon cell on a 12^3 cube, n_cols orthonormal random
    columns, a random right-hand side of unit-order columns, and the twin's dense solution; built once per shape"""
    key = (n_rows, n_cols)
    if key not in _CASES:
        nx, ny, nz = FFT
        lin = np.arange(nx * ny * nz, dtype=np.int64)
        G = twin.G_of_mapping(lin, FFT).astype(float)
        B = 2 * np.pi * np.linalg.inv(np.asarray(LATTICE, dtype=float).T)
        kin_all = 0.5 * np.sum((G @ B.T) ** 2, axis=1)
        mapping = np.sort(np.argsort(kin_all, kind="stable")[:n_rows]).astype(np.int64)
        kin = kin_all[mapping]
        rng = np.random.default_rng(1000 * n_rows + n_cols)
        psi, _ = np.linalg.qr(rng.standard_normal((n_rows, n_cols)) + 1j * rng.standard_normal((n_rows, n_cols)))
        res = (rng.standard_normal((n_rows, n_cols)) + 1j * rng.standard_normal((n_rows, n_cols))) / np.sqrt(n_rows)
        res = res + psi @ (rng.standard_normal((n_cols, n_cols)) + 0.5j)          # a component along psi
        bs = Basis(lib, nx, ny, nz, 1.0)
        kb = KBlock(lib, bs, mapping, kin)
        _CASES[key] = dict(bs=bs, kb=kb, kin=kin, psi=psi, res=res, ref=twin.metric_solve_dense(psi, kin, res))
    return _CASES[key]


def padded(A, ld):
    n, m = A.shape
    buf = np.full((m, ld), complex(np.nan, np.nan))
    buf[:, :n] = A.T
    return dev(buf)


MAXITER = 20                          # the reference's budget (refine.jl:66) and the Python default


def solve(lib, c, tol=TOL, maxiter=MAXITER, res=None):
    psi, res = c["psi"], c["res"] if res is None else res
    n, m = psi.shape
    pd, rd = padded(psi, n + 3), padded(res, n + 6)
    out = dev(np.full((m, n + 9), complex(np.nan, np.nan)))
    iters = np.full(m, -7, dtype=np.int32)
    rn = np.full(m, np.nan)
    torch.cuda.synchronize()
    check(lib.dftk_mi_refinement_metric_solve(c["kb"].h, m, pd.data_ptr(), n + 3, rd.data_ptr(), n + 6, tol, maxiter,
                                              out.data_ptr(), n + 9, iters.ctypes.data, rn.ctypes.data))
    c["bs"].sync()
    got = out.cpu().numpy()
    assert np.isnan(got[:, n:]).all()                       # the padding rows of the output are untouched
    return got[:, :n].T, iters, rn


@pytest.mark.parametrize("n_cols", [1, 4, 33])
@pytest.mark.parametrize("n_rows", [ROW_TILE - 1, ROW_TILE, ROW_TILE + 1])
def test_metric_solve_against_the_dense_solve(lib, n_rows, n_cols):
    c = case(lib, n_rows, n_cols)
    x, iters, rn = solve(lib, c)
    assert np.isfinite(x).all()
    ref = c["ref"]
    err = max(np.linalg.norm(x[:, j] - ref[:, j]) / np.linalg.norm(ref[:, j]) for j in range(n_cols))
    overlap = np.abs(c["psi"].conj().T @ x).max()
    print(f"\nmetric solve {n_rows} x {n_cols}: rel err {err:.3e} (bound {METRIC_BOUND:.1e}), |psi' x| {overlap:.2e}, "
          f"iterations {iters.min()} .. {iters.max()}, residual norms up to {rn.max():.2e}")
    assert err <= METRIC_BOUND
    assert overlap <= 1e-13
    assert np.all(iters >= 1) and np.all(iters <= MAXITER)
    assert np.all(rn <= TOL)                                # every column converged
    # M_n x_n = P res_n, recomputed on the host from the dense M_n
    P = twin.proj_perp(c["psi"])
    for j in range(n_cols):
        r = twin.metric_dense(c["psi"], c["kin"], j) @ x[:, j] - P @ c["res"][:, j]
        assert np.linalg.norm(r) <= 1e-10 * np.linalg.norm(P @ c["res"][:, j])


def test_a_right_hand_side_inside_the_span_of_psi_gives_zero(lib):
    c = case(lib, ROW_TILE + 1, 4)
    x, iters, rn = solve(lib, c, res=c["psi"] @ np.diag([1.0, 2.0j, -1.0, 0.5]))
    assert np.abs(x).max() <= 1e-13 and np.all(rn <= 1e-13)


def host_syncs(lib):
    n = C.c_int64()
    check(lib.dftk_mi_launch_count(None, C.byref(n)))
    return n.value


def test_one_host_synchronisation_per_cg_pass(lib):
    c = case(lib, ROW_TILE + 1, 4)
    counts = {}
    for K in (6, 3, 6):                                     # the first call sizes the workspace
        before = host_syncs(lib)
        _, iters, rn = solve(lib, c, tol=0.0, maxiter=K)
        counts[K] = host_syncs(lib) - before
        assert np.all(iters == K) and np.all(rn > 0.0)
    print(f"\nhost synchronisations: K=3 {counts[3]}, K=6 {counts[6]}")
    assert counts[6] - counts[3] == 3


def test_maxiter_one_reports_non_convergence(lib):
    c = case(lib, ROW_TILE, 4)
    x, iters, rn = solve(lib, c, maxiter=1)
    assert np.isfinite(x).all() and np.abs(c["psi"].conj().T @ x).max() <= 1e-13
    assert np.all(iters == 1) and np.all(rn > TOL)          # reported, and the call returned 0


def test_converged_columns_are_frozen(lib):
    """A column whose right-hand side is zero converges at the start (iteration count 1) and stays exactly zero while the
    others iterate to their own solutions (the columns do not couple)."""
    c = case(lib, ROW_TILE + 1, 4)
    res = c["res"].copy()
    res[:, 2] = 0.0
    x, iters, rn = solve(lib, c, res=res)
    assert iters[2] == 1 and rn[2] == 0.0 and np.all(x[:, 2] == 0.0)
    for j in (0, 1, 3):
        assert iters[j] > 1 and rn[j] <= TOL
        assert np.linalg.norm(x[:, j] - c["ref"][:, j]) <= METRIC_BOUND * np.linalg.norm(c["ref"][:, j])


def test_metric_solve_bad_arguments(lib):
    c = case(lib, ROW_TILE - 1, 1)
    n = ROW_TILE - 1
    pd, rd = padded(c["psi"], n), padded(c["res"], n)
    out = dev(np.full((1, n), 7.0 + 0j))
    iters, rn = np.zeros(1, dtype=np.int32), np.zeros(1)
    torch.cuda.synchronize()
    f = lib.dftk_mi_refinement_metric_solve
    args = lambda **kw: (c["kb"].h, kw.get("n", 1), pd.data_ptr(), kw.get("ld_psi", n), rd.data_ptr(), kw.get("ld_res", n),  # noqa: E731
                         kw.get("tol", TOL), kw.get("maxiter", 20), out.data_ptr(), kw.get("ld_out", n), iters.ctypes.data,
                         rn.ctypes.data)
    for kw in (dict(n=-1), dict(ld_psi=n - 1), dict(ld_res=n - 1), dict(ld_out=n - 1), dict(maxiter=-1), dict(tol=-1.0),
               dict(tol=float("nan"))):
        assert f(*args(**kw)) == -1, kw
    c["bs"].sync()
    assert np.all(out.cpu().numpy() == 7.0)
    assert f(*args(n=0)) == 0
