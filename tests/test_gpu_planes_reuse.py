"""y-planes kept between the density pass and the next LOBPCG call (gamma_kernels.hip: gamma_density_bands,
gamma_apply_local_from_planes; lobpcg.cpp: the kept-A X branch of lobpcg_run_general).  The Gamma-real density pass over the
block the last call returned writes stage B's output into a per-k-block buffer; the next call, promised the same X, applies
(V_new - V_old) from stage C on and forms A_new X = (A_old X + (V_new - V_old) X) inv(R).  Same eigenpairs and the same SCF as
with DFTK_MI_PLANES_REUSE=0; every way the planes can go stale sends the call down the old path.

A launch group the density pass skipped (all weights zero) is FILLED at the start of the call: the planes of its pairs are
produced there from the caller's block (pack, stages A and B), the call still counts as started from kept planes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402

N_OCC = 32          # Si (2,2,2): 64 electrons
_cache = {}


def _planes(lib):
    n = C.c_int64()
    assert lib.dftk_mi_planes_reuse_count(C.byref(n)) == 0
    return n.value


def _ax(lib):
    n = C.c_int64()
    assert lib.dftk_mi_ax_reuse_count(C.byref(n)) == 0
    return n.value


def _setup(edge=None, supercell=(2, 2, 2)):
    """basis (Si (2,2,2), Ecut 10, Gamma, coarse_start=False), the two densities of test_gpu_ax_reuse and a 40-band start
    block; built once per cube edge (and cell)"""
    key = edge if supercell == (2, 2, 2) else (edge, supercell)
    if key not in _cache:
        assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
        lat, atoms, pos = dftk.silicon_cell(supercell)
        model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_pw"))
        if edge is not None:
            assert edge >= max(dftk.compute_fft_size(model, 10))
        basis = dftk.PlaneWaveBasis(model, 10, dftk.ExplicitKpoints([[0.0, 0.0, 0.0]], [1.0]), coarse_start=False,
                                    fft_size=None if edge is None else (edge, edge, edge))
        assert basis.kpoints[0].gamma_real
        rho1 = dftk.guess_density(basis)
        z = torch.arange(basis.fft_size[2], device="cuda", dtype=torch.float64)
        rho2 = rho1 * (1.0 + 0.2 * torch.cos(2 * np.pi * z / basis.fft_size[2]))[:, None, None]
        gen = torch.Generator(device="cuda").manual_seed(3)
        X0 = dftk.random_orbitals(basis, basis.kpoints[0], 40, gen)
        _cache[key] = (basis, rho1, rho2, X0)
    return _cache[key]


def _solve(basis, rho, X, reuse=False, n_conv_check=32):
    _, ham = dftk.energy_hamiltonian(basis, None, None, rho=rho)
    return dftk.lobpcg_hyper(ham[0], X, prec=dftk.PreconditionerTPA(ham[0]), tol=1e-7, n_conv_check=n_conv_check, reuse_AX=reuse)


def _density(basis, X, n_occ=N_OCC):
    occ = np.zeros(X.shape[0])
    occ[:n_occ] = 2.0
    return dftk.compute_density(basis, [X], [occ], real_symmetric=[True])


def _true_residuals(basis, rho, r):
    _, ham = dftk.energy_hamiltonian(basis, None, None, rho=rho)
    HX = ham[0] @ r.X
    return torch.linalg.norm(HX - r.X * torch.as_tensor(r.λ, device="cuda")[:, None], dim=1).cpu().numpy()


def _hand_over(monkeypatch, edge, M, fft_batch, n_occ=N_OCC):
    """LOBPCG on H[rho1], density of the returned X, LOBPCG on H[rho2] with the promise -- with the switch on and off.
    Returns {flag: (result, rise of the planes counter)} after the checks every shape has to pass."""
    basis, rho1, rho2, X0 = _setup(edge)
    lib = basis.lib
    out = {}
    try:
        if fft_batch is not None:
            assert lib.dftk_mi_basis_set_fft_batch(basis.handle, fft_batch) == 0
        for flag in ("1", "0"):
            monkeypatch.setenv("DFTK_MI_PLANES_REUSE", flag)
            r1 = _solve(basis, rho1, X0[:M])
            _density(basis, r1.X, n_occ)
            p0, a0 = _planes(lib), _ax(lib)
            r2 = _solve(basis, rho2, r1.X, reuse=True)
            assert _ax(lib) - a0 == 1
            out[flag] = (r2, _planes(lib) - p0)
    finally:
        monkeypatch.delenv("DFTK_MI_PLANES_REUSE", raising=False)
        assert lib.dftk_mi_basis_set_fft_batch(basis.handle, 32) == 0
    a, b = out["1"][0], out["0"][0]
    assert out["1"][1] == 1 and out["0"][1] == 0
    assert a.converged and b.converged
    np.testing.assert_allclose(a.λ[:32], b.λ[:32], rtol=0, atol=1e-9)
    true = _true_residuals(basis, rho2, a)
    assert true[:32].max() < 1.05e-7, true[:32].max()
    return out


def test_same_eigenpairs_and_the_right_AX(monkeypatch):
    _hand_over(monkeypatch, None, 40, None)


# 39 bands: the last pair holds one band.  fft_batch 3: seven launch groups of the 20 pairs, the last one ragged.  Cube edge 48:
# register-resident z kernels (as the default 45); 49 = 7 * 7 has no entry in REG_SIZES: the LDS-pass k_zpass / k_zdensity.
@pytest.mark.parametrize("edge,M,fft_batch", [(None, 39, None), (None, 40, 3), (None, 39, 3), (48, 39, 3), (49, 40, 3), (49, 39, None)])
def test_slots_and_groups(monkeypatch, edge, M, fft_batch):
    _hand_over(monkeypatch, edge, M, fft_batch)


@pytest.mark.parametrize("M", [40, 39])
def test_groups_the_density_pass_skipped_are_filled(monkeypatch, M):
    """fft_batch 3, 32 occupied bands: pairs 18 and 19 (bands 36 ..) form the last launch group, all of its weights are zero
    and the density pass skips it.  This implementation FILLS the missing planes at the start of the call (it does not
    decline): the counter rises, the criteria of the first test hold, and the A X the call carried is right in the filled
    columns too.  Those bands (36 ..) are outside n_conv_check and still active when the call ends, so the residual norm the
    solver reports for them is ||A X - X lambda|| with the A X it CARRIED from the start (only ever recombined, never
    re-applied); the true residual uses a full H X.  The two differ by the round-off of a few dozen block updates of vectors
    of norm ||H|| ~ 10 Ha, i.e. ~1e-13; a wrong (V_new - V_old) X would show at the size of the potential change, ~1e-2.
    Bound 1e-9, for every column that reports a residual at the last iteration.  (A column that was locked earlier reports
    0: for those the tolerance itself is the bound.  Locking takes a prefix of the converged columns inside n_conv_check, so
    the filled columns 36 .. always report.)"""
    out = _hand_over(monkeypatch, None, M, 3)
    basis, _, rho2, _ = _setup(None)
    a = out["1"][0]
    true = _true_residuals(basis, rho2, a)
    rep = np.asarray(a.residual_norms)
    reported = rep > 0.0          # (a column of the filled group may happen to converge: it still reports its residual)
    assert reported[36:].all(), rep
    assert np.abs(true - rep)[reported].max() < 1e-9, (true, rep)
    assert np.abs(true - rep)[~reported].max() < 1.05e-7


def _stale(monkeypatch, between, second_X=lambda r1: r1.X, setup=(None,), M=40, n_occ=N_OCC, n_conv_check=32):
    basis, rho1, rho2, X0 = _setup(*setup)
    lib = basis.lib
    monkeypatch.delenv("DFTK_MI_PLANES_REUSE", raising=False)
    r1 = _solve(basis, rho1, X0[:M], n_conv_check=n_conv_check)
    _density(basis, r1.X, n_occ)
    between(basis, r1)
    p0 = _planes(lib)
    r2 = _solve(basis, rho2, second_X(r1), reuse=True, n_conv_check=n_conv_check)
    assert _planes(lib) == p0 and r2.converged
    return r2


def test_stale_density_of_another_tensor(monkeypatch):
    _stale(monkeypatch, lambda basis, r1: _density(basis, r1.X.clone()))


def test_stale_another_band_count(monkeypatch):
    _stale(monkeypatch, lambda basis, r1: None, second_X=lambda r1: r1.X[:36])


def test_stale_fft_batch_changed(monkeypatch):
    basis = _setup(None)[0]
    try:
        _stale(monkeypatch, lambda basis, r1: basis.lib.dftk_mi_basis_set_fft_batch(basis.handle, 3))
    finally:
        assert basis.lib.dftk_mi_basis_set_fft_batch(basis.handle, 32) == 0


def test_stale_gamma_real_off_and_on(monkeypatch):
    def toggle(basis, r1):
        h = basis.kpoints[0].handle
        assert basis.lib.dftk_mi_kblock_set_gamma_real(h, 0) == 0
        assert basis.lib.dftk_mi_kblock_set_gamma_real(h, 1) == 0
    _stale(monkeypatch, toggle)


def test_stale_small_driver_call_in_between(monkeypatch):
    """The small-block driver never takes a Gamma-real block, so the format is switched off around a 6-band call: it binds the
    workspace (Lob::bind), which drops the kept A X and the planes with it."""
    def small_call(basis, r1):
        lib, h = basis.lib, basis.kpoints[0].handle
        a0, b0 = C.c_int64(), C.c_int64()
        a1, b1 = C.c_int64(), C.c_int64()
        assert lib.dftk_mi_lobpcg_small_stats(C.byref(a0), C.byref(b0)) == 0
        assert lib.dftk_mi_kblock_set_gamma_real(h, 0) == 0
        try:
            r = _solve(basis, _setup(None)[1], r1.X[:6].clone(), n_conv_check=None)
        finally:
            assert lib.dftk_mi_kblock_set_gamma_real(h, 1) == 0
        assert lib.dftk_mi_lobpcg_small_stats(C.byref(a1), C.byref(b1)) == 0
        assert a1.value - a0.value == 1 and r.converged
    basis = _setup(None)[0]
    a0 = _ax(basis.lib)
    _stale(monkeypatch, small_call)
    assert _ax(basis.lib) == a0


def _stale_small(monkeypatch, between):
    """The two drop events below on the smallest shape that still has every edge: Si primitive cell, cube 24^3 (a few hundred
    plane waves), 7 bands (the last pair holds one band), fft_batch 3 (two launch groups, the second ragged), 4 occupied.
    Returns the rise of the A X counter over the promised call."""
    basis = _setup(24, (1, 1, 1))[0]
    lib = basis.lib
    counts = {}

    def counted(basis, r1):
        between(basis, r1)
        counts["ax"] = _ax(lib)
    try:
        assert lib.dftk_mi_basis_set_fft_batch(basis.handle, 3) == 0
        _stale(monkeypatch, counted, setup=(24, (1, 1, 1)), M=7, n_occ=4, n_conv_check=4)
    finally:
        assert lib.dftk_mi_basis_set_fft_batch(basis.handle, 32) == 0
    return _ax(lib) - counts["ax"]


def test_stale_density_through_the_complex_entry_point(monkeypatch):
    """A density pass over the very tensor the call returned, but not as real-symmetric orbitals: it keeps no planes, and the
    ones the real-symmetric pass before it kept are switched off.  The kept A X is untouched."""
    def complex_pass(basis, r1):
        occ = np.zeros(r1.X.shape[0])
        occ[:4] = 2.0
        dftk.compute_density(basis, [r1.X], [occ], real_symmetric=[False])
    assert _stale_small(monkeypatch, complex_pass) == 1


def test_stale_projectors_rebound(monkeypatch):
    """New projectors (here: the same ones, bound again) between the density pass and the promised call drop the kept A X, the
    promise and the planes: a full application."""
    def rebind(basis, r1):
        T = basis.terms
        D = np.asfortranarray(T.D.cpu().numpy() if torch.is_tensor(T.D) else T.D, dtype=np.float64)
        assert basis.lib.dftk_mi_kblock_set_projectors(basis.kpoints[0].handle, T.P[0].shape[0], T.P[0].data_ptr(),
                                                       T.P[0].stride(0), D.ctypes.data) == 0
    assert _stale_small(monkeypatch, rebind) == 0


def test_scf_with_and_without_the_kept_planes(monkeypatch):
    basis = _setup(None)[0]
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("DFTK_MI_PLANES_REUSE", flag)
        c0 = _planes(basis.lib)
        r = dftk.self_consistent_field(basis, tol=1e-9, seed=2)
        assert r["converged"]
        res[flag] = (r["energies"].total, r["n_iter"], _planes(basis.lib) - c0, r["eigenvalues"][0][:r["n_bands_converge"]].copy())
    monkeypatch.delenv("DFTK_MI_PLANES_REUSE", raising=False)
    assert res["1"][2] >= res["1"][1] - 3 and res["0"][2] == 0
    assert abs(res["1"][0] - res["0"][0]) < 1e-9 * 16
    np.testing.assert_allclose(res["1"][3], res["0"][3], rtol=0, atol=1e-7)
    assert abs(res["1"][1] - res["0"][1]) <= 8
