"""The density response on the device (dftk.jl_amd/response.py, csrc/sternheimer.cpp, csrc/response_kernels.hip) against a
yardstick the test builds itself: the sum over states with the FULL spectrum (E_n, psi_n) of every dense H_k,

    d_rho(r) = sum_k w_k sum_{m,n} r_mn Re[conj(psi_m(r)) psi_n(r) M_nm] + LDOS(r) <LDOS|dV> / DOS,
    M_nm = <psi_n|dV|psi_m>,  r_mn = (f_m - f_n) / (E_m - E_n)  (f'/T on the diagonal and for degenerate pairs, 0 at T = 0),

the LDOS term only when some band is fractionally occupied.  The dense H_k comes from ``mul_`` applied to the identity, its
spectrum from numpy.linalg.eigh: the orbitals handed to the response layer are exact eigenvectors, SCF convergence does not
enter (tests 2-9).  The cell is displaced silicon at Ecut 5 on the reducible 2 x 2 x 2 mesh (fft 18^3, n_G ~ 137 - 150, 8
k-points); on the host this restatement agrees with central differences of the density of dense H +- h dV to 4e-10.

Bounds.  CHI0_MEASURED is the relative maximum error of ``apply_chi0`` against the sum over states measured on the MI355X
with the Sternheimer tolerance 1e-10 on the normalised right-hand side (the worst of tests 2-4; every test prints its own
figure); the tests assert ten times it, and never more than 1e-6.  KERNEL_MEASURED and SPLIT_MEASURED likewise for
``apply_kernel`` against central differences of the potential and for ``solve_OmegaPlusK_split`` against central
differences of the SCF density.  In that last comparison the error at h = 1e-3 is the h^2 truncation error of the yardstick
(3.0e-7) plus the convergence error of its two SCF densities divided by 2 h (0.4e-7; it doubles when h halves): from
h = 1e-3 to h = 5e-4 the whole error falls 2.2-fold, the truncation part of it fourfold."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd.mixing import occupation_derivative  # noqa: E402
from dftk_jl_amd.scf import _smear  # noqa: E402
from dftk_jl_amd.terms import local_potential_fused  # noqa: E402

CHI0_MEASURED = 4.2e-10       # T = 0: 3.7e-10, with extra bands 4.2e-10, T = 0.03: 2.7e-10
CHI0_TOL = min(1e-6, 10 * CHI0_MEASURED)
KERNEL_MEASURED = 1.3e-9      # lda_x 1.2e-9, lda_c_vwn 1.0e-10, lda_c_pw 1.0e-10, Hartree alone 1.3e-11
KERNEL_TOL = min(1e-6, 10 * KERNEL_MEASURED)
SPLIT_MEASURED = 3.4e-7       # h = 1e-3: 3.3e-7, h = 5e-4: 1.5e-7
SPLIT_TOL = min(1e-4, 10 * SPLIT_MEASURED)

LDA = ("lda_x", "lda_c_vwn")
POS = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]
TEMP = 0.03
THR = 1e-12
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------ set-up shared by the tests
def make_basis(temperature=0.0, positions=POS, symmetries=False, kgrid=None, fft_size=None, functionals=LDA, **kw):
    lat, atoms, _ = dftk.silicon_cell()
    extra = dict(temperature=temperature, smearing="fermi_dirac") if temperature > 0 else {}
    model = dftk.model_DFT(lat, atoms, positions, functionals=functionals, symmetries=symmetries, **extra)
    return dftk.PlaneWaveBasis(model, 5, kgrid or dftk.MonkhorstPack((2, 2, 2)), fft_size=fft_size, device=DEV, **kw)


def cosine_potential(basis, terms):
    """sum_j a_j cos(2 pi G_j . r + phi_j) on the (nz, ny, nx) grid; terms = [(a, (gx, gy, gz), phi)]."""
    nx, ny, nz = basis.fft_size
    z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
    v = np.zeros((nz, ny, nx))
    for a, g, phi in terms:
        v += a * np.cos(2 * np.pi * (g[0] * x + g[1] * y + g[2] * z) + phi)
    return v


DV1 = [(0.30, (1, 0, 0), 0.3), (0.20, (0, 1, 1), 1.1), (0.15, (1, -1, 0), 0.0), (0.10, (2, 1, 0), 2.0)]
DV2 = [(0.25, (0, 0, 1), 0.7), (0.20, (1, 1, 0), 0.2), (0.10, (1, 0, -1), 1.5), (0.05, (0, 2, 1), 0.4)]


def ground_hamiltonian(basis):
    rho = dftk.guess_density(basis)
    _, ham = dftk.energy_hamiltonian(basis, None, None, rho=rho, only_hamiltonian=True)
    return rho, ham


def dense_spectrum(basis, ham):
    """[(E, V)] per k-point: H_k = mul_ applied to the identity (row i of the result = H e_i), numpy.linalg.eigh."""
    out = []
    for Hk in ham:
        n = Hk.n_G
        eye = torch.eye(n, dtype=torch.complex128, device=DEV)
        H = Hk.mul_(torch.empty_like(eye), eye).cpu().numpy().T
        assert np.abs(H - H.conj().T).max() < 1e-12
        out.append(np.linalg.eigh((H + H.conj().T) / 2))
    return out


def to_block(V):
    """columns of a host matrix -> band-major device block"""
    return torch.from_numpy(np.ascontiguousarray(V.T)).to(DEV)


def real_space(basis, kpt, V):
    """psi_n(r) of the columns of V on the flattened grid: (n_states, N)"""
    nx, ny, nz = basis.fft_size
    cube = np.zeros((V.shape[1], nx * ny * nz), dtype=complex)
    cube[:, kpt.mapping] = V.T
    cube = cube.reshape(-1, nz, ny, nx)
    return (np.fft.ifftn(cube, axes=(1, 2, 3)) * (nx * ny * nz) / np.sqrt(basis.model.unit_cell_volume)).reshape(V.shape[1], -1)


def sum_over_states(basis, spectrum, dV, eF, temperature):
    """The yardstick: (d_rho, deF, [d_occ per k for all states])."""
    filled = basis.model.filled_occupation
    dv = dV.reshape(-1)
    drho = np.zeros(dv.size)
    ldos = np.zeros(dv.size)
    dos = 0.0
    diag = []
    for (E, V), kpt, w in zip(spectrum, basis.kpoints, basis.kweights):
        psi = real_space(basis, kpt, V)
        M = (psi.conj() * dv) @ psi.T * basis.dvol                      # M[n, m] = <psi_n|dV|psi_m>
        if temperature == 0:
            f = np.where(E < eF, filled, 0.0)
            fp = np.zeros_like(E)
        else:
            x = (E - eF) / temperature
            f = filled * _smear("fermi_dirac", x)
            fp = filled * occupation_derivative("fermi_dirac", x) / temperature
        dE = E[:, None] - E[None, :]
        close = np.abs(dE) < 1e-8
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(close, 0.5 * (fp[:, None] + fp[None, :]), (f[:, None] - f[None, :]) / np.where(close, 1.0, dE))
        B = r * M.T                                                     # B[m, n] = r_mn M_nm
        drho += w * np.real(np.sum(psi.conj() * (B @ psi), axis=0))
        ldos -= w * (fp[:, None] * np.abs(psi) ** 2).sum(axis=0)
        dos -= w * fp.sum()
        diag.append((fp, np.real(np.diag(M))))
    deF = 0.0
    if temperature > 0:
        deF = float(np.dot(ldos, dv)) * basis.dvol / dos
        drho += ldos * deF
    docc = [fp * (de - deF) for fp, de in diag]
    return drho.reshape(dV.shape), deF, docc


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def fixed_tol(basis, psi, occupation, thr, tol=1e-10):
    """every Sternheimer tolerance clamped to ``tol``"""
    return dftk.BandtolBalanced(basis, psi, occupation, occupation_threshold=thr, bandtol_min=tol, bandtol_max=tol)


class Setup:
    pass


@pytest.fixture(scope="module")
def s0():
    """T = 0: the basis, its Hamiltonian, the full spectrum, the four occupied exact eigenvectors per k-point."""
    s = Setup()
    s.basis = make_basis()
    s.rho, s.ham = ground_hamiltonian(s.basis)
    s.spec = dense_spectrum(s.basis, s.ham)
    s.eF = 0.5 * (max(E[3] for E, _ in s.spec) + min(E[4] for E, _ in s.spec))
    s.dV1 = cosine_potential(s.basis, DV1)
    s.dV2 = cosine_potential(s.basis, DV2)
    s.psi = [to_block(V[:, :4]) for _, V in s.spec]
    s.eig = [E[:4].copy() for E, _ in s.spec]
    s.occ = [np.full(4, 2.0) for _ in s.spec]
    s.ref1, _, _ = sum_over_states(s.basis, s.spec, s.dV1, s.eF, 0.0)
    s.ref2, _, _ = sum_over_states(s.basis, s.spec, s.dV2, s.eF, 0.0)
    return s


def chi0(s, dV, psi=None, eig=None, occ=None, thr=1e-6, **kw):
    psi = s.psi if psi is None else psi
    occ = s.occ if occ is None else occ
    eig = s.eig if eig is None else eig
    kw.setdefault("bandtolalg", fixed_tol(s.basis, psi, occ, thr))
    return dftk.apply_chi0(s.ham, psi, occ, s.eF, eig, torch.from_numpy(dV).to(DEV), occupation_threshold=thr, **kw)


# ------------------------------------------------------------------------------------------ 1-3: T = 0
def test_dense_hamiltonian_is_hermitian_and_gapped(s0):
    for E, V in s0.spec:
        assert E[4] - E[3] > 0.01
        assert np.abs(V.conj().T @ V - np.eye(len(E))).max() < 1e-12
    assert abs(s0.ref1.sum()) * s0.basis.dvol < 1e-12                      # the yardstick conserves the charge


def test_chi0_zero_temperature_against_sum_over_states(s0):
    res = chi0(s0, s0.dV1)
    assert res["converged"]
    got = res["drho"].cpu().numpy()
    err = relmax(got, s0.ref1)
    print(f"\nchi0 T=0, no extra bands: rel max err {err:.3e}, CG iterations {res['n_iter']}")
    assert abs(got.sum()) * s0.basis.dvol < 1e-12 * np.abs(got).sum() * s0.basis.dvol + 1e-14
    assert res["deF"] == 0.0 and all(np.all(d == 0) for d in res["doccupation"])
    assert err < CHI0_TOL
    s0.n_iter_plain = res["n_iter"]
    s0.drho_plain = got


def test_chi0_with_extra_bands_that_are_not_eigenvectors(s0):
    rng = np.random.default_rng(11)
    psi, eig, occ = [], [], []
    for E, V in s0.spec:
        n = len(E)
        X = V[:, 4:7] + 1e-2 * (V[:, 7:] @ (rng.standard_normal((n - 7, 3)) + 1j * rng.standard_normal((n - 7, 3))))
        X -= V[:, :4] @ (V[:, :4].conj().T @ X)                         # orthogonal to the occupied eigenvectors
        Q, _ = np.linalg.qr(X)
        Hm = Q.conj().T @ ((V * E) @ (V.conj().T @ Q))                  # Rayleigh-Ritz inside their span
        e3, U = np.linalg.eigh((Hm + Hm.conj().T) / 2)
        psi.append(to_block(np.concatenate([V[:, :4], Q @ U], axis=1)))
        eig.append(np.concatenate([E[:4], e3]))
        occ.append(np.array([2.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0]))
        assert np.abs(e3 - E[4:7]).max() > 1e-7                          # they are NOT eigenvectors
    res = chi0(s0, s0.dV1, psi=psi, eig=eig, occ=occ)
    assert res["converged"]
    got = res["drho"].cpu().numpy()
    err = relmax(got, s0.ref1)
    print(f"\nchi0 T=0, 3 extra bands: rel max err {err:.3e}, CG iterations {res['n_iter']}")
    assert err < CHI0_TOL                                                # the Schur split is exact
    plain = getattr(s0, "n_iter_plain", None) or chi0(s0, s0.dV1)["n_iter"]
    assert all(a <= b for a, b in zip(res["n_iter"], plain)), (res["n_iter"], plain)
    for d in res["dpsi"]:
        assert float(d[4:].abs().max()) == 0.0                           # no response of the extra bands themselves


# ------------------------------------------------------------------------------------------ 4: finite temperature
@pytest.fixture(scope="module")
def sT():
    s = Setup()
    s.basis = make_basis(temperature=TEMP)
    s.rho, s.ham = ground_hamiltonian(s.basis)
    s.spec = dense_spectrum(s.basis, s.ham)
    nb = 12
    while True:
        occ, eF = dftk.compute_occupation(s.basis, [E[:nb] for E, _ in s.spec])
        if max(o[-1] for o in occ) < THR:
            break
        nb += 2
    s.nb, s.occ, s.eF = nb, occ, eF
    s.psi = [to_block(V[:, :nb]) for _, V in s.spec]
    s.eig = [E[:nb].copy() for E, _ in s.spec]
    s.dV1 = cosine_potential(s.basis, DV1)
    s.ref1, s.deF, s.docc = sum_over_states(s.basis, s.spec, s.dV1, s.eF, TEMP)
    return s


def test_chi0_finite_temperature_against_sum_over_states(sT):
    s = sT
    n_frac = sum(int(np.sum((o > 1e-8) & (o < 2 - 1e-8))) for o in s.occ)
    assert n_frac >= 8                                                   # genuinely fractional occupations
    res = chi0(s, s.dV1, thr=THR)
    assert res["converged"]
    got = res["drho"].cpu().numpy()
    err = relmax(got, s.ref1)
    nrm = res["norm_dH"]
    print(f"\nchi0 T={TEMP}: {s.nb} bands, {n_frac} fractional, rel max err {err:.3e}, deF {res['deF'] * nrm:.6e} "
          f"(yardstick {s.deF:.6e}), CG iterations {res['n_iter']}")
    assert err < CHI0_TOL
    # deF and d_occ belong to the NORMALISED perturbation dV / |dV|
    assert res["deF"] * nrm == pytest.approx(s.deF, rel=CHI0_TOL, abs=1e-12)
    scale = max(np.abs(d).max() for d in s.docc)
    for ik, d in enumerate(res["doccupation"]):
        assert np.abs(d * nrm - s.docc[ik][:s.nb]).max() < CHI0_TOL * scale
    tot = sum(w * float(np.sum(d)) for w, d in zip(s.basis.kweights, res["doccupation"]))
    assert abs(tot) < 1e-12 * scale
    assert abs(got.sum()) * s.basis.dvol < 1e-11 * np.abs(got).sum() * s.basis.dvol


# ------------------------------------------------------------------------------------------ 6: linearity, symmetry
def test_chi0_is_linear_and_symmetric(s0):
    a = 0.7
    r1 = getattr(s0, "drho_plain", None)
    if r1 is None:
        r1 = chi0(s0, s0.dV1)["drho"].cpu().numpy()
    r2 = chi0(s0, s0.dV2)["drho"].cpu().numpy()
    r12 = chi0(s0, a * s0.dV1 + s0.dV2)["drho"].cpu().numpy()
    assert relmax(r2, s0.ref2) < CHI0_TOL
    lin = relmax(r12, a * r1 + r2)
    left, right = float(np.sum(s0.dV1 * r2)), float(np.sum(s0.dV2 * r1))
    print(f"\nlinearity {lin:.3e}; <dV1|chi0 dV2> = {left:.12e}, <dV2|chi0 dV1> = {right:.12e}")
    assert lin < CHI0_TOL
    assert abs(left - right) < CHI0_TOL * max(abs(left), abs(right))
    # chi0 is negative semi-definite
    assert float(np.sum(s0.dV1 * r1)) < 0 and float(np.sum(s0.dV2 * r2)) < 0


def test_chi0_of_a_tiny_potential_is_zero_and_of_two_lanes_the_same(s0):
    res = dftk.apply_chi0(s0.ham, s0.psi, s0.occ, s0.eF, s0.eig, torch.zeros_like(s0.rho))
    assert float(res["drho"].abs().max()) == 0.0 and res["norm_dH"] == 0.0
    basis2 = make_basis(n_lanes=2)
    assert basis2.n_lanes == 2 and not basis2.kbatch
    _, ham2 = ground_hamiltonian(basis2)
    alg = fixed_tol(basis2, s0.psi, s0.occ, 1e-6)
    r = dftk.apply_chi0(ham2, s0.psi, s0.occ, s0.eF, s0.eig, torch.from_numpy(s0.dV1).to(DEV), bandtolalg=alg)
    err = relmax(r["drho"].cpu().numpy(), s0.ref1)
    print(f"\ntwo lanes: rel max err {err:.3e}")
    assert err < CHI0_TOL


# ------------------------------------------------------------------------------------------ 7, 8: the solver itself
def solver_inputs(s0, ik=1):
    Hk = s0.ham[ik]
    psik = s0.psi[ik]
    dV = torch.from_numpy(s0.dV1 / np.linalg.norm(s0.dV1)).to(DEV)
    rhs = dftk.multiply_psi_by_potential(s0.basis, s0.psi, dV)[ik]
    return Hk, psik, s0.eig[ik], rhs


def test_sternheimer_solver_residuals_locking_and_reproducibility(s0):
    Hk, psik, eps, rhs = solver_inputs(s0)
    tol = np.array([1e-5, 1e-10, 1e-10, 1e-5])
    res = dftk.sternheimer_solver(Hk, psik, eps, rhs, tol=tol)
    assert res["converged"]
    x = res["dpsik"]
    P, X, B = psik.cpu().numpy().T, x.cpu().numpy().T, rhs.cpu().numpy().T
    assert np.abs(P.conj().T @ X).max() < 1e-12                          # psi_occ' dpsi = 0
    HX = Hk.mul_(torch.empty_like(x), x).cpu().numpy().T

    def Q(Y):
        return Y - P @ (P.conj().T @ Y)
    R = Q(HX - X * eps) + Q(B)                                           # Q (H - eps) Q dpsi + Q rhs
    true = np.linalg.norm(R, axis=0)
    print(f"\nsternheimer: n_iter {res['n_iter']}, reported {res['residual_norms']}, recomputed {true}")
    assert np.all(true <= tol * (1 + 1e-3) + 1e-13)
    assert np.all(np.abs(true - res["residual_norms"]) <= 1e-3 * res["residual_norms"] + 1e-13)
    assert res["residual_norms"][0] > 1e-9 or res["residual_norms"][3] > 1e-9      # the loose columns were locked early
    again = dftk.sternheimer_solver(Hk, psik, eps, rhs, tol=tol)
    assert again["n_iter"] == res["n_iter"]
    assert torch.equal(again["dpsik"], x)                                # bitwise reproducible
    assert np.array_equal(again["residual_norms"], res["residual_norms"])
    # a start vector: a tighter solution passes the first convergence check
    tight = dftk.sternheimer_solver(Hk, psik, eps, rhs, tol=1e-11)
    warm = dftk.sternheimer_solver(Hk, psik, eps, rhs, tol=1e-9, dpsik0=tight["dpsik"])
    assert tight["converged"] and warm["converged"] and warm["n_iter"] == 1
    # no columns at all
    empty = dftk.sternheimer_solver(Hk, psik[:0], eps[:0], rhs[:0])
    assert empty["converged"] and empty["n_iter"] == 0 and empty["dpsik"].shape == (0, Hk.n_G)


def host_syncs(lib):
    n = C.c_int64()
    dftk._lib.check(lib.dftk_mi_launch_count(None, C.byref(n)))
    return n.value


def test_one_host_synchronisation_per_cg_iteration(s0):
    Hk, psik, eps, rhs = solver_inputs(s0, ik=2)
    lib = s0.basis.lib
    counts = {}
    for K in (6, 3, 6):                                                  # the first call sizes every workspace
        before = host_syncs(lib)
        res = dftk.sternheimer_solver(Hk, psik, eps, rhs, tol=0.0, miniter=K, maxiter=K)
        counts[K] = host_syncs(lib) - before
        assert res["n_iter"] == K and not res["converged"]
    print(f"\nhost synchronisations: K=3 {counts[3]}, K=6 {counts[6]}")
    assert counts[6] - counts[3] == 3


# ------------------------------------------------------------------------------------------ 9: symmetries
def test_chi0_on_the_irreducible_mesh_equals_the_full_mesh():
    _, _, pos = dftk.silicon_cell()
    sym, full = Setup(), Setup()
    sym.basis = make_basis(positions=pos, symmetries=True)
    assert len(sym.basis.kpoints) < 8 and len(sym.basis.symmetries) > 1
    full.basis = make_basis(positions=pos, fft_size=sym.basis.fft_size)
    assert len(full.basis.kpoints) == 8
    dV = dftk.symmetrize_rho(sym.basis, torch.from_numpy(cosine_potential(sym.basis, DV1)).to(DEV))
    out = []
    for s in (sym, full):
        s.rho, s.ham = ground_hamiltonian(s.basis)
        s.spec = dense_spectrum(s.basis, s.ham)
        s.eF = 0.5 * (max(E[3] for E, _ in s.spec) + min(E[4] for E, _ in s.spec))
        s.psi = [to_block(V[:, :4]) for _, V in s.spec]
        s.eig = [E[:4].copy() for E, _ in s.spec]
        s.occ = [np.full(4, 2.0) for _ in s.spec]
        out.append(chi0(s, dV.cpu().numpy())["drho"].cpu().numpy())
    ref, _, _ = sum_over_states(full.basis, full.spec, dV.cpu().numpy(), full.eF, 0.0)
    err = relmax(out[0], out[1])
    print(f"\nirreducible vs full mesh: {err:.3e}; full mesh vs sum over states {relmax(out[1], ref):.3e}")
    assert relmax(out[1], ref) < CHI0_TOL
    assert err < CHI0_TOL


# ------------------------------------------------------------------------------------------ 10: Gamma-real
def test_chi0_after_a_gamma_real_scf_equals_the_complex_iteration():
    lat, atoms, pos = dftk.silicon_cell((1, 1, 1))
    model = dftk.model_DFT(lat, atoms, pos, functionals=LDA)
    got = []
    for gamma_real in (None, False):
        basis = dftk.PlaneWaveBasis(model, 5, dftk.MonkhorstPack((1, 1, 1)), device=DEV, gamma_real=gamma_real)
        assert basis.kpoints[0].gamma_real == (gamma_real is None)
        res = dftk.self_consistent_field(basis, tol=1e-10)
        assert res["converged"]
        dV = torch.from_numpy(cosine_potential(basis, DV1)).to(DEV)
        got.append(dftk.apply_chi0(res, dV, tol=1e-10)["drho"].cpu().numpy())
    err = relmax(got[0], got[1])
    print(f"\nGamma-real vs complex SCF: {err:.3e}")
    assert np.abs(got[1]).max() > 1e-3
    assert err < 1e-6


# ------------------------------------------------------------------------------------------ 11: apply_kernel
def kernel_basis(functionals):
    lat, atoms, _ = dftk.silicon_cell()
    if functionals:
        model = dftk.model_DFT(lat, atoms, POS, functionals=functionals)
    else:
        model = dftk.model_atomic(lat, atoms, POS, extra_terms=("Hartree",))
    return dftk.PlaneWaveBasis(model, 5, dftk.MonkhorstPack((1, 1, 1)), device=DEV)


def kernel_drho(basis, rho):
    """rho times a modulation of size <= 1: h d_rho / rho stays at 1e-4 everywhere, also where the density is small and
    f_xc ~ rho^(-2/3) is large -- the truncation error of the central difference is then ~ (h d_rho / rho)^2 ~ 1e-8"""
    mod = cosine_potential(basis, DV2)
    return rho * torch.from_numpy(mod / np.abs(mod).max()).to(DEV)


@pytest.mark.parametrize("functionals", [("lda_x",), ("lda_c_vwn",), ("lda_c_pw",), ()])
def test_apply_kernel_against_central_differences_of_the_potential(functionals):
    basis = kernel_basis(functionals)
    rho = dftk.guess_density(basis)
    drho = kernel_drho(basis, rho)
    h = 1e-4 * float(rho.max()) / float(drho.abs().max())
    assert float((rho - h * drho.abs()).min()) > 0
    Vp = local_potential_fused(basis, rho + h * drho, want_energies=False)["V"]
    Vm = local_potential_fused(basis, rho - h * drho, want_energies=False)["V"]
    fd = ((Vp - Vm) / (2 * h)).cpu().numpy()
    got = dftk.apply_kernel(basis, drho, rho).cpu().numpy()
    err = relmax(got, fd)
    print(f"\napply_kernel {functionals or 'Hartree only'}: rel max err against central differences {err:.3e}")
    assert err < KERNEL_TOL
    rpa = dftk.apply_kernel(basis, drho, rho, RPA=True).cpu().numpy()
    if functionals:
        assert relmax(rpa, got) > 1e-3                                   # the XC kernel is not negligible here
    else:
        assert np.array_equal(rpa, got)


def test_rpa_kernel_is_the_kernel_of_the_hartree_only_model():
    lda, hartree = kernel_basis(LDA), kernel_basis(())
    assert lda.fft_size == hartree.fft_size
    rho = dftk.guess_density(lda)
    drho = kernel_drho(lda, rho)
    rpa = dftk.apply_kernel(lda, drho, rho, RPA=True)
    assert torch.equal(rpa, dftk.apply_kernel(hartree, drho, rho))
    assert torch.equal(rpa, dftk.apply_kernel(hartree, drho))           # no density needed without an XC term
    assert relmax(dftk.apply_kernel(lda, drho, rho).cpu().numpy(), rpa.cpu().numpy()) > 1e-3


# ------------------------------------------------------------------------------------------ 12, 13: SCF level
def scf_with_shift(basis, shift, tol=1e-10):
    V0 = basis.terms.V_loc
    saved = V0.clone()
    try:
        if shift is not None:
            V0 += shift
        res = dftk.self_consistent_field(basis, tol=tol)
        assert res["converged"]
        return res
    finally:
        V0.copy_(saved)


def test_self_consistent_response_against_finite_differences_of_the_scf():
    basis = make_basis()
    dV = torch.from_numpy(cosine_potential(basis, DV1)).to(DEV)
    res = scf_with_shift(basis, None)
    out = dftk.solve_OmegaPlusK_split(res, dftk.multiply_psi_by_potential(basis, res["psi"], dV), tol=1e-9)
    assert out["converged"]
    drho = out["drho"].cpu().numpy()
    fd = {}
    for h in (1e-3, 5e-4):
        rp = scf_with_shift(basis, h * dV)["rho"]
        rm = scf_with_shift(basis, -h * dV)["rho"]
        fd[h] = ((rp - rm) / (2 * h)).cpu().numpy()
    e1, e2 = relmax(fd[1e-3], drho), relmax(fd[5e-4], drho)
    print(f"\nsolve_OmegaPlusK_split against SCF central differences: h=1e-3 {e1:.3e}, h=5e-4 {e2:.3e} (ratio {e1 / e2:.2f})")
    # error(h) = T h^2 + n / h: truncation of the central difference plus the convergence error of the two SCF densities
    # over 2 h.  Pure truncation falls fourfold from h to h / 2; the ratio is (T + n) / (T / 4 + 2 n), i.e. above 2 as long as
    # the noise stays below a sixth of the truncation error at h = 1e-3, and it can never exceed 4 by more than noise.
    assert 2.0 < e1 / e2 < 5.0
    assert e1 < SPLIT_TOL
    # the fixed point: d_rho = chi0 (dV + K d_rho), to the GMRES tolerance (1e-9 on the residual, plus two applications
    # of chi0 whose Sternheimer tolerances target 1e-10 each)
    dVtot = dV + dftk.apply_kernel(basis, out["drho"], res["rho"])
    back = dftk.apply_chi0(res, dVtot, tol=1e-10)["drho"]
    resid = float(torch.linalg.norm(back - out["drho"]).item())
    print(f"fixed point residual {resid:.3e}")
    assert resid < 2e-9
    assert relmax(out["dVind"].cpu().numpy(), (dVtot - dV).cpu().numpy()) < 1e-12
    # first-order eigenvalues are the diagonal of the total perturbation; nothing moves the occupations of an insulator
    assert out["deF"] == 0.0 and len(out["deigenvalues"]) == len(basis.kpoints)
    assert all(np.all(d == 0) for d in out["doccupation"])


def test_a_response_call_leaves_the_scf_state_alone():
    energies = []
    for with_response in (False, True):
        basis = make_basis()
        stepper = dftk.ScfStepper(basis, tol=1e-12)
        for _ in range(3):
            info = stepper.step()
        if with_response:
            dV = torch.from_numpy(cosine_potential(basis, DV1)).to(DEV)
            r = dftk.apply_chi0(info["ham"], info["psi"], info["occupation"], info["eF"], info["eigenvalues"], dV)
            assert float(r["drho"].abs().max()) > 0
        energies.append([stepper.step()["energies"].total for _ in range(2)])
    print(f"\ncontinued SCF energies without / with a response call: {energies}")
    # same kernels, same order, same inputs: the energies agree to the last bits (a few ulp of |E| ~ 8 Ha at most)
    assert np.abs(np.array(energies[0]) - np.array(energies[1])).max() < 1e-13


# ------------------------------------------------------------------------------------------ 14: refusals
def test_out_of_scope_requests_are_refused(s0):
    dV = torch.from_numpy(s0.dV1).to(DEV)
    with pytest.raises(NotImplementedError, match="q != 0"):
        dftk.apply_chi0(s0.ham, s0.psi, s0.occ, s0.eF, s0.eig, dV, q=[0.5, 0, 0])
    with pytest.raises(NotImplementedError, match="q != 0"):
        dftk.compute_delta_rho(s0.basis, s0.psi, s0.psi, s0.occ, q=[0, 0.25, 0])
    lat, atoms, pos = dftk.silicon_cell()
    pbe = dftk.PlaneWaveBasis(dftk.model_DFT(lat, atoms, pos, functionals=("gga_x_pbe", "gga_c_pbe")), 5, device=DEV)
    with pytest.raises(NotImplementedError, match="GGA"):
        dftk.apply_kernel(pbe, dftk.guess_density(pbe), dftk.guess_density(pbe))
    teter = dftk.PlaneWaveBasis(dftk.model_DFT(lat, atoms, pos, functionals=("lda_xc_teter93",)), 5, device=DEV)
    with pytest.raises(NotImplementedError, match="lda_xc_teter93"):
        dftk.apply_kernel(teter, dftk.guess_density(teter), dftk.guess_density(teter))
    spin = dftk.PlaneWaveBasis(dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_pw"), magnetic_moments=[1, -1]),
                               5, device=DEV)
    with pytest.raises(NotImplementedError, match="collinear"):
        dftk.apply_kernel(spin, s0.rho, s0.rho)
    with pytest.raises(NotImplementedError, match="collinear"):
        dftk.compute_delta_rho(spin, s0.psi, s0.psi, s0.occ)
