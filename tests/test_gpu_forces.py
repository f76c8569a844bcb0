"""compute_forces on the device (force_kernels.hip, dftk.jl_amd/forces.py) against the definitions of the reference
(src/terms/local.jl:142-177, nonlocal.jl:49-98, ewald.jl, forces.jl; the checks of test/forces.jl and test/gpu.jl):
the two C entry points against a dense NumPy restatement, every term against finite differences of its energy at
fixed psi and rho, the total against finite differences of the SCF energy, symmetry, Gamma-real blocks, and no side
effect on the SCF."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import _lib  # noqa: E402
from dftk_jl_amd.psp import eval_psp_local_fourier  # noqa: E402

FUN = ("lda_x", "lda_c_vwn")
DISPLACED = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]


def _basis(positions, Ecut, kgrid, fft_size=None, symmetries=False, lattice=None, atoms=None, **kw):
    lat, at, _ = dftk.silicon_cell()
    model = dftk.model_DFT(lat if lattice is None else lattice, at if atoms is None else atoms, positions,
                           functionals=kw.pop("functionals", FUN), symmetries=symmetries,
                           **{k: kw.pop(k) for k in list(kw) if k in ("temperature", "smearing", "magnetic_moments")})
    return dftk.PlaneWaveBasis(model, Ecut, kgrid, fft_size=fft_size, device="cuda:0", **kw)


def _kgrid_222():
    return dftk.MonkhorstPack((2, 2, 2)).reducible()


# ------------------------------------------------------------------------------------------ 1. ABI vs NumPy
def _numpy_local(basis, rho):
    model = basis.model
    nx, ny, nz = basis.fft_size
    rho_np = rho.cpu().numpy()
    rhoG = np.fft.fftn(rho_np) * math.sqrt(model.unit_cell_volume) / basis.N       # [z, y, x]
    ax = [dftk.basis.G_axis(n) for n in (nx, ny, nz)]
    gz, gy, gx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    G = np.stack([gx, gy, gz], axis=-1).astype(float)
    Gc = G @ model.recip_lattice.T
    mask = basis.enforce_real_mask().cpu().numpy()
    F = np.zeros((len(model.atoms), 3))
    for ia, el in enumerate(model.atoms):
        ff = eval_psp_local_fourier(el.psp, torch.as_tensor(np.linalg.norm(Gc, axis=-1))).numpy()
        sf = np.exp(-2j * np.pi * (G @ model.positions[ia]))
        s = np.conj(rhoG) * ff * sf / math.sqrt(model.unit_cell_volume) * mask
        for al in range(3):
            F[ia, al] = -np.real(np.sum(-2j * np.pi * G[..., al] * s))
    return F


def _projector_columns(model):
    """{atom: (first, end) column of P}: species groups in order, atoms in a group in order, count_n_proj columns each
    (nonlocal.jl:166-199)."""
    cols, c = {}, 0
    for group in model.atom_groups:
        for ia in group:
            n = model.atoms[ia].psp.count_n_proj()
            cols[ia] = (c, c + n)
            c += n
    return cols


def _numpy_nonlocal(basis, psi, occ):
    model = basis.model
    D = basis.terms.D
    cols = _projector_columns(model)
    F = np.zeros((len(model.atoms), 3))
    for ik, kpt in enumerate(basis.kpoints):
        P = basis.terms.P[ik].cpu().numpy().T                                    # n_G x n_p
        X = psi[ik].cpu().numpy().T                                              # n_G x n_b
        g = kpt.G_vectors.cpu().numpy().astype(float) + kpt.coordinate[None, :]
        for ia, (c0, c1) in cols.items():
            Pa, Da = P[:, c0:c1], D[c0:c1, c0:c1]
            for al in range(3):
                dPa = -2j * np.pi * g[:, al:al + 1] * Pa
                val = np.einsum("n,n->", occ[ik], np.real(np.einsum("gn,gn->n", X.conj(), Pa @ (Da @ (dPa.conj().T @ X)))))
                F[ia, al] -= basis.kweights[ik] * 2 * val
    return F


def test_abi_matches_numpy_and_is_bitwise_reproducible():
    kg = dftk.ExplicitKpoints([[0.25, 0.0, 0.0], [0.1, 0.2, -0.3]], [0.5, 0.5])
    basis = _basis(DISPLACED, 5, kg)
    rng = np.random.default_rng(0)
    psi, occ = [], []
    for kpt in basis.kpoints:
        A = rng.standard_normal((kpt.n_G, 5)) + 1j * rng.standard_normal((kpt.n_G, 5))
        Q, _ = np.linalg.qr(A)
        psi.append(torch.from_numpy(np.ascontiguousarray(Q.T)).to("cuda:0"))
        occ.append(rng.uniform(0.0, 2.0, 5))
    rho = dftk.guess_density(basis) * (1 + 0.1 * torch.rand(basis.fft_size[::-1], dtype=torch.float64, device="cuda:0"))
    Fl = dftk.compute_forces_term("AtomicLocal", basis, psi, occ, rho=rho)
    Fn = dftk.compute_forces_term("AtomicNonlocal", basis, psi, occ, rho=rho)
    Fl_ref = _numpy_local(basis, rho)
    Fn_ref = _numpy_nonlocal(basis, psi, occ)
    assert np.max(np.abs(Fl - Fl_ref)) <= 1e-11 * np.max(np.abs(Fl_ref)), (Fl, Fl_ref)
    assert np.max(np.abs(Fn - Fn_ref)) <= 1e-11 * np.max(np.abs(Fn_ref)), (Fn, Fn_ref)
    assert np.array_equal(Fl, dftk.compute_forces_term("AtomicLocal", basis, psi, occ, rho=rho))
    assert np.array_equal(Fn, dftk.compute_forces_term("AtomicNonlocal", basis, psi, occ, rho=rho))


def test_nonlocal_rejects_inconsistent_columns():
    kg = dftk.ExplicitKpoints([[0.25, 0.0, 0.0]], [1.0])
    basis = _basis(DISPLACED, 5, kg)
    kpt = basis.kpoints[0]
    psi = torch.zeros((2, kpt.n_G), dtype=torch.complex128, device="cuda:0")
    w = np.ones(2)
    out = np.zeros(6)
    bad = np.array([0, 3, 7], dtype=np.int32)            # does not end at n_p
    kh = np.zeros(3)
    st = basis.lib.dftk_mi_forces_nonlocal(kpt.handle, kh.ctypes.data, 2, psi.data_ptr(), psi.stride(0), w.ctypes.data, 2,
                                           bad.ctypes.data, out.ctypes.data)
    assert st != 0
    # a split that cuts through one atom's block of D is refused
    n_p = basis.terms.P[0].shape[0]
    cut = np.array([0, 1, n_p], dtype=np.int32)            # columns 0 and 1 (l = 0, i = 1, 2) are coupled by h_0
    st = basis.lib.dftk_mi_forces_nonlocal(kpt.handle, kh.ctypes.data, 2, psi.data_ptr(), psi.stride(0), w.ctypes.data, 2,
                                           cut.ctypes.data, out.ctypes.data)
    assert st != 0


# ------------------------------------------------------------------------------------------ 2. / 3. finite differences
@pytest.fixture(scope="module")
def displaced_scf():
    basis = _basis(DISPLACED, 10, _kgrid_222())
    res = dftk.self_consistent_field(basis, tol=1e-10)
    return basis, res


def _rebuild(basis, positions):
    m = basis.model
    model = dftk.model_DFT(m.lattice, m.atoms, positions, functionals=m.functionals)
    kg = dftk.ExplicitKpoints([k.coordinate.tolist() for k in basis.kpoints], list(basis.kweights))
    return dftk.PlaneWaveBasis(model, basis.Ecut, kg, fft_size=basis.fft_size, device="cuda:0")


def test_termwise_forces_match_finite_differences(displaced_scf):
    basis, res = displaced_scf
    psi, occ, rho = res["psi"], res["occupation"], res["rho"]
    rng = np.random.default_rng(7)
    d = rng.standard_normal((2, 3))
    d /= np.linalg.norm(d)
    eps = 1e-5
    Ep, _ = dftk.energy_hamiltonian(_rebuild(basis, [p + eps * x for p, x in zip(DISPLACED, d)]), psi, occ, rho=rho,
                                    only_energies=True)
    Em, _ = dftk.energy_hamiltonian(_rebuild(basis, [p - eps * x for p, x in zip(DISPLACED, d)]), psi, occ, rho=rho,
                                    only_energies=True)
    for name in ("AtomicLocal", "AtomicNonlocal", "Ewald"):
        F = dftk.compute_forces_term(name, basis, psi, occ, rho=rho)
        fd = (Ep[name] - Em[name]) / (2 * eps)
        assert abs(np.sum(F * d) + fd) < 1e-7, (name, np.sum(F * d), -fd)
    for name in ("Kinetic", "Hartree", "Xc", "PspCorrection"):
        assert dftk.compute_forces_term(name, basis, psi, occ, rho=rho) is None


def _scf_energy(positions, tol=1e-11, **kw):
    basis = _basis(positions, 10, kw.pop("kgrid", _kgrid_222()), **kw)
    res = dftk.self_consistent_field(basis, tol=tol)
    return res["energies"].total, res


def test_total_forces_match_energy_finite_differences(displaced_scf):
    basis, res = displaced_scf
    F = dftk.compute_forces(res)
    d = np.random.default_rng(11).standard_normal((2, 3))
    d /= np.linalg.norm(d)
    eps = 1e-5
    Ep, _ = _scf_energy([p + eps * x for p, x in zip(DISPLACED, d)])
    Em, _ = _scf_energy([p - eps * x for p, x in zip(DISPLACED, d)])
    assert abs(np.sum(F * d) + (Ep - Em) / (2 * eps)) < 1e-7
    Fc = dftk.compute_forces_cart(res)
    assert np.allclose(Fc, F @ np.linalg.inv(basis.model.lattice), rtol=0, atol=1e-14)


def test_equilibrium_silicon_has_no_forces():
    _, _, pos = dftk.silicon_cell()
    _, res = _scf_energy(pos, tol=1e-10)
    assert np.max(np.abs(dftk.compute_forces(res))) < 1e-9


# ------------------------------------------------------------------------------------------ 5. symmetry
def test_symmetric_kpoints_give_the_unreduced_forces():
    _, _, pos = dftk.silicon_cell()
    pos = [pos[0] + 0.01 * np.ones(3), pos[1]]
    lat, at, _ = dftk.silicon_cell()
    # (a small temperature: the reduced mesh's Fermi level search needs no integer filling)
    model = dftk.model_DFT(lat, at, pos, functionals=FUN, symmetries=True, temperature=1e-3)
    b_sym = dftk.PlaneWaveBasis(model, 10, dftk.MonkhorstPack((2, 2, 2)), device="cuda:0")
    b_full = _basis(pos, 10, _kgrid_222(), fft_size=b_sym.fft_size, temperature=1e-3)
    assert len(b_sym.kpoints) < len(b_full.kpoints)
    F_sym = dftk.compute_forces(dftk.self_consistent_field(b_sym, tol=1e-10))
    F_full = dftk.compute_forces(dftk.self_consistent_field(b_full, tol=1e-10))
    assert np.max(np.abs(F_sym - F_full)) < 1e-8, (F_sym, F_full)
    Fc = F_sym @ np.linalg.inv(lat)
    axis = np.ones(3) / np.sqrt(3)
    assert np.max(np.abs(Fc - np.outer(Fc @ axis, axis))) < 1e-10


# ------------------------------------------------------------------------------------------ 6. spin + temperature
@pytest.mark.parametrize("smearing", ["fermi_dirac", "gaussian"])
def test_collinear_smeared_forces_match_energy_finite_differences(smearing):
    kg = dftk.MonkhorstPack((4, 1, 2), (0.5, 0, 0)).reducible()

    def run(positions):
        basis = _basis(positions, 7, kg, functionals=("lda_xc_teter93",), temperature=0.03, smearing=smearing,
                       magnetic_moments=[2, 1])
        rho0 = dftk.guess_density(basis, [2, 1])
        res = dftk.self_consistent_field(basis, rho=rho0, tol=1e-12)
        return res["energies"].total, res
    E0, res = run(DISPLACED)
    F = dftk.compute_forces(res)
    d = np.zeros((2, 3))                      # one atom displaced, as test/forces.jl:72-98
    d[1] = np.random.default_rng(5).standard_normal(3)
    d /= np.linalg.norm(d)
    eps = 1e-5
    Ep, _ = run([p + eps * x for p, x in zip(DISPLACED, d)])
    Em, _ = run([p - eps * x for p, x in zip(DISPLACED, d)])
    assert abs(np.sum(F * d) + (Ep - Em) / (2 * eps)) < 5e-6


# ------------------------------------------------------------------------------------------ 7. Gamma-real blocks
def test_gamma_real_nonlocal_matches_the_complex_block():
    lat, at, pos = _gamma_supercell()
    kg = dftk.ExplicitKpoints([[0, 0, 0]], [1.0])
    b_real = _basis(pos, 8, kg, lattice=lat, atoms=at, gamma_real=True)
    assert b_real.kpoints[0].gamma_real
    res = dftk.self_consistent_field(b_real, tol=1e-10)
    b_cplx = _basis(pos, 8, kg, lattice=lat, atoms=at, gamma_real=False, fft_size=b_real.fft_size)
    assert not b_cplx.kpoints[0].gamma_real
    Fr = dftk.compute_forces_term("AtomicNonlocal", b_real, res["psi"], res["occupation"])
    Fc = dftk.compute_forces_term("AtomicNonlocal", b_cplx, res["psi"], res["occupation"])
    assert np.max(np.abs(Fr - Fc)) <= 1e-12 * np.max(np.abs(Fc)), (Fr, Fc)
    F = dftk.compute_forces(res)
    d = np.random.default_rng(3).standard_normal(np.shape(F))
    d /= np.linalg.norm(d)
    eps = 1e-5

    def energy(sign):
        basis = _basis([p + sign * eps * x for p, x in zip(pos, d)], 8, kg, lattice=lat, atoms=at, gamma_real=True,
                       fft_size=b_real.fft_size)
        return dftk.self_consistent_field(basis, tol=1e-11)["energies"].total
    assert abs(np.sum(F * d) + (energy(1) - energy(-1)) / (2 * eps)) < 1e-7


# ------------------------------------------------------------------------------------------ 8. no side effect on the SCF
def _gamma_supercell():
    lat, at, pos = dftk.silicon_cell(supercell=(2, 1, 1))
    return lat, at, [np.asarray(p) + (0.004 * np.array([1.0, 2.0, 3.0]) if i == 0 else 0) for i, p in enumerate(pos)]


@pytest.mark.parametrize("blocks", ["complex_kmesh", "gamma_real"])
def test_forces_between_scf_steps_leave_the_scf_bit_identical(blocks):
    def run(with_forces):
        if blocks == "gamma_real":
            lat, at, pos = _gamma_supercell()
            basis = _basis(pos, 8, dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), lattice=lat, atoms=at, gamma_real=True)
            assert basis.kpoints[0].gamma_real
        else:
            basis = _basis(DISPLACED, 8, _kgrid_222())
        seen = []

        def cb(info):
            if with_forces:
                seen.append(dftk.compute_forces(basis, info["psi"], info["occupation"], rho=info["rho"]))
        res = dftk.self_consistent_field(basis, tol=1e-9, callback=cb)
        return res, seen
    ref, _ = run(False)
    got, seen = run(True)
    assert len(seen) >= 3
    assert got["energies"].total == ref["energies"].total
    assert torch.equal(got["rho"], ref["rho"])
    for a, b in zip(got["eigenvalues"], ref["eigenvalues"]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ------------------------------------------------------------------------------------------ 9. tile and chunk edges
# k_forces_local tiles x by 64, y by FL_WAVES * FL_KY = 32 and z by FL_KZ = 2; k_rowsum loops above 256 waves.  The
# cubes cross every tile edge (nx 63 / 64 / 65 / 129 / 130, ny off the multiple of 32), and every axis is even (the
# Nyquist plane zeroed) and odd at least once.
LOCAL_EDGE_CUBES = [(63, 33, 17), (64, 32, 10), (65, 45, 11), (130, 66, 20), (129, 40, 25)]


def _local_waves(fft_size):
    nx, ny, nz = fft_size
    return -(-nx // 64) * -(-ny // 32) * -(-nz // 2) * 4


def test_local_edge_cubes_cover_the_tiles():
    assert {n % 64 for n, _, _ in LOCAL_EDGE_CUBES} >= {63, 0, 1}
    assert any(ny % 32 for _, ny, _ in LOCAL_EDGE_CUBES)
    for axis in range(3):
        assert {c[axis] % 2 for c in LOCAL_EDGE_CUBES} == {0, 1}
    assert max(_local_waves(c) for c in LOCAL_EDGE_CUBES) > 256


@pytest.mark.parametrize("fft_size", LOCAL_EDGE_CUBES)
def test_local_forces_on_tile_edges(fft_size):
    lat, at, _ = dftk.silicon_cell()
    from dftk_jl_amd.psp import load_psp
    C_ = dftk.ElementPsp("C", load_psp("C", "lda"))
    basis = _basis(DISPLACED, 1.5, dftk.ExplicitKpoints([[0.25, 0.0, 0.0]], [1.0]), fft_size=fft_size,
                   atoms=[at[0], C_])
    g = torch.Generator(device="cuda:0").manual_seed(sum(fft_size))
    rho = dftk.guess_density(basis) * (1 + 0.1 * torch.rand(fft_size[::-1], dtype=torch.float64, device="cuda:0",
                                                            generator=g))
    F = dftk.compute_forces_term("AtomicLocal", basis, None, None, rho=rho)
    F_ref = _numpy_local(basis, rho)
    assert np.max(np.abs(F - F_ref)) <= 1e-11 * np.max(np.abs(F_ref)), (F, F_ref)


def test_nonlocal_band_chunks_at_the_abi():
    """dftk_mi_forces_nonlocal over several band chunks, against the closed formula
    F_{a,alpha} = -4 pi sum_n w_n Re[p_n(a)' D_a q_{alpha,n}(a)], p = P' psi, q_alpha = P' (i g_alpha psi), g = G + k:
    ~400k sphere rows, three atoms of 4 / 0 / 9 columns with banded D blocks, k != 0, ld_psi > rows (NaN padding) and a
    different weight per band.  The chunk is cb = budget / (4 (rows + n_p) 16 B) bands, budget = max(T1, 512 MiB); a
    fresh basis has run no FFT and no H application, so T1 is empty and the budget is the 512 MiB floor."""
    from test_gpu_kernels import Basis, KBlock
    lib = _lib.load()
    n = 96
    ax = dftk.basis.G_axis(n)
    gz, gy, gx = np.meshgrid(ax, ax, ax, indexing="ij")
    inside = (gx * gx + gy * gy + gz * gz <= 2090).reshape(-1)
    mapping = np.nonzero(inside)[0]                                     # (z, y, x) index order, as a sphere
    G = np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], axis=1)[mapping].astype(float)
    rows, nb = len(mapping), 64
    col_start = np.array([0, 4, 4, 13], dtype=np.int32)
    n_p = int(col_start[-1])
    per_band = 4 * (rows + n_p) * 16
    budget = 512 << 20
    cb = budget // per_band
    n_chunks = -(-nb // cb)
    assert nb * per_band >= 3 * budget and n_chunks >= 3 and nb % cb != 0, (rows, cb, n_chunks)   # 20, 20, 20, 4
    rng = np.random.default_rng(41)
    P = rng.standard_normal((rows, n_p)) + 1j * rng.standard_normal((rows, n_p))
    D = np.zeros((n_p, n_p))
    for c0, c1, bw in ((0, 4, 1), (4, 13, 2)):
        for i in range(c0, c1):
            for j in range(i, min(c1, i + bw + 1)):
                D[i, j] = D[j, i] = rng.uniform(-2, 2)
    bs = Basis(lib, n, n, n)
    kb = KBlock(lib, bs, mapping, np.zeros(rows))
    kb.set_projectors(P, D)
    psi = rng.standard_normal((rows, nb)) + 1j * rng.standard_normal((rows, nb))
    ld = rows + 37
    buf = torch.full((nb, ld), float("nan"), dtype=torch.complex128, device="cuda:0")
    buf[:, :rows] = torch.from_numpy(np.ascontiguousarray(psi.T))
    w = np.ascontiguousarray(rng.uniform(0.2, 2.0, nb))
    kpt = np.array([0.13, -0.27, 0.41])
    out = np.zeros(9)
    _lib.check(lib.dftk_mi_forces_nonlocal(kb.h, kpt.ctypes.data, nb, buf.data_ptr(), ld, w.ctypes.data, 3,
                                           col_start.ctypes.data, out.ctypes.data))
    bs.sync()
    g = G + kpt[None, :]
    Ph = P.conj().T
    p = Ph @ psi
    q = [(Ph * (1j * g[:, al])[None, :]) @ psi for al in range(3)]
    ref = np.zeros((3, 3))
    for a in range(3):
        c0, c1 = col_start[a], col_start[a + 1]
        for al in range(3):
            val = np.real(np.sum(p[c0:c1].conj() * (D[c0:c1, c0:c1] @ q[al][c0:c1]), axis=0))
            ref[a, al] = -4 * np.pi * np.dot(w, val)
    got = out.reshape(3, 3)
    assert np.all(got[1] == 0)
    assert np.max(np.abs(got - ref)) <= 1e-11 * np.max(np.abs(ref)), (got, ref)


def _minus_G_index(G):
    """Row of -G for every row G of a sphere (n, 3 integer)."""
    off = int(np.abs(G).max()) + 1
    M = 2 * off + 1
    key = ((G[:, 0] + off) * M + (G[:, 1] + off)) * M + (G[:, 2] + off)
    nkey = ((-G[:, 0] + off) * M + (-G[:, 1] + off)) * M + (-G[:, 2] + off)
    order = np.argsort(key)
    idx = order[np.searchsorted(key[order], nkey)]
    assert np.array_equal(key[idx], nkey)
    return idx


def test_gamma_real_nonlocal_band_chunks():
    """The Gamma-real branch (half-sphere rows, real product) over several band chunks against the complex block.
    Chunks as in the ABI case with the half-sphere rows: this fresh basis has run no H application and no FFT; its T1
    would stay below 512 MiB even then (fft_ensure_scratch: 32 bands x n_lines x nxp x 16 B with n_lines <= ny nz;
    apply_nonlocal_rows: 2 n_p n_b 16 B), so the budget is the 512 MiB floor."""
    lat, at, pos = dftk.silicon_cell(supercell=(2, 2, 2))
    pos = [np.asarray(p) + (0.003 * np.array([1.0, -2.0, 3.0]) if i == 0 else 0) for i, p in enumerate(pos)]
    kg = dftk.ExplicitKpoints([[0, 0, 0]], [1.0])
    b_real = _basis(pos, 20, kg, lattice=lat, atoms=at, gamma_real=True)
    assert b_real.kpoints[0].gamma_real
    b_cplx = _basis(pos, 20, kg, lattice=lat, atoms=at, gamma_real=False, fft_size=b_real.fft_size)
    kpt = b_real.kpoints[0]
    n_G, n_p = kpt.n_G, b_real.terms.P[0].shape[0]
    rows = (n_G + 1) // 2                                                # G = 0 and one row per (G, -G) pair
    nx, ny, nz = b_real.fft_size
    budget = 512 << 20
    per_band = 4 * (rows + n_p) * 16
    cb = budget // per_band
    nb = 2 * cb + 7
    assert max(32 * ny * nz * (-(-nx // 8) * 8) * 16, 2 * n_p * nb * 16) < budget
    assert -(-nb // cb) == 3                                            # cb, cb, 7 bands
    assert -(-nb // (budget // (4 * (n_G + n_p) * 16))) >= 3            # and the complex block chunks as well
    G = kpt.G_vectors.cpu().numpy()
    neg = torch.as_tensor(_minus_G_index(G), device="cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(43)
    A = torch.randn((nb, n_G), dtype=torch.complex128, device="cuda:0", generator=gen)
    psi = [((A + A[:, neg].conj()) / 2).contiguous()]                    # real-symmetric columns
    del A
    occ = [np.random.default_rng(47).uniform(0.1, 2.0, nb)]
    Fr = dftk.compute_forces_term("AtomicNonlocal", b_real, psi, occ)
    Fc = dftk.compute_forces_term("AtomicNonlocal", b_cplx, psi, occ)
    assert np.max(np.abs(Fr - Fc)) <= 1e-12 * np.max(np.abs(Fc)), (Fr, Fc)
