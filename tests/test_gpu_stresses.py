"""compute_stresses_cart on the device (stress_kernels.hip, dftk.jl_amd/stresses.py) against the definition of the reference
(src/postprocess/stresses.jl:30-55, test/stresses.jl): sigma = (1 / Omega) dE[(I + eps) L] / d eps with the orbital
coefficients on the same plane-wave spheres, the occupations and the eigenvalues held fixed and rho recomputed from psi.

YARDSTICK (independent of the code under test): the oracle's energy terms on a "frozen-sphere" twin of the oracle basis
on the strained lattice -- ``_build_kpoint`` returns the parent's G vectors / mapping instead of re-selecting by Ecut --
with rho = oracle compute_density(twin, psi, occ); central differences over the six strains
eps = +-h/2 (e_a e_b' + e_b e_a'), divided by Omega.  At h = 1e-5 its truncation error is <= 2e-10 relative and its
round-off below that (measured on these cells; every test asserts h = 1e-4 against h = 1e-5 to 1e-7 relative, so a
broken yardstick cannot pass silently).  Tolerance per term: 1e-8 x the largest component of that term's yardstick;
for the total, whose terms cancel, 1e-8 x the largest component over all terms."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import psp as lpsp  # noqa: E402
from dftk_jl_amd.stresses import _projector_tables  # noqa: E402

import oracle  # noqa: E402
from oracle import basis as obasis  # noqa: E402
from oracle.scf import compute_density as oracle_compute_density  # noqa: E402
from oracle.terms import energy_hamiltonian as oracle_energy_hamiltonian  # noqa: E402

from test_gpu_forces import _gamma_supercell  # noqa: E402
from test_gpu_multispecies import (KCOORDS, KWEIGHTS, LATTICE, POSITIONS, library_atoms, oracle_atoms)  # noqa: E402

LDA = ("lda_x", "lda_c_vwn")
PBE = ("gga_x_pbe", "gga_c_pbe")
TOL = 1e-8
PAIRS = [(0, 0), (1, 1), (2, 2), (2, 1), (2, 0), (1, 0)]


# ------------------------------------------------------------------------------------------ the yardstick
class FrozenSphereBasis(obasis.PlaneWaveBasis):
    """An oracle basis on another lattice with the plane-wave spheres of ``parent`` (what the reference's dual-number
    basis amounts to)."""

    def __init__(self, parent, model):
        self._parent, self._next = parent, 0
        n_k = parent.n_kcoords
        super().__init__(model, parent.Ecut, obasis.ExplicitKpoints(parent.kcoords, parent.kweights[:n_k]),
                         fft_size=parent.fft_size)

    def _build_kpoint(self, kcoord):
        src = self._parent.kpoints[self._next]
        self._next += 1
        assert np.array_equal(src.coordinate, kcoord)
        return obasis.Kpoint(1, np.asarray(kcoord, dtype=float), src.G_vectors, src.mapping)


def yardstick(parent, make_model, psi, occ, h):
    """{term: (3, 3)} by central differences of the oracle's energies; ``make_model(lattice)`` builds the oracle model,
    ``psi``: oracle layout (n_G, n_bands) per k-block."""
    L = np.asarray(parent.model.lattice, dtype=float)
    vol = parent.model.unit_cell_volume
    out = {}

    def energies(eps):
        twin = FrozenSphereBasis(parent, make_model((np.eye(3) + eps) @ L))
        for k0, k1 in zip(parent.kpoints, twin.kpoints):
            assert np.array_equal(k0.mapping, k1.mapping)
        rho = oracle_compute_density(twin, psi, occ)
        E, _ = oracle_energy_hamiltonian(twin, psi, occ, rho=rho)
        return {n: float(v) for n, v in E.items() if n != "Entropy"}
    for a, b in PAIRS:
        eps = np.zeros((3, 3))
        eps[a, b] += h / 2
        eps[b, a] += h / 2
        Ep, Em = energies(eps), energies(-eps)
        for name in Ep:
            out.setdefault(name, np.zeros((3, 3)))
            out[name][a, b] = out[name][b, a] = (Ep[name] - Em[name]) / (2 * h * vol)
    return out


def checked_yardstick(parent, make_model, psi, occ):
    fine = yardstick(parent, make_model, psi, occ, 1e-5)
    coarse = yardstick(parent, make_model, psi, occ, 1e-4)
    for name in fine:
        scale = np.max(np.abs(fine[name]))
        dev = np.max(np.abs(fine[name] - coarse[name]))
        print(f"yardstick {name}: max {scale:.6e}, h=1e-4 vs 1e-5: {dev / scale:.3e}")
        assert dev <= 1e-7 * scale, (name, fine[name], coarse[name])
    return fine


def to_oracle(psi):
    return [np.ascontiguousarray(p.cpu().numpy().T) for p in psi]


def compare_terms(basis, psi, occ, rho, ref, label):
    """every term and the sum against the yardstick; returns the device terms"""
    got = {}
    big = max(np.max(np.abs(v)) for v in ref.values())
    failures = []
    for name in basis.model.term_types:
        S = dftk.compute_stresses_term(name, basis, psi, occ, rho=rho)
        if name == "Entropy":
            assert S is None
            continue
        got[name] = S
        assert S.shape == (3, 3) and S.dtype == np.float64
        scale = np.max(np.abs(ref[name]))
        err = np.max(np.abs(S - ref[name]))
        print(f"{label} {name}: max |sigma| {scale:.6e}, |device - yardstick| / scale = {err / scale:.3e}")
        if not err <= TOL * scale:
            failures.append((name, err / scale))
    total, total_ref = sum(got.values()), sum(ref[n] for n in got)
    err = np.max(np.abs(total - total_ref))
    print(f"{label} total: |device - yardstick| = {err:.3e}, bound {TOL * big:.3e}")
    if not err <= TOL * big:
        failures.append(("total", err / big))
    assert not failures, failures
    return got


# ------------------------------------------------------------------------------------------ 1. multi-species cell, term-wise
def _multispecies(functionals):
    model = dftk.model_DFT(LATTICE, library_atoms(), POSITIONS, functionals=functionals, symmetries=False, temperature=0.01)
    basis = dftk.PlaneWaveBasis(model, 8, dftk.ExplicitKpoints(KCOORDS, KWEIGHTS), device="cuda:0", gamma_real=False)

    def omodel(lattice):
        return oracle.model_DFT(lattice, oracle_atoms(), POSITIONS, functionals=functionals, temperature=0.01)
    ob = oracle.PlaneWaveBasis(omodel(LATTICE), 8, oracle.ExplicitKpoints(KCOORDS, KWEIGHTS), fft_size=basis.fft_size)
    rng = np.random.default_rng(17)
    psi, occ = [], []
    for kpt in basis.kpoints:
        A = rng.standard_normal((kpt.n_G, 6)) + 1j * rng.standard_normal((kpt.n_G, 6))
        psi.append(torch.from_numpy(np.ascontiguousarray(np.linalg.qr(A)[0].T)).to("cuda:0"))
        occ.append(rng.uniform(0.1, 2.0, 6))
    return basis, ob, omodel, psi, occ


@pytest.mark.parametrize("functionals", [LDA, PBE], ids=["lda", "pbe"])
def test_termwise_stresses_on_the_multispecies_cell(functionals):
    basis, ob, omodel, psi, occ = _multispecies(functionals)
    for k0, k1 in zip(basis.kpoints, ob.kpoints):
        assert np.array_equal(k0.mapping, k1.mapping)
    ref = checked_yardstick(ob, omodel, to_oracle(psi), occ)
    rho = dftk.compute_density(basis, psi, occ)
    got = compare_terms(basis, psi, occ, rho, ref, "multispecies")
    total = dftk.compute_stresses_cart(basis, psi, occ, rho=rho)
    assert np.max(np.abs(total - sum(got.values()))) <= 1e-15 + 1e-14 * np.max(np.abs(total))
    with pytest.raises(ValueError):
        dftk.compute_stresses_term("Magnetic", basis, psi, occ, rho=rho)


# ------------------------------------------------------------------------------------------ 2. twisted Si2, converged SCF
A_SI = 10.0
TWISTED = A_SI / 2 * np.array([[0, 1, 1.02], [1, 0, 1], [1, 1, 0]])
HF_POSITIONS = [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]


def _si_atoms(functional):
    return [dftk.ElementPsp("Si", lpsp.load_psp("Si", functional))] * 2


def _si_basis(lattice, positions, functionals, kgrid, symmetries=False, fft_size=(20, 20, 20), Ecut=7, **kw):
    fun = "pbe" if functionals == PBE else "lda"
    model = dftk.model_DFT(lattice, _si_atoms(fun), positions, functionals=functionals, symmetries=symmetries,
                           **{k: kw.pop(k) for k in list(kw) if k in ("temperature", "smearing", "magnetic_moments")})
    return dftk.PlaneWaveBasis(model, Ecut, kgrid, fft_size=fft_size, device="cuda:0", **kw)


def _si_oracle(lattice, positions, functionals, kgrid, fft_size, Ecut=7, **kw):
    fun = "pbe" if functionals == PBE else "lda"
    atoms = [oracle.ElementPsp("Si", oracle.load_psp_hgh("Si", fun))] * 2

    def omodel(lat):
        return oracle.model_DFT(lat, atoms, positions, functionals=functionals, **kw)
    return oracle.PlaneWaveBasis(omodel(lattice), Ecut, kgrid, fft_size=fft_size), omodel


@pytest.mark.parametrize("functionals", [LDA, PBE], ids=["lda", "pbe"])
def test_twisted_silicon_scf_stress_with_and_without_symmetries(functionals):
    pos = [np.ones(3) / 8, -np.ones(3) / 8]
    b_full = _si_basis(TWISTED, pos, functionals, dftk.MonkhorstPack((2, 2, 2)).reducible())
    b_sym = _si_basis(TWISTED, pos, functionals, dftk.MonkhorstPack((2, 2, 2)), symmetries=True)
    assert len(b_sym.symmetries) > 1 and len(b_sym.kpoints) < len(b_full.kpoints)
    r_full = dftk.self_consistent_field(b_full, tol=1e-11)
    r_sym = dftk.self_consistent_field(b_sym, tol=1e-11)
    assert r_full["converged"] and r_sym["converged"]
    S_full = dftk.compute_stresses_cart(r_full)
    S_sym = dftk.compute_stresses_cart(r_sym)
    print("sigma (full mesh)\n", S_full, "\nsym - full:", np.max(np.abs(S_sym - S_full)))
    assert np.max(np.abs(S_sym - S_full)) <= 1e-10
    assert np.max(np.abs(S_full - S_full.T)) <= 1e-15
    # the full mesh against the yardstick (rho recomputed from psi, as the definition says)
    ob, omodel = _si_oracle(TWISTED, pos, functionals, oracle.MonkhorstPack((2, 2, 2)).reducible(), b_full.fft_size)
    psi, occ = r_full["psi"], [np.asarray(o, dtype=float) for o in r_full["occupation"]]
    ref = checked_yardstick(ob, omodel, to_oracle(psi), occ)
    rho = dftk.compute_density(b_full, psi, occ)
    compare_terms(b_full, psi, occ, rho, ref, "twisted Si2")
    big = max(np.max(np.abs(v)) for v in ref.values())
    assert np.max(np.abs(S_full - sum(ref.values()))) <= TOL * big
    assert np.max(np.abs(S_sym - sum(ref.values()))) <= TOL * big


# ------------------------------------------------------------------------------------------ 3. against the SCF energy
def test_stress_matches_the_strain_derivative_of_the_scf_energy():
    """Hellmann-Feynman (test/stresses.jl:44-59): Omega sum_ab D_ab sigma_ab = dE_SCF[(I + t D) L] / dt by central
    differences, h = 3e-5.  Meaningful only while no plane wave crosses the cut-off: asserted."""
    kg = dftk.MonkhorstPack((2, 2, 2)).reducible()
    D = np.random.default_rng(3).standard_normal((3, 3))
    D = (D + D.T) / 2
    h = 3e-5

    def run(t):
        basis = _si_basis((np.eye(3) + t * D) @ TWISTED, HF_POSITIONS, LDA, kg)
        return dftk.self_consistent_field(basis, tol=1e-9)
    r0, rp, rm = run(0.0), run(h), run(-h)
    sizes = [[k.n_G for k in r["basis"].kpoints] for r in (rm, r0, rp)]
    print("sphere sizes", sizes[1])
    assert sizes[0] == sizes[1] == sizes[2]
    S = dftk.compute_stresses_cart(r0)
    lhs = r0["basis"].model.unit_cell_volume * float(np.sum(D * S))
    rhs = (rp["energies"].total - rm["energies"].total) / (2 * h)
    print(f"Omega D:sigma = {lhs:.10f}, dE/dt = {rhs:.10f}, difference {abs(lhs - rhs):.3e}")
    assert abs(lhs - rhs) <= 1e-7


# ------------------------------------------------------------------------------------------ 4. equilibrium silicon
def test_equilibrium_silicon_stress_is_isotropic():
    lat, _, pos = dftk.silicon_cell()
    basis = _si_basis(lat, pos, LDA, dftk.MonkhorstPack((2, 2, 2)), symmetries=True, fft_size=None)
    assert len(basis.symmetries) == 48
    res = dftk.self_consistent_field(basis, tol=1e-10)
    S = dftk.compute_stresses_cart(res)
    print("sigma\n", S)
    d = np.diag(S)
    assert np.max(np.abs(S - np.diag(d))) <= 1e-10
    assert np.max(d) - np.min(d) <= 1e-10
    assert abs(d[0]) > 1e-6                                   # Ecut 7 is far from the equilibrium volume


# ------------------------------------------------------------------------------------------ 5. Gamma-real blocks
@pytest.fixture(scope="module")
def gamma_pair():
    lat, at, pos = _gamma_supercell()
    kg = dftk.ExplicitKpoints([[0, 0, 0]], [1.0])
    model = dftk.model_DFT(lat, at, pos, functionals=LDA, symmetries=False)
    b_real = dftk.PlaneWaveBasis(model, 8, kg, device="cuda:0", gamma_real=True)
    assert b_real.kpoints[0].gamma_real
    res = dftk.self_consistent_field(b_real, tol=1e-10, nbandsalg=dftk.AdaptiveBands(model, n_bands_converge=11))
    b_cplx = dftk.PlaneWaveBasis(model, 8, kg, device="cuda:0", gamma_real=False, fft_size=b_real.fft_size)
    assert not b_cplx.kpoints[0].gamma_real
    return b_real, b_cplx, res


@pytest.mark.parametrize("ws_kib", [None, "16"], ids=["default_chunks", "small_chunks"])
@pytest.mark.parametrize("n_bands", [7, 10])
def test_gamma_real_block_matches_the_complex_block(gamma_pair, n_bands, ws_kib, monkeypatch):
    """The real half-format products against the complex ones on the same (real-symmetric) orbitals; with the workspace
    budget cut to 16 KiB one atom's projectors and three or four bands fit a chunk: several chunks of both."""
    b_real, b_cplx, res = gamma_pair
    assert res["psi"][0].shape[0] >= n_bands
    psi = [res["psi"][0][:n_bands].contiguous()]
    occ = [np.random.default_rng(n_bands).uniform(0.2, 2.0, n_bands)]
    if ws_kib is not None:
        monkeypatch.setenv("DFTK_MI_STRESS_WS_KIB", ws_kib)
        rows = (b_real.kpoints[0].n_G + 1) // 2
        assert 6 * rows * 16 * 5 > 16384 and (rows + 20 + 30) * 16 * n_bands > 2 * 16384
    got = {}
    for label, basis in (("real", b_real), ("complex", b_cplx)):
        for name in ("Kinetic", "AtomicNonlocal"):
            got[label, name] = dftk.compute_stresses_term(name, basis, psi, occ)
    if ws_kib is not None:
        monkeypatch.delenv("DFTK_MI_STRESS_WS_KIB")
        for key, S in got.items():          # chunking changes the summation order of the contraction only
            basis = b_real if key[0] == "real" else b_cplx
            S1 = dftk.compute_stresses_term(key[1], basis, psi, occ)
            assert np.max(np.abs(S - S1)) <= 1e-12 * np.max(np.abs(S1)), key
    for name in ("Kinetic", "AtomicNonlocal"):
        Sr, Sc = got["real", name], got["complex", name]
        err = np.max(np.abs(Sr - Sc)) / np.max(np.abs(Sc))
        print(f"gamma-real vs complex {name} ({n_bands} bands): {err:.3e}")
        assert err <= 1e-11, (name, Sr, Sc)
        assert np.max(np.abs(Sc)) > 1e-4


def test_gamma_real_scf_stress_against_the_yardstick(gamma_pair):
    b_real, _, res = gamma_pair
    lat, _, pos = _gamma_supercell()
    atoms = [oracle.ElementPsp("Si", oracle.load_psp_hgh("Si", "lda"))] * len(pos)

    def omodel(lattice):
        return oracle.model_DFT(lattice, atoms, pos, functionals=LDA)
    ob = oracle.PlaneWaveBasis(omodel(lat), 8, oracle.ExplicitKpoints([[0, 0, 0]], [1.0]), fft_size=b_real.fft_size)
    psi, occ = res["psi"], [np.asarray(o, dtype=float) for o in res["occupation"]]
    ref = checked_yardstick(ob, omodel, to_oracle(psi), occ)
    compare_terms(b_real, psi, occ, dftk.compute_density(b_real, psi, occ), ref, "gamma-real Si4")


# ------------------------------------------------------------------------------------------ 6. collinear spin, smearing
def test_collinear_smeared_stress_against_the_yardstick():
    kg = dftk.MonkhorstPack((2, 1, 2), (0.5, 0, 0)).reducible()
    fun = ("lda_xc_teter93",)
    basis = _si_basis(TWISTED, HF_POSITIONS, fun, kg, temperature=0.03, smearing="fermi_dirac", magnetic_moments=[2, 1])
    assert basis.model.n_spin_components == 2
    res = dftk.self_consistent_field(basis, rho=dftk.guess_density(basis, [2, 1]), tol=1e-8)
    psi, occ = res["psi"], [np.asarray(o, dtype=float) for o in res["occupation"]]
    # silicon relaxes to the non-magnetic state; the definition holds for any occupations, so the spin-down blocks
    # (the second half of the k-point list) get scaled occupations: the two channels of rho[psi] then differ
    n_k = len(occ) // 2
    occ = occ[:n_k] + [0.8 * o for o in occ[n_k:]]
    assert any(np.any((o > 1e-3) & (o < 0.999)) for o in occ)                   # fractional occupations
    okg = oracle.MonkhorstPack((2, 1, 2), (0.5, 0, 0)).reducible()
    ob, omodel = _si_oracle(TWISTED, HF_POSITIONS, fun, okg, basis.fft_size, temperature=0.03, magnetic_moments=[2, 1])
    assert len(ob.kpoints) == len(basis.kpoints)
    for k0, k1 in zip(basis.kpoints, ob.kpoints):
        assert np.array_equal(k0.mapping, k1.mapping)
    ref = checked_yardstick(ob, omodel, to_oracle(psi), occ)
    rho = dftk.compute_density(basis, psi, occ)
    assert rho.dim() == 4 and float((rho[0] - rho[1]).abs().max()) > 1e-3
    compare_terms(basis, psi, occ, rho, ref, "collinear Si2")


# ------------------------------------------------------------------------------------------ 7. entry points
def _abi_inputs(basis, psi, occ, ik=0):
    kpt = basis.kpoints[ik]
    n_species, rp, nproj, species, positions, col_start = _projector_tables(basis.model)
    Bh = np.asfortranarray(basis.model.recip_lattice, dtype=np.float64)
    kh = np.ascontiguousarray(kpt.coordinate, dtype=np.float64)
    w = np.ascontiguousarray(basis.kweights[ik] * np.asarray(occ[ik], dtype=float))
    return kpt, Bh, kh, w, n_species, rp, nproj, species, positions, col_start


def _call_kn(basis, kpt, Bh, kh, nb, psi, w, n_species, rp, nproj, species, positions, col_start):
    out = np.zeros(12)
    st = basis.lib.dftk_mi_stress_kinetic_nonlocal(kpt.handle, Bh.ctypes.data, kh.ctypes.data, nb, psi.data_ptr(),
                                                   psi.stride(0), w.ctypes.data, n_species, rp.ctypes.data,
                                                   nproj.ctypes.data, len(species), species.ctypes.data,
                                                   positions.ctypes.data, col_start.ctypes.data, out.ctypes.data)
    basis.sync()
    return st, out


def test_entry_points_are_reproducible_and_refuse_bad_arguments():
    basis, _, _, psi, occ = _multispecies(PBE)
    rho = dftk.compute_density(basis, psi, occ)
    for name in ("Kinetic", "AtomicNonlocal", "AtomicLocal", "Hartree", "Xc", "Ewald", "PspCorrection"):
        a = dftk.compute_stresses_term(name, basis, psi, occ, rho=rho)
        b = dftk.compute_stresses_term(name, basis, psi, occ, rho=rho)
        assert np.array_equal(a, b), name
        assert np.array_equal(a, a.T), name
    assert np.array_equal(dftk.compute_stresses_cart(basis, psi, occ, rho=rho),
                          dftk.compute_stresses_cart(basis, psi, occ, rho=rho))
    # dftk_mi_stress_kinetic_nonlocal
    kpt, Bh, kh, w, n_species, rp, nproj, species, positions, col_start = _abi_inputs(basis, psi, occ, 1)
    args = (basis, kpt, Bh, kh, 6, psi[1], w, n_species, rp, nproj, species, positions)
    st, good = _call_kn(*args, col_start)
    assert st == 0 and np.all(good[:6] != 0) and np.all(good[6:] != 0)
    st, again = _call_kn(*args, col_start)
    assert st == 0 and np.array_equal(good, again)
    assert _call_kn(basis, kpt, Bh, kh, -1, psi[1], w, n_species, rp, nproj, species, positions, col_start)[0] != 0
    short = col_start.copy()
    short[-1] -= 1                                            # does not end at n_p
    cut = col_start.copy()
    cut[1] += 2                                               # cuts the D block of the first atom
    for bad in (short, cut):
        st, out = _call_kn(*args, bad)
        assert st != 0 and np.all(out == 0)
    # dftk_mi_stress_cube: a sphere block does not span the cube
    par = np.zeros((1, 8))
    par[0, :3] = [0.44, 4.0, -7.3]
    sp = np.zeros(1, dtype=np.int32)
    pos = np.zeros((1, 3))
    out = np.zeros(14)
    rho_c = rho.contiguous()

    def cube(handle, n_atoms=1):
        st = basis.lib.dftk_mi_stress_cube(handle, Bh.ctypes.data, 1, par.ctypes.data, n_atoms, sp.ctypes.data,
                                           pos.ctypes.data, rho_c.data_ptr(), out.ctypes.data)
        basis.sync()
        return st
    assert cube(kpt.handle) != 0
    assert cube(basis._cube_handle, -1) != 0
    assert cube(basis._cube_handle) == 0
    first = out.copy()
    assert cube(basis._cube_handle) == 0 and np.array_equal(first, out)
    # the energies that travel with the sums are the library's own
    E, _ = dftk.energy_hamiltonian(basis, psi, occ, rho=rho, only_energies=True)
    assert abs(first[13] - E["Hartree"]) <= 1e-11 * abs(E["Hartree"])
    # dftk_mi_stress_xc
    n = rho_c.numel()
    out8 = np.zeros(8)
    lib = basis.lib
    assert lib.dftk_mi_stress_xc(basis.handle, n, 3, rho_c.data_ptr(), rho_c.data_ptr(), None, None, None, out8.ctypes.data) != 0
    assert lib.dftk_mi_stress_xc(basis.handle, -1, 1, rho_c.data_ptr(), rho_c.data_ptr(), None, None, None, out8.ctypes.data) != 0
    assert lib.dftk_mi_stress_xc(basis.handle, n, 1, rho_c.data_ptr(), rho_c.data_ptr(), None, rho_c.data_ptr(), None,
                                 out8.ctypes.data) != 0
    assert lib.dftk_mi_stress_xc(basis.handle, n, 1, rho_c.data_ptr(), rho_c.data_ptr(), None, None, None, out8.ctypes.data) == 0
    basis.sync()
    ref = float((rho_c.double() ** 2).sum().item())
    assert abs(out8[1] - ref) <= 1e-12 * ref and out8[0] == 0 and np.all(out8[2:] == 0)


@pytest.mark.parametrize("blocks", ["complex_kmesh", "gamma_real"])
def test_stresses_between_scf_steps_leave_the_scf_bit_identical(blocks):
    def run(with_stresses):
        if blocks == "gamma_real":
            lat, at, pos = _gamma_supercell()
            model = dftk.model_DFT(lat, at, pos, functionals=LDA, symmetries=False)
            basis = dftk.PlaneWaveBasis(model, 8, dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cuda:0", gamma_real=True)
            assert basis.kpoints[0].gamma_real
        else:
            basis = _si_basis(TWISTED, HF_POSITIONS, LDA, dftk.MonkhorstPack((2, 2, 2)).reducible(), Ecut=8)
        seen = []

        def cb(info):
            if with_stresses:
                seen.append(dftk.compute_stresses_cart(basis, info["psi"], info["occupation"], rho=info["rho"]))
        res = dftk.self_consistent_field(basis, tol=1e-9, callback=cb)
        return res, seen
    ref, _ = run(False)
    got, seen = run(True)
    assert len(seen) >= 3 and all(np.all(np.isfinite(s)) for s in seen)
    assert got["energies"].total == ref["energies"].total
    assert torch.equal(got["rho"], ref["rho"])
    for a, b in zip(got["eigenvalues"], ref["eigenvalues"]):
        assert np.array_equal(np.asarray(a), np.asarray(b))
