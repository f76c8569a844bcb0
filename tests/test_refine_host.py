"""Host-only tests of the transfer layer and the refinement (no device):

* the NumPy twin (tests/refine_twin.py) against the properties src/transfer.jl documents: the literal index blocks of
  ``transfer_mapping`` agree with the dictionary of integer G; small -> large -> small is the identity on orbitals,
  large -> small -> large the low-pass projector; for densities an even small axis breaks the round trip, exactly by the
  unmatched frequency -n/2 (transfer.jl:158-163);
* M_n M_n^-1 = P on the twin;
* every refusal and ``ValueError`` of dftk_jl_amd/transfer.py and dftk_jl_amd/refine.py on descriptor-only bases
  (``device="cpu"``): they are raised before any device work.
"""
import numpy as np
import pytest

import dftk_jl_amd as dftk
import oracle
from dftk_jl_amd import KptComm
import refine_twin as twin

torch = pytest.importorskip("torch")

KCOORDS = [[0.0, 0.0, 0.0], [1 / 2, 1 / 3, 1 / 4], [3 / 2, 1 / 3, -3 / 4]]


def oracle_basis(Ecut, fft_size):
    lat, atoms, pos = dftk.silicon_cell()
    oatoms = [oracle.ElementPsp("Si", oracle.load_psp_hgh("Si", "lda"))] * 2
    model = oracle.model_DFT(lat, oatoms, pos, functionals=("lda_x", "lda_c_pw"))
    return oracle.PlaneWaveBasis(model, Ecut, oracle.ExplicitKpoints(KCOORDS, [1 / 3] * 3), fft_size=fft_size,
                                 build_terms=False)


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ------------------------------------------------------------------------------------------ twin: cubes
CUBES = [((8, 9, 15), (12, 12, 15)), ((12, 12, 15), (8, 9, 15)), ((8, 12, 9), (12, 9, 12)), ((15, 15, 15), (15, 15, 15)),
         ((8, 8, 8), (8, 8, 8)), ((9, 8, 12), (12, 12, 8))]


@pytest.mark.parametrize("fft_in,fft_out", CUBES)
def test_index_blocks_agree_with_the_dictionary_of_G(fft_in, fft_out):
    rng = np.random.default_rng(sum(fft_in))
    c = crandn(rng, fft_in[2], fft_in[1], fft_in[0])
    out = twin.transfer_cube_fourier(c, fft_in, fft_out)
    by_G = np.zeros_like(out)
    pairs = twin.transfer_mapping_cubes_by_G(fft_in, fft_out)
    for (ox, oy, oz), (ix, iy, iz) in pairs.items():
        by_G[oz, oy, ox] = c[iz, iy, ix]
    assert np.array_equal(out, by_G)
    assert len(pairs) == int(np.prod([min(a, b) for a, b in zip(fft_in, fft_out)]))      # the eight blocks tile min(n)^3
    assert len(twin.transfer_mapping_cubes(fft_in, fft_out)) == 8


def test_density_round_trips():
    rng = np.random.default_rng(3)
    odd, even, big = (9, 9, 9), (8, 9, 9), (12, 12, 12)
    rho = rng.random((9, 9, 9))
    back = twin.transfer_density(twin.transfer_density(rho, odd, big), big, odd)
    assert np.abs(back - rho).max() < 1e-14                       # odd axes: small -> large -> small is the identity
    up = twin.transfer_density(rho, odd, big)
    assert abs(up.mean() - rho.mean()) < 1e-15                    # the integral is preserved
    rho = rng.random((9, 9, 8))                                    # (nz, ny, nx) with nx = 8
    back = twin.transfer_density(twin.transfer_density(rho, even, big), big, even)
    assert np.abs(back - rho).max() > 1e-3                        # an even small axis: not the identity ...
    # ... and the difference is exactly half of the unmatched plane g_x = -4: carried to -4 of the large grid without its
    # partner +4, the real part of the inverse transform keeps its Hermitian half
    c = np.fft.fftn(rho)
    nyq = np.zeros_like(c)
    nyq[:, :, 4] = c[:, :, 4]
    assert np.abs((rho - back) - 0.5 * np.real(np.fft.ifftn(nyq))).max() < 1e-13


# ------------------------------------------------------------------------------------------ twin: spheres
def test_orbital_round_trips():
    small, large = oracle_basis(3, (12, 10, 15)), oracle_basis(5, (16, 18, 15))
    rng = np.random.default_rng(11)
    for k_in, k_out, dG in [(0, 0, (0, 0, 0)), (1, 1, (0, 0, 0)), (1, 2, (1, 0, -1))]:
        ks, kl = small.kpoints[k_in], large.kpoints[k_out]
        back_dG = tuple(-x for x in dG)
        psi = crandn(rng, len(ks.mapping), 3)
        up = twin.transfer_blochwave_kpt(psi, ks.mapping, small.fft_size, kl.mapping, large.fft_size, dG)
        down = twin.transfer_blochwave_kpt(up, kl.mapping, large.fft_size, ks.mapping, small.fft_size, back_dG)
        assert np.array_equal(down, psi)                           # small -> large -> small: the identity
        assert np.isclose(np.linalg.norm(up), np.linalg.norm(psi), rtol=0, atol=1e-13)
        big = crandn(rng, len(kl.mapping), 3)
        low = twin.transfer_blochwave_kpt(big, kl.mapping, large.fft_size, ks.mapping, small.fft_size, back_dG)
        proj = twin.transfer_blochwave_kpt(low, ks.mapping, small.fft_size, kl.mapping, large.fft_size, dG)
        again = twin.transfer_blochwave_kpt(twin.transfer_blochwave_kpt(proj, kl.mapping, large.fft_size, ks.mapping,
                                                                        small.fft_size, back_dG),
                                            ks.mapping, small.fft_size, kl.mapping, large.fft_size, dG)
        assert np.array_equal(again, proj)                         # large -> small -> large: a projector ...
        kept = np.any(proj != 0, axis=1)
        assert kept.sum() == len(ks.mapping) and np.array_equal(proj[kept], big[kept])       # ... onto the small sphere
        # the kept rows are those of lowest kinetic energy: the low-pass projector
        kin = 0.5 * np.sum(large.Gplusk_vectors_cart(kl) ** 2, axis=1)
        assert kin[kept].max() <= 3 + 1e-12 < kin[~kept].min()


# ------------------------------------------------------------------------------------------ twin: metric
def test_metric_times_its_inverse_is_the_projector():
    rng = np.random.default_rng(2)
    n, m = 80, 3
    psi, _ = np.linalg.qr(crandn(rng, n, m))
    kin = 5 * rng.random(n)
    res = crandn(rng, n, m) + psi @ crandn(rng, m, m)
    x = twin.metric_solve_dense(psi, kin, res)
    P = twin.proj_perp(psi)
    for j in range(m):
        M = twin.metric_dense(psi, kin, j)
        assert np.abs(M - M.conj().T).max() < 1e-13
        assert np.linalg.norm(M @ x[:, j] - P @ res[:, j]) < 1e-12 * np.linalg.norm(res[:, j])
        assert np.abs(psi.conj().T @ x[:, j]).max() < 1e-13


# ------------------------------------------------------------------------------------------ refusals, descriptors only
def cpu_basis(Ecut=5, functionals=("lda_x", "lda_c_pw"), kgrid=None, scale=1.0, atoms=None, **kw):
    lat, hgh, pos = dftk.silicon_cell()
    basis_kw = {k: kw.pop(k) for k in list(kw) if k in ("comm_pw", "comm_kpts")}
    model = dftk.model_DFT(scale * np.asarray(lat), atoms or hgh, pos, functionals=functionals, **kw)
    return dftk.PlaneWaveBasis(model, Ecut, kgrid or dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu", build_terms=False,
                               **basis_kw)


TWO_KPTS = dftk.MonkhorstPack((2, 1, 1))


def hubbard_basis(Ecut):
    import hubbard_gen
    Si = dftk.ElementPsp("Si", psp=hubbard_gen.hubbard_psp())
    return cpu_basis(Ecut, atoms=[Si, Si], extra_terms=[dftk.Hubbard((dftk.OrbitalManifold("Si", "3P"), 0.1))])


def fake_scfres(basis, occupation=None):
    psi = [torch.zeros((6, k.n_G), dtype=torch.complex128) for k in basis.kpoints]
    occ = occupation or [np.array([2.0, 2, 2, 2, 0, 0]) for _ in basis.kpoints]
    nx, ny, nz = basis.fft_size
    return dict(basis=basis, psi=psi, occupation=occ, rho=torch.zeros((nz, ny, nx), dtype=torch.float64),
                occupation_threshold=1e-6)


def test_transfer_value_errors_on_descriptors():
    a, b = cpu_basis(3), cpu_basis(5)
    other = cpu_basis(5, scale=1.01)
    psi = [torch.zeros((2, k.n_G), dtype=torch.complex128) for k in a.kpoints]
    with pytest.raises(ValueError, match="lattice"):
        dftk.transfer_blochwave(psi, a, other)
    with pytest.raises(ValueError, match="lattice"):
        dftk.transfer_density(torch.zeros(a.fft_size[::-1], dtype=torch.float64), a, other)
    two = cpu_basis(5, kgrid=dftk.ExplicitKpoints([[0, 0, 0], [0.5, 0, 0]], [0.5, 0.5]))
    with pytest.raises(ValueError, match="k-point"):
        dftk.transfer_blochwave(psi, a, two)
    shifted = cpu_basis(5, kgrid=dftk.ExplicitKpoints([[0.25, 0, 0]], [1.0]))
    with pytest.raises(ValueError, match="k-point"):
        dftk.transfer_blochwave(psi, a, shifted)
    with pytest.raises(ValueError, match="integer"):
        dftk.transfer_blochwave_kpt(psi[0], a, a.kpoints[0], shifted, shifted.kpoints[0])
    with pytest.raises(ValueError, match="cube"):
        dftk.transfer_density(torch.zeros((2, 2), dtype=torch.float64), a, b)
    with pytest.raises(ValueError, match="grid of basis_in"):
        dftk.transfer_density(torch.zeros((3, 3, 3), dtype=torch.float64), a, b)
    # valid arguments on descriptor-only bases: the hot path has no CPU fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dftk.transfer_blochwave(psi, a, b)


def test_refinement_refusals_on_descriptors():
    base = cpu_basis(5)
    res = fake_scfres(base)
    with pytest.raises(NotImplementedError, match="GGA"):
        dftk.refine_scfres(res, cpu_basis(9, functionals=("gga_x_pbe", "gga_c_pbe")))
    with pytest.raises(NotImplementedError, match="GGA"):
        dftk.refine_scfres(fake_scfres(cpu_basis(5, functionals=("gga_x_pbe", "gga_c_pbe"))), cpu_basis(9))
    with pytest.raises(NotImplementedError, match="collinear spin"):
        dftk.refine_scfres(res, cpu_basis(9, magnetic_moments=[1.0, 1.0]))
    with pytest.raises(NotImplementedError, match="exact exchange"):
        dftk.refine_scfres(res, dftk.PlaneWaveBasis(dftk.model_HF(*dftk.silicon_cell()), 9,
                                                    dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu", build_terms=False))
    # a Hubbard term and the two kinds of sharding, on the SCF basis and on basis_ref
    assert hubbard_basis(9).model.hubbard is not None
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.refine_scfres(res, hubbard_basis(9))
    with pytest.raises(NotImplementedError, match="Hubbard"):
        dftk.refine_scfres(fake_scfres(hubbard_basis(5)), cpu_basis(9))
    with pytest.raises(NotImplementedError, match="comm_pw"):
        dftk.refine_scfres(res, cpu_basis(9, comm_pw=KptComm(0, 2)))
    with pytest.raises(NotImplementedError, match="comm_pw"):
        dftk.refine_scfres(fake_scfres(cpu_basis(5, comm_pw=KptComm(0, 2))), cpu_basis(9))
    with pytest.raises(NotImplementedError, match="comm_kpts"):
        dftk.refine_scfres(res, cpu_basis(9, kgrid=TWO_KPTS, comm_kpts=KptComm(0, 2)))
    with pytest.raises(NotImplementedError, match="comm_kpts"):
        dftk.refine_scfres(fake_scfres(cpu_basis(5, kgrid=TWO_KPTS, comm_kpts=KptComm(0, 2))), cpu_basis(9, kgrid=TWO_KPTS))
    for name, bad in (("Hubbard", hubbard_basis(5)), ("comm_pw", cpu_basis(5, comm_pw=KptComm(0, 2))),
                      ("comm_kpts", cpu_basis(5, kgrid=TWO_KPTS, comm_kpts=KptComm(0, 2)))):
        with pytest.raises(NotImplementedError, match=name):
            dftk.compute_projected_gradient(bad, None, None)
    with pytest.raises(ValueError, match="lattice"):
        dftk.refine_scfres(res, cpu_basis(9, scale=1.01))
    with pytest.raises(ValueError, match="k-point"):
        dftk.refine_scfres(res, cpu_basis(9, kgrid=dftk.ExplicitKpoints([[0.25, 0, 0]], [1.0])))
    with pytest.raises(ValueError, match="contain"):
        dftk.refine_scfres(res, cpu_basis(3))
    with pytest.raises(ValueError, match="full occupation"):
        dftk.refine_scfres(fake_scfres(base, [np.array([2.0, 2, 2, 1.5, 0, 0])]), cpu_basis(9))
    with pytest.raises(ValueError, match="temperature"):
        hot = cpu_basis(5, temperature=0.01)
        dftk.refine_scfres(fake_scfres(hot), cpu_basis(9, temperature=0.01))
    with pytest.raises(ValueError, match="full occupation"):
        dftk.check_full_occupation(base, [np.array([2.0, 1.0])])
    dftk.check_full_occupation(base, [np.array([2.0, 2.0])])
    # in scope, but descriptor-only: refused at the first device call, after every check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dftk.refine_scfres(res, cpu_basis(9))


def test_sharded_bases_are_refused_by_the_transfer_and_the_metric():
    a, b = cpu_basis(3), cpu_basis(5)
    sa, sb = cpu_basis(3, comm_pw=KptComm(0, 2)), cpu_basis(5, comm_pw=KptComm(0, 2))
    for bin_, bout in ((sa, b), (a, sb)):
        psik = torch.zeros((2, bin_.kpoints[0].n_loc), dtype=torch.complex128)
        with pytest.raises(NotImplementedError, match="comm_pw"):
            dftk.transfer_blochwave_kpt(psik, bin_, bin_.kpoints[0], bout, bout.kpoints[0])
        with pytest.raises(NotImplementedError, match="comm_pw"):
            dftk.transfer_blochwave([psik], bin_, bout)
    blocks = [torch.zeros((2, sb.kpoints[0].n_loc), dtype=torch.complex128)]
    with pytest.raises(NotImplementedError, match="comm_pw"):
        dftk.invert_refinement_metric(sb, blocks, blocks)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # unsharded, descriptor-only: the device is needed
        dftk.invert_refinement_metric(b, blocks, blocks)


def test_select_occupied_orbitals():
    base = cpu_basis(5)
    res = fake_scfres(base)
    psi, occ = dftk.select_occupied_orbitals(base, res["psi"], res["occupation"], threshold=1e-8)
    assert psi[0].shape[0] == 4 and np.array_equal(occ[0], [2.0, 2, 2, 2])
    assert psi[0].data_ptr() == res["psi"][0].data_ptr()             # views, as in the reference
    with pytest.raises(ValueError, match="expected for an insulator"):
        dftk.select_occupied_orbitals(base, res["psi"], [np.array([2.0, 2, 2, 2, 2, 0])], threshold=0.0)
