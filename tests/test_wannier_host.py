"""Host side of the Brillouin-zone unfolding and of the Wannier90 interface (no GPU): descriptor-only bases (device="cpu").

A. ``compute_nnkp`` on simple cubic, fcc, bcc, hexagonal (c/a = 1.6) and a triclinic lattice with 2x2x2, 3x3x3 and 4x4x2
   meshes: completeness sum_b w_b b_a b_b = delta_ab to 1e-10, every (ik, ik+b, G_shift) reproduces a b of the list, every b
   comes with -b.  nntot = 6, 8, 12, 8 for the first four lattices on the n x n x n meshes, whose mesh lattice has the point
   group of the reciprocal lattice.  The 4x4x2 mesh has not (its shells are those of a tetragonally distorted lattice):
   there the counts the scheme produces are pinned, 6, 6, 18, 8, with the shell lengths for fcc and bcc.
B. nnkp write -> read round trip; ``complete_nnkp`` recovers b vectors and weights of a file's list.
C. ``wannier_spreads`` on synthetic overlaps: identity; M_nn = e^{-i b.r_n}; gauge invariance of Omega_I to 1e-12; Omega_I >= 0.
D. The host projections against closed forms: Gaussian; hydrogenic 1s, 4 alpha^(5/2) / (alpha^2 + q^2)^2 Y_00.
E. File writers parsed back number for number at the printed precision.
F. Every refusal, on bases that own no device.
G. ``unfold_mapping`` on the silicon 2x2x2 and 3x3x3 meshes.
"""
import os

import numpy as np
import pytest

import dftk_jl_amd as dftk
from dftk_jl_amd.comm import KptComm
from dftk_jl_amd.model import Model
from dftk_jl_amd.wannier import HARTREE_TO_EV, bvector_weights, hydrogenic_radial_mesh, ylm_real

A0 = 5.0
LATTICES = {
    "sc": A0 * np.eye(3),
    "fcc": A0 / 2 * np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0.0]]),
    "bcc": A0 / 2 * np.array([[-1, 1, 1], [1, -1, 1], [1, 1, -1.0]]),
    "hex": np.array([[A0, -A0 / 2, 0], [0, A0 * np.sqrt(3) / 2, 0], [0, 0, 1.6 * A0]]),
    "tri": np.array([[5, 0.7, 0.3], [0.2, 6, 0.9], [0.4, 0.1, 7.0]]),
}
NNTOT_CUBIC_MESH = {"sc": 6, "fcc": 8, "bcc": 12, "hex": 8}
# 4x4x2: the mesh lattice is no longer cubic, and what the scheme produces is pinned so that a change in the shell selection
# shows.  In units of 2 pi / a: simple cubic, one shell of length 1/2 ((+-2, 0, 0), (0, +-2, 0), (0, 0, +-1): 6); fcc, shells
# of length 0.5 (2 vectors) and 0.7071 (4) with weights 2 and 1 (6); bcc, shells of length 0.3536 (6) and 0.6124 (12) with
# weights 1 and 1/2 (18); hexagonal, the in-plane hexagon and the two vectors along c (8)
NNTOT_442 = {"sc": 6, "fcc": 6, "bcc": 18, "hex": 8}
SHELLS_442 = {"fcc": [(0.5, 2), (0.5 ** 0.5, 4)], "bcc": [(0.125 ** 0.5, 6), (0.375 ** 0.5, 12)]}
MESHES = [(2, 2, 2), (3, 3, 3), (4, 4, 2)]


def empty_basis(lattice, mesh, shift=(0, 0, 0), fft_size=(4, 4, 4)):
    model = Model(lattice, [], [], terms=("Kinetic",))
    return dftk.PlaneWaveBasis(model, 1.0, dftk.MonkhorstPack(mesh, shift), fft_size=fft_size, device="cpu",
                               build_terms=False, use_symmetries_for_kpoint_reduction=False)


def silicon_basis(mesh, shift=(0, 0, 0), reduce=True, **model_kw):
    lat, atoms, pos = dftk.silicon_cell()
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"), symmetries=True, **model_kw)
    return dftk.PlaneWaveBasis(model, 3, dftk.MonkhorstPack(mesh, shift), device="cpu", build_terms=False,
                               use_symmetries_for_kpoint_reduction=reduce)


# ============================================================================================================ A
@pytest.mark.parametrize("mesh", MESHES, ids=lambda m: "x".join(map(str, m)))
@pytest.mark.parametrize("name", list(LATTICES))
def test_compute_nnkp_shells(name, mesh):
    basis = empty_basis(LATTICES[name], mesh)
    nnkp = dftk.compute_nnkp(basis)
    b, w = nnkp["bvectors_cart"], nnkp["weights"]
    nntot = nnkp["nntot"]
    assert b.shape == (nntot, 3) and w.shape == (nntot,) and len(nnkp["nnkpts"]) == nntot * len(basis.kpoints)
    assert np.max(np.abs(np.einsum("j,ja,jb->ab", w, b, b) - np.eye(3))) <= 1e-10
    if mesh[0] == mesh[1] == mesh[2] and name in NNTOT_CUBIC_MESH:
        assert nntot == NNTOT_CUBIC_MESH[name]
    if mesh == (4, 4, 2) and name in NNTOT_442:
        assert nntot == NNTOT_442[name]
    if mesh == (4, 4, 2) and name in SHELLS_442:
        lengths = np.linalg.norm(b, axis=1) * A0 / (2 * np.pi)
        assert [(x, int(np.sum(np.abs(lengths - x) < 1e-9))) for x, _ in SHELLS_442[name]] == SHELLS_442[name]
    recip = np.asarray(basis.model.recip_lattice)
    scale = np.max(np.linalg.norm(b, axis=1))
    count = {}
    for ik, ikpb, G in nnkp["nnkpts"]:
        d = (basis.kpoints[ikpb].coordinate + np.asarray(G) - basis.kpoints[ik].coordinate) @ recip.T
        j = count.get(ik, 0)
        count[ik] = j + 1
        assert np.max(np.abs(d - b[j])) <= 1e-12 * scale          # the j-th neighbour of every k-point is b_j
    for j in range(nntot):                                          # every b comes with -b, at the same weight
        partner = [i for i in range(nntot) if np.max(np.abs(b[i] + b[j])) <= 1e-12 * scale]
        assert len(partner) == 1 and abs(w[partner[0]] - w[j]) <= 1e-12 * abs(w[j])


def test_bvector_weights_skips_dependent_shells():
    """Simple cubic on a 4x4x2 mesh: the second shell (the in-plane diagonals) repeats the column of the first and is skipped;
    the shell that closes the relation, (+-2, 0, 0), (0, +-2, 0), (0, 0, +-1), does so alone, and the first drops out with
    weight zero."""
    h = 2 * np.pi / A0
    s1 = h / 4 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0.0]])
    s2 = h / 4 * np.array([[1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0.0]])
    s3 = h / 2 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1.0]])
    chosen = bvector_weights([s1, s2, s3])
    assert [s for s, _ in chosen] == [2]
    assert abs(chosen[0][1] - 1 / (2 * (h / 2) ** 2)) <= 1e-12 * chosen[0][1]
    with pytest.raises(RuntimeError):
        bvector_weights([s1, s2])


def test_compute_nnkp_shifted_mesh_and_G_shifts():
    basis = empty_basis(LATTICES["fcc"], (3, 3, 3), shift=(0.5, 0.5, 0.5))
    nnkp = dftk.compute_nnkp(basis)
    assert nnkp["nntot"] == 8
    assert any(any(G) for _, _, G in nnkp["nnkpts"]) and any(not any(G) for _, _, G in nnkp["nnkpts"])


# ============================================================================================================ B
def test_nnkp_round_trip(tmp_path):
    basis = empty_basis(LATTICES["hex"], (4, 4, 2))
    nnkp = dftk.compute_nnkp(basis)
    prefix = str(tmp_path / "hex")
    dftk.write_w90_nnkp(prefix, nnkp)
    back = dftk.read_w90_nnkp(prefix)
    assert back["nntot"] == nnkp["nntot"] and back["nnkpts"] == nnkp["nnkpts"]
    lines = open(prefix + ".nnkp").read().splitlines()
    first = lines[lines.index("begin nnkpts") + 2].split()
    assert int(first[0]) == 1 and int(first[1]) == nnkp["nnkpts"][0][1] + 1            # 1-based in the file
    full = dftk.complete_nnkp(basis, back)
    assert np.allclose(full["bvectors_cart"], nnkp["bvectors_cart"], rtol=0, atol=1e-12)
    assert np.allclose(full["weights"], nnkp["weights"], rtol=1e-10, atol=0)
    with pytest.raises(FileNotFoundError):
        dftk.read_w90_nnkp(str(tmp_path / "absent"))


# ============================================================================================================ C
def orthonormal_frames(rng, n_k, N, J):
    return np.stack([np.linalg.qr(rng.standard_normal((N, J)) + 1j * rng.standard_normal((N, J)))[0] for _ in range(n_k)])


def frame_overlaps(Q, nnkp):
    n_k, J = Q.shape[0], Q.shape[2]
    M = np.zeros((n_k, nnkp["nntot"], J, J), dtype=complex)
    seen = [0] * n_k
    for ik, ikpb, _ in nnkp["nnkpts"]:
        M[ik, seen[ik]] = Q[ik].conj().T @ Q[ikpb]
        seen[ik] += 1
    return M


def random_unitaries(rng, n_k, J):
    return np.stack([np.linalg.qr(rng.standard_normal((J, J)) + 1j * rng.standard_normal((J, J)))[0] for _ in range(n_k)])


def test_spreads_identity_and_known_centres():
    basis = empty_basis(LATTICES["tri"], (8, 8, 8), fft_size=(2, 2, 2))
    nnkp = dftk.compute_nnkp(basis)
    n_k, nntot, J = len(basis.kpoints), nnkp["nntot"], 3
    M = np.broadcast_to(np.eye(J, dtype=complex), (n_k, nntot, J, J)).copy()
    s = dftk.wannier_spreads(M, nnkp)
    assert s["omega_I"] == 0 and s["omega_OD"] == 0 and s["omega_D"] == 0 and not s["centers"].any() and not s["spreads"].any()
    # M_nn = e^{-i b.r_n}: Im ln M_nn = -b.r_n, so r_n = sum_b w_b b (b.r_n) exactly, by the completeness relation alone;
    # |b.r| < pi needs the fine mesh (8^3: |b| <= 0.21, |r| <= 4.2)
    r = np.array([[0.3, -1.1, 2.0], [0.0, 0.0, 0.0], [-2.5, 1.7, 0.4]])
    phase = np.exp(-1j * nnkp["bvectors_cart"] @ r.T)                      # (nntot, J)
    M = np.zeros((n_k, nntot, J, J), dtype=complex)
    M[:, :, np.arange(J), np.arange(J)] = phase[None]
    s = dftk.wannier_spreads(M, nnkp)
    assert np.max(np.abs(s["centers"] - r)) <= 1e-12
    assert abs(s["omega_I"]) <= 1e-12 and s["omega_OD"] == 0 and abs(s["omega_D"]) <= 1e-12


def test_omega_I_is_gauge_invariant_and_non_negative():
    rng = np.random.default_rng(3)
    basis = empty_basis(LATTICES["fcc"], (3, 3, 3), fft_size=(2, 2, 2))
    nnkp = dftk.compute_nnkp(basis)
    Q = orthonormal_frames(rng, len(basis.kpoints), 12, 4)
    M = frame_overlaps(Q, nnkp)
    s0 = dftk.wannier_spreads(M, nnkp)
    assert s0["omega_I"] >= 0 and s0["omega_OD"] >= 0 and s0["omega_D"] >= 0
    for _ in range(3):
        U = random_unitaries(rng, len(basis.kpoints), 4)
        M2 = dftk.rotate_mmn(M, U, nnkp)
        assert np.allclose(M2, frame_overlaps(Q @ U, nnkp), rtol=0, atol=1e-13)     # rotating the frames is rotating M
        s = dftk.wannier_spreads(M2, nnkp)
        assert abs(s["omega_I"] - s0["omega_I"]) <= 1e-12 * s0["omega_I"]
        assert s["omega_I"] >= 0
    A = rng.standard_normal((5, 6, 4)) + 1j * rng.standard_normal((5, 6, 4))
    U = dftk.projection_gauge(A)
    assert np.allclose(np.einsum("kmi,kmj->kij", U.conj(), U), np.eye(4)[None], atol=1e-13)
    H = np.einsum("kmi,kmj->kij", U.conj(), A)                             # U' A = (A' A)^(1/2): Hermitian positive definite
    assert np.allclose(H, np.conj(np.swapaxes(H, 1, 2)), atol=1e-12) and np.all(np.linalg.eigvalsh(H) > 0)


def test_centre_finite_difference_error():
    """What the b vectors of a 4x4x4 mesh of the silicon cell allow for a centre: M_nn(b) = <e^{-i b.r}> of a density is its
    characteristic function, Im ln M_nn = -b.mean + kappa_3(b.r) / 6 - ..., so the finite-difference centre of a density that
    is symmetric about its mean is exact, and one whose skewness lies along a unit vector u, third cumulant kappa_3, is moved
    by (kappa_3 / 6) sum_b w_b b (b.u)^3, at most |b|^2 kappa_3 / 6 along u (sum_b w_b (b.u)^2 = 1).  Measured here on a
    mixture of two Gaussians 1.5 bohr apart: 3.0e-3 bohr for weights 0.8 / 0.2 (kappa_3 = 0.324, |b|^2 kappa_3 / 6 = 3.8e-3),
    below 1e-12 for equal weights."""
    lat, _, _ = dftk.silicon_cell()
    basis = empty_basis(np.asarray(lat), (4, 4, 4), fft_size=(2, 2, 2))
    nnkp = dftk.compute_nnkp(basis)
    b, n_k = nnkp["bvectors_cart"], len(basis.kpoints)
    assert nnkp["nntot"] == 8
    u = np.ones(3) / np.sqrt(3)
    r0, d, s = np.array([0.4, -0.3, 0.2]), 1.5, 1.0
    for p1, p2 in ((0.8, 0.2), (0.5, 0.5)):
        phi = (p1 * np.exp(-1j * b @ r0) + p2 * np.exp(-1j * b @ (r0 + d * u))) * np.exp(-s * s * np.sum(b * b, axis=1) / 2)
        M = np.broadcast_to(phi[None, :, None, None], (n_k, len(b), 1, 1)).copy()
        centre = dftk.wannier_spreads(M, nnkp)["centers"][0]
        err = np.linalg.norm(centre - (r0 + p2 * d * u))
        kappa3 = p1 * p2 * (p1 - p2) * d ** 3
        allowed = np.max(np.sum(b * b, axis=1)) * kappa3 / 6
        print(f"\nfinite-difference centre, weights {p1} / {p2}: off by {err:.3e} bohr, |b|^2 kappa_3 / 6 = {allowed:.3e}")
        if p1 == p2:
            assert err <= 1e-12
        else:
            assert 0 < err <= allowed


# ============================================================================================================ D
def test_host_projections_against_closed_forms():
    basis = empty_basis(LATTICES["tri"], (1, 1, 1))
    recip = np.asarray(basis.model.recip_lattice)
    rng = np.random.default_rng(1)
    ps = np.vstack([np.zeros((1, 3)), rng.uniform(-2, 2, (40, 3))])
    p_cart = ps @ recip.T
    q = np.linalg.norm(p_cart, axis=1)
    c = np.array([0.3, -1.2, 0.45])
    g = dftk.GaussianWannierProjection(c)(basis, ps)
    ref = np.exp(-np.pi * q * q / 2) * np.exp(-2j * np.pi * (ps @ c))
    assert np.max(np.abs(g - ref)) <= 1e-14
    # hydrogenic 1s: int r^2 2 alpha^(3/2) e^(-alpha r) j_0(q r) dr = 4 alpha^(5/2) / (alpha^2 + q^2)^2.  The reference's
    # quadrature (333 points of the logarithmic mesh, cut near alpha r = 10) misses it by 2.55e-3 of the q = 0 value over
    # these points, the same for both alpha (measured; it is the truncated tail, e^-10 (10^2 + 2 10 + 2) / 2 = 2.8e-3 at
    # q = 0); the bound is ten times the measured figure
    for alpha in (1.3, 0.8):
        h = dftk.HydrogenicWannierProjection(c, 1, 0, 0, alpha)(basis, ps)
        closed = 4 * alpha ** 2.5 / (alpha ** 2 + q ** 2) ** 2 * np.sqrt(1 / (4 * np.pi)) * np.exp(-2j * np.pi * (ps @ c))
        err = np.max(np.abs(h - closed)) / np.max(np.abs(closed))
        print(f"\nhydrogenic 1s, alpha = {alpha}: quadrature error {err:.3e} of the q = 0 value")
        assert err <= 2.55e-2
    # l > 0: zero at p = 0, and the (l, m) of a p orbital along x follows the sign of p_x
    px = dftk.HydrogenicWannierProjection(np.zeros(3), 2, 1, 1, 1.0)(basis, ps)
    assert px[0] == 0 and np.all(np.sign((px * 1j).real[1:]) == np.sign(p_cart[1:, 0]))
    for l in range(4):
        for m in range(-l, l + 1):
            assert np.isfinite(ylm_real(l, m, p_cart)).all()
    r, w = hydrogenic_radial_mesh(2, 1.7)
    assert len(r) == 333 and abs(r[0] * 1.7 - np.exp(-6.0)) < 1e-15
    assert len(dftk.default_wannier_centers(4, seed=2)) == 4
    assert np.array_equal(dftk.default_wannier_centers(2, seed=5)[1].center, dftk.default_wannier_centers(2, seed=5)[1].center)


# ============================================================================================================ E
def numbers(line):
    return [float(x) for x in line.split()]


def test_file_writers_parse_back(tmp_path):
    basis = silicon_basis((2, 2, 2), reduce=False)
    prefix = str(tmp_path / "sub" / "si")
    os.makedirs(os.path.dirname(prefix))
    rng = np.random.default_rng(0)
    n_k, n_bands, n_w = len(basis.kpoints), 5, 4
    # .win
    dftk.write_w90_win(prefix, basis, num_wann=n_w, num_bands=n_bands, wannier_plot=True, num_iter=500)
    text = open(prefix + ".win").read()
    lines = text.splitlines()
    assert lines[0].startswith("!")
    assert "num_wann             =   4" in text and "num_bands            =   5" in text and "num_iter             =   500" in text
    assert "wvfn_formatted = True" in text and "wannier_plot   = True" in text and "mp_grid : 2 2 2" in text
    i = lines.index("begin unit_cell_cart")
    assert lines[i + 1] == "bohr"
    cell = np.array([numbers(x) for x in lines[i + 2:i + 5]])
    assert np.max(np.abs(cell - np.asarray(basis.model.lattice).T)) <= 0.5e-6          # rows = lattice vectors
    i = lines.index("begin atoms_frac")
    atoms = [x.split() for x in lines[i + 1:lines.index("end atoms_frac")]]
    assert [a[0] for a in atoms] == ["Si", "Si"]
    assert np.max(np.abs(np.array([[float(v) for v in a[1:]] for a in atoms]) - np.array(basis.model.positions))) <= 0.5e-6
    i = lines.index("begin kpoints")
    ks = np.array([numbers(x) for x in lines[i + 1:lines.index("end kpoints")]])
    assert ks.shape == (n_k, 3) and np.max(np.abs(ks - np.array([k.coordinate for k in basis.kpoints]))) <= 0.5e-10
    # .eig: band, k-point (1-based), eV with 18 decimals
    eig = [np.sort(rng.uniform(-0.4, 0.6, 7)) for _ in range(n_k)]
    dftk.write_w90_eig(prefix, eig, n_bands)
    rows = [x.split() for x in open(prefix + ".eig").read().splitlines()]
    assert len(rows) == n_k * n_bands
    for idx, row in enumerate(rows):
        k, n = divmod(idx, n_bands)
        assert (int(row[0]), int(row[1])) == (n + 1, k + 1)
        assert abs(float(row[2]) - eig[k][n] * HARTREE_TO_EV) <= 0.5e-18 + 2e-16 * abs(eig[k][n] * HARTREE_TO_EV)
    assert abs(HARTREE_TO_EV - 27.211386245988) == 0
    # .amn: m, n, k then Re, Im; n outside, m inside
    A = rng.standard_normal((n_k, n_bands, n_w)) + 1j * rng.standard_normal((n_k, n_bands, n_w))
    dftk.write_w90_amn(prefix, A)
    lines = open(prefix + ".amn").read().splitlines()
    assert [int(x) for x in lines[1].split()] == [n_bands, n_k, n_w]
    assert len(lines) == 2 + n_k * n_bands * n_w
    for idx, line in enumerate(lines[2:]):
        ik, rest = divmod(idx, n_bands * n_w)
        n, m = divmod(rest, n_bands)
        f = line.split()
        assert [int(f[0]), int(f[1]), int(f[2])] == [m + 1, n + 1, ik + 1]
        assert abs(complex(float(f[3]), float(f[4])) - A[ik, m, n]) <= 1e-18 + 4e-16 * abs(A[ik, m, n])
    # .mmn: header per (k, b) with 1-based indices and the shift, the matrix column by column
    nnkp = dftk.compute_nnkp(basis)
    M = rng.standard_normal((n_k, nnkp["nntot"], n_bands, n_bands)) + 1j * rng.standard_normal((n_k, nnkp["nntot"], n_bands, n_bands))
    dftk.write_w90_mmn(prefix, M, nnkp)
    lines = open(prefix + ".mmn").read().splitlines()
    assert [int(x) for x in lines[1].split()] == [n_bands, n_k, nnkp["nntot"]]
    at = 2
    for e, (ik, ikpb, G) in enumerate(nnkp["nnkpts"]):
        assert [int(x) for x in lines[at].split()] == [ik + 1, ikpb + 1, G[0], G[1], G[2]]
        block = np.array([complex(*numbers(x)) for x in lines[at + 1:at + 1 + n_bands ** 2]]).reshape(n_bands, n_bands).T
        assert np.max(np.abs(block - M[ik, e % nnkp["nntot"]])) <= 1e-18 + 4e-16 * np.max(np.abs(M))
        at += 1 + n_bands ** 2
    assert at == len(lines)


# ============================================================================================================ F
def test_refusals_before_any_device_work(tmp_path):
    lat, atoms, pos = dftk.silicon_cell()
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
    explicit = dftk.PlaneWaveBasis(model, 3, dftk.ExplicitKpoints([[0, 0, 0], [0.5, 0, 0]], [0.5, 0.5]), device="cpu",
                                   build_terms=False)
    with pytest.raises(ValueError, match="MonkhorstPack"):
        dftk.unfold_bz(explicit)
    with pytest.raises(ValueError, match="MonkhorstPack"):
        dftk.compute_nnkp(explicit)
    with pytest.raises(ValueError, match="MonkhorstPack"):
        dftk.write_w90_win(str(tmp_path / "x"), explicit, num_wann=1, num_bands=1)
    irred = silicon_basis((2, 2, 2))
    assert isinstance(irred.kgrid, dftk.MonkhorstPack) and len(irred.kpoints) < 8
    with pytest.raises(ValueError, match="unfold"):
        dftk.compute_nnkp(irred)                       # not the full mesh
    for attr in ("comm_kpts", "comm_pw"):
        sharded = silicon_basis((2, 2, 2))
        setattr(sharded, attr, KptComm(0, 2))
        with pytest.raises(NotImplementedError):
            dftk.unfold_bz(sharded)
        with pytest.raises(NotImplementedError):
            dftk.unfold_bz(dict(basis=sharded))
        with pytest.raises(NotImplementedError):
            dftk.apply_symop(sharded.symmetries[1], sharded, sharded.kpoints[0], None)
        with pytest.raises(NotImplementedError):
            dftk.compute_nnkp(sharded)
    exx = silicon_basis((2, 2, 2))
    exx.model.exact_exchange = object()
    with pytest.raises(NotImplementedError, match="exact exchange"):
        dftk.unfold_bz(exx)
    spin = silicon_basis((2, 2, 2), reduce=False, magnetic_moments=[1.0, 1.0])
    assert spin.model.n_spin_components == 2
    gauss = dftk.default_wannier_centers(4, seed=0)
    with pytest.raises(NotImplementedError, match="spin"):
        dftk.write_wannier90_files(dict(basis=spin), str(tmp_path / "s"), 4, 4, gauss)
    with pytest.raises(NotImplementedError, match="spin"):
        dftk.compute_nnkp(spin)
    with pytest.raises(NotImplementedError, match="spin"):
        dftk.compute_mmn(spin, [], dict(nntot=0, nnkpts=[]), 1)
    with pytest.raises(NotImplementedError, match="spin"):
        dftk.compute_amn(spin, [], gauss, 1)
    with pytest.raises(NotImplementedError, match="bands_plot"):
        dftk.write_wannier90_files(dict(basis=irred), str(tmp_path / "b"), 4, 4, gauss, bands_plot=True)
    with pytest.raises(NotImplementedError, match="bands_plot"):
        dftk.write_w90_win(str(tmp_path / "b"), irred, bands_plot=True, num_wann=4, num_bands=4)
    with pytest.raises(ValueError, match="projections"):
        dftk.write_wannier90_files(dict(basis=irred), str(tmp_path / "p"), 4, 3, gauss)
    with pytest.raises(ValueError, match="num_bands"):
        dftk.write_w90_win(str(tmp_path / "w"), irred, num_wann=4)
    assert not os.listdir(tmp_path)                   # nothing was written
    with pytest.raises(ValueError):
        dftk.HydrogenicWannierProjection([0, 0, 0], 4, 0, 0, 1.0)
    with pytest.raises(ValueError):
        dftk.HydrogenicWannierProjection([0, 0, 0], 2, 1, 2, 1.0)
    with pytest.raises(ValueError, match="weights"):
        dftk.wannier_spreads(np.zeros((1, 1, 1, 1)), dict(nntot=1, nnkpts=[(0, 0, (0, 0, 0))]))
    # a basis without a device: the identity passes through, every other operation has no CPU fallback
    ident = irred.symmetries[0]
    marker = object()
    assert ident.isone() and dftk.apply_symop(ident, irred, irred.kpoints[1], marker) == (irred.kpoints[1], marker)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dftk.apply_symop(irred.symmetries[1], irred, irred.kpoints[0], None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dftk.compute_mmn(silicon_basis((2, 2, 2), reduce=False), [], dict(nntot=0, nnkpts=[]), 1)


# ============================================================================================================ G
@pytest.mark.parametrize("mesh,shift", [((2, 2, 2), (0, 0, 0)), ((3, 3, 3), (0, 0, 0)), ((3, 3, 3), (0.5, 0.5, 0.5))])
def test_unfold_mapping_reaches_the_full_mesh(mesh, shift):
    irred = silicon_basis(mesh, shift)
    full = dftk.unfold_bz(irred)
    assert full is not irred and len(full.kpoints) == int(np.prod(mesh)) and len(irred.kpoints) < len(full.kpoints)
    assert full.fft_size == irred.fft_size and full.Ecut == irred.Ecut and full.model is irred.model
    assert full.kgrid == irred.kgrid and not full.use_symmetries_for_kpoint_reduction
    assert full.symmetries_respect_rgrid == irred.symmetries_respect_rgrid and len(full.symmetries) == len(irred.symmetries)
    hits = np.zeros(len(irred.kpoints))
    for kpt in full.kpoints:
        ik, symop = dftk.unfold_mapping(irred, kpt)
        Sk = symop.S @ irred.kpoints[ik].coordinate
        d = Sk - kpt.coordinate
        assert np.max(np.abs(d - np.round(d))) < 1e-10
        hits[ik] += 1
    assert np.allclose(hits / len(full.kpoints), irred.kweights, rtol=0, atol=1e-14)      # multiplicities = irreducible weights
    assert dftk.unfold_bz(full) is not None and dftk.unfold_bz(empty_basis(LATTICES["sc"], (2, 2, 2))) is not None
    values = [np.full(3, float(i)) for i in range(len(irred.kpoints))]
    spread = dftk.unfold_array(irred, full, values, False)
    assert [int(v[0]) for v in spread] == [dftk.unfold_mapping(irred, k)[0] for k in full.kpoints]
