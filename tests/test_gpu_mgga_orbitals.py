"""The orbital side of a meta-GGA at the C ABI (csrc/mgga_kernels.hip): the kinetic energy density
``dftk_mi_kinetic_energy_density_accumulate`` and the div-A-grad term that ``dftk_mi_kblock_set_tau_potential`` adds to
``dftk_mi_apply_H_parts(which & 1)``, against complex128 NumPy restatements.

Blocks: the cube (15, 16, 25) with an orthorhombic cell and a (12, 15, 16) cube with a triclinic cell (the cartesian components
of G + k mix the three integer ones), each at Gamma and at one k != 0; spheres of about 500 plane waves whose integer
components stay below the Nyquist index of every axis.  Bands: 1, and fft_group_size + 1 = 4 with ld_psi > n_G (two launch
groups, the second a partial one).

Tolerances are measured in the same test on code that existed before (nothing is taken from the new kernels):
* tau: the error of ``dftk_mi_density_accumulate`` on the same block and bands against its NumPy restatement, relative to
  max |rho|; the tau kernel gets 4 x that relative to max |tau| (three transforms and one multiply per band for one
  transform).  Measured on the MI355X over the eight cases: density 4.2e-16 ... 7.8e-16, tau 4.5e-16 ... 7.9e-16.
* div-A-grad: the error of ``which = 1`` with the same cube bound as LOCAL potential and no tau term against the dense
  NumPy operator (2-norm, relative); the tau term gets 4 x that.  Measured: local 4.4e-16 ... 6.2e-16, tau term 4.2e-16 ... 5.8e-16.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402

from test_gpu_kernels import Basis, KBlock, dev, relerr  # noqa: E402

EINVAL = -1
FFT_GROUP = 3
CELLS = {
    "ortho": ((15, 16, 25), np.diag([6.0, 6.4, 10.0])),
    "triclinic": ((12, 15, 16), np.array([[5.0, 0.0, 0.0], [1.3, 6.1, 0.0], [-0.9, 1.7, 6.6]]).T),
}
KPOINTS = {"gamma": (0.0, 0.0, 0.0), "k": (0.25, -0.4, 0.1)}
N_SPHERE = 500


class Block:
    """a sphere of about N_SPHERE plane waves around k on the cube of a cell, with the NumPy side of every operator"""

    def __init__(self, lib, cell, kname):
        self.fft, lattice = CELLS[cell]
        nx, ny, nz = self.fft
        self.N = nx * ny * nz
        self.vol = abs(np.linalg.det(lattice))
        self.recip = 2 * np.pi * np.linalg.inv(lattice).T            # columns: reciprocal lattice vectors
        self.k = np.array(KPOINTS[kname])
        half = [(n - 1) // 2 for n in self.fft]
        G = np.array([(gx, gy, gz) for gz in range(-half[2], half[2] + 1) for gy in range(-half[1], half[1] + 1)
                      for gx in range(-half[0], half[0] + 1)])
        kin = 0.5 * np.sum(((G + self.k) @ self.recip.T) ** 2, axis=1)
        keep = kin <= np.sort(kin)[N_SPHERE - 1]
        G, kin = G[keep], kin[keep]
        assert all(np.abs(G[:, a]).max() < half[a] for a in range(3)), "the sphere must fit the cube"
        lin = (G[:, 0] % nx) + nx * ((G[:, 1] % ny) + ny * (G[:, 2] % nz))
        order = np.argsort(lin)
        self.G, self.kin, self.mapping = G[order], kin[order], lin[order]
        self.n_G = len(self.mapping)
        self.gk = (self.G + self.k) @ self.recip.T                   # (n_G, 3) cartesian
        assert abs(0.5 * np.sum(self.gk ** 2, axis=1) - self.kin).max() < 1e-12
        self.bs = Basis(lib, nx, ny, nz, self.vol)
        check(lib.dftk_mi_basis_set_fft_batch(self.bs.h, FFT_GROUP))
        self.kb = KBlock(lib, self.bs, self.mapping, self.kin)
        B = np.asfortranarray(self.recip)
        check(lib.dftk_mi_kblock_set_kpoint(self.kb.h, B.ctypes.data, self.k.ctypes.data))

    # ---- NumPy side
    def to_cube(self, c):
        """unnormalised backward transform of sphere coefficients (n_G, M) -> (M, nz, ny, nx)"""
        nx, ny, nz = self.fft
        flat = np.zeros((c.shape[1], self.N), dtype=complex)
        flat[:, self.mapping] = c.T
        return np.fft.ifftn(flat.reshape(-1, nz, ny, nx), axes=(1, 2, 3)) * self.N

    def density(self, psi, w):
        return np.einsum("n,nzyx->zyx", w, np.abs(self.to_cube(psi)) ** 2)

    def tau(self, psi, w):
        return sum(self.density(self.gk[:, a:a + 1] * psi, 0.5 * w) for a in range(3))

    def dense_local(self, V):
        """<G| V |G'> = V_hat(G - G') on the sphere (differences wrap like the cube's circular convolution)"""
        nx, ny, nz = self.fft
        Vh = np.fft.fftn(V) / self.N                                 # [dz, dy, dx]
        d = self.G[:, None, :] - self.G[None, :, :]
        return Vh[d[..., 2] % nz, d[..., 1] % ny, d[..., 0] % nx]

    def dense_div_a_grad(self, Vtau):
        """1/2 (G + k) . (G' + k) Vtau_hat(G - G')"""
        return 0.5 * (self.gk @ self.gk.T) * self.dense_local(Vtau)

    # ---- device side
    def padded(self, psi, extra=11):
        """(M, ld) device block with ld = n_G + extra, the padding NaN"""
        M = psi.shape[1]
        buf = torch.full((M, self.n_G + extra), float("nan"), dtype=torch.complex128, device="cuda")
        buf[:, :self.n_G] = dev(psi.T.copy())
        return buf

    def accumulate(self, lib, entry, psi, w):
        nx, ny, nz = self.fft
        out = torch.zeros((nz, ny, nx), dtype=torch.float64, device="cuda")
        buf = self.padded(psi)
        wh = np.ascontiguousarray(w, dtype=np.float64)
        check(getattr(lib, entry)(self.kb.h, psi.shape[1], buf.data_ptr(), buf.shape[1], wh.ctypes.data, out.data_ptr()))
        self.bs.sync()
        return out.cpu().numpy()

    def apply(self, lib, psi, which):
        buf = self.padded(psi)
        out = torch.full_like(buf, float("nan"))
        check(lib.dftk_mi_apply_H_parts(self.kb.h, which, psi.shape[1], buf.data_ptr(), buf.shape[1], out.data_ptr(), out.shape[1]))
        self.bs.sync()
        res = out.cpu().numpy()
        assert np.isnan(res[:, self.n_G:].real).all(), "padding rows written"
        return res[:, :self.n_G].T

    def set_tau(self, lib, Vtau):
        if Vtau is None:
            check(lib.dftk_mi_kblock_set_tau_potential(self.kb.h, None))
        else:
            self._vt = dev(np.asarray(Vtau, dtype=np.float64))
            check(lib.dftk_mi_kblock_set_tau_potential(self.kb.h, self._vt.data_ptr()))
        self.bs.sync()


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def blocks(lib):
    return {(c, k): Block(lib, c, k) for c in CELLS for k in KPOINTS}


def random_bands(blk, M, seed):
    rng = np.random.default_rng(seed)
    return np.linalg.qr(rng.standard_normal((blk.n_G, M)) + 1j * rng.standard_normal((blk.n_G, M)))[0]


def positive_cube(blk, seed):
    nx, ny, nz = blk.fft
    return 0.2 + np.random.default_rng(seed).random((nz, ny, nx))


CASES = [(c, k, M) for c in CELLS for k in KPOINTS for M in (1, FFT_GROUP + 1)]


@pytest.mark.parametrize("cell,kname,M", CASES)
def test_kinetic_energy_density(lib, blocks, cell, kname, M):
    """tau += sum_n (w_n / 2) sum_a |ifft((G + k)_a psi_n)|^2 against NumPy within 4 x the density kernel's own error on the same
    block; it accumulates (a second call doubles it); sum tau dvol = sum_n f_n w 1/2 |G + k|^2 |c|^2 within the same
    per-point bound."""
    blk = blocks[(cell, kname)]
    psi = random_bands(blk, M, 100 + M)
    occ = np.array([2.0, 1.3, 0.0, 0.7])[:M] if M > 1 else np.array([2.0])
    w = occ * 0.5 / blk.vol                                          # occupation x k-weight x ifft_normalization^2
    rho = blk.accumulate(lib, "dftk_mi_density_accumulate", psi, w)
    rho_ref = blk.density(psi, w)
    e_rho = np.abs(rho - rho_ref).max() / np.abs(rho_ref).max()
    tau = blk.accumulate(lib, "dftk_mi_kinetic_energy_density_accumulate", psi, w)
    tau_ref = blk.tau(psi, w)
    e_tau = np.abs(tau - tau_ref).max() / np.abs(tau_ref).max()
    print(f"MGGA tau {cell} {kname} M={M}: density {e_rho:.2e}, tau {e_tau:.2e}")
    assert 0 < e_rho < 1e-14
    assert e_tau <= 4 * e_rho
    assert np.all(tau >= 0)
    dvol = blk.vol / blk.N
    T = float(np.sum(0.5 * occ[None, :] * blk.kin[:, None] * np.abs(psi) ** 2))      # sum f w 1/2 |G + k|^2 |c|^2, w = 1/2
    assert abs(tau.sum() * dvol - T) <= 4 * e_rho * np.abs(tau_ref).max() * blk.N * dvol
    assert abs(tau_ref.sum() * dvol - T) <= 1e-13 * T


def test_kinetic_energy_density_accumulates_and_refuses(lib, blocks):
    blk = blocks[("ortho", "k")]
    psi = random_bands(blk, 2, 5)
    w = np.array([1.0, 0.5]) / blk.vol
    nx, ny, nz = blk.fft
    out = torch.ones((nz, ny, nx), dtype=torch.float64, device="cuda")
    buf = blk.padded(psi)
    for _ in range(2):
        check(lib.dftk_mi_kinetic_energy_density_accumulate(blk.kb.h, 2, buf.data_ptr(), buf.shape[1], w.ctypes.data, out.data_ptr()))
    blk.bs.sync()
    assert relerr(out.cpu().numpy(), 1.0 + 2.0 * blk.tau(psi, w)) < 1e-14
    # a block that was never told its k-point: refused by name, nothing written
    bare = KBlock(lib, blk.bs, blk.mapping, blk.kin)
    before = out.clone()
    assert lib.dftk_mi_kinetic_energy_density_accumulate(bare.h, 2, buf.data_ptr(), buf.shape[1], w.ctypes.data, out.data_ptr()) == EINVAL
    assert b"dftk_mi_kblock_set_kpoint" in lib.dftk_mi_last_error()
    Vt = dev(np.ones(blk.N))
    assert lib.dftk_mi_kblock_set_tau_potential(bare.h, Vt.data_ptr()) == EINVAL
    blk.bs.sync()
    assert torch.equal(out, before)
    assert lib.dftk_mi_kinetic_energy_density_accumulate(blk.kb.h, 2, buf.data_ptr(), blk.n_G - 1, w.ctypes.data, out.data_ptr()) == EINVAL


@pytest.mark.parametrize("cell,kname,M", CASES)
def test_div_a_grad(lib, blocks, cell, kname, M):
    """which = 1 with no local potential and a random positive v_tau is 1/2 sum_a (G + k)_a fft(v_tau ifft((G + k)_a psi)): against
    the dense operator within 4 x the error of the local term with the same cube; Hermitian to that bound; added to the local
    and kinetic terms when those are present; after unbinding every result equals the one from before binding bit for bit."""
    blk = blocks[(cell, kname)]
    psi, phi = random_bands(blk, M, 200 + M), random_bands(blk, M, 300 + M)
    Vt = positive_cube(blk, 7)
    Vloc = positive_cube(blk, 8) - 0.7
    A_loc, A_tau = blk.dense_local(Vt), blk.dense_div_a_grad(Vt)
    assert np.abs(A_tau - A_tau.conj().T).max() < 1e-14 * np.abs(A_tau).max()
    # parent code: the same cube as local potential
    blk.kb.set_potential(Vt)
    e_loc = relerr(blk.apply(lib, psi, 1), A_loc @ psi)
    blk.kb.set_potential(Vloc)
    before = [blk.apply(lib, psi, which) for which in (1, 3, 7)]
    # the tau term alone
    check(lib.dftk_mi_kblock_set_potential(blk.kb.h, None))
    blk.set_tau(lib, Vt)
    got = blk.apply(lib, psi, 1)
    e_tau = relerr(got, A_tau @ psi)
    print(f"MGGA div-A-grad {cell} {kname} M={M}: local {e_loc:.2e}, tau term {e_tau:.2e}")
    assert 0 < e_loc < 1e-14
    assert e_tau <= 4 * e_loc
    assert relerr(blk.apply(lib, psi, 2), blk.kin[:, None] * psi) < 1e-15       # (which = 2 never sees the tau cube)
    got_phi = blk.apply(lib, phi, 1)
    for i in range(M):
        a, b = np.vdot(phi[:, i], got[:, i]), np.vdot(psi[:, i], got_phi[:, i])
        assert abs(a - np.conj(b)) <= 4 * e_loc * np.linalg.norm(A_tau @ psi[:, i])
    # with the local potential and the kinetic term
    blk.kb.set_potential(Vloc)
    full = blk.apply(lib, psi, 3)
    ref = (blk.dense_local(Vloc) + A_tau) @ psi + blk.kin[:, None] * psi
    assert relerr(full, ref) <= 4 * e_loc
    # unbound again: bit for bit what it was
    blk.set_tau(lib, None)
    after = [blk.apply(lib, psi, which) for which in (1, 3, 7)]
    for x, y in zip(before, after):
        assert np.array_equal(x, y)


def test_one_call_binds_the_tau_cube_of_several_blocks(lib, blocks):
    """``dftk_mi_kblocks_set_tau_potential``: three blocks of one basis handle (two k-points, one of them twice) share ONE padded
    copy.  H psi of each block against its dense operator (4 x the error of the local term on the same block, as above); a second
    call with another cube refills the shared copy (reuse path); binding one block singly gives it a copy of its own and leaves
    the others with theirs; a plural call over a different set of blocks starts a new share; unbinding everything gives, bit for
    bit, the results from before anything was bound."""
    a, g = blocks[("ortho", "k")], blocks[("ortho", "gamma")]
    bs = a.bs
    B = np.asfortranarray(a.recip)

    class Extra:            # further blocks on a's basis handle, with the NumPy side of the Block they mirror
        def __init__(self, src):
            self.src, self.n_G = src, src.n_G
            self.kb = KBlock(lib, bs, src.mapping, src.kin)
            check(lib.dftk_mi_kblock_set_kpoint(self.kb.h, B.ctypes.data, src.k.ctypes.data))

        def apply(self, psi, which=3):
            return self.kb.apply(psi, which)
    ks = [Extra(a), Extra(g), Extra(a)]
    psis = [random_bands(k.src, 4, 40 + i) for i, k in enumerate(ks)]
    V1, V2, V3 = positive_cube(a, 31), positive_cube(a, 32), positive_cube(a, 33)
    v1, v2, v3 = dev(V1), dev(V2), dev(V3)

    def dense(k, Vt):
        return k.src.dense_div_a_grad(Vt) + np.diag(k.src.kin)
    unbound = [k.apply(p) for k, p in zip(ks, psis)]
    # the bound of each block: the local term with the same cube (code that existed before)
    e_loc = []
    for k, p in zip(ks, psis):
        k.kb.set_potential(V1)
        e_loc.append(relerr(k.apply(p, 1), k.src.dense_local(V1) @ p))
        check(lib.dftk_mi_kblock_set_potential(k.kb.h, None))
    assert all(0 < e < 1e-14 for e in e_loc)

    def bind_all(which, vd):
        hs = (C.c_void_p * len(which))(*[ks[i].kb.h for i in which])
        check(lib.dftk_mi_kblocks_set_tau_potential(len(which), hs, vd.data_ptr() if vd is not None else None))
        bs.sync()

    def check_all(cubes, label):
        for i, (k, p, Vt) in enumerate(zip(ks, psis, cubes)):
            got = k.apply(p)
            ref = unbound[i] if Vt is None else dense(k, Vt) @ p
            if Vt is None:
                assert np.array_equal(got, ref), (label, i)
            else:
                e = relerr(got, ref)
                assert e <= 4 * e_loc[i], (label, i, e, e_loc[i])
    bind_all([0, 1, 2], v1)
    check_all([V1, V1, V1], "shared")
    bind_all([0, 1, 2], v2)                                   # the same holders: the shared copy is refilled
    check_all([V2, V2, V2], "refilled")
    check(lib.dftk_mi_kblock_set_tau_potential(ks[1].kb.h, v3.data_ptr()))     # one block leaves the share
    bs.sync()
    check_all([V2, V3, V2], "one block rebound singly")
    bind_all([0, 2], v1)                                      # (fewer holders than the old share had: refilled or new, V1)
    check_all([V1, V3, V1], "the remaining two again")
    bind_all([1, 2], v2)                                      # another set of blocks: a new share, block 0 keeps the old one
    check_all([V1, V2, V2], "a new share")
    check(lib.dftk_mi_kblock_set_tau_potential(ks[2].kb.h, None))
    bs.sync()
    check_all([V1, V2, None], "one unbound")
    bind_all([0, 1, 2], None)
    check_all([None, None, None], "all unbound")
    # argument errors: decided on the host
    assert lib.dftk_mi_kblocks_set_tau_potential(2, None, v1.data_ptr()) == EINVAL
    assert lib.dftk_mi_kblocks_set_tau_potential(-1, None, v1.data_ptr()) == EINVAL
    assert lib.dftk_mi_kblocks_set_tau_potential(0, None, v1.data_ptr()) == 0


def ax_reuse_count(lib):
    n = C.c_int64(-1)
    assert lib.dftk_mi_ax_reuse_count(C.byref(n)) == 0
    return n.value


def run_lobpcg(lib, blk, Xd, M):
    lam, res = np.zeros(M), np.zeros(M)
    n_iter, conv, nmv = C.c_int(), C.c_int(), C.c_int64()
    st = lib.dftk_mi_lobpcg(blk.kb.h, M, Xd.data_ptr(), blk.n_G, 1e-7, 1, 200, 0, 1, 99, lam.ctypes.data, res.ctypes.data,
                            C.byref(n_iter), C.byref(conv), C.byref(nmv))
    blk.bs.sync()
    return st, lam, conv.value


def test_lobpcg_with_tau_potential_and_no_handover(lib, blocks):
    """The per-block LOBPCG on a block with a tau potential finds the eigenvalues of the dense H = T + V + A_tau.  A promised
    A X handover is taken without a tau potential (the counter moves: the set-up does reach that path) and is not taken once one
    is bound; binding forgets what was kept."""
    blk = blocks[("triclinic", "k")]
    M = 12                                                          # (above the small-block driver's limit: the general driver)
    Vloc, Vt = positive_cube(blk, 21) - 0.7, positive_cube(blk, 22)
    blk.kb.set_potential(Vloc)
    Xd = dev(random_bands(blk, M, 9).T.copy())
    st, lam0, conv = run_lobpcg(lib, blk, Xd, M)
    assert st == 0 and conv
    c0 = ax_reuse_count(lib)
    check(lib.dftk_mi_kblock_reuse_AX(blk.kb.h, 1))
    st, lam1, conv = run_lobpcg(lib, blk, Xd, M)
    assert st == 0 and conv and ax_reuse_count(lib) == c0 + 1 and np.allclose(lam0, lam1, atol=1e-8)
    # bind: the kept A X is forgotten, a promise finds nothing
    blk.set_tau(lib, Vt)
    check(lib.dftk_mi_kblock_reuse_AX(blk.kb.h, 1))
    st, lam2, conv = run_lobpcg(lib, blk, Xd, M)
    assert st == 0 and conv and ax_reuse_count(lib) == c0 + 1
    H = np.diag(blk.kin) + blk.dense_local(Vloc) + blk.dense_div_a_grad(Vt)
    assert np.allclose(lam2, np.linalg.eigvalsh(H)[:M], atol=1e-8)
    assert np.abs(lam2 - lam0).max() > 1e-3                          # (the term is not small)
    # the exit of that call kept an A X; promised, it is still not taken while the tau potential is bound
    check(lib.dftk_mi_kblock_reuse_AX(blk.kb.h, 1))
    st, lam3, conv = run_lobpcg(lib, blk, Xd, M)
    assert st == 0 and conv and ax_reuse_count(lib) == c0 + 1 and np.allclose(lam2, lam3, atol=1e-8)
    blk.set_tau(lib, None)
    check(lib.dftk_mi_kblock_set_potential(blk.kb.h, None))


def test_batched_and_gamma_real_entry_points_refuse_a_bound_block(lib, blocks):
    """dftk_mi_lobpcg_multi (the batched executor's apply_H) and dftk_mi_gamma_apply_H do not know the term: DFTK_MI_EINVAL with
    a message naming the tau potential; a Gamma-real block cannot bind one."""
    a, g = blocks[("ortho", "k")], blocks[("ortho", "gamma")]
    Vt = positive_cube(a, 3)
    # two more blocks on a's basis for the batched call (one basis handle)
    b1 = KBlock(lib, a.bs, a.mapping, a.kin)
    B = np.asfortranarray(a.recip)
    check(lib.dftk_mi_kblock_set_kpoint(b1.h, B.ctypes.data, a.k.ctypes.data))
    b2 = KBlock(lib, a.bs, a.mapping, a.kin)
    V = dev(positive_cube(a, 4))
    vt = dev(Vt)
    for kb in (b1, b2):
        check(lib.dftk_mi_kblock_set_potential(kb.h, V.data_ptr()))
    check(lib.dftk_mi_kblock_set_tau_potential(b1.h, vt.data_ptr()))
    M = 4
    X = [dev(random_bands(a, M, s).T.copy()) for s in (1, 2)]
    kbs = (C.c_void_p * 2)(b1.h, b2.h)
    Xp = (C.c_void_p * 2)(X[0].data_ptr(), X[1].data_ptr())
    ld = (C.c_int64 * 2)(a.n_G, a.n_G)
    seeds = (C.c_uint64 * 2)(1, 2)
    lam, res = np.zeros(2 * M), np.zeros(2 * M)
    n_iter, conv, nmv, status = (C.c_int * 2)(), (C.c_int * 2)(), (C.c_int64 * 2)(), (C.c_int * 2)(7, 7)
    st = lib.dftk_mi_lobpcg_multi(2, kbs, M, Xp, ld, 1e-6, 1, 50, 0, 1, seeds, lam.ctypes.data, res.ctypes.data, n_iter, conv, nmv,
                                  status)
    a.bs.sync()
    assert status[0] == EINVAL and status[1] == 0, (st, list(status))
    assert b"tau potential" in lib.dftk_mi_last_error()
    check(lib.dftk_mi_kblock_set_tau_potential(b1.h, None))
    # Gamma-real
    g.set_tau(lib, positive_cube(g, 5))
    check(lib.dftk_mi_kblock_set_gamma_real(g.kb.h, 1))
    nh = C.c_int64()
    check(lib.dftk_mi_gamma_half_size(g.kb.h, C.byref(nh)))
    xh = torch.zeros((2, nh.value), dtype=torch.complex128, device="cuda")
    out = torch.full_like(xh, float("nan"))
    assert lib.dftk_mi_gamma_apply_H(g.kb.h, 3, 2, xh.data_ptr(), nh.value, out.data_ptr(), nh.value) == EINVAL
    assert b"tau potential" in lib.dftk_mi_last_error()
    g.bs.sync()
    assert torch.isnan(out.real).all()
    g.set_tau(lib, None)
    vg = dev(positive_cube(g, 5))
    assert lib.dftk_mi_kblock_set_tau_potential(g.kb.h, vg.data_ptr()) == EINVAL      # the format is on
    check(lib.dftk_mi_kblock_set_gamma_real(g.kb.h, 0))
    check(lib.dftk_mi_kblock_set_tau_potential(g.kb.h, vg.data_ptr()))
    check(lib.dftk_mi_kblock_set_tau_potential(g.kb.h, None))
