"""The four entries of csrc/phonon_kernels.hip at the C ABI, on the smallest shapes where each can go wrong.

Cell: a triclinic lattice, Fe / Si / Fe (two species; Fe has l = 0, 1, 2 channels with 3 / 2 / 1 radial projectors, as in
test_gpu_multispecies.py).  In species-group order the atoms are Fe(0), Fe(2), Si(1); the displaced atom is group index 1,
the second of its species (and index 2, the other species).  Cube 12 x 9 x 10: one even axis (x), so unpaired Nyquist planes
exist on one axis only.  k = (0.137, -0.291, 0.413); 3 bands in blocks with ld = n_G + 7 and NaN in the padding.

Yardsticks are central differences of PRE-EXISTING entries (``dftk_mi_atomic_superposition`` kind 0,
``dftk_mi_forces_local``, ``dftk_mi_build_projectors_hgh`` + ``dftk_mi_zgemm``, ``dftk_mi_forces_nonlocal``) at steps
h = 1e-3 and h / 2 of the reduced position.  The yardstick's own error is estimated without the new code as
|FD(h) - FD(h / 2)| (pure truncation makes the error of FD(h / 2) a third of that); the new result must agree with FD(h / 2)
to within that estimate, the error ratio between h and h / 2 must lie between 2 and 5 (a yardstick drowned in noise would not
show it), and the measured relative error (h / 2, MI355X) is recorded below with TOL = min(cap, 10 x measured).  The cap is
the size of the truncation error itself, (2 pi g h)^2 / 6 relative with |g| <= 6 on these grids at h = 1e-3: 2e-4.

Checks that are exact in exact arithmetic (``dforces`` along dpsi: F_nl is quadratic in psi; along dw: F_nl is linear in w;
Hermiticity; the Gamma-real block; the closed forms in numpy on the big sphere) are bounded by rounding only: RND = 1e-11
relative to the largest entry, the suite's bound for sums of this length (test_gpu_forces.py), divided by h where a
difference quotient is taken.

The refusal "inside a batched multi-k call" cannot be reached through the ABI (``dftk_mi_batch_replay`` takes enumerated
operations only)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import _lib  # noqa: E402
from dftk_jl_amd._lib import ALLREDUCE_FN, check  # noqa: E402
from dftk_jl_amd.terms import (build_projection_coefficients, local_species_tables,  # noqa: E402
                               projector_species_tables)

DV_MEASURED = 1.6e-5          # atom 1: 7.6e-6, atom 2: 1.5e-5 (|FD(h) - FD(h/2)|: 2.3e-5, 4.6e-5)
DV_TOL = min(2e-4, 10 * DV_MEASURED)
LOCAL_MEASURED = 1.6e-5       # (|FD(h) - FD(h/2)|: 4.8e-5)
LOCAL_TOL = min(2e-4, 10 * LOCAL_MEASURED)
DHPSI_MEASURED = 4.0e-5       # atom 1: 3.7e-5 / 3.9e-5 (1 / 3 bands), atom 2: 2.0e-5 / 1.7e-5 (|FD(h) - FD(h/2)|: 1.1e-4 .. 5.2e-5)
DHPSI_TOL = min(2e-4, 10 * DHPSI_MEASURED)
HESS_MEASURED = 6.3e-5        # (|FD(h) - FD(h/2)|: 1.9e-4)
HESS_TOL = min(2e-4, 10 * HESS_MEASURED)
RND = 1e-11

EINVAL = -1
DEV = "cuda:0"
LATTICE = np.array([[7.3, 0.5, -0.3], [0.4, 6.6, 0.8], [-0.6, 0.7, 7.9]]).T
POSITIONS = [np.array([0.07, 0.11, 0.05]), np.array([0.43, 0.52, 0.38]), np.array([0.71, 0.26, 0.83])]
FFT = (12, 9, 10)
KPT = np.array([0.137, -0.291, 0.413])
ECUT = 5.0
NB, PAD = 3, 7
H1 = 1e-3


def relmax(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


class Cell:
    """Raw handles: the basis, the cube block, one sphere block with the HGH projectors of POSITIONS bound."""

    def __init__(self, lib, kpt=KPT, gamma_real=False):
        from test_gpu_kernels import Basis, KBlock
        self.lib = lib
        atoms = [dftk.ElementPsp("Fe", dftk.load_psp("Fe", "lda")), dftk.ElementPsp("Si", dftk.load_psp("Si", "lda"))]
        self.model = dftk.model_DFT(LATTICE, [atoms[0], atoms[1], atoms[0]], POSITIONS)
        assert self.model.atom_groups == [[0, 2], [1]]
        self.vol = self.model.unit_cell_volume
        nx, ny, nz = FFT
        self.N = nx * ny * nz
        self.B = np.asfortranarray(self.model.recip_lattice, dtype=np.float64)
        self.kpt = np.ascontiguousarray(kpt, dtype=np.float64)
        self.bs = Basis(lib, nx, ny, nz, self.vol)
        self.cube = KBlock(lib, self.bs, np.arange(self.N), np.zeros(self.N))
        ax = [np.array(dftk.basis.G_axis(n)) for n in FFT]
        gz, gy, gx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        G = np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], axis=1)
        q = (G + self.kpt[None, :]) @ self.model.recip_lattice.T
        self.mapping = np.nonzero(0.5 * np.sum(q * q, axis=1) <= ECUT)[0]
        self.G = G[self.mapping]
        assert all(np.abs(self.G[:, d]).max() <= (FFT[d] - 1) // 2 for d in range(3))       # the sphere fits the cube
        self.n = len(self.mapping)
        self.kb = KBlock(lib, self.bs, self.mapping, np.zeros(self.n))
        self.G32 = torch.from_numpy(np.ascontiguousarray(self.G, dtype=np.int32)).to(DEV)
        self.par, self.species, self.pos = local_species_tables(self.model)                 # group order
        (self.n_psp, self.rp, self.nproj, self.pspecies, ppos, self.col_start) = projector_species_tables(self.model)
        assert np.array_equal(ppos, self.pos) and list(self.col_start) == [0, 14, 28, 33]
        self.D = np.asfortranarray(build_projection_coefficients(self.model))
        self.n_p = int(self.col_start[-1])
        self.P = self.projectors(self.pos)
        self.bind(self.P)
        if gamma_real:
            check(lib.dftk_mi_kblock_set_gamma_real(self.kb.h, 1))

    def projectors(self, pos):
        """(n_p, n_G) tensor == column-major n_G x n_p, by dftk_mi_build_projectors_hgh"""
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        n_p = C.c_int()
        P = torch.empty((self.n_p, self.n), dtype=torch.complex128, device=DEV)
        check(self.lib.dftk_mi_build_projectors_hgh(self.bs.h, self.n, self.G32.data_ptr(), self.B.ctypes.data,
                                                    self.kpt.ctypes.data, self.vol, self.n_psp, self.rp.ctypes.data,
                                                    self.nproj.ctypes.data, len(self.pspecies), self.pspecies.ctypes.data,
                                                    pos.ctypes.data, P.data_ptr(), self.n, C.byref(n_p)))
        self.bs.sync()
        assert n_p.value == P.shape[0]
        return P

    def bind(self, P, D=None):
        D = self.D if D is None else D
        self._bound = (P, D)
        check(self.lib.dftk_mi_kblock_set_projectors(self.kb.h, P.shape[0], P.data_ptr(), self.n, D.ctypes.data))

    def moved(self, atom, alpha, h):
        pos = self.pos.copy()
        pos[atom, alpha] += h
        return pos

    # ---- pre-existing entries (the yardsticks)
    def superposition(self, pos):
        out = torch.empty(self.N, dtype=torch.float64, device=DEV)
        check(self.lib.dftk_mi_atomic_superposition(self.cube.h, 0, self.B.ctypes.data, self.par.shape[0],
                                                    self.par.ctypes.data, len(self.species), self.species.ctypes.data,
                                                    np.ascontiguousarray(pos).ctypes.data, out.data_ptr()))
        self.bs.sync()
        return out.cpu().numpy()

    def forces_local(self, pos, rho):
        out = np.zeros((len(self.species), 3))
        check(self.lib.dftk_mi_forces_local(self.cube.h, self.B.ctypes.data, self.par.shape[0], self.par.ctypes.data,
                                            len(self.species), self.species.ctypes.data,
                                            np.ascontiguousarray(pos).ctypes.data, rho.data_ptr(), out.ctypes.data))
        return out

    def forces_nonlocal(self, psi, w):
        out = np.zeros((3, 3))
        w = np.ascontiguousarray(w, dtype=np.float64)
        check(self.lib.dftk_mi_forces_nonlocal(self.kb.h, self.kpt.ctypes.data, psi.shape[0], psi.data_ptr(), psi.stride(0),
                                               w.ctypes.data, 3, self.col_start.ctypes.data, out.ctypes.data))
        return out

    def PDP(self, P, psi):
        """P D P' psi with the products by dftk_mi_zgemm; psi: (nb, ld) block, result (nb, n_G)"""
        nb = psi.shape[0]
        one, zero = _lib.cplx(1.0), _lib.cplx(0.0)
        c = torch.empty((nb, self.n_p), dtype=torch.complex128, device=DEV)
        check(self.lib.dftk_mi_zgemm(self.bs.h, b"C", self.n_p, nb, self.n, one, P.data_ptr(), self.n, psi.data_ptr(),
                                     psi.stride(0), zero, c.data_ptr(), self.n_p))
        self.bs.sync()
        y = (c @ torch.from_numpy(np.ascontiguousarray(self.D.T)).to(DEV).to(torch.complex128)).contiguous()
        torch.cuda.synchronize()
        out = torch.empty((nb, self.n), dtype=torch.complex128, device=DEV)
        check(self.lib.dftk_mi_zgemm(self.bs.h, b"N", self.n, nb, self.n_p, one, P.data_ptr(), self.n, y.data_ptr(),
                                     self.n_p, zero, out.data_ptr(), self.n))
        self.bs.sync()
        return out.cpu().numpy()

    # ---- the new entries
    def dv(self, atom, pos=None):
        pos = self.pos if pos is None else pos
        out = torch.full((3, self.N), float("nan"), dtype=torch.float64, device=DEV)
        p = np.ascontiguousarray(pos[atom], dtype=np.float64)
        check(self.lib.dftk_mi_local_potential_displacement(self.cube.h, self.B.ctypes.data, self.par.shape[0],
                                                            self.par.ctypes.data, int(self.species[atom]), p.ctypes.data,
                                                            out.data_ptr()))
        self.bs.sync()
        return out.cpu().numpy()

    def dynmat_local(self, rho):
        out = np.full((len(self.species), 3, 3), np.nan)
        check(self.lib.dftk_mi_dynmat_local(self.cube.h, self.B.ctypes.data, self.par.shape[0], self.par.ctypes.data,
                                            len(self.species), self.species.ctypes.data, self.pos.ctypes.data,
                                            rho.data_ptr(), out.ctypes.data))
        return out

    def dH(self, atom, psi, status=False, out=None, ld_psi=None, ld_out=None, col_start=None, kb=None):
        nb = psi.shape[0]
        if out is None:
            out = torch.full((3, nb, self.n + PAD), float("nan"), dtype=torch.complex128, device=DEV)
        cs = self.col_start if col_start is None else col_start
        st = self.lib.dftk_mi_nonlocal_displacement_apply(kb or self.kb.h, self.kpt.ctypes.data, atom, 3, cs.ctypes.data, nb,
                                                          psi.data_ptr(), ld_psi or psi.stride(0), out.data_ptr(),
                                                          ld_out or out.stride(1))
        if status:
            return st, out
        check(st)
        self.bs.sync()
        return out

    def dynmat_nonlocal(self, psi, w, dpsi=None, wd=None, hess=True, status=False, kb=None, ld_psi=None):
        nb = psi.shape[0]
        w = np.ascontiguousarray(w, dtype=np.float64)
        wd = None if wd is None else np.ascontiguousarray(wd, dtype=np.float64)
        df, hs = np.zeros((3, 3)), np.zeros((3, 3, 3))
        if status:
            df[:], hs[:] = np.nan, np.nan
        st = self.lib.dftk_mi_dynmat_nonlocal(kb or self.kb.h, self.kpt.ctypes.data, nb, psi.data_ptr(),
                                              ld_psi or psi.stride(0), dpsi.data_ptr() if dpsi is not None else None,
                                              dpsi.stride(0) if dpsi is not None else 0, w.ctypes.data,
                                              wd.ctypes.data if wd is not None else None, 3, self.col_start.ctypes.data,
                                              df.ctypes.data if dpsi is not None else None, hs.ctypes.data if hess else None)
        if status:
            return st, df, hs
        check(st)
        return df, hs


def block(cell, nb, seed):
    """(nb, n_G + PAD) band-major block of random orbitals, NaN in the padding"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nb, cell.n)) + 1j * rng.standard_normal((nb, cell.n))
    buf = torch.full((nb, cell.n + PAD), float("nan"), dtype=torch.complex128, device=DEV)
    buf[:, :cell.n] = torch.from_numpy(x).to(DEV)
    return buf


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def cell(lib):
    return Cell(lib)


@pytest.fixture(scope="module")
def rho(cell):
    g = torch.Generator(device=DEV).manual_seed(11)
    return 0.02 + 0.1 * torch.rand(cell.N, dtype=torch.float64, device=DEV, generator=g)


def fd_report(name, got, fd1, fd2, measured, tol):
    yard = relmax(fd1, fd2)
    e1, e2 = relmax(got, fd1), relmax(got, fd2)
    print(f"\n{name}: rel err h=1e-3 {e1:.3e}, h=5e-4 {e2:.3e} (ratio {e1 / e2:.2f}); |FD(h) - FD(h/2)| {yard:.3e}; "
          f"recorded {measured:.1e}, TOL {tol:.1e}")
    assert 2.0 < e1 / e2 < 5.0
    assert e2 <= yard
    assert e2 < tol


# ------------------------------------------------------------------------------------------ 1: the dV cubes
@pytest.mark.parametrize("atom", [1, 2])
def test_displacement_cubes_against_central_differences_of_the_local_potential(cell, atom):
    got = cell.dv(atom)
    assert np.isfinite(got).all()
    fd = {}
    for h in (H1, H1 / 2):
        fd[h] = np.stack([(cell.superposition(cell.moved(atom, al, h)) - cell.superposition(cell.moved(atom, al, -h)))
                          / (2 * h) for al in range(3)])
    fd_report(f"dV cubes of atom {atom}", got, fd[H1], fd[H1 / 2], DV_MEASURED, DV_TOL)
    assert np.array_equal(got, cell.dv(atom))                                   # bitwise reproducible


# ------------------------------------------------------------------------------------------ 2: the local Hessian
def test_local_hessian_against_central_differences_of_the_local_forces(cell, rho):
    got = cell.dynmat_local(rho)
    assert np.isfinite(got).all()
    fd = {}
    for h in (H1, H1 / 2):
        out = np.zeros((3, 3, 3))
        for a in range(3):
            for al in range(3):
                Fp = cell.forces_local(cell.moved(a, al, h), rho)
                Fm = cell.forces_local(cell.moved(a, al, -h), rho)
                out[a, :, al] = -(Fp[a] - Fm[a]) / (2 * h)
                other = [t for t in range(3) if t != a]
                assert np.abs(Fp[other] - Fm[other]).max() <= RND * np.abs(Fp).max()     # no cross term at fixed density
        fd[h] = out
    fd_report("dynmat_local", got, fd[H1], fd[H1 / 2], LOCAL_MEASURED, LOCAL_TOL)
    assert np.array_equal(got, got.transpose(0, 2, 1))                            # symmetric in alpha, beta
    assert np.array_equal(got, cell.dynmat_local(rho))


# ------------------------------------------------------------------------------------------ 3: nonlocal dH psi
@pytest.mark.parametrize("atom", [1, 2])
@pytest.mark.parametrize("nb", [1, NB])
def test_nonlocal_displacement_against_rebuilt_projectors(cell, atom, nb):
    psi = block(cell, nb, 3)
    out = cell.dH(atom, psi)
    got = out[:, :, :cell.n].cpu().numpy()
    assert np.isfinite(got).all() and torch.isnan(out[:, :, cell.n:]).all()       # the padding rows are untouched
    fd = {}
    for h in (H1, H1 / 2):
        fd[h] = np.stack([(cell.PDP(cell.projectors(cell.moved(atom, al, h)), psi)
                           - cell.PDP(cell.projectors(cell.moved(atom, al, -h)), psi)) / (2 * h) for al in range(3)])
    fd_report(f"nonlocal dH psi of atom {atom}, {nb} band(s)", got, fd[H1], fd[H1 / 2], DHPSI_MEASURED, DHPSI_TOL)
    again = cell.dH(atom, psi)
    assert torch.equal(torch.view_as_real(again[:, :, :cell.n]), torch.view_as_real(out[:, :, :cell.n]))
    # Hermitian: <phi|dH psi> = conj <psi|dH phi>  (exact in exact arithmetic: rounding only)
    if nb > 1:
        x = psi[:, :cell.n].cpu().numpy()
        for al in range(3):
            M = x.conj() @ got[al].T
            assert np.abs(M - M.conj().T).max() <= RND * np.abs(M).max()


# ------------------------------------------------------------------------------------------ 4, 5: dforces
def test_dforces_is_the_derivative_of_the_nonlocal_forces(cell):
    psi, dpsi = block(cell, NB, 5), block(cell, NB, 6)
    w = np.array([2.0, 1.3, 0.4]) / 3
    dw = np.array([0.3, -0.7, 0.2])
    zero = np.zeros(NB)
    # along dpsi: F_nl is quadratic in psi, the central difference is exact for any step (rounding only)
    h = 0.5
    plus, minus = psi.clone(), psi.clone()
    plus[:, :cell.n] += h * dpsi[:, :cell.n]
    minus[:, :cell.n] -= h * dpsi[:, :cell.n]
    Fp, Fm = cell.forces_nonlocal(plus, w), cell.forces_nonlocal(minus, w)
    got, _ = cell.dynmat_nonlocal(psi, w, dpsi, zero, hess=False)
    err = np.abs(got - (Fp - Fm) / (2 * h)).max()
    print(f"\ndforces along dpsi: abs err {err:.3e} of {np.abs(Fp).max():.3e}")
    assert err <= RND / h * max(np.abs(Fp).max(), np.abs(Fm).max())
    # along dw: F_nl is linear in w
    ref = cell.forces_nonlocal(psi, dw)
    got_w, _ = cell.dynmat_nonlocal(psi, zero, torch.zeros_like(dpsi), dw, hess=False)
    print(f"dforces along dw: rel err {relmax(got_w, ref):.3e}")
    assert np.abs(got_w - ref).max() <= RND * np.abs(ref).max()
    # both at once, accumulated onto what the output holds; twice the same bits
    both, _ = cell.dynmat_nonlocal(psi, w, dpsi, dw, hess=False)
    assert np.abs(both - (got + got_w)).max() <= RND * np.abs(both).max()
    assert np.array_equal(both, cell.dynmat_nonlocal(psi, w, dpsi, dw, hess=False)[0])


# ------------------------------------------------------------------------------------------ 6: the nonlocal Hessian
def test_nonlocal_hessian_against_central_differences_of_the_nonlocal_forces(cell):
    psi = block(cell, NB, 7)
    w = np.array([2.0, 1.3, 0.4]) / 3
    _, got = cell.dynmat_nonlocal(psi, w)
    fd = {}
    try:
        for h in (H1, H1 / 2):
            out = np.zeros((3, 3, 3))
            for a in range(3):
                for al in range(3):
                    F = []
                    for sign in (1, -1):
                        P = cell.projectors(cell.moved(a, al, sign * h))
                        cell.bind(P)
                        F.append(cell.forces_nonlocal(psi, w))
                    out[a, :, al] = -(F[0][a] - F[1][a]) / (2 * h)
            fd[h] = out
    finally:
        cell.bind(cell.P)
    fd_report("nonlocal Hessian", got, fd[H1], fd[H1 / 2], HESS_MEASURED, HESS_TOL)
    assert np.abs(got - got.transpose(0, 2, 1)).max() == 0.0
    _, again = cell.dynmat_nonlocal(psi, w)
    assert np.array_equal(got, again)
    # accumulation: a second call adds onto the first
    hs = got.copy()
    check(cell.lib.dftk_mi_dynmat_nonlocal(cell.kb.h, cell.kpt.ctypes.data, NB, psi.data_ptr(), psi.stride(0), None, 0,
                                           np.ascontiguousarray(w).ctypes.data, None, 3, cell.col_start.ctypes.data, None,
                                           hs.ctypes.data))
    assert np.array_equal(hs, 2 * got)


# ------------------------------------------------------------------------------------------ 7: Gamma-real block
def test_gamma_real_block_gives_what_the_complex_block_gives(lib):
    out = []
    for gamma_real in (False, True):
        c = Cell(lib, kpt=np.zeros(3), gamma_real=gamma_real)
        psi, dpsi = block(c, NB, 8), block(c, NB, 9)
        w, dw = np.array([2.0, 1.3, 0.4]), np.array([0.3, -0.7, 0.2])
        dh = c.dH(1, psi)[:, :, :c.n].cpu().numpy()
        df, hs = c.dynmat_nonlocal(psi, w, dpsi, dw)
        out.append((dh, df, hs))
    for a, b in zip(out[0], out[1]):
        assert np.abs(b).max() > 0 and np.abs(a - b).max() <= RND * np.abs(a).max()


# ------------------------------------------------------------------------------------------ band chunks (closed forms)
def test_band_chunks_against_the_closed_forms_on_a_large_sphere(lib):
    """~1.1e5 sphere rows, 7 bands: one band more than the chunk of dftk_mi_dynmat_nonlocal (6 + 1) and two chunks of
    dftk_mi_nonlocal_displacement_apply (4 + 3).  The chunk is budget / per-band bytes with
    budget = max(T1, 64 MiB) (a fresh basis has run no FFT: T1 is empty) and per band 8 (rows + n_atom_columns) complex
    numbers for dftk_mi_nonlocal_displacement_apply, 6 rows + 14 n_p for dftk_mi_dynmat_nonlocal.  Random P and banded D:
    the closed forms of the header in numpy are exact, the bound is rounding."""
    from test_gpu_kernels import Basis, KBlock
    n = 64
    ax = np.array(dftk.basis.G_axis(n))
    gz, gy, gx = np.meshgrid(ax, ax, ax, indexing="ij")
    mapping = np.nonzero((gx * gx + gy * gy + gz * gz <= 884).reshape(-1))[0]
    G = np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], axis=1)[mapping].astype(float)
    rows, nb = len(mapping), 7
    col_start = np.array([0, 4, 4, 13], dtype=np.int32)
    n_p, atom = 13, 2
    budget = 64 << 20
    cb3, cb4 = budget // (8 * (rows + 9) * 16), budget // ((6 * rows + 14 * n_p) * 16)
    assert 1 < cb3 < nb and 1 < cb4 < nb and nb in (cb3 + 1, cb4 + 1), (rows, cb3, cb4)
    rng = np.random.default_rng(43)
    P = rng.standard_normal((rows, n_p)) + 1j * rng.standard_normal((rows, n_p))
    D = np.zeros((n_p, n_p))
    for c0, c1, bw in ((0, 4, 1), (4, 13, 2)):
        for i in range(c0, c1):
            for j in range(i, min(c1, i + bw + 1)):
                D[i, j] = D[j, i] = rng.uniform(-2, 2)
    bs = Basis(lib, n, n, n)
    kb = KBlock(lib, bs, mapping, np.zeros(rows))
    kb.set_projectors(P, D)
    ld = rows + 37

    def padded(x):
        buf = torch.full((x.shape[1], ld), float("nan"), dtype=torch.complex128, device=DEV)
        buf[:, :rows] = torch.from_numpy(np.ascontiguousarray(x.T))
        return buf
    psi = rng.standard_normal((rows, nb)) + 1j * rng.standard_normal((rows, nb))
    dpsi = rng.standard_normal((rows, nb)) + 1j * rng.standard_normal((rows, nb))
    w, dw = rng.uniform(0.2, 2.0, nb), rng.uniform(-1.0, 1.0, nb)
    kpt = np.array([0.13, -0.27, 0.41])
    g = G + kpt[None, :]
    pd, dd = padded(psi), padded(dpsi)
    # dH psi of the atom with 9 columns; the atom without columns gives zero
    out = torch.full((3, nb, ld), float("nan"), dtype=torch.complex128, device=DEV)
    for a in (atom, 1):
        check(lib.dftk_mi_nonlocal_displacement_apply(kb.h, kpt.ctypes.data, a, 3, col_start.ctypes.data, nb, pd.data_ptr(), ld,
                                                      out.data_ptr(), ld))
        bs.sync()
        got = out[:, :, :rows].cpu().numpy()
        assert torch.isnan(out[:, :, rows:]).all()
        if a == 1:
            assert np.all(got == 0)
            continue
        c0, c1 = col_start[a], col_start[a + 1]
        Ps, Ds = P[:, c0:c1], D[c0:c1, c0:c1]
        for al in range(3):
            ref = -2j * np.pi * (g[:, al, None] * (Ps @ (Ds @ (Ps.conj().T @ psi)))
                                 - Ps @ (Ds @ (Ps.conj().T @ (g[:, al, None] * psi))))
            assert np.abs(got[al].T - ref).max() <= RND * np.abs(ref).max(), al
    # dforces and hess
    df, hs = np.zeros((3, 3)), np.zeros((3, 3, 3))
    check(lib.dftk_mi_dynmat_nonlocal(kb.h, kpt.ctypes.data, nb, pd.data_ptr(), ld, dd.data_ptr(), ld, w.ctypes.data,
                                      dw.ctypes.data, 3, col_start.ctypes.data, df.ctypes.data, hs.ctypes.data))
    Ph = P.conj().T
    c, dc = Ph @ psi, Ph @ dpsi
    ca = [Ph @ (g[:, al, None] * psi) for al in range(3)]
    dca = [Ph @ (g[:, al, None] * dpsi) for al in range(3)]
    df_ref, hs_ref = np.zeros((3, 3)), np.zeros((3, 3, 3))
    for a in range(3):
        s = slice(col_start[a], col_start[a + 1])
        Ds = D[s, s]
        for al in range(3):
            # F = -4 pi sum w Re[p' D (i c_alpha)]
            f = lambda x, y: np.real(np.sum(x[s].conj() * (Ds @ (1j * y[s])), axis=0))      # noqa: E731
            df_ref[a, al] = -4 * np.pi * (np.dot(dw, f(c, ca[al])) + np.dot(w, f(dc, ca[al]) + f(c, dca[al])))
            for be in range(3):
                cab = Ph @ (g[:, al, None] * g[:, be, None] * psi)
                val = np.real(np.sum(ca[al][s].conj() * (Ds @ ca[be][s]) - cab[s].conj() * (Ds @ c[s]), axis=0))
                hs_ref[a, be, al] = 8 * np.pi ** 2 * np.dot(w, val)
    assert np.all(df[1] == 0) and np.all(hs[1] == 0)
    assert np.abs(df - df_ref).max() <= RND * np.abs(df_ref).max(), (df, df_ref)
    assert np.abs(hs - hs_ref).max() <= RND * np.abs(hs_ref).max(), (hs, hs_ref)


# ------------------------------------------------------------------------------------------ 9: refusals
def test_refusals_leave_the_outputs_untouched(cell, rho):
    lib = cell.lib
    from test_gpu_kernels import KBlock
    psi, dpsi = block(cell, NB, 12), block(cell, NB, 13)
    w = np.ones(NB)
    out = torch.full((3, NB, cell.n + PAD), float("nan"), dtype=torch.complex128, device=DEV)

    def refused_dH(word=None, **kw):
        st, _ = cell.dH(kw.pop("atom", 1), psi, status=True, out=out, **kw)
        assert st == EINVAL, kw
        if word:
            assert word in lib.dftk_mi_last_error().decode(), lib.dftk_mi_last_error()

    def refused_dyn(word=None, **kw):
        st, df, hs = cell.dynmat_nonlocal(psi, w, dpsi, w, status=True, **kw)
        assert st == EINVAL, kw
        assert np.isnan(df).all() and np.isnan(hs).all()
        if word:
            assert word in lib.dftk_mi_last_error().decode(), lib.dftk_mi_last_error()

    refused_dH("leading dimension", ld_psi=cell.n - 1)
    refused_dH("leading dimension", ld_out=cell.n - 1)
    refused_dH(atom=3)
    refused_dH("col_start", col_start=np.array([0, 14, 28, 32], dtype=np.int32))
    refused_dyn("leading dimension", ld_psi=cell.n - 1)
    # a D that couples two atoms (columns 13 and 14 belong to the two Fe atoms)
    Dc = cell.D.copy()
    Dc[13, 14] = Dc[14, 13] = 0.5
    try:
        cell.bind(cell.P, np.asfortranarray(Dc))
        refused_dH("couples", atom=0)
        refused_dH("couples", atom=1)
        refused_dyn("couples")
    finally:
        cell.bind(cell.P)
    # a block sharded over two ranks (the communicator is never used: the calls are refused before any work)
    kb2 = KBlock(lib, cell.bs, cell.mapping, np.zeros(cell.n))
    cb = ALLREDUCE_FN(lambda user, data, count: 0)
    comm = C.c_void_p()
    check(lib.dftk_mi_comm_create_host(2, 0, 0, cb, None, None, C.byref(comm)))
    rows = np.array([0, cell.n // 2, cell.n], dtype=np.int64)
    check(lib.dftk_mi_kblock_set_shard(kb2.h, comm, rows.ctypes.data))
    check(lib.dftk_mi_kblock_set_projectors(kb2.h, cell.n_p, cell.P.data_ptr(), cell.n, cell.D.ctypes.data))
    refused_dH("sharded", kb=kb2.h)
    refused_dyn("sharded", kb=kb2.h)
    check(lib.dftk_mi_kblock_set_shard(kb2.h, None, None))
    check(lib.dftk_mi_comm_destroy(comm))
    cell.bs.sync()
    assert torch.isnan(out).all() and torch.all(out.imag == 0)                 # no refused call wrote anything (NaN + 0 i)
    # the cube entries: a block that is not the whole cube, a species out of range
    cubes = torch.full((3, cell.N), float("nan"), dtype=torch.float64, device=DEV)
    p = np.ascontiguousarray(cell.pos[1])
    for kbh, sp in ((cell.kb.h, 0), (cell.cube.h, 2), (cell.cube.h, -1)):
        assert lib.dftk_mi_local_potential_displacement(kbh, cell.B.ctypes.data, 2, cell.par.ctypes.data, sp, p.ctypes.data,
                                                        cubes.data_ptr()) == EINVAL
    hl = np.full((3, 3, 3), np.nan)
    assert lib.dftk_mi_dynmat_local(cell.kb.h, cell.B.ctypes.data, 2, cell.par.ctypes.data, 3, cell.species.ctypes.data,
                                    cell.pos.ctypes.data, rho.data_ptr(), hl.ctypes.data) == EINVAL
    ungrouped = np.array([0, 1, 0], dtype=np.int32)
    assert lib.dftk_mi_dynmat_local(cell.cube.h, cell.B.ctypes.data, 2, cell.par.ctypes.data, 3, ungrouped.ctypes.data,
                                    cell.pos.ctypes.data, rho.data_ptr(), hl.ctypes.data) == EINVAL
    cell.bs.sync()
    assert torch.isnan(cubes).all() and np.isnan(hl).all()
    # ... and the block still works
    assert torch.isfinite(torch.view_as_real(cell.dH(1, psi)[:, :, :cell.n])).all()
