"""The plane-wave sharded path of ONE k-block at the C ABI, 2-4 ranks as threads of this process (tests/shard_ranks.py):
dftk_mi_kblock_set_shard, the slab <-> band all-to-alls of csrc/api.cpp, the sharded branches of the Gamma-real
kernels, of dftk_mi_lobpcg and of the nonlocal forces, comm_alltoallv / comm_allreduce of the host-staged communicator.

Every result is compared with the CPU oracle's Hamiltonian / density on the WHOLE sphere (tests/gamma_ref.py for the
half format), at the layouts where an offset can go wrong unnoticed: complex (k != 0) and Gamma-real blocks, uneven row
slabs down to one row, ranks that own no band, odd band shares on a Gamma-real block (half-empty last pair),
non-uniform weights, three and four ranks.  Row slabs of the half format are the library's own even split, independent
of the caller's full-sphere split: gamma_apply_H, the half-format projectors and LOBPCG's load / store cross the two.

Spheres: the 2-atom Si cell at Ecut 5 on (15, 15, 15) and (16, 15, 18), a few hundred plane waves each.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402
from dftk_jl_amd.comm import split_evenly  # noqa: E402
from dftk_jl_amd.terms import projector_species_tables  # noqa: E402

from oracle import energy_hamiltonian  # noqa: E402
from oracle.scf import compute_density  # noqa: E402

import gamma_ref as gr  # noqa: E402
from shard_ranks import RankGroup  # noqa: E402
from test_gpu_kernels import RTOL, Basis, KBlock, dev, make_oracle_basis, relerr  # noqa: E402

EINVAL = -1
ECUT = 5
CUBES = [(15, 15, 15), (16, 15, 18)]
IK = {"complex": 1, "gamma": 0}          # k-points of make_oracle_basis: [0, 0, 0] and [1/3, 0.1, -0.25]
LAYOUTS = {"p2-even": 2, "p3-uneven": 3, "p4-even": 4}
WEIGHTS = np.array([2.0, 0.0, 1.3, 0.5, 1.7, 0.0, 0.9, 0.25, 1.1])      # all different where not zero
NAN = complex(np.nan, np.nan)
GUARD = 7                                 # elements beyond the guard column


def row_starts(layout, n):
    p = LAYOUTS[layout]
    if layout == "p3-uneven":
        return np.array([0, 1, n - 7, n], dtype=np.int64)                 # a one-row slab, a 7-row slab
    return np.array([r.start for r in split_evenly(n, p)] + [n], dtype=np.int64)


def band_counts(layout):
    p = LAYOUTS[layout]
    return sorted({1, p - 1, p, p + 1, 2 * p + 1, 9})


CASES = [(layout, nb) for layout in LAYOUTS for nb in band_counts(layout)]
GRID = [(dims, layout, nb) for dims in CUBES for layout, nb in CASES]
GRID_IDS = ["x".join(map(str, d)) + f"-{lay}-nb{nb}" for d, lay, nb in GRID]


def even_starts(n, p):
    return np.array([r.start for r in split_evenly(n, p)] + [n], dtype=np.int64)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


# ------------------------------------------------------------------------------------------ the oracle, once per cube
class Cube:
    def __init__(self, lib, dims):
        self.dims = dims
        nx, ny, nz = dims
        self.obasis = make_oracle_basis(ECUT, dims)
        rng = np.random.default_rng(42)
        self.V = self.obasis.terms.V_loc + 0.1 * rng.standard_normal((nz, ny, nx))   # generic real potential
        _, self.ham = energy_hamiltonian(self.obasis, None, None)
        for H in self.ham:
            H.potential = self.V
        self.vol = self.obasis.model.unit_cell_volume
        # the Gamma sphere is accepted by the half format (inversion-closed, no Nyquist point): host check
        m = np.ascontiguousarray(self.obasis.kpoints[0].mapping, dtype=np.int64)
        cnt = C.c_int64()
        g, mg = np.zeros(len(m), dtype=np.int32), np.zeros(len(m), dtype=np.int32)
        check(lib.dftk_mi_gamma_tables_host(nx, ny, nz, len(m), m.ctypes.data, C.byref(cnt), g.ctypes.data, mg.ctypes.data))
        self.n_half = cnt.value
        self.g, self.mg = g[:self.n_half].astype(np.int64), mg[:self.n_half].astype(np.int64)
        rg, rmg = gr.pairs(dims, m)
        assert self.n_half == (len(m) + 1) // 2 and np.array_equal(self.g, rg) and np.array_equal(self.mg, rmg)
        self._dense = {}

    def H(self, kind):
        return self.ham[IK[kind]]

    def kcoord(self, kind):
        return np.ascontiguousarray(self.obasis.kpoints[IK[kind]].coordinate, dtype=np.float64)

    def dense_eigenvalues(self, kind):
        if kind not in self._dense:
            self._dense[kind] = np.linalg.eigvalsh(self.H(kind).to_dense())
        return self._dense[kind]

    def density(self, kind, psi, occ):
        """compute_density of the oracle with only the k-point of ``kind`` occupied"""
        psis = [np.zeros((len(k.mapping), 1), dtype=complex) for k in self.obasis.kpoints]
        occs = [np.zeros(1) for _ in self.obasis.kpoints]
        psis[IK[kind]], occs[IK[kind]] = psi, occ
        return compute_density(self.obasis, psis, occs)

    def weights(self, kind, occ):
        return np.ascontiguousarray(occ * self.obasis.kweights[IK[kind]] * self.obasis.ifft_normalization ** 2)


class Ranks:
    """p ranks of one sharded block: per rank a basis, a communicator, a k-block, set up in the order of the header."""

    def __init__(self, lib, cube, kind, layout, group=None, P=None):
        self.lib, self.cube, self.kind, self.layout = lib, cube, kind, layout
        self.p = LAYOUTS[layout]
        self.group = group if group is not None else RankGroup(self.p)
        H = self.H = cube.H(kind)
        self.n = H.n_G
        self.rows = row_starts(layout, self.n)
        self.hrows = even_starts(cube.n_half, self.p) if kind == "gamma" else None
        self.bases, self.kbs = [None] * self.p, [None] * self.p
        P = H.P if P is None else P
        nx, ny, nz = cube.dims

        def setup(r, comm):
            bs = Basis(lib, nx, ny, nz, cube.vol)
            kb = KBlock(lib, bs, H.kpoint.mapping, H.kinetic)
            check(lib.dftk_mi_kblock_set_shard(kb.h, comm, self.rows.ctypes.data))
            kb.set_projectors(P[self.rows[r]:self.rows[r + 1]], H.D)
            kb.set_potential(cube.V)
            if kind == "gamma":
                check(lib.dftk_mi_kblock_set_gamma_real(kb.h, 1))
                hl = C.c_int64()
                check(lib.dftk_mi_gamma_half_size(kb.h, C.byref(hl)))
                assert hl.value == self.hrows[r + 1] - self.hrows[r]
            self.bases[r], self.kbs[r] = bs, kb

        self.group.run(setup)

    def nloc(self, r):
        return int(self.rows[r + 1] - self.rows[r])

    def hloc(self, r):
        return int(self.hrows[r + 1] - self.hrows[r])

    def mine(self, r, nb):
        return nb // self.p + (1 if r < nb % self.p else 0)

    def close(self):
        self.kbs, self.bases = [], []
        self.group.close()


@pytest.fixture(scope="module")
def world(lib):
    cubes, ranks = {}, {}

    class World:
        def cube(self, dims):
            if dims not in cubes:
                cubes[dims] = Cube(lib, dims)
            return cubes[dims]

        def ranks(self, dims, kind, layout):
            key = (dims, kind, layout)
            if key not in ranks:
                ranks[key] = Ranks(lib, self.cube(dims), kind, layout)
            return ranks[key]

    yield World()
    for rk in ranks.values():
        rk.close()


# ------------------------------------------------------------------------------------------ packed blocks with guards
def slab_in(X, r0, r1):
    """rows [r0, r1) of the (n, nb) block as a packed column-major device block (ld == r1 - r0)"""
    return dev(np.ascontiguousarray(X[r0:r1].T))


class OutSlab:
    """NaN-filled packed output block of rows x nb, one guard column and GUARD elements more behind it"""

    def __init__(self, rows, nb):
        self.rows, self.nb = rows, nb
        self.host = np.full(rows * (nb + 1) + GUARD, NAN)
        self.t = torch.from_numpy(self.host.copy()).cuda()

    def ptr(self):
        return self.t.data_ptr()

    def take(self, written=True):
        after = self.t.cpu().numpy()
        used = self.rows * self.nb if written else 0
        assert np.array_equal(after[used:].view(np.uint64), self.host[used:].view(np.uint64)), "guard / refused output written"
        return after[:self.rows * self.nb].reshape(self.nb, self.rows).T.copy()


def random_block(seed, n, nb):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, nb)) + 1j * rng.standard_normal((n, nb))


# ------------------------------------------------------------------------------------------ a. complex H psi
@pytest.mark.parametrize("dims,layout,nb", GRID, ids=GRID_IDS)
def test_complex_apply_H_parts(lib, world, dims, layout, nb):
    """dftk_mi_apply_H_parts on a sharded k != 0 block (the ``else`` branch: slab -> band, pipeline on this rank's bands,
    band -> slab, then P D P' with the all-reduced projections): every part and the sums against the oracle."""
    rk = world.ranks(dims, "complex", layout)
    H = rk.H
    psi = np.linalg.qr(random_block(nb, rk.n, nb))[0]
    loc, kin, nl = H.apply_local(psi), H.kinetic[:, None] * psi, H.apply_nonlocal(psi)
    refs = {1: loc, 2: kin, 4: nl, 3: loc + kin, 7: H.mul(psi)}

    def fn(r, _comm):
        pd = slab_in(psi, rk.rows[r], rk.rows[r + 1])
        got = {}
        for which in refs:
            out = OutSlab(rk.nloc(r), nb)
            torch.cuda.synchronize()
            check(lib.dftk_mi_apply_H_parts(rk.kbs[r].h, which, nb, pd.data_ptr(), rk.nloc(r), out.ptr(), rk.nloc(r)))
            rk.bases[r].sync()
            got[which] = out.take()
        return got

    res = rk.group.run(fn)
    for which, ref in refs.items():
        full = np.concatenate([res[r][which] for r in range(rk.p)], axis=0)
        assert relerr(full, ref) < RTOL, (which, relerr(full, ref))


# ------------------------------------------------------------------------------------------ b / d. densities
def _density_case(lib, rk, nb, psi, entry):
    cube = rk.cube
    occ = WEIGHTS[:nb]
    w = cube.weights(rk.kind, occ)
    nx, ny, nz = cube.dims
    ref = cube.density(rk.kind, psi, occ)

    def fn(r, _comm):
        pd = slab_in(psi, rk.rows[r], rk.rows[r + 1])
        rho = torch.zeros(nz * ny * nx + GUARD, dtype=torch.float64, device="cuda")
        rho[nz * ny * nx:] = float("nan")                 # guard behind the cube
        torch.cuda.synchronize()
        check(entry(rk.kbs[r].h, nb, pd.data_ptr(), rk.nloc(r), w.ctypes.data, rho.data_ptr()))
        rk.bases[r].sync()
        host = rho.cpu().numpy()
        assert np.isnan(host[nz * ny * nx:]).all()
        return host[:nz * ny * nx].reshape(nz, ny, nx).copy()

    parts = rk.group.run(fn)
    total = np.zeros_like(parts[0])
    for part in parts:
        total += part
    assert relerr(total, ref) < RTOL, relerr(total, ref)
    c0 = 0
    for r in range(rk.p):
        mine = rk.mine(r, nb)
        if mine == 0 or not np.any(occ[c0:c0 + mine]):
            assert not parts[r].view(np.uint64).any(), f"rank {r} owns no weighted band: its cube stays bitwise zero"
        else:       # each rank adds exactly ITS bands with THEIR weights
            own = np.zeros(nb)
            own[c0:c0 + mine] = occ[c0:c0 + mine]
            assert relerr(parts[r], cube.density(rk.kind, psi, own)) < RTOL, r
        c0 += mine
    if nb == 2 * rk.p + 1:      # (no symmetry hides a misplaced weight: the reference itself moves with a permutation)
        assert relerr(cube.density(rk.kind, psi, occ[::-1]), ref) > 1e-3


@pytest.mark.parametrize("dims,layout,nb", GRID, ids=GRID_IDS)
def test_complex_density_accumulate(lib, world, dims, layout, nb):
    """dftk_mi_density_accumulate on a sharded complex block: rank r adds the bands [c0[r], c0[r+1]) with the weights at
    the same offset (``weight_h + t.c0[t.me]``) into ITS cube; the p cubes sum to the oracle's density."""
    rk = world.ranks(dims, "complex", layout)
    psi = np.linalg.qr(random_block(100 + nb, rk.n, nb))[0]
    _density_case(lib, rk, nb, psi, lib.dftk_mi_density_accumulate)


@pytest.mark.parametrize("dims,layout,nb", GRID, ids=GRID_IDS)
def test_gamma_density_accumulate_real(lib, world, dims, layout, nb):
    """dftk_mi_density_accumulate_real on the sharded Gamma-real block (gamma_density_sharded: two real-symmetric bands
    per transform, an odd share leaves the last pair half empty, ``w_h + t.c0[t.me]``)."""
    rk = world.ranks(dims, "gamma", layout)
    rng = np.random.default_rng(200 + nb)
    psi = gr.symmetric_columns(rng, rk.cube.g, rk.cube.mg, rk.n, nb)
    _density_case(lib, rk, nb, psi, lib.dftk_mi_density_accumulate_real)


# ------------------------------------------------------------------------------------------ c. Gamma-real H psi
def _gamma_refs(rk, h, whichs):
    H, cube = rk.H, rk.cube
    local = lambda c: H.apply_local(np.ascontiguousarray(c.T)).T       # noqa: E731  (nb, n) -> (nb, n)
    return {w: gr.apply_H(h, cube.g, cube.mg, rk.n, w, local, H.kinetic, H.P, H.D, dtype=np.float64) for w in whichs}


def _gamma_apply(lib, rk, h, whichs, written=True, expect=0):
    nb = h.shape[1]

    def fn(r, _comm):
        hd = slab_in(h, rk.hrows[r], rk.hrows[r + 1])
        got = {}
        for which in whichs:
            out = OutSlab(rk.hloc(r), nb)
            torch.cuda.synchronize()
            st = lib.dftk_mi_gamma_apply_H(rk.kbs[r].h, which, nb, hd.data_ptr(), rk.hloc(r), out.ptr(), rk.hloc(r))
            msg = lib.dftk_mi_last_error().decode(errors="replace")
            rk.bases[r].sync()
            assert st == expect, (r, which, st, msg)
            got[which] = (out.take(written), msg)
        return got

    return rk.group.run(fn)


@pytest.mark.parametrize("dims,layout,nb", GRID, ids=GRID_IDS)
def test_gamma_apply_H(lib, world, dims, layout, nb):
    """dftk_mi_gamma_apply_H on half-format row slabs (the library's even split of n_half, computed here and checked
    against dftk_mi_gamma_half_size at set-up) against the oracle Hamiltonian restricted to the half format.  The band
    counts give odd and even shares (``mine2 = (mine + 1) / 2``) and ranks without a band; ``which`` = 4 and 7 use the
    half-format projectors, built from full-sphere row slabs of ANOTHER split."""
    rk = world.ranks(dims, "gamma", layout)
    h = gr.half_columns(np.random.default_rng(300 + nb), rk.cube.n_half, nb)
    whichs = (1, 2, 4, 7)
    refs = _gamma_refs(rk, h, whichs)
    res = _gamma_apply(lib, rk, h, whichs)
    for which in whichs:
        full = np.concatenate([res[r][which][0] for r in range(rk.p)], axis=0)
        assert relerr(full, refs[which]) < RTOL, (which, relerr(full, refs[which]))


# ------------------------------------------------------------------------------------------ e. projector refusal
@pytest.mark.parametrize("layout,bad_rank", [("p2-even", 1), ("p3-uneven", 1), ("p4-even", 2)])
def test_gamma_projectors_refused_on_every_rank(lib, world, layout, bad_rank):
    """One element of P on ONE rank's slab breaks P(-G) = conj P(G): only the rank that transforms that projector column
    sees it, the flag is all-reduced, and dftk_mi_gamma_apply_H (which = 4) returns EINVAL on EVERY rank with nothing
    written.  With the projectors restored (set_projectors on every rank: the call is collective in effect, it drops the
    half-format copy) the same call succeeds and matches the oracle."""
    dims, nb = CUBES[1], 5
    cube = world.cube(dims)
    H = cube.H("gamma")
    rows = row_starts(layout, H.n_G)
    row = int(rows[bad_rank + 1]) - 1                      # a row of that rank's slab, not G = 0
    assert row != cube.g[0]
    Pbad = np.array(H.P, dtype=complex)
    Pbad[row, 3] += 1e-3 * np.abs(H.P).max()
    rk = Ranks(lib, cube, "gamma", layout, P=Pbad)
    try:
        h = gr.half_columns(np.random.default_rng(5), cube.n_half, nb)
        res = _gamma_apply(lib, rk, h, (4,), written=False, expect=EINVAL)
        assert all("real-symmetric" in res[r][4][1] for r in range(rk.p)), [res[r][4][1] for r in range(rk.p)]
        rk.group.run(lambda r, _c: rk.kbs[r].set_projectors(H.P[rows[r]:rows[r + 1]], H.D))
        res = _gamma_apply(lib, rk, h, (4,))
        full = np.concatenate([res[r][4][0] for r in range(rk.p)], axis=0)
        ref = _gamma_refs(rk, h, (4,))[4]
        assert relerr(full, ref) < RTOL, relerr(full, ref)
    finally:
        rk.close()


# ------------------------------------------------------------------------------------------ f. LOBPCG
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("layout", ["p2-even", "p3-uneven"])
@pytest.mark.parametrize("kind", ["complex", "gamma"])
@pytest.mark.parametrize("dims", CUBES, ids=lambda d: "x".join(map(str, d)))
def test_lobpcg(lib, world, dims, kind, layout, M):
    """dftk_mi_lobpcg on row slabs of one random start block.  Every Gram product is a local partial sum + all-reduce
    (``reduce_c`` / ``reduce_d``), every decision (convergence, locking, Cholesky fall-back) is taken from reduced
    numbers: all ranks must report bitwise equal lambda / resid / n_iter / converged.  Eigenvalues against the dense
    oracle Hamiltonian (the bound of test_lobpcg_core_hamiltonian_vs_oracle_and_dense), the gathered X orthonormal and a
    true eigenbasis under the ORACLE's H; a Gamma-real block returns real-symmetric columns."""
    rk = world.ranks(dims, kind, layout)
    H, tol = rk.H, 1e-8
    X0 = np.linalg.qr(random_block(7 * M + rk.p, rk.n, M))[0]

    def fn(r, _comm):
        Xd = slab_in(X0, rk.rows[r], rk.rows[r + 1])
        lam, res = np.zeros(M), np.zeros(M)
        n_iter, conv, nmv = C.c_int(), C.c_int(), C.c_int64()
        torch.cuda.synchronize()
        check(lib.dftk_mi_lobpcg(rk.kbs[r].h, M, Xd.data_ptr(), rk.nloc(r), tol, 1, 200, 0, 1, 1234, lam.ctypes.data,
                                 res.ctypes.data, C.byref(n_iter), C.byref(conv), C.byref(nmv)))
        rk.bases[r].sync()
        return lam, res, n_iter.value, conv.value, nmv.value, Xd.cpu().numpy().T

    out = rk.group.run(fn)
    lam, res, n_iter, conv, _, _ = out[0]
    for r in range(1, rk.p):
        assert np.array_equal(out[r][0].view(np.uint64), lam.view(np.uint64)), r
        assert np.array_equal(out[r][1].view(np.uint64), res.view(np.uint64)), r
        assert out[r][2:5] == out[0][2:5], (r, out[r][2:5], out[0][2:5])
    assert conv == 1 and n_iter < 200
    np.testing.assert_allclose(lam, rk.cube.dense_eigenvalues(kind)[:M], atol=1e-9)
    X = np.concatenate([out[r][5] for r in range(rk.p)], axis=0)
    assert np.linalg.norm(X.conj().T @ X - np.eye(M)) < 1e-10
    true_res = np.linalg.norm(H.mul(X) - X * lam[None, :], axis=0)
    print("n_iter", n_iter, "reported", res, "true", true_res)
    assert true_res.max() <= tol, true_res
    if kind == "gamma":
        g, mg = rk.cube.g, rk.cube.mg
        assert np.array_equal(X[mg[1:]], X[g[1:]].conj()) and np.all(X[g[0]].imag == 0)      # expand writes both from one h


# ------------------------------------------------------------------------------------------ g. forces and stress
def _force_args(cube):
    n_psp, rp, nproj, species, pos, col_start = projector_species_tables(cube.obasis.model)
    return n_psp, rp, nproj, species, pos, np.ascontiguousarray(col_start, dtype=np.int32)


def _forces(lib, kb, kcoord, psi_d, ld, w, col_start, prefill):
    out = np.array(prefill, dtype=np.float64)
    nb = len(w)
    check(lib.dftk_mi_forces_nonlocal(kb.h, kcoord.ctypes.data, nb, psi_d.data_ptr(), ld, w.ctypes.data, len(col_start) - 1,
                                      col_start.ctypes.data, out.ctypes.data))
    return out


@pytest.mark.parametrize("layout", ["p2-even", "p3-uneven"])
@pytest.mark.parametrize("kind", ["complex", "gamma"])
def test_forces_nonlocal_complete_on_every_rank_and_stress_refused(lib, world, kind, layout):
    """dftk_mi_forces_nonlocal on a sharded block: the projections P' [psi | i g psi] are partial sums over the row slab
    and are all-reduced INSIDE the call (force_kernels.hip), so every rank returns the COMPLETE forces, accumulated onto
    its own prefill -- asserted against the same entry point on an unsharded block of the same data (1e-13 relative, the
    sharded-versus-unsharded bound of test_gpu_multirank) and bitwise equal across ranks (identical reduced
    projections, then identical arithmetic).  The row offset of g = G + k (``row0``) and, on the Gamma-real block, the
    half-format offset are what a wrong slab would break.

    dftk_mi_stress_kinetic_nonlocal has no sharded branch: stress_kernels.hip refuses a plane-wave sharded block with
    EINVAL before any work (the header says so).  Asserted here on every rank -- output untouched, no collective --
    next to the unsharded block accepting the very same arguments."""
    dims, nb = CUBES[1], 5
    rk = world.ranks(dims, kind, layout)
    cube, H = rk.cube, rk.H
    n_psp, rp, nproj, species, pos, col_start = _force_args(cube)
    assert col_start[-1] == H.P.shape[1]
    kcoord = cube.kcoord(kind) if kind == "complex" else np.zeros(3)
    if kind == "gamma":
        psi = gr.symmetric_columns(np.random.default_rng(8), cube.g, cube.mg, rk.n, nb)
    else:
        psi = np.linalg.qr(random_block(8, rk.n, nb))[0]
    w = np.ascontiguousarray(WEIGHTS[:nb] * 0.5)
    prefill = np.linspace(-1.0, 2.0, 3 * (len(col_start) - 1))
    B = np.asfortranarray(cube.obasis.model.recip_lattice, dtype=np.float64)
    sprefill = np.linspace(-3.0, 1.0, 12)

    def stress(kb, psi_d, ld):
        out = sprefill.copy()
        st = lib.dftk_mi_stress_kinetic_nonlocal(kb.h, B.ctypes.data, kcoord.ctypes.data, nb, psi_d.data_ptr(), ld,
                                                 w.ctypes.data, n_psp, rp.ctypes.data, nproj.ctypes.data, len(species),
                                                 species.ctypes.data, pos.ctypes.data, col_start.ctypes.data, out.ctypes.data)
        return st, out

    # the unsharded block of the same data
    nx, ny, nz = dims
    bs = Basis(lib, nx, ny, nz, cube.vol)
    kb = KBlock(lib, bs, H.kpoint.mapping, H.kinetic)
    kb.set_projectors(H.P, H.D)
    if kind == "gamma":
        check(lib.dftk_mi_kblock_set_gamma_real(kb.h, 1))
    pd = dev(np.ascontiguousarray(psi.T))
    ref = _forces(lib, kb, kcoord, pd, rk.n, w, col_start, prefill)
    assert np.abs(ref - prefill).max() > 1e-3                    # (something is being compared)
    st, s_ref = stress(kb, pd, rk.n)
    assert st == 0 and np.abs(s_ref - sprefill).max() > 1e-3

    before = list(rk.group.calls)

    def fn_stress(r, _comm):
        sl = slab_in(psi, rk.rows[r], rk.rows[r + 1])
        st, out = stress(rk.kbs[r], sl, rk.nloc(r))
        return st, out, lib.dftk_mi_last_error().decode(errors="replace")

    for st, out, msg in rk.group.run(fn_stress):
        assert st == EINVAL and "sharded" in msg and np.array_equal(out, sprefill)
    assert rk.group.calls == before

    def fn(r, _comm):
        sl = slab_in(psi, rk.rows[r], rk.rows[r + 1])
        torch.cuda.synchronize()
        return _forces(lib, rk.kbs[r], kcoord, sl, rk.nloc(r), w, col_start, prefill)

    got = rk.group.run(fn)
    for r in range(rk.p):
        assert relerr(got[r] - prefill, ref - prefill) < 1e-13, (r, relerr(got[r] - prefill, ref - prefill))
        assert np.array_equal(got[r], got[0]), r
    assert all(c > b for c, b in zip(rk.group.calls, before))


# ------------------------------------------------------------------------------------------ h. refusals
def test_refusals(lib, world):
    """Leading dimensions other than the local rows are refused before any collective and before any write; set_shard
    refuses bad row tables and late calls; set_gamma_real refuses more ranks than half rows; set_shard(kb, NULL, NULL)
    gives the unsharded block back."""
    dims, nb = CUBES[0], 3
    cube = world.cube(dims)
    nx, ny, nz = dims
    for kind in ("complex", "gamma"):
        rk = world.ranks(dims, kind, "p3-uneven")
        before = list(rk.group.calls)
        psi = random_block(1, rk.n, nb)
        w = np.ones(nb)

        def fn(r, _comm):
            kb, nloc = rk.kbs[r], rk.nloc(r)
            pad = dev(np.zeros((nb + 1, nloc + 2), dtype=complex))
            for ld in (nloc + 1, nloc - 1 if nloc > 1 else nloc + 2):
                out = OutSlab(nloc + 2, nb)
                assert lib.dftk_mi_apply_H_parts(kb.h, 7, nb, pad.data_ptr(), ld, out.ptr(), ld) == EINVAL
                assert lib.dftk_mi_apply_H_parts(kb.h, 7, nb, pad.data_ptr(), nloc, out.ptr(), ld) == EINVAL
                out.take(written=False)
                rho = torch.zeros((nz, ny, nx), dtype=torch.float64, device="cuda")
                assert lib.dftk_mi_density_accumulate(kb.h, nb, pad.data_ptr(), ld, w.ctypes.data, rho.data_ptr()) == EINVAL
                assert lib.dftk_mi_density_accumulate_real(kb.h, nb, pad.data_ptr(), ld, w.ctypes.data, rho.data_ptr()) == EINVAL
                assert not rho.cpu().numpy().view(np.uint64).any()
            if kind == "gamma":
                hl = rk.hloc(r)
                for ld in (hl + 1, hl - 1):
                    out = OutSlab(hl + 2, nb)
                    hp = dev(np.zeros((nb + 1, hl + 2), dtype=complex))
                    assert lib.dftk_mi_gamma_apply_H(kb.h, 7, nb, hp.data_ptr(), ld, out.ptr(), ld) == EINVAL
                    assert lib.dftk_mi_gamma_apply_H(kb.h, 7, nb, hp.data_ptr(), hl, out.ptr(), ld) == EINVAL
                    out.take(written=False)
            # a block with projectors / in Gamma-real mode is not re-sharded
            assert lib.dftk_mi_kblock_set_shard(kb.h, _comm, rk.rows.ctypes.data) == EINVAL
            return psi.shape

        rk.group.run(fn)
        assert rk.group.calls == before

    # set_shard on fresh blocks
    H = cube.H("gamma")
    n = H.n_G
    group = RankGroup(3)
    comm = group.comms()[1]
    bs = Basis(lib, nx, ny, nz, cube.vol)

    def fresh():
        return KBlock(lib, bs, H.kpoint.mapping, H.kinetic)

    def starts(*v):
        return np.array(v, dtype=np.int64)

    kb = fresh()
    for bad in (starts(1, 5, 9, n), starts(0, 5, 9, n - 1), starts(0, 5, 9, n + 1), starts(0, 5, 5, n), starts(0, 9, 5, n),
                starts(0, 0, 5, n), starts(0, 5, n, n)):
        assert lib.dftk_mi_kblock_set_shard(kb.h, comm, bad.ctypes.data) == EINVAL, bad
    assert lib.dftk_mi_kblock_set_shard(kb.h, comm, None) == EINVAL
    good = starts(0, 1, n - 7, n)
    check(lib.dftk_mi_kblock_set_shard(kb.h, comm, good.ctypes.data))                  # (and the good one is taken)
    kb = fresh()
    check(lib.dftk_mi_kblock_set_gamma_real(kb.h, 1))
    assert lib.dftk_mi_kblock_set_shard(kb.h, comm, good.ctypes.data) == EINVAL       # after set_gamma_real
    assert b"set_gamma_real" in lib.dftk_mi_last_error()
    kb = fresh()
    kb.set_projectors(H.P, H.D)
    assert lib.dftk_mi_kblock_set_shard(kb.h, comm, good.ctypes.data) == EINVAL       # after set_projectors
    assert b"set_projectors" in lib.dftk_mi_last_error()

    # more ranks than half rows: G = 0 and one pair, three ranks of one row each -> n_half = 2 < 3
    m = np.ascontiguousarray(H.kpoint.mapping, dtype=np.int64)
    tiny = np.array([m[cube.g[0]], m[cube.g[1]], m[cube.mg[1]]])
    order = np.argsort(tiny)
    kin = np.array([H.kinetic[cube.g[0]], H.kinetic[cube.g[1]], H.kinetic[cube.mg[1]]])
    kb = KBlock(lib, bs, tiny[order], kin[order])
    check(lib.dftk_mi_kblock_set_shard(kb.h, comm, starts(0, 1, 2, 3).ctypes.data))
    assert lib.dftk_mi_kblock_set_gamma_real(kb.h, 1) == EINVAL
    assert b"more ranks than half-sphere rows" in lib.dftk_mi_last_error()
    assert group.calls == [0, 0, 0]

    # un-shard: the block is the unsharded one again (projectors of the whole sphere bound after it)
    psi = random_block(2, n, nb)
    kb = fresh()
    check(lib.dftk_mi_kblock_set_shard(kb.h, comm, good.ctypes.data))
    kb.set_projectors(H.P[good[1]:good[2]], H.D)
    check(lib.dftk_mi_kblock_set_shard(kb.h, None, None))
    kb.set_projectors(H.P, H.D)
    kb.set_potential(cube.V)
    ref_kb = fresh()
    ref_kb.set_projectors(H.P, H.D)
    ref_kb.set_potential(cube.V)
    got, ref = np.ascontiguousarray(kb.apply(psi)), np.ascontiguousarray(ref_kb.apply(psi))
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)) and relerr(ref, H.mul(psi)) < RTOL
    assert group.calls == [0, 0, 0]
    group.close()


# ------------------------------------------------------------------------------------------ i. one rank
@pytest.mark.parametrize("kind", ["complex", "gamma"])
def test_one_rank_communicator_is_a_no_op(lib, world, kind):
    """set_shard with a one-rank host communicator takes the ``comm_size(comm) == 1`` branch: the block stays unsharded
    (padded leading dimensions are still accepted), results are bitwise those of a block that never saw a communicator,
    and the callbacks are never called."""
    dims, nb = CUBES[1], 5
    cube = world.cube(dims)
    H = cube.H(kind)
    n = H.n_G
    nx, ny, nz = dims
    group = RankGroup(1)
    psi = np.linalg.qr(random_block(9, n, nb))[0]
    X0 = np.linalg.qr(random_block(10, n, 3))[0]
    w = cube.weights(kind, WEIGHTS[:nb])
    ld = n + 5

    def run_all(comm):
        bs = Basis(lib, nx, ny, nz, cube.vol)
        kb = KBlock(lib, bs, H.kpoint.mapping, H.kinetic)
        if comm is not None:
            check(lib.dftk_mi_kblock_set_shard(kb.h, comm, np.array([0, n], dtype=np.int64).ctypes.data))
        kb.set_projectors(H.P, H.D)
        kb.set_potential(cube.V)
        if kind == "gamma":
            check(lib.dftk_mi_kblock_set_gamma_real(kb.h, 1))
        buf = torch.zeros((nb, ld), dtype=torch.complex128, device="cuda")
        buf[:, :n] = dev(np.ascontiguousarray(psi.T))
        out = torch.full((nb, ld), float("nan"), dtype=torch.complex128, device="cuda")
        rho = torch.zeros((nz, ny, nx), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        check(lib.dftk_mi_apply_H(kb.h, nb, buf.data_ptr(), ld, out.data_ptr(), ld))
        check(lib.dftk_mi_density_accumulate(kb.h, nb, buf.data_ptr(), ld, w.ctypes.data, rho.data_ptr()))
        bs.sync()
        Xd = dev(np.ascontiguousarray(X0.T))
        lam, res = np.zeros(3), np.zeros(3)
        n_iter, conv, nmv = C.c_int(), C.c_int(), C.c_int64()
        check(lib.dftk_mi_lobpcg(kb.h, 3, Xd.data_ptr(), n, 1e-8, 1, 200, 0, 1, 1234, lam.ctypes.data, res.ctypes.data,
                                 C.byref(n_iter), C.byref(conv), C.byref(nmv)))
        bs.sync()
        return out.cpu().numpy(), rho.cpu().numpy(), lam, res, Xd.cpu().numpy(), (n_iter.value, conv.value, nmv.value)

    got = group.run(lambda r, comm: run_all(comm))[0]
    ref = run_all(None)
    for a, b in zip(got[:5], ref[:5]):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
    assert got[5] == ref[5] and ref[5][1] == 1
    assert relerr(ref[0][:, :n].T, H.mul(psi)) < RTOL
    assert group.calls == [0]
    group.close()
