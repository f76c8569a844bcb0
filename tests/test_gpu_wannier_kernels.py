"""``dftk_mi_apply_symop``, ``dftk_mi_wannier_overlaps`` and ``dftk_mi_wannier_guess_columns`` at the C ABI (ctypes, device
memory from torch) against the extended-precision NumPy twin of tests/wannier_twin.py, on synthetic spheres as
tests/test_gpu_transfer_kernels.py builds them (the silicon cell scaled by 1.6: 271 .. 609 rows, two or three workgroups of
256 rows, the last one partial).

A. apply_symop: all 48 operations of the diamond group (origin at the bond centre: the 12 of D3d have tau = 0, 36 have
   tau != 0) at the Gamma point and at k = (-1/2, 1/4, 1/8), whose images leave [-1/2, 1/2)^3 (kshift != 0); Ecut 3 and 5; 1 / 3 / 65 bands (8 columns per thread:
   one partial group, eight full groups plus one); padded leading dimensions, NaN prefill.  Bound per entry, from the
   operation count: the phase argument x = (G + kshift).tau is a sum of three products, |dx| <= 3 eps sum_i |G_i tau_i|, so
   the phase is off by 2 pi |dx|; sincospi and the one complex product add 8 eps:  (8 + 6 pi sum_i |G_i tau_i|) eps |psi|.
   S then S^-1 returns the input bit for bit where tau = 0; two calls give equal bits; an operation that is not a symmetry
   of the sphere and the other bad arguments return DFTK_MI_EINVAL and leave the output as it was.
B. wannier_overlaps: Gamma and a generic k-point against 1 / 3 / 8 neighbours with shifts 0, (1, 0, 0), (1, 0, -1), one
   neighbour that shares no plane wave (the kernel result is zero; the identity is the Python layer's rule), neighbours on
   another basis handle (another stream), 1 / 3 / 33 bands.  Bound per entry n_G eps sum |a| |b|.  Equal bits from two
   calls; the launch count does not depend on the number of bands and there is no host synchronisation.
C. wannier_guess_columns on a triclinic cell: every (l, m) with l <= 3 and the Gaussian against the host callables, centres at
   the origin and outside the first cell, a k-point with a row at p = 0 (l > 0: an exact zero there, everything finite).
   The host callables are fp64 themselves, so both sides carry rounding.  Bound per entry: the radial sum has n_r terms,
   (n_r + 32 + 6 pi sum_i |p_i c_i|) eps sum_i |w_i j_l(q r_i)| |Y_lm|.  The Gaussian exp(-pi q^2 / 2) e^{-2 pi i p.c}: q_a =
   sum_i B_ai p_i is a sum of three products of rounded p_i = G_i + k_i, |dq_a| <= 4 eps sum_i |B_ai p_i|, which on a
   triclinic cell is not small against |q_a|; with A = sum_a |q_a| sum_i |B_ai p_i| >= q^2 the exponent is off by
   (pi / 2) (8 A + 4 q^2) eps on either side, the phase by 6 pi sum_i |p_i c_i| eps on either side, exp, sincospi and the
   product add 8 eps:  (8 + pi (8 A + 4 q^2) + 12 pi sum_i |p_i c_i|) eps |g|.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402
from dftk_jl_amd.symmetry import symmetry_operations  # noqa: E402
from dftk_jl_amd.wannier import (GaussianWannierProjection, HydrogenicWannierProjection, hydrogenic_radial_mesh,  # noqa: E402
                                 ylm_real)

import wannier_twin as twin  # noqa: E402
from test_gpu_kernels import Basis, KBlock, LATTICE, POSITIONS, dev, make_oracle_basis  # noqa: E402

EINVAL = -1
EPS = np.finfo(float).eps
SCALE = 1.6
FFT = (20, 20, 20)
K_SYM = [np.zeros(3), np.array([-0.5, 0.25, 0.125])]
NAN = complex(np.nan, np.nan)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def counts(lib):
    a, b = C.c_int64(), C.c_int64()
    check(lib.dftk_mi_launch_count(C.byref(a), C.byref(b)))
    return a.value, b.value


# =========================================================================================== A: apply_symop
OPS = symmetry_operations(SCALE * LATTICE, [[0, 1]], POSITIONS)
_SYM_SIDES = {}


def sym_side(lib, Ecut):
    """oracle basis over k and every image S k, one library basis, one k-block per k-point; built once per Ecut"""
    if Ecut not in _SYM_SIDES:
        kcoords = []

        def index_of(k):
            for i, q in enumerate(kcoords):
                if np.max(np.abs(q - k)) < 1e-12:
                    return i
            kcoords.append(np.array(k, dtype=float))
            return len(kcoords) - 1

        images = {}
        for ik, k in enumerate(K_SYM):
            index_of(k)
        for ik, k in enumerate(K_SYM):
            for io, op in enumerate(OPS):
                Sk, kshift = twin.symop_image(op.S, k)
                images[(ik, io)] = (index_of(Sk), kshift)
        ob = make_oracle_basis(Ecut, FFT, kcoords=[list(k) for k in kcoords], terms=("Kinetic",), lattice=SCALE * LATTICE)
        bs = Basis(lib, *FFT, ob.model.unit_cell_volume)
        kbs = [KBlock(lib, bs, kpt.mapping, 0.5 * np.sum(ob.Gplusk_vectors_cart(kpt) ** 2, axis=1)) for kpt in ob.kpoints]
        _SYM_SIDES[Ecut] = (ob, bs, kbs, images)
    return _SYM_SIDES[Ecut]


def call_symop(lib, kb_in, kb_out, S, kshift, tau, psi, ld_in, ld_out, fill=NAN, n_bands=None):
    """psi: (n_in, nb) host block -> (status, whole output buffer (nb, ld_out) on the host)"""
    n_in, nb = psi.shape
    buf = np.full((nb, max(ld_in, n_in)), NAN)          # (a short ld_in is only ever passed to a call that is refused)
    buf[:, :n_in] = psi.T
    pin = dev(buf)
    pout = dev(np.full((max(nb, 1), ld_out), fill))
    invS = np.ascontiguousarray(np.rint(np.linalg.inv(np.asarray(S, dtype=float))).astype(np.int32).ravel(order="F"))
    ks = np.ascontiguousarray(kshift, dtype=np.int32)
    tau_h = np.ascontiguousarray(tau, dtype=np.float64)
    torch.cuda.synchronize()
    st = lib.dftk_mi_apply_symop(kb_in.h, kb_out.h, invS.ctypes.data, ks.ctypes.data, tau_h.ctypes.data,
                                 nb if n_bands is None else n_bands, pin.data_ptr(), ld_in, pout.data_ptr(), ld_out)
    kb_in.basis.sync()
    kb_out.basis.sync()
    return st, pout.cpu().numpy()


def test_the_operations_cover_translations_and_shifts(lib):
    """What the parametrised test relies on: 48 operations, 36 of them with a fractional translation, and images of the
    generic k-point that needed a reduction back into [-1/2, 1/2)^3."""
    _, _, _, images = sym_side(lib, 3)
    assert len(OPS) == 48 and sum(1 for op in OPS if op.tau.any()) == 36
    assert sum(1 for (ik, io), (_, ks) in images.items() if ik == 1 and ks.any()) > 0
    assert sum(1 for (ik, io), (_, ks) in images.items() if ik == 1 and ks.any() and OPS[io].tau.any()) > 0


@pytest.mark.parametrize("n_bands", [1, 3, 65])
@pytest.mark.parametrize("Ecut", [3, 5])
def test_apply_symop_against_the_twin(lib, Ecut, n_bands):
    ob, _, kbs, images = sym_side(lib, Ecut)
    rng = np.random.default_rng(100 * Ecut + n_bands)
    worst = 0.0
    for ik in range(len(K_SYM)):
        kp = ob.kpoints[ik]
        n_in = len(kp.mapping)
        psi = crandn(rng, n_in, n_bands)
        for io, op in enumerate(OPS):
            iSk, kshift = images[(ik, io)]
            kq = ob.kpoints[iSk]
            n_out = len(kq.mapping)
            ref, arg = twin.apply_symop(op.S, op.tau, kshift, kp.mapping, kq.mapping, FFT, psi)
            st, got = call_symop(lib, kbs[ik], kbs[iSk], op.S, kshift, op.tau, psi, n_in + 7, n_out + 5)
            assert st == 0, lib.dftk_mi_last_error()
            assert np.isnan(got[:, n_out:]).all() and not np.isnan(got[:, :n_out]).any()
            ref64 = ref.astype(complex)
            bound = (8 + 6 * np.pi * arg)[:, None] * EPS * np.abs(ref64)
            err = np.abs(got[:, :n_out].T - ref64)
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            assert np.all(err <= bound), (Ecut, ik, io)
            if not op.tau.any():                      # the numbers are moved, not multiplied
                assert same_bits(got[:, :n_out].T, ref64)
            if io % 8 == 1:
                st2, again = call_symop(lib, kbs[ik], kbs[iSk], op.S, kshift, op.tau, psi, n_in + 7, n_out + 5)
                assert st2 == 0 and same_bits(again[:, :n_out], got[:, :n_out])
    print(f"\napply_symop Ecut {Ecut}, {n_bands} bands: worst error / bound = {worst:.3f}")


def test_apply_symop_there_and_back_bit_for_bit(lib):
    ob, _, kbs, images = sym_side(lib, 5)
    rng = np.random.default_rng(9)
    done = 0
    for ik in range(len(K_SYM)):
        kp = ob.kpoints[ik]
        psi = crandn(rng, len(kp.mapping), 3)
        for io, op in enumerate(OPS):
            if op.tau.any() or op.isone():
                continue
            inv = next(o for o in OPS if np.array_equal(o.W @ op.W, np.eye(3, dtype=int)) and not o.tau.any())
            iSk, kshift = images[(ik, io)]
            kq = ob.kpoints[iSk]
            st, there = call_symop(lib, kbs[ik], kbs[iSk], op.S, kshift, op.tau, psi, len(kp.mapping), len(kq.mapping))
            assert st == 0, lib.dftk_mi_last_error()
            back_k, back_shift = twin.symop_image(inv.S, kq.coordinate)
            assert np.max(np.abs(back_k - kp.coordinate)) < 1e-12
            st, back = call_symop(lib, kbs[iSk], kbs[ik], inv.S, back_shift, inv.tau, there.T.copy(), len(kq.mapping),
                                  len(kp.mapping))
            assert st == 0, lib.dftk_mi_last_error()
            assert same_bits(back.T, psi), (ik, io)
            done += 1
    assert done == 2 * 11


def test_apply_symop_bad_arguments(lib):
    ob, _, kbs, images = sym_side(lib, 3)
    io = next(i for i, op in enumerate(OPS) if op.tau.any() and images[(1, i)][1].any())
    op = OPS[io]
    iSk, kshift = images[(1, io)]
    n_in, n_out = len(ob.kpoints[1].mapping), len(ob.kpoints[iSk].mapping)
    psi = crandn(np.random.default_rng(5), n_in, 2)
    sentinel = 7.0 + 3.0j

    def status(S=op.S, ks=kshift, k_out=iSk, **kw):
        st, out = call_symop(lib, kbs[1], kbs[k_out], S, ks, op.tau, psi, kw.pop("ld_in", n_in), kw.pop("ld_out", n_out + 2),
                             fill=sentinel, **kw)
        assert st == 0 or np.all(out == sentinel)            # a refused call wrote nothing
        return st

    shear = np.array([[1, 1, 0], [0, 1, 0], [0, 0, 1]])
    assert status(S=shear) == EINVAL                                  # not a symmetry of the sphere
    assert status(S=2 * np.eye(3, dtype=int)) == EINVAL               # not even unimodular
    assert status(ks=kshift + np.array([1, 0, 0])) == EINVAL          # the wrong reduction: rows without a pre-image
    assert status(k_out=0) == EINVAL                                  # the sphere of another k-point
    assert status(n_bands=-1) == EINVAL
    assert status(ld_in=n_in - 1) == EINVAL
    assert status(ld_out=n_out - 1) == EINVAL
    assert lib.dftk_mi_apply_symop(None, kbs[0].h, None, None, None, 1, None, 1, None, 1) == EINVAL
    assert status() == 0
    # the check is remembered per (input block, S^-1, kshift) on the output block: a remembered triple lets no other through
    assert status(S=shear) == EINVAL and status(ks=kshift + np.array([1, 0, 0])) == EINVAL and status() == 0


# =========================================================================================== B: wannier_overlaps
FFT_W = (20, 18, 16)
K_W = [[0.0, 0.0, 0.0], [1 / 2, 1 / 3, 1 / 4], [0.3, -0.2, 0.1], [-0.4, 0.45, 0.05]]
# (k-point of the neighbour, G_shift, which basis handle): the third shares no plane wave (G + 40 is not on the cube)
NEIGHBOURS = [(1, (0, 0, 0), 0), (3, (1, 0, -1), 1), (2, (40, 0, 0), 0), (2, (1, 0, 0), 0), (0, (0, 0, 0), 1), (1, (1, 0, -1), 0),
              (3, (0, 0, 0), 1), (0, (1, 0, 0), 0)]
_W_SIDE = {}


def w_side(lib):
    if not _W_SIDE:
        ob = make_oracle_basis(5, FFT_W, kcoords=K_W, terms=("Kinetic",), lattice=SCALE * LATTICE)
        sides = []
        for _ in range(2):
            bs = Basis(lib, *FFT_W, ob.model.unit_cell_volume)
            sides.append((bs, [KBlock(lib, bs, kpt.mapping, np.zeros(len(kpt.mapping))) for kpt in ob.kpoints]))
        _W_SIDE["x"] = (ob, sides)
    return _W_SIDE["x"]


def call_overlaps(lib, sides, k, nb, psi_dev, neighbours, M_dev):
    n_nb = len(neighbours)
    handles = (C.c_void_p * n_nb)(*[sides[s][1][j].h.value for j, _, s in neighbours])
    ptrs = (C.c_void_p * n_nb)(*[psi_dev[(j, s)].data_ptr() for j, _, s in neighbours])
    lds = np.ascontiguousarray([psi_dev[(j, s)].shape[1] for j, _, s in neighbours], dtype=np.int64)
    dG = np.ascontiguousarray([g for _, g, _ in neighbours], dtype=np.int32).reshape(-1)
    return lib.dftk_mi_wannier_overlaps(sides[0][1][k].h, nb, psi_dev[(k, 0)].data_ptr(), psi_dev[(k, 0)].shape[1], n_nb,
                                        C.cast(handles, C.c_void_p), dG.ctypes.data, C.cast(ptrs, C.c_void_p), lds.ctypes.data,
                                        M_dev.data_ptr())


def overlap_blocks(ob, n_bands, seed):
    """host blocks (n_G, n_bands) per (k-point, side) and their padded, NaN-prefilled device copies (n_bands, ld)"""
    rng = np.random.default_rng(seed)
    host, device = {}, {}
    for s in range(2):
        for j, kpt in enumerate(ob.kpoints):
            n = len(kpt.mapping)
            host[(j, s)] = crandn(rng, n, n_bands)
            buf = np.full((n_bands, n + 3 + j), NAN)
            buf[:, :n] = host[(j, s)].T
            device[(j, s)] = dev(buf)
    return host, device


@pytest.mark.parametrize("n_bands", [1, 3, 33])
@pytest.mark.parametrize("n_nb", [1, 3, 8])
@pytest.mark.parametrize("k", [0, 1], ids=["gamma", "generic"])
def test_wannier_overlaps_against_the_twin(lib, k, n_nb, n_bands):
    ob, sides = w_side(lib)
    host, device = overlap_blocks(ob, n_bands, 7 * n_bands + n_nb + 100 * k)
    neighbours = NEIGHBOURS[:n_nb]
    M = dev(np.full((n_nb * n_bands, n_bands), NAN))
    torch.cuda.synchronize()
    check(call_overlaps(lib, sides, k, n_bands, device, neighbours, M))
    for bs, _ in sides:
        bs.sync()
    got = M.cpu().numpy().reshape(n_nb, n_bands, n_bands).transpose(0, 2, 1)          # [j, m, n]
    assert not np.isnan(got).any()
    n_G = len(ob.kpoints[k].mapping)
    worst = 0.0
    for j, (kj, shift, s) in enumerate(neighbours):
        ref, absM = twin.overlap_Mmn_k_kpb(host[(k, 0)], ob.kpoints[k].mapping, host[(kj, s)], ob.kpoints[kj].mapping, FFT_W, FFT_W,
                                           shift, n_bands, identity_if_zero=False)
        if shift == (40, 0, 0):
            assert not absM.any() and not got[j].any()                 # no plane wave shared: the kernel result is zero
        else:
            assert absM.all()
        err = np.abs(got[j] - ref.astype(complex))
        bound = n_G * EPS * absM
        assert np.all(err <= bound), (k, j)
        if absM.any():
            worst = max(worst, float(np.max(err / bound)))
    print(f"\nwannier_overlaps k {k}, {n_nb} neighbours, {n_bands} bands: worst error / bound = {worst:.4f}")
    M2 = dev(np.full((n_nb * n_bands, n_bands), NAN))
    check(call_overlaps(lib, sides, k, n_bands, device, neighbours, M2))
    for bs, _ in sides:
        bs.sync()
    assert same_bits(M2.cpu().numpy(), M.cpu().numpy())


def test_wannier_overlaps_launches_do_not_depend_on_the_bands(lib):
    ob, sides = w_side(lib)
    seen = {}
    for n_bands in (1, 3, 33):
        _, device = overlap_blocks(ob, n_bands, n_bands)
        M = dev(np.full((8 * n_bands, n_bands), NAN))
        torch.cuda.synchronize()
        check(call_overlaps(lib, sides, 1, n_bands, device, NEIGHBOURS, M))          # (tables of every block exist after this)
        for bs, _ in sides:
            bs.sync()
        l0, s0 = counts(lib)
        check(call_overlaps(lib, sides, 1, n_bands, device, NEIGHBOURS, M))
        l1, s1 = counts(lib)
        for bs, _ in sides:
            bs.sync()
        seen[n_bands] = l1 - l0
        assert s1 - s0 == 0                                           # no host synchronisation inside the entry
    print(f"\nwannier_overlaps launches per call with 8 neighbours: {seen}")
    assert len(set(seen.values())) == 1 and seen[1] >= 1


def test_wannier_overlaps_bad_arguments(lib):
    ob, sides = w_side(lib)
    _, device = overlap_blocks(ob, 2, 1)
    sentinel = 7.0 + 3.0j
    M = dev(np.full((3 * 2, 2), sentinel))
    torch.cuda.synchronize()
    nbs = NEIGHBOURS[:3]
    short = dict(device)
    short[(1, 0)] = device[(1, 0)][:, :len(ob.kpoints[1].mapping) - 1]
    assert call_overlaps(lib, sides, 0, -1, device, nbs, M) == EINVAL
    assert call_overlaps(lib, sides, 0, 2, short, nbs, M) == EINVAL                 # neighbour with a short leading dimension
    assert call_overlaps(lib, sides, 1, 2, short, nbs, M) == EINVAL                 # ... and the block itself
    assert lib.dftk_mi_wannier_overlaps(None, 1, None, 1, 0, None, None, None, None, None) == EINVAL
    assert lib.dftk_mi_wannier_overlaps(sides[0][1][0].h, 1, device[(0, 0)].data_ptr(), device[(0, 0)].shape[1], 2, None, None,
                                        None, None, M.data_ptr()) == EINVAL
    for bs, _ in sides:
        bs.sync()
    assert np.all(M.cpu().numpy() == sentinel)
    assert call_overlaps(lib, sides, 0, 2, device, nbs, M) == 0
    assert call_overlaps(lib, sides, 0, 2, device, [], M) == 0                      # no neighbours: nothing to do


# =========================================================================================== C: wannier_guess_columns
TRI = np.array([[9.0, 1.1, 0.6], [0.4, 10.0, 1.3], [0.8, 0.3, 11.0]])
K_TRI = [[0.0, 0.0, 0.0], [0.3, -0.2, 0.1]]
CENTRES = [np.zeros(3), np.array([1.3, -0.4, 2.2]), np.array([0.25, 0.5, 0.125])]


def tri_side(lib):
    if "tri" not in _W_SIDE:
        fft = dftk.basis.compute_fft_size(TRI, 4)
        ob = make_oracle_basis(4, fft, kcoords=K_TRI, terms=("Kinetic",), lattice=TRI)
        bs = Basis(lib, *fft, ob.model.unit_cell_volume)
        _W_SIDE["tri"] = (ob, fft, bs, [KBlock(lib, bs, kpt.mapping, np.zeros(len(kpt.mapping))) for kpt in ob.kpoints])
    return _W_SIDE["tri"]


def guess_projections():
    projs = [GaussianWannierProjection(c) for c in CENTRES]
    i = 0
    for l in range(4):
        for m in range(-l, l + 1):
            projs.append(HydrogenicWannierProjection(CENTRES[i % 3], 1 + i % 3, l, m, (1.1, 0.7)[i % 2]))
            i += 1
    return projs


def call_guess(lib, ob, bs, kb, ik, projs, normalize, ld_out, fill=NAN):
    kpt = ob.kpoints[ik]
    n_G = len(kpt.mapping)
    q = np.linalg.norm(ob.Gplusk_vectors_cart(kpt), axis=1)
    qd = dev(q)
    channels, kinds, lm, chans = {}, [], [], []
    for p in projs:
        if isinstance(p, GaussianWannierProjection):
            kinds.append(0); lm.append((0, 0)); chans.append(0)
        else:
            kinds.append(1); lm.append((p.l, p.m)); chans.append(channels.setdefault((p.n, p.l, p.alpha), len(channels)))
    R = torch.full((max(len(channels), 1), n_G + 4), float("nan"), dtype=torch.float64, device="cuda")
    for (n, l, alpha), c in channels.items():
        r, w = hydrogenic_radial_mesh(n, alpha)
        row = torch.empty(n_G, dtype=torch.float64, device="cuda")
        check(lib.dftk_mi_radial_transform(bs.h, 0, min(max(l, 0), 3), len(r), r.ctypes.data, w.ctypes.data, 0.0, n_G, qd.data_ptr(), row.data_ptr()))
        bs.sync()
        R[c, :n_G] = row
    out = dev(np.full((len(projs), ld_out), fill))
    Bh = np.asfortranarray(ob.model.recip_lattice, dtype=np.float64)
    kh = np.ascontiguousarray(kpt.coordinate, dtype=np.float64)
    arrs = [np.ascontiguousarray(kinds, dtype=np.int32), np.ascontiguousarray(lm, dtype=np.int32).reshape(-1),
            np.ascontiguousarray(chans, dtype=np.int32), np.ascontiguousarray([p.center for p in projs], dtype=np.float64).reshape(-1)]
    torch.cuda.synchronize()
    st = lib.dftk_mi_wannier_guess_columns(kb.h, Bh.ctypes.data, kh.ctypes.data, len(projs), arrs[0].ctypes.data,
                                           arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data, len(channels),
                                           R.data_ptr(), R.shape[1], normalize, out.data_ptr(), ld_out)
    bs.sync()
    return st, out.cpu().numpy()


def guess_reference(ob, ik, projs):
    """host callables and the per-entry bound of the docstring"""
    from scipy.special import spherical_jn
    kpt = ob.kpoints[ik]
    ps = twin.G_of_mapping(kpt.mapping, ob.fft_size).astype(float) + np.asarray(kpt.coordinate)
    p_cart = ps @ np.asarray(ob.model.recip_lattice).T
    q = np.linalg.norm(p_cart, axis=1)
    ref = np.array([p(ob, ps) for p in projs])
    bound = np.zeros(ref.shape)
    for i, p in enumerate(projs):
        if isinstance(p, GaussianWannierProjection):
            A = np.sum(np.abs(p_cart) * (np.abs(ps) @ np.abs(np.asarray(ob.model.recip_lattice)).T), axis=1)
            bound[i] = (8 + np.pi * (8 * A + 4 * q * q) + 12 * np.pi * np.abs(ps * p.center).sum(axis=1)) * EPS * np.abs(ref[i])
        else:
            r, w = hydrogenic_radial_mesh(p.n, p.alpha)
            mag = np.array([np.sum(np.abs(w * spherical_jn(p.l, x * r))) for x in q]) * np.abs(ylm_real(p.l, p.m, p_cart))
            bound[i] = (len(r) + 32 + 6 * np.pi * np.abs(ps * p.center).sum(axis=1)) * EPS * mag
    return ref, bound


@pytest.mark.parametrize("ik", [0, 1], ids=["gamma", "generic"])
def test_wannier_guess_columns_against_the_host_callables(lib, ik):
    ob, fft, bs, kbs = tri_side(lib)
    projs = guess_projections()
    assert len(projs) == 3 + 16
    n_G = len(ob.kpoints[ik].mapping)
    st, raw = call_guess(lib, ob, bs, kbs[ik], ik, projs, 0, n_G + 6)
    assert st == 0, lib.dftk_mi_last_error()
    assert np.isnan(raw[:, n_G:]).all() and np.isfinite(raw[:, :n_G]).all()
    ref, bound = guess_reference(ob, ik, projs)
    err = np.abs(raw[:, :n_G] - ref)
    ratio = err / np.maximum(bound, 1e-300)
    print(f"\nwannier_guess_columns k-point {ik}: worst error / bound = {ratio.max():.3f}, per column "
          + " ".join(f"{x:.2f}" for x in ratio.max(axis=1)))
    assert np.all(err <= bound)
    if ik == 0:                                                    # the row at p = 0 (G = 0 is the first row of the sphere)
        assert ob.kpoints[0].mapping[0] == 0
        for i, p in enumerate(projs):
            if isinstance(p, HydrogenicWannierProjection) and p.l > 0:
                assert raw[i, 0] == 0
            else:
                assert abs(raw[i, 0]) > 0
    # normalised columns: g / |g|, the norm perturbed by at most |bound| / |g|
    st, nrm = call_guess(lib, ob, bs, kbs[ik], ik, projs, 1, n_G + 6)
    assert st == 0 and np.isnan(nrm[:, n_G:]).all()
    norms = np.linalg.norm(ref, axis=1)
    slack = (bound + (np.linalg.norm(bound, axis=1) / norms + (n_G + 8) * EPS)[:, None] * np.abs(ref)) / norms[:, None]
    assert np.all(np.abs(nrm[:, :n_G] - ref / norms[:, None]) <= slack)
    assert np.max(np.abs(np.linalg.norm(nrm[:, :n_G], axis=1) - 1)) <= (n_G + 8) * EPS
    st, again = call_guess(lib, ob, bs, kbs[ik], ik, projs, 1, n_G + 6)
    assert st == 0 and same_bits(again[:, :n_G], nrm[:, :n_G])


def test_wannier_guess_columns_bad_arguments(lib):
    ob, fft, bs, kbs = tri_side(lib)
    n_G = len(ob.kpoints[1].mapping)
    sentinel = 7.0 + 3.0j
    good = [GaussianWannierProjection(CENTRES[1]), HydrogenicWannierProjection(CENTRES[0], 2, 1, 0, 1.0)]

    def status(projs=good, ld_out=n_G, patch=None):
        if patch is not None:
            projs = [HydrogenicWannierProjection(CENTRES[0], 2, 1, 0, 1.0)]
            projs[0].l, projs[0].m = patch
        st, out = call_guess(lib, ob, bs, kbs[1], 1, projs, 1, ld_out, fill=sentinel)
        assert st == 0 or np.all(out == sentinel)
        return st

    assert status(ld_out=n_G - 1) == EINVAL
    assert status(patch=(4, 0)) == EINVAL and status(patch=(1, 2)) == EINVAL and status(patch=(2, -3)) == EINVAL
    assert lib.dftk_mi_wannier_guess_columns(None, None, None, 1, None, None, None, None, 0, None, 0, 0, None, 0) == EINVAL
    assert status() == 0
