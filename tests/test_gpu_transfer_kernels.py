"""``dftk_mi_transfer_blochwave`` and ``dftk_mi_transfer_density`` at the C ABI (ctypes, device memory from torch) against
the NumPy twin of tests/refine_twin.py.

A. Orbital blocks, BIT FOR BIT (the entry only moves numbers): Ecut 3 -> 5, 5 -> 3 and 5 -> 5; the Gamma point, the generic
   point k = (1/2, 1/3, 1/4) onto itself and onto k + dG with dG = (1, 0, -1) and back; an input cube smaller than the output
   cube and the other way round, including a cube so tight that G + dG leaves it; spheres of two and three workgroups of
   rows; 1, 3 and 65 bands (TR_BANDS = 8 columns
   per thread: one partial group, and eight full groups plus one column); leading dimensions above the rows on both sides,
   the output prefilled with NaN (a row that is not written, or padding that is, shows); two calls give identical bits.
B. Densities to 1e-14 max|rho|: axes 8 -> 12, 9 -> 12, 12 -> 8, 12 -> 9, 15 -> 15, mixed per axis, one and two spin
   components; the integral is preserved small -> large to the same bound.
C. Bad arguments return DFTK_MI_EINVAL and leave the output as it was.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402

import refine_twin as twin  # noqa: E402
from test_gpu_kernels import Basis, KBlock, LATTICE, dev, make_oracle_basis  # noqa: E402

EINVAL = -1
K_GAMMA, K_GEN, K_SHIFTED = 0, 1, 2
KCOORDS = [[0.0, 0.0, 0.0], [1 / 2, 1 / 3, 1 / 4], [3 / 2, 1 / 3, -3 / 4]]        # the last is the second + (1, 0, -1)
# (k_in, k_out, dG = k_out - k_in)
K_CASES = [(K_GAMMA, K_GAMMA, (0, 0, 0)), (K_GEN, K_GEN, (0, 0, 0)), (K_GEN, K_SHIFTED, (1, 0, -1)),
           (K_SHIFTED, K_GEN, (-1, 0, 1))]
# (Ecut_in, cube_in, Ecut_out, cube_out) on a silicon cell scaled by 1.6, where the spheres have 271 .. 609 rows: two or
# three workgroups of TR_NT = 256 rows, the last one partial.  3 -> 5 into a larger cube, 5 -> 3 into a smaller one, 3 -> 5
# into a SMALLER cube, 5 -> 3 into a larger one, and 5 -> 5 out of and into a 12^3 cube that cuts the Ecut-5 sphere of the
# shifted k-point, so that G + dG of some output rows lies outside the input cube
LATTICE_SCALE = 1.6
BASIS_CASES = [(3, (16, 15, 18), 5, (20, 24, 18)), (5, (20, 24, 18), 3, (16, 15, 18)), (3, (20, 24, 18), 5, (15, 15, 15)),
               (5, (15, 15, 15), 3, (20, 24, 18)), (5, (12, 12, 12), 5, (20, 18, 16)), (5, (20, 18, 16), 5, (12, 12, 12))]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


_SIDES = {}


def side(lib, Ecut, fft_size):
    """oracle basis, library basis and one k-block (with its kinetic energies) per k-point of KCOORDS; built once"""
    key = (Ecut, fft_size)
    if key not in _SIDES:
        ob = make_oracle_basis(Ecut, fft_size, kcoords=KCOORDS, terms=("Kinetic",), lattice=LATTICE_SCALE * LATTICE)
        bs = Basis(lib, *fft_size, ob.model.unit_cell_volume)
        kbs = [KBlock(lib, bs, kpt.mapping, 0.5 * np.sum(ob.Gplusk_vectors_cart(kpt) ** 2, axis=1)) for kpt in ob.kpoints]
        _SIDES[key] = (ob, bs, kbs)
    return _SIDES[key]


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def call_transfer(lib, kb_in, kb_out, dG, psi, ld_in, ld_out, fill=complex(np.nan, np.nan), n_bands=None):
    """psi: (n_in, nb) host block -> (status, whole output buffer (nb, ld_out) on the host)"""
    n_in, nb = psi.shape
    buf = np.full((nb, ld_in), complex(np.nan, np.nan))
    buf[:, :n_in] = psi.T
    pin = dev(buf)
    pout = dev(np.full((max(nb, 1), ld_out), fill))
    dG_h = np.ascontiguousarray(dG, dtype=np.int32)
    torch.cuda.synchronize()
    st = lib.dftk_mi_transfer_blochwave(kb_in.h, kb_out.h, dG_h.ctypes.data, nb if n_bands is None else n_bands,
                                        pin.data_ptr(), ld_in, pout.data_ptr(), ld_out)
    kb_in.basis.sync()
    kb_out.basis.sync()
    return st, pout.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# =========================================================================================== A: orbital blocks
@pytest.mark.parametrize("n_bands", [1, 3, 65])
@pytest.mark.parametrize("case", BASIS_CASES, ids=lambda c: f"{c[0]}:{'x'.join(map(str, c[1]))}->{c[2]}:{'x'.join(map(str, c[3]))}")
def test_transfer_blochwave_bit_for_bit(lib, case, n_bands):
    Ecut_in, fft_in, Ecut_out, fft_out = case
    ob_in, _, kbs_in = side(lib, Ecut_in, fft_in)
    ob_out, _, kbs_out = side(lib, Ecut_out, fft_out)
    rng = np.random.default_rng(17 * n_bands + Ecut_in + 100 * fft_out[0])
    for k_in, k_out, dG in K_CASES:
        kp_in, kp_out = ob_in.kpoints[k_in], ob_out.kpoints[k_out]
        n_in, n_out = len(kp_in.mapping), len(kp_out.mapping)
        psi = crandn(rng, n_in, n_bands)
        ref = twin.transfer_blochwave_kpt(psi, kp_in.mapping, fft_in, kp_out.mapping, fft_out, dG)
        st, got = call_transfer(lib, kbs_in[k_in], kbs_out[k_out], dG, psi, n_in + 7, n_out + 5)
        assert st == 0, dftk.load_library().dftk_mi_last_error()
        assert same_bits(got[:, :n_out], ref.T), (case, k_in, k_out)
        assert np.isnan(got[:, n_out:]).all()                   # the padding rows are untouched
        st2, again = call_transfer(lib, kbs_in[k_in], kbs_out[k_out], dG, psi, n_in + 7, n_out + 5)
        assert st2 == 0 and same_bits(again[:, :n_out], got[:, :n_out])


def test_the_cases_cover_every_way_a_row_can_lack_a_partner(lib):
    """What the parametrised test relies on, checked on the twin's mappings: there are output rows without a partner because
    G + dG lies outside the input SPHERE, others because it lies outside the input CUBE, and input rows that are dropped."""
    outside_cube = outside_sphere = dropped = 0
    for Ecut_in, fft_in, Ecut_out, fft_out in BASIS_CASES:
        ob_in, ob_out = side(lib, Ecut_in, fft_in)[0], side(lib, Ecut_out, fft_out)[0]
        for k_in, k_out, dG in K_CASES:
            kp_in, kp_out = ob_in.kpoints[k_in], ob_out.kpoints[k_out]
            idcs_in, idcs_out = twin.transfer_mapping_kpt(kp_in.mapping, fft_in, kp_out.mapping, fft_out, dG)
            dropped += len(kp_in.mapping) - len(idcs_in)
            lonely = np.setdiff1d(np.arange(len(kp_out.mapping)), idcs_out)
            G = twin.G_of_mapping(kp_out.mapping, fft_out)[lonely] + np.asarray(dG)
            lo = [-((n - 1) - (n - 1) // 2) for n in fft_in]
            hi = [(n - 1) // 2 for n in fft_in]
            inside = np.all((G >= lo) & (G <= hi), axis=1)
            outside_cube += int(np.sum(~inside))
            outside_sphere += int(np.sum(inside))
    assert outside_cube > 0 and outside_sphere > 0 and dropped > 0


def test_transfer_blochwave_bad_arguments(lib):
    ob_in, _, kbs_in = side(lib, 3, (16, 15, 18))
    ob_out, _, kbs_out = side(lib, 5, (20, 24, 18))
    n_in, n_out = len(ob_in.kpoints[K_GEN].mapping), len(ob_out.kpoints[K_GEN].mapping)
    psi = crandn(np.random.default_rng(5), n_in, 2)
    sentinel = 7.0 + 3.0j
    n_shift = len(ob_out.kpoints[K_SHIFTED].mapping)
    pin = dev(psi.T.copy())                                          # (2, n_in)
    pout = dev(np.full((2, max(n_out, n_shift) + 2), sentinel))
    ld_o = pout.shape[1]
    torch.cuda.synchronize()

    def status(k_out=K_GEN, dG=(0, 0, 0), n_bands=2, ld_in=n_in, ld_out=ld_o):
        dG_h = np.ascontiguousarray(dG, dtype=np.int32)
        st = lib.dftk_mi_transfer_blochwave(kbs_in[K_GEN].h, kbs_out[k_out].h, dG_h.ctypes.data, n_bands, pin.data_ptr(), ld_in,
                                            pout.data_ptr(), ld_out)
        kbs_out[k_out].basis.sync()
        return st

    assert status(dG=(1, 0, 0)) == EINVAL                            # dG does not match the blocks (the same k-point)
    assert status(k_out=K_SHIFTED) == EINVAL                         # ... nor does 0 between k and k + (1, 0, -1)
    assert status(n_bands=-1) == EINVAL
    assert status(ld_in=n_in - 1) == EINVAL
    assert status(ld_out=n_out - 1) == EINVAL
    assert lib.dftk_mi_transfer_blochwave(None, kbs_out[K_GEN].h, None, 1, None, 1, None, 1) == EINVAL
    assert np.all(pout.cpu().numpy() == sentinel)                    # none of them wrote anything
    assert status() == 0 and status(k_out=K_SHIFTED, dG=(1, 0, -1)) == 0          # the same calls with fitting arguments
    # the check is remembered per (input block, dG) on the output block: a remembered pair does not let another dG through
    assert status(dG=(1, 0, 0)) == EINVAL and status(k_out=K_SHIFTED) == EINVAL
    assert status() == 0 and status(k_out=K_SHIFTED, dG=(1, 0, -1)) == 0


# =========================================================================================== B: densities
# 8 -> 12, 9 -> 12, 12 -> 8, 12 -> 9 and 15 -> 15, mixed per axis
DENSITY_CASES = [((8, 9, 15), (12, 12, 15)), ((12, 12, 15), (8, 9, 15)), ((8, 12, 9), (12, 9, 12)), ((9, 8, 12), (12, 12, 8)),
                 ((12, 15, 8), (9, 15, 12))]


def cube_side(lib, fft_size):
    key = ("cube", fft_size)
    if key not in _SIDES:
        bs = Basis(lib, *fft_size, 1.0)
        N = int(np.prod(fft_size))
        _SIDES[key] = (bs, KBlock(lib, bs, np.arange(N, dtype=np.int64), np.zeros(N)))
    return _SIDES[key]


@pytest.mark.parametrize("n_spin", [1, 2])
@pytest.mark.parametrize("fft_in,fft_out", DENSITY_CASES)
def test_transfer_density_against_the_twin(lib, fft_in, fft_out, n_spin):
    bs_in, kb_in = cube_side(lib, fft_in)
    bs_out, kb_out = cube_side(lib, fft_out)
    rng = np.random.default_rng(sum(fft_in) + 10 * n_spin)
    rho = rng.random((n_spin, fft_in[2], fft_in[1], fft_in[0]))
    ref = twin.transfer_density(rho, fft_in, fft_out)
    rin = dev(rho)
    rout = torch.full((n_spin, fft_out[2], fft_out[1], fft_out[0]), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    check(lib.dftk_mi_transfer_density(kb_in.h, kb_out.h, n_spin, rin.data_ptr(), rout.data_ptr()))
    bs_in.sync()
    bs_out.sync()
    got = rout.cpu().numpy()
    bound = 1e-14 * np.abs(rho).max()
    err = np.abs(got - ref).max()
    print(f"\ntransfer_density {fft_in} -> {fft_out}, n_spin {n_spin}: max err {err:.3e} (bound {bound:.1e})")
    assert err <= bound
    if all(i <= o for i, o in zip(fft_in, fft_out)):          # small -> large: the integral (the mean) is preserved
        for s in range(n_spin):
            assert abs(got[s].mean() - rho[s].mean()) <= bound
    check(lib.dftk_mi_transfer_density(kb_in.h, kb_out.h, n_spin, rin.data_ptr(), rout.data_ptr()))
    bs_in.sync()
    bs_out.sync()
    assert np.array_equal(rout.cpu().numpy(), got)


def test_transfer_density_bad_arguments(lib):
    bs_in, kb_in = cube_side(lib, (8, 9, 15))
    bs_out, kb_out = cube_side(lib, (12, 12, 15))
    _, _, kbs = side(lib, 3, (16, 15, 18))
    rin = dev(np.ones((1, 15, 9, 8)))
    rout = dev(np.full((1, 15, 12, 12), 7.0))
    torch.cuda.synchronize()
    assert lib.dftk_mi_transfer_density(kb_in.h, kb_out.h, 3, rin.data_ptr(), rout.data_ptr()) == EINVAL
    assert lib.dftk_mi_transfer_density(kb_in.h, kb_out.h, 0, rin.data_ptr(), rout.data_ptr()) == EINVAL
    assert lib.dftk_mi_transfer_density(kbs[0].h, kb_out.h, 1, rin.data_ptr(), rout.data_ptr()) == EINVAL   # not a full cube
    assert lib.dftk_mi_transfer_density(kb_in.h, kb_out.h, 1, None, rout.data_ptr()) == EINVAL
    bs_out.sync()
    assert np.all(rout.cpu().numpy() == 7.0)
