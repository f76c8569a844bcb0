"""``dftk_mi_exx_apply`` (csrc/exx_kernels.hip) at the C ABI against the NumPy twin of the reference's exchange operator
(tests/exx_twin.py: apply!(::ExchangeOperator) between the transforms of compress_exchange).

Shapes: a 12 x 15 x 18 grid on a triclinic cell (nx, ny, nz and the padded x pitch 16 all different; sphere of 445 rows) and
the 18^3 grid of the silicon cell at Ecut 5 (x pitch 24; 137 rows).  1, 3 and 9 orbitals -- 9 is two launch groups at the
default batch of 8 and nine at a batch of 1 -- times 1 and 5 columns, every leading dimension above n_G with NaN in the
padding, overwrite and accumulate.  Separately: a weight of zero in the middle of the list (that orbital is NaN: it must not
be read), the path that transforms the orbitals again for every group of columns (cache cap 0), one occupied plane wave
(closed form: Vx e_G = -w K(G - G0) / Omega e_G, zero where G - G0 leaves the sphere), every refusal of the entry point that
the ABI can reach (the guard against a call from inside the library's batched multi-k drivers cannot be reached through the ABI:
``dftk_mi_batch_replay`` takes enumerated operations only, and the header says so), and the balance of
the live device buffers over the life of a basis.

Bound: RTOL = 1e-12 of test_gpu_kernels.py relative to max |W_ref| (the suite's bound for chained FFT identities), valid
because the complex128 twin stays within a tenth of it of the same twin in long double: measured 3.8e-16 .. 1.1e-15 on these
shapes (tests/test_exx_host.py asserts it without a GPU).  ``bound`` falls back to ten times the twin's
own error should that ever not hold."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import ALLREDUCE_FN, check  # noqa: E402

import exx_twin as twin  # noqa: E402
from test_gpu_kernels import RTOL, Basis, KBlock  # noqa: E402

EINVAL = -1
GRIDS = twin.KERNEL_TEST_GRIDS
oracle_basis = twin.kernel_test_basis
case = twin.kernel_test_case
assert RTOL == twin.RTOL_FFT
PAD = 7


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


def bound(twin_error):
    return RTOL if twin_error <= RTOL / 10 else 10 * twin_error


def padded(a, fill=complex(np.nan, np.nan)):
    """(rows x cols) as a band-major device buffer with ld = rows + PAD, `fill` in the padding"""
    h = np.full((a.shape[1], a.shape[0] + PAD), fill)
    h[:, :a.shape[0]] = a.T
    return h, torch.from_numpy(h.copy()).cuda()


def padding_kept(h, t, rows):
    after = np.ascontiguousarray(t.cpu().numpy()).view(np.uint64).reshape(h.shape + (2,))
    return np.array_equal(after[:, rows:], h.view(np.uint64).reshape(h.shape + (2,))[:, rows:])


def device_block(lib, grid):
    ob = oracle_basis(grid)
    nx, ny, nz = ob.fft_size
    bs = Basis(lib, nx, ny, nz, ob.model.unit_cell_volume)
    kb = KBlock(lib, bs, ob.kpoints[0].mapping, np.zeros(len(ob.kpoints[0].mapping)))
    return ob, bs, kb


def exx_apply(lib, bs, kb, phi, w, K, psi, W0, accumulate):
    """one call with padded blocks -> (W as n_G x n_bands, the padding of every block is what it was)"""
    n = kb.n_G
    (ph, pd), (sh, sd), (wh, wd) = padded(phi), padded(psi), padded(W0)
    Kd = torch.from_numpy(np.ascontiguousarray(K)).cuda()
    wts = np.ascontiguousarray(w, dtype=np.float64)
    torch.cuda.synchronize()
    check(lib.dftk_mi_exx_apply(kb.h, phi.shape[1], pd.data_ptr(), n + PAD, wts.ctypes.data, Kd.data_ptr(), psi.shape[1],
                                sd.data_ptr(), n + PAD, wd.data_ptr(), n + PAD, accumulate))
    bs.sync()
    kept = padding_kept(wh, wd, n) and np.array_equal(np.nan_to_num(pd.cpu().numpy()), np.nan_to_num(ph)) and \
        np.array_equal(np.nan_to_num(sd.cpu().numpy()), np.nan_to_num(sh))
    return wd.cpu().numpy()[:, :n].T, kept


def relmax(got, ref):
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def test_shapes_of_the_grids():
    """the shapes are what the module docstring says: a pitch that differs from nx, spheres that fit their grids"""
    for grid, n_G in (("triclinic_12x15x18", 445), ("cubic_18", 137)):
        ob = oracle_basis(grid)
        G = ob.kpoints[0].G_vectors
        assert len(G) == n_G
        for axis, n in enumerate(ob.fft_size):
            assert np.abs(G[:, axis]).max() <= (n - 1) // 2          # no Nyquist row: the sphere is not cut by the grid
        assert ob.fft_size[0] % 8 != 0


@pytest.mark.parametrize("batch", [8, 1])
@pytest.mark.parametrize("n_bands", [1, 5])
@pytest.mark.parametrize("n_occ", [1, 3, 9])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_exx_apply_against_the_twin(lib, grid, n_occ, n_bands, batch):
    phi, w, K, psi, W0, ref, own = case(grid, n_occ, n_bands)
    ob, bs, kb = device_block(lib, grid)
    check(lib.dftk_mi_basis_set_fft_batch(bs.h, batch))
    got, kept = exx_apply(lib, bs, kb, phi, w, K, psi, np.full_like(W0, complex(np.nan, np.nan)), 0)
    err0 = relmax(got, ref)
    got1, kept1 = exx_apply(lib, bs, kb, phi, w, K, psi, W0, 1)
    err1 = relmax(got1, W0 + ref)
    print(f"\nexx_apply {grid} n_occ {n_occ} n_bands {n_bands} batch {batch}: overwrite {err0:.2e}, accumulate {err1:.2e}, "
          f"twin vs long double {own:.2e}")
    assert kept and kept1
    assert err0 <= bound(own) and err1 <= bound(own)


@pytest.mark.parametrize("cache_bytes", [None, "0"])
def test_zero_weight_in_the_middle_and_the_retransforming_path(lib, monkeypatch, cache_bytes):
    """weights (w0 .. w3, 0, w5 .. w8): orbital 4 is skipped -- it is NaN here, so reading it would show -- and the eight
    others are one launch group.  With the cache cap at 0 bytes the orbitals' cubes are transformed again for each of the
    two groups of columns (batch 3: columns 3 + 2, orbitals 3 + 3 + 2)."""
    grid = "triclinic_12x15x18"
    phi, w, K, psi, W0, _, own = case(grid, 9, 5)
    w = w.copy()
    w[4] = 0.0
    ob, bs, kb = device_block(lib, grid)
    ref = twin.exchange_apply(ob, ob.kpoints[0], K, phi, w, psi)
    phi = phi.copy()
    phi[:, 4] = complex(np.nan, np.nan)
    if cache_bytes is not None:
        monkeypatch.setenv("DFTK_MI_EXX_PHI_BYTES", cache_bytes)
        check(lib.dftk_mi_basis_set_fft_batch(bs.h, 3))
    got, kept = exx_apply(lib, bs, kb, phi, w, K, psi, W0, 1)
    err = relmax(got, W0 + ref)
    print(f"\nexx_apply zero weight, cache cap {cache_bytes}: {err:.2e}")
    assert kept and err <= bound(own)


def test_one_occupied_plane_wave(lib):
    """phi = e_G0 with weight w: Vx e_G = -w K(G - G0) / Omega e_G, and zero where G - G0 is not on the sphere.  No transform
    on the reference side: this pins the normalisation and the sphere convention."""
    grid = "cubic_18"
    ob, bs, kb = device_block(lib, grid)
    kpt = ob.kpoints[0]
    n = len(kpt.mapping)
    row = {tuple(g): i for i, g in enumerate(kpt.G_vectors)}
    i0 = n // 2
    K = twin.kernel_coulomb_probe_charge(ob)
    w = 0.7
    phi = np.zeros((n, 1), dtype=complex)
    phi[i0] = 1.0
    cols = [0, i0, 5, n // 3, n - 1]                # G = 0, G0 itself, near and far rows
    psi = np.zeros((n, len(cols)), dtype=complex)
    ref = np.zeros_like(psi)
    inside = 0
    for c, i in enumerate(cols):
        psi[i, c] = 1.0
        j = row.get(tuple(kpt.G_vectors[i] - kpt.G_vectors[i0]))
        if j is not None:
            ref[i, c] = -w * K[j] / ob.model.unit_cell_volume
            inside += 1
    assert 0 < inside < len(cols)                 # both branches of the closed form occur
    got, _ = exx_apply(lib, bs, kb, phi, np.array([w]), K, psi, np.zeros_like(psi), 0)
    err = relmax(got, ref)
    print(f"\nexx_apply plane wave: {err:.2e}")
    assert err <= RTOL


def test_nothing_to_do(lib):
    """n_bands = 0 returns 0 and touches nothing; n_occ = 0 and all-zero weights zero-fill W (accumulate = 0) or leave it
    (accumulate = 1), padding kept"""
    grid = "cubic_18"
    phi, w, K, psi, W0, _, _ = case(grid, 3, 5)
    ob, bs, kb = device_block(lib, grid)
    n = kb.n_G
    Kd = torch.from_numpy(K).cuda()
    (ph, pd), (sh, sd) = padded(phi), padded(psi)
    for n_occ, wts in ((0, w), (3, np.zeros(3))):
        for accumulate in (0, 1):
            wh, wd = padded(W0)
            check(lib.dftk_mi_exx_apply(kb.h, n_occ, pd.data_ptr(), n + PAD, wts.ctypes.data, Kd.data_ptr(), 5, sd.data_ptr(),
                                        n + PAD, wd.data_ptr(), n + PAD, accumulate))
            bs.sync()
            assert padding_kept(wh, wd, n)
            assert np.array_equal(wd.cpu().numpy()[:, :n].T, W0 if accumulate else np.zeros_like(W0))
    wh, wd = padded(W0)
    check(lib.dftk_mi_exx_apply(kb.h, 3, pd.data_ptr(), n + PAD, w.ctypes.data, Kd.data_ptr(), 0, None, 0, None, 0, 0))
    check(lib.dftk_mi_exx_apply(kb.h, 0, None, 0, None, None, 0, None, 0, None, 0, 0))
    bs.sync()
    assert np.array_equal(np.nan_to_num(wd.cpu().numpy()), np.nan_to_num(wh))


def test_refusals(lib):
    """null pointers, leading dimensions below n_G, negative counts, a Gamma-real block and a plane-wave sharded block return
    DFTK_MI_EINVAL with a message and write nothing"""
    grid = "cubic_18"
    phi, w, K, psi, W0, _, _ = case(grid, 3, 5)
    ob, bs, kb = device_block(lib, grid)
    n = kb.n_G
    Kd = torch.from_numpy(K).cuda()
    (_, pd), (_, sd), (wh, wd) = padded(phi), padded(psi), padded(W0)
    good = dict(kb=kb.h, n_occ=3, phi=pd.data_ptr(), ld_phi=n + PAD, w=w.ctypes.data, K=Kd.data_ptr(), n_bands=5,
                psi=sd.data_ptr(), ld_psi=n + PAD, W=wd.data_ptr(), ld_W=n + PAD)

    def refused(word, **change):
        a = dict(good, **change)
        st = lib.dftk_mi_exx_apply(a["kb"], a["n_occ"], a["phi"], a["ld_phi"], a["w"], a["K"], a["n_bands"], a["psi"],
                                   a["ld_psi"], a["W"], a["ld_W"], 0)
        assert st == EINVAL, change
        assert word in lib.dftk_mi_last_error().decode(), (change, lib.dftk_mi_last_error())

    refused("null", kb=None)
    for name in ("phi", "w", "K", "psi", "W"):
        refused("null pointer", **{name: None})
    for name in ("ld_phi", "ld_psi", "ld_W"):
        refused("leading dimension", **{name: n - 1})
    refused("negative", n_occ=-1)
    refused("negative", n_bands=-1)
    check(lib.dftk_mi_kblock_set_gamma_real(kb.h, 1))
    refused("Gamma-real")
    check(lib.dftk_mi_kblock_set_gamma_real(kb.h, 0))
    # a block sharded over two ranks (the communicator is never used: the call is refused before any work)
    kb2 = KBlock(lib, bs, ob.kpoints[0].mapping, np.zeros(n))
    cb = ALLREDUCE_FN(lambda user, data, count: 0)
    comm = C.c_void_p()
    check(lib.dftk_mi_comm_create_host(2, 0, 0, cb, None, None, C.byref(comm)))
    rows = np.array([0, n // 2, n], dtype=np.int64)
    check(lib.dftk_mi_kblock_set_shard(kb2.h, comm, rows.ctypes.data))
    refused("sharded", kb=kb2.h)
    check(lib.dftk_mi_kblock_set_shard(kb2.h, None, None))
    check(lib.dftk_mi_comm_destroy(comm))
    bs.sync()
    assert np.array_equal(np.nan_to_num(wd.cpu().numpy()), np.nan_to_num(wh))       # no refused call wrote anything
    # ... and the block still works
    got, _ = exx_apply(lib, bs, kb, phi, w, K, psi, W0, 0)
    assert relmax(got, case(grid, 3, 5)[5]) <= RTOL


def live(lib):
    count, nbytes = C.c_int64(), C.c_int64()
    check(lib.dftk_mi_device_buffers_live(C.byref(count), C.byref(nbytes)))
    return count.value, nbytes.value


def test_workspace_goes_with_the_basis(lib):
    """dftk_mi_device_buffers_live before a basis is created and after it is destroyed agree; in between the exchange
    workspace shows: (c + 2 g_psi + g_phi) N + (2 g_phi + g_psi) n_G complex numbers with c = n_occ = 9, g = 8, g_psi = 5"""
    grid = "cubic_18"
    phi, w, K, psi, W0, ref, own = case(grid, 9, 5)
    gc.collect()
    before = live(lib)
    ob, bs, kb = device_block(lib, grid)
    created = live(lib)
    got, _ = exx_apply(lib, bs, kb, phi, w, K, psi, W0, 0)
    assert relmax(got, ref) <= bound(own)
    used = live(lib)
    N, n = 18 ** 3, kb.n_G
    assert used[1] - created[1] >= 16 * ((9 + 2 * 5 + 8) * N + (2 * 8 + 5) * n)
    check(lib.dftk_mi_kblock_destroy(kb.h))
    kb.h = C.c_void_p()
    check(lib.dftk_mi_basis_destroy(bs.h))
    bs.h = C.c_void_p()
    assert live(lib) == before
