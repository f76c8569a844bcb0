"""Handles release everything they own (csrc/devbuf.h): one create / use / destroy cycle at the C ABI that touches every
lazily allocated buffer of a basis, its k-blocks, the Gamma-real state and an Anderson accelerator, watched through the
library's own counters of live device allocations (``dftk_mi_device_buffers_live``) -- the device-wide free memory of a
shared machine says nothing.  After a warm-up cycle (the staging pool of the batched k-point driver is kept for the life of
the process) every further cycle returns count and bytes to the warm-up's reading, peaks at the same number of bytes, and
computes the same numbers: a handle is independent of its predecessors.  No allocation failure is provoked here; the failure
paths of the owner are driven on the host by tools/host_devbuf_check.cpp."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check, cplx  # noqa: E402

from test_gpu_kernels import Basis, dev  # noqa: E402

N = 12              # cube edge; the sphere |G|^2 <= 14 has 251 rows and no Nyquist component: it is inversion symmetric
S2 = np.sqrt(2.0)


def sphere():
    ax = np.array([i if i < N // 2 else i - N for i in range(N)])
    gz, gy, gx = np.meshgrid(ax, ax, ax, indexing="ij")
    g2 = (gx * gx + gy * gy + gz * gz).reshape(-1)
    mapping = np.nonzero(g2 <= 14)[0].astype(np.int64)
    ix, iy, iz = mapping % N, (mapping // N) % N, mapping // (N * N)
    minus = (-ix) % N + N * ((-iy) % N + N * ((-iz) % N))
    row = {int(v): i for i, v in enumerate(mapping)}
    partner = np.array([row[int(v)] for v in minus])
    g = np.nonzero(partner >= np.arange(len(mapping)))[0]            # one representative per {G, -G}, G = 0 first
    return mapping, 0.5 * g2[mapping].astype(np.float64), g, partner[g]


def real_symmetric(rng, n, m, g, mg):
    """m columns with x(-G) = conj x(G) on the full sphere, and their half format"""
    h = rng.standard_normal((len(g), m)) + 1j * rng.standard_normal((len(g), m))
    h[0] = h[0].real
    x = np.zeros((n, m), dtype=complex)
    x[g] = h / S2
    x[mg] = np.conj(h) / S2
    x[g[0]] = h[0].real
    return x, h


def live(lib):
    count, nbytes = C.c_int64(), C.c_int64()
    check(lib.dftk_mi_device_buffers_live(C.byref(count), C.byref(nbytes)))
    return count.value, nbytes.value


def cycle(lib):
    """-> (readings of the live counters after every step, the numbers the cycle computed)"""
    rng = np.random.default_rng(7)
    mapping, kin, g, mg = sphere()
    n, nh = len(mapping), len(g)
    assert 240 <= n <= 260 and nh == (n + 1) // 2
    seen, out = [], {}

    def step():
        seen.append(live(lib))

    bs = Basis(lib, N, N, N, 100.0)
    kbs = [C.c_void_p(), C.c_void_p()]
    for h in kbs:
        check(lib.dftk_mi_kblock_create(bs.h, n, mapping.ctypes.data, kin.ctypes.data, C.byref(h)))
    cube = C.c_void_p()
    full = np.arange(N ** 3, dtype=np.int64)
    check(lib.dftk_mi_kblock_create(bs.h, len(full), full.ctypes.data, None, C.byref(cube)))
    ka, kb = kbs
    step()
    # the padded potential: shared by both blocks, then block a gets its own again
    V = dev(rng.standard_normal((N, N, N)))
    arr = (C.c_void_p * 2)(ka, kb)
    check(lib.dftk_mi_kblocks_set_potential(2, arr, V.data_ptr()))
    step()
    check(lib.dftk_mi_kblock_set_potential(ka, V.data_ptr()))
    step()
    # projectors: 4 real-symmetric columns, then 2
    P4, _ = real_symmetric(rng, n, 4, g, mg)
    D4 = np.asfortranarray(np.diag([1.0, -0.5, 0.7, 0.3]) + 0.2 * (np.eye(4, k=1) + np.eye(4, k=-1)))
    Pd4, Pd2 = dev(P4.T.copy()), dev(P4[:, :2].T.copy())
    D2 = np.asfortranarray(D4[:2, :2])
    check(lib.dftk_mi_kblock_set_projectors(ka, 4, Pd4.data_ptr(), n, D4.ctypes.data))
    check(lib.dftk_mi_kblock_set_projectors(ka, 2, Pd2.data_ptr(), n, D2.ctypes.data))
    check(lib.dftk_mi_kblock_set_projectors(kb, 4, Pd4.data_ptr(), n, D4.ctypes.data))
    step()
    # H psi and the density of 3 bands
    X, Xh = real_symmetric(rng, n, 3, g, mg)
    Xd = dev(X.T.copy())
    Hd = torch.full_like(Xd, float("nan"))
    check(lib.dftk_mi_apply_H(ka, 3, Xd.data_ptr(), n, Hd.data_ptr(), n))
    w = np.array([2.0, 1.0, 0.5])
    rho = torch.zeros((N, N, N), dtype=torch.float64, device="cuda")
    check(lib.dftk_mi_density_accumulate(ka, 3, Xd.data_ptr(), n, w.ctypes.data, rho.data_ptr()))
    bs.sync()
    out["Hpsi"], out["rho"] = Hd.cpu().numpy(), rho.cpu().numpy()
    step()
    # LOBPCG twice, the second call behind the promise that its start is the block the first returned
    Ld = dev(np.linalg.qr(X)[0].T.copy())
    lam, res = np.zeros(3), np.zeros(3)
    n_iter, conv, nmv = C.c_int(), C.c_int(), C.c_int64()
    for second in (False, True):
        if second:
            check(lib.dftk_mi_kblock_reuse_AX(ka, 1))
        check(lib.dftk_mi_lobpcg(ka, 3, Ld.data_ptr(), n, 1e-8, 1, 60, 0, 1, 1234, lam.ctypes.data, res.ctypes.data,
                                 C.byref(n_iter), C.byref(conv), C.byref(nmv)))
        out["lambda%d" % second] = lam.copy()
        step()
    # real-symmetric Gamma orbitals: half-format H psi and the paired density pass
    check(lib.dftk_mi_kblock_set_gamma_real(kb, 1))
    hd = dev(Xh.T.copy())
    Gd = torch.full_like(hd, float("nan"))
    check(lib.dftk_mi_gamma_apply_H(kb, 7, 3, hd.data_ptr(), nh, Gd.data_ptr(), nh))
    rho_r = torch.zeros_like(rho)
    check(lib.dftk_mi_density_accumulate_real(kb, 3, Xd.data_ptr(), n, w.ctypes.data, rho_r.data_ptr()))
    bs.sync()
    out["Hpsi_half"], out["rho_real"] = Gd.cpu().numpy(), rho_r.cpu().numpy()
    step()
    forces = np.zeros(3)
    col_start = np.array([0, 4], dtype=np.int32)
    k0 = np.zeros(3)
    check(lib.dftk_mi_forces_nonlocal(kb, k0.ctypes.data, 3, Xd.data_ptr(), n, w.ctypes.data, 1, col_start.ctypes.data,
                                      forces.ctypes.data))
    out["forces"] = forces.copy()
    step()
    S = np.ascontiguousarray(np.stack([np.eye(3).ravel(), -np.eye(3).ravel()]), dtype=np.int32)
    tau = np.zeros((2, 3))
    rho_s = torch.empty_like(rho)
    check(lib.dftk_mi_symmetrize_rho(cube, 2, S.ctypes.data, tau.ctypes.data, 1, rho.data_ptr(), rho_s.data_ptr()))
    bs.sync()
    out["rho_sym"] = rho_s.cpu().numpy()
    step()
    # dense algebra workspaces: Cholesky + inverse at n = 48, eigensolver at n = 40, a split-K product
    A = rng.standard_normal((48, 48)) + 1j * rng.standard_normal((48, 48))
    Ad = dev((A @ A.conj().T + 48 * np.eye(48)).T.copy())
    Rd = torch.zeros_like(Ad)
    check(lib.dftk_mi_potrf_trtri(bs.h, 48, Ad.data_ptr(), 48, Rd.data_ptr(), 48))
    B = rng.standard_normal((40, 40)) + 1j * rng.standard_normal((40, 40))
    Bd = dev((B + B.conj().T).T.copy())
    Vd = torch.zeros_like(Bd)
    W = np.zeros(40)
    check(lib.dftk_mi_heev(bs.h, 40, Bd.data_ptr(), 40, W.ctypes.data, Vd.data_ptr(), 40))
    out["W"] = W.copy()
    Ga = dev(rng.standard_normal((16, 4096)) + 1j * rng.standard_normal((16, 4096)))     # column-major 4096 x 16
    Gc = torch.zeros((16, 16), dtype=torch.complex128, device="cuda")
    check(lib.dftk_mi_zgemm(bs.h, b"C", 16, 16, 4096, cplx(1.0), Ga.data_ptr(), 4096, Ga.data_ptr(), 4096, cplx(0.0),
                            Gc.data_ptr(), 16))
    bs.sync()
    out["invR"], out["gram"] = Rd.cpu().numpy(), Gc.cpu().numpy()
    step()
    acc = C.c_void_p()
    check(lib.dftk_mi_anderson_create(bs.h, N ** 3, 3, 1e6, 1e5, C.byref(acc)))
    x_next = torch.empty_like(rho)
    check(lib.dftk_mi_anderson_step(acc, rho.data_ptr(), 0.5, rho_s.data_ptr(), x_next.data_ptr(), None))
    bs.sync()
    out["anderson"] = x_next.cpu().numpy()
    step()
    check(lib.dftk_mi_anderson_destroy(acc))
    # one k-block (and the cube block) goes before the basis, the other after it
    check(lib.dftk_mi_kblock_destroy(ka))
    check(lib.dftk_mi_kblock_destroy(cube))
    step()
    check(lib.dftk_mi_basis_destroy(bs.h))
    bs.h = C.c_void_p()
    step()
    check(lib.dftk_mi_kblock_destroy(kb))
    return seen, out


def test_handles_release_what_they_own_and_do_not_depend_on_their_predecessors():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    lib = dftk.load_library()
    gc.collect()                                 # (handles that earlier tests dropped go now, not in the middle of a cycle)
    cycle(lib)                                   # warm-up: whatever is kept for the life of the process exists now
    gc.collect()
    base = live(lib)
    runs = []
    for _ in range(2):
        seen, out = cycle(lib)
        assert live(lib) == base, (live(lib), base)
        runs.append((seen, out))
    for seen, _ in runs:
        assert all(c > base[0] and b > base[1] for c, b in seen), (base, seen)
        assert max(b for _, b in seen) > seen[0][1]              # the lazily allocated buffers show
    assert max(b for _, b in runs[0][0]) == max(b for _, b in runs[1][0])
    assert runs[0][0] == runs[1][0]                              # every reading, not only the peak
    for name, a in runs[0][1].items():
        assert np.all(np.isfinite(a)), name
        assert np.array_equal(a, runs[1][1][name]), name
