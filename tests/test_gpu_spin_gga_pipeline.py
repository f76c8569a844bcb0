"""``dftk_mi_local_potential_collinear_gga``: the collinear-spin PBE branch of ``energy_hamiltonian`` in one library call,
on a 12 x 10 x 9 cube with a triclinic reciprocal lattice (an axis mix-up in G or in the lattice cannot cancel there).

The reference is a twin written here: ``numpy.fft`` gradients and divergence around the point-wise restatement of
tests/test_xc_spin_gga_reference.py.  The twin runs in float64 and, with dense DFT matrices, in long double; the difference
of the two on the same data is e_np, and the device is held to 64 x max(e_np, 2.2e-16) relative in the 2-norm (the rule of
DESIGN.md section 3.1.1; the chain is 17 cube FFTs).  The densities are smooth and positive, rho_up != rho_down, and rho_down
dips below the density threshold 1e-12 in one region.
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check as abi_check  # noqa: E402

import test_xc_spin_gga_reference as S  # noqa: E402
from test_gpu_kernels import Basis, KBlock, dev  # noqa: E402

NX, NY, NZ = 12, 10, 9
N = NX * NY * NZ
VOL = 37.5
DVOL = VOL / N
THRESHOLD = 1e-12
EPS = 2.2e-16
FACTOR = 64
NAN = float("nan")
LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")
# reciprocal lattice (columns = reciprocal vectors), triclinic: no two axes alike, every off-diagonal entry non-zero
RECIP = np.array([[1.10, 0.21, -0.13], [0.17, 0.93, 0.29], [-0.08, 0.12, 1.31]])
PBE = ("gga_x_pbe", "gga_c_pbe")


def freq(n):
    return np.array([i if i <= (n - 1) // 2 else i - n for i in range(n)], dtype=float)


def fields():
    """rho (2, nz, ny, nx) with x fastest (the library's cube order), V_loc and the Poisson multiplier, all float64"""
    z, y, x = np.meshgrid(np.arange(NZ) / NZ, np.arange(NY) / NY, np.arange(NX) / NX, indexing="ij")
    c = lambda t: np.cos(2 * math.pi * t)                                   # noqa: E731
    s = lambda t: np.sin(2 * math.pi * t)                                   # noqa: E731
    up = 0.06 * np.exp(0.9 * c(x) + 0.6 * s(y) - 0.7 * c(z) + 0.3 * s(x + y))
    dip = 0.25 * (1 + c(x)) * (1 + c(y - 0.2)) * (1 + c(z + 0.1)) / 2       # 0 ... 1, one smooth bump
    dn = 0.02 * np.exp(0.5 * s(x) - 0.8 * c(y) + 0.4 * s(z) - 29.0 * dip)
    assert dn.min() < THRESHOLD < 1e-3 < up.min() and dn.min() > 1e-20
    vloc = -0.8 * c(x + z) + 0.3 * s(y) - 0.2 * c(2 * x - y)
    g = [freq(n) for n in (NX, NY, NZ)]
    G = np.einsum("aj,jzyx->azyx", RECIP, np.stack(np.meshgrid(g[2], g[1], g[0], indexing="ij")[::-1]))
    G2 = (G * G).sum(axis=0)
    green = np.where(G2 > 0, 4 * math.pi / np.where(G2 > 0, G2, 1.0), 0.0)
    return np.stack([up, dn]), vloc, green


class Fourier:
    """forward / backward cube transforms (unnormalised / divided by N) and the cartesian G, in one float type"""

    def __init__(self, ft, shape=(NX, NY, NZ), recip=RECIP):
        self.ft = ft
        nx, ny, nz = shape
        self.n = nx * ny * nz
        g = [freq(n).astype(ft) for n in shape]
        gz, gy, gx = np.meshgrid(g[2], g[1], g[0], indexing="ij")
        B = np.asarray(recip).astype(ft)
        self.G = [B[a, 0] * gx + B[a, 1] * gy + B[a, 2] * gz for a in range(3)]
        if ft is not np.float64:
            self.mats = []
            for n in (nz, ny, nx):
                jk = np.outer(np.arange(n), np.arange(n)) % n
                ang = (-2 * PI_LD / LD(n)) * jk.astype(LD)
                self.mats.append(np.cos(ang) + 1j * np.sin(ang))

    def fft(self, f):
        if self.ft is np.float64:
            return np.fft.fftn(f, axes=(-3, -2, -1))
        Mz, My, Mx = self.mats
        return np.einsum("ax,by,cz,...zyx->...cba", Mx, My, Mz, f.astype(np.clongdouble))

    def ifft_real(self, c):
        if self.ft is np.float64:
            return np.fft.ifftn(c, axes=(-3, -2, -1)).real
        Mz, My, Mx = (np.conj(m) for m in self.mats)
        return np.einsum("ax,by,cz,...zyx->...cba", Mx, My, Mz, c).real / self.ft(self.n)


def twin(ft, rho, vloc, green, gga=PBE, threshold=THRESHOLD, shape=(NX, NY, NZ), recip=RECIP, volume=VOL):
    """(V (2, nz, ny, nx), [E_Hartree, E_xc, E_loc]) in the float type ft, for rho (2, nz, ny, nx) on a cell with the given
    reciprocal lattice (columns = reciprocal vectors) and volume"""
    F = Fourier(ft, shape, recip)
    n_pts, dvol = F.n, volume / F.n
    rho = rho.astype(ft)
    rho_G = F.fft(rho)
    grad = np.stack([[F.ifft_real(1j * F.G[a] * rho_G[s]) for a in range(3)] for s in range(2)])     # [s][a]
    suu, sud, sdd = (grad[0] * grad[0]).sum(0), (grad[0] * grad[1]).sum(0), (grad[1] * grad[1]).sum(0)
    flat = lambda a: a.reshape(-1)                                          # noqa: E731
    pw = S.pointwise(gga, flat(rho[0]), flat(rho[1]), flat(suu), flat(sud), flat(sdd), threshold)
    pw = {k: v.reshape(rho[0].shape) for k, v in pw.items()}
    V = np.zeros_like(rho)
    for s, (vr, vss, other) in enumerate((("vup", "vsuu", 1), ("vdn", "vsdd", 0))):
        flux = [pw[vss] * grad[s][a] + ft(0.5) * pw["vsud"] * grad[other][a] for a in range(3)]
        div = F.ifft_real(sum(1j * F.G[a] * F.fft(flux[a]) for a in range(3)))
        V[s] = pw[vr] - 2 * div
    E = [ft(0), pw["e"].sum() * ft(dvol), ft(0)]
    if green is not None:
        tot_G = rho_G[0] + rho_G[1]
        V += F.ifft_real(green.astype(ft) * tot_G)[None]
        E[0] = ft(0.5) * ft(volume) / (ft(n_pts) * ft(n_pts)) * (green.astype(ft) * (tot_G.real ** 2 + tot_G.imag ** 2)).sum()
    if vloc is not None:
        V += vloc.astype(ft)[None]
        E[2] = ((rho[0] + rho[1]) * vloc.astype(ft)).sum() * ft(dvol)
    return V, E


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def cube(lib):
    bs = Basis(lib, NX, NY, NZ, VOL)
    return bs, KBlock(lib, bs, np.arange(N), np.zeros(N))


BH = np.asfortranarray(RECIP)


def device(lib, cube, rho, vloc, green, mask, want_energies=True, entry="dftk_mi_local_potential_collinear_gga"):
    bs, kb = cube
    rd = dev(rho)
    vd = dev(vloc) if vloc is not None else None
    gd = dev(green) if green is not None else None
    V = torch.full(rho.shape, NAN, dtype=torch.float64, device="cuda")
    E = (C.c_double * 3)(NAN, NAN, NAN) if want_energies else None
    args = (vd.data_ptr() if vd is not None else None, gd.data_ptr() if gd is not None else None)
    torch.cuda.synchronize()
    if entry == "dftk_mi_local_potential_collinear":
        abi_check(lib.dftk_mi_local_potential_collinear(kb.h, rd.data_ptr(), *args, mask, V.data_ptr(), E))
    elif entry == "dftk_mi_local_potential_gga":
        abi_check(lib.dftk_mi_local_potential_gga(kb.h, BH.ctypes.data, rd.data_ptr(), *args, mask, THRESHOLD, V.data_ptr(), E))
    else:
        abi_check(lib.dftk_mi_local_potential_collinear_gga(kb.h, BH.ctypes.data, rd.data_ptr(), *args, mask, THRESHOLD,
                                                            V.data_ptr(), E))
    bs.sync()
    return V.cpu().numpy(), (list(E) if E is not None else None)


def relerr(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b ** 2).sum()))


def held(label, got, got64, ref):
    """err <= 64 max(e_np, 2.2e-16); prints err / e_np"""
    err, e_np = relerr(got, ref), relerr(got64, ref)
    print(f"[spin-gga pipeline] {label}: err {err:.3e}, e_np {e_np:.3e}, err / max(e_np, eps) = {err / max(e_np, EPS):.2f}")
    assert err <= FACTOR * max(e_np, EPS), (label, err, e_np)


def test_against_the_numpy_twin(lib, cube):
    """V_up, V_down and the three energies of PBE with Hartree and V_loc, and of exchange and correlation alone"""
    rho, vloc, green = fields()
    for mask, names in ((24, PBE), (8, PBE[:1]), (16, PBE[1:])):
        V64, E64 = twin(np.float64, rho, vloc, green, gga=names)
        Vld, Eld = twin(LD, rho, vloc, green, gga=names)
        V, E = device(lib, cube, rho, vloc, green, mask)
        assert np.all(np.isfinite(V))
        for s, name in enumerate(("V_up", "V_down")):
            held(f"mask {mask} {name}", V[s], V64[s], Vld[s])
        for k, name in enumerate(("Hartree", "Xc", "AtomicLocal")):
            held(f"mask {mask} E_{name}", [E[k]], [E64[k]], [Eld[k]])


def test_potential_is_the_derivative_of_the_energy(lib, cube):
    """[E_xc(rho + h d) - E_xc(rho - h d)] / 2h against sum_s int V_xc,s d_s for two smooth (d_up, d_down), V_loc and the
    Poisson multiplier NULL, at h and h / 2: the difference falls fourfold (a central difference; between 3.5 and 4.5 is
    asked, the next term being O(h^2) of the first), and at h / 2 it is within ten times what the float64 twin shows."""
    rho, _, _ = fields()
    z, y, x = np.meshgrid(np.arange(NZ) / NZ, np.arange(NY) / NY, np.arange(NX) / NX, indexing="ij")
    shapes = ((np.cos(2 * math.pi * (x - y)), 0.5 * np.sin(2 * math.pi * z)),
              (0.3 + 0.5 * np.sin(2 * math.pi * (y + z)), -np.cos(2 * math.pi * (x + 0.3))))
    h = 0.08

    def gap(energy, V, d, step):
        fd = (energy(rho + step * d) - energy(rho - step * d)) / (2 * step)
        return float(abs(fd - (V * d).sum() * DVOL))
    V, _ = device(lib, cube, rho, None, None, 24)
    V64, _ = twin(np.float64, rho, None, None)
    for w_up, w_dn in shapes:
        d = np.stack([rho[0] * w_up, rho[1] * w_dn])              # relative perturbations: the densities stay positive
        dev_gap = [gap(lambda r: device(lib, cube, r, None, None, 24)[1][1], V, d, st) for st in (h, h / 2)]
        twin_gap = [gap(lambda r: float(twin(np.float64, r, None, None)[1][1]), V64, d, st) for st in (h, h / 2)]
        print(f"[spin-gga pipeline] dE - int V drho: device {dev_gap[0]:.3e} -> {dev_gap[1]:.3e}, twin {twin_gap[0]:.3e} -> "
              f"{twin_gap[1]:.3e}")
        assert 3.5 < dev_gap[0] / dev_gap[1] < 4.5, dev_gap
        assert dev_gap[1] <= 10 * twin_gap[1], (dev_gap, twin_gap)


def test_unpolarised_limit(lib, cube):
    """rho_up = rho_down = rho / 2: V_up = V_down bit for bit, and both and the energies are those of
    dftk_mi_local_potential_gga(rho) within the bound of the twin test"""
    rho2, vloc, green = fields()
    rho = rho2[0] + rho2[1]
    half = np.stack([rho / 2, rho / 2])
    V, E = device(lib, cube, half, vloc, green, 24)
    assert np.array_equal(V[0], V[1])
    V1, E1 = device(lib, cube, rho, vloc, green, 24, entry="dftk_mi_local_potential_gga")
    V64, E64 = twin(np.float64, half, vloc, green)
    Vld, Eld = twin(LD, half, vloc, green)
    held("unpolarised V, collinear entry", V[0], V64[0], Vld[0])
    held("unpolarised V, unpolarised entry", V1, V64[0], Vld[0])
    e_np = max(relerr(V64[0], Vld[0]), EPS)
    assert relerr(V[0], V1) <= 2 * FACTOR * e_np
    for k in range(3):
        held(f"unpolarised E[{k}], collinear entry", [E[k]], [E64[k]], [Eld[k]])
        held(f"unpolarised E[{k}], unpolarised entry", [E1[k]], [E64[k]], [Eld[k]])


@pytest.mark.parametrize("mask", [1 | 4, 32, 0])
def test_without_gga_bits_it_is_the_collinear_entry(lib, cube, mask):
    rho, vloc, green = fields()
    V, E = device(lib, cube, rho, vloc, green, mask)
    V0, E0 = device(lib, cube, rho, vloc, green, mask, entry="dftk_mi_local_potential_collinear")
    assert np.array_equal(V, V0) and E == E0 and np.all(np.isfinite(V))


def test_lda_bits_mix_with_gga_bits(lib, cube):
    """lda_x | gga_c_pbe: the LDA part is added in the final pass -- the sum of the two separate calls (XC only)"""
    rho, _, _ = fields()
    V, E = device(lib, cube, rho, None, None, 1 | 16)
    Va, Ea = device(lib, cube, rho, None, None, 1, entry="dftk_mi_local_potential_collinear")
    Vb, Eb = device(lib, cube, rho, None, None, 16)
    assert np.max(np.abs(V - (Va + Vb))) <= 4 * EPS * np.max(np.abs(Va) + np.abs(Vb))
    assert abs(E[1] - (Ea[1] + Eb[1])) <= 4 * EPS * (abs(Ea[1]) + abs(Eb[1]))


def counters(lib):
    a, b = C.c_int64(), C.c_int64()
    abi_check(lib.dftk_mi_launch_count(C.byref(a), C.byref(b)))
    return a.value, b.value


def test_without_energies_the_call_does_not_synchronise(lib, cube):
    """energies_h = NULL: no fetch and no host synchronisation; with energies exactly one.  The same launches either way but
    the fetch (printed: DESIGN.md section 3.6 states the count)."""
    bs, kb = cube
    rho, vloc, green = fields()
    rd, vd, gd = dev(rho), dev(vloc), dev(green)
    V = torch.full(rho.shape, NAN, dtype=torch.float64, device="cuda")
    E = (C.c_double * 3)()
    call = lambda e: abi_check(lib.dftk_mi_local_potential_collinear_gga(                     # noqa: E731
        kb.h, BH.ctypes.data, rd.data_ptr(), vd.data_ptr(), gd.data_ptr(), 24, THRESHOLD, V.data_ptr(), e))
    call(E)                                       # (scratch is grown on the first call)
    bs.sync()
    l0, s0 = counters(lib)
    call(None)
    l1, s1 = counters(lib)
    bs.sync()
    want = V.cpu().numpy().copy()
    l2, s2 = counters(lib)
    call(E)
    l3, s3 = counters(lib)
    print(f"[spin-gga pipeline] launches without energies {l1 - l0}, with energies {l3 - l2}")
    assert s1 == s0 and s3 == s2 + 1
    assert 0 < l1 - l0 <= l3 - l2 <= l1 - l0 + 1
    assert np.array_equal(V.cpu().numpy(), want) and np.all(np.isfinite(want))


def test_refusals_write_nothing(lib, cube):
    bs, kb = cube
    rd = dev(np.ones((2, NZ, NY, NX)))
    V = torch.full((2 * N,), NAN, dtype=torch.float64, device="cuda")
    E = (C.c_double * 3)(7.0, 7.0, 7.0)
    for bad_mask in (2, 64, 8 | 2, 24 | 128):
        assert lib.dftk_mi_local_potential_collinear_gga(kb.h, BH.ctypes.data, rd.data_ptr(), None, None, bad_mask, THRESHOLD,
                                                         V.data_ptr(), E) == -1
    assert lib.dftk_mi_local_potential_collinear_gga(kb.h, None, rd.data_ptr(), None, None, 24, THRESHOLD, V.data_ptr(), E) == -1
    bs.sync()
    assert np.all(np.isnan(V.cpu().numpy())) and list(E) == [7.0, 7.0, 7.0]
