"""``dftk_mi_local_potential_core`` and ``dftk_mi_cube_gradient`` at the C ABI: the local-potential pipelines with the core
density of a non-linear core correction as one more operand, on the 12 x 10 x 9 cube and the triclinic reciprocal lattice of
tests/test_gpu_spin_gga_pipeline.py (two even axes: unpaired Nyquist planes) and on a 9 x 7 x 11 cube (all axes odd).

References, none of them a restatement of the new code:
* the composition of two calls of the EXISTING entry of the same kind -- one on rho with no functional (Hartree, local energy,
  V_loc + V_H), one on rho_s + rho_core / n_spin with the other two terms off (E_xc, v_xc);
* NumPy FFTs for the gradient;
* the oracle's ``xc_energy_potential`` / ``xc_energy_potential_spin`` and the long-double twin of
  tests/test_gpu_spin_gga_pipeline.py, called unchanged on rho + rho_core;
* central differences of E_xc at fixed core.

Bounds.  LDA is point-wise: the XC argument rho_s + rho_core / n_spin is one rounded sum in the kernel and in NumPy alike, so
E_xc is bit-identical (same block partition) and V differs by the rounding of its three-term sum, held to
4 x 2.2e-16 x (|V_loc| + max|V_H| + |v_xc|).  For PBE grad(rho + rho_core) and grad rho + grad rho_core differ by rounding
that sigma and the flux amplify where the density is small; no bound can be derived, so it is measured: the existing PBE
entry is run on an input perturbed by one ulp per point at random, and ten times what it moves is the bound (printed,
``pytest -s``; DESIGN.md section 3.19 records the numbers).  No density of the test sits within an ulp of a threshold: there
one ulp switches a point on or off and the "movement" would be the whole potential of that point.  E_xc is a single double,
so its measured movement is at least one spacing of that double.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check as abi_check  # noqa: E402
from oracle import terms as oterms  # noqa: E402

import test_gpu_spin_gga_pipeline as P  # noqa: E402
import test_xc_reference as R  # noqa: E402
from test_gpu_kernels import Basis, KBlock, dev  # noqa: E402

CUBES = {"even": (12, 10, 9), "odd": (9, 7, 11)}
RECIP = P.RECIP
BH = np.asfortranarray(RECIP)
VOL = P.VOL
THRESHOLD = 1e-12
EPS = 2.2e-16
EINVAL = -1
NAN = float("nan")
KINDS = {"lda": (1, 1 | 4), "lda-spin": (2, 1 | 4), "pbe": (1, 24), "pbe-spin": (2, 24)}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def cubes(lib):
    out = {}
    for name, (nx, ny, nz) in CUBES.items():
        bs = Basis(lib, nx, ny, nz, VOL)
        out[name] = (bs, KBlock(lib, bs, np.arange(nx * ny * nz), np.zeros(nx * ny * nz)))
    return out


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _out(n_spin, shape, want_V, want_E):
    V = torch.full((n_spin,) + shape if n_spin == 2 else shape, NAN, dtype=torch.float64, device="cuda") if want_V else None
    E = (C.c_double * 3)(NAN, NAN, NAN) if want_E else None
    return V, E


def fused(lib, cube, n_spin, rho, core, gcore, vloc, green, mask, want_V=True, want_E=True):
    """dftk_mi_local_potential_core; returns (V or None, [E_H, E_xc, E_loc] or None)"""
    bs, kb = cube
    rd, cd_, gd, vd, pd = (dev(a) if a is not None else None for a in (rho, core, gcore, vloc, green))
    V, E = _out(n_spin, rho.shape[-3:], want_V, want_E)
    torch.cuda.synchronize()
    abi_check(lib.dftk_mi_local_potential_core(kb.h, BH.ctypes.data, n_spin, rd.data_ptr(), _ptr(cd_), _ptr(gd), _ptr(vd),
                                               _ptr(pd), mask, THRESHOLD, _ptr(V), E))
    bs.sync()
    return (V.cpu().numpy() if V is not None else None), (list(E) if E is not None else None)


def existing(lib, cube, n_spin, rho, vloc, green, mask, want_V=True, want_E=True, gga_kind=False):
    """the existing entry of the kind (n_spin, LDA / GGA)"""
    bs, kb = cube
    rd, vd, pd = (dev(a) if a is not None else None for a in (rho, vloc, green))
    V, E = _out(n_spin, rho.shape[-3:], want_V, want_E)
    torch.cuda.synchronize()
    a = (_ptr(vd), _ptr(pd))
    if n_spin == 1 and not gga_kind:
        abi_check(lib.dftk_mi_local_potential(kb.h, rd.data_ptr(), *a, mask, _ptr(V), E))
    elif n_spin == 1:
        abi_check(lib.dftk_mi_local_potential_gga(kb.h, BH.ctypes.data, rd.data_ptr(), *a, mask, THRESHOLD, _ptr(V), E))
    elif not gga_kind:
        abi_check(lib.dftk_mi_local_potential_collinear(kb.h, rd.data_ptr(), *a, mask, _ptr(V), E))
    else:
        abi_check(lib.dftk_mi_local_potential_collinear_gga(kb.h, BH.ctypes.data, rd.data_ptr(), *a, mask, THRESHOLD,
                                                            _ptr(V), E))
    bs.sync()
    return (V.cpu().numpy() if V is not None else None), (list(E) if E is not None else None)


def gradient(lib, cube, f):
    bs, kb = cube
    fd = dev(f)
    out = torch.full((3,) + f.shape, NAN, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    abi_check(lib.dftk_mi_cube_gradient(kb.h, BH.ctypes.data, fd.data_ptr(), out.data_ptr()))
    bs.sync()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ inputs
def random_fields(shape, n_spin, seed):
    """random positive rho (n_spin cubes) and rho_core, log-uniform over 1e-16 ... 1, with planted points around the floors:
    rho below the GGA threshold (1e-12) / the spin floor (1e-20) / the 1e-300 guard with rho + rho_core above it and below
    it, zero and tiny core points; V_loc and the Poisson multiplier of the cell"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    rho = 10.0 ** rng.uniform(-16, 0, size=(n_spin, nz, ny, nx))
    core = 10.0 ** rng.uniform(-16, 0, size=(nz, ny, nx))
    flat_r, flat_c = rho.reshape(n_spin, -1), core.reshape(-1)
    plant = [(1e-13, 0.5), (1e-13, 1e-14), (3e-13, 8e-13), (1e-21, 1e-3), (1e-21, 1e-22), (0.0, 0.0), (0.0, 0.2),
             (1e-301, 1e-302), (0.3, 0.0), (0.3, 1e-25), (5e-21, 1.2e-20), (4e-13, 5e-13)]
    idx = (np.arange(len(plant)) * 37 + 5) % flat_c.size
    for i, (r, c) in zip(idx, plant):
        flat_r[:, i] = r / n_spin if n_spin == 2 else r
        flat_c[i] = c
    if n_spin == 2:
        flat_r[1, idx[0]] *= 0.25                       # (channels apart at a planted point)
    tot = rho.sum(axis=0) if n_spin == 2 else rho
    assert np.any((tot <= THRESHOLD) & (tot + core > THRESHOLD)) and np.any((tot <= THRESHOLD) & (tot + core <= THRESHOLD))
    z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
    vloc = -0.8 * np.cos(2 * math.pi * (x + z)) + 0.3 * np.sin(2 * math.pi * y) + rng.uniform(-0.1, 0.1, size=x.shape)
    F = P.Fourier(np.float64, shape, RECIP)
    G2 = sum(g * g for g in F.G)
    green = np.where(G2 > 0, 4 * math.pi / np.where(G2 > 0, G2, 1.0), 0.0)
    return (rho if n_spin == 2 else rho[0]), core, vloc, green


def smooth_fields(shape, n_spin):
    """smooth positive rho and rho_core (the densities of tests/test_gpu_spin_gga_pipeline.py on this cube, without the dip
    below the threshold)"""
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
    c = lambda t: np.cos(2 * math.pi * t)                                   # noqa: E731
    s = lambda t: np.sin(2 * math.pi * t)                                   # noqa: E731
    up = 0.06 * np.exp(0.9 * c(x) + 0.6 * s(y) - 0.7 * c(z) + 0.3 * s(x + y))
    dn = 0.02 * np.exp(0.5 * s(x) - 0.8 * c(y) + 0.4 * s(z))
    core = 0.09 * np.exp(1.1 * c(x - 0.2) + 0.9 * c(y + 0.1) + 1.3 * c(z - 0.3))
    rho = np.stack([up, dn]) if n_spin == 2 else up + dn
    return rho, core


def with_core(rho, core, n_spin):
    return rho + core[None] / 2 if n_spin == 2 else rho + core


# ------------------------------------------------------------------------------------------------ composition
def _perturbed(a, rng):
    """every entry moved by one ulp, up or down at random (zeros stay)"""
    up = rng.integers(0, 2, size=a.shape).astype(bool)
    return np.where(a == 0, a, np.where(up, np.nextafter(a, np.inf), np.nextafter(a, -np.inf)))


@pytest.mark.parametrize("cube_name", sorted(CUBES))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_against_the_composition_of_two_existing_calls(lib, cubes, kind, cube_name):
    n_spin, mask = KINDS[kind]
    gga = bool(mask & 24)
    cube, shape = cubes[cube_name], CUBES[cube_name]
    rho, core, vloc, green = random_fields(shape, n_spin, seed=3 + len(kind))
    gcore = gradient(lib, cube, core) if gga else None
    rho_x = with_core(rho, core, n_spin)
    # XC alone on rho + rho_core / n_spin: E_xc and v_xc
    Vx, Ex = existing(lib, cube, n_spin, rho_x, None, None, mask, gga_kind=gga)
    assert np.all(np.isfinite(Vx))
    rng = np.random.default_rng(17)
    for use_vloc in (False, True):
        for use_green in (False, True):
            vl, gr = (vloc if use_vloc else None), (green if use_green else None)
            # Hartree, the local energy and V_loc + V_H on rho, no functional
            V0, E0 = existing(lib, cube, n_spin, rho, vl, gr, 0, gga_kind=gga)
            want_V = V0 + Vx
            if gga:
                # how far the existing PBE entry moves under one ulp per point: ten times that is the bound
                Va, Ea = existing(lib, cube, n_spin, rho_x, vl, gr, mask, gga_kind=True)
                Vb, Eb = existing(lib, cube, n_spin, _perturbed(rho_x, rng), vl, gr, mask, gga_kind=True)
                # (E_xc is ONE double: a movement below its spacing cannot be observed, so one spacing is the least
                # the measurement can return)
                moved_V, moved_E = float(np.max(np.abs(Vb - Va))), max(abs(Eb[1] - Ea[1]), float(np.spacing(abs(Ea[1]))))
                bound_V, bound_E = 10 * moved_V, 10 * moved_E
            else:
                vh = existing(lib, cube, n_spin, rho, None, gr, 0)[0] if use_green else np.zeros_like(Vx)
                bound_V = 4 * EPS * ((np.abs(vloc) if use_vloc else 0.0) + np.max(np.abs(vh)) + np.abs(Vx))
                bound_E = 0.0
            for want_v, want_e in ((True, True), (True, False), (False, True)):
                V, E = fused(lib, cube, n_spin, rho, core, gcore, vl, gr, mask, want_v, want_e)
                label = f"{kind} {cube_name} vloc={use_vloc} green={use_green} V={want_v} E={want_e}"
                if want_v:
                    assert V.shape == want_V.shape and np.all(np.isfinite(V)), label      # every point written
                    err = np.abs(V - want_V)
                    if gga:
                        print(f"[nlcc composition] {label}: V differs by {err.max():.3e}; one ulp per point moves the "
                              f"existing entry by {moved_V:.3e} (bound {bound_V:.3e})")
                    assert np.all(err <= bound_V), (label, float(err.max()))
                if want_e:
                    if gga:
                        print(f"[nlcc composition] {label}: E_xc differs by {abs(E[1] - Ex[1]):.3e}; one ulp per point moves "
                              f"it by {moved_E:.3e} (bound {bound_E:.3e})")
                    assert abs(E[1] - Ex[1]) <= bound_E, (label, E[1], Ex[1])
                    # the core enters neither the local nor the Hartree energy
                    assert E[2] == E0[2], (label, E[2], E0[2])
                    if gga and n_spin == 2:
                        # (the collinear GGA pipeline sums F[rho_up] + F[rho_down], the call without a functional transforms
                        # rho_up + rho_down: two roundings of one sum; the rule of 64 eps of DESIGN.md 3.1.1)
                        assert abs(E[0] - E0[0]) <= 64 * EPS * abs(E0[0]), (label, E[0], E0[0])
                    else:
                        assert E[0] == E0[0], (label, E[0], E0[0])


@pytest.mark.parametrize("cube_name", sorted(CUBES))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_without_a_core_it_is_the_existing_entry_bit_for_bit(lib, cubes, kind, cube_name):
    n_spin, mask = KINDS[kind]
    gga = bool(mask & 24)
    cube, shape = cubes[cube_name], CUBES[cube_name]
    rho, core, vloc, green = random_fields(shape, n_spin, seed=29)
    for vl, gr in ((vloc, green), (None, None)):
        V0, E0 = existing(lib, cube, n_spin, rho, vl, gr, mask, gga_kind=gga)
        # rho_core_d == NULL; grad_core_d is ignored then, given or not
        for gcore in (None, np.ones((3,) + core.shape)):
            V, E = fused(lib, cube, n_spin, rho, None, gcore, vl, gr, mask)
            assert np.array_equal(V, V0) and E == E0 and np.all(np.isfinite(V))
    # and the core changes E_xc but neither the Hartree nor the local energy, bit for bit
    gcore = gradient(lib, cube, core) if gga else None
    _, E1 = fused(lib, cube, n_spin, rho, core, gcore, vloc, green, mask)
    _, E0 = existing(lib, cube, n_spin, rho, vloc, green, mask, gga_kind=gga)
    assert E1[0] == E0[0] and E1[2] == E0[2] and E1[1] != E0[1]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_two_calls_give_identical_bits(lib, cubes, kind):
    n_spin, mask = KINDS[kind]
    cube, shape = cubes["even"], CUBES["even"]
    rho, core, vloc, green = random_fields(shape, n_spin, seed=41)
    gcore = gradient(lib, cube, core)
    assert np.array_equal(gcore, gradient(lib, cube, core))
    V1, E1 = fused(lib, cube, n_spin, rho, core, gcore, vloc, green, mask)
    existing(lib, cube, 1, np.abs(vloc), None, None, 1)                     # (something else through the same scratch)
    V2, E2 = fused(lib, cube, n_spin, rho, core, gcore, vloc, green, mask)
    assert np.array_equal(V1, V2) and E1 == E2


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_no_launch_and_no_synchronisation_more_than_the_existing_entry(lib, cubes, kind):
    """the core is an operand of passes that run anyway: the library's launch counter (kernels and transform stages) moves
    by the same amount for the entry with a core and the existing entry of the kind, with and without energies; without
    energies neither synchronises (printed: DESIGN.md section 3.19 states the counts)"""
    n_spin, mask = KINDS[kind]
    gga = bool(mask & 24)
    cube, shape = cubes["even"], CUBES["even"]
    bs, kb = cube
    rho, core, vloc, green = random_fields(shape, n_spin, seed=53)
    gcore = gradient(lib, cube, core)
    rd, cd_, gd, vd, pd = (dev(a) for a in (rho, core, gcore, vloc, green))
    V = torch.empty(rho.shape, dtype=torch.float64, device="cuda")
    E = (C.c_double * 3)()
    B = BH.ctypes.data

    def with_core(e):
        abi_check(lib.dftk_mi_local_potential_core(kb.h, B, n_spin, rd.data_ptr(), cd_.data_ptr(), gd.data_ptr(),
                                                   vd.data_ptr(), pd.data_ptr(), mask, THRESHOLD, V.data_ptr(), e))

    def without(e):
        a = (rd.data_ptr(), vd.data_ptr(), pd.data_ptr(), mask)
        if n_spin == 1 and not gga:
            abi_check(lib.dftk_mi_local_potential(kb.h, *a, V.data_ptr(), e))
        elif n_spin == 1:
            abi_check(lib.dftk_mi_local_potential_gga(kb.h, B, *a, THRESHOLD, V.data_ptr(), e))
        elif not gga:
            abi_check(lib.dftk_mi_local_potential_collinear(kb.h, *a, V.data_ptr(), e))
        else:
            abi_check(lib.dftk_mi_local_potential_collinear_gga(kb.h, B, *a, THRESHOLD, V.data_ptr(), e))
    counts = {}
    for name, call in (("core", with_core), ("existing", without)):
        call(E)                                   # (scratch is grown on the first call)
        bs.sync()
        for e in (None, E):
            l0, s0 = P.counters(lib)
            call(e)
            l1, s1 = P.counters(lib)
            bs.sync()
            counts[name, e is not None] = (l1 - l0, s1 - s0)
    print(f"[nlcc launches] {kind}: with a core {counts['core', False]} / {counts['core', True]}, existing entry "
          f"{counts['existing', False]} / {counts['existing', True]} (launches, synchronisations; without / with energies)")
    for e in (False, True):
        assert counts["core", e] == counts["existing", e] and counts["core", e][0] > 0
    assert counts["core", False][1] == 0 and counts["core", True][1] == 1


# ------------------------------------------------------------------------------------------------ the gradient
@pytest.mark.parametrize("cube_name", sorted(CUBES))
def test_cube_gradient_against_numpy(lib, cubes, cube_name):
    """Re ifftn(i G_a fftn(f)) with the G of the pipeline's twin (tests/test_gpu_spin_gga_pipeline.py::Fourier: the unpaired
    Nyquist entries of an even axis carry G = -n/2 and are kept, their imaginary contribution dropped with the real part),
    a random (rough) cube and a smooth one; 64 x max(e_np, eps) in the 2-norm, e_np the error of the NumPy chain against
    its long-double spelling"""
    cube, shape = cubes[cube_name], CUBES[cube_name]
    nx, ny, nz = shape
    rng = np.random.default_rng(5)
    F64, FLD = P.Fourier(np.float64, shape, RECIP), P.Fourier(P.LD, shape, RECIP)
    for label, f in (("random", rng.standard_normal((nz, ny, nx))), ("smooth", smooth_fields(shape, 1)[1])):
        got = gradient(lib, cube, f)
        assert np.all(np.isfinite(got))
        for a in range(3):
            g64 = F64.ifft_real(1j * F64.G[a] * F64.fft(f))
            gld = FLD.ifft_real(1j * FLD.G[a] * FLD.fft(f.astype(P.LD)))
            err, e_np = P.relerr(got[a], gld), P.relerr(g64, gld)
            print(f"[nlcc gradient] {cube_name} {label} d_{a}: err {err:.3e}, e_np {e_np:.3e}")
            assert err <= 64 * max(e_np, EPS), (label, a, err, e_np)


def test_gradient_of_the_sum_is_the_sum_of_the_gradients_to_rounding(lib, cubes):
    cube, shape = cubes["even"], CUBES["even"]
    rho, core = smooth_fields(shape, 1)
    a, b, ab = gradient(lib, cube, rho), gradient(lib, cube, core), gradient(lib, cube, rho + core)
    assert np.max(np.abs(ab - (a + b))) <= 64 * EPS * np.max(np.abs(ab))


# ------------------------------------------------------------------------------------------------ independent references
class _OracleBasis:
    """what oracle.terms.xc_energy_potential(_spin) asks of a basis, on this cube"""

    def __init__(self, shape, functionals):
        F = P.Fourier(np.float64, shape, RECIP)
        self._G = np.stack(F.G, axis=-1)
        self.model = SimpleNamespace(functionals=functionals)
        self.dvol = VOL / (shape[0] * shape[1] * shape[2])

    def G_vectors_cart_cube(self):
        return self._G

    def fft_cube(self, f):
        return np.fft.fftn(f)

    def irfft_cube(self, c):
        return np.fft.ifftn(c).real


@pytest.mark.parametrize("n_spin", [1, 2])
def test_lda_against_the_oracle_on_rho_plus_core(lib, cubes, n_spin):
    """point by point at the tolerance of tests/test_gpu_xc_pointwise.py: (8 + 1) x max(E_REF, 4 x 2^-52) x the LDA-exchange
    potential of the total argument -- 8 for the kernel against the exact value, 1 for the oracle's own error E_REF"""
    cube, shape = cubes["even"], CUBES["even"]
    rho, core, _, _ = random_fields(shape, n_spin, seed=7)
    # (the range the fixtures of E_REF cover without the 1e-300 guard; planted zeros stay)
    rho_x = with_core(rho, core, n_spin)
    funs = ("lda_x", "lda_c_pw")
    ob = _OracleBasis(shape, funs)
    Eo, Vo = (oterms.xc_energy_potential_spin if n_spin == 2 else oterms.xc_energy_potential)(ob, rho_x)
    V, E = fused(lib, cube, n_spin, rho, core, None, None, None, 1 | 4)
    tot = rho_x.sum(axis=0) if n_spin == 2 else rho_x
    dec = np.floor(np.log10(np.maximum(tot, 1e-300))).reshape(-1)
    fam = "spin" if n_spin == 2 else "lda"
    for s in range(n_spin):
        q = ("vup", "vdn")[s] if n_spin == 2 else "v"
        bound = sum(R.bound_of((fam, f, q), dec, R.MARGIN + 1) for f in funs).reshape(tot.shape)
        got, ref = (V[s], Vo[s]) if n_spin == 2 else (V, Vo)
        scale = R.v_x(tot)
        bad = ~(np.abs(got - ref) <= bound * scale)
        worst = float(np.max(R.scaled_error(got, ref, scale)))
        print(f"[nlcc oracle] n_spin {n_spin} channel {s}: worst scaled error {worst:.3e}")
        assert not bad.any(), (n_spin, s, worst)
    e_bound = float(np.sum(sum(R.bound_of((fam, f, "e"), dec, R.MARGIN + 1) for f in funs) * R.e_x(tot).reshape(-1))) * ob.dvol
    assert abs(E[1] - Eo) <= e_bound, (E[1], Eo, e_bound)


def test_pbe_against_the_oracle_on_rho_plus_core(lib, cubes):
    """unpolarised PBE: ``xc_energy_potential`` of the oracle on rho + rho_core (float64 NumPy), and the long-double twin of
    tests/test_gpu_spin_gga_pipeline.py at rho_up = rho_down = (rho + rho_core) / 2 as the yardstick e_np: the device within
    64 x max(e_np, eps) of the twin (that test's rule), and of the oracle within 65 x (the oracle carries e_np itself)"""
    cube, shape = cubes["even"], CUBES["even"]
    rho, core = smooth_fields(shape, 1)
    gcore = gradient(lib, cube, core)
    V, E = fused(lib, cube, 1, rho, core, gcore, None, None, 24)
    Eo, Vo = oterms.xc_energy_potential(_OracleBasis(shape, P.PBE), rho + core)
    half = np.stack([(rho + core) / 2] * 2)
    Vld, Eld = P.twin(P.LD, half, None, None, shape=shape)
    e_np = max(P.relerr(Vo, Vld[0]), EPS)
    err_t, err_o = P.relerr(V, Vld[0]), P.relerr(V, Vo)
    print(f"[nlcc oracle] pbe: device against the long-double twin {err_t:.3e}, against the oracle {err_o:.3e}, oracle "
          f"against the twin {e_np:.3e}")
    assert err_t <= 64 * e_np and err_o <= 65 * e_np
    e_E = max(abs(Eo - float(Eld[1])) / abs(float(Eld[1])), EPS)
    assert abs(E[1] - float(Eld[1])) <= 64 * e_E * abs(float(Eld[1])) and abs(E[1] - Eo) <= 65 * e_E * abs(Eo)


def test_spin_pbe_against_the_twin_on_rho_plus_half_the_core(lib, cubes):
    """collinear PBE has no oracle form: the NumPy twin of tests/test_gpu_spin_gga_pipeline.py (float64 and long double),
    called unchanged on rho_s + rho_core / 2, with that test's rule err <= 64 max(e_np, 2.2e-16)"""
    cube, shape = cubes["even"], CUBES["even"]
    rho, core = smooth_fields(shape, 2)
    gcore = gradient(lib, cube, core)
    V, E = fused(lib, cube, 2, rho, core, gcore, None, None, 24)
    rho_x = with_core(rho, core, 2)
    V64, E64 = P.twin(np.float64, rho_x, None, None, shape=shape)
    Vld, Eld = P.twin(P.LD, rho_x, None, None, shape=shape)
    for s in range(2):
        P.held(f"nlcc V[{s}]", V[s], V64[s], Vld[s])
    P.held("nlcc E_xc", [E[1]], [E64[1]], [Eld[1]])


# ------------------------------------------------------------------------------------------------ V = dE / d rho
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_potential_is_the_derivative_of_the_energy_at_fixed_core(lib, cubes, kind):
    """[E_xc(rho + h d) - E_xc(rho - h d)] / 2h against sum_s int v_xc,s d_s with the core held fixed, along two random
    directions (random combinations of the lowest Fourier modes, relative to rho so that it stays positive), at h and h / 2:
    the gap of a central difference falls fourfold (3.5 ... 4.5 is asked: the next term is O(h^2) of the first)"""
    n_spin, mask = KINDS[kind]
    cube, shape = cubes["even"], CUBES["even"]
    nx, ny, nz = shape
    rho, core = smooth_fields(shape, n_spin)
    gcore = gradient(lib, cube, core) if mask & 24 else None
    dvol = VOL / (nx * ny * nz)
    z, y, x = np.meshgrid(np.arange(nz) / nz, np.arange(ny) / ny, np.arange(nx) / nx, indexing="ij")
    rng = np.random.default_rng(23)

    def direction():
        w = sum(rng.uniform(-1, 1) * np.cos(2 * math.pi * (kx * x + ky * y + kz * z + rng.uniform()))
                for kx, ky, kz in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, -1, 0), (0, 1, 1)))
        return w / np.max(np.abs(w))
    V, _ = fused(lib, cube, n_spin, rho, core, gcore, None, None, mask)
    exc = lambda r: fused(lib, cube, n_spin, r, core, gcore, None, None, mask, want_V=False)[1][1]      # noqa: E731
    h = 0.08
    for _ in range(2):
        d = np.stack([rho[0] * direction(), rho[1] * direction()]) if n_spin == 2 else rho * direction()
        lin = float((V * d).sum() * dvol)
        gap = [abs((exc(rho + st * d) - exc(rho - st * d)) / (2 * st) - lin) for st in (h, h / 2)]
        print(f"[nlcc derivative] {kind}: int V d = {lin:.6e}, gap {gap[0]:.3e} -> {gap[1]:.3e}")
        assert 3.5 < gap[0] / gap[1] < 4.5, (kind, gap)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(lib, cubes):
    bs, kb = cubes["even"]
    nx, ny, nz = CUBES["even"]
    N = nx * ny * nz
    rd, cd_ = dev(np.ones((2, nz, ny, nx))), dev(np.full((nz, ny, nx), 0.5))
    gd = dev(np.zeros((3, nz, ny, nx)))
    V = torch.full((2 * N,), NAN, dtype=torch.float64, device="cuda")
    G = torch.full((3 * N,), NAN, dtype=torch.float64, device="cuda")
    E = (C.c_double * 3)(7.0, 7.0, 7.0)
    call = lib.dftk_mi_local_potential_core
    B = BH.ctypes.data
    # a GGA bit with a core but without its gradient (both spin kinds); without the reciprocal lattice
    for n_spin in (1, 2):
        assert call(kb.h, B, n_spin, rd.data_ptr(), cd_.data_ptr(), None, None, None, 24, THRESHOLD, V.data_ptr(), E) == EINVAL
        assert call(kb.h, None, n_spin, rd.data_ptr(), cd_.data_ptr(), gd.data_ptr(), None, None, 24, THRESHOLD,
                    V.data_ptr(), E) == EINVAL
    # n_spin outside {1, 2}
    for n_spin in (0, 3, -1):
        assert call(kb.h, B, n_spin, rd.data_ptr(), cd_.data_ptr(), gd.data_ptr(), None, None, 1, THRESHOLD, V.data_ptr(),
                    E) == EINVAL
    # the masks of the existing entries: VWN has no spin form, TETER93 does not mix with a GGA bit without spin, unknown bits
    for n_spin, bad in ((2, 2), (2, 8 | 2), (1, 24 | 32), (1, 64), (2, 128 | 1)):
        assert call(kb.h, B, n_spin, rd.data_ptr(), cd_.data_ptr(), gd.data_ptr(), None, None, bad, THRESHOLD, V.data_ptr(),
                    E) == EINVAL
    # neither output asked for
    assert call(kb.h, B, 1, rd.data_ptr(), cd_.data_ptr(), gd.data_ptr(), None, None, 1, THRESHOLD, None, None) == EINVAL
    # a k-block that does not span the cube
    part = KBlock(lib, bs, np.arange(N - 3), np.zeros(N - 3))
    for n_spin, mask in ((1, 1), (2, 1), (1, 24), (2, 24)):
        assert call(part.h, B, n_spin, rd.data_ptr(), cd_.data_ptr(), gd.data_ptr(), None, None, mask, THRESHOLD,
                    V.data_ptr(), E) == EINVAL
    assert lib.dftk_mi_cube_gradient(part.h, B, cd_.data_ptr(), G.data_ptr()) == EINVAL
    assert lib.dftk_mi_cube_gradient(kb.h, None, cd_.data_ptr(), G.data_ptr()) == EINVAL
    assert lib.dftk_mi_cube_gradient(kb.h, B, None, G.data_ptr()) == EINVAL
    bs.sync()
    assert np.all(np.isnan(V.cpu().numpy())) and np.all(np.isnan(G.cpu().numpy())) and list(E) == [7.0, 7.0, 7.0]
