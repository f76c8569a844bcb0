"""The three entries of csrc/stress_kernels.hip at the C ABI against the extended-precision references of stress_ref.py
(dual numbers over numpy.longdouble on the strained energy expressions, checked on the host by test_stress_reference.py).

Tolerance everywhere: |device - reference| <= 1e-12 S, S the sum of the absolute values of the terms behind the output
(stress_ref.py) -- the project's bound for sums of this length against NumPy restatements (RTOL of
test_gpu_multispecies.py), not tuned on the kernels; the reference's own error is <= 1e-15 S and a float64 evaluation of
it sits at <= 1e-13 S (1.2e-14 S at most, on the 41 x 40 x 42 cube).  An output whose S is 0 must be exactly 0.

dftk_mi_stress_kinetic_nonlocal: the sheared lattice, k = (0.23, -0.31, 0.17) and positions of test_gpu_multispecies.py,
cube 15 x 16 x 18 (it only decodes G); atoms in group order X, X (the synthetic species with every HGH channel, 29 columns
each), Fe (14), Si (5): n_p = 77.  Complex blocks on subsets of the Ecut sphere with n_G = 1, 255, 256, 257, 513 rows;
Gamma blocks on inversion-symmetric subsets with n_half = 1, 2, 128, 129, 257 and real-symmetric columns, called with the
real mode off and on.  1, 3 and 6 bands, ld_psi = n_G + 7 with NaN in the padding, one weight exactly 0, stress_h
pre-filled, two calls bitwise equal.  On n_G = 257 / n_half = 129 three workspace budgets (DFTK_MI_STRESS_WS_KIB): one
chunk; column chunks [X, X] [Fe, Si]; column chunks [X] [X] [Fe, Si] with band chunks 2 + 1.

dftk_mi_stress_cube: CUBES (all-odd, one / two / three even axes, N < 256, N a multiple of 256 and not, 270 workgroups);
rho = 1 + random + 0.3 cos(pi i) per even axis; no atom, one species, three species (two atoms in the first; one with all
four c_i, Fe with an empty cloc).

dftk_mi_stress_xc: n = 1, 255, 256, 257, 262144, 262145 (the second trip of the 1024-workgroup loop), 524288 + 77; LDA, GGA
and two spin components; signed random inputs.

Largest measured |device - reference| / S per entry (MI355X; every case prints its own figure):
    kinetic   4.8e-16   Gamma block, n_half = 2, one band, real mode off
    nonlocal  6.9e-16   the same case
    cube      3.9e-14   41 x 40 x 42, one species (the Hartree sums: the fp64 FFT of a density with a large mean)
    xc        1.5e-16   n = 1, GGA
Each of these one-line changes of stress_kernels.hip fails the file: ST_SQRT2 -> 1.0 (every Gamma case with a pair, real
mode on), rotate_minus_i_pow(pc.l + 2, ...) and v[3] / v[4] of k_st_kinetic swapped (every block case with a row other than
G = 0), the unpaired-Nyquist condition removed (every cube with an even axis), the n_spin == 2 addend removed (every
two-component case), 4.0 * 3.14159265 in the Hartree term (every cube).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd import psp as lpsp  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402
from dftk_jl_amd.terms import (build_projection_coefficients, local_species_tables,  # noqa: E402
                               projector_species_tables)

import stress_ref as sr  # noqa: E402
from test_gpu_kernels import Basis, KBlock  # noqa: E402
from test_hgh_channels import synthetic_library_psp  # noqa: E402

TOL = 1e-12
DEV = "cuda:0"
PAD = 7
LD = np.longdouble


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


def _elements():
    return {"X": dftk.ElementPsp("Si", synthetic_library_psp()), "Fe": dftk.ElementPsp("Fe", lpsp.load_psp("Fe", "lda")),
            "Si": dftk.ElementPsp("Si", lpsp.load_psp("Si", "lda"))}


def _model(names):
    el = _elements()
    return dftk.model_DFT(sr.LATTICE, [el[n.rstrip("12")] for n in names], [np.array(sr.POS[n]) for n in names])


def held(name, case, got, ref, S, base=None):
    """|got - base - ref| <= TOL S in long double; exact where S = 0.  Prints the measured error / S."""
    diff = np.abs(np.asarray(got, dtype=LD) - (0 if base is None else np.asarray(base, dtype=LD)) - ref)
    S = np.asarray(S, dtype=LD)
    assert np.all(np.isfinite(np.asarray(got, dtype=float))), (name, case, got)
    assert np.all(diff[S == 0] == 0), (name, case, got)
    rel = float(np.max(diff[S > 0] / S[S > 0])) if np.any(S > 0) else 0.0
    print(f"\n{name} {case}: max |device - reference| / S = {rel:.3e}")
    assert rel <= TOL, (name, case, (diff / np.where(S > 0, S, 1)).astype(float))
    return rel


# ------------------------------------------------------------------------------------------ kinetic + nonlocal
class Block:
    """Raw handles of one sphere: the basis, the k-block with the HGH projectors of the four atoms bound."""

    def __init__(self, lib, mapping, G, kpt):
        self.lib = lib
        model = _model(("X1", "X2", "Fe", "Si"))
        assert model.atom_groups == [[0, 1], [2], [3]]
        recip, self.vol = sr.lattice_tables()
        assert np.array_equal(model.recip_lattice, recip) and model.unit_cell_volume == self.vol
        self.B = np.asfortranarray(recip, dtype=np.float64)
        self.kpt = np.ascontiguousarray(kpt, dtype=np.float64)
        self.n = len(mapping)
        self.bs = Basis(lib, *sr.NL_FFT, self.vol)
        self.kb = KBlock(lib, self.bs, mapping, np.zeros(self.n))
        (self.n_psp, self.rp, self.nproj, self.species, self.pos, self.col_start) = projector_species_tables(model)
        assert list(self.col_start) == [0, 29, 58, 72, 77]
        assert np.array_equal(self.pos, np.array([r for _, r in sr.nonlocal_atoms()]))
        self.n_p = 77
        self.D = np.asfortranarray(build_projection_coefficients(model))
        G32 = torch.from_numpy(np.ascontiguousarray(G, dtype=np.int32)).to(DEV)
        n_p = C.c_int()
        self.P = torch.empty((self.n_p, self.n), dtype=torch.complex128, device=DEV)
        check(lib.dftk_mi_build_projectors_hgh(self.bs.h, self.n, G32.data_ptr(), self.B.ctypes.data, self.kpt.ctypes.data,
                                               self.vol, self.n_psp, self.rp.ctypes.data, self.nproj.ctypes.data,
                                               len(self.species), self.species.ctypes.data, self.pos.ctypes.data,
                                               self.P.data_ptr(), self.n, C.byref(n_p)))
        self.bs.sync()
        assert n_p.value == self.n_p
        check(lib.dftk_mi_kblock_set_projectors(self.kb.h, self.n_p, self.P.data_ptr(), self.n, self.D.ctypes.data))

    def gamma_real(self, on):
        check(self.lib.dftk_mi_kblock_set_gamma_real(self.kb.h, int(on)))

    def stress(self, psi, w, prefill):
        """psi: (n_G, nb) numpy; the entry on a (nb, n_G + PAD) block with NaN padding, accumulated onto ``prefill``"""
        nb = psi.shape[1]
        buf = torch.full((nb, self.n + PAD), float("nan"), dtype=torch.complex128, device=DEV)
        buf[:, :self.n] = torch.from_numpy(np.ascontiguousarray(psi.T)).to(DEV)
        out = np.array(prefill, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        check(self.lib.dftk_mi_stress_kinetic_nonlocal(
            self.kb.h, self.B.ctypes.data, self.kpt.ctypes.data, nb, buf.data_ptr(), buf.stride(0), w.ctypes.data,
            self.n_psp, self.rp.ctypes.data, self.nproj.ctypes.data, len(self.species), self.species.ctypes.data,
            self.pos.ctypes.data, self.col_start.ctypes.data, out.ctypes.data))
        return out


PREFILL = np.array([0.75, -1.25, 2.5, -0.375, 1.125, -3.0, 0.625, 1.75, -0.875, 2.25, -1.5, 0.3125])

_BLOCKS = {}


def block(lib, gamma, n):
    if (gamma, n) not in _BLOCKS:
        mapping, G = sr.nonlocal_case(n, 1, gamma)[:2]
        _BLOCKS[gamma, n] = Block(lib, mapping, G, np.zeros(3) if gamma else sr.KPT)
    return _BLOCKS[gamma, n]


def check_kinetic_nonlocal(blk, case, psi, w, ref):
    got = blk.stress(psi, w, PREFILL)
    assert np.array_equal(got, blk.stress(psi, w, PREFILL)), case          # bitwise reproducible
    rk = held("kinetic", case, got[:6], ref["value"][:6], ref["S"][:6], PREFILL[:6])
    rn = held("nonlocal", case, got[6:], ref["value"][6:], ref["S"][6:], PREFILL[6:])
    return rk, rn


@pytest.mark.parametrize("nb", sr.NBANDS)
@pytest.mark.parametrize("n_G", sr.NG_COMPLEX)
def test_complex_block_against_the_strained_energy(lib, n_G, nb):
    mapping, G, psi, w, ref = sr.nonlocal_case(n_G, nb, False)
    assert len(mapping) == n_G and (nb < 2 or np.count_nonzero(w == 0) == 1)
    check_kinetic_nonlocal(block(lib, False, n_G), f"complex n_G={n_G} nb={nb}", psi, w, ref)


@pytest.mark.parametrize("nb", sr.NBANDS)
@pytest.mark.parametrize("n_half", sr.NHALF_GAMMA)
def test_gamma_block_real_mode_off_and_on_against_the_strained_energy(lib, n_half, nb):
    mapping, G, psi, w, ref = sr.nonlocal_case(n_half, nb, True)
    assert len(mapping) == 2 * n_half - 1 and tuple(G[0]) == (0, 0, 0)
    blk = block(lib, True, n_half)
    try:
        for on in (False, True):
            blk.gamma_real(on)
            check_kinetic_nonlocal(blk, f"gamma n_half={n_half} nb={nb} real={on}", psi, w, ref)
    finally:
        blk.gamma_real(False)


def chunking(budget, rows, gamma, nb, col_start):
    """The two budget formulas of stress_kinetic_nonlocal restated: (cc_max, band chunk, the column chunks as atom lists)"""
    n_p = int(col_start[-1])
    widths = np.diff(col_start)
    cc_max = min(n_p, max(int(widths.max()), budget // (6 * rows * 16)))
    per_band = ((rows if gamma else 0) + n_p + 6 * cc_max) * 16
    cb = max(1, min(nb, budget // per_band))
    chunks, a0 = [], 0
    while a0 < len(widths):
        a1 = a0
        while a1 < len(widths) and col_start[a1 + 1] - col_start[a0] <= cc_max:
            a1 += 1
        chunks.append(list(range(a0, a1)))
        a0 = a1
    return cc_max, cb, chunks


@pytest.mark.parametrize("gamma", [False, True])
def test_column_and_band_chunks_against_the_strained_energy(lib, gamma, monkeypatch):
    """n_G = 257 / n_half = 129, three bands, three budgets: each case held to the reference, not only to the others"""
    n, nb = (129, 3) if gamma else (257, 3)
    mapping, G, psi, w, ref = sr.nonlocal_case(n, nb, gamma)
    blk = block(lib, gamma, n)
    rows = n
    col_start = blk.col_start

    def kib_with(pred):
        return next(k for k in range(1, 1 << 14) if pred(*chunking(k << 10, rows, gamma, nb, col_start)))
    budgets = {"one chunk": kib_with(lambda cc, cb, ch: ch == [[0, 1, 2, 3]] and cb == nb),
               "two column chunks": kib_with(lambda cc, cb, ch: 58 <= cc <= 76 and cb == nb),
               "three column chunks, two band chunks": kib_with(lambda cc, cb, ch: cc == 29 and cb == 2)}
    assert chunking(budgets["two column chunks"] << 10, rows, gamma, nb, col_start)[2] == [[0, 1], [2, 3]]
    assert chunking(budgets["three column chunks, two band chunks"] << 10, rows, gamma, nb, col_start)[2] == [[0], [1], [2, 3]]
    try:
        blk.gamma_real(gamma)
        for name, kib in budgets.items():
            monkeypatch.setenv("DFTK_MI_STRESS_WS_KIB", str(kib))
            check_kinetic_nonlocal(blk, f"{'gamma' if gamma else 'complex'} n={n} {name} ({kib} KiB)", psi, w, ref)
    finally:
        blk.gamma_real(False)


# ------------------------------------------------------------------------------------------ cube
def test_cubes_cover_the_parities_the_tile_and_the_second_rowsum_trip():
    sizes = [nx * ny * nz for nx, ny, nz in sr.CUBES]
    assert {sum(n % 2 == 0 for n in c) for c in sr.CUBES} == {0, 1, 2, 3}          # all-odd, one, two, three even axes
    for axis in range(3):
        assert {c[axis] % 2 for c in sr.CUBES} == {0, 1}
    assert any(N < 256 for N in sizes) and any(N % 256 == 0 for N in sizes) and any(N > 256 and N % 256 for N in sizes)
    assert max(-(-N // 256) for N in sizes) == 270 > 256                          # k_rowsum strides over the partial sums


@pytest.mark.parametrize("atom_set", sr.ATOM_SETS)
@pytest.mark.parametrize("fft_size", sr.CUBES, ids=sr.cube_id)
def test_cube_entry_against_the_strained_energy(lib, fft_size, atom_set):
    rho, ref = sr.cube_case(fft_size, atom_set)
    nx, ny, nz = fft_size
    N = nx * ny * nz
    recip, vol = sr.lattice_tables()
    B = np.asfortranarray(recip, dtype=np.float64)
    names = {"none": ("X1", "X2", "Fe", "Si"), "one": ("X1",), "three": ("X1", "X2", "Fe", "Si")}[atom_set]
    par, species, pos = local_species_tables(_model(names))
    n_atoms = 0 if atom_set == "none" else len(species)
    if atom_set == "three":
        assert list(species) == [0, 0, 1, 2] and np.all(par[0, 2:6] != 0) and np.all(par[1, 2:6] == 0)
    bs = Basis(lib, nx, ny, nz, vol)
    cube = KBlock(lib, bs, np.arange(N), np.zeros(N))
    rho_d = torch.from_numpy(np.ascontiguousarray(rho.reshape(-1))).to(DEV)

    def call():
        out = np.full(14, np.nan)
        check(lib.dftk_mi_stress_cube(cube.h, B.ctypes.data, par.shape[0], par.ctypes.data, n_atoms, species.ctypes.data,
                                      pos.ctypes.data, rho_d.data_ptr(), out.ctypes.data))
        return out
    got = call()
    assert np.array_equal(got, call())
    held("cube", f"{fft_size} atoms={atom_set}", got, ref["value"], ref["S"])
    if atom_set == "none":
        assert np.all(got[:6] == 0) and got[12] == 0


# ------------------------------------------------------------------------------------------ xc
@pytest.mark.parametrize("variant", sr.XC_VARIANTS)
@pytest.mark.parametrize("n", sr.XC_N)
def test_xc_entry_against_the_exact_sums(lib, n, variant):
    d = sr.xc_inputs(n, variant)
    value, S = sr.xc(**d)
    bs = Basis(lib, 4, 4, 4)
    t = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else None) for k, v in d.items()}

    def ptr(k):
        return t[k].data_ptr() if t[k] is not None else None

    def call():
        out = np.full(8, np.nan)
        check(lib.dftk_mi_stress_xc(bs.h, n, d["n_spin"], ptr("rho"), ptr("vrho"), ptr("e"), ptr("vsigma"), ptr("grad"),
                                    out.ctypes.data))
        return out
    got = call()
    assert np.array_equal(got, call())
    held("xc", f"n={n} {variant}", got, value, S)
    if variant != "gga":
        assert got[0] == 0 and np.all(got[2:] == 0)                    # the outputs the header says are 0
