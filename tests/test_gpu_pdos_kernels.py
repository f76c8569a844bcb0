"""csrc/pdos_kernels.hip at the ABI: ``dftk_mi_lowdin_ortho`` and ``dftk_mi_pdos_accumulate``.

Loewdin.  Reference: a 50-digit mpmath Loewdin (Gram matrix, Hermitian eigen-decomposition, S^-1/2, product) of the same
Phi for n_cols <= 8, the NumPy twin (tests/pswfc_gen.py: numpy.linalg.eigh) for n_cols = 18.  Tolerance, relative to
max |Phi~|: the twin's own error against mpmath is measured first, on the CPU, and the device gets 8 x that (the factor
covers the different summation order of the n_rows-long dot products), with the floor n_cols 2^-52 sqrt(cond(S)).  Where the
twin itself is the reference (n_cols = 18) both sides carry such an error: twice the bound, with the twin's error taken from
the n_cols = 8 case of the same n_rows, plus 8 x the twin's own orthonormality defect in the distance to it (the part of the
reference's error that can be measured without a better reference; it is 1e-6 ... 2e-5 and moves with the BLAS thread
count).  |Phi~' Phi~ - I|_max of the device gets the bound without that last term.

Measured on the CPU (twin against mpmath, relative to max |Phi~|; columns with norms spread over 1e-3 ... 1e3, so cond(S) is
about 1e12 for more than one column; LAPACK's eigh loses the small eigenvalues of such a graded matrix, hence the 8-column
figures):
    n_rows x n_cols    1x1      7x1      7x2      257x1    257x2    257x8    1031x1   1031x2   1031x8   cond1e8 257x8
    twin error         0        1.8e-16  1.2e-16  1.7e-16  3.7e-16  7.6e-07  1.6e-16  4.4e-16  2.4e-06  4.1e-10
    floor              2.2e-16  2.2e-16  3.4e-10  2.2e-16  4.1e-10  1.7e-09  2.2e-16  4.6e-10  1.7e-09  1.8e-11
    device (MI355X)    2.8e-17  2.2e-16  1.7e-16  1.8e-16  2.3e-16  1.2e-09  2.0e-16  4.1e-16  2.5e-13  4.9e-10
The 18-column cases against the twin: 7.5e-06 (257 rows, bound 1.6e-04) and 3.3e-07 (1031 rows, bound 4.6e-05), with
|Phi~' Phi~ - I| of 4.2e-15 and 1.0e-10: what is measured there is the twin.  (``test_lowdin_against_mpmath`` prints all of them.)

PDOS accumulation.  Reference: the twin's loops.  Bound per entry: 16 x 2^-52 x weight sum_n |g| |C_pn|^2 -- a plain sum of
n_bands terms that both smearing kinds keep non-negative -- plus the propagated bound of |C|^2 where the device's own
projections enter.  ``proj_d`` against abs(C)**2 of a float64 NumPy product: 8 n_rows 2^-52 |phi_p| |psi_n| per entry of C,
i.e. 2 |C| dC + dC^2 for |C|^2.  Every test prints the largest ratio of error to bound it measured.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd.mixing import occupation_derivative  # noqa: E402

import pswfc_gen  # noqa: E402
from test_gpu_kernels import Basis  # noqa: E402

U = 2.0 ** -52
EINVAL, RANK_DEFICIENT = -1, 6
FERMI_DIRAC, GAUSSIAN = 1, 2
KIND_NAME = {FERMI_DIRAC: "fermi_dirac", GAUSSIAN: "gaussian"}
LOWDIN_SHAPES = [(1, 1), (7, 1), (7, 2), (257, 1), (257, 2), (257, 8), (257, 18), (1031, 1), (1031, 2), (1031, 8), (1031, 18)]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs(lib):
    return Basis(lib, 8, 8, 8)


def to_dev(A, ld=None, fill=np.nan):
    """n x m host matrix -> (m, ld) device tensor == column-major with leading dimension ld, padding rows = fill"""
    n, m = A.shape
    ld = n if ld is None else ld
    buf = np.full((m, ld), fill, dtype=A.dtype)
    buf[:, :n] = A.T
    return torch.from_numpy(buf).cuda()


# ------------------------------------------------------------------------------------------------ Loewdin
def spread_columns(n_rows, n_cols, seed=0):
    rng = np.random.default_rng(1000 * n_rows + n_cols + seed)
    Phi = rng.standard_normal((n_rows, n_cols)) + 1j * rng.standard_normal((n_rows, n_cols))
    scale = 10.0 ** np.linspace(-3, 3, n_cols) if n_cols > 1 else np.array([10.0 ** rng.uniform(-3, 3)])
    return Phi * rng.permutation(scale)[None, :]


def conditioned(n_rows, n_cols, cond_S, seed=0):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.standard_normal((n_rows, n_cols)) + 1j * rng.standard_normal((n_rows, n_cols)))[0]
    W = np.linalg.qr(rng.standard_normal((n_cols, n_cols)) + 1j * rng.standard_normal((n_cols, n_cols)))[0]
    return (Q * np.sqrt(cond_S) ** -np.linspace(0, 1, n_cols)[None, :]) @ W.conj().T


def mp_lowdin(Phi):
    """Loewdin with 50 digits: returns (Phi~ rounded to complex128, eigenvalues of S as floats)."""
    import mpmath as mp
    with mp.workdps(50):
        n, m = Phi.shape
        cols = [[mp.mpc(float(z.real), float(z.imag)) for z in Phi[:, j]] for j in range(m)]
        S = mp.matrix(m, m)
        for i in range(m):
            for j in range(i, m):
                S[i, j] = mp.fdot(cols[j], cols[i], conjugate=True)       # sum conj(phi_i) phi_j
                S[j, i] = mp.conj(S[i, j])
        w, V = mp.eigh(S)
        M = mp.matrix(m, m)
        for i in range(m):
            for j in range(m):
                M[i, j] = mp.fsum(V[i, k] * mp.conj(V[j, k]) / mp.sqrt(w[k]) for k in range(m))
        out = np.empty((n, m), dtype=complex)
        Mcols = [[M[k, j] for k in range(m)] for j in range(m)]
        for r in range(n):
            row = [cols[k][r] for k in range(m)]
            for j in range(m):
                out[r, j] = complex(mp.fdot(row, Mcols[j]))
        return out, np.array([float(x) for x in w])


_REF = {}


def lowdin_reference(name, make):
    """(Phi, reference Phi~, eigenvalues, twin Phi~, twin error or None): computed once per case and shared"""
    if name not in _REF:
        Phi = make()
        twin, lam_twin = pswfc_gen.twin_lowdin(Phi)
        if Phi.shape[1] <= 8:
            ref, lam = mp_lowdin(Phi)
            e_twin = np.max(np.abs(twin - ref)) / np.max(np.abs(ref))
        else:
            ref, lam, e_twin = twin, lam_twin, None
        _REF[name] = (Phi, ref, lam, twin, e_twin)
    return _REF[name]


def lowdin_bound(n_rows, n_cols, lam, e_twin, twin=None):
    """relative to max |Phi~|.  ``twin``: the reference when it is the twin itself (18 columns); the bound on the distance to
    it then also carries the twin's own orthonormality defect, the one figure of its error that needs no better reference
    (LAPACK's eigh on these graded Gram matrices: 1e-6 ... 2e-5, and it moves with the BLAS thread count)."""
    floor = n_cols * U * np.sqrt(lam.max() / lam.min())
    if e_twin is None:      # the twin is the reference: its error is that of the 8-column case of the same n_rows
        e8 = lowdin_reference(f"spread-{n_rows}-8", lambda: spread_columns(n_rows, 8))[4]
        defect = 0.0 if twin is None else np.max(np.abs(twin.conj().T @ twin - np.eye(n_cols)))
        return 2 * max(8 * e8, floor) + 8 * defect
    return max(8 * e_twin, floor)


def run_lowdin(lib, bs, Phi, ld=None, want_evals=True):
    n, m = Phi.shape
    Pd = to_dev(Phi, ld, fill=7.0 - 3.0j)
    lam = np.full(m, np.nan)
    st = lib.dftk_mi_lowdin_ortho(bs.h, n, m, Pd.data_ptr(), Pd.stride(0), lam.ctypes.data if want_evals else None)
    bs.sync()
    return st, Pd, lam


@pytest.mark.parametrize("n_rows,n_cols", LOWDIN_SHAPES)
def test_lowdin_against_mpmath(lib, bs, n_rows, n_cols):
    Phi, ref, lam, _, e_twin = lowdin_reference(f"spread-{n_rows}-{n_cols}", lambda: spread_columns(n_rows, n_cols))
    st, Pd, lam_dev = run_lowdin(lib, bs, Phi)
    assert st == 0, lib.dftk_mi_last_error()
    got = Pd.cpu().numpy().T
    scale = np.max(np.abs(ref))
    bound = lowdin_bound(n_rows, n_cols, lam, e_twin)                          # (orthonormality: no reference involved)
    bound_ref = lowdin_bound(n_rows, n_cols, lam, e_twin, twin=ref if e_twin is None else None)
    err = np.max(np.abs(got - ref)) / scale
    orth = np.max(np.abs(got.conj().T @ got - np.eye(n_cols)))
    print(f"{n_rows}x{n_cols}: cond(S) {lam.max() / lam.min():.1e}, twin {e_twin if e_twin is None else f'{e_twin:.1e}'}, "
          f"device {err:.1e} (bound {bound_ref:.1e}), |Phi~'Phi~ - I| {orth:.1e} (bound {bound:.1e})")
    assert err <= bound_ref
    assert orth <= bound
    # evals_h against eigvalsh of the float64 Gram matrix, within its own conditioning: n_rows 2^-52 |S| absolute
    S = Phi.conj().T @ Phi
    np.testing.assert_allclose(lam_dev, np.linalg.eigvalsh((S + S.conj().T) / 2), rtol=0,
                               atol=8 * max(n_rows, 8) * U * np.linalg.norm(S, 2))
    assert np.all(np.diff(lam_dev) >= 0)


def test_lowdin_cond_1e8(lib, bs):
    Phi, ref, lam, _, e_twin = lowdin_reference("cond1e8", lambda: conditioned(257, 8, 1e8))
    assert 0.5e8 < lam.max() / lam.min() < 2e8
    st, Pd, _ = run_lowdin(lib, bs, Phi, want_evals=False)
    assert st == 0, lib.dftk_mi_last_error()
    got = Pd.cpu().numpy().T
    bound = lowdin_bound(257, 8, lam, e_twin)
    err = np.max(np.abs(got - ref)) / np.max(np.abs(ref))
    orth = np.max(np.abs(got.conj().T @ got - np.eye(8)))
    print(f"cond 1e8: twin {e_twin:.1e}, device {err:.1e}, |Phi~'Phi~ - I| {orth:.1e}, bound {bound:.1e}")
    assert err <= bound and orth <= bound


def test_lowdin_reproducible_and_padding(lib, bs):
    Phi = spread_columns(1031, 18)
    st1, P1, l1 = run_lowdin(lib, bs, Phi, ld=1031 + 5)
    st2, P2, l2 = run_lowdin(lib, bs, Phi, ld=1031 + 5)
    st3, P3, _ = run_lowdin(lib, bs, Phi)
    assert st1 == st2 == st3 == 0
    a, b = P1.cpu().numpy(), P2.cpu().numpy()
    assert np.array_equal(a.view(np.float64), b.view(np.float64)) and np.array_equal(l1, l2)
    assert np.all(a[:, 1031:] == 7.0 - 3.0j)                       # padding rows untouched
    # the leading dimension changes no value (the products are the same products)
    assert np.array_equal(a[:, :1031].view(np.float64).copy(), P3.cpu().numpy().view(np.float64))


def test_lowdin_dependent_columns_are_reported(lib, bs):
    Phi = spread_columns(257, 8)
    Phi[:, 5] = Phi[:, 2]
    st, Pd, lam = run_lowdin(lib, bs, Phi)
    msg = lib.dftk_mi_last_error().decode()
    print(st, msg)
    assert st == RANK_DEFICIENT
    assert "min |lambda| / max |lambda|" in msg and "e-" in msg
    assert np.array_equal(Pd.cpu().numpy().T, Phi)                 # untouched
    assert np.all(np.isfinite(lam)) and abs(lam[0]) <= U * lam[-1]


def test_lowdin_einval(lib, bs):
    Phi = spread_columns(7, 2)
    Pd = to_dev(Phi)
    before = Pd.clone()
    for args in [(7, 0, Pd.data_ptr(), 7), (7, -1, Pd.data_ptr(), 7), (1, 2, Pd.data_ptr(), 7), (7, 2, Pd.data_ptr(), 6),
                 (7, 2, None, 7)]:
        assert lib.dftk_mi_lowdin_ortho(bs.h, *args, None) == EINVAL, args
    assert lib.dftk_mi_lowdin_ortho(None, 7, 2, Pd.data_ptr(), 7, None) == EINVAL
    bs.sync()
    assert torch.equal(Pd, before)


# ------------------------------------------------------------------------------------------------ PDOS accumulation
def pdos_case(n_rows, n_bands, n_proj, n_eps, seed=0):
    rng = np.random.default_rng(seed + 7 * n_rows + 11 * n_bands + 13 * n_proj + 17 * n_eps)
    cplx = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)                      # noqa: E731
    Phi = np.linalg.qr(cplx(n_rows, n_proj))[0] if n_proj <= n_rows else cplx(n_rows, n_proj)
    psi = cplx(n_rows, n_bands) / np.sqrt(2 * n_rows)
    eig = np.sort(rng.uniform(-0.5, 0.5, n_bands))
    eps = np.linspace(-0.6, 0.6, n_eps) if n_eps > 1 else np.array([0.013])
    return Phi, psi, eig, eps


def run_pdos(lib, bs, Phi, psi, eig, eps, weight, kind, T, want_proj=True, pdos0=None, ld_extra=0, handle=None):
    n_rows, n_proj = Phi.shape
    n_bands = psi.shape[1]
    Pd, Xd = to_dev(Phi, n_rows + ld_extra), to_dev(psi, n_rows + ld_extra)
    proj = torch.full((n_bands, n_proj), np.nan, dtype=torch.float64, device="cuda") if want_proj else None
    pdos = None
    if pdos0 is not None:
        pdos = torch.from_numpy(np.ascontiguousarray(pdos0.T)).cuda()           # (n_proj, n_eps) == column-major n_eps x n_proj
    eig = np.ascontiguousarray(eig, dtype=np.float64)
    eps = np.ascontiguousarray(eps, dtype=np.float64)
    st = lib.dftk_mi_pdos_accumulate(handle or bs.h, n_rows, n_bands, Xd.data_ptr(), Xd.stride(0), n_proj, Pd.data_ptr(),
                                     Pd.stride(0), eig.ctypes.data, weight, kind, T, len(eps), eps.ctypes.data,
                                     None if proj is None else proj.data_ptr(), None if pdos is None else pdos.data_ptr())
    bs.sync()
    torch.cuda.synchronize()
    return st, (None if proj is None else proj.cpu().numpy()), (None if pdos is None else pdos.cpu().numpy().T.copy())


def g_matrix(kind, eps, eig, T):
    """g[e, n] = -occupation_derivative((eig_n - eps_e) / T) / T"""
    return -occupation_derivative(KIND_NAME[kind], (eig[None, :] - eps[:, None]) / T) / T


@pytest.mark.parametrize("n_proj", [1, 4, 8, 33])
@pytest.mark.parametrize("n_bands", [1, 7, 40])
def test_projections(lib, bs, n_proj, n_bands):
    n_rows = 263
    Phi, psi, eig, eps = pdos_case(n_rows, n_bands, n_proj, 1)
    st, proj, _ = run_pdos(lib, bs, Phi, psi, eig, eps, 1.0, 0, 0.0, ld_extra=3)        # (no pdos_d: kind / T are not read)
    assert st == 0, lib.dftk_mi_last_error()
    Cm = psi.conj().T @ Phi                                                             # (n_bands, n_proj)
    dC = 8 * n_rows * U * np.linalg.norm(psi, axis=0)[:, None] * np.linalg.norm(Phi, axis=0)[None, :]
    bound = 2 * np.abs(Cm) * dC + dC ** 2
    ratio = np.max(np.abs(proj - np.abs(Cm) ** 2) / bound)
    print(f"n_proj {n_proj}, n_bands {n_bands}: |C|^2 error / bound = {ratio:.2e}")
    assert ratio <= 1


@pytest.mark.parametrize("kind", [FERMI_DIRAC, GAUSSIAN], ids=["fermi_dirac", "gaussian"])
@pytest.mark.parametrize("n_eps", [1, 64, 257])
@pytest.mark.parametrize("n_proj,n_bands", [(1, 1), (4, 7), (8, 40), (33, 7), (33, 40), (8, 1)])
def test_pdos_against_the_twin(lib, bs, kind, n_eps, n_proj, n_bands):
    n_rows, T, weight = 101, 0.02, 2 * 0.125
    Phi, psi, eig, eps = pdos_case(n_rows, n_bands, n_proj, n_eps)
    st, proj, pdos = run_pdos(lib, bs, Phi, psi, eig, eps, weight, kind, T, pdos0=np.zeros((n_eps, n_proj)))
    assert st == 0, lib.dftk_mi_last_error()
    # the twin's loops on the DEVICE's projections: what is compared is the accumulation kernel
    twin = pswfc_gen.twin_pdos(eps, [proj], [eig], [0.125], [1], 2, KIND_NAME[kind], T)[:, :, 0]
    scale = weight * np.abs(g_matrix(kind, eps, eig, T)) @ proj                         # sum_n |g| |C|^2, (n_eps, n_proj)
    # far from every band g runs through the subnormal range before it underflows: there a term is exact to one spacing of
    # the format, 2^-1074 (times weight / T, the factors applied after the exponential), not to 2^-52 of itself
    bound = 16 * U * scale + 2 * n_bands * weight / T * 2.0 ** -1074
    err = np.abs(pdos - twin)
    ratio = np.max(err / bound)
    print(f"{KIND_NAME[kind]} n_eps {n_eps} n_proj {n_proj} n_bands {n_bands}: error / bound = {ratio:.2e}, "
          f"largest |error| {err.max():.2e}")
    assert np.all(err <= bound)


def test_pdos_accumulates_and_reproduces(lib, bs):
    Phi, psi, eig, eps = pdos_case(101, 40, 33, 257)
    zero = np.zeros((257, 33))
    _, _, once = run_pdos(lib, bs, Phi, psi, eig, eps, 0.5, GAUSSIAN, 0.02, pdos0=zero)
    _, _, again = run_pdos(lib, bs, Phi, psi, eig, eps, 0.5, GAUSSIAN, 0.02, pdos0=zero)
    assert np.array_equal(once, again) and np.any(once > 0)
    _, _, twice = run_pdos(lib, bs, Phi, psi, eig, eps, 0.5, GAUSSIAN, 0.02, pdos0=once)
    assert np.array_equal(twice, 2 * once)                                              # x + x is exact
    # without proj_d, and with a larger leading dimension: the same numbers
    _, p_none, alone = run_pdos(lib, bs, Phi, psi, eig, eps, 0.5, GAUSSIAN, 0.02, want_proj=False, pdos0=zero, ld_extra=9)
    assert p_none is None and np.array_equal(alone, once)


def test_fermi_dirac_far_from_the_level_is_exactly_zero(lib, bs):
    Phi, psi, _, _ = pdos_case(101, 7, 8, 1)
    T = 1e-3
    eig = np.array([0.8, -0.8] * 3 + [0.8])                        # (eig - eps) / T = +-800: exp(-800) underflows to 0
    assert np.all(np.abs(np.abs(eig / T) - 800) < 1e-9)
    for kind in (FERMI_DIRAC, GAUSSIAN):
        st, _, pdos = run_pdos(lib, bs, Phi, psi, eig, np.array([0.0]), 2.0, kind, T, pdos0=np.zeros((1, 8)))
        assert st == 0 and np.all(pdos == 0.0), pdos
    # one band at the energy, the others +-800 T away: the whole output is finite and is that band's term
    eig[3] = 0.0
    st, proj, pdos = run_pdos(lib, bs, Phi, psi, eig, np.array([0.0, 0.8, -0.8]), 2.0, FERMI_DIRAC, T, pdos0=np.zeros((3, 8)))
    assert st == 0 and np.all(np.isfinite(pdos))
    np.testing.assert_allclose(pdos[0], 2.0 * 0.25 / T * proj[3], rtol=4 * U)
    assert np.all(pdos[1] > 0) and np.all(pdos[2] > 0)


def test_gamma_real_basis_handle(lib):
    """a basis whose only k-block runs the Gamma-real iteration: blocks in the full-sphere complex layout are served"""
    lat, atoms, pos = dftk.silicon_cell()
    basis = dftk.PlaneWaveBasis(dftk.model_DFT(lat, atoms, pos), 5, dftk.ExplicitKpoints([[0, 0, 0]], [1.0]),
                                device="cuda:0", gamma_real=True)
    kpt = basis.kpoints[0]
    assert kpt.gamma_real
    Phi, psi, eig, eps = pdos_case(kpt.n_G, 7, 8, 64)

    class H:
        h = basis.handle

        @staticmethod
        def sync():
            basis.sync()
    st, proj, pdos = run_pdos(lib, H, Phi, psi, eig, eps, 2.0, GAUSSIAN, 0.02, pdos0=np.zeros((64, 8)))
    assert st == 0, lib.dftk_mi_last_error()
    want = np.abs(psi.conj().T @ Phi) ** 2
    np.testing.assert_allclose(proj, want, rtol=0, atol=64 * kpt.n_G * U * np.max(want) + 1e-300)
    twin = pswfc_gen.twin_pdos(eps, [proj], [eig], [1.0], [1], 2, "gaussian", 0.02)[:, :, 0]
    assert np.all(np.abs(pdos - twin) <= 16 * U * np.abs(twin) + 1e-300)


def test_pdos_einval_leaves_outputs_untouched(lib, bs):
    Phi, psi, eig, eps = pdos_case(101, 7, 8, 64)
    Pd, Xd = to_dev(Phi), to_dev(psi)
    proj = torch.full((7, 8), 5.0, dtype=torch.float64, device="cuda")
    pdos = torch.full((8, 64), 6.0, dtype=torch.float64, device="cuda")
    good = dict(n_rows=101, n_bands=7, ld_psi=101, n_proj=8, ld_phi=101, kind=GAUSSIAN, T=0.02, n_eps=64, proj=proj.data_ptr(),
                pdos=pdos.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.dftk_mi_pdos_accumulate(bs.h, a["n_rows"], a["n_bands"], Xd.data_ptr(), a["ld_psi"], a["n_proj"],
                                           Pd.data_ptr(), a["ld_phi"], eig.ctypes.data, 1.0, a["kind"], a["T"], a["n_eps"],
                                           eps.ctypes.data, a["proj"], a["pdos"])
    for bad in (dict(T=0.0), dict(T=-0.01), dict(T=float("nan")), dict(kind=0), dict(kind=3), dict(proj=None, pdos=None),
                dict(ld_psi=100), dict(ld_phi=100), dict(n_bands=0), dict(n_proj=0), dict(n_rows=0), dict(n_eps=0)):
        assert call(**bad) == EINVAL, bad
    bs.sync()
    torch.cuda.synchronize()
    assert torch.all(proj == 5.0) and torch.all(pdos == 6.0)
    assert call() == 0                                                                  # the good call goes through
    bs.sync()
    assert not torch.any(proj == 5.0)
