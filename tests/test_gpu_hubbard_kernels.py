"""csrc/hubbard_kernels.hip at the ABI: ``dftk_mi_hubbard_occupation`` and ``dftk_mi_hubbard_rotate``.

Occupation matrices.  Reference: C = Phi' psi and n_b[m1, m2] = sum_n w_n C[p0 + m1, n] conj(C[p0 + m2, n]) formed in
``numpy.longdouble`` from the same inputs.  Bound per entry: the GEMM's error dC[p, n] = 8 n_rows 2^-52 |psi_n| |phi_p| (the
constant of tests/test_gpu_pdos_kernels.py for the same product) propagated through the product of two entries,
sum_n |w_n| (|C1| dC2 + |C2| dC1 + dC1 dC2), plus (n_bands + 4) 2^-52 sum_n |w_n| |C1| |C2| for the sum (at most n_bands
additions, in whatever order, and the roundings of one complex product), plus 2^-52 |n_0| for the one addition onto what
the buffer held before.  Blocks of 1, 3, 5 and 7 orbitals in one call, neither contiguous nor in order; leading dimensions
above n_rows; some weights zero.

Rotation.  Reference: the product formed in ``numpy.clongdouble``.  Bound per entry: gamma_k sum_m |Phi[r, m]| |V[m, j]| with
k = 2 s + 4 (s complex products of 4 real ones each, summed), gamma_k = k 2^-52 / (1 - k 2^-52).  Every test prints the
largest ratio of error to bound it measured."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402

from test_gpu_kernels import Basis  # noqa: E402
from test_gpu_pdos_kernels import to_dev  # noqa: E402

U = 2.0 ** -52
EINVAL = -1
N_PROJ = 24
FIRST = np.array([17, 0, 9, 4], dtype=np.int32)          # columns 17-23, 0-2, 9-13, 4: gaps at 3, 5-8, 14-16
SIZE = np.array([7, 3, 5, 1], dtype=np.int32)
OFFSET = np.concatenate([[0], np.cumsum(SIZE.astype(np.int64) ** 2)])


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.fixture(scope="module")
def bs(lib):
    return Basis(lib, 8, 8, 8)


def case(n_rows, n_bands, seed=0):
    rng = np.random.default_rng(7919 * n_rows + n_bands + seed)
    Phi = rng.standard_normal((n_rows, N_PROJ)) + 1j * rng.standard_normal((n_rows, N_PROJ))
    Phi *= 10.0 ** rng.uniform(-1, 1, N_PROJ)[None, :] / np.sqrt(n_rows)
    psi = (rng.standard_normal((n_rows, n_bands)) + 1j * rng.standard_normal((n_rows, n_bands))) / np.sqrt(n_rows)
    w = rng.uniform(0.0, 0.5, n_bands)
    w[rng.random(n_bands) < 0.25] = 0.0
    if n_bands > 2:
        w[1] = 0.0
    return Phi, psi, w


def unpack(flat):
    """the packed column-major blocks as a list of s x s matrices"""
    return [flat[OFFSET[b]:OFFSET[b + 1]].reshape(SIZE[b], SIZE[b]).T for b in range(len(SIZE))]


def pack(blocks):
    return np.concatenate([np.asarray(B).T.reshape(-1) for B in blocks])


def run_occupation(lib, bs, Phi, psi, w, n0=None, ld_extra=0, first=FIRST, size=SIZE):
    n_rows = Phi.shape[0]
    Pd, Xd = to_dev(Phi, n_rows + ld_extra), to_dev(psi, n_rows + ld_extra)
    total = int(np.sum(size.astype(np.int64) ** 2))
    n_d = torch.from_numpy(np.zeros(total, dtype=complex) if n0 is None else n0.copy()).cuda()
    w = np.ascontiguousarray(w, dtype=np.float64)
    st = lib.dftk_mi_hubbard_occupation(bs.h, n_rows, psi.shape[1], Xd.data_ptr(), Xd.stride(0), Phi.shape[1], Pd.data_ptr(),
                                        Pd.stride(0), w.ctypes.data, len(first), first.ctypes.data, size.ctypes.data,
                                        n_d.data_ptr())
    bs.sync()
    torch.cuda.synchronize()
    return st, n_d.cpu().numpy()


def occupation_reference(Phi, psi, w):
    """(blocks in long double rounded to complex128, the bound per entry without the n_0 term)"""
    ld = np.clongdouble
    Cm = Phi.astype(ld).conj().T @ psi.astype(ld)                                       # (n_proj, n_bands)
    absC = np.abs(Cm).astype(float)
    dC = 8 * Phi.shape[0] * U * np.linalg.norm(Phi, axis=0)[:, None] * np.linalg.norm(psi, axis=0)[None, :]
    aw = np.abs(w)
    blocks, bounds = [], []
    for p0, s in zip(FIRST, SIZE):
        c, a, d = Cm[p0:p0 + s], absC[p0:p0 + s], dC[p0:p0 + s]
        blocks.append(((c * w.astype(np.longdouble)[None, :]) @ c.conj().T).astype(complex))
        prop = (a * aw) @ d.T + (d * aw) @ a.T + (d * aw) @ d.T
        bounds.append(prop + (psi.shape[1] + 4) * U * ((a * aw) @ a.T))
    return blocks, bounds


@pytest.mark.parametrize("n_bands", [1, 63, 64, 65, 257])
def test_occupation_against_long_double(lib, bs, n_bands):
    n_rows = 263
    Phi, psi, w = case(n_rows, n_bands)
    assert n_bands == 1 or np.any(w == 0)
    want, bound = occupation_reference(Phi, psi, w)
    st, flat = run_occupation(lib, bs, Phi, psi, w, ld_extra=3)
    assert st == 0, lib.dftk_mi_last_error()
    ratio = max(np.max(np.abs(g - r) / np.maximum(b, 1e-300)) for g, r, b in zip(unpack(flat), want, bound))
    print(f"n_bands {n_bands}: occupation error / bound = {ratio:.2e}")
    assert ratio <= 1
    for g in unpack(flat):                                                              # Hermitian up to the same bound
        assert np.all(np.abs(np.diag(g).imag) <= 1e-300 + 4 * U * np.abs(np.diag(g).real))
    # accumulation onto what the buffer holds
    rng = np.random.default_rng(n_bands)
    n0 = rng.standard_normal(len(flat)) + 1j * rng.standard_normal(len(flat))
    st, acc = run_occupation(lib, bs, Phi, psi, w, n0=n0, ld_extra=3)
    assert st == 0
    ratio = max(np.max(np.abs(g - (r + z)) / (b + U * np.abs(z)))
                for g, r, b, z in zip(unpack(acc), want, bound, unpack(n0)))
    print(f"n_bands {n_bands}: accumulated error / bound = {ratio:.2e}")
    assert ratio <= 1


def test_occupation_reproduces_bit_for_bit(lib, bs):
    Phi, psi, w = case(263, 257)
    _, once = run_occupation(lib, bs, Phi, psi, w)
    _, again = run_occupation(lib, bs, Phi, psi, w, ld_extra=5)
    assert np.array_equal(once, again) and np.any(once != 0)
    _, twice = run_occupation(lib, bs, Phi, psi, w, n0=once)
    assert np.array_equal(twice, 2 * once)                                              # x + x is exact
    # one block alone gives the numbers it has among the others
    _, alone = run_occupation(lib, bs, Phi, psi, w, first=FIRST[2:3], size=SIZE[2:3])
    assert np.array_equal(alone, once[OFFSET[2]:OFFSET[3]])
    # a weight of zero is a band left out
    keep = w != 0
    _, fewer = run_occupation(lib, bs, Phi, psi[:, keep], w[keep])
    want, bound = occupation_reference(Phi, psi, w)
    assert all(np.all(np.abs(g - r) <= b) for g, r, b in zip(unpack(fewer), want, bound))


def test_occupation_einval_leaves_the_output_untouched(lib, bs):
    Phi, psi, w = case(101, 7)
    Pd, Xd = to_dev(Phi), to_dev(psi)
    n_d = torch.full((int(OFFSET[-1]),), 5.0 + 0j, dtype=torch.complex128, device="cuda")
    good = dict(h=bs.h, n_rows=101, n_bands=7, ld_psi=101, n_proj=N_PROJ, ld_phi=101, n_blocks=4, first=FIRST, size=SIZE,
                psi=Xd.data_ptr(), phi=Pd.data_ptr(), w=w.ctypes.data, out=n_d.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.dftk_mi_hubbard_occupation(a["h"], a["n_rows"], a["n_bands"], a["psi"], a["ld_psi"], a["n_proj"], a["phi"],
                                              a["ld_phi"], a["w"], a["n_blocks"], a["first"].ctypes.data,
                                              a["size"].ctypes.data, a["out"])
    i32 = lambda *v: np.array(v, dtype=np.int32)                                        # noqa: E731
    for bad in (dict(n_rows=0), dict(n_bands=0), dict(n_proj=0), dict(n_blocks=0), dict(ld_psi=100), dict(ld_phi=100),
                dict(first=i32(17, 0, 9, -1)), dict(first=i32(18, 0, 9, 4)), dict(first=i32(17, 0, 9, 24)),
                dict(size=i32(7, 3, 5, 0)), dict(size=i32(7, 3, 5, 8), first=i32(17, 0, 9, 2)), dict(n_proj=23),
                dict(h=None), dict(psi=None), dict(phi=None), dict(w=None), dict(out=None)):
        assert call(**bad) == EINVAL, bad
    bs.sync()
    torch.cuda.synchronize()
    assert torch.all(n_d == 5.0)
    assert b"block" in lib.dftk_mi_last_error() or b"hubbard_occupation" in lib.dftk_mi_last_error()
    assert call() == 0                                                                  # the good call goes through
    bs.sync()
    assert not torch.any(n_d == 5.0)


# ------------------------------------------------------------------------------------------------ rotation
def rotation_matrices(seed, real=False):
    rng = np.random.default_rng(seed)
    out = []
    for s in SIZE:
        A = rng.standard_normal((s, s)) + (0 if real else 1j) * rng.standard_normal((s, s))
        out.append(np.linalg.qr(A)[0].astype(complex))
    return out


def run_rotate(lib, bs, Phi, V, ld_extra=0, first=FIRST, size=SIZE):
    n_rows = Phi.shape[0]
    Pd = to_dev(Phi, n_rows + ld_extra)
    Out = torch.full((Phi.shape[1], n_rows + ld_extra + 2), 9.0 + 0j, dtype=torch.complex128, device="cuda")
    Vh = np.ascontiguousarray(pack(V), dtype=np.complex128)
    st = lib.dftk_mi_hubbard_rotate(bs.h, n_rows, len(first), first.ctypes.data, size.ctypes.data, Pd.data_ptr(), Pd.stride(0),
                                    Vh.ctypes.data, Out.data_ptr(), Out.stride(0))
    bs.sync()
    torch.cuda.synchronize()
    return st, Out.cpu().numpy().T                                                       # (ld_out, n_proj)


@pytest.mark.parametrize("n_rows", [1, 255, 256, 257, 1031])
def test_rotate_against_numpy(lib, bs, n_rows):
    Phi, _, _ = case(n_rows, 3)
    V = rotation_matrices(n_rows)
    st, out = run_rotate(lib, bs, Phi, V, ld_extra=3)
    assert st == 0, lib.dftk_mi_last_error()
    touched = np.zeros(N_PROJ, dtype=bool)
    worst = 0.0
    for p0, s, Vb in zip(FIRST, SIZE, V):
        k = 2 * s + 4
        gamma = k * U / (1 - k * U)
        want = Phi[:, p0:p0 + s].astype(np.clongdouble) @ Vb.astype(np.clongdouble)
        bound = gamma * (np.abs(Phi[:, p0:p0 + s]) @ np.abs(Vb))
        worst = max(worst, float(np.max(np.abs(out[:n_rows, p0:p0 + s] - want) / bound)))
        touched[p0:p0 + s] = True
    print(f"n_rows {n_rows}: rotation error / bound = {worst:.2e}")
    assert worst <= 1
    assert np.all(out[n_rows:] == 9.0) and np.all(out[:, ~touched] == 9.0)             # padding rows, columns of no block
    # a real rotation of real columns stays real
    Vr = rotation_matrices(n_rows + 1, real=True)
    st, out = run_rotate(lib, bs, Phi.real.astype(complex), Vr)
    assert st == 0 and np.all(out[:n_rows][:, touched].imag == 0)


def test_rotate_einval_leaves_the_output_untouched(lib, bs):
    Phi, _, _ = case(101, 3)
    Pd = to_dev(Phi)
    Out = torch.full((N_PROJ, 101), 9.0 + 0j, dtype=torch.complex128, device="cuda")
    Vh = np.ascontiguousarray(pack(rotation_matrices(0)), dtype=np.complex128)
    good = dict(h=bs.h, n_rows=101, n_blocks=4, first=FIRST, size=SIZE, phi=Pd.data_ptr(), ld_phi=101, V=Vh.ctypes.data,
                out=Out.data_ptr(), ld_out=101)

    def call(**kw):
        a = dict(good, **kw)
        return lib.dftk_mi_hubbard_rotate(a["h"], a["n_rows"], a["n_blocks"], a["first"].ctypes.data, a["size"].ctypes.data,
                                          a["phi"], a["ld_phi"], a["V"], a["out"], a["ld_out"])
    i32 = lambda *v: np.array(v, dtype=np.int32)                                        # noqa: E731
    for bad in (dict(n_rows=0), dict(n_blocks=0), dict(ld_phi=100), dict(ld_out=100), dict(first=i32(17, 0, 9, -1)),
                dict(size=i32(7, 3, 5, 0)), dict(size=i32(8, 3, 5, 1)), dict(h=None), dict(phi=None), dict(V=None),
                dict(first=i32(17, 0, 2, 4)), dict(first=i32(17, 0, 9, 13)), dict(first=i32(17, 17, 9, 4)),   # shared columns
                dict(out=None), dict(out=Pd.data_ptr()), dict(out=Pd.data_ptr() + 16 * 101 * 5)):
        assert call(**bad) == EINVAL, bad
    bs.sync()
    torch.cuda.synchronize()
    assert torch.all(Out == 9.0) and np.array_equal(Pd.cpu().numpy().T, Phi)
    assert call() == 0
    bs.sync()
    assert not torch.any(Out[17:] == 9.0)
