"""The one-launch Cholesky + inverse (``k_potrf_trtri_coop``, dense_kernels.hip) at the ABI, on the sizes where its panel
dataflow can go wrong: n = 33 (first size of the cooperative path), 47 / 48 / 49 and 64 / 65 (around a block-column
boundary of 16 and of 32), 259 and 503 (the Gram matrices of the 250-atom cell), 512 (the largest admitted size).

Inputs: G = X' X of seeded tall blocks X = Q diag(s) V' with singular values spread so that cond(G) = 1e2 and 1e10, for the
complex entry (``dftk_mi_potrf_trtri``, complex X) and the real one (``dftk_mi_potrf_trtri_real``); one indefinite
matrix per size and entry, which both entries must report as DFTK_MI_NUM_CHOLESKY (status 2: the drivers' shift-and-retry
of ``safe_cholesky`` hangs on that status).

Reference arithmetic: the residuals ``|R' R - G|_F / |G|_F`` and ``|R inv(R) - I|_F`` are evaluated in long double
(64-bit mantissa), so that what is measured is the error of the device results and not of the check.

Bounds: 8 x the figures of the kernel BEFORE the critical path of a panel step was shortened (factor of the diagonal
block in registers, one lane's fences per hand-off), measured on one MI355X on these very inputs and recorded in
``PARENT`` below as (residual of R, residual of inv(R)) per (entry, n, cond).  The change keeps every operation of the
factorisation and its order per entry; measured on the same device, R and inv(R) of all 36 cases came back bit for bit
equal to the earlier kernel's, i.e. the figures below are also the ones this test prints.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import dftk_jl_amd as dftk  # noqa: E402
from dftk_jl_amd._lib import check  # noqa: E402

SIZES = [33, 47, 48, 49, 64, 65, 259, 503, 512]
CONDS = [1e2, 1e10]
LD = np.longdouble

# (entry, n, cond) -> (|R'R - G|_F / |G|_F, |R inv(R) - I|_F) of the parent commit's kernel on one MI355X
PARENT = {
    ("real", 33, 1e02): (1.070e-16, 1.481e-15),
    ("real", 33, 1e10): (1.237e-16, 1.457e-11),
    ("real", 47, 1e02): (1.056e-16, 1.827e-15),
    ("real", 47, 1e10): (1.355e-16, 3.407e-11),
    ("real", 48, 1e02): (1.040e-16, 1.950e-15),
    ("real", 48, 1e10): (1.325e-16, 2.279e-11),
    ("real", 49, 1e02): (1.184e-16, 2.075e-15),
    ("real", 49, 1e10): (1.215e-16, 2.142e-11),
    ("real", 64, 1e02): (1.186e-16, 2.516e-15),
    ("real", 64, 1e10): (1.360e-16, 2.743e-11),
    ("real", 65, 1e02): (1.137e-16, 2.876e-15),
    ("real", 65, 1e10): (1.360e-16, 2.963e-11),
    ("real", 259, 1e02): (1.396e-16, 1.029e-14),
    ("real", 259, 1e10): (1.198e-16, 1.244e-10),
    ("real", 503, 1e02): (1.633e-16, 2.002e-14),
    ("real", 503, 1e10): (1.210e-16, 2.221e-10),
    ("real", 512, 1e02): (1.607e-16, 2.033e-14),
    ("real", 512, 1e10): (1.221e-16, 2.297e-10),
    ("complex", 33, 1e02): (1.147e-16, 1.763e-15),
    ("complex", 33, 1e10): (1.044e-16, 1.705e-11),
    ("complex", 47, 1e02): (1.220e-16, 2.006e-15),
    ("complex", 47, 1e10): (1.396e-16, 2.395e-11),
    ("complex", 48, 1e02): (1.213e-16, 2.255e-15),
    ("complex", 48, 1e10): (1.295e-16, 2.320e-11),
    ("complex", 49, 1e02): (1.262e-16, 2.187e-15),
    ("complex", 49, 1e10): (1.407e-16, 2.937e-11),
    ("complex", 64, 1e02): (1.205e-16, 2.828e-15),
    ("complex", 64, 1e10): (1.380e-16, 3.586e-11),
    ("complex", 65, 1e02): (1.247e-16, 2.930e-15),
    ("complex", 65, 1e10): (1.453e-16, 2.988e-11),
    ("complex", 259, 1e02): (1.448e-16, 1.052e-14),
    ("complex", 259, 1e10): (1.303e-16, 1.254e-10),
    ("complex", 503, 1e02): (1.641e-16, 2.026e-14),
    ("complex", 503, 1e10): (1.299e-16, 2.292e-10),
    ("complex", 512, 1e02): (1.673e-16, 2.064e-14),
    ("complex", 512, 1e10): (1.314e-16, 2.326e-10),
}


def gram(kind, n, cond):
    """G = X' X (fp64, exactly Hermitian / symmetric) of a seeded (3 n + 5) x n block with cond(G) = cond."""
    rng = np.random.default_rng([n, int(round(np.log10(cond))), int(kind == "complex")])
    cplx = kind == "complex"

    def rnd(r, c):
        return rng.standard_normal((r, c)) + (1j * rng.standard_normal((r, c)) if cplx else 0.0)

    Q, _ = np.linalg.qr(rnd(3 * n + 5, n))
    V, _ = np.linalg.qr(rnd(n, n))
    s = np.logspace(0.0, -0.5 * np.log10(cond), n)
    X = (Q * s) @ V.conj().T
    G = X.conj().T @ X
    G = 0.5 * (G + G.conj().T)
    return G.astype(complex)


def _parts(M):
    M = np.asarray(M)
    re = np.ascontiguousarray(M.real, dtype=LD)
    im = np.ascontiguousarray(M.imag, dtype=LD) if np.iscomplexobj(M) and np.any(M.imag) else None
    return re, im


def residuals(G, R, invR, blk=128):
    """(|R'R - G|_F / |G|_F, |R inv(R) - I|_F) in long double.  NumPy has no fast long-double product, so only the blocks
    that the triangular shapes leave non-zero are multiplied: R'R block (I, J >= I) sums over K <= I (the blocks below the
    diagonal count through their mirror images), R inv(R) block (I, J >= I) over I <= K <= J (its lower blocks are exact
    zeros)."""
    n = G.shape[0]
    Rr, Ri = _parts(R)
    Zr, Zi = _parts(invR)
    Gr, Gi = _parts(G)
    e = list(range(0, n, blk)) + [n]
    sl = [slice(e[i], e[i + 1]) for i in range(len(e) - 1)]
    zero = LD(0)
    s_r = s_g = s_i = zero
    for I, si in enumerate(sl):
        for J in range(I, len(sl)):
            sj = sl[J]
            w = 1 if I == J else 2
            re = -Gr[si, sj]
            im = -Gi[si, sj] if Gi is not None else None
            for K in range(I + 1):                       # (R'R)_IJ = sum_K conj(R_KI)' R_KJ
                sk = sl[K]
                re = re + Rr[sk, si].T @ Rr[sk, sj]
                if Ri is not None:
                    re = re + Ri[sk, si].T @ Ri[sk, sj]
                    t = Rr[sk, si].T @ Ri[sk, sj] - Ri[sk, si].T @ Rr[sk, sj]
                    im = t if im is None else im + t
            s_r += w * (np.sum(re * re) + (np.sum(im * im) if im is not None else zero))
            s_g += w * (np.sum(Gr[si, sj] ** 2) + (np.sum(Gi[si, sj] ** 2) if Gi is not None else zero))
            re = -np.eye(n, dtype=LD)[si, sj]
            im = None
            for K in range(I, J + 1):                    # (R Z)_IJ = sum_K R_IK Z_KJ
                sk = sl[K]
                re = re + Rr[si, sk] @ Zr[sk, sj]
                if Ri is not None or Zi is not None:
                    ri = Ri[si, sk] if Ri is not None else np.zeros((si.stop - si.start, sk.stop - sk.start), dtype=LD)
                    zi = Zi[sk, sj] if Zi is not None else np.zeros((sk.stop - sk.start, sj.stop - sj.start), dtype=LD)
                    re = re - ri @ zi
                    t = Rr[si, sk] @ zi + ri @ Zr[sk, sj]
                    im = t if im is None else im + t
            s_i += np.sum(re * re) + (np.sum(im * im) if im is not None else zero)
    return float(np.sqrt(s_r / s_g)), float(np.sqrt(s_i))


class Basis:
    def __init__(self, lib):
        self.lib = lib
        self.h = C.c_void_p()
        check(lib.dftk_mi_basis_create(8, 8, 8, 1.0, 0, C.byref(self.h)))

    def __del__(self):
        try:
            self.lib.dftk_mi_basis_destroy(self.h)
        except Exception:
            pass


def factor(lib, bs, kind, G):
    """status, R (upper), inv(R) of the entry `kind` on G; the strict lower triangle of the input and the whole of the
    inverse's buffer are NaN on entry (neither is read)."""
    n = G.shape[0]
    fn = lib.dftk_mi_potrf_trtri if kind == "complex" else lib.dftk_mi_potrf_trtri_real
    A = np.triu(G) + np.tril(np.full((n, n), complex(np.nan, np.nan)), -1)
    Ad = torch.from_numpy(np.ascontiguousarray(A.T)).cuda()      # column-major n x n
    Zd = torch.full_like(Ad, float("nan"))
    st = fn(bs.h, n, Ad.data_ptr(), n, Zd.data_ptr(), n)
    check(lib.dftk_mi_basis_sync(bs.h))
    return st, Ad.cpu().numpy().T, Zd.cpu().numpy().T


def measure(lib, bs, kind, n, cond):
    G = gram(kind, n, cond)
    st, A, invR = factor(lib, bs, kind, G)
    assert st == 0, (kind, n, cond, st)
    assert np.all(np.isnan(A[np.tril_indices(n, -1)])), "strict lower triangle of A written"
    R = np.triu(A)
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(invR))
    assert np.all(invR[np.tril_indices(n, -1)] == 0), "inv(R) is not upper triangular"
    if kind == "real":
        assert np.all(R.imag == 0) and np.all(invR.imag == 0)
    return residuals(G, R, invR), R, invR


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dftk.load_library()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_potrf_panels_within_8x_of_parent(lib, kind, n):
    bs = Basis(lib)
    for cond in CONDS:
        (e_r, e_i), _, _ = measure(lib, bs, kind, n, cond)
        p_r, p_i = PARENT[(kind, n, cond)]
        print(f"{kind} n={n} cond={cond:.0e}: |R'R-G|/|G| = {e_r:.3e} (parent {p_r:.3e}), "
              f"|R inv(R) - I| = {e_i:.3e} (parent {p_i:.3e})")
        assert e_r <= 8.0 * p_r, (kind, n, cond, e_r, p_r)
        assert e_i <= 8.0 * p_i, (kind, n, cond, e_i, p_i)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_potrf_panels_indefinite_input_is_reported(lib, kind, n):
    """G - 2 mean(diag G) I has negative pivots: status 2 (DFTK_MI_NUM_CHOLESKY), from either entry, and a positive
    definite matrix factors on the same handle right after (the drivers shift the diagonal and call again)."""
    bs = Basis(lib)
    G = gram(kind, n, 1e2)
    bad = G - 2.0 * np.trace(G).real / n * np.eye(n)
    st, _, _ = factor(lib, bs, kind, bad)
    assert st == 2, (kind, n, st)
    st, A, _ = factor(lib, bs, kind, G)
    assert st == 0
    R = np.triu(A)
    assert np.linalg.norm(R.conj().T @ R - G) <= 1e-13 * np.linalg.norm(G)
