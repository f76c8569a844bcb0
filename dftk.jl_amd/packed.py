"""What the orbital-space solvers (refine, direct_minimization, newton) share on the host: the block algebra on band-major
``(n_bands, n_G)`` complex128 CUDA blocks, and the base of the native handles over packed vectors (csrc/packed.h)."""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib


def zgemm(basis, kpt, trans, m, n, k, alpha, A, lda, B, ldb, beta, Cm, ldc):
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_zgemm(basis.lane_handles[kpt.lane], trans, m, n, k, _lib.cplx(alpha), A.data_ptr(), lda,
                                       B.data_ptr(), ldb, _lib.cplx(beta), Cm.data_ptr(), ldc))
    basis.post_call(kpt.lane)


def overlaps(basis, kpt, A, B):
    """A' B for band-major blocks: an (n_B, n_A) tensor holding the column-major n_A x n_B matrix"""
    S = torch.empty((B.shape[0], A.shape[0]), dtype=torch.complex128, device=A.device)
    if A.shape[0] and B.shape[0]:
        zgemm(basis, kpt, b"C", A.shape[0], B.shape[0], kpt.n_G, 1.0, A, A.stride(0), B, B.stride(0), 0.0, S, A.shape[0])
    return S


def sub_product(basis, kpt, Y, A, S):
    """Y -= A S in place (A: (n_A, n_G) band-major, S as ``overlaps`` returns it)"""
    if A.shape[0] and Y.shape[0]:
        zgemm(basis, kpt, b"N", kpt.n_G, Y.shape[0], A.shape[0], -1.0, A, A.stride(0), S, A.shape[0], 1.0, Y, Y.stride(0))
    return Y


def mean_kin(basis, psi):
    out = []
    for kpt, p in zip(basis.kpoints, psi):
        mk = np.zeros(p.shape[0])
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_tpa_precondprep(kpt.handle, p.shape[0], p.data_ptr(), p.stride(0), mk.ctypes.data))
        out.append(mk)
    return out


def rayleigh_ritz(basis, ham, psi):
    """the final Rayleigh-Ritz of direct_minimization.jl:181-188: eigenvalues of psi_k' H_k psi_k and psi_k times the vectors"""
    eigenvalues, out = [], []
    for kpt, Hk, p in zip(basis.kpoints, ham, psi):
        nb = p.shape[0]
        M = overlaps(basis, kpt, p, Hk @ p)
        M = (0.5 * (M + M.conj().T)).contiguous()
        V = torch.empty_like(M)
        lam = np.zeros(nb)
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_heev(basis.lane_handles[kpt.lane], nb, M.data_ptr(), nb, lam.ctypes.data, V.data_ptr(), nb))
        basis.post_call(kpt.lane)
        q = torch.empty_like(p)
        zgemm(basis, kpt, b"N", kpt.n_G, nb, nb, 1.0, p, p.stride(0), V, nb, 0.0, q, q.stride(0))
        eigenvalues.append(lam)
        out.append(q)
    return eigenvalues, out


def packed_dot(a, b):
    """Optim's inner product of two packed vectors, sum over blocks of Re(conj(a) b), as a 0-dim device tensor"""
    return sum((x.real * y.real).sum() + (x.imag * y.imag).sum() for x, y in zip(a, b))


class PackedHandle:
    """Base of the native handles over packed vectors shaped like ``shapes`` (band-major ``(n_bands, n_G)``): ``create`` names
    the create entry, ``extra`` is what it takes between the block sizes and the handle."""

    def __init__(self, basis, shapes, create, *extra):
        self.basis, self.handle, self._destroy = basis, None, create.replace("_create", "_destroy")
        self.shapes = [(int(nb), int(ng)) for nb, ng in shapes]
        n = len(self.shapes)
        rows = (C.c_int64 * n)(*[ng for _, ng in self.shapes])
        cols = (C.c_int * n)(*[nb for nb, _ in self.shapes])
        h = C.c_void_p()
        _lib.check(getattr(basis.lib, create)(basis.handle, n, rows, cols, *extra, C.byref(h)))
        self.handle = h

    def _tables(self, *vectors):
        n, who, out = len(self.shapes), type(self).__name__, []
        for blocks in vectors:
            if len(blocks) != n or any(tuple(b.shape) != s for b, s in zip(blocks, self.shapes)):
                raise ValueError(f"{who}: the blocks differ from those given at creation")
            if not all(b.is_cuda and b.dtype == torch.complex128 and b.stride(1) == 1 for b in blocks):
                raise TypeError(f"{who}: complex128 CUDA band-major blocks required")
            out += [(C.c_void_p * n)(*[b.data_ptr() for b in blocks]), (C.c_int64 * n)(*[b.stride(0) for b in blocks])]
        return out

    def _call(self, entry, *args, post=True):
        self.basis.pre_call()
        _lib.check(getattr(self.basis.lib, entry)(self.handle, *args))
        if post:
            self.basis.post_call(0)

    def close(self):
        if self.handle is not None:
            getattr(self.basis.lib, self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        with contextlib.suppress(Exception):
            self.close()
