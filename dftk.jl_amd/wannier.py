"""The Wannier90 interface (host mirror of src/external/wannier_shared.jl): overlaps M^{k,b}, projections A_k, the
``.win / .nnkp / .eig / .amn / .mmn / UNK`` files, and a check of the result that needs no external program.

Device work, one library call per k-point each:

* ``compute_mmn`` / ``overlap_Mmn_k_kpb``: ``dftk_mi_wannier_overlaps`` -- the overlaps of a k-point with ALL its neighbours;
  the partner of a plane wave is looked up through the neighbour's inverse cube -> row map inside the product kernel.
* ``compute_amn`` / ``compute_amn_kpoint``: the radial part of a hydrogenic guess through ``dftk_mi_radial_transform``
  (kind 0) on the reference's logarithmic mesh, all guess columns of the k-point by ``dftk_mi_wannier_guess_columns``
  (centre phase, real solid harmonic, (-i)^l or the closed-form Gaussian, column normalisation), A = psi' g by the library's
  zgemm.  ``GaussianWannierProjection`` / ``HydrogenicWannierProjection`` are callable on host arrays of p = k + G as in
  the reference: that host form is the twin the kernels are tested against.

Host work (n_bands-sized or text): ``compute_nnkp`` builds the b-vector shells and their weights the way wannier90's kmesh
module does (neither wannier90 nor Wannier.jl is needed), ``read_w90_nnkp`` / ``write_w90_nnkp`` move them through the file
format, ``write_w90_*`` and ``write_wannier90_files`` write the reference's formats field for field (eigenvalues in eV,
1-based indices, the reference's loop orders), ``wannier_spreads`` evaluates the Marzari-Vanderbilt functional,
``projection_gauge`` the Loewdin gauge U_k = A_k (A_k' A_k)^{-1/2} and ``rotate_mmn`` applies a gauge to the overlaps.

Supported: spin-unpolarised Monkhorst-Pack calculations on one rank.  Refused: collinear spin, ``bands_plot=True`` (there
is no ``irrfbz_path`` here), ``ExplicitKpoints`` bases, sharded bases, exact exchange (``unfold_bz``).  Left to the external
programs: the spread minimisation itself, disentanglement, band exclusion.
"""
from __future__ import annotations

import ctypes as C
import datetime
import math
import os

import numpy as np

from .model import MonkhorstPack

HARTREE_TO_EV = 27.211386245988          # CODATA 2018, the value behind the reference's auconvert(eV, .)


# ===================================================================================================== projections
def _ps_array(ps):
    ps = np.asarray(ps, dtype=float)
    return ps.reshape(-1, 3)


class GaussianWannierProjection:
    """A Gaussian-shaped initial guess (wannier_shared.jl:9-22); ``center`` in reduced coordinates."""

    def __init__(self, center):
        self.center = np.asarray(center, dtype=float).reshape(3)

    def __call__(self, basis, ps):
        """Fourier transform of the guess at the points ``ps`` = k + G (reduced coordinates, shape (n, 3)), host array."""
        ps = _ps_array(ps)
        p_cart = ps @ np.asarray(basis.model.recip_lattice, dtype=float).T
        return np.exp(2 * np.pi * (-1j * (ps @ self.center) - np.sum(p_cart * p_cart, axis=1) / 4))

    def __repr__(self):
        return f"GaussianWannierProjection({self.center.tolist()})"


def radial_hydrogenic(r, n, alpha=1.0):
    """The radial function R_n0(r) of a hydrogen-like atom with Z / a = ``alpha``, n = 1, 2, 3, normalised to
    int r^2 R^2 dr = 1 (the reference uses the l = 0 radial function for every l)."""
    r = np.asarray(r, dtype=float)
    a = float(alpha)
    if n == 1:
        return 2 * a ** 1.5 * np.exp(-a * r)
    if n == 2:
        return 2 ** -1.5 * a ** 1.5 * (2 - a * r) * np.exp(-a * r / 2)
    if n == 3:
        return math.sqrt(4 / 27) * a ** 1.5 * (1 - 2 / 3 * a * r + 2 / 27 * a ** 2 * r ** 2) * np.exp(-a * r / 3)
    raise ValueError(f"radial_hydrogenic: n = {n} is not supported (1, 2, 3)")


def hydrogenic_radial_mesh(n, alpha):
    """``(r, r^2 R dr)`` on the mesh of the reference (that of QE's pw2wannier90): x from -6 in steps of 0.025 up to
    r = 10, r = e^x / alpha, dr = r dx."""
    xmin, dx, rmax = -6.0, 0.025, 10.0
    n_r = int(round((math.log(rmax) - xmin) / dx)) + 1
    r = np.exp(xmin + dx * np.arange(n_r)) / float(alpha)
    return r, r * r * radial_hydrogenic(r, n, alpha) * (r * dx)


def ylm_real(l, m, rvec):
    """Real spherical harmonics of the reference (spherical_harmonics.jl:8-66: Wikipedia's table), l <= 3; zero at
    |r| <= 10 eps for l > 0.  ``rvec``: (n, 3) -> (n,)."""
    rvec = np.asarray(rvec, dtype=float).reshape(-1, 3)
    if l == 0 and m == 0:
        return np.full(len(rvec), math.sqrt(1 / (4 * np.pi)))
    r = np.linalg.norm(rvec, axis=1)
    small = r <= 10 * np.finfo(float).eps
    u = rvec / np.where(small, 1.0, r)[:, None]
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    pi = np.pi
    table = {
        (1, -1): lambda: math.sqrt(3 / (4 * pi)) * y, (1, 0): lambda: math.sqrt(3 / (4 * pi)) * z,
        (1, 1): lambda: math.sqrt(3 / (4 * pi)) * x,
        (2, -2): lambda: math.sqrt(15 / (4 * pi)) * x * y, (2, -1): lambda: math.sqrt(15 / (4 * pi)) * y * z,
        (2, 0): lambda: math.sqrt(5 / (16 * pi)) * (2 * z ** 2 - x ** 2 - y ** 2),
        (2, 1): lambda: math.sqrt(15 / (4 * pi)) * x * z, (2, 2): lambda: math.sqrt(15 / (16 * pi)) * (x ** 2 - y ** 2),
        (3, -3): lambda: math.sqrt(35 / (32 * pi)) * (3 * x ** 2 - y ** 2) * y,
        (3, -2): lambda: math.sqrt(105 / (4 * pi)) * x * y * z,
        (3, -1): lambda: math.sqrt(21 / (32 * pi)) * y * (4 * z ** 2 - x ** 2 - y ** 2),
        (3, 0): lambda: math.sqrt(7 / (16 * pi)) * z * (2 * z ** 2 - 3 * x ** 2 - 3 * y ** 2),
        (3, 1): lambda: math.sqrt(21 / (32 * pi)) * x * (4 * z ** 2 - x ** 2 - y ** 2),
        (3, 2): lambda: math.sqrt(105 / (16 * pi)) * (x ** 2 - y ** 2) * z,
        (3, 3): lambda: math.sqrt(35 / (32 * pi)) * (x ** 2 - 3 * y ** 2) * x,
    }
    if (l, m) not in table:
        raise ValueError(f"ylm_real: (l, m) = ({l}, {m}) is not implemented (l <= 3, |m| <= l)")
    return np.where(small, 0.0, table[(l, m)]())


class HydrogenicWannierProjection:
    """A hydrogenic initial guess (wannier_shared.jl:30-71): ``center`` in reduced coordinates, quantum numbers
    ``n`` (1..3), ``l`` (0..3), ``m``, and the diffusivity ``alpha`` = Z / a."""

    def __init__(self, center, n, l, m, alpha):
        self.center = np.asarray(center, dtype=float).reshape(3)
        self.n, self.l, self.m, self.alpha = int(n), int(l), int(m), float(alpha)
        if not (1 <= self.n <= 3 and 0 <= self.l <= 3 and abs(self.m) <= self.l and self.alpha > 0):
            raise ValueError(f"HydrogenicWannierProjection: n = {n} (1..3), l = {l} (0..3), |m| <= l and alpha > 0 required")

    def __call__(self, basis, ps):
        """The reference's host evaluation: a sum over the radial mesh per point (the twin of the device path)."""
        from scipy.special import spherical_jn
        ps = _ps_array(ps)
        r, w = hydrogenic_radial_mesh(self.n, self.alpha)
        p_cart = ps @ np.asarray(basis.model.recip_lattice, dtype=float).T
        pnorm = np.linalg.norm(p_cart, axis=1)
        radial = np.array([np.sum(w * spherical_jn(self.l, q * r)) for q in pnorm])
        return np.exp(-2j * np.pi * (ps @ self.center)) * ylm_real(self.l, self.m, p_cart) * (-1j) ** self.l * radial

    def __repr__(self):
        return f"HydrogenicWannierProjection({self.center.tolist()}, {self.n}, {self.l}, {self.m}, {self.alpha})"


def default_wannier_centers(n_wannier, seed=None):
    """Random Gaussian guesses in reduced coordinates (wannier_shared.jl:328); ``seed`` makes them repeatable."""
    rng = np.random.default_rng(seed)
    return [GaussianWannierProjection(rng.random(3)) for _ in range(n_wannier)]


# ===================================================================================================== refusals
def _refuse_basis(basis, who):
    if basis.model.n_spin_components != 1:
        raise NotImplementedError(f"{who}: collinear spin is not supported in the Wannier interface (the reference asserts "
                                  "spin_polarization in (:none, :spinless))")
    if basis.comm_kpts.size > 1 or basis.comm_pw.size > 1:
        raise NotImplementedError(f"{who}: not supported over comm_kpts or comm_pw")


def _mp_grid(basis, who):
    if not isinstance(getattr(basis, "kgrid", None), MonkhorstPack):
        raise ValueError(f"{who}: the basis must be constructed from a MonkhorstPack grid")
    return np.asarray(basis.kgrid.kgrid_size, dtype=int), np.asarray(basis.kgrid.kshift, dtype=float)


def _check_block(psik, kpt, n_bands, who):
    import torch
    if not (torch.is_tensor(psik) and psik.is_cuda and psik.dtype == torch.complex128 and psik.dim() == 2
            and psik.stride(1) == 1 and psik.shape[1] == kpt.n_G):
        raise TypeError(f"{who}: band-major (n_bands, {kpt.n_G}) complex128 CUDA blocks required (the hot path has no CPU "
                        "fallback)")
    if not 0 < n_bands <= psik.shape[0]:
        raise ValueError(f"{who}: n_bands = {n_bands} outside 1 .. {psik.shape[0]}")


# ===================================================================================================== overlaps
def _overlaps_of_kpoint(basis, psi, ik, neighbours, n_bands, out):
    """``out`` (len(neighbours) n_bands, n_bands) <- the overlaps of k-point ``ik`` with [(ik_plus_b, G_shift)] (device)."""
    from . import _lib
    kpt = basis.kpoints[ik]
    n_nb = len(neighbours)
    handles = (C.c_void_p * n_nb)(*[basis.kpoints[j].handle.value for j, _ in neighbours])
    ptrs = (C.c_void_p * n_nb)(*[psi[j].data_ptr() for j, _ in neighbours])
    lds = np.ascontiguousarray([psi[j].stride(0) for j, _ in neighbours], dtype=np.int64)
    dG = np.ascontiguousarray([list(g) for _, g in neighbours], dtype=np.int32).reshape(-1)
    _lib.check(basis.lib.dftk_mi_wannier_overlaps(kpt.handle, n_bands, psi[ik].data_ptr(), psi[ik].stride(0), n_nb,
                                                  C.cast(handles, C.c_void_p), dG.ctypes.data, C.cast(ptrs, C.c_void_p),
                                                  lds.ctypes.data, out.data_ptr()))


def _as_reference_M(dev_block, n_nb, n_bands):
    """device (n_nb n_bands, n_bands) [= column-major n_bands x (n_nb n_bands)] -> host (n_nb, m, n); a matrix of zeros (no
    shared plane wave) becomes the identity (wannier_shared.jl:239)."""
    M = dev_block.cpu().numpy().reshape(n_nb, n_bands, n_bands).transpose(0, 2, 1).copy()
    for j in range(n_nb):
        if not M[j].any():
            M[j] = np.eye(n_bands)
    return M


def overlap_Mmn_k_kpb(basis, psi, ik, ik_plus_b, G_shift, n_bands):
    """``overlap_Mmn_k_kpb`` (wannier_shared.jl:220-241) with 0-based k-point indices: [M^{k,b}]_{mn} = <u_mk | u_n,k+b>
    over the plane waves G of k whose partner G + G_shift is a plane wave of k + b; the identity when none is shared.
    Host (n_bands, n_bands) complex array."""
    import torch
    _refuse_basis(basis, "overlap_Mmn_k_kpb")
    basis._require_gpu()
    for j in (ik, ik_plus_b):
        _check_block(psi[j], basis.kpoints[j], n_bands, "overlap_Mmn_k_kpb")
    out = torch.empty((n_bands, n_bands), dtype=torch.complex128, device=basis.device)
    basis.pre_call()
    _overlaps_of_kpoint(basis, psi, ik, [(ik_plus_b, tuple(int(g) for g in G_shift))], n_bands, out)
    basis.post_call(basis.kpoints[ik].lane)
    return _as_reference_M(out, 1, n_bands)[0]


def _neighbour_lists(nnkp, n_k):
    lists = [[] for _ in range(n_k)]
    for ik, ikpb, G_shift in nnkp["nnkpts"]:
        if not (0 <= ik < n_k and 0 <= ikpb < n_k):
            raise ValueError(f"nnkp: k-point indices ({ik}, {ikpb}) outside 0 .. {n_k - 1}")
        lists[ik].append((int(ikpb), tuple(int(g) for g in G_shift)))
    nntot = int(nnkp["nntot"])
    if any(len(entry) != nntot for entry in lists):
        raise ValueError(f"nnkp: every k-point needs nntot = {nntot} neighbours")
    return lists


def compute_mmn(basis, psi, nnkp, n_bands):
    """All overlaps of ``nnkp``: host array (n_k, nntot, n_bands, n_bands), ``M[ik, j]`` the matrix of the j-th neighbour
    of k-point ``ik`` in the order of ``nnkp["nnkpts"]``.  One library call per k-point serves all its neighbours."""
    import torch
    _refuse_basis(basis, "compute_mmn")
    n_k = len(basis.kpoints)
    lists = _neighbour_lists(nnkp, n_k)
    basis._require_gpu()
    if len(psi) != n_k:
        raise ValueError("compute_mmn: one block per k-point of the basis")
    for kpt, psik in zip(basis.kpoints, psi):
        _check_block(psik, kpt, n_bands, "compute_mmn")
    nntot = int(nnkp["nntot"])
    out = torch.empty((n_k, nntot * n_bands, n_bands), dtype=torch.complex128, device=basis.device)
    basis.pre_call()
    for ik in range(n_k):
        _overlaps_of_kpoint(basis, psi, ik, lists[ik], n_bands, out[ik])
    basis.post_call()
    return np.stack([_as_reference_M(out[ik], nntot, n_bands) for ik in range(n_k)])


# ===================================================================================================== projections A_k
def _guess_columns(basis, kpt, projections, normalize=True):
    """(n_wannier, n_G) device block of the guess orbitals at k + G of ``kpt`` (column-major n_G x n_wannier)."""
    import torch
    from . import _lib
    from .terms import radial_transform_abi
    kinds, lm, chans, centers, channels = [], [], [], [], {}
    for proj in projections:
        if isinstance(proj, GaussianWannierProjection):
            kinds.append(0); lm.append((0, 0)); chans.append(0)
        elif isinstance(proj, HydrogenicWannierProjection):
            kinds.append(1); lm.append((proj.l, proj.m))
            chans.append(channels.setdefault((proj.n, proj.l, proj.alpha), len(channels)))
        else:
            raise TypeError(f"compute_amn_kpoint: {type(proj).__name__} has no device form (GaussianWannierProjection and "
                            "HydrogenicWannierProjection have)")
        centers.append(proj.center)
    n_G, n_w = kpt.n_G, len(projections)
    R = None
    if channels:
        q = torch.linalg.norm(kpt.Gplusk_cart, dim=1).contiguous()
        R = torch.empty((len(channels), n_G), dtype=torch.float64, device=basis.device)
        for (n, l, alpha), c in channels.items():
            r, w = hydrogenic_radial_mesh(n, alpha)
            R[c] = radial_transform_abi(basis, 0, l, r, w, 0.0, q)
    out = torch.empty((n_w, n_G), dtype=torch.complex128, device=basis.device)
    if n_w == 0:
        return out
    Bh = np.asfortranarray(basis.model.recip_lattice, dtype=np.float64)
    kh = np.ascontiguousarray(kpt.coordinate, dtype=np.float64)
    kind_h = np.ascontiguousarray(kinds, dtype=np.int32)
    lm_h = np.ascontiguousarray(lm, dtype=np.int32).reshape(-1)
    chan_h = np.ascontiguousarray(chans, dtype=np.int32)
    cen_h = np.ascontiguousarray(centers, dtype=np.float64).reshape(-1)
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_wannier_guess_columns(kpt.handle, Bh.ctypes.data, kh.ctypes.data, n_w, kind_h.ctypes.data,
                                                       lm_h.ctypes.data, chan_h.ctypes.data, cen_h.ctypes.data, len(channels),
                                                       R.data_ptr() if R is not None else None, n_G, 1 if normalize else 0,
                                                       out.data_ptr(), n_G))
    basis.post_call(kpt.lane)
    return out


def compute_amn_kpoint(basis, kpt, psi_k, projections, n_bands):
    """``compute_amn_kpoint`` (wannier_shared.jl:278-298): [A_k]_{mn} = <psi_mk | g_n / |g_n|> with the guesses evaluated at
    the plane waves of ``kpt`` on the device.  Host (n_bands, n_wannier) complex array."""
    import torch
    from . import _lib
    _refuse_basis(basis, "compute_amn_kpoint")
    basis._require_gpu()
    _check_block(psi_k, kpt, n_bands, "compute_amn_kpoint")
    g = _guess_columns(basis, kpt, projections)
    n_w = g.shape[0]
    out = torch.empty((n_w, n_bands), dtype=torch.complex128, device=basis.device)      # column-major n_bands x n_w
    if n_w == 0:
        return np.zeros((n_bands, 0), dtype=complex)
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_zgemm(basis.lane_handles[kpt.lane], b"C", n_bands, n_w, kpt.n_G, _lib.cplx(1.0),
                                       psi_k.data_ptr(), psi_k.stride(0), g.data_ptr(), g.stride(0), _lib.cplx(0.0),
                                       out.data_ptr(), n_bands))
    basis.post_call(kpt.lane)
    return out.cpu().numpy().T.copy()


def compute_amn(basis, psi, projections, n_bands):
    """A_k of every k-point: host array (n_k, n_bands, n_wannier)."""
    _refuse_basis(basis, "compute_amn")
    if len(psi) != len(basis.kpoints):
        raise ValueError("compute_amn: one block per k-point of the basis")
    return np.stack([compute_amn_kpoint(basis, kpt, psik, projections, n_bands) for kpt, psik in zip(basis.kpoints, psi)])


# ===================================================================================================== neighbours
_VOIGT = ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (2, 0))


def _shell_column(bs):
    return np.array([np.sum(bs[:, a] * bs[:, b]) for a, b in _VOIGT])


def _mesh_index(basis, size, shift):
    """{integer address of a mesh point modulo the reciprocal lattice: index of the k-point}; the basis must hold the whole
    mesh, every point once."""
    coords = [np.asarray(k.coordinate, dtype=float) for k in basis.kpoints]
    index = {}
    for ik, k in enumerate(coords):
        x = k * size - shift
        if np.any(np.abs(x - np.rint(x)) > 1e-8):
            raise ValueError(f"compute_nnkp: the k-point {k} is not on the Monkhorst-Pack mesh of the basis")
        index[tuple(np.mod(np.rint(x).astype(int), size))] = ik
    if len(index) != len(coords) or len(coords) != int(np.prod(size)):
        raise ValueError(f"compute_nnkp: the basis holds {len(coords)} k-points, the full mesh has {int(np.prod(size))}: unfold "
                         "it first (unfold_bz)")
    return coords, index


def _bvector_shells(recip, size, n_search=5, tol=1e-6):
    """The vectors B (n / size), n integer, 0 < |n_i| <= n_search, grouped into shells of equal length, by increasing length;
    within a shell in lexicographic order of n.  Returns [(n (m, 3) int, b_cart (m, 3))]."""
    rng = range(-n_search, n_search + 1)
    ns = np.array([(i, j, k) for i in rng for j in rng for k in rng if (i, j, k) != (0, 0, 0)], dtype=int)
    b = (ns / size) @ np.asarray(recip, dtype=float).T
    norm = np.linalg.norm(b, axis=1)
    order = np.argsort(norm, kind="stable")
    ns, b, norm = ns[order], b[order], norm[order]
    shells, start = [], 0
    for i in range(1, len(ns) + 1):
        if i == len(ns) or norm[i] - norm[start] > tol * norm[start]:
            inner = np.lexsort((ns[start:i, 2], ns[start:i, 1], ns[start:i, 0]))
            shells.append((ns[start:i][inner], b[start:i][inner]))
            start = i
    # only shells that the search cube holds completely: those inside the sphere inscribed in it
    r_in = min(np.linalg.norm(np.linalg.inv((np.asarray(recip, dtype=float) / size).T), axis=0) ** -1) * n_search
    return [s for s in shells if np.linalg.norm(s[1][0]) < r_in * (1 - tol)]


def bvector_weights(shells_b, tol=1e-10):
    """Which of the shells (list of (m, 3) Cartesian b vectors, by increasing length) to use and with which weights so that
    sum_b w_b b_a b_b = delta_ab (Marzari-Vanderbilt eq. B1), the way wannier90's kmesh module chooses: go through the shells
    by increasing |b|, solve the 6 x n_shells least-squares problem by SVD; a shell that makes the system singular (its
    column depends on those already taken) or does not reduce the residual is skipped; stop once the condition holds to
    ``tol``.  Returns [(shell index, weight)] of the shells with a non-zero weight."""
    target = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    taken, cols, residual, w = [], [], np.linalg.norm(target), np.zeros(0)
    for s, bs in enumerate(shells_b):
        col = _shell_column(bs)
        A = np.array(cols + [col]).T
        sv = np.linalg.svd(A / np.linalg.norm(A, axis=0), compute_uv=False)
        if sv[-1] < 1e-6 * sv[0]:
            continue
        w_try = np.linalg.lstsq(A, target, rcond=None)[0]
        r_try = np.linalg.norm(A @ w_try - target)
        if not r_try < residual * (1 - 1e-9):
            continue
        taken.append(s); cols.append(col); w = w_try; residual = r_try
        if residual <= tol:
            break
    if residual > tol:
        raise RuntimeError(f"compute_nnkp: no set of b-vector shells satisfies the completeness relation (residual {residual:.3e})")
    scale = np.max(np.abs(w))
    return [(s, float(x)) for s, x in zip(taken, w) if abs(x) > 1e-10 * scale]


def compute_nnkp(basis):
    """The finite-difference neighbours of every k-point of a full Monkhorst-Pack mesh and their weights, as wannier90's
    kmesh module finds them: ``dict(nntot, nnkpts=[(ik, ik_plus_b, G_shift)], bvectors_cart (nntot, 3), weights (nntot,))``,
    0-based indices, k_{ik_plus_b} + G_shift - k_ik = b_j for the j-th entry of k-point ik (the same order of b for every
    k-point).  Host NumPy; a descriptor-only basis will do."""
    _refuse_basis(basis, "compute_nnkp")
    size, shift = _mp_grid(basis, "compute_nnkp")
    coords, index = _mesh_index(basis, size, shift)
    recip = np.asarray(basis.model.recip_lattice, dtype=float)
    shells = _bvector_shells(recip, size)
    chosen = bvector_weights([b for _, b in shells])
    ns = np.concatenate([shells[s][0] for s, _ in chosen])
    bcart = np.concatenate([shells[s][1] for s, _ in chosen])
    weights = np.concatenate([np.full(len(shells[s][0]), w) for s, w in chosen])
    nnkpts = []
    for ik, k in enumerate(coords):
        addr = np.rint(k * size - shift).astype(int)
        for n in ns:
            j = index[tuple(np.mod(addr + n, size))]
            G = k + n / size - coords[j]
            if np.any(np.abs(G - np.rint(G)) > 1e-8):
                raise RuntimeError("compute_nnkp: inconsistent mesh")
            nnkpts.append((ik, j, tuple(int(g) for g in np.rint(G))))
    return dict(nntot=len(ns), nnkpts=nnkpts, bvectors_cart=bcart, weights=weights)


def complete_nnkp(basis, nnkp):
    """A copy of an ``nnkp`` read from a file with ``bvectors_cart`` and ``weights`` added (``wannier_spreads`` needs them):
    the b vectors are read off the k-points of ``basis``, the weights solved per shell as ``compute_nnkp`` does.  The j-th
    neighbour must be the same b for every k-point, as wannier90 writes them."""
    lists = _neighbour_lists(nnkp, len(basis.kpoints))
    recip = np.asarray(basis.model.recip_lattice, dtype=float)
    coords = [np.asarray(k.coordinate, dtype=float) for k in basis.kpoints]
    b = np.array([[(coords[j] + np.asarray(G) - coords[ik]) @ recip.T for j, G in lists[ik]] for ik in range(len(coords))])
    if np.max(np.abs(b - b[0][None])) > 1e-8 * np.max(np.abs(b)):
        raise ValueError("complete_nnkp: the neighbours are not listed in the same order of b for every k-point")
    b = b[0]
    norm = np.linalg.norm(b, axis=1)
    order = np.argsort(norm, kind="stable")
    groups, start = [], 0
    for i in range(1, len(order) + 1):
        if i == len(order) or norm[order[i]] - norm[order[start]] > 1e-6 * norm[order[start]]:
            groups.append(order[start:i]); start = i
    A = np.array([_shell_column(b[g]) for g in groups]).T
    w_shell = np.linalg.lstsq(A, np.array([1.0, 1, 1, 0, 0, 0]), rcond=None)[0]
    weights = np.zeros(len(b))
    for g, w in zip(groups, w_shell):
        weights[g] = w
    if np.max(np.abs(np.einsum("j,ja,jb->ab", weights, b, b) - np.eye(3))) > 1e-8:
        raise ValueError("complete_nnkp: the b vectors of the file do not satisfy the completeness relation")
    return dict(nnkp, bvectors_cart=b, weights=weights)


def write_w90_nnkp(fileprefix, nnkp):
    """The ``nnkpts`` block of a ``.nnkp`` file as wannier90 writes it (1-based indices in the file)."""
    with open(fileprefix + ".nnkp", "w") as fp:
        fp.write(f"File written on {datetime.datetime.now().isoformat(sep=' ', timespec='seconds')}\n\n")
        fp.write("begin nnkpts\n")
        fp.write(f"{int(nnkp['nntot']):4d}\n")
        for ik, ikpb, G in nnkp["nnkpts"]:
            fp.write(f"{ik + 1:6d}{ikpb + 1:6d}   {G[0]:6d}{G[1]:6d}{G[2]:6d}\n")
        fp.write("end nnkpts\n")


def read_w90_nnkp(fileprefix):
    """``read_w90_nnkp`` (wannier_shared.jl:152-174) of a file wannier90 wrote (``wannier90.x -pp prefix``):
    ``dict(nntot, nnkpts=[(ik, ik_plus_b, G_shift)])`` with 0-based indices (1-based in the file)."""
    fn = fileprefix + ".nnkp"
    if not os.path.isfile(fn):
        raise FileNotFoundError(f"Expected file {fn} not found.")
    with open(fn) as fp:
        lines = [line.strip() for line in fp]
    try:
        i0, i1 = lines.index("begin nnkpts"), lines.index("end nnkpts")
    except ValueError:
        raise ValueError(f"{fn}: no nnkpts block") from None
    nntot = int(lines[i0 + 1])
    nnkpts = []
    for line in lines[i0 + 2:i1]:
        v = [int(x) for x in line.split()]
        if len(v) != 5:
            raise ValueError(f"{fn}: an nnkpts line needs 5 integers, got {line!r}")
        nnkpts.append((v[0] - 1, v[1] - 1, (v[2], v[3], v[4])))
    return dict(nntot=nntot, nnkpts=nnkpts)


# ===================================================================================================== file writers
def _now():
    return datetime.datetime.now().isoformat(timespec="milliseconds")


def write_w90_win(fileprefix, basis, bands_plot=False, wannier_plot=False, **kwargs):
    """``write_w90_win`` (wannier_shared.jl:77-139); wannier90 parameters as keyword arguments (``num_bands`` and
    ``num_wann`` are required).  ``bands_plot=True`` needs a k-path through the irreducible Brillouin zone, which this
    package does not provide: ``NotImplementedError``."""
    if bands_plot:
        raise NotImplementedError("write_w90_win: bands_plot=True needs irrfbz_path, which is not available")
    if "num_bands" not in kwargs or "num_wann" not in kwargs:
        raise ValueError("write_w90_win: num_bands and num_wann are required")
    size, _ = _mp_grid(basis, "write_w90_win")
    with open(fileprefix + ".win", "w") as fp:
        fp.write(f"! Generated by dftk_jl_amd at {_now()}\n\n")
        for key, value in kwargs.items():
            fp.write("%-20s =   %-30s\n" % (key, value))
        if wannier_plot:
            fp.write("wvfn_formatted = True\n")
            fp.write("wannier_plot   = True\n")
        fp.write("\n" + "!" * 20 + " System \n\n\n")
        fp.write("begin unit_cell_cart\nbohr\n")
        for vec in np.asarray(basis.model.lattice, dtype=float).T:           # lattice vectors are rows in wannier90
            fp.write("%10.6f %10.6f %10.6f \n" % tuple(vec))
        fp.write("end unit_cell_cart \n\n")
        fp.write("begin atoms_frac\n")
        for atom, pos in zip(basis.model.atoms, basis.model.positions):
            fp.write("%-2s %10.6f %10.6f %10.6f \n" % ((atom.symbol,) + tuple(float(x) for x in pos)))
        fp.write("end atoms_frac\n\n")
        fp.write("!" * 20 + " k_points\n\n")
        fp.write(f"mp_grid : {size[0]} {size[1]} {size[2]}\n\n")
        fp.write("begin kpoints\n")
        for kpt in basis.kpoints[:basis.n_kcoords_local]:
            fp.write("%10.10f %10.10f %10.10f\n" % tuple(kpt.coordinate))
        fp.write("end kpoints\n")


def write_w90_eig(fileprefix, eigenvalues, n_bands):
    """``write_w90_eig`` (wannier_shared.jl:180-189): band index, k-point index (1-based), eigenvalue in eV."""
    with open(fileprefix + ".eig", "w") as fp:
        for k, eps in enumerate(eigenvalues):
            for n in range(n_bands):
                fp.write("%3i  %3i   %25.18f \n" % (n + 1, k + 1, float(eps[n]) * HARTREE_TO_EV))


def write_w90_amn(fileprefix, A):
    """``write_w90_amn`` (wannier_shared.jl:301-322) of the projections ``A`` (n_k, n_bands, n_wannier) that ``compute_amn``
    returns: per k-point the Wannier index n outside, the band index m inside."""
    A = np.asarray(A)
    n_k, n_bands, n_w = A.shape
    with open(fileprefix + ".amn", "w") as fp:
        fp.write(f"Generated by dftk_jl_amd at {_now()}\n")
        fp.write(f"{n_bands}   {n_k}  {n_w}\n")
        for ik in range(n_k):
            for n in range(n_w):
                for m in range(n_bands):
                    fp.write("%3i %3i %3i  %22.18f %22.18f \n" % (m + 1, n + 1, ik + 1, A[ik, m, n].real, A[ik, m, n].imag))


def write_w90_mmn(fileprefix, M, nnkp):
    """``write_w90_mmn`` (wannier_shared.jl:243-255) of the overlaps ``M`` (n_k, nntot, n_bands, n_bands) that ``compute_mmn``
    returns for ``nnkp``: per (k, b) the header line with 1-based indices, then the matrix column by column."""
    M = np.asarray(M)
    n_k, nntot, n_bands, _ = M.shape
    lists = _neighbour_lists(nnkp, n_k)
    with open(fileprefix + ".mmn", "w") as fp:
        fp.write(f"Generated by dftk_jl_amd at {_now()}\n")
        fp.write(f"{n_bands}  {n_k}  {nntot}\n")
        seen = [0] * n_k
        for ik, ikpb, G in nnkp["nnkpts"]:
            j = seen[ik]
            seen[ik] += 1
            assert lists[ik][j][0] == ikpb
            fp.write("%i  %i  %i  %i  %i \n" % (ik + 1, ikpb + 1, G[0], G[1], G[2]))
            for n in range(n_bands):
                for m in range(n_bands):
                    fp.write("%22.18f %22.18f \n" % (M[ik, j, m, n].real, M[ik, j, m, n].imag))


def write_w90_unk(fileprefix, basis, psi, n_bands, spin=1):
    """``write_w90_unk`` (wannier_shared.jl:192-207): ``UNK<ik>.<spin>`` next to ``fileprefix``, the periodic part of every
    band on the FFT grid (x fastest) through the library's per-band inverse transform."""
    import torch
    from . import _lib
    basis._require_gpu()
    nx, ny, nz = basis.fft_size
    cube = torch.empty((nz, ny, nx), dtype=torch.complex128, device=basis.device)
    folder = os.path.dirname(fileprefix) or "."
    for ik, kpt in enumerate(basis.kpoints):
        if kpt.spin != spin:
            continue
        _check_block(psi[ik], kpt, n_bands, "write_w90_unk")
        with open(os.path.join(folder, "UNK%05i.%i" % (ik + 1, spin)), "w") as fp:
            fp.write(f"{nx} {ny} {nz} {ik + 1} {n_bands}\n")
            for n in range(n_bands):
                basis.pre_call()
                _lib.check(basis.lib.dftk_mi_ifft_sphere(kpt.handle, psi[ik][n].data_ptr(), cube.data_ptr()))
                basis.post_call(kpt.lane)
                vals = (cube * basis.ifft_normalization).reshape(-1).cpu().numpy()
                fp.write("".join("%25.18f %25.18f\n" % (v.real, v.imag) for v in vals))


def write_wannier90_files(scfres, fileprefix, n_bands, n_wannier, projections, nnkp=None, wannier_plot=False, **win_kwargs):
    """``write_wannier90_files`` (wannier_shared.jl:333-368): unfold the SCF result onto the full mesh, write ``.win``,
    ``.nnkp``, ``.eig``, ``.amn``, ``.mmn`` (and the ``UNK`` files with ``wannier_plot``).  ``nnkp``: the neighbours from a
    wannier90 preprocessing run (``read_w90_nnkp``); None: ``compute_nnkp``.  Further keyword arguments go into the
    ``.win`` file.  Returns ``dict(scfres=<unfolded>, nnkp, M, A)``."""
    from .unfold import unfold_bz
    basis = scfres["basis"]
    _refuse_basis(basis, "write_wannier90_files")
    if win_kwargs.get("bands_plot"):
        raise NotImplementedError("write_wannier90_files: bands_plot=True needs irrfbz_path, which is not available")
    if len(projections) != n_wannier:
        raise ValueError(f"write_wannier90_files: {len(projections)} projections for n_wannier = {n_wannier}")
    _mp_grid(basis, "write_wannier90_files")
    unfolded = unfold_bz(scfres)
    basis, psi = unfolded["basis"], unfolded["psi"]
    folder = os.path.dirname(fileprefix)
    if folder:
        os.makedirs(folder, exist_ok=True)
    write_w90_win(fileprefix, basis, num_wann=n_wannier, num_bands=n_bands, wannier_plot=wannier_plot, **win_kwargs)
    if nnkp is None:
        nnkp = compute_nnkp(basis)
        write_w90_nnkp(fileprefix, nnkp)
    write_w90_eig(fileprefix, unfolded["eigenvalues"], n_bands)
    A = compute_amn(basis, psi, projections, n_bands)
    write_w90_amn(fileprefix, A)
    M = compute_mmn(basis, psi, nnkp, n_bands)
    write_w90_mmn(fileprefix, M, nnkp)
    if wannier_plot:
        write_w90_unk(fileprefix, basis, psi, n_bands, spin=1)
    return dict(scfres=unfolded, nnkp=nnkp, M=M, A=A)


# ===================================================================================================== spreads and gauges
def wannier_spreads(M, nnkp):
    """The Marzari-Vanderbilt spread functional of the overlaps ``M`` (n_k, nntot, J, J) in the gauge they are given in
    (Phys. Rev. B 56, 12847, eqs. 31, 34-36), with b_j = ``nnkp["bvectors_cart"][j]`` and w_j = ``nnkp["weights"][j]``:
    ``dict(omega_I, omega_OD, omega_D, omega, centers (J, 3) Cartesian, spreads (J,))``.  Host, n_bands-sized matrices."""
    M = np.asarray(M)
    if "weights" not in nnkp or "bvectors_cart" not in nnkp:
        raise ValueError("wannier_spreads: nnkp needs bvectors_cart and weights (compute_nnkp, or complete_nnkp of a file's)")
    b = np.asarray(nnkp["bvectors_cart"], dtype=float)
    w = np.asarray(nnkp["weights"], dtype=float)
    n_k, nntot, J, _ = M.shape
    if b.shape != (nntot, 3) or w.shape != (nntot,):
        raise ValueError("wannier_spreads: M and nnkp do not fit")
    diag = np.einsum("kjnn->kjn", M)
    phase = np.angle(diag)                                              # Im ln M_nn
    centers = -np.einsum("j,ja,kjn->na", w, b, phase) / n_k
    abs2 = np.abs(M) ** 2
    omega_I = float(np.einsum("j,kj->", w, J - abs2.sum(axis=(2, 3))) / n_k)
    omega_OD = float(np.einsum("j,kj->", w, abs2.sum(axis=(2, 3)) - (np.abs(diag) ** 2).sum(axis=2)) / n_k)
    q = -phase - np.einsum("ja,na->jn", b, centers)[None]
    omega_D = float(np.einsum("j,kjn->", w, q ** 2) / n_k)
    r2 = np.einsum("j,kjn->n", w, 1 - np.abs(diag) ** 2 + phase ** 2) / n_k
    return dict(omega_I=omega_I, omega_OD=omega_OD, omega_D=omega_D, omega=omega_I + omega_OD + omega_D, centers=centers,
                spreads=r2 - np.sum(centers ** 2, axis=1))


def projection_gauge(A):
    """U_k = A_k (A_k' A_k)^{-1/2} for every k-point of ``A`` (n_k, n_bands, n_wannier): the Loewdin-orthonormalised
    projections, through the singular value decomposition A = W S V' (U = W V')."""
    A = np.asarray(A)
    W, s, Vh = np.linalg.svd(A, full_matrices=False)
    if np.min(s) < 1e-10 * np.max(s):
        raise ValueError("projection_gauge: the projections of a k-point are linearly dependent")
    return W @ Vh


def rotate_mmn(M, U, nnkp):
    """The overlaps in the gauge ``U`` (n_k, n_bands, n_wannier): M^{k,b} -> U_k' M^{k,b} U_{k+b}."""
    M, U = np.asarray(M), np.asarray(U)
    lists = _neighbour_lists(nnkp, M.shape[0])
    out = np.empty((M.shape[0], M.shape[1], U.shape[2], U.shape[2]), dtype=complex)
    for ik, entry in enumerate(lists):
        for j, (ikpb, _) in enumerate(entry):
            out[ik, j] = U[ik].conj().T @ M[ik, j] @ U[ikpb]
    return out
