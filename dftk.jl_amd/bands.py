"""Band structures and projected densities of states (src/postprocess/band_structure.jl:14-92, :276-283;
src/postprocess/dos.jl:70-238).

``compute_bands`` builds a basis of the same discretisation on new k-points, the Hamiltonian of a given density on it, and
diagonalises with the existing ``diagonalize_all_kblocks`` (LOBPCG, k -> k+1 interpolation, batched small blocks): nothing of
the eigensolver is new.  The orbital side is: per k-point the pseudo-atomic orbitals of the UPF files as a device matrix
(``dftk_mi_radial_transform`` per channel, ``dftk_mi_build_projectors_radial``), orthonormalised by
``dftk_mi_lowdin_ortho``; projections and the smeared sum over bands by ``dftk_mi_pdos_accumulate`` (csrc/pdos_kernels.hip).

Conventions: ``iatom`` of a label indexes ``model.atoms`` (0-based); ``n`` is the 1-based index of the radial function among
those of its l in the file, as the reference's (dos.jl:149-151); the i of ``pswfc_label(i, l)`` is 1-based like every
``eval_psp_*`` function of this package.  There is no automatic k-path (``irrfbz_path`` needs Spglib / Brillouin): paths are
given as ``KPath`` objects.
"""
from __future__ import annotations

import ctypes as C
import gc
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .basis import PlaneWaveBasis
from .eigen import diagonalize_all_kblocks, lobpcg_hyper
from .model import ExplicitKpoints, MonkhorstPack
from .scf import _occupations, default_n_bands
from .terms import energy_hamiltonian, guess_density, radial_transform_abi

SMEARING_KINDS = {"fermi_dirac": 1, "gaussian": 2}       # the codes of dftk_mi_fermi_bisection / dftk_mi_pdos_accumulate


# ------------------------------------------------------------------------------------------ k-paths
@dataclass
class KPath:
    """``KPath(points, paths)``: ``points`` maps a label to reduced coordinates, ``paths`` lists the branches, each a list of
    labels joined by straight segments (Brillouin.jl's ``KPath`` without the lattice, which the model supplies)."""
    points: dict
    paths: list


def kpath_interpolate(model, kpath: KPath, kline_density: float = 40.0):
    """k-points along ``kpath`` with about ``kline_density`` points per inverse bohr of Cartesian length
    (band_structure.jl:88-92): a segment of length L carries max(2, ceil(L density)) points, both ends included, and a joint
    of two segments appears once.  Returns a dict: ``kcoords`` (reduced), ``kdistances`` (cumulative Cartesian length; a new
    branch continues where the previous one ended), ``labels`` (list of (index, label)), ``branches`` (index ranges)."""
    B = np.asarray(model.recip_lattice, dtype=float)
    kcoords, dist, labels, branches = [], [], [], []
    offset = 0.0
    for path in kpath.paths:
        if len(path) < 2:
            raise ValueError("a branch of a KPath needs at least two labels")
        start = len(kcoords)
        pts = [np.asarray(kpath.points[name], dtype=float) for name in path]
        kcoords.append(pts[0])
        dist.append(offset)
        labels.append((len(kcoords) - 1, path[0]))
        for a, b, name in zip(pts[:-1], pts[1:], path[1:]):
            length = float(np.linalg.norm(B @ (b - a)))
            n = max(2, int(math.ceil(length * kline_density)))
            d0 = dist[-1]
            for i in range(1, n):
                t = i / (n - 1)
                kcoords.append(a + t * (b - a) if i < n - 1 else b)
                dist.append(d0 + t * length)
            labels.append((len(kcoords) - 1, name))
        offset = dist[-1]
        branches.append(range(start, len(kcoords)))
    return dict(kcoords=[np.asarray(k) for k in kcoords], kdistances=np.asarray(dist), labels=labels, branches=branches)


# ------------------------------------------------------------------------------------------ bands
def default_n_bands_bandstructure(model_or_scfres_or_n):
    """band_structure.jl:276-283: ceil(n + 5 sqrt(n)) with n the number of SCF bands (of an ``scfres``: those it carries; of
    a model: ``default_n_bands``)."""
    x = model_or_scfres_or_n
    if isinstance(x, dict):
        n = len(x["occupation"][0])
    elif isinstance(x, (int, np.integer)):
        n = int(x)
    else:
        n = default_n_bands(x)
    return int(math.ceil(n + 5 * math.sqrt(n)))


def _refuse_unsupported(basis, what):
    if getattr(basis.model, "exact_exchange", None) is not None:
        raise NotImplementedError("Band structure computations with exact exchange not yet supported.")
    if basis.comm_pw.size > 1:
        raise NotImplementedError(f"{what} on a plane-wave sharded basis (comm_pw.size > 1) is not implemented")
    if basis.comm_kpts.size > 1:
        raise NotImplementedError(f"{what} on a k-point sharded basis (comm_kpts.size > 1) is not implemented")


def _basis_on(basis, kgrid, build_terms=True):
    """``PlaneWaveBasis(basis, kgrid)``: the same model, Ecut, fft_size, device and block switches on other k-points."""
    return PlaneWaveBasis(basis.model, basis.Ecut, kgrid, fft_size=basis.fft_size, device=basis.device,
                          build_terms=build_terms, gamma_real=basis.gamma_real,
                          use_symmetries_for_kpoint_reduction=basis.use_symmetries_for_kpoint_reduction)


def _solve(bs_basis, rho, n_bands, n_extra, tol, seed, diag_kwargs, hubbard_n=None, tau=None):
    with bs_basis.on_library_stream():
        # (the Hubbard term of bs_basis builds the manifold's orbitals at the new k-points)
        _, ham = energy_hamiltonian(bs_basis, None, None, rho=rho, only_hamiltonian=True, hubbard_n=hubbard_n, tau=tau)
        gen = torch.Generator(device=bs_basis.device)
        gen.manual_seed(seed)
        eig = diagonalize_all_kblocks(lobpcg_hyper, ham, n_bands + n_extra, n_conv_check=n_bands, tol=tol, generator=gen,
                                      seed=seed, **diag_kwargs)
        # select_eigenpairs_all_kblocks(eigres, 1:n_bands)
        eig["λ"] = [lam[:n_bands].copy() for lam in eig["λ"]]
        eig["X"] = [X[:n_bands] for X in eig["X"]]
        eig["residual_norms"] = [r[:n_bands].copy() for r in eig["residual_norms"]]
        bs_basis.sync()
    return eig


def compute_bands(basis_or_scfres, kgrid_or_kpath, n_bands=None, n_extra=3, rho=None, eF=None, tol=1e-3,
                  kline_density=40, kchunk=None, keep_psi=True, seed=0, hubbard_n=None, tau=None, **diag_kwargs):
    """``compute_bands(basis | scfres, kgrid | kpath; n_bands, n_extra, rho, eF, tol, kline_density)``
    (band_structure.jl:14-92): ``n_bands`` eigenpairs of the Hamiltonian of ``rho`` at other k-points.  From an ``scfres`` the
    density and the Fermi level are its own and ``n_bands`` defaults to ``default_n_bands_bandstructure(scfres)``.  Returns a
    dict shaped like an ``scfres``: basis, psi, eigenvalues, rho, eF, occupation (None without eF), diagonalization,
    converged, and for a ``KPath`` the interpolation as ``kinter``.

    ``kchunk`` (an extension): the k-points are solved in chunks of that many on bases of their own, each released before the
    next, so that a long path on a large cell needs the device memory of one chunk; the returned basis then carries the
    k-points only (no terms).  ``keep_psi=False`` keeps the eigenvalues alone (no ``psi`` entry).  ``hubbard_n`` (models with
    a Hubbard term): the occupation matrices of the Hamiltonian; from an ``scfres`` they are its own."""
    if isinstance(basis_or_scfres, dict):
        scfres = basis_or_scfres
        basis = scfres["basis"]
        rho = scfres["rho"] if rho is None else rho
        eF = scfres.get("eF") if eF is None else eF
        hubbard_n = scfres.get("hubbard_n") if hubbard_n is None else hubbard_n
        tau = scfres.get("tau") if tau is None else tau      # (meta-GGA: the kinetic energy density beside rho)
        if n_bands is None:
            n_bands = default_n_bands_bandstructure(scfres)
    else:
        basis = basis_or_scfres
        if n_bands is None:
            n_bands = default_n_bands_bandstructure(basis.model)
    _refuse_unsupported(basis, "compute_bands")
    if rho is None and any(t in basis.model.term_types for t in ("Hartree", "Xc")):
        raise ValueError("If a non-linear term is present in the model the converged density is required to compute "
                         "bands. Either pass the self-consistent density as the rho keyword argument or use "
                         "compute_bands(scfres, ...).")
    kinter = None
    kgrid = kgrid_or_kpath
    if isinstance(kgrid, KPath):
        kinter = kpath_interpolate(basis.model, kgrid, kline_density)
        nk = len(kinter["kcoords"])
        kgrid = ExplicitKpoints([list(k) for k in kinter["kcoords"]], [1.0 / nk] * nk)
    if not isinstance(kgrid, (ExplicitKpoints, MonkhorstPack)):
        raise TypeError("compute_bands: the k-points are an ExplicitKpoints, a MonkhorstPack or a KPath")
    n_bands, n_extra = int(n_bands), int(n_extra)
    basis._require_gpu()
    if rho is None:
        rho = guess_density(basis)

    if kchunk is None:
        bs_basis = _basis_on(basis, kgrid)
        eig = _solve(bs_basis, rho, n_bands, n_extra, tol, seed, diag_kwargs, hubbard_n, tau)
        X = eig.pop("X")
        eigenvalues, psi, diag = eig["λ"], X if keep_psi else None, [eig]
    else:
        kchunk = int(kchunk)
        if kchunk < 1:
            raise ValueError("kchunk must be at least 1")
        bs_basis = _basis_on(basis, kgrid, build_terms=False)           # the k-points (reduced as the basis would)
        kc, kw = bs_basis.kcoords_global, bs_basis.kweights_global
        n_spin = basis.model.n_spin_components
        per_spin = [([], []) for _ in range(n_spin)]
        diag = []
        for c0 in range(0, len(kc), kchunk):
            sub = ExplicitKpoints([list(k) for k in kc[c0:c0 + kchunk]], list(kw[c0:c0 + kchunk]))
            cb = _basis_on(basis, sub)
            eig = _solve(cb, rho, n_bands, n_extra, tol, seed + c0, diag_kwargs, hubbard_n, tau)
            nc = len(sub.kcoords)
            for s in range(n_spin):
                per_spin[s][0].extend(eig["λ"][s * nc:(s + 1) * nc])
                if keep_psi:
                    per_spin[s][1].extend(X.clone() for X in eig["X"][s * nc:(s + 1) * nc])
            eig.pop("X")                                                # (sliced views of the n_bands + n_extra blocks)
            diag.append(eig)
            del cb, eig                                                 # the chunk's k-blocks and LOBPCG workspaces go
            gc.collect()                                                # (basis <-> k-point reference cycles: now, not later)
        eigenvalues = [e for s in range(n_spin) for e in per_spin[s][0]]
        psi = [x for s in range(n_spin) for x in per_spin[s][1]] if keep_psi else None
    occupation = None if eF is None else _occupations(basis.model, eigenvalues, eF)
    out = dict(basis=bs_basis, eigenvalues=eigenvalues, rho=rho, eF=eF, occupation=occupation, diagonalization=diag,
               converged=all(d["converged"] for d in diag), seed=seed)
    if keep_psi:
        out["psi"] = psi
    if kinter is not None:
        out["kinter"] = kinter
    return out


# ------------------------------------------------------------------------------------------ atomic orbitals
def _orbital_plan(model, isonmanifold):
    """Which orbitals: per atom the selected (l, n) of its pseudopotential, the labels in the reference's column order
    (atom, l, n, m; dos.jl:167-186), and the species groups the projector builder takes (same pseudopotential, same
    selection)."""
    selected, labels = [], []
    for iatom, atom in enumerate(model.atoms):
        psp = atom.psp
        count = getattr(psp, "count_n_pswfc", None)
        if count is None or count() == 0:
            raise ValueError(f"atom {iatom} ({atom.symbol}): its pseudopotential ({type(psp).__name__}) carries no "
                             "pseudo-atomic orbitals (PP_PSWFC of a UPF file) to project on")
        sel = []
        for l in range(psp.lmax + 1):
            for n in range(1, psp.count_n_pswfc_radial(l) + 1):
                label = psp.pswfc_label(n, l)
                if isonmanifold is not None and not isonmanifold(dict(iatom=iatom, species=atom.symbol, label=label)):
                    continue
                sel.append((l, n))
                for m in range(-l, l + 1):
                    labels.append(dict(iatom=iatom, species=atom.symbol, n=n, l=l, m=m, label=label))
        selected.append(tuple(sel))
    if not labels:
        raise ValueError("atomic_orbital_projectors: no orbital selected")
    groups = {}
    for iatom, atom in enumerate(model.atoms):
        if selected[iatom]:
            groups.setdefault((id(atom.psp), selected[iatom]), []).append(iatom)
    return selected, labels, list(groups.values())


def _orbital_matrix(basis, kpt, plan, positions):
    """Phi of one k-point, (n_proj, n_G) on the device == column-major n_G x n_proj, Loewdin-orthonormalised."""
    model = basis.model
    selected, labels, groups = plan
    q =torch.linalg.norm(kpt.Gplusk_cart, dim=1).contiguous()
    first = np.zeros((len(groups), 4), dtype=np.int32)
    count = np.zeros((len(groups), 4), dtype=np.int32)
    chans, species, pos, built = [], [], [], []          # built: (iatom, l, n, m) of every column the builder writes
    for s_idx, g in enumerate(groups):
        psp = model.atoms[g[0]].psp
        sel = selected[g[0]]
        for l in range(4):
            ns = [n for (ll, n) in sel if ll == l]
            first[s_idx, l], count[s_idx, l] = len(chans), len(ns)
            for n in ns:
                r, wf = psp.pswfc_channel(l, n - 1)
                chans.append(radial_transform_abi(basis, 0, l, r, wf, 0.0, q))
        for ia in g:
            species.append(s_idx)
            pos.append(np.asarray(positions[ia], dtype=float))
            for l in range(4):                          # the builder's order within an atom: (l, m, i)
                ns = [n for (ll, n) in sel if ll == l]
                built.extend((ia, l, n, m) for m in range(-l, l + 1) for n in ns)
    R = torch.stack(chans).contiguous()
    species = np.asarray(species, dtype=np.int32)
    pos = np.ascontiguousarray(np.asarray(pos, dtype=np.float64).reshape(-1, 3))
    G32 = kpt.G_vectors.to(torch.int32).contiguous()
    Bh = np.asfortranarray(model.recip_lattice, dtype=np.float64)
    kh = np.ascontiguousarray(kpt.coordinate, dtype=np.float64)
    n_p = C.c_int()
    args = (basis.handle, kpt.n_G, G32.data_ptr(), Bh.ctypes.data, kh.ctypes.data, model.unit_cell_volume, len(groups),
            R.data_ptr(), max(kpt.n_G, 1), first.ctypes.data, count.ctypes.data, len(species), species.ctypes.data,
            pos.ctypes.data)
    _lib.check(basis.lib.dftk_mi_build_projectors_radial(*args, None, kpt.n_G, C.byref(n_p)))
    if n_p.value != len(labels) or len(built) != len(labels):
        raise RuntimeError("atomic_orbital_projectors: the projector builder disagrees about the number of orbitals")
    P = torch.empty((n_p.value, kpt.n_G), dtype=torch.complex128, device=basis.device)
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_build_projectors_radial(*args, P.data_ptr(), kpt.n_G, C.byref(n_p)))
    basis.post_call()
    where = {t: i for i, t in enumerate(built)}
    perm = [where[(lab["iatom"], lab["l"], lab["n"], lab["m"])] for lab in labels]
    Phi = P if perm == list(range(len(perm))) else P[torch.tensor(perm, device=basis.device)].contiguous()
    if Phi.shape[0] > kpt.n_G:
        raise ValueError(f"{Phi.shape[0]} atomic orbitals on {kpt.n_G} plane waves: increase Ecut")
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_lowdin_ortho(basis.handle, kpt.n_G, Phi.shape[0], Phi.data_ptr(), Phi.stride(0), None))
    basis.post_call()
    return Phi


def _orbital_matrices(basis, plan, positions):
    """Generator over the k-blocks of ``basis``: (ik, kpt, Phi).  Without spin one matrix is alive at a time; with collinear
    spin the spin-down block of a k-point reuses the matrix of its spin-up partner."""
    _refuse_unsupported(basis, "atomic-orbital projections")
    basis._require_gpu()
    positions = basis.model.positions if positions is None else positions
    cache = {}
    n_k = basis.n_kcoords_local
    for ik, kpt in enumerate(basis.kpoints):
        key = ik % n_k
        if key not in cache:
            if basis.model.n_spin_components == 1:
                cache.clear()
            cache[key] = _orbital_matrix(basis, kpt, plan, positions)
        yield ik, kpt, cache[key]


def atomic_orbital_projectors(basis, isonmanifold=None, positions=None):
    """``atomic_orbital_projectors(basis; isonmanifold, positions)`` (dos.jl:122-192): per k-block the orthonormalised
    pseudo-atomic orbitals as a device tensor (n_proj, n_G) (column-major n_G x n_proj) and the labels of its columns, dicts
    with iatom, species, n, l, m, label.  ``isonmanifold`` takes a dict (iatom, species, label) and keeps the orbital where it
    returns true; the kept orbitals are then orthonormal among themselves only, as the reference warns."""
    plan = _orbital_plan(basis.model, isonmanifold)
    return [Phi for _, _, Phi in _orbital_matrices(basis, plan, positions)], plan[1]


def _accumulate(basis, psik, Phi, eig=None, weight=0.0, kind=0, temperature=0.0, eps=None, proj=None, pdos=None):
    if not (psik.is_cuda and psik.dtype == torch.complex128 and psik.stride(1) == 1 and psik.shape[1] == Phi.shape[1]):
        raise ValueError("orbital blocks are (n_bands, n_G) complex128 device tensors")
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_pdos_accumulate(
        basis.handle, Phi.shape[1], psik.shape[0], psik.data_ptr(), psik.stride(0), Phi.shape[0], Phi.data_ptr(),
        Phi.stride(0), None if eig is None else eig.ctypes.data, float(weight), int(kind), float(temperature),
        0 if eps is None else len(eps), None if eps is None else eps.ctypes.data,
        None if proj is None else proj.data_ptr(), None if pdos is None else pdos.data_ptr()))
    basis.post_call()


def atomic_orbital_projections(basis, psi, isonmanifold=None, positions=None):
    """``atomic_orbital_projections(basis, psi; ...)`` (dos.jl:194-212): per k-block the (n_bands, n_proj) device tensor
    |<phi_p, psi_n>|^2 (the fat-band weights), and the labels."""
    plan = _orbital_plan(basis.model, isonmanifold)
    out = []
    for ik, _, Phi in _orbital_matrices(basis, plan, positions):
        proj = torch.empty((psi[ik].shape[0], Phi.shape[0]), dtype=torch.float64, device=basis.device)
        _accumulate(basis, psi[ik], Phi, proj=proj)
        out.append(proj)
    return out, plan[1]


def compute_pdos(eps, basis_or_bands, psi=None, eigenvalues=None, positions=None, smearing=None, temperature=None):
    """``compute_pdos(eps, basis, psi, eigenvalues; positions, smearing, temperature)`` or ``compute_pdos(eps, bands)``
    (dos.jl:70-120).  Returns a dict: ``pdos`` (n_eps, n_proj, n_spin), ``projector_labels``, ``eps``."""
    if isinstance(basis_or_bands, dict):
        bands = basis_or_bands
        basis = bands["basis"]
        psi = bands["psi"] if psi is None else psi
        eigenvalues = bands["eigenvalues"] if eigenvalues is None else eigenvalues
    else:
        basis = basis_or_bands
    model = basis.model
    smearing = smearing or model.smearing
    temperature = model.temperature if temperature is None else temperature
    if temperature == 0 or smearing == "none":
        raise ValueError("compute_pdos only supports finite temperature")
    if smearing not in SMEARING_KINDS:
        raise NotImplementedError(f"smearing {smearing}")
    if psi is None or eigenvalues is None:
        raise ValueError("compute_pdos needs the orbitals and the eigenvalues")
    eps = np.ascontiguousarray(np.atleast_1d(np.asarray(eps, dtype=np.float64)))
    plan = _orbital_plan(model, None)
    pdos, labels = None, plan[1]
    for ik, kpt, Phi in _orbital_matrices(basis, plan, positions):
        if pdos is None:
            pdos = torch.zeros((model.n_spin_components, Phi.shape[0], len(eps)), dtype=torch.float64, device=basis.device)
        eig = np.ascontiguousarray(np.asarray(eigenvalues[ik], dtype=np.float64)[:psi[ik].shape[0]])
        if len(eig) != psi[ik].shape[0]:
            raise ValueError(f"k-block {ik}: fewer eigenvalues than orbitals")
        _accumulate(basis, psi[ik], Phi, eig=eig, weight=model.filled_occupation * basis.kweights[ik],
                    kind=SMEARING_KINDS[smearing], temperature=temperature, eps=eps, pdos=pdos[kpt.spin - 1])
    basis.sync()
    return dict(pdos=pdos.permute(2, 1, 0).cpu().numpy().copy(), projector_labels=labels, eps=eps)


def sum_pdos(pdos_res, filters):
    """``sum_pdos(pdos_res, projector_filters)`` (dos.jl:214-238): the sum of the columns whose label any filter accepts,
    shape (n_eps, n_spin)."""
    pdos = np.asarray(pdos_res["pdos"])
    out = np.zeros((pdos.shape[0], pdos.shape[2]))
    for j, orb in enumerate(pdos_res["projector_labels"]):
        if any(f(orb) for f in filters):
            out += pdos[:, j, :]
    return out
