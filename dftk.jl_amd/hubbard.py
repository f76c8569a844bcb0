"""DFT+U: the Hubbard term of Dudarev et al. in its rotationally invariant form (src/terms/hubbard.jl,
``symmetrize_hubbard_n`` of src/symmetry.jl:425-452, ``wigner_d_matrix`` of src/common/spherical_harmonics.jl:76-96).

    E = filled_occ sum_{manifold, sigma, I} U / 2 Re tr[n (1 - n)],        n = hubbard_n[manifold][sigma, I, I]
    V = Phi_k D_sigma Phi_k',   D_sigma = blockdiag(U / 2 (1 - 2 n))

``Phi`` are the Loewdin-orthonormalised pseudo-atomic orbitals of bands.py (all orbitals of all atoms are orthonormalised
together, then the manifolds' columns are kept; column order: manifold, atom, m).  The occupation matrices are accumulated on
the device (``dftk_mi_hubbard_occupation``, csrc/hubbard_kernels.hip).  The operator rides in the k-block's projector slot
behind the nonlocal term, like the compressed exchange operator; the library's coupling matrix is real, so each Hermitian
block n = V nu V' is diagonalised on the host (at most 7 x 7) and the slot receives the rotated orbitals Phi V
(``dftk_mi_hubbard_rotate``) with the real diagonal couplings U / 2 (1 - 2 nu):
Phi (U / 2)(1 - 2 n) Phi' = (Phi V) diag(U / 2 (1 - 2 nu)) (Phi V)' exactly, whatever the degeneracies of nu.

Atom indices are 0-based; U is in Hartree.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .symmetry import SYMMETRY_TOLERANCE, find_symmetry_preimage

MAX_L = 3                     # blocks of at most 7 orbitals (dftk_mi_hubbard_occupation)
# largest |Im n| a Gamma-real block accepts: n has entries of order 1 and its rounding error is (n_bands + 4) 2^-52 of that
# (some 1e-14 with the error of the projections); 1e-10 is far above it and changes no eigenvalue by more than U x 1e-10
GAMMA_REAL_IMAG_TOL = 1e-10


# ------------------------------------------------------------------------------------------ the public objects
class OrbitalManifold:
    """``OrbitalManifold(atoms, projectors)`` (hubbard.jl:19-28): the atomic sites -- an ``ElementPsp``, a symbol string or
    a list of atom indices -- and the pseudo-atomic orbital -- a label ("3D") or the pair (l, i), also as ``dict(l=, i=)``;
    i is 1-based like every ``eval_psp_*`` function."""

    def __init__(self, atoms, projectors):
        if hasattr(atoms, "symbol") and hasattr(atoms, "psp"):
            atoms = atoms.symbol
        if isinstance(atoms, str):
            self.atoms = atoms
        else:
            self.atoms = tuple(int(i) for i in atoms)
        if isinstance(projectors, str):
            self.projectors = projectors
        elif isinstance(projectors, dict):
            self.projectors = (int(projectors["l"]), int(projectors["i"]))
        else:
            l, i = projectors
            self.projectors = (int(l), int(i))

    def __repr__(self):
        return f"OrbitalManifold({self.atoms!r}, {self.projectors!r})"

    def __eq__(self, other):
        return (isinstance(other, OrbitalManifold) and self.atoms == other.atoms and self.projectors == other.projectors)

    def __hash__(self):
        return hash((self.atoms, self.projectors))


@dataclass(frozen=True)
class ResolvedOrbitalManifold:
    """hubbard.jl:37-42: the manifold with its atoms and its orbital looked up in a model."""
    psp: object
    iatoms: tuple
    l: int
    i: int


class Hubbard:
    """``Hubbard(manifold => U, ...)`` as ``Hubbard((manifold, U), ...)``, ``Hubbard([manifolds], [U])`` or ``Hubbard()``
    (hubbard.jl:109-126).  In a term list it stands for the name "Hubbard"; the model keeps the object as
    ``model.hubbard``."""

    def __init__(self, *args):
        if len(args) == 2 and all(isinstance(a, (list, tuple)) for a in args) \
                and all(isinstance(m, OrbitalManifold) for m in args[0]):
            manifolds, U = list(args[0]), list(args[1])
            if len(manifolds) != len(U):
                raise ValueError(f"Number of U values ({len(U)}) must match number of manifolds ({len(manifolds)}).")
        else:
            manifolds, U = [], []
            for pair in args:
                if not (isinstance(pair, (list, tuple)) and len(pair) == 2 and isinstance(pair[0], OrbitalManifold)):
                    raise TypeError("Hubbard takes (manifold, U) pairs, or a list of manifolds and a list of U values")
                manifolds.append(pair[0])
                U.append(pair[1])
        self.manifolds = tuple(manifolds)
        self.U = tuple(float(u) for u in U)

    def __repr__(self):
        return "Hubbard(" + ", ".join(f"({m!r}, {u!r})" for m, u in zip(self.manifolds, self.U)) + ")"


def resolve_hubbard_manifold(manifold, model):
    """hubbard.jl:44-88; the reference's errors as ``ValueError``, a manifold beyond l = 3 as ``NotImplementedError``."""
    if isinstance(manifold.atoms, str):
        iatoms = tuple(i for i, a in enumerate(model.atoms) if getattr(a, "symbol", None) == manifold.atoms)
    else:
        iatoms = tuple(manifold.atoms)
    if not iatoms:
        raise ValueError("Orbital manifold has no atoms.")
    if any(i < 0 or i >= len(model.atoms) for i in iatoms):
        raise ValueError(f"Orbital manifold names atoms {list(iatoms)}, the model has {len(model.atoms)}.")
    psp = getattr(model.atoms[iatoms[0]], "psp", None)
    for i in iatoms:
        other = getattr(model.atoms[i], "psp", None)
        if other is None:
            raise ValueError("Orbital manifold elements must have a psp.")
        if other is not psp:
            raise ValueError(f"Orbital manifold contains multiple psps: {psp.identifier} and {other.identifier}")
    # the atoms must be mapped onto each other by every symmetry of the model: the manifold would be a valid atom group
    positions = [np.asarray(model.positions[i], dtype=float) for i in iatoms]
    for symop in model.symmetries:
        W, w = np.asarray(symop.W, dtype=float), np.asarray(symop.w, dtype=float)
        for coord in positions:
            image = W @ coord + w
            if not any(np.all(np.abs((image - c) - np.round(image - c)) <= SYMMETRY_TOLERANCE) for c in positions):
                raise ValueError("Inconsistency between orbital manifold and model symmetries: Cannot map the atom at "
                                 f"position {coord} to another atom of the manifold under the symmetry operation "
                                 f"(W, w):\n({W}, {w})")
    if isinstance(manifold.projectors, str):
        find = getattr(psp, "find_pswfc", None)
        if find is None:
            raise ValueError(f"the pseudopotential of the manifold ({type(psp).__name__}) carries no pseudo-atomic "
                             "orbitals (PP_PSWFC of a UPF file)")
        l, i = find(manifold.projectors)
    else:
        l, i = manifold.projectors
    if l > MAX_L:
        raise NotImplementedError(f"Hubbard manifolds with l = {l} are not implemented (l <= {MAX_L})")
    return ResolvedOrbitalManifold(psp, iatoms, int(l), int(i))


def refuse(model, what):
    """Entry points that have no Hubbard term yet."""
    if getattr(model, "hubbard", None) is not None:
        raise NotImplementedError(f"{what} is not implemented for models with a Hubbard term (DFT+U)")


def refuse_sharded(basis, what):
    if basis.comm_pw.size > 1:
        raise NotImplementedError(f"{what} on a plane-wave sharded basis (comm_pw.size > 1) is not implemented")
    if basis.comm_kpts.size > 1:
        raise NotImplementedError(f"{what} on a k-point sharded basis (comm_kpts.size > 1) is not implemented")


# ------------------------------------------------------------------------------------------ Wigner matrices, symmetrisation
def _wigner_directions(n):
    """n unit vectors on a golden-angle spiral: a fixed set in general position (no two on a common symmetry element)."""
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    phi = i * math.pi * (3 - math.sqrt(5)) + 0.3
    s = np.sqrt(1 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


def wigner_d_matrix(l, Wcart):
    """``wigner_d_matrix(l, Wcart)`` (spherical_harmonics.jl:76-96): the matrix D with Y_lm1(W r) = sum_m2 D[m1, m2] Y_lm2(r)
    for the real spherical harmonics, by least squares over a fixed set of 4 l + 4 directions (the reference draws 2 l + 2
    seeded random ones)."""
    import torch
    from .psp import solid_harmonic_real
    Wcart = np.asarray(Wcart, dtype=float)
    if l == 0:
        return np.ones((1, 1))
    r = _wigner_directions(4 * l + 4)
    r0 = r @ Wcart.T
    ms = range(-l, l + 1)
    A = np.stack([solid_harmonic_real(l, m, torch.from_numpy(r)).numpy() for m in ms])
    B = np.stack([solid_harmonic_real(l, m, torch.from_numpy(r0)).numpy() for m in ms])
    kappa = np.linalg.cond(A)
    assert kappa < 100.0, f"The Wigner matrix computation is badly conditioned. cond(A) = {kappa}"
    return np.linalg.lstsq(A.T, B.T, rcond=None)[0].T           # D A = B


def symmetrize_hubbard_n(model, manifold, hubbard_n, symmetries, tol_symmetry=SYMMETRY_TOLERANCE):
    """``symmetrize_hubbard_n`` (symmetry.jl:425-452): the atom-diagonal blocks averaged over the symmetry operations, the
    cross-atom blocks zero.  ``hubbard_n``: (n_spin, n_atoms, n_atoms, 2 l + 1, 2 l + 1)."""
    n = np.asarray(hubbard_n, dtype=complex)
    positions = [np.asarray(model.positions[i], dtype=float) for i in manifold.iatoms]
    n_spin, n_atoms = n.shape[0], n.shape[1]
    lattice = np.asarray(model.lattice, dtype=float)
    inv_lattice = np.linalg.inv(lattice)
    out = np.zeros_like(n)
    for symop in symmetries:
        Wcart = lattice @ np.asarray(symop.W, dtype=float) @ inv_lattice
        WigD = wigner_d_matrix(manifold.l, Wcart)
        for iatom in range(n_atoms):
            sym_atom = find_symmetry_preimage(positions, positions[iatom], symop, tol_symmetry)
            for s in range(n_spin):
                out[s, iatom, iatom] += WigD.T @ n[s, sym_atom, sym_atom] @ WigD
    return out / len(symmetries)


# ------------------------------------------------------------------------------------------ term set-up
class HubbardTerm:
    """``TermHubbard`` (hubbard.jl:141-147): resolved manifolds, U, per k-block the manifolds' orbitals as a device tensor
    (n_cols, n_G), and the blocks (first column, size) in the column order manifold, atom, m."""


def hubbard_term(basis):
    """The term of ``basis`` (built on first use, then kept on the basis); None for a model without Hubbard term or with an
    empty one."""
    import torch
    from .bands import _orbital_matrices, _orbital_plan
    hub = getattr(basis.model, "hubbard", None)
    if hub is None or not hub.U:
        return None
    term = getattr(basis, "_hubbard_term", None)
    if term is not None:
        return term
    refuse_sharded(basis, "the Hubbard term")
    model = basis.model
    term = HubbardTerm()
    term.manifolds = [resolve_hubbard_manifold(m, model) for m in hub.manifolds]
    term.U = list(hub.U)
    plan = _orbital_plan(model, None)
    where = {(lab["iatom"], lab["l"], lab["n"], lab["m"]): j for j, lab in enumerate(plan[1])}
    cols, first, size = [], [], []
    for man in term.manifolds:
        for ia in man.iatoms:
            first.append(len(cols))
            size.append(2 * man.l + 1)
            for m in range(-man.l, man.l + 1):
                key = (ia, man.l, man.i, m)
                if key not in where:
                    raise ValueError(f"Projector for the manifold (l = {man.l}, i = {man.i}) not found on atom {ia}.")
                cols.append(where[key])
    term.first = np.ascontiguousarray(first, dtype=np.int32)
    term.size = np.ascontiguousarray(size, dtype=np.int32)
    term.offset = np.concatenate([[0], np.cumsum(term.size.astype(np.int64) ** 2)])
    term.n_cols = len(cols)
    index = torch.tensor(cols, device=basis.device)
    term.Phi, made = [], {}
    n_k = basis.n_kcoords_local
    for ik, _, Phi in _orbital_matrices(basis, plan, None):
        if ik % n_k not in made:                                # (the spin-down block shares its spin-up partner's matrix)
            made[ik % n_k] = Phi.index_select(0, index).contiguous()
        term.Phi.append(made[ik % n_k])
    basis._hubbard_term = term
    return term


def _blocks(term):
    """(manifold index, atom index within the manifold, block index) of every block"""
    out, b = [], 0
    for iman, man in enumerate(term.manifolds):
        for ia in range(len(man.iatoms)):
            out.append((iman, ia, b))
            b += 1
    return out


# ------------------------------------------------------------------------------------------ occupation matrices
def compute_hubbard_n(basis, psi, occupation):
    """``compute_hubbard_n(term, basis, psi, occupation)`` (hubbard.jl:186-232): one array per manifold,
    (n_spin, n_atoms, n_atoms, 2 l + 1, 2 l + 1) complex, symmetrised with ``basis.symmetries``; only the atom-diagonal
    blocks are filled.  One ``dftk_mi_hubbard_occupation`` call per k-block into one device buffer per spin, one fetch."""
    import torch
    from . import _lib
    model = basis.model
    if getattr(model, "hubbard", None) is None:
        raise ValueError("compute_hubbard_n: the model of this basis has no Hubbard term")
    term = hubbard_term(basis)
    if term is None:
        return []
    basis._require_gpu()
    n_spin = model.n_spin_components
    n_d = torch.zeros((n_spin, int(term.offset[-1])), dtype=torch.complex128, device=basis.device)
    for ik, kpt in enumerate(basis.kpoints):
        psik, Phi = psi[ik], term.Phi[ik]
        if not (psik.is_cuda and psik.dtype == torch.complex128 and psik.stride(1) == 1 and psik.shape[1] == Phi.shape[1]):
            raise ValueError("orbital blocks are (n_bands, n_G) complex128 device tensors")
        occ = np.asarray(occupation[ik], dtype=np.float64)[:psik.shape[0]]
        if len(occ) != psik.shape[0]:
            raise ValueError(f"k-block {ik}: fewer occupations than orbitals")
        w = np.ascontiguousarray(basis.kweights[ik] * occ / model.filled_occupation)
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_hubbard_occupation(
            basis.handle, Phi.shape[1], psik.shape[0], psik.data_ptr(), psik.stride(0), Phi.shape[0], Phi.data_ptr(),
            Phi.stride(0), w.ctypes.data, len(term.first), term.first.ctypes.data, term.size.ctypes.data,
            n_d[kpt.spin - 1].data_ptr()))
        basis.post_call()
    basis.sync()
    flat = n_d.cpu().numpy()
    out = []
    for man in term.manifolds:
        d = 2 * man.l + 1
        out.append(np.zeros((n_spin, len(man.iatoms), len(man.iatoms), d, d), dtype=complex))
    for iman, ia, b in _blocks(term):
        d = int(term.size[b])
        for s in range(n_spin):
            out[iman][s, ia, ia] = flat[s, term.offset[b]:term.offset[b + 1]].reshape(d, d).T      # (column-major blocks)
    return [symmetrize_hubbard_n(model, man, n, basis.symmetries) for man, n in zip(term.manifolds, out)]


# ------------------------------------------------------------------------------------------ energy and operator
@dataclass
class HubbardOperator:
    """What a Hamiltonian block keeps of the Hubbard term: the rotated orbitals (n_cols, n_G) and their real couplings."""
    rows: object
    couplings: np.ndarray


def hubbard_energy(term, hubbard_n, filled_occ):
    """filled_occ sum U / 2 Re tr[n (1 - n)] over manifolds, spins and atoms (hubbard.jl:169-178)."""
    E = 0.0
    for iman, ia, _ in _blocks(term):
        n_man = np.asarray(hubbard_n[iman])
        for s in range(n_man.shape[0]):
            n = n_man[s, ia, ia]
            E += filled_occ * 0.5 * term.U[iman] * float(np.real(np.trace(n @ (np.eye(n.shape[0]) - n))))
    return E


def _check_hubbard_n(term, hubbard_n, n_spin):
    if len(hubbard_n) != len(term.manifolds):
        raise ValueError(f"hubbard_n holds {len(hubbard_n)} arrays, the term has {len(term.manifolds)} manifolds")
    for man, n in zip(term.manifolds, hubbard_n):
        d = 2 * man.l + 1
        want = (n_spin, len(man.iatoms), len(man.iatoms), d, d)
        if tuple(np.shape(n)) != want:
            raise ValueError(f"hubbard_n of a manifold has shape {tuple(np.shape(n))}, expected {want}")


def hubbard_energy_ops(basis, hubbard_n, want_ops=True):
    """``ene_ops(term::TermHubbard, ...)`` (hubbard.jl:149-184) -> (E, {k-block index: HubbardOperator} | None).  Per spin
    the blocks U / 2 (1 - 2 n) are diagonalised on the host; one ``dftk_mi_hubbard_rotate`` call per k-block writes the
    rotated orbitals."""
    import torch
    from . import _lib
    term = hubbard_term(basis)
    model = basis.model
    n_spin = model.n_spin_components
    _check_hubbard_n(term, hubbard_n, n_spin)
    E = hubbard_energy(term, hubbard_n, model.filled_occupation)
    if not want_ops:
        return E, None
    basis._require_gpu()
    rotations = {}

    def rotation(spin, real):
        """packed V and the couplings of one spin channel.  ``real`` (Gamma-real blocks, which iterate real orbitals): n must
        be real symmetric -- as it is for real orbitals at Gamma -- so that V is real, the rotated orbitals stay real
        functions and the block applies the operator the energy belongs to; an imaginary part beyond rounding is refused."""
        if (spin, real) not in rotations:
            V = np.zeros(int(term.offset[-1]), dtype=np.complex128)
            couplings = np.zeros(term.n_cols)
            for iman, ia, b in _blocks(term):
                n = np.asarray(hubbard_n[iman])[spin - 1, ia, ia]
                n = (n + n.conj().T) / 2
                if real:
                    if np.max(np.abs(n.imag)) > GAMMA_REAL_IMAG_TOL:
                        raise ValueError(f"hubbard_n has an imaginary part of {np.max(np.abs(n.imag)):.2e} (occupations "
                                         "of a k-mesh that is not closed under k -> -k, or not converged): a Gamma-real "
                                         "block cannot apply this operator; build the basis with gamma_real=False")
                    n = n.real
                nu, Vb = np.linalg.eigh(n)
                V[term.offset[b]:term.offset[b + 1]] = Vb.T.reshape(-1)                            # (column-major blocks)
                p0 = int(term.first[b])
                couplings[p0:p0 + len(nu)] = 0.5 * term.U[iman] * (1 - 2 * nu)
            rotations[(spin, real)] = (V, couplings)
        return rotations[(spin, real)]

    ops = {}
    for ik, kpt in enumerate(basis.kpoints):
        Phi = term.Phi[ik]
        rows = torch.empty_like(Phi)
        Vs, couplings = rotation(kpt.spin, bool(getattr(kpt, "gamma_real", False)))
        basis.pre_call()
        _lib.check(basis.lib.dftk_mi_hubbard_rotate(basis.handle, Phi.shape[1], len(term.first), term.first.ctypes.data,
                                                    term.size.ctypes.data, Phi.data_ptr(), Phi.stride(0), Vs.ctypes.data,
                                                    rows.data_ptr(), rows.stride(0)))
        basis.post_call()
        ops[ik] = HubbardOperator(rows=rows, couplings=couplings.copy())
    return E, ops


def bind_projector_rows(basis, ik, op=None):
    """Make the k-block's projector slot hold [P_nl; rows] with couplings blockdiag(D, diag(couplings)) (``op`` None: the
    nonlocal term alone) -- the sibling of ``exchange.bind_projectors`` for rows with couplings of their own.  The buffer
    has room for the rows: a rebind copies them, not P."""
    import torch
    from . import _lib
    kpt, T = basis.kpoints[ik], basis.terms
    P = T.P[ik] if T is not None and T.P is not None else None
    n_p = 0 if P is None else P.shape[0]
    basis.pre_call()
    if op is None:
        if n_p == 0:
            _lib.check(basis.lib.dftk_mi_kblock_set_projectors(kpt.handle, 0, None, kpt.n_G, None))
        else:
            _lib.check(basis.lib.dftk_mi_kblock_set_projectors(kpt.handle, n_p, P.data_ptr(), kpt.n_loc,
                                                               kpt._keep["D"].ctypes.data))
        return
    n_h = op.rows.shape[0]
    buf = old = kpt._keep.get("hubbard_P")
    if buf is None or buf.shape[0] != n_p + n_h:
        # (the library may still read the old buffer: `old` holds it until set_projectors below has synchronised)
        buf = torch.empty((n_p + n_h, kpt.n_G), dtype=torch.complex128, device=op.rows.device)
        if n_p:
            buf[:n_p] = P
        kpt._keep["hubbard_P"] = buf
    buf[n_p:] = op.rows
    D = np.zeros((n_p + n_h, n_p + n_h), order="F")
    if n_p:
        D[:n_p, :n_p] = T.D
    D[n_p:, n_p:] = np.diag(op.couplings)
    kpt._keep["hubbard_D"] = D
    basis.pre_call()
    _lib.check(basis.lib.dftk_mi_kblock_set_projectors(kpt.handle, n_p + n_h, buf.data_ptr(), kpt.n_G, D.ctypes.data))
    del old
