"""Physics specification: ``Model``, ``ElementPsp``, standard models, supercells, k-grids.

Mirrors the parts of src/Model.jl, src/elements.jl, src/standard_models.jl:45-61,116-131,220,
src/supercell.jl:5-20 and src/bzmesh.jl:4-48 that the SCF hot path consumes.  Symmetry
detection, k-mesh reduction and density symmetrisation live in symmetry.py (``symmetries=True``); the default
is ``symmetries=False`` (explicit lists / unreduced Monkhorst-Pack meshes).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from .exchange import Coulomb
from .hubbard import Hubbard
from .psp import AMU_IN_ELECTRON_MASSES, ATOMIC_NUMBER, ATOMIC_WEIGHT, PspHgh, load_psp


@dataclass(eq=False)
class ElementPsp:
    symbol: str
    psp: PspHgh
    mass: float | None = None      # atomic units (electron masses); default: the standard atomic weight of ``symbol``

    def __post_init__(self):
        if self.mass is None and self.symbol in ATOMIC_WEIGHT:
            self.mass = ATOMIC_WEIGHT[self.symbol] * AMU_IN_ELECTRON_MASSES

    @property
    def charge_nuclear(self):
        return ATOMIC_NUMBER[self.symbol]

    @property
    def charge_ionic(self):
        return self.psp.Zion

    n_elec_valence = charge_ionic

    @property
    def n_elec_core(self):
        return self.charge_nuclear - self.psp.Zion


@dataclass(frozen=True)
class ExactExchange:
    """``ExactExchange(; scaling_factor, kernel)`` (terms/exact_exchange.jl:19-22): the only term that carries parameters.
    In a term list it stands for the name "ExactExchange"; the model keeps the object as ``model.exact_exchange``."""
    scaling_factor: float = 1.0
    kernel: object = field(default_factory=Coulomb)


@dataclass(frozen=True)
class PBE0:
    """``PBE0(; exx_fraction, exx_kernel)`` (standard_models.jl): ``functionals=PBE0()`` of ``model_DFT`` expands to
    (1 - a) gga_x_pbe + gga_c_pbe + ExactExchange(a, kernel) with a = 0.25 and the Coulomb kernel unless given."""
    exx_fraction: float | None = None
    exx_kernel: object = None


def compute_recip_lattice(lattice):
    """structure.jl:24-26 (lattice vectors are columns)."""
    return 2 * math.pi * np.linalg.inv(np.asarray(lattice, dtype=float).T)


MGGA_FUNCTIONALS = ("mgga_x_scan", "mgga_c_scan")      # the functionals of tau = 1/2 sum f |grad psi|^2 with a kernel


def refuse_meta_gga(model_or_basis, what):
    """``what`` does not know the kinetic energy density or the div-A-grad term: NotImplementedError for a meta-GGA model"""
    model = getattr(model_or_basis, "model", model_or_basis)
    if getattr(model, "uses_tau", False):
        raise NotImplementedError(f"{what} is not implemented for meta-GGA functionals {model.functionals}")


class Model:
    """``Model`` (src/Model.jl): lattice (columns), atoms, fractional positions, term list, XC functionals,
    temperature / smearing, and the spin polarisation -- ``:none`` or ``:collinear`` (Model.jl:29-39), inferred from the
    per-atom initial ``magnetic_moments`` (mu_B, z components) as ``determine_spin_polarization`` does."""

    def __init__(self, lattice, atoms, positions, terms, functionals=("lda_x", "lda_c_pw"),
                 temperature=0.0, smearing=None, n_electrons=None, symmetries=False, magnetic_moments=(),
                 spin_polarization=None, functional_scales=None, use_nlcc=True):
        self.lattice = np.asarray(lattice, dtype=float)
        self.atoms = list(atoms)
        self.positions = [np.asarray(p, dtype=float) for p in positions]
        if len(self.atoms) != len(self.positions):
            raise ValueError("Length of atoms and positions vectors need to agree.")
        # terms are names; ExactExchange alone has parameters: the object (or the bare name: the defaults) is kept apart
        exx = [t for t in terms if isinstance(t, ExactExchange) or t == "ExactExchange"]
        if len(exx) > 1:
            raise ValueError("Model with more than one ExactExchange term not supported.")
        self.exact_exchange = (ExactExchange() if exx[0] == "ExactExchange" else exx[0]) if exx else None
        # likewise the Hubbard term (hubbard.py): the object carries the manifolds and their U
        hub = [t for t in terms if isinstance(t, Hubbard) or (isinstance(t, str) and t == "Hubbard")]
        if len(hub) > 1:
            raise ValueError("Model with more than one Hubbard term not supported.")
        self.hubbard = (Hubbard() if isinstance(hub[0], str) else hub[0]) if hub else None
        if self.hubbard is not None and self.exact_exchange is not None:
            raise NotImplementedError("a Hubbard term together with ExactExchange is not implemented (both use the "
                                      "k-block's projector slot)")
        self.term_types = tuple("ExactExchange" if isinstance(t, ExactExchange) else "Hubbard" if isinstance(t, Hubbard)
                                else t for t in terms)
        if not self.term_types:
            raise ValueError("Model without terms not supported.")
        self.functionals = tuple(functionals)
        # multiplier of every functional in the Xc term (1 unless a hybrid scales its exchange part)
        self.functional_scales = (tuple(float(s) for s in functional_scales) if functional_scales is not None
                                  else (1.0,) * len(self.functionals))
        if len(self.functional_scales) != len(self.functionals):
            raise ValueError("one scale per functional")
        # Xc(...; use_nlcc) (xc.jl:9-17): whether the core densities of the pseudopotentials join rho in the Xc term
        self.use_nlcc = bool(use_nlcc)
        self.temperature = float(temperature)
        self.smearing = smearing if smearing is not None else ("fermi_dirac" if temperature > 0 else "none")
        self.recip_lattice = compute_recip_lattice(self.lattice)
        self.unit_cell_volume = abs(np.linalg.det(self.lattice))
        self.n_electrons = int(sum(a.charge_ionic for a in self.atoms)) if n_electrons is None else n_electrons
        self.magnetic_moments = tuple(float(np.asarray(m, dtype=float).reshape(-1)[-1]) for m in magnetic_moments)
        if self.magnetic_moments and len(self.magnetic_moments) != len(self.atoms):
            raise ValueError("Length of atoms and magnetic_moments vectors need to agree.")
        if spin_polarization is None:
            spin_polarization = "collinear" if any(m != 0 for m in self.magnetic_moments) else "none"
        if spin_polarization not in ("none", "collinear"):
            raise NotImplementedError(f"spin_polarization = {spin_polarization!r} (Model.jl:190-192: :full is not "
                                      "supported by the reference either; :spinless is outside the hot path)")
        self.spin_polarization = spin_polarization
        self.n_spin_components = 2 if spin_polarization == "collinear" else 1          # Model.jl:196, :366-372
        # meta-GGA: SCAN, unpolarised, alone with the standard terms -- everything else is refused here, by name
        self.uses_tau = any(f in MGGA_FUNCTIONALS for f in self.functionals)
        other = [f for f in self.functionals if f.startswith(("mgga_", "hyb_mgga_")) and f not in MGGA_FUNCTIONALS]
        if other:
            raise NotImplementedError(f"meta-GGA: {MGGA_FUNCTIONALS} (SCAN) are the functionals with a kernel, got {other}")
        if self.uses_tau:
            if spin_polarization == "collinear":
                raise NotImplementedError("meta-GGA with collinear spin is not implemented (the SCAN forms are unpolarised)")
            if self.hubbard is not None or self.exact_exchange is not None:
                raise NotImplementedError("meta-GGA together with a Hubbard or ExactExchange term is not implemented")
            if any(s != 1.0 for s in self.functional_scales):
                raise NotImplementedError("meta-GGA with scaled functionals (hybrids) is not implemented")
            if self.use_nlcc and any(getattr(getattr(a, "psp", None), "has_core_density", lambda: False)() for a in self.atoms):
                raise NotImplementedError("meta-GGA with a pseudopotential that carries a core correction is not implemented "
                                          "(no tau_core); pass use_nlcc=False to drop the correction")
        # atom_groups (Model.jl:169): indices of identical elements, in order of first appearance
        self.atom_groups = []
        reps = []
        for i, a in enumerate(self.atoms):
            for g, r in zip(self.atom_groups, reps):
                if r is a or (r.symbol == a.symbol and r.psp.identifier == a.psp.identifier):
                    g.append(i)
                    break
            else:
                self.atom_groups.append([i])
                reps.append(a)

        # Model.jl:104-110: True = automatic detection (symmetry.py; the reference asks Spglib), False = identity
        # only, or an explicit list of SymOp.  Default False: explicit / unreduced k-lists unless asked for.
        from . import symmetry as _sym
        if symmetries is True:
            if self.spin_polarization == "collinear" and not self.magnetic_moments:
                symmetries = [_sym.identity()]          # default_symmetries (Model.jl:330-332): the breaking is unknown
            else:
                # atoms that carry different moments are different species for the search (symmetry.jl:66-125 hands
                # the moments to Spglib)
                groups = self.atom_groups
                if self.magnetic_moments:
                    groups = []
                    for g in self.atom_groups:
                        by_m = {}
                        for i in g:
                            by_m.setdefault(round(self.magnetic_moments[i], 10), []).append(i)
                        groups.extend(by_m.values())
                symmetries = _sym.symmetry_operations(self.lattice, groups, self.positions)
        elif symmetries is False or symmetries is None:
            symmetries = [_sym.identity()]
        self.symmetries = list(symmetries)

    @property
    def filled_occupation(self):   # Model.jl:352-360
        return 1 if self.spin_polarization == "collinear" else 2


def model_atomic(lattice, atoms, positions, extra_terms=(), **kw):
    """standard_models.jl:45-61."""
    terms = ("Kinetic", "AtomicLocal", "AtomicNonlocal", "Ewald", "PspCorrection") + tuple(extra_terms)
    if kw.get("temperature", 0) != 0:          # :56-58: the total becomes the free energy E - TS
        terms = terms + ("Entropy",)
    return Model(lattice, atoms, positions, terms, **kw)


def model_DFT(lattice, atoms, positions, functionals=("lda_x", "lda_c_pw"), **kw):
    """standard_models.jl:116-131; default functionals = ``LDA()`` (:220).  ``functionals=PBE0(...)``: the hybrid.
    ``use_nlcc=False`` (the switch of the reference's ``Xc``) leaves the non-linear core correction of the pseudopotentials
    out of the Xc term."""
    if isinstance(functionals, PBE0):
        a = 0.25 if functionals.exx_fraction is None else float(functionals.exx_fraction)
        kernel = Coulomb() if functionals.exx_kernel is None else functionals.exx_kernel
        extra = tuple(kw.pop("extra_terms", ()))
        return model_atomic(lattice, atoms, positions, extra_terms=("Hartree", "Xc", ExactExchange(a, kernel)) + extra,
                            functionals=("gga_x_pbe", "gga_c_pbe"), functional_scales=(1.0 - a, 1.0), **kw)
    extra = tuple(kw.pop("extra_terms", ()))              # (e.g. a Hubbard(...) term, as the reference's extra_terms)
    return model_atomic(lattice, atoms, positions, extra_terms=("Hartree", "Xc") + extra,
                        functionals=tuple(functionals), **kw)


def model_HF(lattice, atoms, positions, exx_kernel=None, **kw):
    """``model_HF`` (standard_models.jl): the atomic model + Hartree + ExactExchange(1, exx_kernel)."""
    kernel = Coulomb() if exx_kernel is None else exx_kernel
    return model_atomic(lattice, atoms, positions, extra_terms=("Hartree", ExactExchange(1.0, kernel)), **kw)


def create_supercell(lattice, atoms, positions, supercell_size):
    """supercell.jl:5-20 (species-major, then (i,j,k) with i fastest)."""
    nx, ny, nz = supercell_size
    size = np.array([nx, ny, nz], dtype=float)
    lat = np.asarray(lattice, dtype=float) * size[None, :]
    new_atoms, new_pos = [], []
    for atom, pos in zip(atoms, positions):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    new_pos.append((np.asarray(pos, dtype=float) + np.array([i, j, k])) / size)
                    new_atoms.append(atom)
    return lat, new_atoms, new_pos


def silicon_cell(supercell=(1, 1, 1), a=10.26, functional="lda"):
    """fcc silicon of examples/silicon.jl:5-11 with the vendored HGH pseudopotential."""
    lattice = a / 2 * np.array([[0, 1, 1.0], [1, 0, 1.0], [1, 1, 0.0]])
    Si = ElementPsp("Si", load_psp("Si", functional))
    atoms, positions = [Si, Si], [np.ones(3) / 8, -np.ones(3) / 8]
    if tuple(supercell) != (1, 1, 1):
        lattice, atoms, positions = create_supercell(lattice, atoms, positions, supercell)
    return lattice, atoms, positions


@dataclass
class ExplicitKpoints:
    kcoords: list
    kweights: list


@dataclass
class MonkhorstPack:
    kgrid_size: tuple
    kshift: tuple = (0, 0, 0)

    def reducible(self) -> ExplicitKpoints:
        """bzmesh.jl:41-48; uniform weights (no symmetry reduction)."""
        size = np.array(self.kgrid_size)
        start = -np.floor((size - 1) / 2).astype(int)
        stop = np.ceil((size - 1) / 2).astype(int)
        ks = []
        for k in range(start[2], stop[2] + 1):
            for j in range(start[1], stop[1] + 1):
                for i in range(start[0], stop[0] + 1):
                    kc = (np.array(self.kshift, dtype=float) + np.array([i, j, k])) / size
                    ks.append(kc - np.floor(kc + 0.5))
        return ExplicitKpoints(ks, [1.0 / len(ks)] * len(ks))
