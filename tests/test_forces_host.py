"""Host-side pieces of compute_forces (no GPU): the Ewald forces (ewald.jl:64-168) against finite differences of
``energy_ewald``, symmetrize_forces (symmetry.jl:379-423) and the reduced -> Cartesian conversion (forces.jl:44-47)."""
import numpy as np
import pytest

import dftk_jl_amd as dftk
from dftk_jl_amd.forces import forces_red_to_cart
from dftk_jl_amd.terms import energy_ewald, energy_forces_ewald


def _displaced_si():
    lat, atoms, _ = dftk.silicon_cell()
    return lat, atoms, [np.array([1.01, 1.02, 1.03]) / 8, -np.ones(3) / 8]


def _fd_ewald(lat, charges, pos, direction, eps=1e-5):
    p = [np.asarray(x, dtype=float) + eps * d for x, d in zip(pos, direction)]
    m = [np.asarray(x, dtype=float) - eps * d for x, d in zip(pos, direction)]
    return (energy_ewald(lat, charges, p) - energy_ewald(lat, charges, m)) / (2 * eps)


def test_ewald_energy_unchanged():
    lat, atoms, pos = _displaced_si()
    q = [a.charge_ionic for a in atoms]
    E, _ = energy_forces_ewald(lat, q, pos)
    E0 = energy_ewald(lat, q, pos)
    assert abs(E - E0) <= 1e-14 * abs(E0)


@pytest.mark.parametrize("system", ["si", "three_species"])
def test_ewald_forces_match_finite_differences(system):
    if system == "si":
        lat, atoms, pos = _displaced_si()
        q = [a.charge_ionic for a in atoms]
    else:   # test/ewald.jl:59-76 style: a 3-species cell with unequal charges
        lat = np.array([[5.0, 0.3, 0.0], [0.0, 6.0, 0.4], [0.2, 0.0, 5.5]])
        pos = [np.array([0.0, 0.0, 0.0]), np.array([0.3, 0.45, 0.1]), np.array([0.62, 0.2, 0.71]),
               np.array([0.1, 0.8, 0.5])]
        q = [4.0, 1.0, 6.0, 1.0]
    _, F = energy_forces_ewald(lat, q, pos)
    rng = np.random.default_rng(1)
    for _ in range(3):
        d = rng.standard_normal((len(pos), 3))
        d /= np.linalg.norm(d)
        fd = _fd_ewald(lat, q, pos, d)
        assert abs(np.sum(F * d) + fd) < 1e-8, (np.sum(F * d), -fd)


def test_ewald_forces_vanish_at_equilibrium():
    lat, atoms, pos = dftk.silicon_cell()
    _, F = energy_forces_ewald(lat, [a.charge_ionic for a in atoms], pos)
    assert np.max(np.abs(F)) < 1e-10


def _si_model(positions, symmetries):
    lat, atoms, _ = dftk.silicon_cell()
    return dftk.model_DFT(lat, atoms, positions, functionals=("lda_x", "lda_c_vwn"), symmetries=symmetries)


def test_symmetrize_forces_identity_only():
    model = _si_model(_displaced_si()[2], False)
    F = np.random.default_rng(0).standard_normal((2, 3))
    assert np.array_equal(dftk.symmetrize_forces(model, F, symmetries=model.symmetries), F)


def test_symmetrize_forces_projects_onto_symmetric_part():
    lat, _, pos = dftk.silicon_cell()
    model = _si_model(pos, True)
    syms = model.symmetries
    assert len(syms) == 48
    F = np.random.default_rng(2).standard_normal((2, 3))
    Fs = dftk.symmetrize_forces(model, F, symmetries=syms)
    # idempotent, and the Si point group leaves no symmetric force on the atoms (each site has Td symmetry)
    assert np.allclose(dftk.symmetrize_forces(model, Fs, symmetries=syms), Fs, atol=1e-14)
    assert np.max(np.abs(Fs)) < 1e-14
    # atom 1 moved along [111]: C3v survives, the symmetric part lies along [111] (reduced: along inv(A') e_111)
    pos2 = [pos[0] + 0.01 * np.ones(3), pos[1]]
    model2 = _si_model(pos2, True)
    Fs2 = dftk.symmetrize_forces(model2, F, symmetries=model2.symmetries)
    assert np.allclose(dftk.symmetrize_forces(model2, Fs2, symmetries=model2.symmetries), Fs2, atol=1e-14)
    Fc = forces_red_to_cart(lat, Fs2)
    axis = np.ones(3) / np.sqrt(3)
    perp = Fc - np.outer(Fc @ axis, axis)
    assert np.max(np.abs(perp)) < 1e-12
    assert np.max(np.abs(Fc)) > 1e-3


def test_red_to_cart_conversion():
    lat = np.array([[5.0, 0.3, 0.0], [0.0, 6.0, 0.4], [0.2, 0.0, 5.5]])
    F = np.random.default_rng(3).standard_normal((3, 3))
    ref = np.stack([np.linalg.inv(lat.T) @ f for f in F])
    assert np.allclose(forces_red_to_cart(lat, F), ref, rtol=1e-14, atol=1e-14)


def test_xc_forces_refuse_a_core_corrected_pseudopotential():
    import dataclasses
    from types import SimpleNamespace
    from dftk_jl_amd.forces import compute_forces_term
    lat, atoms, pos = dftk.silicon_cell()
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
    assert compute_forces_term("Xc", SimpleNamespace(model=model), None, None) is None     # HGH: no core density

    class PspWithCore(type(atoms[0].psp)):
        def has_core_density(self):
            return True
    core = dataclasses.replace(atoms[0], psp=PspWithCore(**dataclasses.asdict(atoms[0].psp)))
    model2 = dftk.model_DFT(lat, [core, core], pos, functionals=("lda_x", "lda_c_vwn"))
    with pytest.raises(NotImplementedError):
        compute_forces_term("Xc", SimpleNamespace(model=model2), None, None)
