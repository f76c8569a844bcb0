"""The extended-precision stress references of stress_ref.py, checked on the host before test_gpu_stress_kernels.py holds the
device entries to them at 1e-12 S:

  * at eps = 0 they are the oracle's energies (normalisation, column order, Nyquist convention, sign of the phase);
  * their own error estimate (dual numbers against a Richardson table) is <= 1e-15 S on every case of the GPU file;
  * the same code in float64 agrees to <= 1e-13 S: a correct fp64 evaluation sits 10x under the device tolerance;
  * the inputs exercise what they claim: dropping a rule (Nyquist, G = 0, sqrt 2 / row 0 of the half format, the phase of
    l >= 2) moves an output by more than 1e-6 S, and no component of a tensor is below 1e-3 S."""
from fractions import Fraction

import numpy as np
import pytest

import oracle
import stress_ref as sr

OWN_ERR, ROOM, MOVES, COMPONENT = 1e-15, 1e-13, 1e-6, 1e-3

NL_CASES = ([(False, n, nb) for n in sr.NG_COMPLEX for nb in sr.NBANDS]
            + [(True, n, nb) for n in sr.NHALF_GAMMA for nb in sr.NBANDS])
CUBE_CASES = [(fft, atoms) for fft in sr.CUBES for atoms in sr.ATOM_SETS]


def _rel(diff, S):
    """max |diff| / S over the outputs with S > 0; where S = 0 the difference must vanish"""
    diff, S = np.abs(np.asarray(diff, dtype=np.longdouble)), np.asarray(S, dtype=np.longdouble)
    assert np.all(diff[S == 0] == 0)
    return float(np.max(diff[S > 0] / S[S > 0])) if np.any(S > 0) else 0.0


def _again(gamma, n, nb, **kw):
    """the reference of a case of the GPU file with other options (no error estimate)"""
    _, G, psi, w, _ = sr.nonlocal_case(n, nb, gamma)
    recip, vol = sr.lattice_tables()
    return sr.kinetic_nonlocal(recip, vol, np.zeros(3) if gamma else sr.KPT, G, psi, w, sr.nonlocal_atoms(), estimate=False, **kw)


# ------------------------------------------------------------------------------------------ the oracle's energies
def test_reference_energies_are_the_oracles_on_the_multispecies_cell():
    """The cell of test_gpu_multispecies.py (five species in interleaved groups, one without projectors, two k-points):
    random orthonormal orbitals, random occupations, a perturbed guess density, as its ``state`` fixture."""
    from test_gpu_multispecies import FUN, KCOORDS, KWEIGHTS, LATTICE, POSITIONS, oracle_atoms
    assert np.array_equal(LATTICE, sr.LATTICE) and np.array_equal(KCOORDS[1], sr.KPT)
    model = oracle.model_DFT(LATTICE, oracle_atoms(), POSITIONS, functionals=FUN, temperature=0.01)
    ob = oracle.PlaneWaveBasis(model, 8, oracle.ExplicitKpoints(KCOORDS, KWEIGHTS))
    rng = np.random.default_rng(17)
    psi, occ = [], []
    for kpt in ob.kpoints:
        n = len(kpt.mapping)
        psi.append(np.linalg.qr(rng.standard_normal((n, 6)) + 1j * rng.standard_normal((n, 6)))[0])
        occ.append(rng.uniform(0.1, 2.0, 6))
    nx, ny, nz = ob.fft_size
    rho = oracle.guess_density(ob) * (1 + 0.1 * rng.random((nz, ny, nx)))
    E, _ = oracle.energy_hamiltonian(ob, psi, occ, rho=rho)
    groups = [(model.atoms[g[0]].psp, [model.positions[ia] for ia in g]) for g in model.atom_groups]
    atoms = [(psp, r) for psp, pos in groups if psp.count_n_proj() > 0 for r in pos]
    assert sum(psp.count_n_proj() for psp, _ in atoms) == 83
    e_kin = e_nl = 0
    for ik, kpt in enumerate(ob.kpoints):
        ref = sr.kinetic_nonlocal(model.recip_lattice, model.unit_cell_volume, kpt.coordinate, kpt.G_vectors, psi[ik],
                                  ob.kweights[ik] * occ[ik], atoms, estimate=False)
        e_kin, e_nl = e_kin + ref["E"][0], e_nl + ref["E"][1]
    cube = sr.cube(model.recip_lattice, model.unit_cell_volume, ob.fft_size, rho, groups, estimate=False)
    for name, got in (("Kinetic", e_kin), ("AtomicNonlocal", e_nl), ("AtomicLocal", cube["value"][12]),
                      ("Hartree", cube["value"][13])):
        print(f"{name}: reference {float(got):.15e}, oracle {E[name]:.15e}, rel {abs(float(got) - E[name]) / abs(E[name]):.2e}")
        assert abs(float(got) - E[name]) <= 1e-12 * abs(E[name]), name


# ------------------------------------------------------------------------------------------ own error, room
@pytest.mark.parametrize("gamma,n,nb", NL_CASES)
def test_kinetic_nonlocal_reference_error_and_float64_room(gamma, n, nb):
    ref = sr.nonlocal_case(n, nb, gamma)[4]
    assert ref["value"].dtype == np.longdouble
    own = _rel(ref["err"], ref["S"])
    f64 = _again(gamma, n, nb, dtype=np.float64)
    assert f64["value"].dtype == np.float64
    room = _rel(f64["value"] - ref["value"], ref["S"])
    print(f"own error {own:.2e} S, float64 {room:.2e} S")
    assert own <= OWN_ERR and room <= ROOM
    # every component counts: none is zero by symmetry or by accident (the only row of the one-row Gamma sphere is G = 0)
    big = np.abs(ref["value"]) >= COMPONENT * ref["S"]
    assert np.all(big), ref["value"] / ref["S"]
    if not (gamma and n == 1):
        assert np.all(ref["S"] > 0)


@pytest.mark.parametrize("fft_size,atom_set", CUBE_CASES, ids=lambda v: sr.cube_id(v) if isinstance(v, tuple) else v)
def test_cube_reference_error_and_float64_room(fft_size, atom_set):
    rho, ref = sr.cube_case(fft_size, atom_set)
    recip, vol = sr.lattice_tables()
    own = _rel(ref["err"], ref["S"])
    f64 = sr.cube(recip, vol, fft_size, rho, sr.cube_groups(atom_set), dtype=np.float64, estimate=False)
    room = _rel(f64["value"] - ref["value"], ref["S"])
    print(f"own error {own:.2e} S, float64 {room:.2e} S")
    assert own <= OWN_ERR and room <= ROOM
    assert np.all(np.abs(ref["value"]) >= COMPONENT * ref["S"]), ref["value"] / ref["S"]
    assert np.all(ref["S"][6:12] > 0) and ref["S"][13] > 0
    if atom_set == "none":
        assert np.all(ref["value"][:6] == 0) and ref["value"][12] == 0
    else:
        assert np.all(ref["S"][:6] > 0) and ref["S"][12] > 0


# ------------------------------------------------------------------------------------------ the inputs bite
@pytest.mark.parametrize("fft_size", sr.CUBES, ids=sr.cube_id)
def test_cube_inputs_see_the_nyquist_and_the_g0_rule(fft_size):
    rho, ref = sr.cube_case(fft_size, "three")
    recip, vol = sr.lattice_tables()
    groups = sr.cube_groups("three")
    nyq = sr.cube(recip, vol, fft_size, rho, groups, estimate=False, keep_nyquist=True)
    moved = np.abs(nyq["value"] - ref["value"]) / ref["S"]
    if all(n % 2 for n in fft_size):
        assert np.all(moved == 0)                                      # no Nyquist plane on an all-odd cube
    else:
        assert moved[:6].max() > 0 and moved[6:12].max() > MOVES and moved[13] > MOVES, moved
    # G = 0: q_eps = 0 at every strain, so 1 / q^2 of both forms is not finite -- and rho's mean is the largest
    # coefficient by far, so that no finite treatment of that entry would go unseen either
    g0 = sr.cube(recip, vol, fft_size, rho, groups, estimate=False, keep_g0=True)
    assert not np.any(np.isfinite(g0["value"].astype(float)))
    rho_G = np.abs(np.fft.fftn(rho)).ravel()
    assert rho_G[0] > 3 * rho_G[1:].max()


@pytest.mark.parametrize("gamma,n,nb", NL_CASES)
def test_nonlocal_inputs_see_the_half_format_rule_and_the_phase_of_high_l(gamma, n, nb):
    ref = sr.nonlocal_case(n, nb, gamma)[4]
    S = ref["S"]
    fixed = _again(gamma, n, nb, bra_fixed=True)
    assert _rel(fixed["value"] - ref["value"], S) <= OWN_ERR           # the bilinear form has the same derivative
    if gamma and n == 1:
        return                                                          # (G = 0 alone: no pair, no l >= 1 amplitude)
    shifted = _again(gamma, n, nb, bra_fixed=True, ket_l_shift=2)
    assert np.all(shifted["value"][:6] == ref["value"][:6])
    assert _rel(shifted["value"] - ref["value"], S) > MOVES
    if gamma:
        rule = _again(gamma, n, nb, bra_fixed=True, half="rule")
        assert _rel(rule["value"] - ref["value"], S) <= OWN_ERR        # the half format gives the full sphere's sums
        for broken in ("no_sqrt2", "no_row0"):
            assert _rel(_again(gamma, n, nb, bra_fixed=True, half=broken)["value"] - ref["value"], S) > MOVES, broken


# ------------------------------------------------------------------------------------------ xc
def test_xc_reference_is_the_exact_sum():
    for variant in sr.XC_VARIANTS:
        d = sr.xc_inputs(257, variant)
        value, S = sr.xc(**d)

        def fr(x):
            return [Fraction(float(v)) for v in np.ravel(x)]
        rho, vrho = fr(d["rho"]), fr(d["vrho"])
        exact = sum(a * b for a, b in zip(rho, vrho))
        assert abs(Fraction(value[1]) - exact) <= Fraction(2.0 ** -52) * abs(exact)
        assert S[1] >= abs(value[1]) and S[1] == pytest.approx(float(np.sum(np.abs(d["rho"] * d["vrho"]))), rel=1e-14)
        if variant == "gga":
            g, vs = d["grad"], fr(d["vsigma"])
            exact = sum(v * Fraction(float(a)) * Fraction(float(b)) for v, a, b in zip(vs, g[2], g[1]))
            assert abs(Fraction(value[5]) - exact) <= Fraction(2.0 ** -52) * abs(exact)          # out[5]: zy
            assert abs(Fraction(value[0]) - sum(fr(d["e"]))) <= Fraction(2.0 ** -52) * abs(sum(fr(d["e"])))
        else:
            assert value[0] == 0 and np.all(value[2:] == 0) and np.all(S[2:] == 0)
