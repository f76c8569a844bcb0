"""The non-linear core correction of UPF pseudopotentials on the host: what the reader accepts and refuses, the core
channel and its host form factor against the NumPy twin and the closed form of a Gaussian core, the ``use_nlcc`` switch of
the model, and the Xc forces without a device (None / refusals)."""
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dftk_jl_amd as dftk
from dftk_jl_amd import psp as psp_mod
from dftk_jl_amd import psp_upf
from dftk_jl_amd.forces import compute_forces_term

import nlcc_gen
import upf_gen
from nlcc_gen import CORE, E_QUAD_CORE

FUN = ("lda_x", "lda_c_vwn")


# ------------------------------------------------------------------------------------------------ reader
@pytest.mark.parametrize("mesh", ["uniform", "log"])
def test_reader_round_trip(mesh):
    r = upf_gen.uniform_mesh(301) if mesh == "uniform" else upf_gen.log_mesh(300)
    u = dftk.parse_psp_upf(nlcc_gen.core_text("Si", mesh=r))
    c, d = CORE["Si"]
    np.testing.assert_allclose(u.r2_rhocore, r ** 2 * upf_gen.gaussian_density_real(c, d, r), rtol=4e-15, atol=1e-300)
    assert u.has_core_density() is True
    rr, wf = u.core_channel()
    assert np.array_equal(rr, r) and np.array_equal(wf, u.weights(len(r)) * u.r2_rhocore)
    # cut by rcut like every other channel
    v = dftk.PspUpf(nlcc_gen.core_text("Si", mesh=r), rcut=6.0)
    n = int(np.argmax(r >= 6.0)) + 1
    assert v.ircut == n < len(r)
    rr, wf = v.core_channel()
    assert len(rr) == len(wf) == n and np.array_equal(rr, r[:n])
    assert np.array_equal(wf, v.weights(n) * v.r2_rhocore[:n]) and len(v.valence_channel()[0]) == n
    # the same file without a core: every other field unchanged, no core density
    w = dftk.parse_psp_upf(nlcc_gen.core_text("Si", core=False, mesh=r))
    assert w.has_core_density() is False and np.all(w.r2_rhocore == 0) and len(w.r2_rhocore) == len(r)
    assert np.array_equal(w.vloc, u.vloc) and np.array_equal(w.r2_rhoion, u.r2_rhoion)
    for pw, pu in zip(w.r2_projs, u.r2_projs):
        assert all(np.array_equal(a, b) for a, b in zip(pw, pu))
    assert dftk.load_psp("Si", "lda").has_core_density() is False             # HGH: never


def test_reader_accepts_and_refuses():
    r = upf_gen.log_mesh(60)
    core = upf_gen.gaussian_density_real(*CORE["Si"], r)
    # accepted: flag and data agree; a zero block under "F"; no block under "F"
    assert dftk.parse_psp_upf(nlcc_gen.core_text(mesh=r, header_flag=True, nlcc=core)).has_core_density()
    assert not dftk.parse_psp_upf(nlcc_gen.core_text(mesh=r, header_flag=False, nlcc=np.zeros(60))).has_core_density()
    assert not dftk.parse_psp_upf(nlcc_gen.core_text(mesh=r, core=False)).has_core_density()
    # refused: the flag without usable data (no block, a zero block, a block of another length); data under "F"
    for kw in (dict(core=False, header_flag=True), dict(header_flag=True, nlcc=np.zeros(60)),
               dict(header_flag=True, nlcc=core[:40]), dict(header_flag=False, nlcc=core)):
        with pytest.raises(NotImplementedError, match="core correction"):
            dftk.parse_psp_upf(nlcc_gen.core_text(mesh=r, **kw))


# ------------------------------------------------------------------------------------------------ form factor
@pytest.fixture(scope="module")
def fine():
    return {s: nlcc_gen.core_psp(s) for s in ("Si", "C")}


Q = np.concatenate([[0.0, 1e-8, 1e-3], np.linspace(0.05, 12.0, 240)])


def _twin_core(u, q):
    n = u.ircut
    r = u.rgrid[:n]
    return upf_gen.twin_hankel(r, upf_gen.twin_weights(r) * u.r2_rhocore[:n], 0, q)


@pytest.mark.parametrize("symbol", ["Si", "C"])
def test_host_form_factor_against_the_twin(fine, symbol):
    """the same sum in two spellings (weights folded in / the reference's rule, series + closed form of g_0 / scipy's j_0):
    a few units of rounding of the 2001-term sum, relative to the form factor's scale c"""
    u = fine[symbol]
    host = psp_upf.eval_psp_core_density_fourier_upf(u, Q)
    assert np.array_equal(psp_mod.eval_psp_core_density_fourier(u, torch.from_numpy(Q)).numpy(), host)
    err = np.max(np.abs(host - _twin_core(u, Q))) / CORE[symbol][0]
    print(f"{symbol}: host against twin {err:.2e}")
    assert err <= 64 * 2.2e-16
    with pytest.raises(ValueError):
        psp_mod.eval_psp_core_density_fourier(nlcc_gen.core_psp(symbol, core=False), torch.from_numpy(Q))


@pytest.mark.parametrize("symbol", ["Si", "C"])
def test_closed_form(fine, symbol):
    """c exp(-(q d)^2) within the quadrature error of the mesh, measured from the twin and recorded as E_QUAD_CORE"""
    u = fine[symbol]
    want = nlcc_gen.closed_core_ff(symbol)(Q)
    e_twin = np.max(np.abs(_twin_core(u, Q) - want)) / CORE[symbol][0]
    e_host = np.max(np.abs(psp_upf.eval_psp_core_density_fourier_upf(u, Q) - want)) / CORE[symbol][0]
    print(f"{symbol}: quadrature error of the core channel: twin {e_twin:.2e}, host {e_host:.2e} (E_QUAD_CORE {E_QUAD_CORE:.0e})")
    assert e_twin <= E_QUAD_CORE and e_host <= E_QUAD_CORE


# ------------------------------------------------------------------------------------------------ model and terms
def _model(psp, **kw):
    lat, _, pos = dftk.silicon_cell()
    return dftk.model_DFT(lat, [dftk.ElementPsp("Si", psp=psp)] * 2, pos, functionals=FUN, **kw)


def test_use_nlcc_switch_on_a_descriptor_only_basis(fine):
    from dftk_jl_amd.io import model_to_dict
    from dftk_jl_amd.terms import model_uses_nlcc
    kg = dftk.ExplicitKpoints([[0, 0, 0]], [1.0])
    on, off = _model(fine["Si"]), _model(fine["Si"], use_nlcc=False)
    bare = _model(nlcc_gen.core_psp("Si", core=False))
    assert on.use_nlcc is True and off.use_nlcc is False and bare.use_nlcc is True
    assert model_to_dict(on)["use_nlcc"] is True and model_to_dict(off)["use_nlcc"] is False
    assert model_uses_nlcc(on) and not model_uses_nlcc(off) and not model_uses_nlcc(bare)
    b_on = dftk.PlaneWaveBasis(on, 5, kg, device="cpu")
    for m in (off, bare):
        T = dftk.PlaneWaveBasis(m, 5, kg, device="cpu").terms
        assert T.rho_core is None and T.grad_core is None and T.core_ff is None
    # descriptor only: the host values of the form factors (no cube without the library's FFT)
    T = b_on.terms
    assert T.rho_core is None and T.core_ff.shape == (1, b_on.N)
    q = torch.linalg.norm(b_on.G_vectors_cart_cube(), dim=-1).reshape(-1).numpy()
    assert np.max(np.abs(T.core_ff[0].numpy() - nlcc_gen.closed_core_ff("Si")(q))) <= 10 * E_QUAD_CORE * CORE["Si"][0]
    # a model without an Xc term has no use for the core
    lat, _, pos = dftk.silicon_cell()
    atomic = dftk.model_atomic(lat, [dftk.ElementPsp("Si", psp=fine["Si"])] * 2, pos)
    assert not model_uses_nlcc(atomic)


def test_two_species_table_has_a_zero_row(fine):
    lat, _, pos = dftk.silicon_cell()
    atoms = [dftk.ElementPsp("Si", psp=dftk.load_psp("Si", "lda")), dftk.ElementPsp("C", psp=fine["C"])]
    model = dftk.model_DFT(lat, atoms, pos, functionals=FUN)
    b = dftk.PlaneWaveBasis(model, 5, dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu")
    ff = b.terms.core_ff
    assert ff.shape[0] == 2 and bool((ff[0] == 0).all()) and abs(float(ff[1].max()) - CORE["C"][0]) < 1e-12


# ------------------------------------------------------------------------------------------------ forces
def test_xc_forces_none_and_refusals(fine):
    ns = lambda m: SimpleNamespace(model=m)                              # noqa: E731
    assert compute_forces_term("Xc", ns(_model(nlcc_gen.core_psp("Si", core=False))), None, None) is None
    assert compute_forces_term("Xc", ns(_model(fine["Si"], use_nlcc=False)), None, None) is None
    lat, atoms, pos = dftk.silicon_cell()
    assert compute_forces_term("Xc", ns(dftk.model_DFT(lat, atoms, pos, functionals=FUN)), None, None) is None

    class PspWithCore(type(atoms[0].psp)):                               # claims a core density nobody can evaluate
        def has_core_density(self):
            return True
    core = dataclasses.replace(atoms[0], psp=PspWithCore(**dataclasses.asdict(atoms[0].psp)))
    with pytest.raises(NotImplementedError, match="core correction"):
        compute_forces_term("Xc", ns(dftk.model_DFT(lat, [core, core], pos, functionals=FUN)), None, None)

    class PspSilent:                                                     # cannot say
        identifier = "silent"
    silent = dataclasses.replace(atoms[0], psp=PspSilent())
    with pytest.raises(NotImplementedError, match="core correction"):
        compute_forces_term("Xc", ns(SimpleNamespace(atoms=[silent], term_types=("Xc",), use_nlcc=True)), None, None)
    # with a core the term needs the device: a descriptor-only basis raises instead of returning zeros
    b = dftk.PlaneWaveBasis(_model(fine["Si"]), 5, dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu")
    with pytest.raises(RuntimeError):
        compute_forces_term("Xc", b, None, None, rho=torch.zeros(1))
    # and set-up refuses to build a core cube from a core density it cannot evaluate
    with pytest.raises(NotImplementedError, match="core"):
        dftk.PlaneWaveBasis(dftk.model_DFT(lat, [core, core], pos, functionals=FUN), 5,
                            dftk.ExplicitKpoints([[0, 0, 0]], [1.0]), device="cpu")
