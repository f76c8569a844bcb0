"""UPF norm-conserving pseudopotentials on the host: the reader, its refusals, the quadrature weights and the host form
factors against the HGH closed forms (GTH pseudopotentials written as UPF files by tests/upf_gen.py)."""
import math

import numpy as np
import pytest
import torch

import dftk_jl_amd as dftk
from dftk_jl_amd import psp as psp_mod
from dftk_jl_amd import psp_upf

import upf_gen

SI = dftk.load_psp("Si", "lda")          # l = 0: 2 channels, l = 1: 1 channel


def _check_fields(u, hgh, r, cut=None, rho=None):
    assert u.Zion == hgh.Zion and isinstance(u.Zion, int)
    assert u.lmax == hgh.lmax
    assert np.array_equal(u.rgrid, r)
    assert len(u.drgrid) == len(r)
    np.testing.assert_allclose(u.vloc, upf_gen.hgh_local_real(hgh, r), rtol=1e-15, atol=0)
    ib = 0
    for l in range(hgh.lmax + 1):
        assert u.count_n_proj_radial(l) == hgh.count_n_proj_radial(l)
        assert u.count_n_proj(l) == hgh.count_n_proj(l)
        np.testing.assert_allclose(u.h[l], hgh.h[l], rtol=1e-15)
        for i in range(hgh.h[l].shape[0]):
            n = len(r) if cut is None else cut[ib]
            assert len(u.r2_projs[l][i]) == n
            np.testing.assert_allclose(u.r2_projs[l][i], r[:n] ** 2 * upf_gen.hgh_projector_real(hgh, i + 1, l, r[:n]),
                                       rtol=4e-15, atol=1e-300)
            ib += 1
    assert u.count_n_proj() == hgh.count_n_proj() and u.count_n_proj_radial() == hgh.count_n_proj_radial()
    assert u.rcut == r[-1] and u.ircut == len(r)
    assert u.has_core_density() is False
    if rho is None:
        assert not u.has_valence_density() and np.all(u.r2_rhoion == 0)
    else:
        assert u.has_valence_density()
        np.testing.assert_allclose(u.r2_rhoion, r ** 2 * rho, rtol=4e-15, atol=1e-300)
    assert "as UPF" in u.description


@pytest.mark.parametrize("case", ["log", "uniform", "columns1", "dexp", "betas_out_of_order", "no_rhoatom",
                                  "single_line_attrs"])
def test_round_trip(case):
    r = upf_gen.uniform_mesh(301) if case == "uniform" else upf_gen.log_mesh(300)
    rho = None if case == "no_rhoatom" else upf_gen.gaussian_density_real(4.0, 0.9, r)
    kw = {}
    cut = None
    if case == "columns1":
        kw["columns"] = 1
    if case == "dexp":
        kw["dexp"] = True
    if case == "betas_out_of_order":
        kw["beta_order"] = [2, 0, 1]
        cut = kw["cutoff_index"] = [250, 300, 211]
    if case == "single_line_attrs":
        kw["multiline_attrs"] = False
        kw["pswfc"] = False
    text = upf_gen.write_upf(SI, r, rhoatom=rho, **kw)
    u = dftk.parse_psp_upf(text, identifier="si-test")
    assert u.identifier == "si-test"
    _check_fields(u, SI, r, cut, rho)


def test_rcut_and_identifier(tmp_path):
    r = upf_gen.log_mesh(200)
    path = tmp_path / "Si.upf"
    path.write_text(upf_gen.write_upf(SI, r))
    u = dftk.PspUpf(str(path), rcut=10.0)
    assert u.identifier == str(path)
    assert u.rcut == 10.0 and u.ircut == int(np.argmax(r >= 10.0)) + 1
    assert len(u.projector_channel(0, 0)[0]) == u.ircut
    v = dftk.load_psp(str(path))
    assert isinstance(v, dftk.PspUpf) and v.ircut == len(r)
    el = dftk.ElementPsp("Si", psp=v)
    assert el.charge_ionic == 4 and el.n_elec_core == 10
    assert dftk.load_psp("Si", "lda").Zion == 4           # the (symbol, functional) form is untouched
    # two text-built objects of the same file group together, different files do not
    a, b = dftk.parse_psp_upf(path.read_text()), dftk.parse_psp_upf(path.read_text())
    c = dftk.parse_psp_upf(upf_gen.write_upf(SI, upf_gen.log_mesh(201)))
    assert a.identifier == b.identifier != c.identifier


@pytest.mark.parametrize("kw, word", [
    (dict(core_correction=True), "core correction"),
    (dict(nlcc=np.full(50, 0.1)), "core correction"),
    (dict(has_so=True), "has_so"),
    (dict(pseudo_type="SL"), "SL"),
    (dict(pseudo_type="US"), "US"),
    (dict(pseudo_type="USPP"), "USPP"),
    (dict(pseudo_type="PAW"), "PAW"),
    (dict(pseudo_type="1/r"), "1/r"),
    (dict(has_gipaw=True), "GIPAW"),
    (dict(gipaw_block=True), "GIPAW"),
    (dict(version="1.0.0"), "version 1"),
])
def test_refusals(kw, word):
    with pytest.raises(NotImplementedError, match=word):
        dftk.parse_psp_upf(upf_gen.write_upf(SI, upf_gen.log_mesh(50), **kw))


def test_refuses_upf_v1_and_psp8(tmp_path):
    with pytest.raises(NotImplementedError, match="version 1"):
        dftk.parse_psp_upf(upf_gen.write_upf_v1(SI, upf_gen.log_mesh(20)))
    p8 = tmp_path / "Li.psp8"
    p8.write_text("Li    ONCVPSP-3.3.0\n")
    with pytest.raises(NotImplementedError, match="psp8"):
        dftk.load_psp(str(p8))
    with pytest.raises(NotImplementedError, match="psp8"):
        dftk.PspUpf(str(p8))
    # a zero PP_NLCC with core_correction="F" is no core correction
    dftk.parse_psp_upf(upf_gen.write_upf(SI, upf_gen.log_mesh(50), nlcc=np.zeros(50)))


# ------------------------------------------------------------------------------------------------ quadrature
def _poly_integral(c, a, b):
    return sum(ck / (k + 1) * (b ** (k + 1) - a ** (k + 1)) for k, ck in enumerate(c))


@pytest.mark.parametrize("n", range(1, 10))
@pytest.mark.parametrize("mesh", ["uniform", "nonuniform", "uniform_within_approx"])
def test_quadrature_weights_exact_on_polynomials(n, mesh):
    """n = 1..9 hits the <= 4-point trapezoid and both parities of the interval count.  Simpson (and its odd-interval tail,
    a parabola through the last three points) integrates quadratics exactly, the trapezoid linear functions."""
    if mesh == "uniform":
        x = 0.3 + 0.25 * np.arange(n)
    elif mesh == "nonuniform":
        x = 0.3 * 1.37 ** np.arange(n)
    else:
        # steps equal to 1e-9 relative: '≈' (sqrt(eps) = 1.5e-8) takes the uniform rule
        x = 0.3 + 0.25 * np.arange(n) * (1 + 1e-9 * np.arange(n))
    w = psp_upf.quadrature_weights(x)
    rule = psp_upf.quadrature_rule(x)
    assert rule == ("trapezoidal" if n <= 4 else "simpson_nonuniform" if mesh == "nonuniform" else "simpson_uniform")
    np.testing.assert_allclose(w, upf_gen.twin_weights(x), rtol=1e-14, atol=1e-17)
    if n == 1:
        assert w[0] == 0.0
        return
    degree = 1 if n <= 4 else 2
    c = [0.7, -1.3, 0.45][:degree + 1]
    got = float(np.dot(w, np.polyval(c[::-1], x)))
    want = _poly_integral(c, x[0], x[-1])
    tol = 1e-13 * max(1.0, abs(want))
    if mesh == "uniform_within_approx" and n > 4:
        tol = 1e-8 * (x[-1] - x[0])          # the uniform rule on an almost-uniform mesh: exact to the mesh's deviation
    assert abs(got - want) <= tol, (got, want)


# ------------------------------------------------------------------------------------------------ against closed forms
N_MESH = 2001        # asserted below: the uniform mesh on which the quadrature error is negligible
# The quadrature error of that mesh, relative to each quantity's scale (a form factor's largest value), as the two tests
# below measure it against the closed forms: form factors 2e-16 ... 1e-15 (the twin up to 7e-15), the energy correction
# 8.6e-14 (it sums r^2 vloc up to r = 30: round-off of the sum and of the file's 17 digits, the same on a 6001-point mesh).
# The constant is the largest of them within a factor of 2.4; both tests assert it, the GPU tests take 10 x E_QUAD x scale.
E_QUAD = 2e-13


@pytest.fixture(scope="module")
def fine():
    r = upf_gen.uniform_mesh(N_MESH, 30.0)
    rho = upf_gen.gaussian_density_real(4.0, 0.8, r)
    return dftk.parse_psp_upf(upf_gen.write_upf(SI, r, rhoatom=rho))


def test_form_factors_against_closed_forms(fine):
    assert len(fine.rgrid) == N_MESH
    q = np.concatenate([[0.0, 1e-8, 1e-3], np.linspace(0.05, 12.0, 240)])
    qt = torch.from_numpy(q)
    tw = upf_gen.twin_channels(fine)
    errs = {}
    for l in range(SI.lmax + 1):
        for i in range(SI.h[l].shape[0]):
            want = psp_mod.eval_psp_projector_fourier(SI, i + 1, l, qt).numpy()
            host = psp_mod.eval_psp_projector_fourier(fine, i + 1, l, qt).numpy()
            twin = upf_gen.twin_hankel(*tw[(l, i)], l, q)
            scale = np.max(np.abs(want))
            errs[f"proj l={l} i={i}"] = (np.max(np.abs(host - want)) / scale, np.max(np.abs(twin - want)) / scale)
    nz = q > 0.04            # the local form factor diverges like Z / q^2: relative to its own size there
    want = psp_mod.eval_psp_local_fourier(SI, qt).numpy()
    host = psp_mod.eval_psp_local_fourier(fine, qt).numpy()
    twin = upf_gen.twin_local(*tw["local"], SI.Zion, q)
    assert host[0] == 0.0 and twin[0] == 0.0 and want[0] == 0.0
    errs["local"] = (np.max(np.abs(host - want)[nz] / np.abs(want[nz]).max()),
                     np.max(np.abs(twin - want)[nz] / np.abs(want[nz]).max()))
    want = 4.0 * np.exp(-(q * 0.8) ** 2)
    host = psp_mod.eval_psp_valence_density_fourier(fine, qt).numpy()
    twin = upf_gen.twin_hankel(*tw["rho"], 0, q)
    errs["rho"] = (np.max(np.abs(host - want)) / 4.0, np.max(np.abs(twin - want)) / 4.0)
    for name, (eh, et) in errs.items():
        print(f"{name}: host {eh:.2e}, twin {et:.2e} (relative to the form factor's scale)")
    for name, (eh, et) in errs.items():
        assert eh <= E_QUAD and et <= E_QUAD, (name, eh, et)


def test_energy_correction(fine):
    want = psp_mod.eval_psp_energy_correction(SI)
    got = psp_mod.eval_psp_energy_correction(fine)
    twin = upf_gen.twin_energy_correction(fine)
    print(f"energy correction: closed {want:.15g}, host {got:.15g}, twin {twin:.15g}")
    assert abs(got - want) <= E_QUAD * abs(want)
    assert abs(twin - want) <= E_QUAD * abs(want)


def test_host_g_l_against_mpmath():
    """Both branches of the host g_l within 4 units of 2^-52 g_l(0) of 40-digit values (each branch measures below 1
    unit in its range, tools/host_radial_check.cpp)."""
    import mpmath as mp
    mp.mp.dps = 40
    for l in range(4):
        xs = psp_upf.SWITCH_POINTS[l]
        x = np.concatenate([np.linspace(0.01, 12, 150), [xs * (1 - 1e-15), xs, 60.0, 1234.5]])
        ref = np.array([float(mp.besselj(l + mp.mpf(1) / 2, mp.mpf(float(v))) * mp.sqrt(mp.pi / (2 * mp.mpf(float(v))))
                              / mp.mpf(float(v)) ** l) for v in x])
        np.testing.assert_allclose(psp_upf.g_l(l, x), ref, rtol=0, atol=4 * 2.0 ** -52 / [1, 3, 15, 105][l])
        assert psp_upf.g_l(l, np.zeros(1))[0] == 1 / [1, 3, 15, 105][l]


def test_compiled_g_l_on_the_host():
    """csrc/radial_forms.h as compiled (both branches of g_l across the switch points, up to x of several thousand) through
    tools/host_radial_check.cpp: no GPU, host code under AddressSanitizer and UBSan, a long-double reference."""
    import subprocess
    from dftk_jl_amd import _build
    exe = _build.build_host_radial_check()
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout[-3000:], res.stderr[-3000:])
    assert "host_radial_check OK" in res.stdout and "FAILURES" not in res.stdout
    assert "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-3000:]


def test_reader_takes_a_path_object_and_a_short_rhoatom(tmp_path):
    import re
    r = upf_gen.log_mesh(60)
    text = upf_gen.write_upf(SI, r, rhoatom=upf_gen.gaussian_density_real(4.0, 0.9, r))
    path = tmp_path / "Si.upf"
    path.write_text(text)
    u = dftk.PspUpf(path)                          # a pathlib.Path
    assert u.identifier == str(path) and len(u.rgrid) == 60
    # PP_RHOATOM with fewer values than the mesh: zero beyond them
    m = re.search(r"(<PP_RHOATOM[^>]*>)(.*?)(</PP_RHOATOM>)", text, flags=re.S)
    vals = m.group(2).split()
    short = text[:m.start(2)] + "\n" + " ".join(vals[:40]) + "\n" + text[m.end(2):]
    v = dftk.parse_psp_upf(short)
    assert len(v.r2_rhoion) == 60 and np.array_equal(v.r2_rhoion[:40], u.r2_rhoion[:40]) and np.all(v.r2_rhoion[40:] == 0)
    assert len(v.valence_channel()[1]) == 60


def test_quadrature_rule_comes_from_the_whole_mesh():
    """a channel cut to four points of a uniform mesh keeps the mesh's Simpson rule (default_psp_quadrature(psp.rgrid))"""
    r = upf_gen.uniform_mesh(41, 10.0)
    u = dftk.parse_psp_upf(upf_gen.write_upf(SI, r, cutoff_index=[4, 41, 3]))
    np.testing.assert_allclose(u.weights(4), psp_upf.simpson_uniform_weights(r[:4]), rtol=0, atol=0)
    np.testing.assert_allclose(u.weights(3), psp_upf.simpson_uniform_weights(r[:3]), rtol=0, atol=0)
    assert len(u.projector_channel(0, 0)[1]) == 4 and len(u.projector_channel(1, 0)[1]) == 3


def test_descriptor_basis_and_model_io(fine):
    """A model with a UPF species builds a descriptor-only basis without a GPU: the torch constructions of P and of the
    valence form factor take the host quadrature values and agree with the HGH ones; the projector columns are counted
    for the memory estimate, the resident form-factor table too; stresses refuse by name."""
    lat, _, pos = dftk.silicon_cell()
    atoms = [dftk.ElementPsp("Si", psp=fine)] * 2
    model = dftk.model_DFT(lat, atoms, pos, functionals=("lda_x", "lda_c_vwn"))
    assert model.n_electrons == 8 and len(model.atom_groups) == 1
    from dftk_jl_amd.io import model_to_dict
    assert model_to_dict(model)["n_atoms"] == 2
    hgh_model = dftk.model_DFT(lat, [dftk.ElementPsp("Si", psp=SI)] * 2, pos, functionals=("lda_x", "lda_c_vwn"))
    from dftk_jl_amd.terms import build_projection_coefficients, energy_psp_correction
    np.testing.assert_allclose(build_projection_coefficients(model), build_projection_coefficients(hgh_model), rtol=1e-15)
    assert abs(energy_psp_correction(model) - energy_psp_correction(hgh_model)) <= E_QUAD * abs(
        energy_psp_correction(hgh_model))
    kg = dftk.ExplicitKpoints([[0, 0, 0], [0.25, 0.0, -0.5]], [0.5, 0.5])
    bu = dftk.PlaneWaveBasis(model, 5, kg, device="cpu")
    bh = dftk.PlaneWaveBasis(hgh_model, 5, kg, device="cpu")
    for Pu, Ph in zip(bu.terms.P, bh.terms.P):
        assert Pu.shape == Ph.shape == (10, Ph.shape[1])
        for c in range(Ph.shape[0]):
            assert float((Pu[c] - Ph[c]).abs().max()) <= 10 * E_QUAD * float(Ph[c].abs().max())
    assert abs(bu.terms.E_pspcorr - bh.terms.E_pspcorr) <= 10 * E_QUAD * abs(bh.terms.E_pspcorr)
    from dftk_jl_amd.terms import _valence_form_factor
    q = torch.linspace(0.0, 8.0, 50, dtype=torch.float64)
    ff = _valence_form_factor(bu, model.atoms[0], q)                 # the file's PP_RHOATOM: a Gaussian of width 0.8
    assert float((ff - 4.0 * torch.exp(-(q * 0.8) ** 2)).abs().max()) <= 10 * E_QUAD * 4.0
    from dftk_jl_amd.memory_usage import estimate_memory_usage, form_factor_table_bytes
    assert estimate_memory_usage(model, 5).n_nonlocal_projectors == estimate_memory_usage(hgh_model, 5).n_nonlocal_projectors == 10
    assert form_factor_table_bytes(model, (12, 12, 12)) == 8 * 12 ** 3 and form_factor_table_bytes(hgh_model, (12, 12, 12)) == 0
    with pytest.raises(NotImplementedError, match="UPF"):
        dftk.compute_stresses_cart({"basis": type("B", (), {"model": model})(), "psi": None, "occupation": None,
                                    "rho": None})
