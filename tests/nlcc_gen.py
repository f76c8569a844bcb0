"""Core-corrected UPF files for the tests of the non-linear core correction: a GTH pseudopotential written as UPF
(tests/upf_gen.py) with a Gaussian core density in PP_NLCC, whose form factor is known in closed form.
Test helper: imported by tests/test_nlcc_host.py and tests/test_gpu_nlcc.py.
"""
import numpy as np

import dftk_jl_amd as dftk
from dftk_jl_amd.terms import atom_decay_length

import upf_gen

N_MESH = 2001            # the uniform mesh of tests/test_upf_host.py (r <= 30 bohr)
R_MAX = 30.0
# (charge c, decay d): rho_core(r) = gaussian_density_real(c, d, r), form factor c exp(-(q d)^2)
CORE = {"Si": (2.0, 0.45), "C": (1.2, 0.30)}
# Quadrature error of that mesh for the core channel, relative to the form factor's largest value c: the twin's Simpson rule
# against the closed form measures 3.3e-16 (Si) and 3.7e-16 (C) for q in [0, 12], the host's sum 6.7e-16 and 5.6e-16
# (tests/test_nlcc_host.py::test_closed_form prints both and asserts the constant, about 150 times what is measured: the margin
# that E_QUAD of tests/test_upf_host.py has over its own measurements).
E_QUAD_CORE = 1e-13


def closed_core_ff(symbol):
    c, d = CORE[symbol]
    return lambda q: c * np.exp(-(np.asarray(q, dtype=float) * d) ** 2)


def core_text(symbol="Si", functional="lda", core=True, rhoatom=True, mesh=None, header_flag=None, nlcc=None):
    """UPF text of the GTH pseudopotential of ``symbol`` with the Gaussian core of ``CORE`` (``core=False``: the same file
    without one).  ``header_flag`` / ``nlcc`` override the header's core_correction and the PP_NLCC block."""
    hgh = dftk.load_psp(symbol, functional)
    r = upf_gen.uniform_mesh(N_MESH, R_MAX) if mesh is None else np.asarray(mesh, dtype=float)
    rho = upf_gen.gaussian_density_real(float(hgh.Zion), atom_decay_length(10 if symbol == "Si" else 2, hgh.Zion), r) \
        if rhoatom else None
    if nlcc is None and core:
        nlcc = upf_gen.gaussian_density_real(*CORE[symbol], r)
    flag = core if header_flag is None else header_flag
    return upf_gen.write_upf(hgh, r, element=symbol, rhoatom=rho, core_correction=flag, nlcc=nlcc)


def core_psp(symbol="Si", functional="lda", core=True, **kw):
    return dftk.parse_psp_upf(core_text(symbol, functional, core, **kw),
                              identifier=f"{symbol.lower()}-{functional}-{'core' if core else 'nocore'}.upf")
