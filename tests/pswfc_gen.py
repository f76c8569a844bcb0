"""UPF files with pseudo-atomic wavefunctions (PP_PSWFC) for the tests of band structures and projected densities of
states, and a NumPy twin of the orbital path.

* ``pswfc_text`` takes the text of ``upf_gen.write_upf(..., pswfc=False)`` -- a GTH pseudopotential as a UPF file on the
  2001-point uniform mesh of tests/nlcc_gen.py -- inserts a PP_PSWFC block and corrects ``number_of_wfc``.  The orbitals are
  phi_l(r) = r^l exp(-r^2 / 2 a^2), written as chi = r phi: "3S" (a = 1.1), "3P" (a = 1.3) and a second s channel "4S"
  (a = 2.0).  Their transform is known in closed form: hankel(r, r^2 phi, l, q) = 4 pi sqrt(pi / 2) a^(2l+3) exp(-q^2 a^2 / 2)
  (the radial part that multiplies the solid harmonic, i.e. already divided by q^l).
* the twin: Phi from the closed forms and ``upf_gen.solid_harmonic`` in the reference's column order (atom, l, n, m),
  Loewdin by ``numpy.linalg.eigh``, |Phi~' psi|^2, and the reference's loops for the PDOS (dos.jl:100-112).

Quadrature error of the mesh for these channels, relative to a channel's largest value: the twin's Simpson rule against the
closed form measures 1.7e-16 (3S), 1.2e-15 (3P), 1.1e-16 (4S) for q in [0, 12], the host's weighted sum 6.8e-16, 8.5e-16,
7.9e-16 (tests/test_bands_host.py::test_pswfc_transform_against_closed_form prints them).  All are below E_QUAD = 2e-13 of
tests/test_upf_host.py, so that constant is the bound here too and no constant of this file's own is needed.
Test helper: imported by tests/test_bands_host.py, tests/test_gpu_pdos_kernels.py and tests/test_gpu_bands.py.
"""
import math
import re

import numpy as np

import dftk_jl_amd as dftk
from dftk_jl_amd.mixing import occupation_derivative
from dftk_jl_amd.terms import atom_decay_length

import upf_gen

N_MESH = 2001
R_MAX = 30.0
# label: (l, a, occupation, pseudo_energy in Ry)
ORBITALS = {"3S": (0, 1.1, 2.0, -0.80), "3P": (1, 1.3, 2.0, -0.30), "4S": (0, 2.0, 0.0, -0.05)}


def orbital_chi(label, r):
    l, a, _, _ = ORBITALS[label]
    return r * r ** l * np.exp(-r ** 2 / (2 * a ** 2))


def closed_form(label):
    l, a, _, _ = ORBITALS[label]
    return lambda q: 4 * math.pi * math.sqrt(math.pi / 2) * a ** (2 * l + 3) * np.exp(-(np.asarray(q, float) * a) ** 2 / 2)


def pswfc_block(labels, r, energies=True):
    out = ["<PP_PSWFC>\n"]
    for i, label in enumerate(labels):
        l, _, occ, e = ORBITALS[label]
        attrs = f' index="{i + 1}" label="{label}" l="{l}" occupation="{occ:.3f}"'
        if energies:
            attrs += f' pseudo_energy="{e:.8E}"'
        out.append(upf_gen._block(f"PP_CHI.{i + 1}", orbital_chi(label, r), 4, attrs))
    out.append("</PP_PSWFC>\n")
    return "".join(out)


def pswfc_text(labels=("3S", "3P"), symbol="Si", functional="lda", mesh=None, energies=True):
    """UPF text of the GTH pseudopotential of ``symbol`` with the orbitals ``labels`` (in that order) in PP_PSWFC."""
    hgh = dftk.load_psp(symbol, functional)
    r = upf_gen.uniform_mesh(N_MESH, R_MAX) if mesh is None else np.asarray(mesh, dtype=float)
    rho = upf_gen.gaussian_density_real(float(hgh.Zion), atom_decay_length(10 if symbol == "Si" else 2, hgh.Zion), r)
    text = upf_gen.write_upf(hgh, r, element=symbol, rhoatom=rho, pswfc=False)
    assert "<PP_PSWFC>" not in text and 'number_of_wfc="0"' in text
    text = text.replace('number_of_wfc="0"', f'number_of_wfc="{len(labels)}"')
    at = text.index("<PP_RHOATOM")
    return text[:at] + pswfc_block(labels, r, energies) + text[at:]


def pswfc_psp(labels=("3S", "3P"), symbol="Si", functional="lda", **kw):
    return dftk.parse_psp_upf(pswfc_text(labels, symbol, functional, **kw),
                              identifier=f"{symbol.lower()}-{functional}-{'-'.join(labels)}.upf")


def strip_pswfc(text):
    """The same file without its PP_PSWFC block."""
    text = re.sub(r"<PP_PSWFC>.*?</PP_PSWFC>\n", "", text, flags=re.S)
    return re.sub(r'number_of_wfc="\d+"', 'number_of_wfc="0"', text)


# ------------------------------------------------------------------------------------------------ the twin
def ordered_channels(labels):
    """[(l, n, label)] in the reference's order: l ascending, then the order of the file within l (n 1-based)."""
    out = []
    for l in range(4):
        mine = [lab for lab in labels if ORBITALS[lab][0] == l]
        out.extend((l, n + 1, lab) for n, lab in enumerate(mine))
    return out


def twin_labels(labels_per_atom, species="Si"):
    out = []
    for ia, labels in enumerate(labels_per_atom):
        for l, n, lab in ordered_channels(labels):
            out.extend(dict(iatom=ia, species=species, n=n, l=l, m=m, label=lab) for m in range(-l, l + 1))
    return out


def twin_orbitals(G, k, recip, volume, positions, labels_per_atom, radial=closed_form):
    """Phi (n_G x n_proj complex), columns (atom, l, n, m): radial(|q|) Y_lm-solid(q) (-i)^l e^{-2 pi i (G+k).R} / sqrt(Omega).
    ``radial(label)`` returns the function of the norms (default: the closed forms)."""
    p = np.asarray(G, dtype=float) + np.asarray(k, dtype=float)[None, :]
    q = p @ np.asarray(recip).T
    qn = np.linalg.norm(q, axis=1)
    cols = []
    for pos, labels in zip(positions, labels_per_atom):
        ph = np.exp(-2j * math.pi * (p @ np.asarray(pos, dtype=float)))
        for l, _, lab in ordered_channels(labels):
            Rv = radial(lab)(qn)
            for m in range(-l, l + 1):
                cols.append(Rv * upf_gen.solid_harmonic(l, m, q) * (-1j) ** l / math.sqrt(volume) * ph)
    return np.stack(cols, axis=1)


def twin_lowdin(Phi):
    """ortho_lowdin (ortho.jl:11-17) with numpy.linalg.eigh; returns (Phi S^-1/2, eigenvalues of S)."""
    S = Phi.conj().T @ Phi
    w, V = np.linalg.eigh((S + S.conj().T) / 2)
    return Phi @ ((V * w ** -0.5) @ V.conj().T), w


def twin_projections(Phi_t, psi):
    """|psi' Phi~|^2, (n_bands, n_proj); psi is n_G x n_bands."""
    return np.abs(psi.conj().T @ Phi_t) ** 2


def twin_pdos(eps, projections, eigenvalues, kweights, spins, filled_occ, smearing, temperature, n_spin=1):
    """The loops of compute_pdos (dos.jl:100-112): D[ie, p, s] -= filled w_k proj[n, p] / T occupation_derivative(x)."""
    n_proj = projections[0].shape[1]
    D = np.zeros((len(eps), n_proj, n_spin))
    for ie, e in enumerate(eps):
        for proj, eig, w, s in zip(projections, eigenvalues, kweights, spins):
            for n, enk in enumerate(np.asarray(eig)[:proj.shape[0]]):
                x = (enk - e) / temperature
                D[ie, :, s - 1] -= filled_occ * w * proj[n] / temperature * float(occupation_derivative(smearing, x))
    return D
