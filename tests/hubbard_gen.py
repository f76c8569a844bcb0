"""UPF files with a d channel for the DFT+U tests, and a NumPy twin of the Hubbard term.

* ``hubbard_text`` takes the file of ``pswfc_gen.pswfc_text`` (the GTH pseudopotential of silicon as a UPF file with Gaussian
  pseudo-atomic orbitals), drops its PP_PSWFC block and writes one of its own that also holds "3D": l = 2,
  phi(r) = r^2 exp(-r^2 / 2 a^2) with a = 1.2, chi = r phi.  Its transform is the closed form of pswfc_gen for l = 2,
  4 pi sqrt(pi / 2) a^7 exp(-q^2 a^2 / 2).  The header's l_max becomes 2 (the reader keeps the orbitals up to l_max).
* the twin: Phi from the closed forms in the reference's column order (atom, l, n, m), Loewdin by ``numpy.linalg.eigh``,
  ``extract_manifold``; the loops of ``compute_hubbard_n`` (hubbard.jl:201-228) over ALL atom pairs, the symmetrisation of
  symmetry.jl:425-452 with Wigner matrices of its own (seeded random directions, ``upf_gen.solid_harmonic``), the energy, the
  dense Phi D Phi' and the analytic gradient H_U psi.
Test helper: imported by tests/test_hubbard_host.py, tests/test_gpu_hubbard_kernels.py and tests/test_gpu_hubbard.py.
"""
import math
import re

import numpy as np

import dftk_jl_amd as dftk

import pswfc_gen
import upf_gen

# label: (l, a, occupation, pseudo_energy in Ry)
ORBITALS = dict(pswfc_gen.ORBITALS)
ORBITALS["3D"] = (2, 1.2, 0.0, -0.02)
LABELS = ("3S", "3P", "3D")


def orbital_chi(label, r):
    l, a, _, _ = ORBITALS[label]
    return r * r ** l * np.exp(-r ** 2 / (2 * a ** 2))


def closed_form(label):
    l, a, _, _ = ORBITALS[label]
    return lambda q: 4 * math.pi * math.sqrt(math.pi / 2) * a ** (2 * l + 3) * np.exp(-(np.asarray(q, float) * a) ** 2 / 2)


def hubbard_text(labels=LABELS, symbol="Si", functional="lda"):
    text = pswfc_gen.strip_pswfc(pswfc_gen.pswfc_text(("3S", "3P"), symbol, functional))
    r = upf_gen.uniform_mesh(pswfc_gen.N_MESH, pswfc_gen.R_MAX)
    block = ["<PP_PSWFC>\n"]
    for i, label in enumerate(labels):
        l, _, occ, e = ORBITALS[label]
        attrs = f' index="{i + 1}" label="{label}" l="{l}" occupation="{occ:.3f}" pseudo_energy="{e:.8E}"'
        block.append(upf_gen._block(f"PP_CHI.{i + 1}", orbital_chi(label, r), 4, attrs))
    block.append("</PP_PSWFC>\n")
    text = text.replace('number_of_wfc="0"', f'number_of_wfc="{len(labels)}"')
    lmax = max(ORBITALS[lab][0] for lab in labels)
    text = re.sub(r'l_max="(\d+)"', lambda m: f'l_max="{max(int(m.group(1)), lmax)}"', text)
    at = text.index("<PP_RHOATOM")
    return text[:at] + "".join(block) + text[at:]


def hubbard_psp(labels=LABELS, symbol="Si", functional="lda"):
    return dftk.parse_psp_upf(hubbard_text(labels, symbol, functional),
                              identifier=f"{symbol.lower()}-{functional}-{'-'.join(labels)}-hubbard.upf")


# ------------------------------------------------------------------------------------------------ orbitals
def ordered_channels(labels):
    out = []
    for l in range(4):
        mine = [lab for lab in labels if ORBITALS[lab][0] == l]
        out.extend((l, n + 1, lab) for n, lab in enumerate(mine))
    return out


def twin_labels(n_atoms, labels=LABELS):
    out = []
    for ia in range(n_atoms):
        for l, n, lab in ordered_channels(labels):
            out.extend(dict(iatom=ia, n=n, l=l, m=m, label=lab) for m in range(-l, l + 1))
    return out


def twin_orbitals(G, k, recip, volume, positions, labels=LABELS):
    """Loewdin-orthonormalised Phi (n_G x n_proj complex), columns (atom, l, n, m), with the eigenvalues of S."""
    p = np.asarray(G, dtype=float) + np.asarray(k, dtype=float)[None, :]
    q = p @ np.asarray(recip).T
    qn = np.linalg.norm(q, axis=1)
    cols = []
    for pos in positions:
        ph = np.exp(-2j * math.pi * (p @ np.asarray(pos, dtype=float)))
        for l, _, lab in ordered_channels(labels):
            Rv = closed_form(lab)(qn)
            for m in range(-l, l + 1):
                cols.append(Rv * upf_gen.solid_harmonic(l, m, q) * (-1j) ** l / math.sqrt(volume) * ph)
    return pswfc_gen.twin_lowdin(np.stack(cols, axis=1))


def manifold_columns(n_atoms, manifolds, labels=LABELS):
    """``manifolds``: [(iatoms, label)].  Per manifold and atom the columns of its 2 l + 1 orbitals in ``twin_orbitals``."""
    labs = twin_labels(n_atoms, labels)
    out = []
    for iatoms, label in manifolds:
        out.append([[j for j, o in enumerate(labs) if o["iatom"] == ia and o["label"] == label] for ia in iatoms])
    return out


# ------------------------------------------------------------------------------------------------ the term
def twin_hubbard_n(Phi, psi, occupation, kweights, spins, filled_occ, n_spin, columns):
    """The loops of compute_hubbard_n (hubbard.jl:213-226), unsymmetrised: ``Phi`` / ``psi`` per k-block (n_G x n_proj,
    n_G x n_bands), ``columns`` = manifold_columns(...).  Returns one (n_spin, n_at, n_at, 2l+1, 2l+1) array per manifold."""
    out = []
    for per_atom in columns:
        d = len(per_atom[0])
        n = np.zeros((n_spin, len(per_atom), len(per_atom), d, d), dtype=complex)
        for Pk, psik, occ, w, s in zip(Phi, psi, occupation, kweights, spins):
            occ = np.asarray(occ, dtype=float)[:psik.shape[1]]
            for i, ci in enumerate(per_atom):
                for j, cj in enumerate(per_atom):
                    i_projection = Pk[:, ci].conj().T @ psik
                    j_projection = psik.conj().T @ Pk[:, cj]
                    n[s - 1, i, j] += w * i_projection @ np.diag(occ / filled_occ) @ j_projection
        out.append(n)
    return out


def twin_wigner(l, Wcart, seed=1234):
    if l == 0:
        return np.ones((1, 1))
    rng = np.random.default_rng(seed)
    r = rng.random((2 * l + 2, 3))
    r /= np.linalg.norm(r, axis=1)[:, None]
    A = np.stack([upf_gen.solid_harmonic(l, m, r) for m in range(-l, l + 1)])
    B = np.stack([upf_gen.solid_harmonic(l, m, r @ np.asarray(Wcart).T) for m in range(-l, l + 1)])
    return B @ np.linalg.pinv(A)


def twin_symmetrize(lattice, positions, l, n, symmetries):
    """symmetry.jl:425-452; ``positions``: those of the manifold's atoms, ``symmetries``: objects with W and w."""
    lattice = np.asarray(lattice, dtype=float)
    out = np.zeros_like(n)
    for op in symmetries:
        W, w = np.asarray(op.W, dtype=float), np.asarray(op.w, dtype=float)
        D = twin_wigner(l, lattice @ W @ np.linalg.inv(lattice))
        for ia, pos in enumerate(positions):
            pre = np.linalg.solve(W, np.asarray(pos, dtype=float) - w)
            dev = [np.max(np.abs((np.asarray(p) - pre) - np.round(np.asarray(p) - pre))) for p in positions]
            ja = int(np.argmin(dev))
            assert dev[ja] < 1e-4
            for s in range(n.shape[0]):
                out[s, ia, ia] += D.T @ n[s, ja, ja] @ D
    return out / len(symmetries)


def twin_energy(U, hubbard_n, filled_occ):
    E = 0.0
    for u, n in zip(U, hubbard_n):
        for s in range(n.shape[0]):
            for ia in range(n.shape[1]):
                b = n[s, ia, ia]
                E += filled_occ * 0.5 * u * float(np.real(np.trace(b @ (np.eye(len(b)) - b))))
    return E


def twin_coupling(U, hubbard_n, spin, columns, n_proj):
    """D_sigma (n_proj x n_proj complex) over ALL columns of ``twin_orbitals``: blocks U / 2 (1 - 2 n[sigma, I, I])."""
    D = np.zeros((n_proj, n_proj), dtype=complex)
    for u, n, per_atom in zip(U, hubbard_n, columns):
        for ia, c in enumerate(per_atom):
            D[np.ix_(c, c)] = 0.5 * u * (np.eye(len(c)) - 2 * n[spin - 1, ia, ia])
    return D


def twin_operator(Phi_k, D):
    """dense Phi D Phi'"""
    return Phi_k @ D @ Phi_k.conj().T


def twin_gradient(Phi, psi, occupation, kweights, spins, U, hubbard_n, columns):
    """dE / d conj(psi_nk) = kweight f_n (Phi D_sigma Phi' psi)_n per k-block (n_G x n_bands)."""
    out = []
    for Pk, psik, occ, w, s in zip(Phi, psi, occupation, kweights, spins):
        D = twin_coupling(U, hubbard_n, s, columns, Pk.shape[1])
        occ = np.asarray(occ, dtype=float)[:psik.shape[1]]
        out.append(w * (Pk @ (D @ (Pk.conj().T @ psik))) * occ[None, :])
    return out
