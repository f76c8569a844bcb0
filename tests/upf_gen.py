"""Generator of UPF 2.0.1 text from the analytic real-space HGH forms, and a NumPy twin of the UPF path.

* ``write_upf(psp_hgh, ...)``: the local potential, r beta_{l,i}(r) and PP_DIJ of an HGH pseudopotential in the file's
  Rydberg units on a logarithmic or uniform mesh of any length, a ``cutoff_radius_index`` per projector, optionally a
  PP_RHOATOM, and flags that inject every feature the reader refuses.  This is the reference's own way of testing PspUpf
  (GTH in UPF form against PspHgh, test/PspUpf.jl): every number of the UPF path has an exact partner, the closed forms of
  psp.py.
* the twin: the three quadrature rules spelled as the reference spells them (functions of the integrand, the weights are
  their values on unit vectors), Hankel sums with scipy.special.spherical_jn, the projector matrix, the cubes, the local
  energy and its forces by differences.
Test helper: imported by tests/test_upf_host.py, tests/test_gpu_upf_kernels.py and tests/test_gpu_upf.py.
"""
import math

import numpy as np
from scipy.special import erf, gamma, spherical_jn


# ------------------------------------------------------------------------------------------------ real-space HGH forms
def hgh_local_real(psp, r):
    """V_loc(r) of HGH (Hartwigsen, Goedecker, Hutter 1998, eq. 1), Hartree."""
    r = np.asarray(r, dtype=float)
    x = r / psp.rloc
    c = psp.cloc
    poly = c[0] + c[1] * x ** 2 + c[2] * x ** 4 + c[3] * x ** 6
    safe = np.where(r > 0, r, 1.0)
    coul = np.where(r > 0, -psp.Zion / safe * erf(safe / (math.sqrt(2) * psp.rloc)),
                    -psp.Zion * math.sqrt(2 / math.pi) / psp.rloc)
    return coul + np.exp(-0.5 * x * x) * poly


def hgh_projector_real(psp, i, l, r):
    """p_i^l(r) (eq. 3), i 1-based."""
    rp = psp.rp[l]
    ired = (4 * i - 1) / 2
    return math.sqrt(2) * r ** (l + 2 * (i - 1)) * np.exp(-r ** 2 / (2 * rp ** 2)) / (rp ** (l + ired) *
                                                                                      math.sqrt(gamma(l + ired)))


def gaussian_density_real(charge, decay, r):
    """rho(r) whose Fourier transform is charge exp(-(q decay)^2)."""
    return charge / (4 * math.pi * decay ** 2) ** 1.5 * np.exp(-r ** 2 / (4 * decay ** 2))


def log_mesh(n, rmin=1e-5, rmax=40.0):
    return rmin * (rmax / rmin) ** (np.arange(n) / max(n - 1, 1))


def uniform_mesh(n, rmax=40.0):
    return np.linspace(0.0, rmax, n)


def _block(tag, values, columns=4, attrs="", dexp=False):
    vals = [f"{v:.16E}" for v in values]
    if dexp:
        vals = [v.replace("E", "D") for v in vals]
    lines = [" ".join(vals[i:i + columns]) for i in range(0, len(vals), columns)]
    return (f'<{tag} type="real" size="{len(values)}" columns="{columns}"{attrs}>\n' + "\n".join(lines) +
            f"\n</{tag}>\n")


def write_upf(psp, r, *, element="Si", columns=4, dexp=False, cutoff_index=None, beta_order=None, rhoatom=None,
              channels=None, pswfc=True, pseudo_type="NC", core_correction=False, nlcc=None, has_so=False,
              has_gipaw=False, gipaw_block=False, version="2.0.1", multiline_attrs=True):
    """UPF text of the HGH pseudopotential ``psp`` on the mesh ``r``.  ``channels``: list of (l, i) to write (default all);
    ``beta_order``: a permutation of the written betas (their PP_BETA.n elements appear in that order, each with its own
    index / angular_momentum); ``cutoff_index``: one cutoff_radius_index per written beta (default: the whole mesh);
    ``rhoatom``: rho(r) values or None for no PP_RHOATOM."""
    r = np.asarray(r, dtype=float)
    n = len(r)
    rab = np.gradient(r) if n > 1 else np.ones(1)
    if channels is None:
        channels = [(l, i) for l in range(psp.lmax + 1) for i in range(1, psp.h[l].shape[0] + 1)]
    nb = len(channels)
    cut = [n] * nb if cutoff_index is None else list(cutoff_index)
    fb = "T" if core_correction else "F"
    sep = "\n    " if multiline_attrs else " "
    hdr = sep.join([f'generated="upf_gen"', f'comment="{psp.description} as UPF"', f'element="{element}"',
                    f'pseudo_type="{pseudo_type}"', 'relativistic="scalar"', 'is_ultrasoft="F"', 'is_paw="F"',
                    'is_coulomb="F"', f'has_so="{"T" if has_so else "F"}"', 'has_wfc="F"',
                    f'has_gipaw="{"T" if has_gipaw else "F"}"', f'core_correction="{fb}"', 'functional="PADE"',
                    f'z_valence="{float(psp.Zion):.8E}"', f'l_max="{max([c[0] for c in channels], default=-1)}"',
                    f'mesh_size="{n}"', f'number_of_wfc="{1 if pswfc else 0}"', f'number_of_proj="{nb}"'])
    out = [f'<UPF version="{version}">\n<PP_INFO>\nGTH pseudopotential & its "numeric" form, a < b\n</PP_INFO>\n',
           f"<PP_HEADER{sep}{hdr}/>\n", "<PP_MESH>\n", _block("PP_R", r, columns, dexp=dexp),
           _block("PP_RAB", rab, columns, dexp=dexp), "</PP_MESH>\n"]
    if nlcc is not None:
        out.append(_block("PP_NLCC", nlcc, columns))
    out.append(_block("PP_LOCAL", 2 * hgh_local_real(psp, r), columns, dexp=dexp))            # Ha -> Ry
    out.append("<PP_NONLOCAL>\n")
    order = list(range(nb)) if beta_order is None else list(beta_order)
    for ib in order:
        l, i = channels[ib]
        beta = 2 * r * hgh_projector_real(psp, i, l, r)                                       # r beta, Ha -> Ry
        beta = np.where(np.arange(n) < cut[ib], beta, 0.0)
        attrs = (f'{sep}index="{ib + 1}"{sep}angular_momentum="{l}"{sep}cutoff_radius_index="{cut[ib]}"'
                 f'{sep}cutoff_radius="{r[cut[ib] - 1]:.8E}"')
        out.append(_block(f"PP_BETA.{ib + 1}", beta, columns, attrs, dexp=dexp))
    dij = np.zeros((nb, nb))
    for a, (la, ia) in enumerate(channels):
        for b, (lb, ib_) in enumerate(channels):
            if la == lb:
                dij[a, b] = psp.h[la][ia - 1, ib_ - 1] / 2                                    # Ha -> the file's units
    out.append(_block("PP_DIJ", dij.reshape(-1), columns, dexp=dexp))
    out.append("</PP_NONLOCAL>\n")
    if pswfc:
        out.append("<PP_PSWFC>\n" + _block("PP_CHI.1", r * np.exp(-r), columns,
                                           ' label="3S" l="0" occupation="2.0" index="1"') + "</PP_PSWFC>\n")
    if rhoatom is not None:
        out.append(_block("PP_RHOATOM", 4 * math.pi * r ** 2 * np.asarray(rhoatom), columns, dexp=dexp))
    if gipaw_block:
        out.append('<PP_GIPAW gipaw_data_format="2">\n</PP_GIPAW>\n')
    out.append("</UPF>\n")
    return "".join(out)


def write_upf_v1(psp, r):
    return ("<PP_INFO>\nGenerated\n</PP_INFO>\n<PP_HEADER>\n   0   Version Number\n  Si   Element\n</PP_HEADER>\n"
            "<PP_MESH>\n<PP_R>\n" + " ".join(f"{v:.8E}" for v in r) + "\n</PP_R>\n</PP_MESH>\n")


# ------------------------------------------------------------------------------------------------ twin: quadrature
def trapezoidal(y, x):
    n = len(x)
    if n == 1:
        return 0.0
    I = (x[1] - x[0]) * y[0]
    for i in range(1, n - 1):
        I += (x[i + 1] - x[i - 1]) * y[i]
    I += (x[n - 1] - x[n - 2]) * y[n - 1]
    return I / 2


def simpson_uniform(y, x):
    dx = x[1] - x[0]
    n = len(x)
    odd = (n - 1) % 2 == 1
    istop = n - 2 if odd else n - 1
    I = dx / 3 * y[0]
    for i in range(2, istop + 1):           # 1-based i
        I += (4 / 3 * dx if i % 2 == 0 else 2 / 3 * dx) * y[i - 1]
    if odd:
        I += 5 / 12 * dx * y[n - 1]
        I += dx * y[n - 2]
        I -= dx / 12 * y[n - 3]
    else:
        I += dx / 3 * y[n - 1]
    return I


def simpson_nonuniform(y, x):
    n = len(x)
    odd = (n - 1) % 2 == 1
    istop = n - 3 if odd else n - 2
    I = 0.0
    for i in range(1, istop + 1, 2):        # 1-based i
        dx0 = x[i] - x[i - 1]
        dx1 = x[i + 1] - x[i]
        c = (dx0 + dx1) / 6
        I += c * (2 - dx1 / dx0) * y[i - 1]
        I += c * (dx0 + dx1) ** 2 / (dx0 * dx1) * y[i]
        I += c * (2 - dx0 / dx1) * y[i + 1]
    if odd:
        dxn = x[-1] - x[-2]
        dxm = x[-2] - x[-3]
        I += (2 * dxn ** 2 + 3 * dxn * dxm) / (6 * (dxm + dxn)) * y[n - 1]
        I += (dxn ** 2 + 3 * dxn * dxm) / (6 * dxm) * y[n - 2]
        I -= dxn ** 3 / (6 * dxm * (dxm + dxn)) * y[n - 3]
    return I


def simpson(y, x):
    if len(x) <= 4:
        return trapezoidal(y, x)
    a, b = x[1] - x[0], x[2] - x[1]
    if abs(a - b) <= math.sqrt(np.finfo(float).eps) * max(abs(a), abs(b)):
        return simpson_uniform(y, x)
    return simpson_nonuniform(y, x)


def twin_weights(x):
    """The weight vector of ``simpson`` on the mesh x: the rule's values on the unit vectors."""
    # (y[i] of the rules is row i of the identity: one pass gives the rule's value on every unit vector)
    out = simpson(np.eye(len(x)), x)
    return np.zeros(len(x)) if np.isscalar(out) else np.asarray(out, dtype=float)


# ------------------------------------------------------------------------------------------------ twin: transforms
def twin_hankel(r, wf, l, q):
    """4 pi sum_i wf_i j_l(q r_i) / q^l, the q -> 0 limit r^l / (2l+1)!! where q r underflows the Bessel function."""
    q = np.asarray(q, dtype=float).reshape(-1)
    out = np.empty(len(q))
    dfact = [1.0, 3.0, 15.0, 105.0][l]
    for j, qj in enumerate(q):
        x = qj * r
        small = x < 1e-3 * (l + 1)
        xs = np.where(small, 1.0, x)
        # below the threshold three terms of the series are exact to 1e-20 relative
        g = np.where(small, (1 - x * x / (2 * (2 * l + 3)) + x ** 4 / (8 * (2 * l + 3) * (2 * l + 5))) / dfact,
                     spherical_jn(l, xs) / xs ** l)
        out[j] = 4 * math.pi * np.sum(wf * r ** l * g)
    return out


def twin_local(r, wf, Zion, q):
    q = np.asarray(q, dtype=float).reshape(-1)
    out = np.zeros(len(q))
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        for j, qj in enumerate(q):
            if qj != 0:
                out[j] = 4 * math.pi * (np.sum(wf * np.sin(qj * r)) / qj - Zion / qj ** 2 * math.exp(-qj * qj / 4))
    return out


def twin_channels(psp):
    """{'local': (r, wf), 'rho': (r, wf) or None, (l, i0): (r, wf)} of a parsed PspUpf, with the twin's own weights."""
    n = psp.ircut
    r = psp.rgrid[:n]
    w = twin_weights(r)
    out = {"local": (r, w * (r * psp.vloc[:n] + psp.Zion * erf(r))),
           "rho": (r, w * psp.r2_rhoion[:n]) if np.any(psp.r2_rhoion != 0) else None}
    for l in range(psp.lmax + 1):
        for i, p in enumerate(psp.r2_projs[l]):
            m = min(n, len(p))
            out[(l, i)] = (psp.rgrid[:m], twin_weights(psp.rgrid[:m]) * p[:m])
    return out


def twin_energy_correction(psp):
    n = psp.ircut
    r = psp.rgrid[:n]
    return 4 * math.pi * simpson(r * (r * psp.vloc[:n] + psp.Zion), r)


# ------------------------------------------------------------------------------------------------ twin: P, cubes, forces
def signed_freq(n):
    return np.array([i if i <= (n - 1) // 2 else i - n for i in range(n)])


def solid_harmonic(l, m, q):
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    pi = math.pi
    if l == 0:
        return np.full(len(q), math.sqrt(1 / (4 * pi)))
    if l == 1:
        return math.sqrt(3 / (4 * pi)) * {-1: y, 0: z, 1: x}[m]
    if l == 2:
        return {-2: math.sqrt(15 / (4 * pi)) * x * y, -1: math.sqrt(15 / (4 * pi)) * y * z,
                0: math.sqrt(5 / (16 * pi)) * (2 * z * z - x * x - y * y), 1: math.sqrt(15 / (4 * pi)) * x * z,
                2: math.sqrt(15 / (16 * pi)) * (x * x - y * y)}[m]
    return {-3: math.sqrt(35 / (32 * pi)) * (3 * x * x - y * y) * y, -2: math.sqrt(105 / (4 * pi)) * x * y * z,
            -1: math.sqrt(21 / (32 * pi)) * y * (4 * z * z - x * x - y * y),
            0: math.sqrt(7 / (16 * pi)) * z * (2 * z * z - 3 * x * x - 3 * y * y),
            1: math.sqrt(21 / (32 * pi)) * x * (4 * z * z - x * x - y * y),
            2: math.sqrt(105 / (16 * pi)) * (x * x - y * y) * z, 3: math.sqrt(35 / (32 * pi)) * (x * x - 3 * y * y) * x}[m]


def twin_projectors(G, k, recip, volume, species, atoms):
    """P (n_rows x n_p, complex).  ``species``: per species a list over l = 0..3 of lists of radial functions
    ``R(q norms) -> values``; ``atoms``: (species index, reduced position) in column order."""
    p = G.astype(float) + np.asarray(k)[None, :]
    q = p @ np.asarray(recip).T
    qn = np.linalg.norm(q, axis=1)
    cols = []
    for s, pos in atoms:
        ph = np.exp(-2j * math.pi * (p @ np.asarray(pos)))
        for l, chans in enumerate(species[s]):
            radial = [R(qn) for R in chans]
            for m in range(-l, l + 1):
                for Rv in radial:
                    cols.append(Rv * solid_harmonic(l, m, q) * (-1j) ** l / math.sqrt(volume) * ph)
    return np.stack(cols, axis=1)


def cube_G(nx, ny, nz):
    """integer G of every cube point, x fastest, and the mask of entries that have their -G partner on the grid"""
    gx, gy, gz = signed_freq(nx), signed_freq(ny), signed_freq(nz)
    G = np.stack(np.meshgrid(gz, gy, gx, indexing="ij")[::-1], axis=-1).reshape(-1, 3)
    ok = np.ones((nz, ny, nx), dtype=bool)
    if nx % 2 == 0:
        ok[:, :, nx // 2] = False
    if ny % 2 == 0:
        ok[:, ny // 2, :] = False
    if nz % 2 == 0:
        ok[nz // 2, :, :] = False
    return G, ok.reshape(-1)


def twin_superposition(shape, recip, volume, ff_of_species, atoms):
    """irfft(enforce_real(sum_s ff_s(|G|) sum_a e^{-2 pi i G.r_a} / sqrt(Omega))), shape (nz, ny, nx); ``ff_of_species[s]``
    is a function of the norms; ``atoms``: (species, position)."""
    nx, ny, nz = shape
    G, ok = cube_G(nx, ny, nz)
    qn = np.linalg.norm(G.astype(float) @ np.asarray(recip).T, axis=1)
    ffs = [f(qn) for f in ff_of_species]
    c = np.zeros(len(G), dtype=complex)
    for s, pos in atoms:
        c += ffs[s] * np.exp(-2j * math.pi * (G @ np.asarray(pos))) / math.sqrt(volume)
    c = np.where(ok, c, 0.0)
    N = nx * ny * nz
    # x(r) = sum_G c(G) e^{iG.r} / sqrt(Omega)
    return (np.fft.ifftn(c.reshape(nz, ny, nx)) * N / math.sqrt(volume)).real


def twin_local_energy(shape, recip, volume, ff_of_species, atoms, rho):
    """sum_r V(r) rho(r) dvol with the cube of ``twin_superposition``"""
    V = twin_superposition(shape, recip, volume, ff_of_species, atoms)
    return float(np.sum(V * rho) * volume / rho.size)
