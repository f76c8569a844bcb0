"""Numeric norm-conserving pseudopotentials in UPF files (src/pseudo/PspUpf.jl), host side.

``PspUpf`` holds what the file gives on its radial mesh, in the reference's units (PspUpf.jl:5-64, 110-175).  Everything a
calculation needs from it is a radial quadrature; the reference's three rules (src/common/quadrature.jl) are linear in the
integrand, so each reduces to a weight vector ``w`` with ``I = sum_i w_i f_i`` (``quadrature_weights``), computed once per
mesh length.  The device evaluates the transforms (``dftk_mi_radial_transform``, csrc/radial_kernels.hip); the NumPy
functions here are their host values, used by descriptor-only bases and by the tests.
"""
from __future__ import annotations

import math
import re
import xml.etree.ElementTree as ET

import numpy as np

_DFACT = (1.0, 3.0, 15.0, 105.0)             # (2l+1)!!
SWITCH_POINTS = (1.0, 2.0, 3.0, 4.0)         # of g_l: series below, closed form above (csrc/radial_forms.h)
_SERIES_TERMS = 16


# ------------------------------------------------------------------------------------------ quadrature
def _isapprox(a, b):
    return abs(a - b) <= math.sqrt(np.finfo(float).eps) * max(abs(a), abs(b))


def trapezoidal_weights(x):
    x = np.asarray(x, dtype=float)
    n = len(x)
    w = np.zeros(n)
    if n == 1:
        return w
    w[0] = (x[1] - x[0]) / 2
    w[1:-1] = (x[2:] - x[:-2]) / 2
    w[-1] = (x[-1] - x[-2]) / 2
    return w


def simpson_uniform_weights(x):
    x = np.asarray(x, dtype=float)
    n = len(x)
    dx = x[1] - x[0]
    odd = (n - 1) % 2 == 1
    istop = n - 2 if odd else n - 1           # 1-based, as quadrature.jl:61
    w = np.zeros(n)
    w[0] = dx / 3
    for i in range(2, istop + 1):
        w[i - 1] = (4 / 3 if i % 2 == 0 else 2 / 3) * dx
    if odd:
        w[n - 1] += 5 / 12 * dx
        w[n - 2] += dx
        w[n - 3] -= dx / 12
    else:
        w[n - 1] += dx / 3
    return w


def simpson_nonuniform_weights(x):
    x = np.asarray(x, dtype=float)
    n = len(x)
    odd = (n - 1) % 2 == 1
    istop = n - 3 if odd else n - 2           # 1-based, as quadrature.jl:91
    w = np.zeros(n)
    for i in range(1, istop + 1, 2):
        dx0 = x[i] - x[i - 1]
        dx1 = x[i + 1] - x[i]
        c = (dx0 + dx1) / 6
        w[i - 1] += c * (2 - dx1 / dx0)
        w[i] += c * (dx0 + dx1) ** 2 / (dx0 * dx1)
        w[i + 1] += c * (2 - dx0 / dx1)
    if odd:
        dxn = x[-1] - x[-2]
        dxm = x[-2] - x[-3]
        w[n - 1] += (2 * dxn ** 2 + 3 * dxn * dxm) / (6 * (dxm + dxn))
        w[n - 2] += (dxn ** 2 + 3 * dxn * dxm) / (6 * dxm)
        w[n - 3] -= dxn ** 3 / (6 * dxm * (dxm + dxn))
    return w


def quadrature_rule(x):
    """``default_psp_quadrature`` / ``simpson`` (quadrature.jl:40-48, 121-129): the name of the rule for mesh ``x``."""
    if len(x) <= 4:
        return "trapezoidal"
    return "simpson_uniform" if _isapprox(x[1] - x[0], x[2] - x[1]) else "simpson_nonuniform"


def quadrature_weights(x, rule=None):
    """Weights ``w`` with ``sum_i w_i f(x_i)`` == the reference's ``simpson(f, x)`` in exact arithmetic.  ``rule``: the rule
    chosen elsewhere (the reference picks it from the WHOLE mesh, ``default_psp_quadrature(psp.rgrid)``, and applies it to a
    cut one); a Simpson rule needs three points, fewer take the trapezoid."""
    if rule is None or len(x) < 3:
        rule = quadrature_rule(x)
    return {"trapezoidal": trapezoidal_weights, "simpson_uniform": simpson_uniform_weights,
            "simpson_nonuniform": simpson_nonuniform_weights}[rule](x)


# ------------------------------------------------------------------------------------------ the object
class PspUpf:
    """``struct PspUpf`` (PspUpf.jl:5-64).  ``PspUpf(path_or_text, identifier=None, rcut=None)`` reads a UPF version 2
    file (or its text); lists are indexed ``[l][i]`` with 0-based i."""

    def __init__(self, path_or_text, identifier=None, rcut=None):
        path_or_text = text = str(path_or_text)           # (a pathlib.Path is a path)
        if "<" not in path_or_text:
            if str(path_or_text).lower().endswith(".psp8"):
                raise NotImplementedError("psp8 pseudopotential files are not implemented (UPF version 2 only)")
            with open(path_or_text) as fh:
                text = fh.read()
            if identifier is None:
                identifier = str(path_or_text)
        elif identifier is None:
            import hashlib
            identifier = "upf-" + hashlib.sha256(text.encode()).hexdigest()[:16]     # (atom groups compare identifiers)
        f = _read_upf(text)
        self.Zion = f["Zion"]
        self.lmax = f["lmax"]
        self.rgrid = f["r"]
        self.drgrid = f["rab"]
        self.vloc = f["vloc"] / 2                                   # Ry -> Ha
        rcut = float(self.rgrid[-1]) if rcut is None else min(float(rcut), float(self.rgrid[-1]))
        self.rcut = rcut
        self.ircut = int(np.argmax(self.rgrid >= rcut)) + 1         # number of mesh points up to the cutoff
        self.r2_projs = [[] for _ in range(self.lmax + 1)]
        order = [[] for _ in range(self.lmax + 1)]
        for ib, (l, cut, beta) in enumerate(f["betas"]):
            self.r2_projs[l].append(self.rgrid[:cut] * (beta[:cut] / 2))      # r beta / 2 (Ry -> Ha) * r
            order[l].append(ib)
        self.h = tuple(f["dij"][np.ix_(idx, idx)] * 2 if idx else np.zeros((0, 0)) for idx in order)
        # pseudo-atomic wavefunctions (PspUpf.jl:140-154): per l, in the file's order, r chi -> r^2 chi
        self.r2_pswfcs = [[] for _ in range(self.lmax + 1)]
        self.pswfc_occs = [[] for _ in range(self.lmax + 1)]
        self.pswfc_energies = [[] for _ in range(self.lmax + 1)]
        self.pswfc_labels = [[] for _ in range(self.lmax + 1)]
        for l, chi, label, occ, energy in f["pswfc"]:
            if l <= self.lmax:                                      # (the reference's loop runs over l = 0..lmax)
                self.r2_pswfcs[l].append(self.rgrid * chi)
                self.pswfc_occs[l].append(occ)
                self.pswfc_energies[l].append(energy)
                self.pswfc_labels[l].append(label)
        self.r2_rhoion = f["rhoatom"] / (4 * math.pi)
        self.r2_rhocore = self.rgrid ** 2 * f["nlcc"]               # PP_NLCC is rho_core(r) itself (PspUpf.jl:147-151)
        self.identifier = "" if identifier is None else identifier
        self.description = f["comment"]
        self._weights = {}

    # -- the interface PspHgh has
    def count_n_proj_radial(self, l=None):
        if l is None:
            return sum(len(p) for p in self.r2_projs)
        return len(self.r2_projs[l])

    def count_n_proj(self, l=None):
        if l is None:
            return sum(self.count_n_proj(ll) for ll in range(self.lmax + 1))
        return self.count_n_proj_radial(l) * (2 * l + 1)

    # -- pseudo-atomic wavefunctions (PspUpf.jl:210-212); i is 1-based in the label functions, as the reference's
    def count_n_pswfc_radial(self, l):
        return len(self.r2_pswfcs[l]) if 0 <= l <= self.lmax else 0

    def count_n_pswfc(self):
        return sum((2 * l + 1) * len(w) for l, w in enumerate(self.r2_pswfcs))

    def pswfc_label(self, i, l):
        return self.pswfc_labels[l][i - 1]

    def find_pswfc(self, label):
        """``(l, i)`` (i 1-based) of the orbital called ``label``."""
        for l, labels in enumerate(self.pswfc_labels):
            for i, name in enumerate(labels):
                if name == label:
                    return l, i + 1
        raise ValueError(f"could not find pseudo-atomic orbital with label {label!r}")

    def has_core_density(self):
        return bool(np.any(self.r2_rhocore != 0))

    def has_valence_density(self):
        return bool(np.any(self.r2_rhoion != 0))

    # -- what the radial transforms take: the mesh, cut, and w_i * (the integrand's r^2 f)
    def weights(self, n):
        if n not in self._weights:
            self._weights[n] = quadrature_weights(self.rgrid[:n], rule=quadrature_rule(self.rgrid))
        return self._weights[n]

    def projector_channel(self, l, i):
        """``(r, wf)`` of projector i (0-based) of angular momentum l, cut as PspUpf.jl:190."""
        n = min(self.ircut, len(self.r2_projs[l][i]))
        return self.rgrid[:n], self.weights(n) * self.r2_projs[l][i][:n]

    def pswfc_channel(self, l, i):
        """``(r, wf)`` of pseudo-atomic wavefunction i (0-based) of angular momentum l on the WHOLE mesh: the reference does
        not cut these at rcut (PspUpf.jl:218-224)."""
        n = len(self.rgrid)
        return self.rgrid, self.weights(n) * self.r2_pswfcs[l][i]

    def local_channel(self):
        """``(r, wf)`` with wf_i = w_i (r_i vloc_i + Zion erf(r_i)) (PspUpf.jl:237-240)."""
        from scipy.special import erf
        n = self.ircut
        r = self.rgrid[:n]
        return r, self.weights(n) * (r * self.vloc[:n] + self.Zion * erf(r))

    def valence_channel(self):
        n = self.ircut
        return self.rgrid[:n], self.weights(n) * self.r2_rhoion[:n]

    def core_channel(self):
        """``(r, wf)`` of the core density of the non-linear core correction, cut at ircut (PspUpf.jl:279-283)."""
        n = self.ircut
        return self.rgrid[:n], self.weights(n) * self.r2_rhocore[:n]


def parse_psp_upf(text, identifier=""):
    """Reader of UPF version 2 text; without an identifier the object gets one derived from the text."""
    return PspUpf(text, identifier=identifier or None)


def is_upf(psp):
    return isinstance(psp, PspUpf)


def model_has_upf(model):
    return any(is_upf(a.psp) for a in model.atoms)


def refuse_upf(model, what):
    """Consumers that evaluate HGH closed forms and their derivatives inside their kernels."""
    if model_has_upf(model):
        raise NotImplementedError(f"{what} with UPF pseudopotentials is not implemented (HGH closed forms only)")


# ------------------------------------------------------------------------------------------ the reader
def _truthy(v):
    return v is not None and v.strip().strip(".").lower() in ("t", "true")


def _numbers(el):
    if el is None or el.text is None:
        return np.zeros(0)
    return np.array([float(t) for t in re.sub(r"[dD]", "E", el.text).split()], dtype=float)


def _read_upf(text):
    m = re.search(r"<UPF\s+version\s*=\s*[\"']([^\"']*)[\"']", text)
    if m is None:
        if "<PP_HEADER>" in text or "<PP_INFO>" in text:
            raise NotImplementedError("UPF version 1 files are not implemented (UPF version 2 only)")
        raise ValueError("not a UPF file: no <UPF version=...> element")
    if not m.group(1).strip().startswith("2"):
        raise NotImplementedError(f"UPF version {m.group(1)} files are not implemented (UPF version 2 only)")
    # the free-text block may hold anything, '<' and '&' included: it is not needed
    text = re.sub(r"<PP_INFO>.*?</PP_INFO>", "", text, flags=re.S)
    text = re.sub(r"&(?!(amp|lt|gt|quot|apos);)", "&amp;", text)
    root = ET.fromstring(text[text.index("<UPF"):])
    hdr = root.find("PP_HEADER")
    if hdr is None:
        raise ValueError("UPF file without PP_HEADER")
    a = hdr.attrib
    ptype = a.get("pseudo_type", "").strip()
    unsupported = []
    if _truthy(a.get("has_so")):
        unsupported.append("spin-orbit coupling (has_so)")
    names = {"SL": "semilocal potential (SL)", "US": "ultrasoft (US)", "USPP": "ultrasoft (USPP)",
             "PAW": "projector-augmented wave (PAW)", "1/r": "Coulomb potential (1/r)"}
    if ptype in names:
        unsupported.append(names[ptype])
    elif ptype != "NC":
        unsupported.append(f"pseudo_type {ptype!r}")
    if _truthy(a.get("has_gipaw")) or root.find("PP_GIPAW") is not None:
        unsupported.append("GIPAW data")
    if _truthy(a.get("is_paw")):
        unsupported.append("projector-augmented wave (PAW)")
    if _truthy(a.get("is_ultrasoft")):
        unsupported.append("ultrasoft (US)")
    nlcc = _numbers(root.find("PP_NLCC"))
    # a core correction is taken when header and data agree; the two inconsistent forms are refused
    if _truthy(a.get("core_correction")):
        if not np.any(nlcc != 0):
            unsupported.append("non-linear core correction flagged in the header (core_correction) without PP_NLCC data")
    elif np.any(nlcc != 0):
        unsupported.append('non-zero PP_NLCC data although the header says core_correction="F" (non-linear core correction)')
    if unsupported:
        raise NotImplementedError("UPF pseudopotential with unsupported features: " + ", ".join(unsupported))
    mesh = root.find("PP_MESH")
    r = _numbers(mesh.find("PP_R"))
    rab = _numbers(mesh.find("PP_RAB"))
    vloc = _numbers(root.find("PP_LOCAL"))
    if len(r) == 0 or len(vloc) != len(r):
        raise ValueError("malformed UPF file: PP_R / PP_LOCAL")
    betas = []
    nl = root.find("PP_NONLOCAL")
    dij = np.zeros((0, 0))
    if nl is not None:
        found = []
        for el in nl:
            mm = re.fullmatch(r"PP_BETA\.(\d+)", el.tag)
            if mm:
                found.append((int(el.attrib.get("index", mm.group(1))), el))
        for _, el in sorted(found, key=lambda t: t[0]):
            l = int(el.attrib["angular_momentum"])
            if l > 3:
                raise NotImplementedError(f"UPF projector with angular momentum l = {l} > 3")
            beta = _numbers(el)
            cut = int(el.attrib.get("cutoff_radius_index", 0) or 0)
            cut = len(beta) if cut <= 0 else min(cut, len(beta))
            betas.append((l, cut, beta))
        d = _numbers(nl.find("PP_DIJ"))
        if len(d) != len(betas) ** 2:
            raise ValueError("malformed UPF file: PP_DIJ")
        dij = d.reshape(len(betas), len(betas))
    lmax = max([int(a.get("l_max", -1))] + [b[0] for b in betas])
    if np.any(nlcc != 0) and len(nlcc) != len(r):
        raise NotImplementedError("UPF pseudopotential with unsupported features: non-linear core correction whose "
                                  "PP_NLCC block is not as long as the mesh")
    if len(nlcc) != len(r):
        nlcc = np.zeros(len(r))
    # PP_PSWFC: the PP_CHI.n elements in index order, each with its l, label, occupation and (optional) pseudo_energy
    pswfc = []
    wfc = root.find("PP_PSWFC")
    if wfc is not None:
        found = []
        for el in wfc:
            mm = re.fullmatch(r"PP_CHI\.(\d+)", el.tag)
            if mm:
                found.append((int(el.attrib.get("index", mm.group(1))), el))
        for _, el in sorted(found, key=lambda t: t[0]):
            chi = _numbers(el)
            if len(chi) < len(r):                # shorter than the mesh: zero beyond what the file gives
                chi = np.concatenate([chi, np.zeros(len(r) - len(chi))])

            def _float(name):
                v = el.attrib.get(name)
                return None if v is None or not v.strip() else float(re.sub(r"[dD]", "E", v))
            occ = _float("occupation")
            pswfc.append((int(el.attrib["l"]), chi[:len(r)], (el.attrib.get("label") or "").strip(),
                          0.0 if occ is None else occ, _float("pseudo_energy")))
    rho = _numbers(root.find("PP_RHOATOM"))
    if len(rho) < len(r):                    # absent, or shorter than the mesh: zero beyond what the file gives
        rho = np.concatenate([rho, np.zeros(len(r) - len(rho))])
    return {"Zion": int(round(float(re.sub(r"[dD]", "E", a["z_valence"])))), "lmax": lmax, "r": r, "rab": rab,
            "vloc": vloc, "betas": betas, "dij": dij, "rhoatom": rho[:len(r)], "nlcc": nlcc, "comment": a.get("comment", "") or "",
            "pswfc": pswfc}


# ------------------------------------------------------------------------------------------ host values
def g_l(l, x):
    """j_l(x) / x^l on the host, the two branches of csrc/radial_forms.h."""
    x = np.asarray(x, dtype=float)
    h = -0.5 * x * x
    acc = np.zeros_like(x)
    for k in range(_SERIES_TERMS, 0, -1):
        acc = (1.0 + acc) * h / (k * (2 * l + 2 * k + 1))
    series = (1.0 + acc) / _DFACT[l]
    xs = np.where(x < SWITCH_POINTS[l], 1.0, x)
    s, c = np.sin(xs), np.cos(xs)
    x2 = xs * xs
    closed = (s / xs if l == 0 else (s - xs * c) / (x2 * xs) if l == 1
              else ((3 - x2) * s - 3 * xs * c) / (x2 * x2 * xs) if l == 2
              else ((15 - 6 * x2) * s - (15 - x2) * xs * c) / (x2 * x2 * x2 * xs))
    return np.where(x < SWITCH_POINTS[l], series, closed)


def _chunks(q, n_r):
    step = max(1, (1 << 22) // max(n_r, 1))
    for i in range(0, len(q), step):
        yield slice(i, i + step)


def hankel_host(r, wf, l, q):
    """4 pi sum_i wf_i r_i^l g_l(q r_i) for every q (kind 0 of ``dftk_mi_radial_transform``)."""
    q = np.asarray(q, dtype=float).reshape(-1)
    wr = wf * r ** l
    out = np.empty(len(q))
    for sl in _chunks(q, len(r)):
        out[sl] = 4 * math.pi * (g_l(l, q[sl, None] * r[None, :]) @ wr)
    return out


def local_host(r, wf, Zion, q):
    """kind 1 of ``dftk_mi_radial_transform`` (PspUpf.jl:229-242); 0 at q == 0."""
    q = np.asarray(q, dtype=float).reshape(-1)
    out = np.zeros(len(q))
    for sl in _chunks(q, len(r)):
        qq = q[sl]
        safe = np.where(qq == 0, 1.0, qq)
        val = 4 * math.pi * ((np.sin(safe[:, None] * r[None, :]) @ wf) / safe - Zion / safe ** 2 * np.exp(-safe ** 2 / 4))
        out[sl] = np.where(qq == 0, 0.0, val)
    return out


def eval_psp_local_fourier_upf(psp, q):
    r, wf = psp.local_channel()
    return local_host(r, wf, float(psp.Zion), q)


def eval_psp_projector_fourier_upf(psp, i, l, q):
    """i is 1-based, as for the HGH function."""
    r, wf = psp.projector_channel(l, i - 1)
    return hankel_host(r, wf, l, q)


def eval_psp_pswfc_fourier_upf(psp, i, l, q):
    """PspUpf.jl:218-224: hankel(rgrid, r2_pswfc, l, q) on the whole mesh; i is 1-based."""
    r, wf = psp.pswfc_channel(l, i - 1)
    return hankel_host(r, wf, l, q)


def eval_psp_valence_density_fourier_upf(psp, q):
    r, wf = psp.valence_channel()
    return hankel_host(r, wf, 0, q)


def eval_psp_core_density_fourier_upf(psp, q):
    """PspUpf.jl:279-283: hankel(rgrid[1:ircut], r2_rhocore, 0, q); no normalisation."""
    r, wf = psp.core_channel()
    return hankel_host(r, wf, 0, q)


def eval_psp_energy_correction_upf(psp):
    """4 pi simpson(r (r vloc + Zion)) up to ircut (PspUpf.jl:308-315)."""
    n = psp.ircut
    r = psp.rgrid[:n]
    return 4 * math.pi * float(np.dot(psp.weights(n), r * (r * psp.vloc[:n] + psp.Zion)))

