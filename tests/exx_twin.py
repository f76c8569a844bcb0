"""NumPy twin of exact exchange at the Gamma point, built on the oracle's basis: the loops of the reference written densely.

* interaction kernels on the Gamma sphere: src/coulomb.jl (Coulomb with ProbeCharge / ReplaceSingularity,
  ShortRangeCoulomb, SphericallyTruncatedCoulomb; the long-range formula for the sum rule);
* ``exchange_apply``: apply!(Hpsi, ::ExchangeOperator, psi) (src/terms/operators.jl:192-210) between the transforms of
  compress_exchange (src/terms/exact_exchange.jl:136-154);
* ``exchange_energy``: exx_energy_only (:162-183), the m <= n pair sum;
* ``ace``: compress_exchange (:136-154).

Every transform is the oracle's sphere <-> cube transform of the k-point (scipy.fft); ``longdouble=True`` runs the same
loops in extended precision (scipy.fft transforms long double natively) to measure the twin's own round-off.
Test helper: imported by tests/test_exx_host.py and tests/test_gpu_exx_kernels.py, no test of its own.
"""
import math

import numpy as np
import scipy.fft as sfft


# ----------------------------------------------------------------------------------------------- interaction kernels
def sphere_G2(basis, kpt=None):
    """|G|^2 (cartesian) of every row of the Gamma sphere; row 0 is G = 0 (the mapping ascends)"""
    kpt = basis.kpoints[0] if kpt is None else kpt
    if np.any(kpt.coordinate != 0) or np.any(kpt.G_vectors[0] != 0):
        raise ValueError("exact exchange: Gamma point only")
    G = basis.Gplusk_vectors_cart(kpt)
    return np.sum(G * G, axis=1)


def _with_G0(formula, G2, value):
    out = np.empty_like(G2)
    out[1:] = formula(G2[1:])
    out[0] = value
    return out


def kernel_coulomb_replace(basis, value):
    """Coulomb(ReplaceSingularity(value)) (coulomb.jl:353-363)"""
    return _with_G0(lambda g2: 4 * math.pi / g2, sphere_G2(basis), value)


def kernel_coulomb_probe_charge(basis, alpha=None):
    """Coulomb(ProbeCharge(alpha)) (coulomb.jl:312-339): alpha = pi^2 / Ecut"""
    alpha = math.pi ** 2 / basis.Ecut if alpha is None else alpha
    G2 = sphere_G2(basis)
    K = 4 * math.pi / G2[1:]
    recip_cell_volume = abs(np.linalg.det(basis.model.recip_lattice))
    integral = 8 * math.pi ** 2 * math.sqrt(math.pi / alpha) / recip_cell_volume
    return np.concatenate([[integral - np.sum(K * np.exp(-alpha * G2[1:]))], K])


def kernel_short_range(basis, mu):
    """ShortRangeCoulomb(mu): erfc(mu r) / r (coulomb.jl:68-80)"""
    return _with_G0(lambda g2: -(4 * math.pi / g2) * np.expm1(-g2 / (4 * mu ** 2)), sphere_G2(basis), math.pi / mu ** 2)


def long_range_formula(basis, mu):
    """eval_kernel_fourier(::LongRangeCoulomb) (coulomb.jl:93-95) off G = 0 (NaN there): erf(mu r) / r"""
    return _with_G0(lambda g2: (4 * math.pi / g2) * np.exp(-g2 / (4 * mu ** 2)), sphere_G2(basis), math.nan)


def kernel_spherically_truncated(basis, Rcut=None):
    """SphericallyTruncatedCoulomb(Rcut) (coulomb.jl:156-172): Rcut = cbrt(3 Omega / 4 pi)"""
    Rcut = np.cbrt(3 * basis.model.unit_cell_volume / (4 * math.pi)) if Rcut is None else Rcut
    return _with_G0(lambda g2: 4 * math.pi / g2 * (1 - np.cos(Rcut * np.sqrt(g2))), sphere_G2(basis),
                    2 * math.pi * Rcut ** 2)


# ----------------------------------------------------------------------------------------------- transforms
def _types(longdouble):
    return (np.longdouble, np.clongdouble) if longdouble else (np.float64, np.complex128)


def ifft(basis, kpt, c, longdouble=False):
    """ifft(basis, kpt, c) (fft.jl:110-122): sphere coefficients (n_G,) or (n_G, m) -> cube(s) ([m,] nz, ny, nx), normalised"""
    rt, ct = _types(longdouble)
    nx, ny, nz = basis.fft_size
    c = np.asarray(c)
    cols = c.reshape(len(kpt.mapping), -1).T
    cube = np.zeros((cols.shape[0], basis.N), dtype=ct)
    cube[:, kpt.mapping] = cols
    out = sfft.ifftn(cube.reshape(-1, nz, ny, nx), axes=(1, 2, 3), norm="forward") / np.sqrt(rt(basis.model.unit_cell_volume))
    return out[0] if c.ndim == 1 else out


def fft(basis, kpt, f, longdouble=False):
    """fft(basis, kpt, f) (fft.jl:162-172): cube(s) -> the coefficients on the k-point's sphere, (n_G,) or (n_G, m)"""
    rt, ct = _types(longdouble)
    f = np.asarray(f, dtype=ct)
    out = sfft.fftn(f, axes=(-3, -2, -1), norm="backward").reshape(f.shape[:-3] + (-1,))[..., kpt.mapping]
    return (out * (np.sqrt(rt(basis.model.unit_cell_volume)) / basis.N)).T


# ----------------------------------------------------------------------------------------------- operator, energy, ACE
def exchange_apply(basis, kpt, kernel, phi, weights, psi, longdouble=False):
    """W[:, m] = Vx psi[:, m]: Hpsi.real .-= (occ_n / filled) phi_n(r) ifft(K fft(conj(phi_n(r)) psi(r))) over the
    orbitals phi[:, n] with weights[n] = occ_n / filled_occupation, then fft! onto the sphere (all columns m at once)."""
    rt, ct = _types(longdouble)
    phi, psi = np.asarray(phi, dtype=ct), np.asarray(psi, dtype=ct)
    kernel, weights = np.asarray(kernel, dtype=rt), np.asarray(weights, dtype=rt)
    psi_real = ifft(basis, kpt, psi, longdouble)
    acc = np.zeros(psi_real.shape, dtype=ct)
    for n in range(phi.shape[1]):
        phin = ifft(basis, kpt, phi[:, n], longdouble)
        x_four = fft(basis, kpt, np.conj(phin)[None] * psi_real, longdouble)
        acc -= weights[n] * phin[None] * ifft(basis, kpt, x_four * kernel[:, None], longdouble)
    return fft(basis, kpt, acc, longdouble)


def exchange_matrix(basis, kpt, kernel, phi, weights):
    """the dense n_G x n_G matrix of Vx (small spheres only)"""
    return exchange_apply(basis, kpt, kernel, phi, weights, np.eye(len(kpt.mapping), dtype=complex))


def exchange_energy(basis, kpt, kernel, psi_occ, occ, filled_occupation):
    """exx_energy_only (exact_exchange.jl:162-183)"""
    real = [ifft(basis, kpt, psi_occ[:, n]) for n in range(psi_occ.shape[1])]
    E = 0.0
    for n in range(len(real)):
        for m in range(n + 1):
            rho_mn = fft(basis, kpt, np.conj(real[m]) * real[n])
            fac = occ[n] * occ[m] / filled_occupation * (2 if m != n else 1)
            E -= 0.5 * fac * np.real(np.vdot(rho_mn * kernel, rho_mn))
    return float(E)


def n_occupied(occ, occupation_threshold=0.0):
    """occupied_empty_masks (occupation.jl:242-249): bands 1 .. the last one with |occupation| above the threshold"""
    idx = np.nonzero(np.abs(np.asarray(occ, dtype=float)) > occupation_threshold)[0]
    return int(idx[-1]) + 1 if len(idx) else 0


def ace(basis, kpt, kernel, psi, occ, filled_occupation, occupation_threshold=0.0, sketch_with_extra_orbitals=True):
    """exx_operator(::AceExx) (exact_exchange.jl:104-154): W = Vx psi on the sketch, M = psi' W, -M = L L',
    xi = W L^-H; the compressed operator is -xi xi'.  E = 1/2 sum_n occ_n Re M_nn."""
    occ = np.asarray(occ, dtype=float)
    n_occ = n_occupied(occ, occupation_threshold)
    n_sk = len(occ) if sketch_with_extra_orbitals else n_occ
    W = exchange_apply(basis, kpt, kernel, psi[:, :n_occ], occ[:n_occ] / filled_occupation, psi[:, :n_sk])
    M = psi[:, :n_sk].conj().T @ W
    M = (M + M.conj().T) / 2
    L = np.linalg.cholesky(-M)
    xi = np.linalg.solve(L, W.conj().T).conj().T       # W L^-H
    E = 0.5 * float(np.real(np.sum(np.diag(M) * occ[:n_sk])))
    return dict(W=W, M=M, xi=xi, E=E, n_sketch=n_sk, n_occ=n_occ)


# ----------------------------------------------------------------------------------------------- shapes of the kernel tests
# (shared by tests/test_gpu_exx_kernels.py, which holds the device to RTOL_FFT on them, and tests/test_exx_host.py, which
# checks without a GPU that the twin itself is good to a tenth of that)
RTOL_FFT = 1e-12          # the suite's bound for chained FFT identities (RTOL of tests/test_gpu_kernels.py)
TRICLINIC = np.array([[8.0, 0.5, -0.4], [0.7, 9.5, 0.6], [0.3, 0.9, 11.5]])
KERNEL_TEST_GRIDS = {"triclinic_12x15x18": (5.0, (12, 15, 18), TRICLINIC), "cubic_18": (5.0, (18, 18, 18), None)}
_cache = {}


def kernel_test_basis(grid):
    """the oracle basis of one grid: silicon atoms, Gamma only; lattice None = the fcc silicon cell"""
    if ("basis", grid) not in _cache:
        import oracle
        Ecut, fft_size, lattice = KERNEL_TEST_GRIDS[grid]
        lat, atoms, pos = oracle.basis.silicon_primitive()
        model = oracle.Model(lat if lattice is None else lattice, atoms, pos, terms=("Kinetic",))
        _cache[("basis", grid)] = oracle.PlaneWaveBasis(model, Ecut, oracle.ExplicitKpoints([[0.0, 0.0, 0.0]], [1.0]),
                                                        fft_size=fft_size)
    return _cache[("basis", grid)]


def kernel_test_case(grid, n_occ, n_bands):
    """inputs and the twin's results of one shape, computed once: (phi, w, K, psi, W0, Vx psi, the twin's own error =
    complex128 against long double, relative to max |Vx psi|)"""
    key = (grid, n_occ, n_bands)
    if key not in _cache:
        ob = kernel_test_basis(grid)
        kpt = ob.kpoints[0]
        n = len(kpt.mapping)
        rng = np.random.default_rng(1000 * n_occ + n_bands + len(grid))
        phi = np.linalg.qr(rng.standard_normal((n, n_occ)) + 1j * rng.standard_normal((n, n_occ)))[0]
        psi = rng.standard_normal((n, n_bands)) + 1j * rng.standard_normal((n, n_bands))
        W0 = rng.standard_normal((n, n_bands)) + 1j * rng.standard_normal((n, n_bands))
        w = rng.uniform(0.1, 1.0, n_occ)
        K = 0.25 * kernel_coulomb_probe_charge(ob)
        ref = exchange_apply(ob, kpt, K, phi, w, psi)
        ref_ld = exchange_apply(ob, kpt, K, phi, w, psi, longdouble=True)
        _cache[key] = (phi, w, K, psi, W0, ref, float(np.abs(ref - ref_ld).max() / np.abs(ref_ld).max()))
    return _cache[key]


# ----------------------------------------------------------------------------------------------- HF / hybrid models, dense
class HybridTwin:
    """A model with exact exchange on top of the oracle: every other term comes from ``oracle.energy_hamiltonian`` of the
    model WITHOUT the exchange term; a scaled exchange functional (PBE0: (1 - a) gga_x_pbe) is the full Xc minus a times an
    Xc of that functional alone (the Xc term is linear in its functionals).

    ``scaling_factor``: of the ExactExchange term; ``kernel``: the unscaled kernel on the Gamma sphere (a function of the
    oracle basis); ``functionals``: None for Hartree-Fock (no Xc term), else the Xc functionals with ``x_scale`` on the first.
    """

    def __init__(self, lattice, atoms, positions, Ecut, fft_size, kernel, scaling_factor=1.0, functionals=None,
                 x_scale=1.0, **model_kw):
        import oracle
        gamma = oracle.ExplicitKpoints([[0.0, 0.0, 0.0]], [1.0])
        if functionals is None:
            model = oracle.model_atomic(lattice, atoms, positions, extra_terms=("Hartree",), **model_kw)
        else:
            model = oracle.model_DFT(lattice, atoms, positions, functionals=tuple(functionals), **model_kw)
        self.oracle = oracle
        self.basis = oracle.PlaneWaveBasis(model, Ecut, gamma, fft_size=fft_size)
        self.model = model
        self.x_scale = float(x_scale) if functionals is not None else 1.0
        self.x_basis = None
        if self.x_scale != 1.0:
            xm = oracle.Model(lattice, atoms, positions, terms=("Xc",), functionals=(functionals[0],), **model_kw)
            self.x_basis = oracle.PlaneWaveBasis(xm, Ecut, gamma, fft_size=fft_size)
        self.scaling_factor = float(scaling_factor)
        self.K = self.scaling_factor * kernel(self.basis)
        self.filled = model.filled_occupation

    def energy_hamiltonian(self, psi, occupation, rho, occupation_threshold=0.0):
        """-> (energies with "ExactExchange", [oracle HamiltonianBlock], [(phi, weights) of the exchange operator])"""
        b = self.basis
        E, ham = self.oracle.energy_hamiltonian(b, psi, occupation, rho=rho)
        if self.x_basis is not None:
            Ex, hx = self.oracle.energy_hamiltonian(self.x_basis, None, None, rho=rho)
            E["Xc"] = E["Xc"] - (1 - self.x_scale) * Ex["Xc"]
            for H, Hx in zip(ham, hx):
                H.potential = H.potential - (1 - self.x_scale) * Hx.potential
        exx, e = [], 0.0
        for ik, kpt in enumerate(b.kpoints):
            if psi is None or occupation is None:
                exx.append(None)
                continue
            n_occ = n_occupied(occupation[ik], occupation_threshold)
            occ = np.asarray(occupation[ik], dtype=float)[:n_occ]
            e += exchange_energy(b, kpt, self.K, psi[ik][:, :n_occ], occ, self.filled)
            exx.append((psi[ik][:, :n_occ], occ / self.filled))
        E["ExactExchange"] = e
        return E, ham, exx

    def apply(self, ham, exx, ik, psi):
        """H psi of k-block ik"""
        out = ham[ik].mul(psi)
        if exx[ik] is not None:
            out = out + exchange_apply(self.basis, self.basis.kpoints[ik], self.K, exx[ik][0], exx[ik][1], psi)
        return out

    def dense(self, ham, exx, ik):
        H = self.apply(ham, exx, ik, np.eye(len(self.basis.kpoints[ik].mapping), dtype=complex))
        return (H + H.conj().T) / 2

    def scf(self, rho, psi=None, occupation=None, damping=0.4, tol=1e-11, maxiter=200, n_bands=None, record_at=(),
            compressed=True):
        """Dense fixed-point iteration: H[rho_in, psi] is diagonalised exactly, rho_in += damping (rho_out - rho_in).
        ``compressed`` (the reference's SCF default, exxalg = AceExx()): the exchange operator of a step is the ACE of the
        previous step's ``n_bands`` orbitals, exact on their span only -- the same fixed point as with the full operator,
        another path to it.
        (Plain damping: Anderson acceleration on the density alone stalls near 1e-7 here, the orbitals that build the exchange
        operator lag one step behind the density it extrapolates.)  Returns the state at convergence and, for every residual
        in ``record_at``, the state of the first iterate whose residual is below it."""
        from oracle.scf import compute_density, compute_occupation
        b = self.basis
        rho_in = rho
        recorded = {}
        for it in range(maxiter):
            _, ham, exx = self.energy_hamiltonian(psi, occupation, rho_in)
            psi_prev, occ_prev = psi, occupation
            eig, psi = [], []
            for ik in range(len(b.kpoints)):
                if compressed and exx[ik] is not None:
                    a = ace(b, b.kpoints[ik], self.K, psi_prev[ik], occ_prev[ik], self.filled)
                    H = ham[ik].to_dense() - a["xi"] @ a["xi"].conj().T
                    H = (H + H.conj().T) / 2
                else:
                    H = self.dense(ham, exx, ik)
                lam, V = np.linalg.eigh(H)
                nb = len(lam) if n_bands is None else n_bands
                eig.append(lam[:nb])
                psi.append(V[:, :nb])
            occupation, eF = compute_occupation(b, eig)
            rho_out = compute_density(b, psi, occupation)
            drho = float(np.linalg.norm(rho_out - rho_in) * math.sqrt(b.dvol))
            state = dict(psi=psi, occupation=occupation, eigenvalues=eig, rho=rho_out, drho=drho, n_iter=it + 1, eF=eF)
            for r in record_at:
                if r not in recorded and drho < r:
                    recorded[r] = dict(state, energies=self.energy_hamiltonian(psi, occupation, rho_out)[0])
            if drho < tol:
                break
            rho_in = rho_in + damping * (rho_out - rho_in)
        state["energies"] = self.energy_hamiltonian(psi, occupation, rho_out)[0]
        state["recorded"] = recorded
        return state
