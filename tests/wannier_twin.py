"""NumPy twin of the symmetry / Wannier kernels (not a test): the reference's loops written out literally on the oracle's
basis tables -- ``apply_symop`` (src/symmetry.jl:229-270), ``overlap_Mmn_k_kpb`` and ``compute_amn_kpoint``
(src/external/wannier_shared.jl:220-241, :278-298).  A k-point is given by its ``mapping`` (0-based cube indices of the
sphere rows, ascending) and the FFT size; orbital blocks are (n_G, n_bands).  ``dtype=np.clongdouble`` evaluates phases and
sums in extended precision (the reference values of the kernel tests), ``np.complex128`` is the fp64 twin.  The loops over
plane waves are literal; the loop over bands is a NumPy row operation.
"""
import numpy as np

PI_LD = np.longdouble("3.14159265358979323846264338327950288")


def G_axis(n):
    """[0 .. floor((n-1)/2), -ceil((n-1)/2) .. -1] (fft.jl:24-31)"""
    stop = (n - 1) // 2
    return np.array(list(range(0, stop + 1)) + list(range(stop - (n - 1), 0)), dtype=np.int64)


def G_of_mapping(mapping, fft_size):
    nx, ny, nz = fft_size
    m = np.asarray(mapping, dtype=np.int64)
    return np.stack([G_axis(nx)[m % nx], G_axis(ny)[(m // nx) % ny], G_axis(nz)[m // (nx * ny)]], axis=1)


def row_of_G(mapping, fft_size):
    """index_G_vectors(basis, kpoint, .) as a dictionary {G: row}"""
    return {tuple(int(x) for x in g): r for r, g in enumerate(G_of_mapping(mapping, fft_size))}


def normalize_kpoint_coordinate(k):
    k = np.asarray(k, dtype=float)
    return k - np.floor(k + 0.5)


def cis2pi(x, dtype):
    """e^{2 pi i x} in the real type of ``dtype``"""
    if dtype == np.clongdouble:
        x = np.longdouble(x)
        x = x - np.rint(x)
        return np.cos(2 * PI_LD * x) + 1j * np.sin(2 * PI_LD * x)
    return complex(np.cos(2 * np.pi * x), np.sin(2 * np.pi * x))


def symop_image(S, kcoord):
    """(Sk in [-0.5, 0.5)^3, kshift = Sk - S k) (symmetry.jl:236-240)"""
    kcoord = np.asarray(kcoord, dtype=float)
    assert np.all((-0.5 <= kcoord) & (kcoord < 0.5))
    Sk_raw = np.asarray(S, dtype=float) @ kcoord
    Sk = normalize_kpoint_coordinate(Sk_raw)
    return Sk, np.rint(Sk - Sk_raw).astype(int)


def apply_symop(S, tau, kshift, mapping_k, mapping_Sk, fft_size, psi_k, dtype=np.clongdouble):
    """symmetry.jl:258-267: psi_Sk[ig] = cis2pi(-G_full . tau) psi_k[index of S^-1 G_full], G_full = G + kshift over the
    plane waves G of S k.  ``ValueError`` where the reference's ``@assert igired !== nothing`` fails.
    Also returns the phase arguments G_full . tau (fp64 magnitudes, for error bounds): (psi_Sk, sum_i |G_i tau_i|)."""
    invS = np.rint(np.linalg.inv(np.asarray(S, dtype=float))).astype(int)
    rows = row_of_G(mapping_k, fft_size)
    Gs_full = G_of_mapping(mapping_Sk, fft_size) + np.asarray(kshift, dtype=int)
    psi_k = np.asarray(psi_k)
    out = np.zeros((len(Gs_full), psi_k.shape[1]), dtype=dtype)
    real = np.longdouble if dtype == np.clongdouble else np.float64
    tau_r = np.asarray(tau, dtype=real)
    arg_mag = np.zeros(len(Gs_full))
    for ig, G_full in enumerate(Gs_full):
        igired = rows.get(tuple(int(x) for x in invS @ G_full))
        if igired is None:
            raise ValueError(f"apply_symop: S^-1 G = {invS @ G_full} is not a plane wave of the k-point")
        x = real(0)
        for a in range(3):
            x = x + real(int(G_full[a])) * tau_r[a]
        arg_mag[ig] = float(np.sum(np.abs(G_full * np.asarray(tau, dtype=float))))
        row = psi_k[igired, :].astype(dtype)
        out[ig, :] = row if not np.any(np.asarray(tau)) else cis2pi(-x, dtype) * row      # (tau = 0: cis2pi(0) = 1)
    return out, arg_mag


def overlap_Mmn_k_kpb(psi_k, mapping_k, psi_kpb, mapping_kpb, fft_kpb, fft_k, G_shift, n_bands, dtype=np.clongdouble,
                      identity_if_zero=True):
    """wannier_shared.jl:220-241: the common Fourier modes by look-up, then Mkb[m, n] = dot(psi_k[ip, m], psi_kpb[ip_plus_b, n]).
    Also returns sum_G |a| |b| per entry (error bounds): (Mkb, absM)."""
    rows_b = row_of_G(mapping_kpb, fft_kpb)
    ip, ip_plus_b = [], []
    for i, p in enumerate(G_of_mapping(mapping_k, fft_k)):
        j = rows_b.get(tuple(int(x) for x in p + np.asarray(G_shift, dtype=int)))
        if j is not None:
            ip.append(i)
            ip_plus_b.append(j)
    Mkb = np.zeros((n_bands, n_bands), dtype=dtype)
    absM = np.zeros((n_bands, n_bands))
    a = np.asarray(psi_k)[ip, :n_bands].astype(dtype)
    b = np.asarray(psi_kpb)[ip_plus_b, :n_bands].astype(dtype)
    for n in range(n_bands):
        for m in range(n_bands):
            Mkb[m, n] = np.sum(np.conj(a[:, m]) * b[:, n])
            absM[m, n] = float(np.sum(np.abs(a[:, m]) * np.abs(b[:, n])))
    if identity_if_zero and not np.any(Mkb):
        return np.eye(n_bands, dtype=dtype), absM
    return Mkb, absM


def compute_amn_kpoint(basis_like, kcoord, mapping, fft_size, psi_k, projections, n_bands, dtype=np.clongdouble):
    """wannier_shared.jl:278-298: per projection the guess at p = k + G of the sphere rows (the projection's own host
    callable, fp64), l2-normalised, then Ak[m, n] = dot(psi_k[:, m], coeffs)."""
    ps = G_of_mapping(mapping, fft_size).astype(float) + np.asarray(kcoord, dtype=float)
    Ak = np.zeros((n_bands, len(projections)), dtype=dtype)
    psi_k = np.asarray(psi_k).astype(dtype)
    for n, proj in enumerate(projections):
        gn_per = np.asarray(proj(basis_like, ps)).astype(dtype)
        coeffs = gn_per / np.sqrt(np.sum(np.abs(gn_per) ** 2))
        for m in range(n_bands):
            Ak[m, n] = np.sum(np.conj(psi_k[:, m]) * coeffs)
    return Ak
