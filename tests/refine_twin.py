"""NumPy twin of the transfer layer and of the refinement metric (src/transfer.jl, src/postprocess/refine.jl:20-84), for the
tests of dftk_jl_amd/transfer.py, dftk_mi_transfer_*, dftk_mi_refinement_metric_solve and invert_refinement_metric.

Independent of the package under test: it works on the oracle's ``PlaneWaveBasis`` (or on bare mappings and FFT sizes) with
dictionaries of integer G vectors and dense matrices, and calls nothing of dftk_jl_amd.

* ``transfer_mapping_cubes``: the reference's eight index blocks, literally (1-based ranges turned 0-based).
* ``transfer_mapping_cubes_by_G``: the same correspondence by dictionary look-up of the integer G of every index.
* ``transfer_mapping_kpt``: ``(idcs_in, idcs_out)`` of two k-points by dictionary look-up of G - dG.
* ``transfer_blochwave_kpt``, ``transfer_density``: the reference's functions on NumPy arrays.
* ``metric_dense``, ``metric_solve_dense``: M_n as a dense matrix and the minimum-norm solution of M_n x = P res.
* ``refine_scfres_dense``: refine.jl:116-167 with dense operators -- dense H_k of both bases handed in, the Hartree kernel
  from numpy FFTs, f_xc handed in (``fxc_central``: central differences of a v_xc), (Omega + K)_11 inverted exactly by
  applying the twin's own ``apply_Omega_dense`` + ``apply_K_dense`` to a real basis of the tangent space.
"""
import itertools

import numpy as np


def G_axis(n):
    """[0 .. floor((n-1)/2), -ceil((n-1)/2) .. -1] (fft.jl:24-31)"""
    stop = (n - 1) // 2
    return np.array(list(range(0, stop + 1)) + list(range(stop - (n - 1), 0)), dtype=np.int64)


# ------------------------------------------------------------------------------------------ cubes
def _axis_blocks(fft_in, fft_out):
    """transfer.jl:14-26 for one axis, 0-based half-open ranges: ((in_a, in_b), (out_a, out_b))"""
    if fft_in <= fft_out:
        a, b = -(-fft_in // 2), fft_in // 2
        return ((range(0, a), range(a, fft_in)), (range(0, a), range(fft_out - b, fft_out)))
    a, b = -(-fft_out // 2), fft_out // 2
    return ((range(0, a), range(fft_in - b, fft_in)), (range(0, a), range(a, fft_out)))


def transfer_mapping_cubes(fft_in, fft_out):
    """The eight pairs ``(block_in, block_out)`` of transfer.jl:10-31; a block is a triple of index ranges (x, y, z)."""
    ax = [_axis_blocks(i, o) for i, o in zip(fft_in, fft_out)]
    pairs = []
    for cz, cy, cx in itertools.product((0, 1), repeat=3):          # Iterators.product: x fastest
        block_in = (ax[0][0][cx], ax[1][0][cy], ax[2][0][cz])
        block_out = (ax[0][1][cx], ax[1][1][cy], ax[2][1][cz])
        pairs.append((block_in, block_out))
    return pairs


def transfer_cube_fourier(c_in, fft_in, fft_out):
    """``x_out_fourier[block_out] = x_in_fourier[block_in]`` over the eight blocks; cubes are (nz, ny, nx) arrays"""
    out = np.zeros((fft_out[2], fft_out[1], fft_out[0]), dtype=complex)
    for (bx, by, bz), (ox, oy, oz) in transfer_mapping_cubes(fft_in, fft_out):
        if len(bx) == 0 or len(by) == 0 or len(bz) == 0:
            continue
        out[np.ix_(list(oz), list(oy), list(ox))] = c_in[np.ix_(list(bz), list(by), list(bx))]
    return out


def transfer_mapping_cubes_by_G(fft_in, fft_out):
    """{(ix, iy, iz) of the output cube: (ix, iy, iz) of the input cube} by dictionary look-up of the integer G: indices of
    equal G correspond, over the G range of the shorter axis."""
    per_axis = []
    for n_in, n_out in zip(fft_in, fft_out):
        where_in = {int(g): i for i, g in enumerate(G_axis(n_in))}
        per_axis.append({o: where_in[int(g)] for o, g in enumerate(G_axis(n_out)) if int(g) in where_in})
    return {(ox, oy, oz): (per_axis[0][ox], per_axis[1][oy], per_axis[2][oz])
            for ox in per_axis[0] for oy in per_axis[1] for oz in per_axis[2]}


def transfer_density(rho_in, fft_in, fft_out):
    """transfer.jl:165-178 with the inverse transform of this project (complex transform, real part): rho on (.., nz, ny, nx).
    The normalisations of fft(basis_in) and irfft(basis_out) combine to 1 / N_in."""
    rho_in = np.asarray(rho_in, dtype=float)
    if rho_in.ndim == 4:
        return np.stack([transfer_density(r, fft_in, fft_out) for r in rho_in])
    c_in = np.fft.fftn(rho_in)
    c_out = transfer_cube_fourier(c_in, fft_in, fft_out)
    return np.real(np.fft.ifftn(c_out)) * (np.prod(fft_out) / np.prod(fft_in))


# ------------------------------------------------------------------------------------------ spheres
def G_of_mapping(mapping, fft_size):
    nx, ny, nz = fft_size
    m = np.asarray(mapping, dtype=np.int64)
    return np.stack([G_axis(nx)[m % nx], G_axis(ny)[(m // nx) % ny], G_axis(nz)[m // (nx * ny)]], axis=1)


def transfer_mapping_kpt(mapping_in, fft_in, mapping_out, fft_out, dG=(0, 0, 0)):
    """``(idcs_in, idcs_out)`` of transfer.jl:46-83 (0-based): row idcs_in[j] of the input block carries G, row idcs_out[j] of
    the output block carries G - dG.  G - dG outside the output cube or outside the output sphere: the pair is dropped."""
    G_in = G_of_mapping(mapping_in, fft_in)
    row_out = {tuple(int(x) for x in g): r for r, g in enumerate(G_of_mapping(mapping_out, fft_out))}
    idcs_in, idcs_out = [], []
    for r, g in enumerate(G_in):
        key = (int(g[0]) - int(dG[0]), int(g[1]) - int(dG[1]), int(g[2]) - int(dG[2]))
        if key in row_out:
            idcs_in.append(r)
            idcs_out.append(row_out[key])
    return np.array(idcs_in, dtype=np.int64), np.array(idcs_out, dtype=np.int64)


def transfer_blochwave_kpt(psik_in, mapping_in, fft_in, mapping_out, fft_out, dG=(0, 0, 0)):
    """transfer.jl:112-124: psik_in is (n_G_in, n_bands); the result (n_G_out, n_bands), zero where no partner exists"""
    idcs_in, idcs_out = transfer_mapping_kpt(mapping_in, fft_in, mapping_out, fft_out, dG)
    out = np.zeros((len(mapping_out), psik_in.shape[1]), dtype=psik_in.dtype)
    out[idcs_out] = psik_in[idcs_in]
    return out


# ------------------------------------------------------------------------------------------ metric
def proj_perp(psik):
    return np.eye(psik.shape[0]) - psik @ psik.conj().T


def metric_dense(psik, kin, n):
    """M_n = P T_n^{1/2} P T_n^{1/2} P with T_n = kin + mean_kin[n], mean_kin[n] = sum kin |psi_n|^2 (refine.jl:20-25, :45-51)"""
    P = proj_perp(psik)
    mean_kin = float(np.sum(kin * np.abs(psik[:, n]) ** 2))
    sq = np.sqrt(kin + mean_kin)
    return P @ (sq[:, None] * P * sq[None, :]) @ P


def metric_solve_dense(psik, kin, res):
    """x_n with M_n x_n = P res_n and psi' x_n = 0, column by column: M_n is positive definite on the range of P, so the
    solution is that of the full-rank matrix M_n + psi psi' (which maps the range of P onto itself)."""
    P = proj_perp(psik)
    out = np.zeros_like(res)
    for n in range(res.shape[1]):
        M = metric_dense(psik, kin, n)
        out[:, n] = P @ np.linalg.solve(M + psik @ psik.conj().T, P @ res[:, n])
    return out


# ------------------------------------------------------------------------------------------ refine_scfres, dense
# A "side" describes one basis by plain arrays: fft_size, volume, recip (3 x 3, columns = reciprocal vectors in the
# convention G_cart = recip @ G_red), weights [k], mappings [k], H [k] (dense n_G x n_G), fxc (nz, ny, nx) = f_xc at the
# density the kernel is taken at, and on the large side kin [k] and Hgrad [k] (the dense Hamiltonian of the density of the
# transferred orbitals, which the projected gradient uses).
def fxc_central(v_xc, rho, h=1e-5):
    """f_xc = d v_xc / d rho by central differences with the relative step h (v_xc: a point-wise function of rho)"""
    rho = np.asarray(rho, dtype=float)
    return (v_xc(rho * (1 + h)) - v_xc(rho * (1 - h))) / (2 * h * rho)


def _to_real_space(side, k, c):
    """psi(r) = sum_G c_G e^{iG.r} / sqrt(volume) on the (nz, ny, nx) grid, for the columns of c"""
    nx, ny, nz = side["fft_size"]
    cube = np.zeros((c.shape[1], nx * ny * nz), dtype=complex)
    cube[:, side["mappings"][k]] = c.T
    return np.fft.ifftn(cube.reshape(-1, nz, ny, nx), axes=(1, 2, 3)) * (nx * ny * nz) / np.sqrt(side["volume"])


def _to_sphere(side, k, f):
    nx, ny, nz = side["fft_size"]
    c = np.fft.fftn(f, axes=(1, 2, 3)).reshape(f.shape[0], -1)[:, side["mappings"][k]]
    return c.T * np.sqrt(side["volume"]) / (nx * ny * nz)


def delta_rho_dense(side, psi, dpsi, occ):
    out = 0.0
    for k, w in enumerate(side["weights"]):
        p, d = _to_real_space(side, k, psi[k]), _to_real_space(side, k, dpsi[k])
        out = out + w * np.einsum("n,nzyx->zyx", np.asarray(occ[k], dtype=float), 2 * np.real(np.conj(p) * d))
    return out


def kernel_dense(side, drho):
    """dV = v_c * drho + f_xc drho (hartree.jl:68-81, xc.jl:245-330)"""
    nx, ny, nz = side["fft_size"]
    gz, gy, gx = np.meshgrid(G_axis(nz), G_axis(ny), G_axis(nx), indexing="ij")
    Gc = np.stack([gx, gy, gz], axis=-1).astype(float) @ np.asarray(side["recip"], dtype=float).T
    G2 = np.sum(Gc * Gc, axis=-1)
    green = np.where(G2 > 0, 4 * np.pi / np.where(G2 > 0, G2, 1.0), 0.0)
    return np.real(np.fft.ifftn(green * np.fft.fftn(drho))) + side["fxc"] * drho


def apply_Omega_dense(side, dpsi, psi):
    out = []
    for k in range(len(psi)):
        P, H = proj_perp(psi[k]), side["H"][k]
        d = P @ dpsi[k]
        out.append(P @ (H @ d - d @ (psi[k].conj().T @ H @ psi[k])))
    return out


def apply_K_dense(side, dpsi, psi, occ):
    d = [proj_perp(p) @ x for p, x in zip(psi, dpsi)]
    dV = kernel_dense(side, delta_rho_dense(side, psi, d, occ))
    return [proj_perp(psi[k]) @ _to_sphere(side, k, dV[None] * _to_real_space(side, k, psi[k])) for k in range(len(psi))]


def solve_OmegaPlusK_dense(side, psi, rhs, occ):
    """d on the tangent space with (Omega + K) d = -P rhs, exactly: the operator is applied to a real basis of the tangent
    space (K is only R-linear) and the dense system solved."""
    Q = []                                                  # orthonormal bases of the complements of psi_k
    for p in psi:
        u, _, _ = np.linalg.svd(np.eye(p.shape[0]) - p @ p.conj().T)
        Q.append(u[:, :p.shape[0] - p.shape[1]])
    shapes = [(q.shape[1], p.shape[1]) for q, p in zip(Q, psi)]
    sizes = [2 * a * b for a, b in shapes]

    def unpack(x):
        out, at = [], 0
        for (a, b), q, n in zip(shapes, Q, sizes):
            v = x[at:at + n]
            out.append(q @ (v[:a * b] + 1j * v[a * b:]).reshape(a, b))
            at += n
        return out

    def pack(blocks):
        parts = []
        for q, blk in zip(Q, blocks):
            c = (q.conj().T @ blk).reshape(-1)
            parts += [c.real, c.imag]
        return np.concatenate(parts)

    def op(d):
        return [a + b for a, b in zip(apply_Omega_dense(side, d, psi), apply_K_dense(side, d, psi, occ))]

    D = sum(sizes)
    A = np.zeros((D, D))
    for j in range(D):
        e = np.zeros(D)
        e[j] = 1.0
        A[:, j] = pack(op(unpack(e)))
    return unpack(np.linalg.solve(A, -pack(rhs)))


def refine_scfres_dense(small, large, psi, occ):
    """refine.jl:116-167 with dense operators; psi: the occupied orbitals [k] on the small basis (n_G x n_occ).
    Returns dict(psir, res, e2, e1, dpsi, drho)."""
    nk = len(psi)
    up = lambda x: [transfer_blochwave_kpt(x[k], small["mappings"][k], small["fft_size"], large["mappings"][k],  # noqa: E731
                                           large["fft_size"]) for k in range(nk)]
    down = lambda x: [transfer_blochwave_kpt(x[k], large["mappings"][k], large["fft_size"], small["mappings"][k],  # noqa: E731
                                             small["fft_size"]) for k in range(nk)]
    psir = up(psi)
    res = [-(proj_perp(psir[k]) @ (large["Hgrad"][k] @ psir[k])) for k in range(nk)]
    resLF = down(res)
    resHF = [r - x for r, x in zip(res, up(resLF))]
    e2 = [metric_solve_dense(psir[k], large["kin"][k], resHF[k]) for k in range(nk)]
    OpKe2 = [a + b for a, b in zip(apply_Omega_dense(large, e2, psir), apply_K_dense(large, e2, psir, occ))]
    rhs = [a - b for a, b in zip(down(OpKe2), resLF)]
    e1_small = solve_OmegaPlusK_dense(small, psi, rhs, occ)
    e1 = up(e1_small)
    dpsi = [a + b for a, b in zip(e1, e2)]
    return dict(psir=psir, res=res, e2=e2, e1=e1, dpsi=dpsi, drho=delta_rho_dense(large, psir, dpsi, occ))
