// phonon_kernels.hip -- the explicit pieces of the dynamical matrix at q = 0 (src/postprocess/phonon.jl) for HGH
// pseudopotentials (gfx950 only).  Reduced coordinates throughout; R_s = position of atom s, g = G + k.
//
// Local term (local.jl:183-213).  The local energy of this library is E = sum_G Re[ W_s(G) e^{-2 pi i G.R_a} ] summed
// over the atoms, W_s(G) = ff_s(|G|) conj(R(G)) / N with R the unnormalised forward DFT of the total density
// (force_kernels.hip), unpaired Nyquist entries dropped.  So
//     dV_{alpha,s}(G) = -2 pi i G_alpha ff_s(|G|) e^{-2 pi i G.R_s} / sqrt(Omega)              (the perturbing potential)
//     d^2 E / dR_{a,beta} dR_{a,alpha} = -4 pi^2 sum_G G_alpha G_beta Re[ W_s(G) e^{-2 pi i G.R_a} ]
//
// Nonlocal term (nonlocal.jl:307-383).  The projector columns of atom s carry e^{-2 pi i g.R_s}: d_alpha P_s =
// -2 pi i g_alpha o P_s.  With Q = P_s' [psi | i g_x psi | i g_y psi | i g_z psi] (the operands of forces_nonlocal) and
// Y = D_s Q:
//     dH_{alpha,s} psi = -2 pi i [ g_alpha o (P_s D_s P_s' psi) - P_s D_s P_s' (g_alpha o psi) ]
//                      = -2 pi i g_alpha o (P_s Y_0) + 2 pi P_s Y_alpha
//     <psi| d_alpha d_beta (P_s D_s P_s') |psi> = (2 pi)^2 2 Re[ c_alpha' D_s c_beta - c_alphabeta' D_s c ],
//         c = P_s' psi, c_alpha = P_s'(g_alpha psi) = -i Q_alpha, c_alphabeta = P_s'(g_alpha g_beta psi)
// and the derivative of F_{a,alpha} = -4 pi sum_n w_n Re[ p_n' D_a q_{alpha,n} ] (forces_nonlocal) along (dpsi, dw).
// All sums run in a fixed order without atomics: two calls give bitwise equal results.  A Gamma-real block is handled in
// the general complex full-sphere layout with the block's complex projectors (as the Sternheimer solver does).
#include "common.h"
#include "batch.h"
#include "hgh_forms.h"
#include <algorithm>
#include <cmath>
#include <vector>

// ------------------------------------------------------------------------------------------------ local term
struct OneAtom {       // passed to kernels by value: no host table outlives the launch
    double par[8];     // rloc, Zion, c1..c4 of its species
    double r[3];
};

// out[alpha N + idx] = -2 pi i G_alpha ff(|G|) e^{-2 pi i G.R} / sqrt(Omega), unpaired Nyquist entries zero
__global__ __launch_bounds__(256) void k_dv_displacement(int nx, int ny, int nz, Mat3 B, OneAtom at, double inv_sqrt_vol,
                                                         cd* __restrict__ out) {
    const int64_t N = (int64_t)nx * ny * nz;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N) return;
    const int ix = (int)(idx % nx), iy = (int)((idx / nx) % ny), iz = (int)(idx / ((int64_t)nx * ny));
    double re = 0.0, im = 0.0;
    const double g[3] = {(double)signed_freq(ix, nx), (double)signed_freq(iy, ny), (double)signed_freq(iz, nz)};
    if (!unpaired_nyquist(ix, iy, iz, nx, ny, nz)) {
        double qx, qy, qz;
        recip_times(B, g[0], g[1], g[2], &qx, &qy, &qz);
        const double p = sqrt(qx * qx + qy * qy + qz * qz);
        const double ff = hgh_local_ff(at.par, (p * at.par[0]) * (p * at.par[0])) * inv_sqrt_vol;
        double sn, cs;
        sincos(-2.0 * M_PI * (g[0] * at.r[0] + g[1] * at.r[1] + g[2] * at.r[2]), &sn, &cs);
        re = ff * cs;
        im = ff * sn;
    }
#pragma unroll
    for (int al = 0; al < 3; ++al) {
        const double s = 2.0 * M_PI * g[al];           // (re + i im) (-i s) = s im - i s re
        out[(int64_t)al * N + idx] = make_double2(s * im, -s * re);
    }
}

__global__ __launch_bounds__(256) void k_real_parts(int64_t n, const cd* __restrict__ c, double scale,
                                                    double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = scale * c[i].x;
}

// partial[(6 a + c) n_blocks + block] = sum over this workgroup's cube points of G_alpha G_beta Re[ W_s(G) e^{-2 pi i G.R_a} ],
// c = xx, yy, zz, xy, xz, yz; W_s = ff_s conj(R) / N.  grid: (n_blocks, n_atoms); every thread walks the cube with the
// stride of the grid, so the order of the sum depends on the cube alone.
__global__ __launch_bounds__(256) void k_dynmat_local(int nx, int ny, int nz, Mat3 B, const double* __restrict__ par,
                                                      const int* __restrict__ species, const double* __restrict__ pos,
                                                      const cd* __restrict__ R, double inv_N, double* __restrict__ partial) {
    __shared__ double sh[4];
    const int a = blockIdx.y;
    const double* q = par + 8 * species[a];
    const double rx = pos[3 * a], ry = pos[3 * a + 1], rz = pos[3 * a + 2];
    const int64_t N = (int64_t)nx * ny * nz;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < N; idx += (int64_t)gridDim.x * 256) {
        const int ix = (int)(idx % nx), iy = (int)((idx / nx) % ny), iz = (int)(idx / ((int64_t)nx * ny));
        if (unpaired_nyquist(ix, iy, iz, nx, ny, nz)) continue;
        const double gx = (double)signed_freq(ix, nx), gy = (double)signed_freq(iy, ny), gz = (double)signed_freq(iz, nz);
        double qx, qy, qz;
        recip_times(B, gx, gy, gz, &qx, &qy, &qz);
        const double p = sqrt(qx * qx + qy * qy + qz * qz);
        const double ff = hgh_local_ff(q, (p * q[0]) * (p * q[0])) * inv_N;
        double sn, cs;
        sincos(-2.0 * M_PI * (gx * rx + gy * ry + gz * rz), &sn, &cs);
        const cd r = R[idx];
        const double v = ff * (r.x * cs + r.y * sn);         // Re[ conj(R) e^{i phase} ]
        s[0] += gx * gx * v;
        s[1] += gy * gy * v;
        s[2] += gz * gz * v;
        s[3] += gx * gy * v;
        s[4] += gx * gz * v;
        s[5] += gy * gz * v;
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const double t = block_sum<256>(s[c], sh);
        if (threadIdx.x == 0) partial[(int64_t)(6 * a + c) * gridDim.x + blockIdx.x] = t;
    }
}

static int cube_block(const char* who, const dftk_mi_kblock* cube_kb) {
    const dftk_mi_basis* b = cube_kb->basis;
    if (cube_kb->n_G != (int64_t)b->nx * b->ny * b->nz || cube_kb->sh_comm) {
        dftk_set_error("%s: the k-block must span the whole cube", who);
        return DFTK_MI_EINVAL;
    }
    return 0;
}

extern "C" int dftk_mi_local_potential_displacement(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, int n_species,
                                                    const double* params_h, int species, const double* position_h,
                                                    double* out_d) {
    if (!cube_kb || !recip_lattice_h || !params_h || !position_h || !out_d || species < 0 || species >= n_species)
        return DFTK_MI_EINVAL;
    CHK(cube_block("local_potential_displacement", cube_kb));
    dftk_mi_basis* b = cube_kb->basis;
    HIPCHK(hipSetDevice(b->device));
    const int64_t N = (int64_t)b->nx * b->ny * b->nz;
    OneAtom at;
    for (int i = 0; i < 8; ++i) at.par[i] = params_h[8 * species + i];
    for (int i = 0; i < 3; ++i) at.r[i] = position_h[i];
    CHK(scratch_grow(b, b->dense_ws, 6 * (size_t)N * sizeof(cd)));
    cd* c1 = reinterpret_cast<cd*>(b->dense_ws.get());
    cd* c2 = c1 + 3 * N;
    const double inv_sqrt_vol = 1.0 / sqrt(b->volume);
    hipLaunchKernelGGL(k_dv_displacement, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, b->stream, b->nx, b->ny, b->nz,
                       make_mat3(recip_lattice_h), at, inv_sqrt_vol, c1);
    HIPCHK(hipGetLastError());
    CHK(launch_ifft_to_cube(cube_kb, c1, c2, 3));        // the three cubes through ONE transform pipeline
    hipLaunchKernelGGL(k_real_parts, dim3((unsigned)((3 * N + 255) / 256)), dim3(256), 0, b->stream, 3 * N, (const cd*)c2,
                       inv_sqrt_vol, out_d);            // ifft_normalization (fft.jl:87)
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int dftk_mi_dynmat_local(dftk_mi_kblock* cube_kb, const double* recip_lattice_h, int n_species,
                                    const double* params_h, int n_atoms, const int* species_of_atom_h,
                                    const double* positions_h, const double* rho_d, double* out_h) {
    if (!cube_kb || !recip_lattice_h || n_atoms < 0 || n_species < 0 || !rho_d ||
        (n_atoms > 0 && (!species_of_atom_h || !positions_h || !params_h || !out_h)))
        return DFTK_MI_EINVAL;
    CHK(cube_block("dynmat_local", cube_kb));
    CHK(check_species_grouped("dynmat_local", n_species, n_atoms, species_of_atom_h));
    if (n_atoms == 0) return 0;
    dftk_mi_basis* b = cube_kb->basis;
    HIPCHK(hipSetDevice(b->device));
    const int nx = b->nx, ny = b->ny, nz = b->nz;
    const int64_t N = (int64_t)nx * ny * nz;
    CHK(scratch_grow(b, b->dense_ws, 2 * (size_t)N * sizeof(cd)));
    cd* c1 = reinterpret_cast<cd*>(b->dense_ws.get());
    cd* c2 = c1 + N;
    CHK(launch_real_to_cplx(b, N, rho_d, c1));
    CHK(launch_fft_from_cube(cube_kb, c1, c2));          // R(G), unnormalised
    const int n_blocks = (int)std::min<int64_t>((N + 255) / 256, 512);
    double *d_par, *d_pos, *d_part, *d_out;
    int* d_sp;
    WsCarver ws;
    ws.take(&d_par, (size_t)8 * n_species), ws.take(&d_pos, (size_t)3 * n_atoms), ws.take(&d_sp, (size_t)n_atoms);
    ws.take(&d_part, (size_t)6 * n_atoms * n_blocks), ws.take(&d_out, (size_t)6 * n_atoms);
    CHK(ensure_ws(b, ws.bytes()));
    ws.bind(b->ws);
    HIPCHK(hipMemcpyAsync(d_par, params_h, (size_t)8 * n_species * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_pos, positions_h, (size_t)3 * n_atoms * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_sp, species_of_atom_h, (size_t)n_atoms * sizeof(int), hipMemcpyHostToDevice, b->stream));
    hipLaunchKernelGGL(k_dynmat_local, dim3((unsigned)n_blocks, (unsigned)n_atoms), dim3(256), 0, b->stream, nx, ny, nz,
                       make_mat3(recip_lattice_h), (const double*)d_par, (const int*)d_sp, (const double*)d_pos,
                       (const cd*)c2, 1.0 / (double)N, d_part);
    HIPCHK(hipGetLastError());
    CHK(launch_rowsum(b, 6 * n_atoms, n_blocks, d_part, -4.0 * M_PI * M_PI, d_out));
    std::vector<double> h((size_t)6 * n_atoms);
    HIPCHK(hipMemcpyAsync(h.data(), d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    const int pair[3][3] = {{0, 3, 4}, {3, 1, 5}, {4, 5, 2}};
    for (int a = 0; a < n_atoms; ++a)
        for (int be = 0; be < 3; ++be)
            for (int al = 0; al < 3; ++al) out_h[9 * a + 3 * be + al] = h[6 * (size_t)a + pair[be][al]];
    return 0;
}

// ------------------------------------------------------------------------------------------------ nonlocal term
// Z[:, p nb + n] = g_alpha g_beta psi[:, n], p = xx, yy, zz, xy, xz, yz
__global__ __launch_bounds__(256) void k_nl_operands_second(int64_t rows, int nb, const int* __restrict__ G3, double kx,
                                                            double ky, double kz, const cd* __restrict__ psi, int64_t ldpsi,
                                                            cd* __restrict__ Z, int64_t ldz) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (i >= rows) return;
    const int* g = G3 + 3 * i;
    const double gx = g[0] + kx, gy = g[1] + ky, gz = g[2] + kz;
    const double f[6] = {gx * gx, gy * gy, gz * gz, gx * gy, gx * gz, gy * gz};
    const cd x = psi[i + (int64_t)n * ldpsi];
#pragma unroll
    for (int p = 0; p < 6; ++p) Z[i + (int64_t)(p * nb + n) * ldz] = make_double2(f[p] * x.x, f[p] * x.y);
}

// flag[0] = 1 when D couples the columns [c0, c1) of an atom to columns outside it (one workgroup per atom)
__global__ __launch_bounds__(256) void k_d_coupling(int n_p, const double* __restrict__ D, int bw,
                                                    const int* __restrict__ col_start, double* __restrict__ flag) {
    const int c0 = col_start[blockIdx.x], c1 = col_start[blockIdx.x + 1];
    const int width = 2 * bw + 1;
    for (int t = threadIdx.x; t < (c1 - c0) * width; t += 256) {
        const int i = c0 + t / width, j = i - bw + t % width;
        if (j < 0 || j >= n_p || (j >= c0 && j < c1)) continue;
        if (D[i + (int64_t)j * n_p] != 0.0) flag[0] = 1.0;     // (benign race: every writer stores the same value)
    }
}

// Y = D_s Q for the na x ncols block Q of one atom (D_s = D[c0 .. c0 + na, c0 .. c0 + na])
__global__ __launch_bounds__(256) void k_apply_D_atom(int na, int64_t ncols, const double* __restrict__ D, int n_p, int c0,
                                                      const cd* __restrict__ Q, cd* __restrict__ Y) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)na * ncols) return;
    const int i = (int)(t % na);
    const int64_t col = t / na;
    double re = 0.0, im = 0.0;
    for (int j = 0; j < na; ++j) {
        const double d = D[(c0 + i) + (int64_t)(c0 + j) * n_p];
        const cd q = Q[j + col * na];
        re += d * q.x;
        im += d * q.y;
    }
    Y[t] = make_double2(re, im);
}

// out_alpha[i, n] = -2 pi i g_alpha(i) T[i, n] + 2 pi T[i, (1 + alpha) nb + n]; out_alpha starts at out + alpha out_stride
__global__ __launch_bounds__(256) void k_displacement_combine(int64_t rows, int nb, const int* __restrict__ G3, double kx,
                                                              double ky, double kz, const cd* __restrict__ T, int64_t ldt,
                                                              cd* __restrict__ out, int64_t ldout, int64_t out_stride) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (i >= rows) return;
    const int* g = G3 + 3 * i;
    const double gv[3] = {g[0] + kx, g[1] + ky, g[2] + kz};
    const cd t0 = T[i + (int64_t)n * ldt];
#pragma unroll
    for (int al = 0; al < 3; ++al) {
        const cd ta = T[i + (int64_t)((1 + al) * nb + n) * ldt];
        const double s = 2.0 * M_PI * gv[al];
        out[i + (int64_t)n * ldout + al * out_stride] = make_double2(s * t0.y + 2.0 * M_PI * ta.x, -s * t0.x + 2.0 * M_PI * ta.y);
    }
}

// acc[9 a + 0..2] += sum_n { dw_n Re[p' D q_alpha] + w_n Re[dp' D q_alpha + p' D dq_alpha] }      (dQ non-null)
// acc[9 a + 3..8] += sum_n w_n Re[ Q_alpha' D Q_beta - Q2_alphabeta' D p ], alphabeta = xx, yy, zz, xy, xz, yz   (Q2 non-null)
// Q = [p | q_x | q_y | q_z], dQ the same of dpsi (n_p x 4 nb), Q2 = P' [g_alpha g_beta psi] (n_p x 6 nb); one workgroup per
// atom (fixed reduction order).  acc[9 n_atoms] is set non-zero when D couples atom a's columns to columns outside it.
__global__ __launch_bounds__(256) void k_dynmat_nl_contract(int n_p, int nb, const cd* __restrict__ Q, const cd* __restrict__ dQ,
                                                            const cd* __restrict__ Q2, const double* __restrict__ D, int bw,
                                                            const int* __restrict__ col_start, const double* __restrict__ w,
                                                            const double* __restrict__ dw, int n_atoms,
                                                            double* __restrict__ acc) {
    __shared__ double sh[4];
    const int a = blockIdx.x;
    const int c0 = col_start[a], c1 = col_start[a + 1], na = c1 - c0;
    double f[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool bad = false;
    const int pa[6] = {0, 1, 2, 0, 0, 1}, pb[6] = {0, 1, 2, 1, 2, 2};
    const int64_t items = (int64_t)na * nb;
    for (int64_t t = threadIdx.x; t < items; t += 256) {
        const int n = (int)(t / na), i = c0 + (int)(t % na);
        const int64_t col = (int64_t)n * n_p;
        const cd p_i = Q[i + col];
        for (int j = i - bw; j <= i + bw; ++j) {
            if (j < 0 || j >= n_p) continue;
            const double d = D[i + (int64_t)j * n_p];
            if (d == 0.0) continue;
            if (j < c0 || j >= c1) {
                bad = true;
                continue;
            }
            if (dQ) {
                const cd dp_i = dQ[i + col];
#pragma unroll
                for (int al = 0; al < 3; ++al) {
                    const int64_t ca = (int64_t)((1 + al) * nb + n) * n_p;
                    const cd q = Q[j + ca], dq = dQ[j + ca];
                    const double pq = p_i.x * q.x + p_i.y * q.y;      // Re(conj(p) q)
                    f[al] += d * (dw[n] * pq + w[n] * (dp_i.x * q.x + dp_i.y * q.y + p_i.x * dq.x + p_i.y * dq.y));
                }
            }
            if (Q2) {
                const cd p_j = Q[j + col];
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    const cd qa = Q[i + (int64_t)((1 + pa[c]) * nb + n) * n_p], qb = Q[j + (int64_t)((1 + pb[c]) * nb + n) * n_p];
                    const cd q2 = Q2[i + (int64_t)(c * nb + n) * n_p];
                    f[3 + c] += w[n] * d * (qa.x * qb.x + qa.y * qb.y - q2.x * p_j.x - q2.y * p_j.y);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        const double t = block_sum<256>(f[c], sh);
        if (threadIdx.x == 0) acc[9 * a + c] += t;
    }
    if (bad) acc[9 * n_atoms] = 1.0;     // (benign race: every writer stores the same value)
}

// what entries 3 and 4 refuse alike; n = rows every block must have
static int check_nl_block(const char* who, const dftk_mi_kblock* kb, const double* kcoord_h, int n_atoms,
                          const int* col_start_h) {
    if (kb->sh_comm) {
        dftk_set_error("%s: plane-wave sharded k-blocks are not supported", who);
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("%s: not available inside a batched multi-k call", who);
        return DFTK_MI_EINVAL;
    }
    if (!kcoord_h || !col_start_h || n_atoms < 0) return DFTK_MI_EINVAL;
    if (col_start_h[0] != 0 || col_start_h[n_atoms] != kb->n_p) {
        dftk_set_error("%s: col_start must run from 0 to n_p (%d) over n_atoms + 1 entries", who, kb->n_p);
        return DFTK_MI_EINVAL;
    }
    for (int a = 0; a < n_atoms; ++a)
        if (col_start_h[a + 1] < col_start_h[a]) return DFTK_MI_EINVAL;
    if (kb->n_p > 0 && (!kb->P || !kb->d_D)) {
        dftk_set_error("%s: the block has no projectors bound", who);
        return DFTK_MI_EINVAL;
    }
    return 0;
}

extern "C" int dftk_mi_nonlocal_displacement_apply(dftk_mi_kblock* kb, const double* kcoord_h, int atom, int n_atoms,
                                                   const int* col_start_h, int n_bands, const dftk_mi_cplx* psi_d,
                                                   int64_t ld_psi, dftk_mi_cplx* out_d, int64_t ld_out) {
    if (!kb || n_bands < 0) return DFTK_MI_EINVAL;
    CHK(check_nl_block("nonlocal_displacement_apply", kb, kcoord_h, n_atoms, col_start_h));
    if (atom < 0 || atom >= n_atoms) return DFTK_MI_EINVAL;
    if (n_bands == 0) return 0;
    const int64_t rows = kb->n_G;
    if (!psi_d || !out_d || ld_psi < rows || ld_out < rows) {
        dftk_set_error("nonlocal_displacement_apply: null block or leading dimension below n_G = %lld", (long long)rows);
        return DFTK_MI_EINVAL;
    }
    dftk_mi_basis* b = kb->basis;
    HIPCHK(hipSetDevice(b->device));
    const cd* psi = reinterpret_cast<const cd*>(psi_d);
    cd* out = reinterpret_cast<cd*>(out_d);
    const int nb = n_bands, n_p = kb->n_p;
    const int c0 = col_start_h[atom], na = col_start_h[atom + 1] - c0;
    CHK(ensure_G3(kb));
    // band chunk: operands and back-product (rows x 4 cb each), projections and D times them (na x 4 cb each), in the basis
    // scratch T1 (free outside the FFT pipeline)
    const size_t per_band = 8 * (size_t)(rows + na) * sizeof(cd);
    const size_t budget = std::max(b->T1.bytes(), (size_t)64 << 20);
    const int cb = (int)std::max<size_t>(1, std::min<size_t>((size_t)nb, budget / per_band));
    cd *Z, *T, *Q, *Y;
    double* d_flag;
    int* d_cs;
    WsCarver ws;
    ws.take(&Z, (size_t)rows * 4 * cb), ws.take(&T, (size_t)rows * 4 * cb), ws.take(&Q, (size_t)na * 4 * cb);
    ws.take(&Y, (size_t)na * 4 * cb), ws.take(&d_flag, (size_t)1), ws.take(&d_cs, (size_t)2);
    CHK(scratch_grow(b, b->T1, ws.bytes()));
    ws.bind(b->T1);
    if (na > 0) {
        // refuse a D that couples this atom to another BEFORE anything is written to out
        double flag = 0.0;
        HIPCHK(hipMemcpyAsync(d_cs, col_start_h + atom, 2 * sizeof(int), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemsetAsync(d_flag, 0, sizeof(double), b->stream));
        hipLaunchKernelGGL(k_d_coupling, dim3(1), dim3(256), 0, b->stream, n_p, (const double*)kb->d_D, kb->D_bw,
                           (const int*)d_cs, d_flag);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&flag, d_flag, sizeof(double), hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        if (flag != 0.0) {
            dftk_set_error("nonlocal_displacement_apply: D couples the projector columns of different atoms");
            return DFTK_MI_EINVAL;
        }
    }
    const int64_t out_stride = (int64_t)nb * ld_out;
    const cd one = {1.0, 0.0}, zero = {0.0, 0.0};
    const cd* Ps = kb->P + (int64_t)c0 * kb->ldP;
    for (int n0 = 0; n0 < nb; n0 += cb) {
        const int m = std::min(cb, nb - n0);
        cd* o = out + (int64_t)n0 * ld_out;
        if (na == 0) {       // an atom without projectors: the perturbation is zero
            for (int al = 0; al < 3; ++al)
                HIPCHK(hipMemset2DAsync(o + al * out_stride, (size_t)ld_out * sizeof(cd), 0, (size_t)rows * sizeof(cd), m,
                                        b->stream));
            continue;
        }
        CHK(launch_nl_operands_full(b, rows, m, 0, kb->d_G3, kcoord_h, psi + (int64_t)n0 * ld_psi, ld_psi, Z, rows));
        CHK(zgemm(b, 'C', na, 4 * (int64_t)m, rows, one, Ps, kb->ldP, Z, rows, zero, Q, na));
        hipLaunchKernelGGL(k_apply_D_atom, dim3((unsigned)(((int64_t)na * 4 * m + 255) / 256)), dim3(256), 0, b->stream, na,
                           4 * (int64_t)m, (const double*)kb->d_D, n_p, c0, (const cd*)Q, Y);
        HIPCHK(hipGetLastError());
        CHK(zgemm(b, 'N', rows, 4 * (int64_t)m, na, one, Ps, kb->ldP, Y, na, zero, T, rows));
        hipLaunchKernelGGL(k_displacement_combine, dim3((unsigned)((rows + 255) / 256), (unsigned)m), dim3(256), 0, b->stream,
                           rows, m, (const int*)kb->d_G3, kcoord_h[0], kcoord_h[1], kcoord_h[2], (const cd*)T, rows, o, ld_out,
                           out_stride);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

extern "C" int dftk_mi_dynmat_nonlocal(dftk_mi_kblock* kb, const double* kcoord_h, int n_bands, const dftk_mi_cplx* psi_d,
                                       int64_t ld_psi, const dftk_mi_cplx* dpsi_d, int64_t ld_dpsi, const double* w_h,
                                       const double* wd_h, int n_atoms, const int* col_start_h, double* dforces_h,
                                       double* hess_h) {
    if (!kb || n_bands < 0) return DFTK_MI_EINVAL;
    CHK(check_nl_block("dynmat_nonlocal", kb, kcoord_h, n_atoms, col_start_h));
    const bool want_df = dpsi_d != nullptr, want_h = hess_h != nullptr;
    if (want_df && (!dforces_h || !wd_h)) return DFTK_MI_EINVAL;
    if (n_bands == 0 || kb->n_p == 0 || n_atoms == 0 || (!want_df && !want_h)) return 0;
    const int64_t rows = kb->n_G;
    if (!psi_d || !w_h || ld_psi < rows || (want_df && ld_dpsi < rows)) {
        dftk_set_error("dynmat_nonlocal: null block or leading dimension below n_G = %lld", (long long)rows);
        return DFTK_MI_EINVAL;
    }
    dftk_mi_basis* b = kb->basis;
    HIPCHK(hipSetDevice(b->device));
    const cd* psi = reinterpret_cast<const cd*>(psi_d);
    const cd* dpsi = reinterpret_cast<const cd*>(dpsi_d);
    const int nb = n_bands, n_p = kb->n_p;
    CHK(ensure_G3(kb));
    // band chunk: one operand panel (rows x 6 cb, reused by the three products) and the projections (n_p x 14 cb)
    const size_t per_band = (6 * (size_t)rows + 14 * (size_t)n_p) * sizeof(cd);
    const size_t budget = std::max(b->T1.bytes(), (size_t)64 << 20);
    const int cb = (int)std::max<size_t>(1, std::min<size_t>((size_t)nb, budget / per_band));
    cd *Z, *Q, *dQ, *Q2;
    double *d_w, *d_dw, *d_acc;
    int* d_cs;
    WsCarver ws;
    ws.take(&Z, (size_t)rows * 6 * cb), ws.take(&Q, (size_t)n_p * 4 * cb), ws.take(&dQ, (size_t)n_p * 4 * cb);
    ws.take(&Q2, (size_t)n_p * 6 * cb), ws.take(&d_w, (size_t)nb), ws.take(&d_dw, (size_t)nb);
    ws.take(&d_acc, (size_t)(9 * n_atoms + 1)), ws.take(&d_cs, (size_t)(n_atoms + 1));
    CHK(scratch_grow(b, b->T1, ws.bytes()));
    ws.bind(b->T1);
    HIPCHK(hipMemcpyAsync(d_w, w_h, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, b->stream));
    if (want_df) HIPCHK(hipMemcpyAsync(d_dw, wd_h, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_cs, col_start_h, (size_t)(n_atoms + 1) * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemsetAsync(d_acc, 0, (size_t)(9 * n_atoms + 1) * sizeof(double), b->stream));
    const cd one = {1.0, 0.0}, zero = {0.0, 0.0};
    for (int n0 = 0; n0 < nb; n0 += cb) {
        const int m = std::min(cb, nb - n0);
        const cd* ps = psi + (int64_t)n0 * ld_psi;
        CHK(launch_nl_operands_full(b, rows, m, 0, kb->d_G3, kcoord_h, ps, ld_psi, Z, rows));
        CHK(zgemm(b, 'C', n_p, 4 * (int64_t)m, rows, one, kb->P, kb->ldP, Z, rows, zero, Q, n_p));
        if (want_df) {
            CHK(launch_nl_operands_full(b, rows, m, 0, kb->d_G3, kcoord_h, dpsi + (int64_t)n0 * ld_dpsi, ld_dpsi, Z, rows));
            CHK(zgemm(b, 'C', n_p, 4 * (int64_t)m, rows, one, kb->P, kb->ldP, Z, rows, zero, dQ, n_p));
        }
        if (want_h) {
            hipLaunchKernelGGL(k_nl_operands_second, dim3((unsigned)((rows + 255) / 256), (unsigned)m), dim3(256), 0, b->stream,
                               rows, m, (const int*)kb->d_G3, kcoord_h[0], kcoord_h[1], kcoord_h[2], ps, ld_psi, Z, rows);
            HIPCHK(hipGetLastError());
            CHK(zgemm(b, 'C', n_p, 6 * (int64_t)m, rows, one, kb->P, kb->ldP, Z, rows, zero, Q2, n_p));
        }
        hipLaunchKernelGGL(k_dynmat_nl_contract, dim3((unsigned)n_atoms), dim3(256), 0, b->stream, n_p, m, (const cd*)Q,
                           want_df ? (const cd*)dQ : (const cd*)nullptr, want_h ? (const cd*)Q2 : (const cd*)nullptr,
                           (const double*)kb->d_D, kb->D_bw, (const int*)d_cs, (const double*)(d_w + n0),
                           (const double*)(d_dw + n0), n_atoms, d_acc);
        HIPCHK(hipGetLastError());
    }
    std::vector<double> acc((size_t)9 * n_atoms + 1);
    HIPCHK(hipMemcpyAsync(acc.data(), d_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (acc[9 * (size_t)n_atoms] != 0.0) {
        dftk_set_error("dynmat_nonlocal: D couples the projector columns of different atoms");
        return DFTK_MI_EINVAL;
    }
    const int pair[3][3] = {{0, 3, 4}, {3, 1, 5}, {4, 5, 2}};
    for (int a = 0; a < n_atoms; ++a) {
        if (want_df)
            for (int al = 0; al < 3; ++al) dforces_h[3 * a + al] += -4.0 * M_PI * acc[9 * (size_t)a + al];
        if (want_h)
            for (int be = 0; be < 3; ++be)
                for (int al = 0; al < 3; ++al)
                    hess_h[9 * a + 3 * be + al] += 8.0 * M_PI * M_PI * acc[9 * (size_t)a + 3 + pair[be][al]];
    }
    return 0;
}
