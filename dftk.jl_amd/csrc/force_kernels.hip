// force_kernels.hip -- atomic forces of the HGH local and nonlocal terms (gfx950 only).
//
// compute_forces(::TermAtomicLocal) (src/terms/local.jl:142-177): with W_s(G) = ff_s(|G|) conj(R(G)) / N, R the
// unnormalised forward DFT of the total density, the local energy of this library is E = sum_G c(G) conj(rho(G)),
// c = sum_a ff_s e^{-2 pi i G.r_a} / sqrt(Omega) (the cube atomic_superposition kind 0 builds), so
//     F_{a,alpha} = -2 pi sum_G G_alpha Im( W_s(G) e^{-2 pi i G.r_a} )      (reduced coordinates)
// summed over the whole cube, unpaired Nyquist entries zeroed exactly as k_atomic_sum does.  The phase is separable,
// e^{-2 pi i G.r} = t_x[gx] t_y[gy] t_z[gz] (1-D tables built once per atom on the host); W_s is built once per
// species on the cube, and a thread of the force kernel keeps W of
// FL_KY x FL_KZ points of one x-column in registers and, per atom, pays one complex multiply per point; the
// y / z weighting and the x phase are applied to the partial sums.  Wave sums are written per (atom, component) and
// reduced in a second pass in a fixed order: no atomics, bitwise reproducible.
//
// compute_forces(::TermAtomicNonlocal) (src/terms/nonlocal.jl:49-98): with p = P' psi and q_alpha = P' (i g_alpha psi)
// (g = G + k reduced), dP_alpha' psi = 2 pi q_alpha and
//     F_{a,alpha} = -4 pi sum_n w_n Re[ p_n(a)' D_a q_{alpha,n}(a) ]
// i.e. ONE product P' [psi | i g_x psi | i g_y psi | i g_z psi] per band chunk (the library's zgemm; on a Gamma-real
// block the REAL product over the half-sphere rows with the block's half-format projectors) and a small per-atom
// contraction with the banded D.
#include "common.h"
#include "hgh_forms.h"
#include <algorithm>
#include <cmath>
#include <vector>

// ------------------------------------------------------------------------------------------------ local term
#define FL_KY 8         // consecutive y rows per thread
#define FL_KZ 2         // consecutive z planes per thread
#define FL_WAVES 4      // waves per workgroup, stacked along y

// xor butterfly: the sum arrives in every lane (common.h's wave_sum is the shuffle-down tree, lane 0 only)
__device__ inline double wave_sum_all(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// W_s(G) = ff_s(|G|) conj(R(G)) / N on the whole cube (one species), unpaired Nyquist entries zero.  TABLE = true: q is
// the species' row of a device table of form factors per cube point (dftk_mi_forces_local_table), not its 8 parameters
template <bool TABLE>
__global__ __launch_bounds__(256) void k_forces_local_w(int nx, int ny, int nz, Mat3 B, const double* __restrict__ q,
                                                        const cd* __restrict__ R, double inv_N, cd* __restrict__ W) {
    const int64_t N = (int64_t)nx * ny * nz;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N) return;
    const int ix = (int)(idx % nx), iy = (int)((idx / nx) % ny), iz = (int)(idx / ((int64_t)nx * ny));
    if (unpaired_nyquist(ix, iy, iz, nx, ny, nz)) {
        W[idx] = make_double2(0.0, 0.0);
        return;
    }
    double qx, qy, qz;
    recip_times(B, (double)signed_freq(ix, nx), (double)signed_freq(iy, ny), (double)signed_freq(iz, nz), &qx, &qy, &qz);
    const double p = sqrt(qx * qx + qy * qy + qz * qz);
    const double ff = (TABLE ? q[idx] : hgh_local_ff(q, (p * q[0]) * (p * q[0]))) * inv_N;
    const cd r = R[idx];
    W[idx] = make_double2(ff * r.x, -ff * r.y);
}

// atoms [a0, a1) of one species against its W.  grid: (ceil(nx / 64), ceil(ny / (FL_WAVES FL_KY)), ceil(nz / FL_KZ));
// partial[(3 a + alpha) * n_waves + wave id]
__global__ __launch_bounds__(64 * FL_WAVES, 4) void k_forces_local(int nx, int ny, int nz, int a0, int a1,
                                                                const cd* __restrict__ W, const cd* __restrict__ tab,
                                                                double* __restrict__ partial, int64_t n_waves) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ix = blockIdx.x * 64 + lane;
    // (y / z indices are wave-uniform: the phase-table reads become scalar loads)
    const int iy0 = __builtin_amdgcn_readfirstlane((blockIdx.y * FL_WAVES + wave) * FL_KY);
    const int iz0 = blockIdx.z * FL_KZ;
    const int64_t wid = ((int64_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * FL_WAVES + wave;
    const int ixc = ix < nx ? ix : nx - 1;
    const double gx = (double)signed_freq(ixc, nx);
    const int64_t tstride = (int64_t)nx + ny + nz;
    cd w[FL_KZ][FL_KY];
#pragma unroll
    for (int kz = 0; kz < FL_KZ; ++kz)
#pragma unroll
        for (int ky = 0; ky < FL_KY; ++ky) {
            const int iy = iy0 + ky, iz = iz0 + kz;
            w[kz][ky] = (ix < nx && iy < ny && iz < nz) ? W[ix + (int64_t)nx * (iy + (int64_t)ny * iz)]
                                                        : make_double2(0.0, 0.0);
        }
#pragma unroll 1
    for (int a = a0; a < a1; ++a) {
        const cd* tx = tab + a * tstride;
        const cd* ty = tx + nx;
        const cd* tz = ty + ny;
        double S0r = 0.0, S0i = 0.0, Syr = 0.0, Syi = 0.0, Szr = 0.0, Szi = 0.0;
#pragma unroll
        for (int kz = 0; kz < FL_KZ; ++kz) {
            const int iz = iz0 + kz;
            double s0r = 0.0, s0i = 0.0, syr = 0.0, syi = 0.0;
#pragma unroll
            for (int ky = 0; ky < FL_KY; ++ky) {
                const int iy = iy0 + ky;
                const cd t = ty[iy < ny ? iy : ny - 1];
                const cd v = w[kz][ky];
                const double ur = v.x * t.x - v.y * t.y, ui = v.x * t.y + v.y * t.x;
                const double gy = (double)signed_freq(iy < ny ? iy : ny - 1, ny);
                s0r += ur;
                s0i += ui;
                syr += gy * ur;
                syi += gy * ui;
            }
            const cd t = tz[iz < nz ? iz : nz - 1];
            const double gz = (double)signed_freq(iz < nz ? iz : nz - 1, nz);
            const double ar = s0r * t.x - s0i * t.y, ai = s0r * t.y + s0i * t.x;
            S0r += ar;
            S0i += ai;
            Szr += gz * ar;
            Szi += gz * ai;
            Syr += syr * t.x - syi * t.y;
            Syi += syr * t.y + syi * t.x;
        }
        const cd t = tx[ixc];
        const double fx = gx * (S0r * t.y + S0i * t.x);      // Im(t S)
        const double fy = Syr * t.y + Syi * t.x;
        const double fz = Szr * t.y + Szi * t.x;
        const double sx = wave_sum_all(fx), sy = wave_sum_all(fy), sz = wave_sum_all(fz);
        if (lane == 0) {
            partial[(int64_t)(3 * a + 0) * n_waves + wid] = sx;
            partial[(int64_t)(3 * a + 1) * n_waves + wid] = sy;
            partial[(int64_t)(3 * a + 2) * n_waves + wid] = sz;
        }
    }
}

// out[r] = scale * sum_i in[r * n + i], one workgroup per row, fixed reduction order
__global__ __launch_bounds__(256) void k_rowsum(int64_t n, const double* __restrict__ in, double scale,
                                                double* __restrict__ out) {
    const double* x = in + (int64_t)blockIdx.x * n;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += x[i];
    block_reduce<1>(&s);
    if (threadIdx.x == 0) out[blockIdx.x] = scale * s;
}
int launch_rowsum(dftk_mi_basis* b, int rows, int64_t n, const double* in, double scale, double* out) {
    hipLaunchKernelGGL(k_rowsum, dim3((unsigned)rows), dim3(256), 0, b->stream, n, in, scale, out);
    HIPCHK(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void k_real_to_cplx(int64_t n, const double* __restrict__ x, cd* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = make_double2(x[i], 0.0);
}
int launch_real_to_cplx(dftk_mi_basis* b, int64_t n, const double* x, cd* y) {
    hipLaunchKernelGGL(k_real_to_cplx, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, n, x, y);
    HIPCHK(hipGetLastError());
    return 0;
}

// par_h: 8 HGH parameters per species (host), or, with ff_d given, unused: form factors from the device table ff_d[s][N]
static int forces_local_impl(dftk_mi_kblock* cube_kb, const double* recip_h, int n_species, const double* par_h,
                             const double* ff_d, int n_atoms, const int* species_of_atom_h, const double* positions_h,
                             const double* rho_d, double* forces_h) {
    dftk_mi_basis* b = cube_kb->basis;
    const int nx = b->nx, ny = b->ny, nz = b->nz;
    const int64_t N = (int64_t)nx * ny * nz;
    if (cube_kb->n_G != N) {
        dftk_set_error("forces_local: the k-block must span the whole cube");
        return DFTK_MI_EINVAL;
    }
    if (n_atoms < 0 || n_species < 0 || (n_atoms > 0 && (!species_of_atom_h || !positions_h || (!par_h && !ff_d))) || !rho_d ||
        (n_atoms > 0 && !forces_h))
        return DFTK_MI_EINVAL;
    CHK(check_species_grouped("forces_local", n_species, n_atoms, species_of_atom_h));
    if (n_atoms == 0) return 0;
    // R(G): forward cube DFT of the total density (unnormalised), in the dense workspace as atomic_superposition uses it
    CHK(scratch_grow(b, b->dense_ws, 2 * (size_t)N * sizeof(cd)));
    cd* c1 = reinterpret_cast<cd*>(b->dense_ws.get());
    cd* c2 = c1 + N;
    CHK(launch_real_to_cplx(b, N, rho_d, c1));
    CHK(launch_fft_from_cube(cube_kb, c1, c2));          // (c1 is overwritten by the transform)
    const std::vector<cd> tab = phase_tables_host(nx, ny, nz, n_atoms, positions_h);
    const dim3 grid((unsigned)((nx + 63) / 64), (unsigned)((ny + FL_WAVES * FL_KY - 1) / (FL_WAVES * FL_KY)),
                    (unsigned)((nz + FL_KZ - 1) / FL_KZ));
    const int64_t n_waves = (int64_t)grid.x * grid.y * grid.z * FL_WAVES;
    // workspace: tables, per-wave partial sums, result (W_s goes into c1, free again after the transform)
    const size_t b_out = (size_t)3 * n_atoms * sizeof(double), b_par = (size_t)n_species * 8 * sizeof(double);
    cd* d_tab;
    double *d_part, *d_out, *d_par;
    WsCarver ws;
    ws.take(&d_tab, tab.size()), ws.take(&d_part, (size_t)3 * n_atoms * n_waves);
    ws.take(&d_out, (size_t)3 * n_atoms), ws.take(&d_par, (size_t)n_species * 8);
    CHK(ensure_ws(b, ws.bytes()));
    ws.bind(b->ws);
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(cd), hipMemcpyHostToDevice, b->stream));
    if (!ff_d) HIPCHK(hipMemcpyAsync(d_par, par_h, b_par, hipMemcpyHostToDevice, b->stream));
    const Mat3 B = make_mat3(recip_h);
    for (int a0 = 0; a0 < n_atoms;) {
        int a1 = a0 + 1;
        while (a1 < n_atoms && species_of_atom_h[a1] == species_of_atom_h[a0]) ++a1;
        if (ff_d) {
            hipLaunchKernelGGL(k_forces_local_w<true>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, b->stream, nx, ny,
                               nz, B, ff_d + (int64_t)species_of_atom_h[a0] * N, (const cd*)c2, 1.0 / (double)N, c1);
        } else {
            hipLaunchKernelGGL(k_forces_local_w<false>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, b->stream, nx,
                               ny, nz, B, (const double*)(d_par + 8 * species_of_atom_h[a0]), (const cd*)c2,
                               1.0 / (double)N, c1);
        }
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_forces_local, grid, dim3(64 * FL_WAVES), 0, b->stream, nx, ny, nz, a0, a1, (const cd*)c1,
                           (const cd*)d_tab, d_part, n_waves);
        HIPCHK(hipGetLastError());
        a0 = a1;
    }
    CHK(launch_rowsum(b, 3 * n_atoms, n_waves, d_part, -2.0 * M_PI, d_out));
    HIPCHK(hipMemcpyAsync(forces_h, d_out, b_out, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));     // (host tables and b->ws are free again)
    return 0;
}

int forces_local(dftk_mi_kblock* cube_kb, const double* recip_h, int n_species, const double* par_h, int n_atoms,
                 const int* species_of_atom_h, const double* positions_h, const double* rho_d, double* forces_h) {
    return forces_local_impl(cube_kb, recip_h, n_species, par_h, nullptr, n_atoms, species_of_atom_h, positions_h, rho_d,
                             forces_h);
}
int forces_local_table(dftk_mi_kblock* cube_kb, const double* recip_h, int n_species, const double* ff_d, int n_atoms,
                       const int* species_of_atom_h, const double* positions_h, const double* rho_d, double* forces_h) {
    return forces_local_impl(cube_kb, recip_h, n_species, nullptr, ff_d, n_atoms, species_of_atom_h, positions_h, rho_d,
                             forces_h);
}

// ------------------------------------------------------------------------------------------------ nonlocal term
// full-sphere operands: Z[:, n] = psi[:, n], Z[:, (1 + alpha) nb + n] = i g_alpha psi[:, n], g = G + k (reduced) of
// sphere row row0 + i
__global__ __launch_bounds__(256) void k_nl_operands_full(int64_t rows, int nb, int64_t row0, const int* __restrict__ G3,
                                                          double kx, double ky, double kz, const cd* __restrict__ psi,
                                                          int64_t ldpsi, cd* __restrict__ Z, int64_t ldz) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (i >= rows) return;
    const int* g = G3 + 3 * (row0 + i);
    const double gv[3] = {g[0] + kx, g[1] + ky, g[2] + kz};
    const cd x = psi[i + (int64_t)n * ldpsi];
    Z[i + (int64_t)n * ldz] = x;
#pragma unroll
    for (int al = 0; al < 3; ++al)
        Z[i + (int64_t)((1 + al) * nb + n) * ldz] = make_double2(-gv[al] * x.y, gv[al] * x.x);
}

int launch_nl_operands_full(dftk_mi_basis* b, int64_t rows, int nb, int64_t row0, const int* G3, const double* kcoord_h,
                            const cd* psi, int64_t ldpsi, cd* Z, int64_t ldz) {
    hipLaunchKernelGGL(k_nl_operands_full, dim3((unsigned)((rows + 255) / 256), (unsigned)nb), dim3(256), 0, b->stream, rows,
                       nb, row0, G3, kcoord_h[0], kcoord_h[1], kcoord_h[2], psi, ldpsi, Z, ldz);
    HIPCHK(hipGetLastError());
    return 0;
}

// half-format operands from the half-format block in Z[:, 0 .. nb): row j holds i G_alpha(G_j) psi_h(j), G_j = the
// representative of global pair row0 + j (row 0 is G = 0: zero)
__global__ __launch_bounds__(256) void k_nl_operands_half(int64_t rows, int nb, int64_t row0, const int* __restrict__ G3,
                                                          const int* __restrict__ gidx, cd* __restrict__ Z, int64_t ldz) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (j >= rows) return;
    const int* g = G3 + 3 * (int64_t)gidx[row0 + j];
    const cd x = Z[j + (int64_t)n * ldz];
#pragma unroll
    for (int al = 0; al < 3; ++al) {
        const double ga = (double)g[al];
        Z[j + (int64_t)((1 + al) * nb + n) * ldz] = make_double2(-ga * x.y, ga * x.x);
    }
}

// acc[3 a + alpha] += sum_n w_n Re[ p_n(a)' D_a q_{alpha,n}(a) ]; Q = [p | q_x | q_y | q_z] (n_p x 4 nb, ld n_p);
// one workgroup per atom (fixed reduction order).  acc[3 n_atoms] is set non-zero when D couples atom a's columns to
// columns outside the atom.
__global__ __launch_bounds__(256) void k_nl_contract(int n_p, int nb, const cd* __restrict__ Q, const double* __restrict__ D,
                                                     int bw, const int* __restrict__ col_start, const double* __restrict__ w,
                                                     int n_atoms, double* __restrict__ acc) {
    const int a = blockIdx.x;
    const int c0 = col_start[a], c1 = col_start[a + 1], na = c1 - c0;
    double f[3] = {0.0, 0.0, 0.0};
    bool bad = false;
    const int64_t items = (int64_t)na * nb;
    for (int64_t t = threadIdx.x; t < items; t += 256) {
        const int n = (int)(t / na), i = c0 + (int)(t % na);
        const cd p = Q[i + (int64_t)n * n_p];
        const int jlo = i - bw, jhi = i + bw;
        for (int j = jlo; j <= jhi; ++j) {
            if (j < 0 || j >= n_p) continue;
            const double d = D[i + (int64_t)j * n_p];
            if (d == 0.0) continue;
            if (j < c0 || j >= c1) {
                bad = true;
                continue;
            }
#pragma unroll
            for (int al = 0; al < 3; ++al) {
                const cd q = Q[j + (int64_t)((1 + al) * nb + n) * n_p];
                f[al] += w[n] * d * (p.x * q.x + p.y * q.y);     // Re(conj(p) d q)
            }
        }
    }
    block_reduce<3>(f);
    if (threadIdx.x == 0)
#pragma unroll
        for (int al = 0; al < 3; ++al) acc[3 * a + al] += f[al];
    if (bad) acc[3 * n_atoms] = 1.0;     // (benign race: every writer stores the same value)
}

// integer G of every sphere row (3 per row), built from the block's host mapping on first use
int ensure_G3(dftk_mi_kblock* kb) {
    if (kb->d_G3) return 0;
    dftk_mi_basis* b = kb->basis;
    if (kb->h_mapping.empty()) return DFTK_MI_EINVAL;
    const int nx = b->nx, ny = b->ny, nz = b->nz;
    std::vector<int> G((size_t)3 * kb->n_G);
    for (int64_t c = 0; c < kb->n_G; ++c) {
        const int64_t lin = kb->h_mapping[c];
        const int ix = (int)(lin % nx), iy = (int)((lin / nx) % ny), iz = (int)(lin / ((int64_t)nx * ny));
        G[3 * c + 0] = signed_freq(ix, nx);
        G[3 * c + 1] = signed_freq(iy, ny);
        G[3 * c + 2] = signed_freq(iz, nz);
    }
    HIPCHK(kb->d_G3.alloc(G.size() * sizeof(int)));
    HIPCHK(hipMemcpy(kb->d_G3, G.data(), G.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

int forces_nonlocal(dftk_mi_kblock* kb, const double* kcoord_h, int nb, const cd* psi, int64_t ld_psi,
                    const double* weight_h, int n_atoms, const int* col_start_h, double* forces_h) {
    dftk_mi_basis* b = kb->basis;
    if (nb < 0 || n_atoms < 0 || !col_start_h || (n_atoms > 0 && !forces_h) || !kcoord_h) return DFTK_MI_EINVAL;
    if (col_start_h[0] != 0 || col_start_h[n_atoms] != kb->n_p) {
        dftk_set_error("forces_nonlocal: col_start must run from 0 to n_p (%d) over n_atoms + 1 entries", kb->n_p);
        return DFTK_MI_EINVAL;
    }
    for (int a = 0; a < n_atoms; ++a)
        if (col_start_h[a + 1] < col_start_h[a]) return DFTK_MI_EINVAL;
    if (nb == 0 || kb->n_p == 0) return 0;
    if (!psi || !weight_h) return DFTK_MI_EINVAL;
    const bool sharded = kb->sh_comm != nullptr;
    const int64_t full_rows = sharded ? kb->sh_rows[comm_rank(kb->sh_comm) + 1] - kb->sh_rows[comm_rank(kb->sh_comm)]
                                      : kb->n_G;
    const int64_t full_row0 = sharded ? kb->sh_rows[comm_rank(kb->sh_comm)] : 0;
    if (ld_psi < full_rows) return DFTK_MI_EINVAL;
    const bool gamma = kb->gr && kb->gr->on;
    if (gamma && (kcoord_h[0] != 0.0 || kcoord_h[1] != 0.0 || kcoord_h[2] != 0.0)) return DFTK_MI_EINVAL;
    CHK(ensure_G3(kb));
    const cd* P = kb->P;
    int64_t ldP = kb->ldP, rows = full_rows, row0 = full_row0;
    if (gamma) {
        CHK(gamma_projectors(kb));
        rows = gamma_local_rows(kb);
        row0 = gamma_row0(kb);
        P = kb->gr->P_half;
        ldP = rows;
    }
    const int n_p = kb->n_p;
    // band chunk: panel (rows x 4 cb) + products (n_p x 4 cb) in the basis scratch T1 (free outside the FFT pipeline)
    const size_t per_band = 4 * (size_t)(rows + n_p) * sizeof(cd);
    const size_t budget = std::max(b->T1.bytes(), (size_t)512 << 20);
    const int cb = (int)std::max<size_t>(1, std::min<size_t>((size_t)nb, budget / per_band));
    cd *Z, *Q;
    double *d_w, *d_acc;
    int* d_cs;
    WsCarver ws;
    ws.take(&Z, (size_t)rows * 4 * cb), ws.take(&Q, (size_t)n_p * 4 * cb), ws.take(&d_w, (size_t)nb);
    ws.take(&d_acc, (size_t)(3 * n_atoms + 1)), ws.take(&d_cs, (size_t)(n_atoms + 1));
    CHK(scratch_grow(b, b->T1, ws.bytes()));
    ws.bind(b->T1);
    HIPCHK(hipMemcpyAsync(d_w, weight_h, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_cs, col_start_h, (size_t)(n_atoms + 1) * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemsetAsync(d_acc, 0, (size_t)(3 * n_atoms + 1) * sizeof(double), b->stream));
    const cd one = {1.0, 0.0}, zero = {0.0, 0.0};
    for (int n0 = 0; n0 < nb; n0 += cb) {
        const int m = std::min(cb, nb - n0);
        const cd* ps = psi + (int64_t)n0 * ld_psi;
        if (gamma) {
            // (every column is a real-symmetric field up to a global phase: the aligned compression)
            CHK(gamma_lobpcg_load(kb, m, ps, ld_psi, Z, rows, true));
            hipLaunchKernelGGL(k_nl_operands_half, dim3((unsigned)((rows + 255) / 256), (unsigned)m), dim3(256), 0,
                               b->stream, rows, m, row0, (const int*)kb->d_G3, (const int*)kb->gr->d_g, Z, rows);
        } else {
            CHK(launch_nl_operands_full(b, rows, m, row0, kb->d_G3, kcoord_h, ps, ld_psi, Z, rows));
        }
        HIPCHK(hipGetLastError());
        CHK(zgemm(b, 'C', n_p, 4 * (int64_t)m, rows, one, P, ldP, Z, rows, zero, Q, n_p, gamma ? DFTK_MI_GEMM_REAL : 0));
        if (sharded) CHK(comm_allreduce(kb->sh_comm, b, reinterpret_cast<double*>(Q), 2 * (size_t)n_p * 4 * m));
        hipLaunchKernelGGL(k_nl_contract, dim3((unsigned)n_atoms), dim3(256), 0, b->stream, n_p, m, (const cd*)Q,
                           (const double*)kb->d_D, kb->D_bw, (const int*)d_cs, (const double*)(d_w + n0), n_atoms, d_acc);
        HIPCHK(hipGetLastError());
    }
    std::vector<double> acc((size_t)3 * n_atoms + 1);
    HIPCHK(hipMemcpyAsync(acc.data(), d_acc, acc.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (acc[3 * (size_t)n_atoms] != 0.0) {
        dftk_set_error("forces_nonlocal: D couples the projector columns of different atoms");
        return DFTK_MI_EINVAL;
    }
    for (int i = 0; i < 3 * n_atoms; ++i) forces_h[i] += -4.0 * M_PI * acc[i];
    return 0;
}
