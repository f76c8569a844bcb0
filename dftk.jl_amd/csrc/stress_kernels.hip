// stress_kernels.hip -- the stress tensor at fixed orbital coefficients, term by term (gfx950 only).
//
// compute_stresses_cart (src/postprocess/stresses.jl) differentiates the total energy on the strained lattice
// (I + eps) L with dual numbers, psi (reduced-coordinate coefficients on the same spheres), occupations and eigenvalues
// held fixed.  Here the derivative is written out (Nielsen-Martin): q = B (G + k) -> (I - eps) q, Omega -> Omega (1 + tr eps),
// structure factors do not change.  All results are Omega * sigma_ab, six numbers in the order xx, yy, zz, zy, zx, yx.
//
//   Kinetic         -sum_n w_n sum_G q_a q_b |psi_n(G)|^2                                     (sphere reduction)
//   AtomicNonlocal   sum_n w_n 2 Re[(P' psi_n)' D (dP_ab' psi_n)],
//                    dP_ab = -1/2 delta_ab P - 1/2 (q_a dP/dq_b + q_b dP/dq_a):  with P = R_li(|q|) Y_lm(q) * phase / sqrt(Omega)
//                    (Y the solid harmonic, R the HGH radial form divided by |q|^l, t2 = (|q| r_l)^2)
//                    dP_ab = [-1/2 delta_ab R Y - 2 r_l^2 (dR/dt2) q_a q_b Y - 1/2 R (q_a dY/dq_b + q_b dY/dq_a)] * phase / sqrt(Omega)
//                    The six dP_ab are built on the fly for a chunk of whole atoms, multiplied with the orbitals by the
//                    library's zgemm (Gamma-real block: REAL product over the half-sphere rows -- dP_ab is the transform
//                    of a real function like P) and contracted per atom with the banded D.
//   AtomicLocal     -delta_ab E_loc - sum_G Re[conj(rho(G)) S_s(G) / sqrt(Omega)] ff_s'(|G|) G_a G_b / |G|
//   Hartree         -delta_ab E_H + sum_G 4 pi |rho(G)|^2 G_a G_b / |G|^4     (one cube pass and one FFT with AtomicLocal)
//   Xc               point-wise sums of e, v_rho rho and v_sigma grad_a rho grad_b rho
//
// WORKSPACE BOUND of the nonlocal term (in the basis scratch T1, like the force kernels): the derivative projectors of
// one chunk, 6 x rows x cc complex numbers with cc = the columns of as many whole atoms as fit 512 MiB (at least one
// atom), plus per band chunk cb (as many bands as fit 512 MiB) the panel rows x cb (Gamma-real only), P' psi
// (n_p x cb) and the six products (6 cc x cb) -- never a multiple of the whole P.
// Every reduction has a fixed order (per-workgroup partial sums, then one workgroup per output): no atomics, two calls
// give bitwise identical results.
#include "common.h"
#include "hgh_forms.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#define ST_SQRT2 1.4142135623730951

// thread 0 writes the workgroup's K sums to partial[k * n_blocks + block]
template <int K>
__device__ inline void st_block_reduce(double* v, double* __restrict__ partial, int64_t n_blocks, int64_t block) {
    block_reduce<K>(v);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) partial[(int64_t)k * n_blocks + block] = v[k];
}

// workspace budgets in bytes; DFTK_MI_STRESS_WS_KIB (testing aid, read at every call) replaces both defaults so that a
// small cell runs through several projector-column and band chunks
static size_t st_budget(size_t dflt) {
    const char* e = getenv("DFTK_MI_STRESS_WS_KIB");
    if (!e || !*e) return dflt;
    const long v = atol(e);
    return v > 0 ? (size_t)v << 10 : dflt;
}

// ------------------------------------------------------------------------------------------------ kinetic
// partial[t * n_blocks + block] = sum over the block's rows of q_a q_b sum_n w_n |psi_n(row)|^2
__global__ __launch_bounds__(256) void k_st_kinetic(int64_t rows, int nb, const int* __restrict__ G3, Mat3 B, double kx,
                                                    double ky, double kz, const cd* __restrict__ psi, int64_t ldpsi,
                                                    const double* __restrict__ w, double* __restrict__ partial) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < rows) {
        double s = 0.0;
        for (int n = 0; n < nb; ++n) {
            const cd x = psi[i + (int64_t)n * ldpsi];
            s += w[n] * (x.x * x.x + x.y * x.y);
        }
        const double px = (double)G3[3 * i + 0] + kx, py = (double)G3[3 * i + 1] + ky, pz = (double)G3[3 * i + 2] + kz;
        double qx, qy, qz;
        recip_times(B, px, py, pz, &qx, &qy, &qz);
        v[0] = qx * qx * s; v[1] = qy * qy * s; v[2] = qz * qz * s;
        v[3] = qz * qy * s; v[4] = qz * qx * s; v[5] = qy * qx * s;
    }
    st_block_reduce<6>(v, partial, gridDim.x, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------ nonlocal
// W[j, t * cc + c] = dP_ab(t) of projector column c0 + c at row j.  Full-sphere rows: sphere row j.  Half format
// (gidx != null): row j stands for G of sphere row gidx[j], scaled by sqrt(2) (row 0 is G = 0: real part, unscaled) as
// the half-format projectors are.
__global__ __launch_bounds__(256) void k_st_build_dproj(int64_t rows, int c0, int cc, const int* __restrict__ G3,
                                                        const int* __restrict__ gidx, Mat3 B, double kx, double ky,
                                                        double kz, double inv_sqrt_vol, const ProjCol* __restrict__ cols,
                                                        cd* __restrict__ W, int64_t ldw) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= rows) return;
    const int64_t r = gidx ? (int64_t)gidx[j] : j;
    const double px = (double)G3[3 * r + 0] + kx, py = (double)G3[3 * r + 1] + ky, pz = (double)G3[3 * r + 2] + kz;
    double qx, qy, qz;
    recip_times(B, px, py, pz, &qx, &qy, &qz);
    const double scale = inv_sqrt_vol * ((gidx && j > 0) ? ST_SQRT2 : 1.0);
    for (int c = blockIdx.y; c < cc; c += gridDim.y) {
        const ProjCol pc = cols[c0 + c];
        double amp[6];
        hgh_dproj_amplitudes(pc.l, pc.m, pc.i, pc.rp, qx, qy, qz, amp);
        double sn, cs;
        sincos(-2.0 * M_PI * (px * pc.rx + py * pc.ry + pz * pc.rz), &sn, &cs);
        double ur = cs, ui = sn;
        rotate_minus_i_pow(pc.l, &ur, &ui);        // (-i)^l e^{i ph}
        const bool row0 = gidx && j == 0;
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const double f = amp[t] * scale;
            W[j + (int64_t)(t * cc + c) * ldw] = make_double2(f * ur, row0 ? 0.0 : f * ui);
        }
    }
}

// per atom a of the chunk [a0, a0 + gridDim.x): part[6 a + t] += sum_n w_n sum_ij Re[conj(p_i) D_ij T[t cc + j - c0, n]];
// Pp = P' psi (n_p x nb, ld n_p), T = W' psi (6 cc x nb, ld 6 cc).  part[6 n_atoms] is set when D couples atom a's
// columns to columns outside the atom.
__global__ __launch_bounds__(256) void k_st_nl_contract(int n_p, int nb, int a0, int c0, int cc, const cd* __restrict__ Pp,
                                                        const cd* __restrict__ T, const double* __restrict__ D, int bw,
                                                        const int* __restrict__ col_start, const double* __restrict__ w,
                                                        int n_atoms, double* __restrict__ part) {
    const int a = a0 + blockIdx.x;
    const int s0 = col_start[a], s1 = col_start[a + 1], na = s1 - s0;
    double f[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool bad = false;
    const int64_t items = (int64_t)na * nb;
    const int64_t ldt = 6 * (int64_t)cc;
    for (int64_t it = threadIdx.x; it < items; it += 256) {
        const int n = (int)(it / na), i = s0 + (int)(it % na);
        const cd p = Pp[i + (int64_t)n * n_p];
        for (int j = i - bw; j <= i + bw; ++j) {
            if (j < 0 || j >= n_p) continue;
            const double d = D[i + (int64_t)j * n_p];
            if (d == 0.0) continue;
            if (j < s0 || j >= s1) {
                bad = true;
                continue;
            }
            const double wd = w[n] * d;
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const cd q = T[(int64_t)t * cc + (j - c0) + (int64_t)n * ldt];
                f[t] += wd * (p.x * q.x + p.y * q.y);
            }
        }
    }
    block_reduce<6>(f);
    if (threadIdx.x == 0)
#pragma unroll
        for (int t = 0; t < 6; ++t) part[6 * a + t] += f[t];
    if (bad) part[6 * n_atoms] = 1.0;     // (benign race: every writer stores the same value)
}

int stress_kinetic_nonlocal(dftk_mi_kblock* kb, const double* recip_h, const double* kcoord_h, int nb, const cd* psi,
                            int64_t ld_psi, const double* weight_h, int n_species, const double* rp_h, const int* nproj_h,
                            int n_atoms, const int* species_of_atom_h, const double* positions_h, const int* col_start_h,
                            double* stress_h) {
    dftk_mi_basis* b = kb->basis;
    if (nb < 0 || n_atoms < 0 || n_species < 0) return DFTK_MI_EINVAL;
    if (kb->sh_comm) {
        dftk_set_error("stress_kinetic_nonlocal: plane-wave sharded blocks are not supported");
        return DFTK_MI_EINVAL;
    }
    if (n_atoms > 0 && (!species_of_atom_h || !positions_h || !rp_h || !nproj_h || !col_start_h)) return DFTK_MI_EINVAL;
    // projector columns exactly as build_projectors_hgh lists them
    std::vector<ProjCol> cols;
    std::vector<int> implied;
    CHK(list_projector_columns(n_species, rp_h, nproj_h, n_atoms, species_of_atom_h, positions_h, &cols, &implied));
    for (int a = 0; a < n_atoms; ++a)
        if (col_start_h[a] != implied[a]) {
            dftk_set_error("stress_kinetic_nonlocal: col_start[%d] = %d, the species table implies %d", a, col_start_h[a],
                           implied[a]);
            return DFTK_MI_EINVAL;
        }
    if ((int)cols.size() != kb->n_p || (n_atoms > 0 && col_start_h[n_atoms] != kb->n_p)) {
        dftk_set_error("stress_kinetic_nonlocal: the atoms own %d projector columns, the block has n_p = %d",
                       (int)cols.size(), kb->n_p);
        return DFTK_MI_EINVAL;
    }
    if (nb == 0) return 0;
    if (!psi || !weight_h || ld_psi < kb->n_G) return DFTK_MI_EINVAL;
    const bool gamma = kb->gr && kb->gr->on;
    if (gamma && (kcoord_h[0] != 0.0 || kcoord_h[1] != 0.0 || kcoord_h[2] != 0.0)) return DFTK_MI_EINVAL;
    CHK(ensure_G3(kb));
    const int n_p = kb->n_p;
    const int64_t n_G = kb->n_G;
    const cd* P = kb->P;
    int64_t ldP = kb->ldP, rows = n_G;
    if (gamma && n_p > 0) {
        CHK(gamma_projectors(kb));
        rows = gamma_local_rows(kb);
        P = kb->gr->P_half;
        ldP = rows;
    }
    // chunk of derivative-projector columns: whole atoms within 512 MiB (at least one atom; on the 250-atom bench cell
    // 256 MiB left the complex path with 60-row products, half a tile of the zgemm kernel)
    int max_atom = 0;
    for (int a = 0; a < n_atoms; ++a) max_atom = std::max(max_atom, col_start_h[a + 1] - col_start_h[a]);
    const size_t w_budget = st_budget((size_t)512 << 20);
    const int cc_max = n_p == 0 ? 0
                                : (int)std::min<size_t>((size_t)n_p, std::max<size_t>((size_t)max_atom,
                                                                                     w_budget / (6 * (size_t)rows * sizeof(cd))));
    const size_t per_band = ((size_t)(gamma ? rows : 0) + (size_t)n_p + 6 * (size_t)cc_max) * sizeof(cd);
    const size_t budget = st_budget((size_t)512 << 20);
    const int cb = (int)std::max<size_t>(1, std::min<size_t>((size_t)nb, per_band ? budget / per_band : (size_t)nb));
    const int64_t kin_blocks = (n_G + 255) / 256;
    cd *W, *Z, *Pp, *T;
    double *d_w, *d_part, *d_kin, *d_out;
    int* d_cs;
    ProjCol* d_cols;
    WsCarver ws;
    ws.take(&W, (size_t)rows * 6 * cc_max), ws.take(&Z, gamma ? (size_t)rows * cb : 0), ws.take(&Pp, (size_t)n_p * cb);
    ws.take(&T, (size_t)6 * cc_max * cb), ws.take(&d_w, (size_t)nb), ws.take(&d_part, (size_t)(6 * n_atoms + 1));
    ws.take(&d_cs, (size_t)(n_atoms + 1)), ws.take(&d_cols, cols.size()), ws.take(&d_kin, (size_t)6 * kin_blocks);
    ws.take(&d_out, 6);
    CHK(scratch_grow(b, b->T1, ws.bytes()));
    ws.bind(b->T1);
    HIPCHK(hipMemcpyAsync(d_w, weight_h, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, b->stream));
    const Mat3 B = make_mat3(recip_h);
    // kinetic: one pass over the caller's full-sphere orbitals
    hipLaunchKernelGGL(k_st_kinetic, dim3((unsigned)kin_blocks), dim3(256), 0, b->stream, n_G, nb, (const int*)kb->d_G3, B,
                       kcoord_h[0], kcoord_h[1], kcoord_h[2], psi, ld_psi, (const double*)d_w, d_kin);
    HIPCHK(hipGetLastError());
    CHK(launch_rowsum(b, 6, kin_blocks, d_kin, -1.0, d_out));
    double kin[6];
    HIPCHK(hipMemcpyAsync(kin, d_out, sizeof(kin), hipMemcpyDeviceToHost, b->stream));
    std::vector<double> part((size_t)6 * n_atoms + 1, 0.0);
    if (n_p > 0) {
        HIPCHK(hipMemcpyAsync(d_cs, col_start_h, (size_t)(n_atoms + 1) * sizeof(int), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(d_cols, cols.data(), cols.size() * sizeof(ProjCol), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemsetAsync(d_part, 0, (size_t)(6 * n_atoms + 1) * sizeof(double), b->stream));
        const cd one = {1.0, 0.0}, zero = {0.0, 0.0};
        const int flags = gamma ? DFTK_MI_GEMM_REAL : 0;
        for (int n0 = 0; n0 < nb; n0 += cb) {
            const int m = std::min(cb, nb - n0);
            const cd* X = psi + (int64_t)n0 * ld_psi;
            int64_t ldx = ld_psi;
            if (gamma) {
                // (every column is a real-symmetric field up to a global phase: the aligned compression)
                CHK(gamma_lobpcg_load(kb, m, X, ld_psi, Z, rows, true));
                X = Z;
                ldx = rows;
            }
            CHK(zgemm(b, 'C', n_p, m, rows, one, P, ldP, X, ldx, zero, Pp, n_p, flags));
            for (int a0 = 0; a0 < n_atoms;) {
                int a1 = a0;
                while (a1 < n_atoms && col_start_h[a1 + 1] - col_start_h[a0] <= cc_max) ++a1;
                if (a1 == a0) return DFTK_MI_EINVAL;      // (cannot happen: cc_max >= the largest atom)
                const int c0 = col_start_h[a0], cc = col_start_h[a1] - c0;
                if (cc > 0) {
                    const unsigned gy = (unsigned)std::min(cc, 64);
                    hipLaunchKernelGGL(k_st_build_dproj, dim3((unsigned)((rows + 255) / 256), gy), dim3(256), 0, b->stream,
                                       rows, c0, cc, (const int*)kb->d_G3, gamma ? (const int*)kb->gr->d_g : (const int*)nullptr,
                                       B, kcoord_h[0], kcoord_h[1], kcoord_h[2], 1.0 / sqrt(b->volume),
                                       (const ProjCol*)d_cols, W, rows);
                    HIPCHK(hipGetLastError());
                    CHK(zgemm(b, 'C', 6 * (int64_t)cc, m, rows, one, W, rows, X, ldx, zero, T, 6 * (int64_t)cc, flags));
                    hipLaunchKernelGGL(k_st_nl_contract, dim3((unsigned)(a1 - a0)), dim3(256), 0, b->stream, n_p, m, a0, c0,
                                       cc, (const cd*)Pp, (const cd*)T, (const double*)kb->d_D, kb->D_bw, (const int*)d_cs,
                                       (const double*)(d_w + n0), n_atoms, d_part);
                    HIPCHK(hipGetLastError());
                }
                a0 = a1;
            }
        }
        HIPCHK(hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    if (part[6 * (size_t)n_atoms] != 0.0) {
        dftk_set_error("stress_kinetic_nonlocal: D couples the projector columns of different atoms");
        return DFTK_MI_EINVAL;
    }
    for (int t = 0; t < 6; ++t) {
        stress_h[t] += kin[t];
        double s = 0.0;
        for (int a = 0; a < n_atoms; ++a) s += part[6 * (size_t)a + t];
        stress_h[6 + t] += 2.0 * s;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ cube terms
// R: unnormalised forward DFT of the total density, rho(G) = norm R(G).  partial[k * n_blocks + block], k = 0..13 as
// dftk_mi_stress_cube lists them.  tab: per atom [t_x(nx) | t_y(ny) | t_z(nz)], t(i) = exp(-2 pi i g(i) r)
__global__ __launch_bounds__(256) void k_st_cube(int nx, int ny, int nz, Mat3 B, double norm, double inv_sqrt_vol,
                                                 const cd* __restrict__ R, int n_atoms, const int* __restrict__ species,
                                                 const double* __restrict__ par, const cd* __restrict__ tab,
                                                 double* __restrict__ partial) {
    const int64_t N = (int64_t)nx * ny * nz;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double v[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) v[k] = 0.0;
    if (idx < N) {
        const int ix = (int)(idx % nx), iy = (int)((idx / nx) % ny), iz = (int)(idx / ((int64_t)nx * ny));
        if (!unpaired_nyquist(ix, iy, iz, nx, ny, nz) && idx != 0) {
            double qx, qy, qz;
            recip_times(B, (double)signed_freq(ix, nx), (double)signed_freq(iy, ny), (double)signed_freq(iz, nz), &qx, &qy,
                        &qz);
            const double qq[6] = {qx * qx, qy * qy, qz * qz, qz * qy, qz * qx, qy * qx};
            const double q2 = qq[0] + qq[1] + qq[2];
            const cd r = R[idx];
            const double rr = norm * r.x, ri = norm * r.y;
            const double h = 4.0 * M_PI * (rr * rr + ri * ri) / q2;
            v[13] = 0.5 * h;
#pragma unroll
            for (int t = 0; t < 6; ++t) v[6 + t] = h * qq[t] / q2;
            const int64_t tstride = (int64_t)nx + ny + nz;
            double eloc = 0.0, dl = 0.0;
            int a = 0;
            while (a < n_atoms) {
                const int s = species[a];
                double Sr = 0.0, Si = 0.0;
                for (; a < n_atoms && species[a] == s; ++a) {
                    const cd* t = tab + a * tstride;
                    const cd tx = t[ix], ty = t[nx + iy], tz = t[nx + ny + iz];
                    const double ur = tx.x * ty.x - tx.y * ty.y, ui = tx.x * ty.y + tx.y * ty.x;
                    Sr += ur * tz.x - ui * tz.y;
                    Si += ur * tz.y + ui * tz.x;
                }
                const double* p = par + 8 * s;
                double ff, dff;
                hgh_local_ff_deriv(p, q2 * p[0] * p[0], &ff, &dff);
                const double c = (rr * Sr + ri * Si) * inv_sqrt_vol;       // Re[conj(rho(G)) S_s(G)] / sqrt(Omega)
                eloc += c * ff;
                dl += c * dff * 2.0 * p[0] * p[0];                          // ff'(|G|) / |G|
            }
            v[12] = eloc;
#pragma unroll
            for (int t = 0; t < 6; ++t) v[t] = -dl * qq[t];
        }
    }
    st_block_reduce<14>(v, partial, gridDim.x, blockIdx.x);
}

int stress_cube(dftk_mi_kblock* cube_kb, const double* recip_h, int n_species, const double* par_h, int n_atoms,
                const int* species_of_atom_h, const double* positions_h, const double* rho_d, double* out_h) {
    dftk_mi_basis* b = cube_kb->basis;
    const int nx = b->nx, ny = b->ny, nz = b->nz;
    const int64_t N = (int64_t)nx * ny * nz;
    if (cube_kb->n_G != N) {
        dftk_set_error("stress_cube: the k-block must span the whole cube");
        return DFTK_MI_EINVAL;
    }
    if (n_atoms < 0 || n_species < 0 || (n_atoms > 0 && (!species_of_atom_h || !positions_h || !par_h))) return DFTK_MI_EINVAL;
    CHK(check_species_grouped("stress_cube", n_species, n_atoms, species_of_atom_h));
    CHK(scratch_grow(b, b->dense_ws, 2 * (size_t)N * sizeof(cd)));
    cd* c1 = reinterpret_cast<cd*>(b->dense_ws.get());
    cd* c2 = c1 + N;
    CHK(launch_real_to_cplx(b, N, rho_d, c1));
    CHK(launch_fft_from_cube(cube_kb, c1, c2));
    const std::vector<cd> tab = phase_tables_host(nx, ny, nz, n_atoms, positions_h);
    const int64_t n_blocks = (N + 255) / 256;
    cd* d_tab;
    double *d_part, *d_out, *d_par;
    int* d_sp;
    WsCarver ws;
    ws.take(&d_tab, tab.size()), ws.take(&d_part, (size_t)14 * n_blocks), ws.take(&d_out, 14);
    ws.take(&d_par, (size_t)n_species * 8), ws.take(&d_sp, (size_t)n_atoms);
    CHK(ensure_ws(b, ws.bytes()));
    ws.bind(b->ws);
    if (n_atoms > 0) {
        HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(cd), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(d_par, par_h, (size_t)n_species * 8 * sizeof(double), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(d_sp, species_of_atom_h, (size_t)n_atoms * sizeof(int), hipMemcpyHostToDevice, b->stream));
    }
    hipLaunchKernelGGL(k_st_cube, dim3((unsigned)n_blocks), dim3(256), 0, b->stream, nx, ny, nz, make_mat3(recip_h),
                       sqrt(b->volume) / (double)N, 1.0 / sqrt(b->volume), (const cd*)c2, n_atoms, (const int*)d_sp,
                       (const double*)d_par, (const cd*)d_tab, d_part);
    HIPCHK(hipGetLastError());
    CHK(launch_rowsum(b, 14, n_blocks, d_part, 1.0, d_out));
    HIPCHK(hipMemcpyAsync(out_h, d_out, 14 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));     // (host tables and b->ws are free again)
    return 0;
}

// ------------------------------------------------------------------------------------------------ exchange-correlation
#define ST_XC_BLOCKS 1024
__global__ __launch_bounds__(256) void k_st_xc(int64_t n, int n_spin, const double* __restrict__ rho,
                                               const double* __restrict__ vrho, const double* __restrict__ e,
                                               const double* __restrict__ vsigma, const double* __restrict__ grad,
                                               double* __restrict__ partial) {
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (e) v[0] += e[i];
        double s = vrho[i] * rho[i];
        if (n_spin == 2) s += vrho[n + i] * rho[n + i];
        v[1] += s;
        if (vsigma) {
            const double vs = vsigma[i], gx = grad[i], gy = grad[n + i], gz = grad[2 * n + i];
            v[2] += vs * gx * gx; v[3] += vs * gy * gy; v[4] += vs * gz * gz;
            v[5] += vs * gz * gy; v[6] += vs * gz * gx; v[7] += vs * gy * gx;
        }
    }
    st_block_reduce<8>(v, partial, gridDim.x, blockIdx.x);
}

int stress_xc(dftk_mi_basis* b, int64_t n, int n_spin, const double* rho_d, const double* vrho_d, const double* e_d,
              const double* vsigma_d, const double* grad_d, double* out_h) {
    const int64_t n_blocks = std::max<int64_t>(1, std::min<int64_t>(ST_XC_BLOCKS, (n + 255) / 256));
    double *d_part, *d_out;
    WsCarver ws;
    ws.take(&d_part, (size_t)8 * n_blocks), ws.take(&d_out, 8);
    CHK(ensure_ws(b, ws.bytes()));
    ws.bind(b->ws);
    hipLaunchKernelGGL(k_st_xc, dim3((unsigned)n_blocks), dim3(256), 0, b->stream, n, n_spin, rho_d, vrho_d, e_d, vsigma_d,
                       grad_d, d_part);
    HIPCHK(hipGetLastError());
    CHK(launch_rowsum(b, 8, n_blocks, d_part, 1.0, d_out));
    HIPCHK(hipMemcpyAsync(out_h, d_out, 8 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}
