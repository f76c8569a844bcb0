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
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#define ST_SQRT2 1.4142135623730951

struct SMat3 {       // recip_lattice, column-major
    double b[9];
};

struct SCol {        // one column of P
    double rx, ry, rz;   // atom position (reduced)
    double rp;           // r_l of the species
    int l, m, i, pad;    // angular momentum, magnetic index, radial index (1-based)
};

// ------------------------------------------------------------------------------------------------ HGH forms
// eval_psp_projector_fourier (PspHgh.jl:140-164, divided by p^l) as a function of t2 = (p r_l)^2, and its t2 derivative
__host__ __device__ inline bool st_hgh_radial(int l, int i, double rp, double t2, double* R, double* dR) {
    const double common = 4.0 * pow(M_PI, 1.25) * sqrt(ldexp(1.0, l + 1) * rp * rp * rp) * exp(-t2 / 2.0);
    double c, poly = 1.0, dpoly = 0.0;
    switch (l * 4 + i) {
        case 0 * 4 + 1: c = 1.0; break;
        case 0 * 4 + 2: c = 2.0 / sqrt(15.0); poly = 3.0 - t2; dpoly = -1.0; break;
        case 0 * 4 + 3: c = 4.0 / (3.0 * sqrt(105.0)); poly = 15.0 - 10.0 * t2 + t2 * t2; dpoly = -10.0 + 2.0 * t2; break;
        case 1 * 4 + 1: c = rp / sqrt(3.0); break;
        case 1 * 4 + 2: c = 2.0 * rp / sqrt(105.0); poly = 5.0 - t2; dpoly = -1.0; break;
        case 1 * 4 + 3: c = 4.0 * rp / (3.0 * sqrt(1155.0)); poly = 35.0 - 14.0 * t2 + t2 * t2; dpoly = -14.0 + 2.0 * t2; break;
        case 2 * 4 + 1: c = rp * rp / sqrt(15.0); break;
        case 2 * 4 + 2: c = 2.0 * rp * rp / (3.0 * sqrt(105.0)); poly = 7.0 - t2; dpoly = -1.0; break;
        case 3 * 4 + 1: c = rp * rp * rp / sqrt(105.0); break;
        default: *R = *dR = nan(""); return false;
    }
    *R = common * c * poly;
    *dR = common * c * (dpoly - 0.5 * poly);
    return true;
}

// r^l Y_lm (spherical_harmonics.jl:31-66) and its gradient
__host__ __device__ inline double st_solid_harmonic(int l, int m, double x, double y, double z, double* g) {
    const double pi = M_PI;
    g[0] = g[1] = g[2] = 0.0;
    if (l == 0) return sqrt(1.0 / (4.0 * pi));
    if (l == 1) {
        const double c = sqrt(3.0 / (4.0 * pi));
        if (m == -1) { g[1] = c; return c * y; }
        if (m == 0) { g[2] = c; return c * z; }
        g[0] = c;
        return c * x;
    }
    if (l == 2) {
        const double c = sqrt(15.0 / (4.0 * pi));
        switch (m) {
            case -2: g[0] = c * y; g[1] = c * x; return c * x * y;
            case -1: g[1] = c * z; g[2] = c * y; return c * y * z;
            case 0: {
                const double d = sqrt(5.0 / (16.0 * pi));
                g[0] = -2.0 * d * x; g[1] = -2.0 * d * y; g[2] = 4.0 * d * z;
                return d * (2.0 * z * z - x * x - y * y);
            }
            case 1: g[0] = c * z; g[2] = c * x; return c * x * z;
            default: {
                const double d = sqrt(15.0 / (16.0 * pi));
                g[0] = 2.0 * d * x; g[1] = -2.0 * d * y;
                return d * (x * x - y * y);
            }
        }
    }
    switch (m) {
        case -3: {
            const double a = sqrt(35.0 / (32.0 * pi));
            g[0] = a * 6.0 * x * y; g[1] = a * (3.0 * x * x - 3.0 * y * y);
            return a * (3.0 * x * x - y * y) * y;
        }
        case -2: {
            const double a = sqrt(105.0 / (4.0 * pi));
            g[0] = a * y * z; g[1] = a * x * z; g[2] = a * x * y;
            return a * x * y * z;
        }
        case -1: {
            const double a = sqrt(21.0 / (32.0 * pi));
            g[0] = -2.0 * a * x * y; g[1] = a * (4.0 * z * z - x * x - 3.0 * y * y); g[2] = 8.0 * a * y * z;
            return a * y * (4.0 * z * z - x * x - y * y);
        }
        case 0: {
            const double a = sqrt(7.0 / (16.0 * pi));
            g[0] = -6.0 * a * x * z; g[1] = -6.0 * a * y * z; g[2] = a * (6.0 * z * z - 3.0 * x * x - 3.0 * y * y);
            return a * z * (2.0 * z * z - 3.0 * x * x - 3.0 * y * y);
        }
        case 1: {
            const double a = sqrt(21.0 / (32.0 * pi));
            g[0] = a * (4.0 * z * z - 3.0 * x * x - y * y); g[1] = -2.0 * a * x * y; g[2] = 8.0 * a * x * z;
            return a * x * (4.0 * z * z - x * x - y * y);
        }
        case 2: {
            const double a = sqrt(105.0 / (16.0 * pi));
            g[0] = 2.0 * a * x * z; g[1] = -2.0 * a * y * z; g[2] = a * (x * x - y * y);
            return a * (x * x - y * y) * z;
        }
        default: {
            const double a = sqrt(35.0 / (32.0 * pi));
            g[0] = a * (3.0 * x * x - 3.0 * y * y); g[1] = -6.0 * a * x * y;
            return a * (x * x - 3.0 * y * y) * x;
        }
    }
}

// real amplitudes of the six strain derivatives of R_li(|q|) Y_lm(q) / sqrt(Omega) (without the 1 / sqrt(Omega) itself)
__host__ __device__ inline void st_dproj_amplitudes(int l, int m, int i, double rp, double qx, double qy, double qz,
                                                    double* out) {
    const double t2 = (qx * qx + qy * qy + qz * qz) * rp * rp;
    double R, dR, gY[3];
    st_hgh_radial(l, i, rp, t2, &R, &dR);
    const double Y = st_solid_harmonic(l, m, qx, qy, qz, gY);
    const double q[3] = {qx, qy, qz};
    const int ia[6] = {0, 1, 2, 2, 2, 1}, ib[6] = {0, 1, 2, 1, 0, 0};
    const double cr = 2.0 * rp * rp * dR * Y;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int a = ia[t], b = ib[t];
        out[t] = (a == b ? -0.5 * R * Y : 0.0) - cr * q[a] * q[b] - 0.5 * R * (q[a] * gY[b] + q[b] * gY[a]);
    }
}

// the HGH local form factor ff(p) (as hgh_local_ff of force_kernels.hip) and d ff / d t2, t2 = (p rloc)^2 > 0
__host__ __device__ inline void st_hgh_local(const double* q, double t2, double* ff, double* dff) {
    const double rloc = q[0], Zion = q[1];
    const double P = q[2] + q[3] * (3.0 - t2) + q[4] * (15.0 - 10.0 * t2 + t2 * t2) +
                     q[5] * (105.0 - 105.0 * t2 + 21.0 * t2 * t2 - t2 * t2 * t2);
    const double dP = -q[3] + q[4] * (-10.0 + 2.0 * t2) + q[5] * (-105.0 + 42.0 * t2 - 3.0 * t2 * t2);
    const double A = 4.0 * M_PI * rloc * rloc * exp(-t2 / 2.0), Bc = sqrt(M_PI / 2.0) * rloc;
    const double inner = -Zion / t2 + Bc * P;
    *ff = A * inner;
    *dff = A * (Zion / (t2 * t2) + Bc * dP - 0.5 * inner);
}

// (tools/host_stress_check.cpp includes this file with DFTK_STRESS_HOST_CHECK and checks the closed forms above against
// finite differences on the host: everything below needs the HIP runtime and is left out there)
#ifndef DFTK_STRESS_HOST_CHECK
// ------------------------------------------------------------------------------------------------ reductions
// sum of K values per thread over a workgroup of 256; thread 0 writes partial[k * n_blocks + block]
template <int K>
__device__ inline void st_block_reduce(const double* v, double* __restrict__ partial, int64_t n_blocks, int64_t block) {
    __shared__ double sh[K][256];
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) partial[(int64_t)k * n_blocks + block] = sh[k][0];
}

// out[r] (+)= scale * sum_i in[r * n + i], one workgroup per row, fixed order
__global__ __launch_bounds__(256) void k_st_rowsum(int64_t n, const double* __restrict__ in, double scale,
                                                   double* __restrict__ out, int accumulate) {
    __shared__ double sh[256];
    const double* x = in + (int64_t)blockIdx.x * n;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += x[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (accumulate ? out[blockIdx.x] : 0.0) + scale * sh[0];
}

// workspace budgets in bytes; DFTK_MI_STRESS_WS_KIB (testing aid, read at every call) replaces both defaults so that a
// small cell runs through several projector-column and band chunks
static size_t st_budget(size_t dflt) {
    const char* e = getenv("DFTK_MI_STRESS_WS_KIB");
    if (!e || !*e) return dflt;
    const long v = atol(e);
    return v > 0 ? (size_t)v << 10 : dflt;
}

static int st_grow(cd** buf, size_t* have, size_t need, hipStream_t s) {
    if (need <= *have) return 0;
    HIPCHK(hipStreamSynchronize(s));
    if (*buf) HIPCHK(hipFree(*buf));
    *buf = nullptr;
    *have = 0;
    HIPCHK(dftk_scratch_malloc((void**)buf, need));
    *have = need;
    return 0;
}

// ------------------------------------------------------------------------------------------------ kinetic
// partial[t * n_blocks + block] = sum over the block's rows of q_a q_b sum_n w_n |psi_n(row)|^2
__global__ __launch_bounds__(256) void k_st_kinetic(int64_t rows, int nb, const int* __restrict__ G3, SMat3 B, double kx,
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
        const double qx = px * B.b[0] + py * B.b[3] + pz * B.b[6];
        const double qy = px * B.b[1] + py * B.b[4] + pz * B.b[7];
        const double qz = px * B.b[2] + py * B.b[5] + pz * B.b[8];
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
                                                        const int* __restrict__ gidx, SMat3 B, double kx, double ky,
                                                        double kz, double inv_sqrt_vol, const SCol* __restrict__ cols,
                                                        cd* __restrict__ W, int64_t ldw) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= rows) return;
    const int64_t r = gidx ? (int64_t)gidx[j] : j;
    const double px = (double)G3[3 * r + 0] + kx, py = (double)G3[3 * r + 1] + ky, pz = (double)G3[3 * r + 2] + kz;
    const double qx = px * B.b[0] + py * B.b[3] + pz * B.b[6];
    const double qy = px * B.b[1] + py * B.b[4] + pz * B.b[7];
    const double qz = px * B.b[2] + py * B.b[5] + pz * B.b[8];
    const double scale = inv_sqrt_vol * ((gidx && j > 0) ? ST_SQRT2 : 1.0);
    for (int c = blockIdx.y; c < cc; c += gridDim.y) {
        const SCol pc = cols[c0 + c];
        double amp[6];
        st_dproj_amplitudes(pc.l, pc.m, pc.i, pc.rp, qx, qy, qz, amp);
        double sn, cs;
        sincos(-2.0 * M_PI * (px * pc.rx + py * pc.ry + pz * pc.rz), &sn, &cs);
        // (-i)^l e^{i ph}: 1, -i, -1, i times (cs + i sn)
        double ur, ui;
        switch (pc.l & 3) {
            case 0: ur = cs; ui = sn; break;
            case 1: ur = sn; ui = -cs; break;
            case 2: ur = -cs; ui = -sn; break;
            default: ur = -sn; ui = cs; break;
        }
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
    __shared__ double sh[6][256];
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
#pragma unroll
    for (int t = 0; t < 6; ++t) sh[t][threadIdx.x] = f[t];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h)
#pragma unroll
            for (int t = 0; t < 6; ++t) sh[t][threadIdx.x] += sh[t][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0)
#pragma unroll
        for (int t = 0; t < 6; ++t) part[6 * a + t] += sh[t][0];
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
    std::vector<SCol> cols;
    for (int a = 0; a < n_atoms; ++a) {
        const int s = species_of_atom_h[a];
        if (s < 0 || s >= n_species) return DFTK_MI_EINVAL;
        if (col_start_h[a] != (int)cols.size()) {
            dftk_set_error("stress_kinetic_nonlocal: col_start[%d] = %d, the species table implies %d", a, col_start_h[a],
                           (int)cols.size());
            return DFTK_MI_EINVAL;
        }
        for (int l = 0; l < 4; ++l) {
            const int nl = nproj_h[4 * s + l];
            if (nl < 0 || nl > 3 || (l == 2 && nl > 2) || (l == 3 && nl > 1)) {
                dftk_set_error("HGH projector l=%d with %d radial functions is not tabulated", l, nl);
                return DFTK_MI_EINVAL;
            }
            for (int m = -l; m <= l; ++m)
                for (int i = 1; i <= nl; ++i)
                    cols.push_back(SCol{positions_h[3 * a], positions_h[3 * a + 1], positions_h[3 * a + 2],
                                        rp_h[4 * s + l], l, m, i, 0});
        }
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
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_W = up((size_t)rows * 6 * cc_max * sizeof(cd)), b_Z = up(gamma ? (size_t)rows * cb * sizeof(cd) : 0),
                 b_Pp = up((size_t)n_p * cb * sizeof(cd)), b_T = up((size_t)6 * cc_max * cb * sizeof(cd)),
                 b_w = up((size_t)nb * sizeof(double)), b_part = up((size_t)(6 * n_atoms + 1) * sizeof(double)),
                 b_cs = up((size_t)(n_atoms + 1) * sizeof(int)), b_cols = up(cols.size() * sizeof(SCol)),
                 b_kin = up((size_t)6 * kin_blocks * sizeof(double)), b_out = up(6 * sizeof(double));
    CHK(st_grow(&b->T1, &b->T1_bytes, b_W + b_Z + b_Pp + b_T + b_w + b_part + b_cs + b_cols + b_kin + b_out, b->stream));
    char* base = reinterpret_cast<char*>(b->T1);
    cd* W = reinterpret_cast<cd*>(base); base += b_W;
    cd* Z = reinterpret_cast<cd*>(base); base += b_Z;
    cd* Pp = reinterpret_cast<cd*>(base); base += b_Pp;
    cd* T = reinterpret_cast<cd*>(base); base += b_T;
    double* d_w = reinterpret_cast<double*>(base); base += b_w;
    double* d_part = reinterpret_cast<double*>(base); base += b_part;
    int* d_cs = reinterpret_cast<int*>(base); base += b_cs;
    SCol* d_cols = reinterpret_cast<SCol*>(base); base += b_cols;
    double* d_kin = reinterpret_cast<double*>(base); base += b_kin;
    double* d_out = reinterpret_cast<double*>(base);
    HIPCHK(hipMemcpyAsync(d_w, weight_h, (size_t)nb * sizeof(double), hipMemcpyHostToDevice, b->stream));
    SMat3 B;
    for (int i = 0; i < 9; ++i) B.b[i] = recip_h[i];
    // kinetic: one pass over the caller's full-sphere orbitals
    hipLaunchKernelGGL(k_st_kinetic, dim3((unsigned)kin_blocks), dim3(256), 0, b->stream, n_G, nb, (const int*)kb->d_G3, B,
                       kcoord_h[0], kcoord_h[1], kcoord_h[2], psi, ld_psi, (const double*)d_w, d_kin);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_st_rowsum, dim3(6), dim3(256), 0, b->stream, kin_blocks, (const double*)d_kin, -1.0, d_out, 0);
    HIPCHK(hipGetLastError());
    double kin[6];
    HIPCHK(hipMemcpyAsync(kin, d_out, sizeof(kin), hipMemcpyDeviceToHost, b->stream));
    std::vector<double> part((size_t)6 * n_atoms + 1, 0.0);
    if (n_p > 0) {
        HIPCHK(hipMemcpyAsync(d_cs, col_start_h, (size_t)(n_atoms + 1) * sizeof(int), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(d_cols, cols.data(), cols.size() * sizeof(SCol), hipMemcpyHostToDevice, b->stream));
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
                                       (const SCol*)d_cols, W, rows);
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
__device__ inline int st_fold(int i, int n) { return i <= (n - 1) / 2 ? i : i - n; }

__global__ __launch_bounds__(256) void k_st_real_to_cplx(int64_t n, const double* __restrict__ x, cd* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = make_double2(x[i], 0.0);
}

// R: unnormalised forward DFT of the total density, rho(G) = norm R(G).  partial[k * n_blocks + block], k = 0..13 as
// dftk_mi_stress_cube lists them.  tab: per atom [t_x(nx) | t_y(ny) | t_z(nz)], t(i) = exp(-2 pi i g(i) r)
__global__ __launch_bounds__(256) void k_st_cube(int nx, int ny, int nz, SMat3 B, double norm, double inv_sqrt_vol,
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
        const bool unpaired = ((nx % 2 == 0) && ix == nx / 2) || ((ny % 2 == 0) && iy == ny / 2) || ((nz % 2 == 0) && iz == nz / 2);
        if (!unpaired && idx != 0) {
            const double gx = (double)st_fold(ix, nx), gy = (double)st_fold(iy, ny), gz = (double)st_fold(iz, nz);
            const double qx = gx * B.b[0] + gy * B.b[3] + gz * B.b[6];
            const double qy = gx * B.b[1] + gy * B.b[4] + gz * B.b[7];
            const double qz = gx * B.b[2] + gy * B.b[5] + gz * B.b[8];
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
                st_hgh_local(p, q2 * p[0] * p[0], &ff, &dff);
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
    for (int a = 0; a < n_atoms; ++a) {
        if (species_of_atom_h[a] < 0 || species_of_atom_h[a] >= n_species) return DFTK_MI_EINVAL;
        if (a > 0 && species_of_atom_h[a] < species_of_atom_h[a - 1]) {
            dftk_set_error("stress_cube: atoms must be grouped by species");
            return DFTK_MI_EINVAL;
        }
    }
    const size_t need = 2 * (size_t)N * sizeof(cd);
    if (need > b->dense_ws_bytes) {
        HIPCHK(hipStreamSynchronize(b->stream));
        if (b->dense_ws) HIPCHK(hipFree(b->dense_ws));
        b->dense_ws = nullptr;
        b->dense_ws_bytes = 0;
        HIPCHK(dftk_scratch_malloc(&b->dense_ws, need));
        b->dense_ws_bytes = need;
    }
    cd* c1 = reinterpret_cast<cd*>(b->dense_ws);
    cd* c2 = c1 + N;
    hipLaunchKernelGGL(k_st_real_to_cplx, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, b->stream, N, rho_d, c1);
    HIPCHK(hipGetLastError());
    CHK(launch_fft_from_cube(cube_kb, c1, c2));
    const int dims[3] = {nx, ny, nz};
    const int64_t tstride = (int64_t)nx + ny + nz;
    std::vector<cd> tab((size_t)n_atoms * tstride);
    for (int a = 0; a < n_atoms; ++a) {
        cd* t = tab.data() + (size_t)a * tstride;
        for (int d = 0; d < 3; ++d) {
            const int n = dims[d];
            for (int i = 0; i < n; ++i) {
                const int g = i <= (n - 1) / 2 ? i : i - n;
                const double ph = -2.0 * M_PI * (double)g * positions_h[3 * a + d];
                *t++ = make_double2(cos(ph), sin(ph));
            }
        }
    }
    const int64_t n_blocks = (N + 255) / 256;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_tab = up(tab.size() * sizeof(cd)), b_part = up((size_t)14 * n_blocks * sizeof(double)),
                 b_out = up(14 * sizeof(double)), b_par = up((size_t)n_species * 8 * sizeof(double)),
                 b_sp = up((size_t)n_atoms * sizeof(int));
    CHK(ensure_ws(b, b_tab + b_part + b_out + b_par + b_sp));
    char* ws = reinterpret_cast<char*>(b->ws);
    cd* d_tab = reinterpret_cast<cd*>(ws); ws += b_tab;
    double* d_part = reinterpret_cast<double*>(ws); ws += b_part;
    double* d_out = reinterpret_cast<double*>(ws); ws += b_out;
    double* d_par = reinterpret_cast<double*>(ws); ws += b_par;
    int* d_sp = reinterpret_cast<int*>(ws);
    if (n_atoms > 0) {
        HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(cd), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(d_par, par_h, (size_t)n_species * 8 * sizeof(double), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(d_sp, species_of_atom_h, (size_t)n_atoms * sizeof(int), hipMemcpyHostToDevice, b->stream));
    }
    SMat3 B;
    for (int i = 0; i < 9; ++i) B.b[i] = recip_h[i];
    hipLaunchKernelGGL(k_st_cube, dim3((unsigned)n_blocks), dim3(256), 0, b->stream, nx, ny, nz, B,
                       sqrt(b->volume) / (double)N, 1.0 / sqrt(b->volume), (const cd*)c2, n_atoms, (const int*)d_sp,
                       (const double*)d_par, (const cd*)d_tab, d_part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_st_rowsum, dim3(14), dim3(256), 0, b->stream, n_blocks, (const double*)d_part, 1.0, d_out, 0);
    HIPCHK(hipGetLastError());
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
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_part = up((size_t)8 * n_blocks * sizeof(double));
    CHK(ensure_ws(b, b_part + up(8 * sizeof(double))));
    double* d_part = reinterpret_cast<double*>(b->ws);
    double* d_out = reinterpret_cast<double*>(reinterpret_cast<char*>(b->ws) + b_part);
    hipLaunchKernelGGL(k_st_xc, dim3((unsigned)n_blocks), dim3(256), 0, b->stream, n, n_spin, rho_d, vrho_d, e_d, vsigma_d,
                       grad_d, d_part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_st_rowsum, dim3(8), dim3(256), 0, b->stream, n_blocks, (const double*)d_part, 1.0, d_out, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_h, d_out, 8 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}
#endif   // DFTK_STRESS_HOST_CHECK
