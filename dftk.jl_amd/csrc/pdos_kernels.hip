// pdos_kernels.hip -- the orbital side of band structures and projected densities of states (src/postprocess/dos.jl:70-212,
// src/common/ortho.jl:11-17) (gfx950 only).
//
// dftk_mi_lowdin_ortho: Phi <- Phi S^-1/2 with S = Phi' Phi.  The Gram matrix and the two back-products run on the library's
// zgemm, the eigen-decomposition S = V diag(lambda) V' on its blocked Jacobi (dense_heev); S^-1/2 = V diag(lambda^-1/2) V' is
// one n_cols^3 product of V with the row-scaled V' (k_scaled_adjoint).  Phi is updated in place panel by panel: a panel of
// rows is copied out and multiplied back into its own rows, so the workspace is one panel and three n_cols^2 matrices.
//
// dftk_mi_pdos_accumulate: C = Phi' psi (one zgemm), |C|^2 (k_abs2: the fat-band weights), and
//     pdos[e, p] += weight sum_n g(eps_e, eig_n) |C_pn|^2,   g = -occupation_derivative((eig_n - eps_e) / T) / T
// by k_pdos_tile: one workgroup (one wave) per tile of PD_TE energies x PD_TP projectors, a lane per energy with PD_TP
// accumulators; the band loop runs in ascending order in chunks of PD_BK bands whose |C|^2 and eigenvalues are staged in LDS
// (every lane reads the same address: broadcasts, no bank conflicts), and g is evaluated once per (energy, band) for all
// projectors of the tile.  No atomics, fixed order: two calls give bitwise equal results.
#include "common.h"
#include "batch.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int PD_TE = 64;   // energies per workgroup = lanes of its one wave
constexpr int PD_TP = 8;    // projectors per workgroup = accumulators per lane
constexpr int PD_BK = 32;   // bands per LDS stage

// T[i, j] = s[i] conj(V[j, i]): the adjoint of V with its rows scaled (n x n, both with leading dimension n)
__global__ __launch_bounds__(256) void k_scaled_adjoint(int n, const cd* __restrict__ V, const double* __restrict__ s,
                                                        cd* __restrict__ T) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * n) return;
    const int i = (int)(idx % n), j = (int)(idx / n);
    const cd v = V[j + (int64_t)n * i];
    T[idx] = make_double2(s[i] * v.x, -s[i] * v.y);
}

// w = |c|^2 entry by entry; out (optional) receives the same values
__global__ __launch_bounds__(256) void k_abs2(int64_t n, const cd* __restrict__ c, double* __restrict__ w,
                                              double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const cd v = c[idx];
    const double a = v.x * v.x + v.y * v.y;
    w[idx] = a;
    if (out) out[idx] = a;
}

// -occupation_derivative(x) of Smearing.jl:66-92, the forms of the host mirror's mixing.occupation_derivative.
// KIND 1 Fermi-Dirac: e / (1 + e)^2 with e = exp(-|x|) <= 1, so nothing overflows and |x| beyond 745 gives exactly 0;
// KIND 2 Gaussian: exp(-x^2) / sqrt(pi).
template <int KIND>
__device__ __forceinline__ double neg_occupation_derivative(double x) {
    if (KIND == 1) {
        const double e = exp(-fabs(x));
        return e / ((1.0 + e) * (1.0 + e));
    }
    return exp(-(x * x)) / 1.7724538509055160273;
}

template <int KIND>
__global__ __launch_bounds__(PD_TE) void k_pdos_tile(int n_eps, int n_proj, int n_bands, const double* __restrict__ eps,
                                                     const double* __restrict__ eig, const double* __restrict__ W,
                                                     double temperature, double weight, double* __restrict__ pdos) {
    __shared__ double sw[PD_BK][PD_TP];
    __shared__ double se[PD_BK];
    const int e = blockIdx.x * PD_TE + threadIdx.x;
    const int p0 = blockIdx.y * PD_TP;
    const double ee = e < n_eps ? eps[e] : 0.0;
    double acc[PD_TP];
#pragma unroll
    for (int j = 0; j < PD_TP; ++j) acc[j] = 0.0;
    for (int n0 = 0; n0 < n_bands; n0 += PD_BK) {
        const int nb = min(PD_BK, n_bands - n0);
        for (int t = threadIdx.x; t < PD_BK * PD_TP; t += PD_TE) {
            const int n = t / PD_TP, j = t % PD_TP;
            sw[n][j] = (n < nb && p0 + j < n_proj) ? W[(int64_t)n_proj * (n0 + n) + p0 + j] : 0.0;
        }
        if ((int)threadIdx.x < PD_BK) se[threadIdx.x] = (int)threadIdx.x < nb ? eig[n0 + threadIdx.x] : 0.0;
        __syncthreads();
        for (int n = 0; n < nb; ++n) {
            const double g = neg_occupation_derivative<KIND>((se[n] - ee) / temperature) / temperature;
#pragma unroll
            for (int j = 0; j < PD_TP; ++j) acc[j] += g * sw[n][j];
        }
        __syncthreads();
    }
    if (e >= n_eps) return;
#pragma unroll
    for (int j = 0; j < PD_TP; ++j)
        if (p0 + j < n_proj) pdos[(int64_t)n_eps * (p0 + j) + e] += weight * acc[j];
}

}   // namespace

extern "C" int dftk_mi_lowdin_ortho(dftk_mi_basis* b, int64_t n_rows, int n_cols, dftk_mi_cplx* Phi_d, int64_t ld,
                                    double* evals_h) {
    if (!b || !Phi_d || n_cols < 1 || n_cols > n_rows || ld < n_rows || n_rows > INT32_MAX) {
        dftk_set_error("lowdin_ortho: needs 1 <= n_cols <= n_rows <= ld and a block");
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("lowdin_ortho: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    HIPCHK(hipSetDevice(b->device));
    cd* Phi = reinterpret_cast<cd*>(Phi_d);
    const int n = n_cols;
    // panel of rows: at most 64 MiB, at least 256 rows
    const int64_t panel_rows = std::min<int64_t>(n_rows, std::max<int64_t>(256, ((int64_t)64 << 20) / ((int64_t)n * sizeof(cd))));
    cd *S, *V, *M, *Pn;
    double* d_s;
    WsCarver ws;
    ws.take(&S, (size_t)n * n), ws.take(&V, (size_t)n * n), ws.take(&M, (size_t)n * n);
    ws.take(&Pn, (size_t)panel_rows * n), ws.take(&d_s, (size_t)n);
    CHK(scratch_grow(b, b->T1, ws.bytes()));
    ws.bind(b->T1);
    const cd one = {1.0, 0.0}, zero = {0.0, 0.0};
    CHK(zgemm(b, 'C', n, n, n_rows, one, Phi, ld, Phi, ld, zero, S, n));
    CHK(ew_hermitize_upper(b, n, S, n));
    std::vector<double> lam(n), s(n);
    CHK(dense_heev(b, n, S, n, lam.data(), V, n));              // (S is destroyed; lam ascending on the host)
    double lmin = INFINITY, lmax = 0.0;
    for (int i = 0; i < n; ++i) {
        if (!std::isfinite(lam[i])) {
            dftk_set_error("lowdin_ortho: the overlap matrix has a non-finite eigenvalue");
            return DFTK_MI_NUM_NONFINITE;
        }
        lmin = std::min(lmin, std::fabs(lam[i]));
        lmax = std::max(lmax, std::fabs(lam[i]));
    }
    if (evals_h) std::copy(lam.begin(), lam.end(), evals_h);
    // the reference's assertion (ortho.jl:14): min |lambda| > eps max |lambda|; a negative eigenvalue has no square root
    if (!(lmin > 0x1p-52 * lmax) || lam[0] <= 0.0) {
        dftk_set_error("lowdin_ortho: linearly dependent columns, min |lambda| / max |lambda| = %.3e is not above 2^-52 "
                       "(lambda_min = %.3e)", lmax > 0.0 ? lmin / lmax : 0.0, lam[0]);
        return DFTK_MI_NUM_RANK_DEFICIENT;
    }
    for (int i = 0; i < n; ++i) s[i] = 1.0 / std::sqrt(lam[i]);
    HIPCHK(hipMemcpyAsync(d_s, s.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));                    // (s leaves scope with the call)
    hipLaunchKernelGGL(k_scaled_adjoint, dim3((unsigned)(((int64_t)n * n + 255) / 256)), dim3(256), 0, b->stream, n,
                       (const cd*)V, (const double*)d_s, S);
    HIPCHK(hipGetLastError());
    CHK(zgemm(b, 'N', n, n, n, one, V, n, S, n, zero, M, n));   // S^-1/2 = V diag(lambda^-1/2) V'
    for (int64_t r0 = 0; r0 < n_rows; r0 += panel_rows) {
        const int64_t pr = std::min(panel_rows, n_rows - r0);
        CHK(ew_copy(b, pr, n, Phi + r0, ld, Pn, pr));
        CHK(zgemm(b, 'N', pr, n, n, one, Pn, pr, M, n, zero, Phi + r0, ld));
    }
    return 0;
}

extern "C" int dftk_mi_pdos_accumulate(dftk_mi_basis* b, int64_t n_rows, int n_bands, const dftk_mi_cplx* psi_d,
                                       int64_t ld_psi, int n_proj, const dftk_mi_cplx* Phi_d, int64_t ld_phi,
                                       const double* eig_h, double weight, int smearing_kind, double temperature, int n_eps,
                                       const double* eps_h, double* proj_d, double* pdos_d) {
    if (!b || !psi_d || !Phi_d || n_rows < 1 || n_rows > INT32_MAX || n_bands < 1 || n_proj < 1) return DFTK_MI_EINVAL;
    if (ld_psi < n_rows || ld_phi < n_rows) {
        dftk_set_error("pdos_accumulate: leading dimension below n_rows = %lld", (long long)n_rows);
        return DFTK_MI_EINVAL;
    }
    if (!proj_d && !pdos_d) {
        dftk_set_error("pdos_accumulate: neither proj_d nor pdos_d given");
        return DFTK_MI_EINVAL;
    }
    if (pdos_d) {
        if (!(temperature > 0.0) || !std::isfinite(temperature)) {
            dftk_set_error("pdos_accumulate: only finite temperature is supported (temperature = %g)", temperature);
            return DFTK_MI_EINVAL;
        }
        if (smearing_kind != 1 && smearing_kind != 2) {
            dftk_set_error("pdos_accumulate: unknown smearing kind %d (1 = Fermi-Dirac, 2 = Gaussian)", smearing_kind);
            return DFTK_MI_EINVAL;
        }
        if (n_eps < 1 || !eps_h || !eig_h || !std::isfinite(weight)) return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("pdos_accumulate: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    HIPCHK(hipSetDevice(b->device));
    const size_t n_c = (size_t)n_proj * n_bands;
    cd* Cm;
    double *W, *d_eig, *d_eps;
    WsCarver ws;
    ws.take(&Cm, n_c), ws.take(&W, n_c), ws.take(&d_eig, (size_t)n_bands), ws.take(&d_eps, (size_t)std::max(n_eps, 1));
    CHK(scratch_grow(b, b->T1, ws.bytes()));
    ws.bind(b->T1);
    if (pdos_d) {
        HIPCHK(hipMemcpyAsync(d_eig, eig_h, (size_t)n_bands * sizeof(double), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipMemcpyAsync(d_eps, eps_h, (size_t)n_eps * sizeof(double), hipMemcpyHostToDevice, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));                // (the caller's host arrays are free when the call returns)
    }
    const cd one = {1.0, 0.0}, zero = {0.0, 0.0};
    CHK(zgemm(b, 'C', n_proj, n_bands, n_rows, one, reinterpret_cast<const cd*>(Phi_d), ld_phi,
              reinterpret_cast<const cd*>(psi_d), ld_psi, zero, Cm, n_proj));
    hipLaunchKernelGGL(k_abs2, dim3((unsigned)((n_c + 255) / 256)), dim3(256), 0, b->stream, (int64_t)n_c, (const cd*)Cm, W,
                       proj_d);
    HIPCHK(hipGetLastError());
    if (pdos_d) {
        const dim3 grid((unsigned)((n_eps + PD_TE - 1) / PD_TE), (unsigned)((n_proj + PD_TP - 1) / PD_TP));
        if (smearing_kind == 1)
            hipLaunchKernelGGL(k_pdos_tile<1>, grid, dim3(PD_TE), 0, b->stream, n_eps, n_proj, n_bands, (const double*)d_eps,
                               (const double*)d_eig, (const double*)W, temperature, weight, pdos_d);
        else
            hipLaunchKernelGGL(k_pdos_tile<2>, grid, dim3(PD_TE), 0, b->stream, n_eps, n_proj, n_bands, (const double*)d_eps,
                               (const double*)d_eig, (const double*)W, temperature, weight, pdos_d);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
