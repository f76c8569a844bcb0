// response_kernels.hip -- the n_G-sized element-wise kernels of the Sternheimer solver (sternheimer.cpp; reference:
// src/response/cg.jl:58-128).  Every kernel updates ALL active columns in one launch and takes its per-column scalars
// (alpha = gamma / <p, c>, beta = gamma' / gamma) from device memory, so that a CG iteration needs no host round trip
// besides the fetch of the residual norms.
//
// All of them are HBM-bound streams of complex fp64 numbers: one element = one 16-byte access (global_load_dwordx4 /
// global_store_dwordx4), RESP_UNR independent loads per operand and thread in flight before the first use, workgroups of
// 256 threads = 4 waves of 64, grid = (row blocks, columns) with the row blocks capped and a grid-stride loop behind the
// cap.  No reductions here (the column dots and norms are dense_kernels.hip's k_col_reduce): nothing depends on the grid,
// results are bitwise reproducible.
#include "common.h"

namespace dftk_resp {
const int RESP_NT = 256;
const int RESP_UNR = 4;
const int RESP_MAX_ROW_BLOCKS = 2048;

__device__ __forceinline__ double safe_ratio(double num, double den) { return den != 0.0 ? num / den : 0.0; }

// x[:, c] += alpha_c p[:, c];  r[:, c] -= alpha_c c[:, c];  alpha_c = gamma[c] / pc[c]
__global__ __launch_bounds__(RESP_NT) void k_update_xr(int64_t n, const double* __restrict__ gamma,
                                                       const double* __restrict__ pc, const cd* __restrict__ P, int64_t ldp,
                                                       const cd* __restrict__ Cc, int64_t ldc, cd* __restrict__ X,
                                                       int64_t ldx, cd* __restrict__ R, int64_t ldr) {
    const int col = blockIdx.y;
    const double a = safe_ratio(gamma[col], pc[col]);
    const cd* p = P + (int64_t)col * ldp;
    const cd* c = Cc + (int64_t)col * ldc;
    cd* x = X + (int64_t)col * ldx;
    cd* r = R + (int64_t)col * ldr;
    const int64_t step = (int64_t)gridDim.x * RESP_NT * RESP_UNR;
    for (int64_t i0 = (int64_t)blockIdx.x * RESP_NT * RESP_UNR + threadIdx.x; i0 < n; i0 += step) {
        cd pv[RESP_UNR], cv[RESP_UNR], xv[RESP_UNR], rv[RESP_UNR];
#pragma unroll
        for (int u = 0; u < RESP_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * RESP_NT;
            if (i < n) {
                pv[u] = p[i];
                cv[u] = c[i];
                xv[u] = x[i];
                rv[u] = r[i];
            }
        }
#pragma unroll
        for (int u = 0; u < RESP_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * RESP_NT;
            if (i < n) {
                x[i] = make_double2(fma(a, pv[u].x, xv[u].x), fma(a, pv[u].y, xv[u].y));
                r[i] = make_double2(fma(-a, cv[u].x, rv[u].x), fma(-a, cv[u].y, rv[u].y));
            }
        }
    }
}

// p[:, c] = z[:, c] + beta_c p[:, c];  beta_c = gamma_new[c] / gamma_old[c]
__global__ __launch_bounds__(RESP_NT) void k_update_p(int64_t n, const double* __restrict__ gamma_new,
                                                      const double* __restrict__ gamma_old, const cd* __restrict__ Z,
                                                      int64_t ldz, cd* __restrict__ P, int64_t ldp) {
    const int col = blockIdx.y;
    const double bt = safe_ratio(gamma_new[col], gamma_old[col]);
    const cd* z = Z + (int64_t)col * ldz;
    cd* p = P + (int64_t)col * ldp;
    const int64_t step = (int64_t)gridDim.x * RESP_NT * RESP_UNR;
    for (int64_t i0 = (int64_t)blockIdx.x * RESP_NT * RESP_UNR + threadIdx.x; i0 < n; i0 += step) {
        cd zv[RESP_UNR], pv[RESP_UNR];
#pragma unroll
        for (int u = 0; u < RESP_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * RESP_NT;
            if (i < n) {
                zv[u] = z[i];
                pv[u] = p[i];
            }
        }
#pragma unroll
        for (int u = 0; u < RESP_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * RESP_NT;
            if (i < n) p[i] = make_double2(fma(bt, pv[u].x, zv[u].x), fma(bt, pv[u].y, zv[u].y));
        }
    }
}

// Y[:, c] = a s_c X[:, c] + bcoef Y[:, c]  (s_c = sd[c] or 1; bcoef == 0: Y is written only)
__global__ __launch_bounds__(RESP_NT) void k_axpby(int64_t n, double a, const double* __restrict__ sd,
                                                   const cd* __restrict__ X, int64_t ldx, double bcoef, cd* __restrict__ Y,
                                                   int64_t ldy) {
    const int col = blockIdx.y;
    const double as = sd ? a * sd[col] : a;
    const cd* x = X + (int64_t)col * ldx;
    cd* y = Y + (int64_t)col * ldy;
    const int64_t step = (int64_t)gridDim.x * RESP_NT * RESP_UNR;
    for (int64_t i0 = (int64_t)blockIdx.x * RESP_NT * RESP_UNR + threadIdx.x; i0 < n; i0 += step) {
        cd xv[RESP_UNR], yv[RESP_UNR];
#pragma unroll
        for (int u = 0; u < RESP_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * RESP_NT;
            if (i < n) {
                xv[u] = x[i];
                yv[u] = bcoef != 0.0 ? y[i] : make_double2(0.0, 0.0);
            }
        }
#pragma unroll
        for (int u = 0; u < RESP_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * RESP_NT;
            if (i < n) y[i] = make_double2(fma(as, xv[u].x, bcoef * yv[u].x), fma(as, xv[u].y, bcoef * yv[u].y));
        }
    }
}

// S[i, l] /= (ee[i] - e[l]): the inverse of psi_extra' (H - eps_l) psi_extra, diagonal after the Rayleigh-Ritz step
__global__ __launch_bounds__(RESP_NT) void k_scale_inv(int n_extra, int m, cd* __restrict__ S, int64_t lds,
                                                       const double* __restrict__ ee, const double* __restrict__ e) {
    const int idx = blockIdx.x * RESP_NT + threadIdx.x;
    if (idx >= n_extra * m) return;
    const int l = idx / n_extra, i = idx - l * n_extra;
    const double f = 1.0 / (ee[i] - e[l]);
    cd v = S[i + (int64_t)l * lds];
    S[i + (int64_t)l * lds] = make_double2(f * v.x, f * v.y);
}

__global__ __launch_bounds__(RESP_NT) void k_broadcast(int m, const double* __restrict__ src, double* __restrict__ dst) {
    const int i = blockIdx.x * RESP_NT + threadIdx.x;
    if (i < m) dst[i] = src[0];
}

static dim3 col_grid(int64_t n, int m) {
    int64_t rb = (n + (int64_t)RESP_NT * RESP_UNR - 1) / ((int64_t)RESP_NT * RESP_UNR);
    if (rb > RESP_MAX_ROW_BLOCKS) rb = RESP_MAX_ROW_BLOCKS;
    if (rb < 1) rb = 1;
    return dim3((unsigned)rb, (unsigned)m);
}
}   // namespace dftk_resp

using namespace dftk_resp;

int resp_update_xr(dftk_mi_basis* b, int64_t n, int m, const double* gamma_d, const double* pc_d, const cd* p, int64_t ldp,
                   const cd* c, int64_t ldc, cd* x, int64_t ldx, cd* r, int64_t ldr) {
    if (m <= 0 || n <= 0) return 0;
    ProfScope prof_scope(b, PROF_EW, n >= 4096 ? 96.0 * (double)n * m : 0.0);
    hipLaunchKernelGGL(k_update_xr, col_grid(n, m), dim3(RESP_NT), 0, b->stream, n, gamma_d, pc_d, p, ldp, c, ldc, x, ldx, r,
                       ldr);
    HIPCHK(hipGetLastError());
    return 0;
}

int resp_update_p(dftk_mi_basis* b, int64_t n, int m, const double* gamma_new_d, const double* gamma_old_d, const cd* z,
                  int64_t ldz, cd* p, int64_t ldp) {
    if (m <= 0 || n <= 0) return 0;
    ProfScope prof_scope(b, PROF_EW, n >= 4096 ? 48.0 * (double)n * m : 0.0);
    hipLaunchKernelGGL(k_update_p, col_grid(n, m), dim3(RESP_NT), 0, b->stream, n, gamma_new_d, gamma_old_d, z, ldz, p, ldp);
    HIPCHK(hipGetLastError());
    return 0;
}

int resp_axpby(dftk_mi_basis* b, int64_t n, int m, double a, const double* sd, const cd* X, int64_t ldx, double bcoef, cd* Y,
               int64_t ldy) {
    if (m <= 0 || n <= 0) return 0;
    ProfScope prof_scope(b, PROF_EW, n >= 4096 ? (bcoef != 0.0 ? 48.0 : 32.0) * (double)n * m : 0.0);
    hipLaunchKernelGGL(k_axpby, col_grid(n, m), dim3(RESP_NT), 0, b->stream, n, a, sd, X, ldx, bcoef, Y, ldy);
    HIPCHK(hipGetLastError());
    return 0;
}

int resp_scale_inv(dftk_mi_basis* b, int n_extra, int m, cd* S, int64_t lds, const double* ee_d, const double* e_d) {
    if (n_extra <= 0 || m <= 0) return 0;
    const int total = n_extra * m;
    hipLaunchKernelGGL(k_scale_inv, dim3((unsigned)((total + RESP_NT - 1) / RESP_NT)), dim3(RESP_NT), 0, b->stream, n_extra,
                       m, S, lds, ee_d, e_d);
    HIPCHK(hipGetLastError());
    return 0;
}

int resp_broadcast(dftk_mi_basis* b, int m, const double* src_d, double* dst_d) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_broadcast, dim3((unsigned)((m + RESP_NT - 1) / RESP_NT)), dim3(RESP_NT), 0, b->stream, m, src_d,
                       dst_d);
    HIPCHK(hipGetLastError());
    return 0;
}
