// exx_kernels.hip -- dftk_mi_exx_apply: the exact-exchange (Fock) operator of one Gamma-point k-block on a block of
// columns, apply!(Hpsi, ::ExchangeOperator, psi) of the reference (src/terms/operators.jl:192-210) with the transforms of
// compress_exchange (src/terms/exact_exchange.jl:136-154) around it:
//
//     W_m (+)= - sum_n w_n FFT[ phi_n(r) IFFT[ K(G) FFT[ conj(phi_n(r)) psi_m(r) ] ] ]
//
// Every transform is the k-block's own pruned sphere <-> cube pipeline (launch_ifft_to_cube / launch_fft_from_cube): the
// pair density is taken on the sphere of the orbitals, as the reference does.  With the library's unnormalised transforms
// the reference's normalisations (ifft: 1 / sqrt(Omega), fft: sqrt(Omega) / N) collect into ONE factor 1 / (N^2 Omega),
// which rides on the weights.
//
// Structure: the psi columns go to cubes in groups of g = fft_group_size(b); for every psi cube the occupied orbitals are
// taken in groups of g:  one launch forms the g pair products (psi(r) loaded once), a batched forward transform, one launch
// multiplies by K on the sphere, a batched backward transform, one launch does acc(r) -= sum_n w_n phi_n(r) V_n(r) for the
// whole group (one writer per entry of acc, no atomics); a last forward transform of the group's acc cubes gives W.
//
// The phi cubes stay in the basis' exchange workspace for the whole call when they fit under EXX_PHI_CACHE_BYTES;
// otherwise every group of them is transformed again for every psi group.  Workspace in complex numbers, with N = nx ny nz,
// g_phi = min(g, n_occ), g_psi = min(g, n_bands), c = n_occ (cached) or g_phi:
//     (c + 2 g_psi + g_phi) N  +  (2 g_phi + g_psi) n_G
//
// The element-wise kernels are HBM-bound streams in the form of response_kernels.hip: 256 threads, grid-stride loop, one
// complex fp64 number per 16-byte access, EXX_UNR independent loads per operand in flight before the first use.
#include "common.h"
#include "batch.h"
#include <algorithm>
#include <cstdlib>
#include <vector>

namespace dftk_exx {
const int EXX_NT = 256;
const int EXX_UNR = 4;
const int EXX_MAX_BLOCKS = 4096;
// the phi cubes of a call are kept for all psi groups while they need no more than this (env DFTK_MI_EXX_PHI_BYTES
// overrides, read at every call: 0 forces the re-transforming path)
const size_t EXX_PHI_CACHE_BYTES = (size_t)8 << 30;

// pair[j][i] = conj(phi[j][i]) psi[i] for the nb cubes of a group (n apart): psi is loaded once
__global__ __launch_bounds__(EXX_NT) void k_exx_pair(int64_t n, int nb, const cd* __restrict__ psi,
                                                     const cd* __restrict__ phi, cd* __restrict__ pair) {
    const int64_t step = (int64_t)gridDim.x * EXX_NT * EXX_UNR;
    for (int64_t i0 = (int64_t)blockIdx.x * EXX_NT * EXX_UNR + threadIdx.x; i0 < n; i0 += step) {
        cd pv[EXX_UNR];
#pragma unroll
        for (int u = 0; u < EXX_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * EXX_NT;
            if (i < n) pv[u] = psi[i];
        }
        for (int j = 0; j < nb; ++j) {
            const cd* f = phi + (int64_t)j * n;
            cd* o = pair + (int64_t)j * n;
            cd fv[EXX_UNR];
#pragma unroll
            for (int u = 0; u < EXX_UNR; ++u) {
                const int64_t i = i0 + (int64_t)u * EXX_NT;
                if (i < n) fv[u] = f[i];
            }
#pragma unroll
            for (int u = 0; u < EXX_UNR; ++u) {
                const int64_t i = i0 + (int64_t)u * EXX_NT;
                if (i < n)
                    o[i] = make_double2(fma(fv[u].x, pv[u].x, fv[u].y * pv[u].y), fma(fv[u].x, pv[u].y, -(fv[u].y * pv[u].x)));
            }
        }
    }
}

// c[:, j] *= K for the nb coefficient vectors of a group (n_G apart); grid = (row blocks, nb)
__global__ __launch_bounds__(EXX_NT) void k_exx_mul_kernel(int64_t n_G, const double* __restrict__ K, cd* __restrict__ c) {
    cd* x = c + (int64_t)blockIdx.y * n_G;
    const int64_t step = (int64_t)gridDim.x * EXX_NT * EXX_UNR;
    for (int64_t i0 = (int64_t)blockIdx.x * EXX_NT * EXX_UNR + threadIdx.x; i0 < n_G; i0 += step) {
        cd xv[EXX_UNR];
        double kv[EXX_UNR];
#pragma unroll
        for (int u = 0; u < EXX_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * EXX_NT;
            if (i < n_G) {
                xv[u] = x[i];
                kv[u] = K[i];
            }
        }
#pragma unroll
        for (int u = 0; u < EXX_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * EXX_NT;
            if (i < n_G) x[i] = make_double2(kv[u] * xv[u].x, kv[u] * xv[u].y);
        }
    }
}

// acc[i] = (first ? 0 : acc[i]) - sum_j w[j] phi[j][i] V[j][i] over the nb cubes of a group: one writer per entry
__global__ __launch_bounds__(EXX_NT) void k_exx_accumulate(int64_t n, int nb, const double* __restrict__ w,
                                                           const cd* __restrict__ phi, const cd* __restrict__ V,
                                                           cd* __restrict__ acc, int first) {
    const int64_t step = (int64_t)gridDim.x * EXX_NT * EXX_UNR;
    for (int64_t i0 = (int64_t)blockIdx.x * EXX_NT * EXX_UNR + threadIdx.x; i0 < n; i0 += step) {
        cd a[EXX_UNR];
#pragma unroll
        for (int u = 0; u < EXX_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * EXX_NT;
            a[u] = (!first && i < n) ? acc[i] : make_double2(0.0, 0.0);
        }
        for (int j = 0; j < nb; ++j) {
            const cd* f = phi + (int64_t)j * n;
            const cd* v = V + (int64_t)j * n;
            const double wj = w[j];
            cd fv[EXX_UNR], vv[EXX_UNR];
#pragma unroll
            for (int u = 0; u < EXX_UNR; ++u) {
                const int64_t i = i0 + (int64_t)u * EXX_NT;
                if (i < n) {
                    fv[u] = f[i];
                    vv[u] = v[i];
                }
            }
#pragma unroll
            for (int u = 0; u < EXX_UNR; ++u) {
                const int64_t i = i0 + (int64_t)u * EXX_NT;
                if (i < n) {
                    a[u].x = fma(-wj, fma(fv[u].x, vv[u].x, -(fv[u].y * vv[u].y)), a[u].x);
                    a[u].y = fma(-wj, fma(fv[u].x, vv[u].y, fv[u].y * vv[u].x), a[u].y);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < EXX_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * EXX_NT;
            if (i < n) acc[i] = a[u];
        }
    }
}

// W[:, c] = (accumulate ? W[:, c] : 0) + src[:, c]; src == null: no addend (zero fill, or nothing to do); grid = (row
// blocks, columns).  Rows beyond n_G of a column (the caller's padding) are neither read nor written.
__global__ __launch_bounds__(EXX_NT) void k_exx_store(int64_t n_G, const cd* __restrict__ src, cd* __restrict__ W, int64_t ldW,
                                                      int accumulate) {
    const cd* s = src ? src + (int64_t)blockIdx.y * n_G : nullptr;
    cd* o = W + (int64_t)blockIdx.y * ldW;
    const int64_t step = (int64_t)gridDim.x * EXX_NT * EXX_UNR;
    for (int64_t i0 = (int64_t)blockIdx.x * EXX_NT * EXX_UNR + threadIdx.x; i0 < n_G; i0 += step) {
        cd sv[EXX_UNR], ov[EXX_UNR];
#pragma unroll
        for (int u = 0; u < EXX_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * EXX_NT;
            sv[u] = (s && i < n_G) ? s[i] : make_double2(0.0, 0.0);
            ov[u] = (accumulate && i < n_G) ? o[i] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < EXX_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * EXX_NT;
            if (i < n_G) o[i] = make_double2(ov[u].x + sv[u].x, ov[u].y + sv[u].y);
        }
    }
}

static unsigned row_blocks(int64_t n) {
    int64_t rb = (n + (int64_t)EXX_NT * EXX_UNR - 1) / ((int64_t)EXX_NT * EXX_UNR);
    return (unsigned)std::min<int64_t>(std::max<int64_t>(rb, 1), EXX_MAX_BLOCKS);
}

static size_t phi_cache_cap() {
    const char* e = getenv("DFTK_MI_EXX_PHI_BYTES");
    return e ? (size_t)strtoull(e, nullptr, 10) : EXX_PHI_CACHE_BYTES;
}

struct Exx {
    dftk_mi_kblock* kb;
    dftk_mi_basis* b;
    int64_t N, n_G;
    cd *phi_cubes, *psi_cubes, *acc_cubes, *pair_cubes, *coef, *wout, *stage;
    double* w_d;

    // columns cols[0 .. m) of X as m vectors n_G apart: X itself where they are adjacent and unpadded, else copies in `stage`
    int packed(const cd* X, int64_t ldx, const int* cols, int m, const cd** out) {
        bool adjacent = ldx == n_G;
        for (int j = 1; j < m && adjacent; ++j) adjacent = cols[j] == cols[j - 1] + 1;
        if (adjacent) {
            *out = X + (int64_t)cols[0] * ldx;
            return 0;
        }
        for (int j = 0; j < m;) {     // one copy per run of adjacent columns
            int r = 1;
            while (j + r < m && cols[j + r] == cols[j] + r) ++r;
            CHK(ew_copy(b, n_G, r, X + (int64_t)cols[j] * ldx, ldx, stage + (int64_t)j * n_G, n_G));
            j += r;
        }
        *out = stage;
        return 0;
    }
    int to_cubes(const cd* X, int64_t ldx, const int* cols, int m, cd* cubes) {
        const cd* c = nullptr;
        CHK(packed(X, ldx, cols, m, &c));
        return launch_ifft_to_cube(kb, c, cubes, m);
    }
};
}   // namespace dftk_exx

using namespace dftk_exx;

static int exx_store(dftk_mi_basis* b, int64_t n_G, int m, const cd* src, cd* W, int64_t ldW, int accumulate) {
    if (m <= 0 || n_G <= 0 || (!src && accumulate)) return 0;
    hipLaunchKernelGGL(k_exx_store, dim3(row_blocks(n_G), (unsigned)m), dim3(EXX_NT), 0, b->stream, n_G, src, W, ldW,
                       accumulate);
    HIPCHK(hipGetLastError());
    return 0;
}

static int exx_apply(dftk_mi_kblock* kb, int n_occ, const cd* phi, int64_t ld_phi, const double* weight_h,
                     const double* kernel_d, int n_bands, const cd* psi, int64_t ld_psi, cd* W, int64_t ld_W, int accumulate) {
    dftk_mi_basis* b = kb->basis;
    Exx x;
    x.kb = kb;
    x.b = b;
    x.N = (int64_t)b->nx * b->ny * b->nz;
    x.n_G = kb->n_G;
    const int64_t N = x.N, n_G = x.n_G;

    // the orbitals that contribute, and their weights with the transforms' normalisation 1 / (N^2 Omega) folded in
    std::vector<int> act;
    std::vector<double> w_act;
    const double scale = 1.0 / ((double)N * (double)N * b->volume);
    for (int n = 0; n < n_occ; ++n)
        if (weight_h[n] != 0.0) {
            act.push_back(n);
            w_act.push_back(weight_h[n] * scale);
        }
    const int n_act = (int)act.size();
    if (n_act == 0) return exx_store(b, n_G, n_bands, nullptr, W, ld_W, accumulate);

    const int g = fft_group_size(b);
    const int g_phi = std::min(g, n_act), g_psi = std::min(g, n_bands);
    const bool cached = (size_t)n_act * (size_t)N * sizeof(cd) <= phi_cache_cap();
    WsCarver ws;
    ws.take(&x.phi_cubes, (size_t)(cached ? n_act : g_phi) * N);
    ws.take(&x.psi_cubes, (size_t)g_psi * N);
    ws.take(&x.acc_cubes, (size_t)g_psi * N);
    ws.take(&x.pair_cubes, (size_t)g_phi * N);
    ws.take(&x.coef, (size_t)g_phi * n_G);
    ws.take(&x.wout, (size_t)g_psi * n_G);
    ws.take(&x.stage, (size_t)std::max(g_phi, g_psi) * n_G);
    ws.take(&x.w_d, (size_t)n_act);
    CHK(scratch_grow(b, b->exx_ws, ws.bytes()));
    ws.bind(b->exx_ws);
    // (from the caller's pageable array: staged by the runtime before the call returns)
    HIPCHK(hipMemcpyAsync(x.w_d, w_act.data(), (size_t)n_act * sizeof(double), hipMemcpyHostToDevice, b->stream));

    if (cached)
        for (int n0 = 0; n0 < n_act; n0 += g_phi)
            CHK(x.to_cubes(phi, ld_phi, act.data() + n0, std::min(g_phi, n_act - n0), x.phi_cubes + (int64_t)n0 * N));

    std::vector<int> cols(g_psi);
    const unsigned cube_blocks = row_blocks(N);
    for (int m0 = 0; m0 < n_bands; m0 += g_psi) {
        const int gm = std::min(g_psi, n_bands - m0);
        for (int m = 0; m < gm; ++m) cols[m] = m0 + m;
        CHK(x.to_cubes(psi, ld_psi, cols.data(), gm, x.psi_cubes));
        for (int n0 = 0; n0 < n_act; n0 += g_phi) {
            const int gn = std::min(g_phi, n_act - n0);
            const cd* phi_g = x.phi_cubes + (cached ? (int64_t)n0 * N : 0);
            if (!cached) CHK(x.to_cubes(phi, ld_phi, act.data() + n0, gn, x.phi_cubes));
            for (int m = 0; m < gm; ++m) {
                hipLaunchKernelGGL(k_exx_pair, dim3(cube_blocks), dim3(EXX_NT), 0, b->stream, N, gn,
                                   (const cd*)(x.psi_cubes + (int64_t)m * N), phi_g, x.pair_cubes);
                CHK(launch_fft_from_cube(kb, x.pair_cubes, x.coef, gn));
                hipLaunchKernelGGL(k_exx_mul_kernel, dim3(row_blocks(n_G), (unsigned)gn), dim3(EXX_NT), 0, b->stream, n_G,
                                   kernel_d, x.coef);
                CHK(launch_ifft_to_cube(kb, x.coef, x.pair_cubes, gn));
                hipLaunchKernelGGL(k_exx_accumulate, dim3(cube_blocks), dim3(EXX_NT), 0, b->stream, N, gn,
                                   (const double*)(x.w_d + n0), phi_g, (const cd*)x.pair_cubes,
                                   x.acc_cubes + (int64_t)m * N, n0 == 0 ? 1 : 0);
            }
        }
        CHK(launch_fft_from_cube(kb, x.acc_cubes, x.wout, gm));
        CHK(exx_store(b, n_G, gm, x.wout, W + (int64_t)m0 * ld_W, ld_W, accumulate));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int dftk_mi_exx_apply(dftk_mi_kblock* kb, int n_occ, const dftk_mi_cplx* phi_d, int64_t ld_phi,
                                 const double* weight_h, const double* kernel_d, int n_bands, const dftk_mi_cplx* psi_d,
                                 int64_t ld_psi, dftk_mi_cplx* W_d, int64_t ld_W, int accumulate) {
    if (!kb || n_occ < 0 || n_bands < 0) {
        dftk_set_error("exx_apply: null k-block or negative count");
        return DFTK_MI_EINVAL;
    }
    if (kb->gr && kb->gr->on) {
        dftk_set_error("exx_apply: Gamma-real k-blocks are not supported (the pair densities are not real-symmetric)");
        return DFTK_MI_EINVAL;
    }
    if (kb->sh_comm) {
        dftk_set_error("exx_apply: plane-wave sharded k-blocks are not supported");
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("exx_apply: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    const int64_t n = kb->n_G;
    if ((n_occ > 0 && (!phi_d || !weight_h || !kernel_d)) || (n_bands > 0 && (!psi_d || !W_d))) {
        dftk_set_error("exx_apply: null pointer argument");
        return DFTK_MI_EINVAL;
    }
    if ((n_occ > 0 && ld_phi < n) || (n_bands > 0 && (ld_psi < n || ld_W < n))) {
        dftk_set_error("exx_apply: leading dimension below n_G = %lld", (long long)n);
        return DFTK_MI_EINVAL;
    }
    if (n_bands == 0) return 0;
    HIPCHK(hipSetDevice(kb->basis->device));
    return exx_apply(kb, n_occ, reinterpret_cast<const cd*>(phi_d), ld_phi, weight_h, kernel_d, n_bands,
                     reinterpret_cast<const cd*>(psi_d), ld_psi, reinterpret_cast<cd*>(W_d), ld_W, accumulate);
}
