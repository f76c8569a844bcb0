// hubbard_kernels.hip -- the device side of DFT+U (src/terms/hubbard.jl:149-228) (gfx950 only).
//
// dftk_mi_hubbard_occupation: C = Phi' psi (one zgemm into basis scratch), then per block b of s <= 7 consecutive orbitals
//     n_b[m1, m2] += sum_n w_n C[p0 + m1, n] conj(C[p0 + m2, n])
// by k_hubbard_occ: one workgroup of HB_NT threads (four waves of 64 lanes) per block.  The block matrix is formed one row m1
// at a time: a thread strides over the bands n = t, t + HB_NT, ... (any n_bands: the tail threads simply run out) and keeps
// the 7 complex partial sums of the row in registers, 14 doubles, so the kernel never holds the 49 of the whole block.  The
// partial sums are added by block_reduce<14> of common.h: LDS as sh[k][t], k = 0 .. 13 (for a fixed k the 64 lanes of a wave
// read 64 consecutive doubles: no bank conflicts within a 32-lane half), a tree with halving strides 128, 64, ..., 1, in an
// order that depends on nothing but the workgroup size; thread 0 adds the row to the output.  No atomics: two calls give
// bitwise equal results.  C is re-read once per row, s times in all; it is n_proj x n_bands and lives in L2.
//
// dftk_mi_hubbard_rotate: Out[:, p0 + j] = sum_m Phi[:, p0 + m] V_b[m, j], a thread per row of a block, V_b staged in LDS
// (every lane reads the same entry: a broadcast).
#include "common.h"
#include "batch.h"
#include <algorithm>
#include <utility>
#include <vector>

namespace {

constexpr int HB_NT = 256;   // threads per workgroup (what block_reduce of common.h is written for)
constexpr int HB_S = 7;      // largest block: 2 l + 1 for l = 3

__global__ __launch_bounds__(HB_NT) void k_hubbard_occ(int n_proj, int n_bands, const cd* __restrict__ Cm,
                                                       const double* __restrict__ w, const int* __restrict__ first,
                                                       const int* __restrict__ size, const int* __restrict__ offset,
                                                       cd* __restrict__ n_d) {
    const int t = threadIdx.x;
    const int p0 = first[blockIdx.x], s = size[blockIdx.x];
    cd* out = n_d + offset[blockIdx.x];
    for (int m1 = 0; m1 < s; ++m1) {
        double acc[2 * HB_S];
#pragma unroll
        for (int k = 0; k < 2 * HB_S; ++k) acc[k] = 0.0;
        for (int n = t; n < n_bands; n += HB_NT) {
            const cd* col = Cm + (int64_t)n_proj * n + p0;
            const double wn = w[n];
            const cd a = col[m1];
            const double ax = wn * a.x, ay = wn * a.y;
#pragma unroll
            for (int m2 = 0; m2 < HB_S; ++m2) {
                if (m2 < s) {
                    const cd c = col[m2];                       // (w a) conj(c)
                    acc[2 * m2] += ax * c.x + ay * c.y;
                    acc[2 * m2 + 1] += ay * c.x - ax * c.y;
                }
            }
        }
        block_reduce<2 * HB_S>(acc);                            // (ends with a barrier; the totals are thread 0's acc)
        if (t == 0) {
#pragma unroll
            for (int m2 = 0; m2 < HB_S; ++m2) {
                if (m2 < s) {                                   // entry (m1, m2) of the column-major s x s block
                    cd v = out[m1 + s * m2];
                    v.x += acc[2 * m2];
                    v.y += acc[2 * m2 + 1];
                    out[m1 + s * m2] = v;
                }
            }
        }
    }
}

__global__ __launch_bounds__(HB_NT) void k_hubbard_rotate(int64_t n_rows, const int* __restrict__ first,
                                                          const int* __restrict__ size, const int* __restrict__ offset,
                                                          const cd* __restrict__ Phi, int64_t ld_phi,
                                                          const cd* __restrict__ V, cd* __restrict__ Out, int64_t ld_out) {
    __shared__ cd sv[HB_S * HB_S];
    const int p0 = first[blockIdx.y], s = size[blockIdx.y];
    if ((int)threadIdx.x < s * s) sv[threadIdx.x] = V[offset[blockIdx.y] + threadIdx.x];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * HB_NT + threadIdx.x;
    if (r >= n_rows) return;
    cd x[HB_S];
#pragma unroll
    for (int m = 0; m < HB_S; ++m) x[m] = m < s ? Phi[r + ld_phi * (p0 + m)] : make_double2(0.0, 0.0);
    for (int j = 0; j < s; ++j) {
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int m = 0; m < HB_S; ++m) {
            if (m < s) {
                const cd v = sv[m + s * j];
                re += x[m].x * v.x - x[m].y * v.y;
                im += x[m].x * v.y + x[m].y * v.x;
            }
        }
        Out[r + ld_out * (p0 + j)] = make_double2(re, im);
    }
}

// the checks both entries share; offsets[b] = sum of size^2 over the blocks before b (n_proj < 0: no upper limit)
int check_blocks(const char* who, int n_proj, int n_blocks, const int* first_h, const int* size_h,
                 std::vector<int>& offsets) {
    if (n_blocks < 1 || !first_h || !size_h) {
        dftk_set_error("%s: needs at least one block", who);
        return DFTK_MI_EINVAL;
    }
    offsets.assign((size_t)n_blocks + 1, 0);
    for (int b = 0; b < n_blocks; ++b) {
        const int p0 = first_h[b], s = size_h[b];
        if (s < 1 || s > HB_S) {
            dftk_set_error("%s: block %d has %d orbitals (1 .. %d are supported: l <= 3)", who, b, s, HB_S);
            return DFTK_MI_EINVAL;
        }
        if (p0 < 0 || p0 > INT32_MAX - s || (n_proj >= 0 && p0 > n_proj - s)) {
            dftk_set_error("%s: block %d = columns [%d, %d) lies outside [0, %d)", who, b, p0, p0 + s, n_proj);
            return DFTK_MI_EINVAL;
        }
        offsets[b + 1] = offsets[b] + s * s;
    }
    return 0;
}

}   // namespace

extern "C" int dftk_mi_hubbard_occupation(dftk_mi_basis* b, int64_t n_rows, int n_bands, const dftk_mi_cplx* psi_d,
                                          int64_t ld_psi, int n_proj, const dftk_mi_cplx* Phi_d, int64_t ld_phi,
                                          const double* w_h, int n_blocks, const int* block_first_h,
                                          const int* block_size_h, dftk_mi_cplx* n_d) {
    if (!b || !psi_d || !Phi_d || !w_h || !n_d || n_rows < 1 || n_rows > INT32_MAX || n_bands < 1 || n_proj < 1) {
        dftk_set_error("hubbard_occupation: needs a basis, the blocks and sizes of at least 1");
        return DFTK_MI_EINVAL;
    }
    if (ld_psi < n_rows || ld_phi < n_rows) {
        dftk_set_error("hubbard_occupation: leading dimension below n_rows = %lld", (long long)n_rows);
        return DFTK_MI_EINVAL;
    }
    std::vector<int> offsets;
    CHK(check_blocks("hubbard_occupation", n_proj, n_blocks, block_first_h, block_size_h, offsets));
    if (batching()) {
        dftk_set_error("hubbard_occupation: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    HIPCHK(hipSetDevice(b->device));
    cd* Cm;
    double* d_w;
    int *d_first, *d_size, *d_off;
    WsCarver ws;
    ws.take(&Cm, (size_t)n_proj * n_bands), ws.take(&d_w, (size_t)n_bands);
    ws.take(&d_first, (size_t)n_blocks), ws.take(&d_size, (size_t)n_blocks), ws.take(&d_off, (size_t)n_blocks);
    CHK(scratch_grow(b, b->T1, ws.bytes()));
    ws.bind(b->T1);
    HIPCHK(hipMemcpyAsync(d_w, w_h, (size_t)n_bands * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_first, block_first_h, (size_t)n_blocks * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_size, block_size_h, (size_t)n_blocks * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_off, offsets.data(), (size_t)n_blocks * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));                    // (the host arrays are free when the call returns)
    const cd one = {1.0, 0.0}, zero = {0.0, 0.0};
    CHK(zgemm(b, 'C', n_proj, n_bands, n_rows, one, reinterpret_cast<const cd*>(Phi_d), ld_phi,
              reinterpret_cast<const cd*>(psi_d), ld_psi, zero, Cm, n_proj));
    hipLaunchKernelGGL(k_hubbard_occ, dim3((unsigned)n_blocks), dim3(HB_NT), 0, b->stream, n_proj, n_bands, (const cd*)Cm,
                       (const double*)d_w, (const int*)d_first, (const int*)d_size, (const int*)d_off,
                       reinterpret_cast<cd*>(n_d));
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int dftk_mi_hubbard_rotate(dftk_mi_basis* b, int64_t n_rows, int n_blocks, const int* block_first_h,
                                      const int* block_size_h, const dftk_mi_cplx* Phi_d, int64_t ld_phi,
                                      const dftk_mi_cplx* V_h, dftk_mi_cplx* Out_d, int64_t ld_out) {
    if (!b || !Phi_d || !V_h || !Out_d || n_rows < 1 || n_rows > INT32_MAX) {
        dftk_set_error("hubbard_rotate: needs a basis, the blocks and sizes of at least 1");
        return DFTK_MI_EINVAL;
    }
    if (ld_phi < n_rows || ld_out < n_rows) {
        dftk_set_error("hubbard_rotate: leading dimension below n_rows = %lld", (long long)n_rows);
        return DFTK_MI_EINVAL;
    }
    std::vector<int> offsets;
    CHK(check_blocks("hubbard_rotate", -1, n_blocks, block_first_h, block_size_h, offsets));
    int n_proj = 0;                                             // the columns the call can touch
    for (int k = 0; k < n_blocks; ++k) n_proj = std::max(n_proj, block_first_h[k] + block_size_h[k]);
    // two blocks that share a column would have two workgroups write it
    std::vector<std::pair<int, int>> spans((size_t)n_blocks);
    for (int k = 0; k < n_blocks; ++k) spans[k] = {block_first_h[k], block_first_h[k] + block_size_h[k]};
    std::sort(spans.begin(), spans.end());
    for (int k = 1; k < n_blocks; ++k)
        if (spans[k].first < spans[k - 1].second) {
            dftk_set_error("hubbard_rotate: the blocks [%d, %d) and [%d, %d) overlap", spans[k - 1].first,
                           spans[k - 1].second, spans[k].first, spans[k].second);
            return DFTK_MI_EINVAL;
        }
    const cd* Phi = reinterpret_cast<const cd*>(Phi_d);
    cd* Out = reinterpret_cast<cd*>(Out_d);
    const cd* phi_end = Phi + ld_phi * (int64_t)(n_proj - 1) + n_rows;
    const cd* out_end = Out + ld_out * (int64_t)(n_proj - 1) + n_rows;
    if (Phi < out_end && Out < phi_end) {
        dftk_set_error("hubbard_rotate: Out_d may not overlap Phi_d");
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("hubbard_rotate: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    HIPCHK(hipSetDevice(b->device));
    cd* d_V;
    int *d_first, *d_size, *d_off;
    WsCarver ws;
    ws.take(&d_V, (size_t)offsets[n_blocks]);
    ws.take(&d_first, (size_t)n_blocks), ws.take(&d_size, (size_t)n_blocks), ws.take(&d_off, (size_t)n_blocks);
    CHK(scratch_grow(b, b->T1, ws.bytes()));
    ws.bind(b->T1);
    HIPCHK(hipMemcpyAsync(d_V, V_h, (size_t)offsets[n_blocks] * sizeof(cd), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_first, block_first_h, (size_t)n_blocks * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_size, block_size_h, (size_t)n_blocks * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_off, offsets.data(), (size_t)n_blocks * sizeof(int), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));                    // (the host arrays are free when the call returns)
    const dim3 grid((unsigned)((n_rows + HB_NT - 1) / HB_NT), (unsigned)n_blocks);
    hipLaunchKernelGGL(k_hubbard_rotate, grid, dim3(HB_NT), 0, b->stream, n_rows, (const int*)d_first, (const int*)d_size,
                       (const int*)d_off, Phi, ld_phi, (const cd*)d_V, Out, ld_out);
    HIPCHK(hipGetLastError());
    return 0;
}
