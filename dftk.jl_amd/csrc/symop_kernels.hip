// symop_kernels.hip -- a symmetry operation applied to the orbitals of a k-block (reference: apply_symop,
// src/symmetry.jl:229-270).
//
//   dftk_mi_apply_symop   u_{Sk}(G) = e^{-2 pi i (G + kshift).tau} u_k(S^-1 (G + kshift)) for all bands of one k-block in ONE
//       launch.  A GATHER over the rows of the OUTPUT sphere, like dftk_mi_transfer_blochwave: row r reads its integer G from
//       the block's G table (d_G3), adds kshift, multiplies by S^-1 and looks the row of the input block up in that block's
//       inverse cube -> row map (d_inv, the map the transfer entry builds and keeps).  The phase is computed once per row
//       (sincospi of -2 (G + kshift).tau) and multiplied into TR_BANDS columns; with tau = 0 the numbers are moved, not
//       multiplied.  Every output entry is written exactly once by one thread: no atomics, bit-for-bit reproducible.
//       A row whose pre-image lies outside the input cube or sphere means that the operation is not a symmetry of this
//       discretisation (the reference asserts): found on the HOST, one pass over the output rows per (input block, S^-1,
//       kshift), remembered on the output block -- DFTK_MI_EINVAL and nothing written.
//
// Streams: as in transfer_kernels.hip -- the kernel runs on the stream of the output block's basis after a device-side wait
// for the stream of the input block's basis, which in turn waits for the kernel.
#include "common.h"
#include "batch.h"
#include "hgh_forms.h"      // signed_freq
#include <cmath>
#include <cstring>
#include <vector>

namespace dftk_symop {
const int SY_NT = 256;         // rows per workgroup (one thread per output row)
const int SY_BANDS = 8;        // columns a thread writes after one look-up and one phase

using dftk_transfer::cube_index;      // (common.h)

struct SymArgs {               // by value: S^-1 column-major, kshift, tau
    int invS[9];
    int kshift[3];
    double tau[3];
    int has_tau;
};

// cube index on the input grid of S^-1 (G + kshift)
__host__ __device__ inline int64_t preimage(const SymArgs& a, int g0, int g1, int g2, int nx, int ny, int nz) {
    const int f0 = g0 + a.kshift[0], f1 = g1 + a.kshift[1], f2 = g2 + a.kshift[2];
    return cube_index(a.invS[0] * f0 + a.invS[3] * f1 + a.invS[6] * f2, a.invS[1] * f0 + a.invS[4] * f1 + a.invS[7] * f2,
                      a.invS[2] * f0 + a.invS[5] * f1 + a.invS[8] * f2, nx, ny, nz);
}

__global__ __launch_bounds__(SY_NT) void k_apply_symop(int64_t n_out, const int32_t* __restrict__ G3_out, SymArgs a,
                                                       int nx_in, int ny_in, int nz_in, int64_t n_in,
                                                       const int32_t* __restrict__ inv_in, int n_bands,
                                                       const cd* __restrict__ in, int64_t ld_in, cd* __restrict__ out,
                                                       int64_t ld_out) {
    const int64_t r = (int64_t)blockIdx.x * SY_NT + threadIdx.x;
    if (r >= n_out) return;
    const int g0 = G3_out[3 * r], g1 = G3_out[3 * r + 1], g2 = G3_out[3 * r + 2];
    const int64_t lin = preimage(a, g0, g1, g2, nx_in, ny_in, nz_in);
    int64_t src = lin >= 0 ? (int64_t)inv_in[lin] : -1;
    if (src >= n_in) src = -1;          // (the host pass has refused such a call; never read out of bounds)
    double c = 1.0, s = 0.0;
    if (a.has_tau)
        sincospi(-2.0 * ((g0 + a.kshift[0]) * a.tau[0] + (g1 + a.kshift[1]) * a.tau[1] + (g2 + a.kshift[2]) * a.tau[2]), &s, &c);
    const int c0 = blockIdx.y * SY_BANDS;
    cd v[SY_BANDS];
#pragma unroll
    for (int u = 0; u < SY_BANDS; ++u)
        v[u] = (src >= 0 && c0 + u < n_bands) ? in[src + (int64_t)(c0 + u) * ld_in] : make_double2(0.0, 0.0);
#pragma unroll
    for (int u = 0; u < SY_BANDS; ++u)
        if (c0 + u < n_bands)
            out[r + (int64_t)(c0 + u) * ld_out] = a.has_tau ? make_double2(c * v[u].x - s * v[u].y, c * v[u].y + s * v[u].x) : v[u];
}

// every output row must have its pre-image in the input sphere; one host pass per (input block, S^-1, kshift), remembered
int check_symmetry(dftk_mi_kblock* kb_in, dftk_mi_kblock* kb_out, const SymArgs& a) {
    int key[12];
    std::memcpy(key, a.invS, sizeof(a.invS));
    std::memcpy(key + 9, a.kshift, sizeof(a.kshift));
    if (kb_out->symop_in_serial == kb_in->serial && std::memcmp(kb_out->symop_key, key, sizeof(key)) == 0) return 0;
    const int* S = a.invS;
    const int det = S[0] * (S[4] * S[8] - S[7] * S[5]) - S[3] * (S[1] * S[8] - S[7] * S[2]) + S[6] * (S[1] * S[5] - S[4] * S[2]);
    if (det != 1 && det != -1) {
        dftk_set_error("apply_symop: det S^-1 = %d, not +-1", det);
        return DFTK_MI_EINVAL;
    }
    const dftk_mi_basis *bi = kb_in->basis, *bo = kb_out->basis;
    std::vector<int32_t> inv;
    CHK(dftk_transfer::inverse_map_host(kb_in, &inv));
    if (kb_out->h_mapping.empty()) return DFTK_MI_EINVAL;
    for (int64_t r = 0; r < kb_out->n_G; ++r) {
        const int64_t lo = kb_out->h_mapping[r];
        const int ix = (int)(lo % bo->nx), iy = (int)((lo / bo->nx) % bo->ny), iz = (int)(lo / ((int64_t)bo->nx * bo->ny));
        const int g0 = signed_freq(ix, bo->nx), g1 = signed_freq(iy, bo->ny), g2 = signed_freq(iz, bo->nz);
        const int64_t lin = preimage(a, g0, g1, g2, bi->nx, bi->ny, bi->nz);
        if (lin < 0 || inv[(size_t)lin] < 0) {
            dftk_set_error("apply_symop: the plane wave G = (%d, %d, %d) of the output block has no pre-image in the input "
                           "block: the operation is not a symmetry of this discretisation", g0, g1, g2);
            return DFTK_MI_EINVAL;
        }
    }
    kb_out->symop_in_serial = kb_in->serial;
    std::memcpy(kb_out->symop_key, key, sizeof(key));
    return 0;
}
}   // namespace dftk_symop
using namespace dftk_symop;

extern "C" int dftk_mi_apply_symop(dftk_mi_kblock* kb_in, dftk_mi_kblock* kb_out, const int* invS_h, const int* kshift_h,
                                   const double* tau_h, int n_bands, const dftk_mi_cplx* in_d, int64_t ld_in,
                                   dftk_mi_cplx* out_d, int64_t ld_out) {
    if (!kb_in || !kb_out || !invS_h || !kshift_h || !tau_h || n_bands < 0) return DFTK_MI_EINVAL;
    if (kb_in->sh_comm || kb_out->sh_comm) {
        dftk_set_error("apply_symop: plane-wave sharded k-blocks are not supported");
        return DFTK_MI_EINVAL;
    }
    if (kb_in->device != kb_out->device) {
        dftk_set_error("apply_symop: the two blocks live on different devices");
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("apply_symop: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    if (ld_in < kb_in->n_G || ld_out < kb_out->n_G || (n_bands > 0 && (!in_d || !out_d))) {
        dftk_set_error("apply_symop: null block or leading dimension below the rows of its sphere (%lld in, %lld out)",
                       (long long)kb_in->n_G, (long long)kb_out->n_G);
        return DFTK_MI_EINVAL;
    }
    SymArgs a;
    for (int i = 0; i < 9; ++i) a.invS[i] = invS_h[i];
    for (int i = 0; i < 3; ++i) {
        a.kshift[i] = kshift_h[i];
        a.tau[i] = tau_h[i];
        if (!std::isfinite(tau_h[i])) return DFTK_MI_EINVAL;
    }
    a.has_tau = (a.tau[0] != 0.0 || a.tau[1] != 0.0 || a.tau[2] != 0.0) ? 1 : 0;
    dftk_mi_basis *bi = kb_in->basis, *bo = kb_out->basis;
    HIPCHK(hipSetDevice(bo->device));
    CHK(check_symmetry(kb_in, kb_out, a));
    CHK(dftk_transfer::ensure_inverse_map(kb_in));
    CHK(ensure_G3(kb_out));
    if (n_bands == 0) return 0;
    CHK(dftk_transfer::order_after(bo, bi));
    {
        ProfScope prof_scope(bo, PROF_EW, kb_out->n_G >= 4096 ? 32.0 * (double)kb_out->n_G * n_bands : 0.0);
        const dim3 grid((unsigned)((kb_out->n_G + SY_NT - 1) / SY_NT), (unsigned)((n_bands + SY_BANDS - 1) / SY_BANDS));
        hipLaunchKernelGGL(k_apply_symop, grid, dim3(SY_NT), 0, bo->stream, kb_out->n_G, kb_out->d_G3.get(), a, bi->nx, bi->ny,
                           bi->nz, kb_in->n_G, kb_in->d_inv.get(), n_bands, reinterpret_cast<const cd*>(in_d), ld_in,
                           reinterpret_cast<cd*>(out_d), ld_out);
        HIPCHK(hipGetLastError());
    }
    return dftk_transfer::order_after(bi, bo);
}
