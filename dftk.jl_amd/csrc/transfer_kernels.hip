// transfer_kernels.hip -- moving orbital blocks and densities between two plane-wave bases of the same lattice
// (reference: src/transfer.jl:10-178).
//
//   dftk_mi_transfer_blochwave   transfer_blochwave_kpt (transfer.jl:46-124): the coefficient of plane wave G of the input
//       block lands in the row of the output block that carries G - dG, dG = k_out - k_in.  Written as a GATHER over the
//       rows of the OUTPUT sphere: row r reads its integer G from the block's G table (d_G3), adds dG and looks the partner
//       row up in the inverse cube -> row map of the input block (d_inv, built once per block and kept with it on the
//       device).  A row without a partner -- G + dG outside the input cube or outside the input sphere -- is written as zero; input rows
//       whose plane wave the output sphere lacks are never read.  Every output entry is written exactly once by one thread:
//       no atomics, no dependence on the grid, bit-for-bit reproducible, and the numbers are moved, not recomputed.
//       One launch for all bands: a thread finds the partner of its row once and then walks TR_BANDS columns; consecutive
//       threads take consecutive rows, so the stores are contiguous 16-byte accesses and the loads nearly so (partners of
//       neighbouring sphere rows are neighbours except at the ends of an x-line).
//   dftk_mi_transfer_density     transfer_density (transfer.jl:165-178): forward cube FFT on the input grid, the eight index
//       blocks of transfer_mapping(basis_in, basis_out) (transfer.jl:10-31) as a gather over the OUTPUT cube, inverse cube FFT
//       on the output grid.  In terms of the signed frequency g of an index (fft.jl:24-31: [0 .. (n-1)/2, -ceil((n-1)/2) ..
//       -1]) the eight blocks say: per axis, output index and input index with the SAME g correspond, over the range of g of
//       the shorter axis; everything else of the output is zero.  The unmatched plane g = -n/2 of an even shorter axis is
//       therefore carried along with g = -n/2 (its partner +n/2 on the longer axis stays zero), exactly as the index blocks do.
//
// Two bases, two streams.  The blocks of one call may belong to two basis handles of the same device, each with its own HIP
// stream.  The kernels that write the output run on the stream of the OUTPUT basis.  Before them that stream waits for an
// event recorded on the input basis' stream (whatever produced the input there is complete), and after them the input basis'
// stream waits for an event recorded on the output basis' stream (nothing queued later on the input side can overwrite the
// input, or the input side's scratch, while it is still read).  Both waits are device-side: the host does not block.  With
// one handle on both sides there is one stream and no event.
#include "common.h"
#include "batch.h"
#include "hgh_forms.h"
#include <cmath>
#include <vector>

int cube_forward_real(dftk_mi_kblock* cube_kb, const double* f, const double* g, cd* tmp, cd* c_out);     // cube_kernels.hip
int cube_backward_real(dftk_mi_kblock* cube_kb, const cd* c, cd* tmp, double scale, double* out);

namespace dftk_transfer {
const int TR_NT = 256;         // rows per workgroup (one thread per output row)
const int TR_BANDS = 8;        // columns a thread writes after one partner look-up

// (freq_on_axis / freq_index / cube_index: common.h, shared with symop_kernels.hip and wannier_kernels.hip)

__global__ __launch_bounds__(TR_NT) void k_transfer_blochwave(int64_t n_out, const int32_t* __restrict__ G3_out, int d0,
                                                              int d1, int d2, int nx_in, int ny_in, int nz_in,
                                                              const int32_t* __restrict__ inv_in, int n_bands,
                                                              const cd* __restrict__ in, int64_t ld_in,
                                                              cd* __restrict__ out, int64_t ld_out) {
    const int64_t r = (int64_t)blockIdx.x * TR_NT + threadIdx.x;
    if (r >= n_out) return;
    const int64_t lin = cube_index(G3_out[3 * r] + d0, G3_out[3 * r + 1] + d1, G3_out[3 * r + 2] + d2, nx_in, ny_in, nz_in);
    const int64_t src = lin >= 0 ? (int64_t)inv_in[lin] : -1;
    const int c0 = blockIdx.y * TR_BANDS;
    cd v[TR_BANDS];
#pragma unroll
    for (int u = 0; u < TR_BANDS; ++u)
        v[u] = (src >= 0 && c0 + u < n_bands) ? in[src + (int64_t)(c0 + u) * ld_in] : make_double2(0.0, 0.0);
#pragma unroll
    for (int u = 0; u < TR_BANDS; ++u)
        if (c0 + u < n_bands) out[r + (int64_t)(c0 + u) * ld_out] = v[u];
}

// c_out[i] = c_in[index of the same signed frequency on the input grid], 0 where the input grid has none
__global__ __launch_bounds__(256) void k_transfer_cube(int nx_o, int ny_o, int nz_o, int nx_i, int ny_i, int nz_i,
                                                       const cd* __restrict__ c_in, cd* __restrict__ c_out) {
    const int64_t N = (int64_t)nx_o * ny_o * nz_o;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const int ix = (int)(i % nx_o), iy = (int)((i / nx_o) % ny_o), iz = (int)(i / ((int64_t)nx_o * ny_o));
        const int64_t src = cube_index(signed_freq(ix, nx_o), signed_freq(iy, ny_o), signed_freq(iz, nz_o), nx_i, ny_i, nz_i);
        c_out[i] = src >= 0 ? c_in[src] : make_double2(0.0, 0.0);
    }
}

// the stream of `waiter` goes on only after everything queued so far on the stream of `producer` is complete (device-side
// wait).  The event is the producer's own, created once; recording it again later does not disturb a wait already queued
// (a wait refers to the record that preceded it).
int order_after(dftk_mi_basis* waiter, dftk_mi_basis* producer) {
    if (waiter == producer || waiter->stream.s == producer->stream.s) return 0;
    if (!producer->order_ev.e) HIPCHK(hipEventCreateWithFlags(&producer->order_ev.e, hipEventDisableTiming));
    HIPCHK(hipEventRecord(producer->order_ev.e, producer->stream));
    HIPCHK(hipStreamWaitEvent(waiter->stream, producer->order_ev.e, 0));
    return 0;
}

// sphere row of every cube index of the block's grid (-1: none), on the host
int inverse_map_host(const dftk_mi_kblock* kb, std::vector<int32_t>* inv) {
    const dftk_mi_basis* b = kb->basis;
    if (kb->h_mapping.empty()) return DFTK_MI_EINVAL;
    const int64_t N = (int64_t)b->nx * b->ny * b->nz;
    inv->assign((size_t)N, -1);
    for (int64_t r = 0; r < kb->n_G; ++r) {
        const int64_t lin = kb->h_mapping[r];
        if (lin < 0 || lin >= N) return DFTK_MI_EINVAL;
        (*inv)[(size_t)lin] = (int32_t)r;
    }
    return 0;
}

// kb->d_inv, built on first use (the host copy is a temporary)
int ensure_inverse_map(dftk_mi_kblock* kb) {
    if (kb->d_inv) return 0;
    std::vector<int32_t> inv;
    CHK(inverse_map_host(kb, &inv));
    HIPCHK(kb->d_inv.alloc(inv.size() * sizeof(int32_t)));
    HIPCHK(hipMemcpy(kb->d_inv, inv.data(), inv.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

// dG = k_out - k_in has to fit the two blocks: partners carry the same k + G, hence the same kinetic energy.  Checked on the
// host once per (input block, dG) and remembered on the output block.
int check_dG(dftk_mi_kblock* kb_in, dftk_mi_kblock* kb_out, const int* dG) {
    if (!(kb_in->kin_given && kb_out->kin_given)) return 0;
    if (kb_out->transfer_in_serial == kb_in->serial && kb_out->transfer_dG[0] == dG[0] && kb_out->transfer_dG[1] == dG[1] &&
        kb_out->transfer_dG[2] == dG[2])
        return 0;
    const dftk_mi_basis *bi = kb_in->basis, *bo = kb_out->basis;
    std::vector<int32_t> inv;
    CHK(inverse_map_host(kb_in, &inv));
    for (int64_t r = 0; r < kb_out->n_G; ++r) {
        const int64_t lo = kb_out->h_mapping[r];
        const int ix = (int)(lo % bo->nx), iy = (int)((lo / bo->nx) % bo->ny), iz = (int)(lo / ((int64_t)bo->nx * bo->ny));
        const int64_t lin = cube_index(signed_freq(ix, bo->nx) + dG[0], signed_freq(iy, bo->ny) + dG[1],
                                       signed_freq(iz, bo->nz) + dG[2], bi->nx, bi->ny, bi->nz);
        const int32_t src = lin >= 0 ? inv[(size_t)lin] : -1;
        if (src < 0) continue;
        const double a = kb_out->h_kin[r], c = kb_in->h_kin[src];
        if (std::fabs(a - c) > 1e-10 * (1.0 + std::fabs(a) + std::fabs(c))) {
            dftk_set_error("transfer_blochwave: dG = (%d, %d, %d) does not match the blocks (kinetic energies %.17g and "
                           "%.17g of one plane wave: other lattice, or dG is not k_out - k_in)", dG[0], dG[1], dG[2], c, a);
            return DFTK_MI_EINVAL;
        }
    }
    kb_out->transfer_in_serial = kb_in->serial;
    for (int i = 0; i < 3; ++i) kb_out->transfer_dG[i] = dG[i];
    return 0;
}

bool is_full_cube(const dftk_mi_kblock* kb) {
    const dftk_mi_basis* b = kb->basis;
    return kb->n_G == (int64_t)b->nx * b->ny * b->nz;
}
}   // namespace dftk_transfer
using namespace dftk_transfer;

extern "C" int dftk_mi_transfer_blochwave(dftk_mi_kblock* kb_in, dftk_mi_kblock* kb_out, const int* dG_h, int n_bands,
                                          const dftk_mi_cplx* in_d, int64_t ld_in, dftk_mi_cplx* out_d, int64_t ld_out) {
    if (!kb_in || !kb_out || !dG_h || n_bands < 0) return DFTK_MI_EINVAL;
    if (kb_in->sh_comm || kb_out->sh_comm) {
        dftk_set_error("transfer_blochwave: plane-wave sharded k-blocks are not supported");
        return DFTK_MI_EINVAL;
    }
    if (kb_in->device != kb_out->device) {
        dftk_set_error("transfer_blochwave: the two blocks live on different devices");
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("transfer_blochwave: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    if (ld_in < kb_in->n_G || ld_out < kb_out->n_G || (n_bands > 0 && (!in_d || !out_d))) {
        dftk_set_error("transfer_blochwave: null block or leading dimension below the rows of its sphere (%lld in, %lld out)",
                       (long long)kb_in->n_G, (long long)kb_out->n_G);
        return DFTK_MI_EINVAL;
    }
    dftk_mi_basis *bi = kb_in->basis, *bo = kb_out->basis;
    HIPCHK(hipSetDevice(bo->device));
    CHK(ensure_inverse_map(kb_in));
    CHK(ensure_G3(kb_out));
    CHK(check_dG(kb_in, kb_out, dG_h));
    if (n_bands == 0) return 0;
    CHK(order_after(bo, bi));
    {
        ProfScope prof_scope(bo, PROF_EW, kb_out->n_G >= 4096 ? 32.0 * (double)kb_out->n_G * n_bands : 0.0);
        const dim3 grid((unsigned)((kb_out->n_G + TR_NT - 1) / TR_NT), (unsigned)((n_bands + TR_BANDS - 1) / TR_BANDS));
        hipLaunchKernelGGL(k_transfer_blochwave, grid, dim3(TR_NT), 0, bo->stream, kb_out->n_G, kb_out->d_G3.get(), dG_h[0],
                           dG_h[1], dG_h[2], bi->nx, bi->ny, bi->nz, kb_in->d_inv.get(), n_bands,
                           reinterpret_cast<const cd*>(in_d), ld_in, reinterpret_cast<cd*>(out_d), ld_out);
        HIPCHK(hipGetLastError());
    }
    return order_after(bi, bo);
}

extern "C" int dftk_mi_transfer_density(dftk_mi_kblock* cube_kb_in, dftk_mi_kblock* cube_kb_out, int n_spin,
                                        const double* rho_in_d, double* rho_out_d) {
    if (!cube_kb_in || !cube_kb_out || !rho_in_d || !rho_out_d || (n_spin != 1 && n_spin != 2)) return DFTK_MI_EINVAL;
    if (!is_full_cube(cube_kb_in) || !is_full_cube(cube_kb_out) || cube_kb_in->sh_comm || cube_kb_out->sh_comm) {
        dftk_set_error("transfer_density: both k-blocks must span their whole cube and be unsharded");
        return DFTK_MI_EINVAL;
    }
    if (cube_kb_in->device != cube_kb_out->device) {
        dftk_set_error("transfer_density: the two bases live on different devices");
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("transfer_density: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    dftk_mi_basis *bi = cube_kb_in->basis, *bo = cube_kb_out->basis;
    HIPCHK(hipSetDevice(bo->device));
    const int64_t Ni = (int64_t)bi->nx * bi->ny * bi->nz, No = (int64_t)bo->nx * bo->ny * bo->nz;
    cd *tmp_i, *c_i, *tmp_o, *c_o;
    if (bi == bo) {
        CHK(scratch_grow(bi, bi->dense_ws, 4 * (size_t)Ni * sizeof(cd)));
        tmp_i = reinterpret_cast<cd*>(bi->dense_ws.get());
        tmp_o = tmp_i + 2 * Ni;
    } else {
        CHK(scratch_grow(bi, bi->dense_ws, 2 * (size_t)Ni * sizeof(cd)));
        CHK(scratch_grow(bo, bo->dense_ws, 2 * (size_t)No * sizeof(cd)));
        tmp_i = reinterpret_cast<cd*>(bi->dense_ws.get());
        tmp_o = reinterpret_cast<cd*>(bo->dense_ws.get());
    }
    c_i = tmp_i + Ni;
    c_o = tmp_o + No;
    for (int s = 0; s < n_spin; ++s) {
        CHK(cube_forward_real(cube_kb_in, rho_in_d + (size_t)s * Ni, nullptr, tmp_i, c_i));      // input stream: c_i = F[rho]
        CHK(order_after(bo, bi));
        hipLaunchKernelGGL(k_transfer_cube, dim3(2048), dim3(256), 0, bo->stream, bo->nx, bo->ny, bo->nz, bi->nx, bi->ny,
                           bi->nz, (const cd*)c_i, c_o);
        HIPCHK(hipGetLastError());
        CHK(order_after(bi, bo));                                                // c_i may be rewritten
        // fft(basis_in, .) carries sqrt(Omega) / N_in and irfft(basis_out, .) 1 / sqrt(Omega) (fft.jl:87-88)
        CHK(cube_backward_real(cube_kb_out, c_o, tmp_o, 1.0 / (double)Ni, rho_out_d + (size_t)s * No));
    }
    return order_after(bi, bo);
}
