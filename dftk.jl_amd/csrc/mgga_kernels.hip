// mgga_kernels.hip -- what a meta-GGA adds on the orbital side (src/densities.jl:110-125, src/terms/operators.jl
// DivAgradOperator):
//   tau   += sum_n (w_n / 2) sum_a |ifft((G + k)_a psi_n)|^2                       the kinetic energy density
//   H psi += 1/2 sum_a (G + k)_a fft(v_tau ifft((G + k)_a psi))                    -1/2 div(v_tau grad psi)
// with (G + k) in cartesian coordinates from the frame of the block (dftk_mi_kblock_set_kpoint).  Both feed the existing
// pipelines (the density stages, the local-apply stages with the tau cube in the place of the local potential): the new work
// is the multiplication on the way in and the scaled accumulation on the way out, three transform pairs per band.
#include "common.h"
#include "batch.h"

namespace dftk_mgga {
struct Row3 {     // one row of the row-major reciprocal lattice and the k-point: (G + k)_a = sum_j r[j] (G_j + k[j])
    double r[3], k[3];
};
__device__ __forceinline__ double gk_component(const Row3& f, const int* __restrict__ G3, int64_t row) {
    return f.r[0] * ((double)G3[3 * row] + f.k[0]) + f.r[1] * ((double)G3[3 * row + 1] + f.k[1]) +
           f.r[2] * ((double)G3[3 * row + 2] + f.k[2]);
}
// out[:, n] = (G + k)_a in[:, n]
__global__ __launch_bounds__(256) void k_gk_scale(int64_t n_G, int nb, const int* __restrict__ G3, Row3 f,
                                                  const cd* __restrict__ in, int64_t ldin, cd* __restrict__ out, int64_t ldout) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n_G) return;
    const double g = gk_component(f, G3, row);
    for (int n = blockIdx.y; n < nb; n += gridDim.y) {
        const cd v = in[row + (int64_t)n * ldin];
        out[row + (int64_t)n * ldout] = make_double2(g * v.x, g * v.y);
    }
}
// H[:, n] += 1/2 (G + k)_a t[:, n]
__global__ __launch_bounds__(256) void k_gk_scale_accumulate(int64_t n_G, int nb, const int* __restrict__ G3, Row3 f,
                                                             const cd* __restrict__ t, int64_t ldt, cd* __restrict__ H,
                                                             int64_t ldH) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n_G) return;
    const double g = 0.5 * gk_component(f, G3, row);
    for (int n = blockIdx.y; n < nb; n += gridDim.y) {
        const cd v = t[row + (int64_t)n * ldt];
        cd h = H[row + (int64_t)n * ldH];
        h.x += g * v.x;
        h.y += g * v.y;
        H[row + (int64_t)n * ldH] = h;
    }
}
}  // namespace dftk_mgga
using namespace dftk_mgga;

static Row3 frame_row(const dftk_mi_kblock* kb, int a) {
    Row3 f;
    for (int j = 0; j < 3; ++j) {
        f.r[j] = kb->frame_B[3 * a + j];
        f.k[j] = kb->frame_k[j];
    }
    return f;
}
static dim3 rows_grid(const dftk_mi_kblock* kb, int nb) {
    return dim3((unsigned)((kb->n_G + 255) / 256), (unsigned)std::min(nb, 64));
}
// the block's n_G x nb scratch for the scaled orbitals; a regrow waits for the kernels that may still read the old one
static int mgga_scratch(dftk_mi_kblock* kb, int nb, const char* who) {
    if (!kb->frame_set) {
        dftk_set_error("%s: the block does not know its k-point (dftk_mi_kblock_set_kpoint)", who);
        return DFTK_MI_EINVAL;
    }
    if (kb->sh_comm || batching() || (kb->gr && kb->gr->on)) {
        dftk_set_error("%s: meta-GGA runs on un-sharded blocks of complex orbitals outside a batched call only", who);
        return DFTK_MI_EINVAL;
    }
    CHK(ensure_G3(kb));
    const size_t need = (size_t)kb->n_G * nb * sizeof(cd);
    if (need > kb->mgga_buf.bytes()) {
        HIPCHK(hipStreamSynchronize(kb->basis->stream));
        HIPCHK(kb->mgga_buf.reserve(need));
    }
    return 0;
}

int mgga_tau_accumulate(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, const double* w_h, double* tau) {
    CHK(mgga_scratch(kb, nb, "kinetic_energy_density_accumulate"));
    dftk_mi_basis* b = kb->basis;
    std::vector<double> half(w_h, w_h + nb);
    for (double& w : half) w *= 0.5;
    cd* t = kb->mgga_buf;
    for (int a = 0; a < 3; ++a) {
        hipLaunchKernelGGL(k_gk_scale, rows_grid(kb, nb), dim3(256), 0, b->stream, kb->n_G, nb, (const int*)kb->d_G3.get(),
                           frame_row(kb, a), psi, ldpsi, t, kb->n_G);
        HIPCHK(hipGetLastError());
        CHK(launch_density(kb, nb, t, kb->n_G, half.data(), tau));
    }
    // (`half` is pageable host memory owned by this call: band_groups (fft_kernels.hip) copies a group's weights to the device
    //  with hipMemcpyAsync, which stages pageable sources before it returns -- the convention its comment states for the
    //  callers' weight arrays; `half` may therefore go once the last launch_density has returned)
    return 0;
}

// H += 1/2 sum_a (G + k)_a fft(v_tau ifft((G + k)_a psi)): the local-apply pipeline, in place on the scaled block, with the
// tau cube bound where the stages read the local potential (the kernels take the pointer at launch)
int mgga_div_a_grad(dftk_mi_kblock* kb, int nb, const cd* psi, int64_t ldpsi, cd* H, int64_t ldH) {
    CHK(mgga_scratch(kb, nb, "apply_H"));
    dftk_mi_basis* b = kb->basis;
    cd* t = kb->mgga_buf;
    double* const Vs_bound = kb->d_Vs;
    for (int a = 0; a < 3; ++a) {
        const Row3 f = frame_row(kb, a);
        hipLaunchKernelGGL(k_gk_scale, rows_grid(kb, nb), dim3(256), 0, b->stream, kb->n_G, nb, (const int*)kb->d_G3.get(), f,
                           psi, ldpsi, t, kb->n_G);
        HIPCHK(hipGetLastError());
        kb->d_Vs = kb->d_Vtau;
        const int st = launch_local_apply(kb, nb, t, kb->n_G, t, kb->n_G, false, true);
        kb->d_Vs = Vs_bound;
        CHK(st);
        hipLaunchKernelGGL(k_gk_scale_accumulate, rows_grid(kb, nb), dim3(256), 0, b->stream, kb->n_G, nb,
                           (const int*)kb->d_G3.get(), f, (const cd*)t, kb->n_G, H, ldH);
        HIPCHK(hipGetLastError());
    }
    return 0;
}
