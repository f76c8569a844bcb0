// potmix_kernels.hip -- the cube-sized scalars of the potential-mixing SCF (src/scf/potential_mixing.jl): the slope and
// curvature of the quadratic energy model (:54-56), ||P^-1 dV||^2 of ScfAcceptImprovingStep (:14) and ||rho_next - rho_in||^2
// (:224) are all inner products of DIFFERENCES of arrays that exist already.  dftk_mi_diff_dots forms up to eight of them,
//   out[p] = sum_i (a_p[i] - b_p[i]) (c_p[i] - d_p[i]),
// in one launch without a temporary: block partials go straight into the basis' pinned landing zone and are summed on the host
// in block order, like dftk_mi_step_sums (mix_kernels.hip) -- one synchronisation, no atomics, bitwise repeatable.
//
// A pair has two operands (a - b) and (c - d); the 2 n_pairs operands are numbered in order.  The host marks an operand whose
// two pointers equal those of an earlier one (src[s] = that operand, else -1): the kernel then copies the earlier value
// instead of reading memory again (the density change drho enters four of the five scalars of a trial step).  src is uniform,
// so the choice is a scalar branch; the kernel is instantiated per n_pairs so that the operand values stay in registers.
#include "common.h"

namespace dftk_potmix {
const int MB = 128;          // blocks (partials are summed in block order)
const int MT = 256;
const int MAXP = 8;          // pairs of one call

struct Operands {
    const double* x[2 * MAXP];   // operand s = x[s][i] - y[s][i]; y[s] may be null (= 0)
    const double* y[2 * MAXP];
    int src[2 * MAXP];           // an earlier operand with the same two pointers, or -1
};

template <int NP>
__global__ __launch_bounds__(MT) void k_diff_dots(int64_t n, Operands op, double* __restrict__ hpart) {
    __shared__ double sh[MT / 64];
    double acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * MT + threadIdx.x; i < n; i += (int64_t)MB * MT) {
        double v[2 * NP];
#pragma unroll
        for (int s = 0; s < 2 * NP; ++s) {
            if (op.src[s] < 0) {
                double t = op.x[s][i];
                if (op.y[s]) t -= op.y[s][i];
                v[s] = t;
            } else {
                double t = 0.0;
#pragma unroll
                for (int q = 0; q < s; ++q) t = op.src[s] == q ? v[q] : t;
                v[s] = t;
            }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p] += v[2 * p] * v[2 * p + 1];
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const double t = block_sum<MT>(acc[p], sh);
        if (threadIdx.x == 0) hpart[(size_t)blockIdx.x * NP + p] = t;
    }
}

template <int NP>
void launch(dftk_mi_basis* b, int64_t n, const Operands& op, double* hpart) {
    hipLaunchKernelGGL(k_diff_dots<NP>, dim3(MB), dim3(MT), 0, b->stream, n, op, hpart);
}
}  // namespace dftk_potmix
using namespace dftk_potmix;

extern "C" int dftk_mi_diff_dots(dftk_mi_basis* b, int64_t n, int n_pairs, const double* const* a_d, const double* const* b_d,
                                 const double* const* c_d, const double* const* d_d, double* out_h) {
    if (!b || n < 1 || n_pairs < 1 || n_pairs > MAXP || !a_d || !c_d || !out_h) return DFTK_MI_EINVAL;
    Operands op;
    for (int p = 0; p < n_pairs; ++p) {
        if (!a_d[p] || !c_d[p]) return DFTK_MI_EINVAL;
        op.x[2 * p] = a_d[p];
        op.y[2 * p] = b_d ? b_d[p] : nullptr;
        op.x[2 * p + 1] = c_d[p];
        op.y[2 * p + 1] = d_d ? d_d[p] : nullptr;
    }
    for (int s = 0; s < 2 * MAXP; ++s) {
        if (s >= 2 * n_pairs) {
            op.x[s] = op.y[s] = nullptr;
            op.src[s] = -1;
            continue;
        }
        op.src[s] = -1;
        for (int q = 0; q < s && op.src[s] < 0; ++q)
            if (op.src[q] < 0 && op.x[q] == op.x[s] && op.y[q] == op.y[s]) op.src[s] = q;
    }
    static_assert((size_t)MB * MAXP * sizeof(double) <= HOST_FETCH_BYTES, "the block partials must fit the landing zone");
    HIPCHK(hipSetDevice(b->device));
    double* hpart = reinterpret_cast<double*>(b->h_fetch.get());
    switch (n_pairs) {
        case 1: launch<1>(b, n, op, hpart); break;
        case 2: launch<2>(b, n, op, hpart); break;
        case 3: launch<3>(b, n, op, hpart); break;
        case 4: launch<4>(b, n, op, hpart); break;
        case 5: launch<5>(b, n, op, hpart); break;
        case 6: launch<6>(b, n, op, hpart); break;
        case 7: launch<7>(b, n, op, hpart); break;
        default: launch<8>(b, n, op, hpart); break;
    }
    HIPCHK(hipGetLastError());
    CHK(host_wait(b));
    for (int p = 0; p < n_pairs; ++p) {
        double t = 0.0;
        for (int i = 0; i < MB; ++i) t += hpart[(size_t)i * n_pairs + p];
        out_h[p] = t;
    }
    return 0;
}
