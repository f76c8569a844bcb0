// radial_kernels.hip -- radial (Hankel) transforms of numeric pseudopotentials on the device (gfx950 only).
//
// A UPF pseudopotential enters through quadratures over its radial mesh (about 10^3 points): per plane wave and
// projector channel (src/pseudo/PspUpf.jl:196-208), per cube point for the local potential (:229-263) and the atomic
// density.  The integrand enters every quadrature rule of the reference linearly (src/common/quadrature.jl), so the host
// folds the rule into a weight vector once per mesh and hands over wf_i = w_i r2_f_i; the device evaluates
//     kind 0:  out[j] = 4 pi sum_i wf_i r_i^l g_l(q_j r_i),     g_l(x) = j_l(x) / x^l    (hankel.jl, 1 / p^l folded in)
//     kind 1:  out[j] = 4 pi (sum_i wf_i sin(q_j r_i) / q_j - Zion / q_j^2 exp(-q_j^2 / 4)),  exactly 0 at q_j = 0
//              with wf_i = w_i (r_i vloc_i + Zion erf(r_i))                               (PspUpf.jl:229-242)
// One lane owns one q.  r and wf r^l are staged through LDS in tiles of RADIAL_TILE points; every lane of a wave reads
// the same LDS word (a broadcast: no bank conflicts) and pays one fp64 sincos per (q, r) pair above the switch point of
// g_l, the series below it (radial_forms.h).  The sum over i runs in ascending order in one lane with a compensation term
// (Kahan): no atomics, no cross-lane reduction, two calls are bitwise identical and the rounding of the sum does not grow
// with n_r.  n_r is not limited by LDS.
#include "common.h"
#include "radial_forms.h"
#include <cmath>

#define RADIAL_TILE 1024
#define RADIAL_THREADS 256

extern "C" int dftk_mi_radial_tile(void) { return RADIAL_TILE; }

// MODE 0..3: kind 0 with l = MODE; MODE 4: kind 1
template <int MODE>
__global__ __launch_bounds__(RADIAL_THREADS) void k_radial_transform(int n_r, const double* __restrict__ r,
                                                                     const double* __restrict__ wf, double Zion,
                                                                     int64_t n_q, const double* __restrict__ q,
                                                                     double* __restrict__ out) {
    __shared__ double s_r[RADIAL_TILE], s_w[RADIAL_TILE];
    const int64_t j = (int64_t)blockIdx.x * RADIAL_THREADS + threadIdx.x;
    const double qj = j < n_q ? q[j] : 0.0;
    double sum = 0.0, comp = 0.0;
    for (int t0 = 0; t0 < n_r; t0 += RADIAL_TILE) {
        const int nt = n_r - t0 < RADIAL_TILE ? n_r - t0 : RADIAL_TILE;
        __syncthreads();          // the previous tile has been consumed by every wave
        for (int i = threadIdx.x; i < nt; i += RADIAL_THREADS) {
            const double ri = r[t0 + i];
            double w = wf[t0 + i];
            if (MODE >= 1 && MODE <= 3) w *= ri;
            if (MODE >= 2 && MODE <= 3) w *= ri;
            if (MODE == 3) w *= ri;
            s_r[i] = ri;
            s_w[i] = w;
        }
        __syncthreads();
        for (int i = 0; i < nt; ++i) {
            const double x = qj * s_r[i];
            double term;
            if (MODE == 4) {
                term = s_w[i] * sin(x);
            } else {
                term = s_w[i] * radial_g<(MODE < 4 ? MODE : 0)>(x);
            }
            const double y = term - comp;
            const double t = sum + y;
            comp = (t - sum) - y;
            sum = t;
        }
    }
    if (j >= n_q) return;
    if (MODE == 4) {
        out[j] = qj == 0.0 ? 0.0 : 4.0 * M_PI * (sum / qj - Zion / (qj * qj) * exp(-0.25 * qj * qj));
    } else {
        out[j] = 4.0 * M_PI * sum;
    }
}

int radial_transform(dftk_mi_basis* b, int kind, int l, int n_r, const double* r_h, const double* wf_h, double Zion,
                     int64_t n_q, const double* q_d, double* out_d) {
    if (n_q == 0) return 0;
    // the two mesh vectors travel through the basis' workspace; the stream orders them against earlier users of it, and a
    // copy from pageable host memory returns once the host vectors have been read
    double *d_r, *d_w;
    WsCarver ws;
    ws.take(&d_r, (size_t)n_r), ws.take(&d_w, (size_t)n_r);
    CHK(ensure_ws(b, ws.bytes()));
    ws.bind(b->ws);
    HIPCHK(hipMemcpyAsync(d_r, r_h, (size_t)n_r * sizeof(double), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(d_w, wf_h, (size_t)n_r * sizeof(double), hipMemcpyHostToDevice, b->stream));
    const dim3 grid((unsigned)((n_q + RADIAL_THREADS - 1) / RADIAL_THREADS)), block(RADIAL_THREADS);
    const int mode = kind == 1 ? 4 : l;
#define RADIAL_LAUNCH(M)                                                                                           \
    hipLaunchKernelGGL(k_radial_transform<M>, grid, block, 0, b->stream, n_r, (const double*)d_r, (const double*)d_w, \
                       Zion, n_q, q_d, out_d)
    switch (mode) {
        case 0: RADIAL_LAUNCH(0); break;
        case 1: RADIAL_LAUNCH(1); break;
        case 2: RADIAL_LAUNCH(2); break;
        case 3: RADIAL_LAUNCH(3); break;
        default: RADIAL_LAUNCH(4); break;
    }
#undef RADIAL_LAUNCH
    HIPCHK(hipGetLastError());
    return 0;
}
