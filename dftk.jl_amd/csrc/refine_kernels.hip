// refine_kernels.hip -- the n_G-sized element-wise kernels of the refinement metric solve (refine.cpp; reference:
// invert_refinement_metric, src/postprocess/refine.jl:43-84).  The metric of column n is
//     M_n = P T_n^{1/2} P T_n^{1/2} P,   T_n = kin + mean_kin[n],   P = 1 - psi psi'
// and its preconditioner P T_n^{-1} P: between the projections (zgemm) stand two diagonal scalings whose factor depends on
// the row (kin) and on the column (mean_kin[n]).  One launch scales all columns; mean_kin is read from device memory.
// HBM-bound streams like the column ops of dense_kernels.hip: the body is ew_rows_kin of ew_device.h (EW_ROWS = 1024 rows of
// one column per workgroup of 256 threads, EW_UNR 16-byte loads per thread in flight).  No reductions: bitwise reproducible.
#include "common.h"
#include "ew_device.h"

namespace dftk_refine {
template <bool INV>
__global__ __launch_bounds__(256) void k_scale_T(int64_t n, const double* __restrict__ kin,
                                                 const double* __restrict__ mean_kin, const cd* X, int64_t ldx, cd* Y,
                                                 int64_t ldy) {
    const int c = blockIdx.y;
    ew_rows_kin<INV>(n, blockIdx.x, X + (int64_t)c * ldx, Y + (int64_t)c * ldy, kin, mean_kin[c]);
}

// gamma[c] = 0 where the column has converged (res[c] <= tol): alpha = gamma / <p, A p> and beta = gamma' / gamma of the CG
// kernels (response_kernels.hip) are then 0, so x and r of a converged column stay exactly as they are
__global__ __launch_bounds__(256) void k_lock(int m, const double* __restrict__ res, double tol, double* __restrict__ gamma) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < m && res[c] <= tol) gamma[c] = 0.0;
}
}   // namespace dftk_refine
using namespace dftk_refine;

int refine_scale_T(dftk_mi_basis* b, int64_t n, int m, int mode, const double* kin_d, const double* mean_kin_d, const cd* X,
                   int64_t ldx, cd* Y, int64_t ldy) {
    if (m <= 0 || n <= 0) return 0;
    ProfScope prof_scope(b, PROF_EW, n >= 4096 ? 40.0 * (double)n * m : 0.0);
    const dim3 grid((unsigned)((n + EW_ROWS - 1) / EW_ROWS), (unsigned)m);
    if (mode == 1)
        hipLaunchKernelGGL(k_scale_T<true>, grid, dim3(256), 0, b->stream, n, kin_d, mean_kin_d, X, ldx, Y, ldy);
    else
        hipLaunchKernelGGL(k_scale_T<false>, grid, dim3(256), 0, b->stream, n, kin_d, mean_kin_d, X, ldx, Y, ldy);
    HIPCHK(hipGetLastError());
    return 0;
}

int refine_lock(dftk_mi_basis* b, int m, const double* res_d, double tol, double* gamma_d) {
    if (m <= 0) return 0;
    hipLaunchKernelGGL(k_lock, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, b->stream, m, res_d, tol, gamma_d);
    HIPCHK(hipGetLastError());
    return 0;
}
