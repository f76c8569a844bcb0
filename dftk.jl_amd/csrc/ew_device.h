// ew_device.h -- the device bodies of the small column / element-wise operations of LOBPCG, each stated once.
// dense_kernels.hip wraps them in the single-block kernels that ew_* / apply_D launch (the column is blockIdx.x or
// blockIdx.y of one block), batch_kernels.hip in the table-driven kernels of a lock-step batch (the item is blockIdx.z):
// the wrappers pick the pointers of one column, the arithmetic is here.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------- column reductions
// The n_G-sized streaming kernels of one LOBPCG iteration.  They are HBM-bound, and what bounds them is the number of
// bytes in flight: one 16-byte load per thread and 2 x 256 threads per CU keeps 8 KB per CU in the
// air and reaches 1.2-1.5 TB/s (tools/ew_bench.py).  Here every thread issues EW_UNR independent loads per operand before
// it touches any of them, and a long column gets a workgroup of 1024 threads: 64 KB per operand and workgroup in flight.
// One workgroup of NT threads per column; deterministic (fixed strides, fixed tree; the tree depends on the workgroup
// size, which is a function of n alone).  A slot past the end of the column is never read or written and adds +0.0.
#define EW_UNR 4
#define EW_LONG 8192      // rows from which a column of a single block gets 1024 threads
// ax bx + ay by = fma(ax, bx, ay * by): the x product fused onto the rounded y product.  Which of two products
// -ffp-contract fuses depends on the IR around the expression; written out, every kernel that includes a body rounds
// its |z|^2 and Re conj(x) y alike; Im conj(x) y below is written out the same way.
__device__ __forceinline__ double ew_dot2(double ax, double bx, double ay, double by) { return fma(ax, bx, ay * by); }

// mode 0: *out = sqrt(sum |x|^2) ; 1: Re sum conj(x) y ; 2: sum w |x|^2 ; 3: sum |x|^2 ; 4: Im sum conj(x) y
template <int NT>
__device__ __forceinline__ void ew_col_reduce(int mode, int64_t n, const cd* __restrict__ x, const cd* __restrict__ y,
                                              const double* __restrict__ w, double* __restrict__ out) {
    __shared__ double sh[NT / 64];
    const bool two = mode == 1 || mode == 4;
    double acc = 0.0;
    for (int64_t i0 = threadIdx.x; i0 < n; i0 += (int64_t)NT * EW_UNR) {
        cd a[EW_UNR], bb[EW_UNR];
        double ww[EW_UNR];
#pragma unroll
        for (int u = 0; u < EW_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * NT;
            const bool in = i < n;
            a[u] = in ? x[i] : make_double2(0.0, 0.0);
            bb[u] = (in && two) ? y[i] : make_double2(0.0, 0.0);
            ww[u] = (in && mode == 2) ? w[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < EW_UNR; ++u) {
            if (mode == 1)
                acc += ew_dot2(a[u].x, bb[u].x, a[u].y, bb[u].y);
            else if (mode == 4)      // Im conj(a) b
                acc += fma(a[u].x, bb[u].y, -(a[u].y * bb[u].x));
            else if (mode == 2)
                acc += ww[u] * ew_dot2(a[u].x, a[u].x, a[u].y, a[u].y);
            else
                acc += ew_dot2(a[u].x, a[u].x, a[u].y, a[u].y);
        }
    }
    const double r = block_sum<NT>(acc, sh);
    if (threadIdx.x == 0) *out = (mode == 0) ? sqrt(r) : r;
}

// *out_xy = Re sum conj(x) y and *out_xx = sum |x|^2 from ONE read of x: per quantity the loop and the tree of
// ew_col_reduce<NT> (modes 1 and 3), so both results are bit for bit those of two separate reductions
template <int NT>
__device__ __forceinline__ void ew_col_dots2(int64_t n, const cd* __restrict__ x, const cd* __restrict__ y,
                                             double* __restrict__ out_xy, double* __restrict__ out_xx) {
    __shared__ double sh[NT / 64];
    double acc = 0.0, accx = 0.0;
    for (int64_t i0 = threadIdx.x; i0 < n; i0 += (int64_t)NT * EW_UNR) {
        cd a[EW_UNR], bb[EW_UNR];
#pragma unroll
        for (int u = 0; u < EW_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * NT;
            const bool in = i < n;
            a[u] = in ? x[i] : make_double2(0.0, 0.0);
            bb[u] = in ? y[i] : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int u = 0; u < EW_UNR; ++u) {
            acc += ew_dot2(a[u].x, bb[u].x, a[u].y, bb[u].y);
            accx += ew_dot2(a[u].x, a[u].x, a[u].y, a[u].y);
        }
    }
    const double s = block_sum<NT>(acc, sh);
    const double sx = block_sum<NT>(accx, sh);
    if (threadIdx.x == 0) {
        *out_xy = s;
        *out_xx = sx;
    }
}

// r = ax - l x ; *norm = ||r|| ; in the same pass over x (optional, kin != null / xx != null):
// *mk = sum kin |x|^2 (precondprep! of the TPA preconditioner) and *xx = sum |x|^2 (normalisation check)
template <int NT>
__device__ __forceinline__ void ew_residual_col(int64_t n, const cd* __restrict__ ax, const cd* __restrict__ xc, double l,
                                                cd* __restrict__ rc, double* __restrict__ norm,
                                                const double* __restrict__ kin, double* __restrict__ mk,
                                                double* __restrict__ xx) {
    __shared__ double sh[NT / 64];
    double acc = 0.0, acck = 0.0, accx = 0.0;
    for (int64_t i0 = threadIdx.x; i0 < n; i0 += (int64_t)NT * EW_UNR) {
        cd a[EW_UNR], x[EW_UNR];
        double kk[EW_UNR];
#pragma unroll
        for (int u = 0; u < EW_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * NT;
            const bool in = i < n;
            a[u] = in ? ax[i] : make_double2(0.0, 0.0);
            x[u] = in ? xc[i] : make_double2(0.0, 0.0);
            kk[u] = (in && kin) ? kin[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < EW_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * NT;
            const cd r = make_double2(a[u].x - l * x[u].x, a[u].y - l * x[u].y);
            if (i < n) rc[i] = r;
            acc += ew_dot2(r.x, r.x, r.y, r.y);
            const double x2 = ew_dot2(x[u].x, x[u].x, x[u].y, x[u].y);
            accx += x2;
            acck += kk[u] * x2;
        }
    }
    const double s = block_sum<NT>(acc, sh);
    const double sk = block_sum<NT>(acck, sh);
    const double sx = block_sum<NT>(accx, sh);
    if (threadIdx.x == 0) {
        *norm = sqrt(s);
        if (kin) *mk = sk;
        if (xx) *xx = sx;
    }
}

// ldiv!(precon, R) of the TPA preconditioner, out of place and with the column norm of the result:
//   dc = sc * mean_kin / (mean_kin + kin) ; *norm = ||dc||     (kin == null: plain copy)
// mean_kin: the column's mean kinetic energy, or null: precondprep! has not run yet ->
// ldiv!(Y, Diagonal(kin .+ default_shift), R)
template <int NT>
__device__ __forceinline__ void ew_tpa_col(int64_t n, const cd* __restrict__ sc, cd* __restrict__ dc,
                                           const double* __restrict__ kin, const double* __restrict__ mean_kin,
                                           double* __restrict__ norm, double default_shift) {
    __shared__ double sh[NT / 64];
    const double mk = (kin && mean_kin) ? *mean_kin : 0.0;
    double acc = 0.0;
    for (int64_t i0 = threadIdx.x; i0 < n; i0 += (int64_t)NT * EW_UNR) {
        cd r[EW_UNR];
        double kk[EW_UNR];
#pragma unroll
        for (int u = 0; u < EW_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * NT;
            const bool in = i < n;
            r[u] = in ? sc[i] : make_double2(0.0, 0.0);
            kk[u] = (in && kin) ? kin[i] : 1.0;
        }
#pragma unroll
        for (int u = 0; u < EW_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * NT;
            if (kin) {
                const double f = mean_kin ? mk / (mk + kk[u]) : 1.0 / (kk[u] + default_shift);
                r[u].x *= f;
                r[u].y *= f;
            }
            if (i < n) dc[i] = r[u];
            acc += ew_dot2(r[u].x, r[u].x, r[u].y, r[u].y);
        }
    }
    const double s = block_sum<NT>(acc, sh);
    if (threadIdx.x == 0) *norm = sqrt(s);
}

// ---------------------------------------------------------------------------- row-parallel forms
// a workgroup of 256 threads takes the EW_ROWS consecutive rows of one column that start at row block rb:
// y = f x (SCALE; x == y scales in place) or y = x (copy; a gather is a copy whose source column the caller permutes)
#define EW_ROWS (256 * EW_UNR)
template <bool SCALE>
__device__ __forceinline__ void ew_rows(int64_t n, int64_t rb, const cd* x, cd* y, double f) {
    const int64_t i0 = rb * EW_ROWS + threadIdx.x;
    cd v[EW_UNR];
#pragma unroll
    for (int u = 0; u < EW_UNR; ++u) {
        const int64_t i = i0 + u * 256;
        v[u] = i < n ? x[i] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int u = 0; u < EW_UNR; ++u) {
        const int64_t i = i0 + u * 256;
        if (i < n) y[i] = SCALE ? make_double2(v[u].x * f, v[u].y * f) : v[u];
    }
}

// y = f(kin + shift) x row by row, f(t) = 1 / t (INV) or sqrt(t): the diagonal operators T_n^{-1} and T_n^{1/2} of the
// refinement metric (T_n = kin + mean_kin[n], refine.jl:20-25); same row tile and load pattern as ew_rows, x == y allowed
template <bool INV>
__device__ __forceinline__ void ew_rows_kin(int64_t n, int64_t rb, const cd* x, cd* y, const double* __restrict__ kin,
                                            double shift) {
    const int64_t i0 = rb * EW_ROWS + threadIdx.x;
    cd v[EW_UNR];
    double t[EW_UNR];
#pragma unroll
    for (int u = 0; u < EW_UNR; ++u) {
        const int64_t i = i0 + u * 256;
        v[u] = i < n ? x[i] : make_double2(0.0, 0.0);
        t[u] = i < n ? kin[i] + shift : 1.0;
    }
#pragma unroll
    for (int u = 0; u < EW_UNR; ++u) {
        const int64_t i = i0 + u * 256;
        const double f = INV ? 1.0 / t[u] : sqrt(t[u]);
        if (i < n) y[i] = make_double2(v[u].x * f, v[u].y * f);
    }
}

// ---------------------------------------------------------------------------- small matrices: one thread per entry idx
// C[row0 + a, a] -= 1 for a in [0, cols)   (the "e" matrix of lobpcg_hyper_impl.jl:493-499)
__device__ __forceinline__ void ew_sub_identity_at(int64_t a, int64_t rows, int cols, cd* __restrict__ C, int64_t ldc,
                                                   int row0) {
    if (a < cols && row0 + a < rows) C[(row0 + a) + a * ldc].x -= 1.0;
}
__device__ __forceinline__ void ew_add_diag_at(int64_t i, int n, cd* __restrict__ A, int64_t lda, double shift) {
    if (i < n) A[i + i * lda].x += shift;
}
// make A exactly Hermitian from its upper triangle: A[j,i] = conj(A[i,j]) (i<j), Im A[i,i] = 0
__device__ __forceinline__ void ew_hermitize_at(int64_t idx, int n, cd* __restrict__ A, int64_t lda) {
    if (idx >= (int64_t)n * n) return;
    const int j = (int)(idx / n), i = (int)(idx - (int64_t)j * n);
    if (i == j) A[i + (int64_t)j * lda].y = 0.0;
    if (i < j) {
        const cd v = A[i + (int64_t)j * lda];
        A[j + (int64_t)i * lda] = make_double2(v.x, -v.y);
    }
}
// B = A^H (n x n)
__device__ __forceinline__ void ew_conj_transpose_at(int64_t idx, int n, const cd* __restrict__ A, int64_t lda,
                                                     cd* __restrict__ B, int64_t ldb) {
    if (idx >= (int64_t)n * n) return;
    const int j = (int)(idx / n), i = (int)(idx - (int64_t)j * n);
    const cd v = A[j + (int64_t)i * lda];
    B[i + (int64_t)j * ldb] = make_double2(v.x, -v.y);
}
// Y = D * X for the banded real D (n_p x n_p, half bandwidth bw), X is n_p x nb complex
__device__ __forceinline__ void ew_apply_D_at(int64_t idx, int n_p, int nb, int bw, const double* __restrict__ D,
                                              const cd* __restrict__ X, cd* __restrict__ Y) {
    if (idx >= (int64_t)n_p * nb) return;
    const int c = (int)(idx / n_p), i = (int)(idx - (int64_t)c * n_p);
    const int j0 = max(0, i - bw), j1 = min(n_p - 1, i + bw);
    double sr = 0.0, si = 0.0;
    for (int j = j0; j <= j1; ++j) {
        const double d = D[i + (int64_t)j * n_p];
        const cd x = X[j + (int64_t)c * n_p];
        sr += d * x.x;
        si += d * x.y;
    }
    Y[idx] = make_double2(sr, si);
}
