// refine.cpp -- dftk_mi_refinement_metric_solve: the inverse of the refinement metric of one k-block as ONE library call.
//
// Reference: invert_refinement_metric (src/postprocess/refine.jl:43-84) on top of cg! (src/response/cg.jl:30-128).  For every
// column n it solves
//     M_n x_n = P res_n,   M_n = P T_n^{1/2} P T_n^{1/2} P,   T_n = kin + mean_kin[n],   P = 1 - psi psi'
// by conjugate gradients preconditioned with P T_n^{-1} P, from x = 0, until ||r_n|| <= tol, and projects the result once
// more.  The reference runs one CG per column; here all columns iterate together, as in sternheimer.cpp: the projections
// are two zgemm calls for the whole block, the scalings one launch (refine_kernels.hip), and alpha_n = gamma_n / <p_n, M p_n>
// and beta_n = gamma_n' / gamma_n stay on the device (response_kernels.hip), so that an iteration waits for the host exactly
// once, for the residual norms.  The columns do not couple: each has its own alpha and beta, and a converged column is
// locked by setting its gamma to zero on the device (its x and r then stay bit for bit as they are), while the launches
// shrink to the contiguous range of columns that still iterate.  The iteration count of a column is the reference's n_iter:
// the pass of the loop in which its residual norm was first seen at or below tol (1 = the right-hand side was already
// there), maxiter if it never was.
//
// The blocks live in the basis' response workspace (resp_ws), which nothing here shares with the zgemm (ws).
#include "common.h"
#include "batch.h"
#include <cmath>
#include <vector>

namespace {
const cd ONE = {1.0, 0.0}, ZERO = {0.0, 0.0}, MINUS_ONE = {-1.0, 0.0};

struct MetricSolver {
    dftk_mi_kblock* kb;
    dftk_mi_basis* b;
    int64_t n;          // rows = leading dimension of every internal block
    int m;              // columns of psi and of the right-hand side
    cd *Phi, *X, *R, *Pb, *Cb, *S;
    double *mk_d, *gam[2], *pc_d, *res_d;

    // Y <- P Y for the columns [lo, lo + k)
    int project(cd* Y, int lo, int k) {
        cd* y = Y + (int64_t)lo * n;
        CHK(zgemm(b, 'C', m, k, n, ONE, Phi, n, y, n, ZERO, S, m));
        return zgemm(b, 'N', n, k, m, MINUS_ONE, Phi, n, S, m, ONE, y, n);
    }
    int scale(cd* Y, int lo, int k, int mode) {
        cd* y = Y + (int64_t)lo * n;
        return refine_scale_T(b, n, k, mode, kb->d_kin, mk_d + lo, y, n, y, n);
    }
    // Cb[:, lo .. lo + k) = M IN[:, lo .. lo + k)
    int apply_M(const cd* IN, int lo, int k) {
        const int64_t off = (int64_t)lo * n;
        CHK(ew_copy(b, n, k, IN + off, n, Cb + off, n));
        CHK(project(Cb, lo, k));
        CHK(scale(Cb, lo, k, 0));
        CHK(project(Cb, lo, k));
        CHK(scale(Cb, lo, k, 0));
        return project(Cb, lo, k);
    }
    // Cb[:, lo .. lo + k) = P T^{-1} P R[:, lo .. lo + k)
    int precondition(int lo, int k) {
        const int64_t off = (int64_t)lo * n;
        CHK(ew_copy(b, n, k, R + off, n, Cb + off, n));
        CHK(project(Cb, lo, k));
        CHK(scale(Cb, lo, k, 1));
        return project(Cb, lo, k);
    }
    int fetch_norms(std::vector<double>& h) {
        CHK(host_fetch(b, h.data(), res_d, (size_t)m * sizeof(double)));
        for (double v : h)
            if (!std::isfinite(v)) {
                dftk_set_error("refinement_metric_solve: non-finite residual norm");
                return DFTK_MI_NUM_NONFINITE;
            }
        return 0;
    }
};
}   // namespace

int refinement_metric_solve(dftk_mi_kblock* kb, int m, const cd* psi, int64_t ld_psi, const cd* res, int64_t ld_res,
                            double tol, int maxiter, cd* out, int64_t ld_out, int* iters_h, double* resnorm_h) {
    dftk_mi_basis* b = kb->basis;
    if (batching()) {
        dftk_set_error("refinement_metric_solve: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    MetricSolver s;
    s.kb = kb;
    s.b = b;
    s.n = kb->n_G;
    s.m = m;
    const int64_t n = s.n;
    const size_t col = (size_t)n;
    double* dbl;
    WsCarver ws;
    ws.take(&s.Phi, col * m);
    ws.take(&s.X, col * m);
    ws.take(&s.R, col * m);
    ws.take(&s.Pb, col * m);
    ws.take(&s.Cb, col * m);
    ws.take(&s.S, (size_t)m * m);
    ws.take(&dbl, 5 * (size_t)m);
    CHK(scratch_grow(b, b->resp_ws, ws.bytes()));
    ws.bind(b->resp_ws);
    s.mk_d = dbl;
    s.gam[0] = s.mk_d + m;
    s.gam[1] = s.gam[0] + m;
    s.pc_d = s.gam[1] + m;
    s.res_d = s.pc_d + m;

    // ---- set-up: mean kinetic energies (precondprep!), r = P res, x = 0, z = precon r, p = z -----------------------------
    CHK(ew_copy(b, n, m, psi, ld_psi, s.Phi, n));
    CHK(ew_weighted_colsums(b, n, m, s.Phi, n, kb->d_kin, s.mk_d));
    CHK(ew_copy(b, n, m, res, ld_res, s.R, n));
    CHK(s.project(s.R, 0, m));
    CHK(ew_fill_zero(b, s.X, col * m));
    int cur = 0;      // gam[cur] = gamma of this iteration
    CHK(s.precondition(0, m));
    CHK(ew_coldots(b, n, m, s.R, n, s.Cb, n, s.gam[cur]));
    CHK(ew_copy(b, n, m, s.Cb, n, s.Pb, n));
    CHK(ew_colnorms(b, n, m, s.R, n, s.res_d));
    CHK(refine_lock(b, m, s.res_d, tol, s.gam[cur]));
    std::vector<double> rn(m);
    CHK(s.fetch_norms(rn));

    // ---- preconditioned CG, every column on its own (cg.jl:78-125): one host synchronisation per iteration ----------------
    std::vector<int> iters(m, 0);
    int n_iter = 0;
    while (n_iter < maxiter) {
        n_iter += 1;
        int lo = -1, hi = -1;
        for (int c = 0; c < m; ++c) {
            if (rn[c] <= tol) {
                if (iters[c] == 0) iters[c] = n_iter;
            } else {
                if (lo < 0) lo = c;
                hi = c;
            }
        }
        if (lo < 0) break;
        const int k = hi - lo + 1;
        const int64_t off = (int64_t)lo * n;
        CHK(s.apply_M(s.Pb, lo, k));                                                      // c = M p
        CHK(ew_coldots(b, n, k, s.Pb + off, n, s.Cb + off, n, s.pc_d + lo));
        CHK(resp_update_xr(b, n, k, s.gam[cur] + lo, s.pc_d + lo, s.Pb + off, n, s.Cb + off, n, s.X + off, n, s.R + off,
                           n));                                                           // x += p alpha, r -= c alpha
        CHK(ew_colnorms(b, n, k, s.R + off, n, s.res_d + lo));
        CHK(s.precondition(lo, k));                                                       // c = P T^-1 P r
        CHK(ew_coldots(b, n, k, s.R + off, n, s.Cb + off, n, s.gam[1 - cur] + lo));
        CHK(refine_lock(b, k, s.res_d + lo, tol, s.gam[1 - cur] + lo));
        CHK(resp_update_p(b, n, k, s.gam[1 - cur] + lo, s.gam[cur] + lo, s.Cb + off, n, s.Pb + off, n));   // p = c + p beta
        cur = 1 - cur;
        CHK(s.fetch_norms(rn));                                                           // THE host synchronisation
    }
    CHK(s.project(s.X, 0, m));
    CHK(ew_copy(b, n, m, s.X, n, out, ld_out));
    for (int c = 0; c < m; ++c) {
        iters_h[c] = iters[c] ? iters[c] : n_iter;      // never seen converged: all passes were spent on it
        resnorm_h[c] = rn[c];
    }
    return 0;
}

extern "C" int dftk_mi_refinement_metric_solve(dftk_mi_kblock* kb, int n, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                                               const dftk_mi_cplx* res_d, int64_t ld_res, double tol, int maxiter,
                                               dftk_mi_cplx* out_d, int64_t ld_out, int* iters_h, double* resnorm_h) {
    if (!kb || n < 0 || maxiter < 0 || !(tol >= 0.0)) return DFTK_MI_EINVAL;
    if (n == 0) return 0;
    if (kb->sh_comm) {
        dftk_set_error("refinement_metric_solve: plane-wave sharded k-blocks are not supported");
        return DFTK_MI_EINVAL;
    }
    const int64_t n_G = kb->n_G;
    if (!psi_d || !res_d || !out_d || !iters_h || !resnorm_h || ld_psi < n_G || ld_res < n_G || ld_out < n_G || n > n_G ||
        n > 65535) {
        dftk_set_error("refinement_metric_solve: invalid argument (null block, leading dimension below n_G = %lld, or more "
                       "columns than plane waves)", (long long)n_G);
        return DFTK_MI_EINVAL;
    }
    HIPCHK(hipSetDevice(kb->basis->device));
    return refinement_metric_solve(kb, n, reinterpret_cast<const cd*>(psi_d), ld_psi, reinterpret_cast<const cd*>(res_d),
                                   ld_res, tol, maxiter, reinterpret_cast<cd*>(out_d), ld_out, iters_h, resnorm_h);
}
