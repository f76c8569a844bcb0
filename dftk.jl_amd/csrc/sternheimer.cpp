// sternheimer.cpp -- dftk_mi_sternheimer: the Sternheimer solve of one k-block as ONE library call.
//
// Reference: sternheimer_solver (src/response/chi0.jl:115-232) on top of the block conjugate gradient cg! of
// src/response/cg.jl:30-128 -- same projections, same preconditioner, same locking of converged columns on a contiguous
// active range, same iteration count convention.  What differs is where the scalars live: alpha = gamma / <p, c> and
// beta = gamma' / gamma stay on the device (response_kernels.hip reads them there), so that an iteration waits for the
// host exactly once, for the residual norms that decide locking and convergence.
//
//   Phi = [psi_occ psi_extra]   one stacked basis: R(phi) = phi - Phi (Phi' phi) is one pair of zgemm calls
//   b   = -Q rhs,  Q = 1 - psi_occ psi_occ'
//   A   = R (H - eps) (1 - M (H - eps)) R,  M = psi_extra inv(psi_extra' (H - eps) psi_extra) psi_extra'
//   rhs of the CG: R (1 - (H psi_extra) inv(...) psi_extra') b;  preconditioner R TPA R with the mean kinetic energy of
//   the FIRST occupied column for every column;  x, r and p are re-projected by R after every update
//   back-substitution: alpha_k = inv(eps_extra - eps) .* (psi_extra' (b - (H - eps) x)),  dpsi = psi_extra alpha_k + x
//
// (H - eps_n) phi_n leaves the H apply finished: the shift rides on the kinetic multiplier of the gather pass
// (fft_kernels.hip: k_xfwd_gather).  The blocks live in the basis' response workspace (resp_ws): nothing of the k-block's
// LOBPCG state (lob_buf, the kept A X) is touched.
#include "common.h"
#include "batch.h"
#include <cmath>
#include <utility>
#include <vector>

namespace {
const cd ONE = {1.0, 0.0}, ZERO = {0.0, 0.0}, MINUS_ONE = {-1.0, 0.0};

struct Solver {
    dftk_mi_kblock* kb;
    dftk_mi_basis* b;
    int64_t n;          // rows = leading dimension of every internal block
    int n_occ, n_extra, nc;
    cd *Phi, *HPe, *Bq, *XR, *Cb, *Hb, *Pb, *S, *U;
    double* dbl;
    double *eps_d, *ee_d, *gam[2], *pc_d, *res_d, *mk_d, *junk_d;
    cd* X() const { return XR; }
    cd* Rr() const { return XR + (int64_t)n_occ * n; }
    cd* Pe() const { return Phi + (int64_t)n_occ * n; }

    // Y <- R Y for m columns
    int project(cd* Y, int m) {
        if (nc == 0 || m == 0) return 0;
        CHK(zgemm(b, 'C', nc, m, n, ONE, Phi, n, Y, n, ZERO, S, nc));
        return zgemm(b, 'N', n, m, nc, MINUS_ONE, Phi, n, S, nc, ONE, Y, n);
    }
    // OUT = (H - diag(eps)) Y for m columns (eps: device, m values)
    int apply_H_minus_eps(const cd* Y, cd* OUT, int m, const double* e_d) {
        if (kb->d_Vtau) {
            dftk_set_error("sternheimer: the block has a tau potential bound (meta-GGA): the solver does not know the "
                           "div-A-grad term");
            return DFTK_MI_EINVAL;
        }
        const int slot = prof_begin(b, PROF_APPLY_H, (double)m);
        int st = 0;
        if (kb->d_Vs) {
            st = launch_local_apply(kb, m, Y, n, OUT, n, true, true, e_d);
        } else {   // no local potential bound: kinetic pass, then the shift as a pass of its own
            st = launch_local_apply(kb, m, Y, n, OUT, n, true, false);
            if (st == 0) st = resp_axpby(b, n, m, -1.0, e_d, Y, n, 1.0, OUT, n);
        }
        if (st == 0) st = apply_nonlocal_rows(kb, m, kb->P, kb->ldP, n, Y, n, OUT, n, true, 0, nullptr);
        prof_end(b, slot);
        return st;
    }
    // U = inv(eps_extra - eps) .* (A' Y), n_extra x m
    int extra_coefficients(const cd* A, const cd* Y, int m, const double* e_d) {
        CHK(zgemm(b, 'C', n_extra, m, n, ONE, A, n, Y, n, ZERO, U, n_extra));
        return resp_scale_inv(b, n_extra, m, U, n_extra, ee_d, e_d);
    }
    // Cb[:, lo .. lo + m) = A IN[:, lo .. lo + m)   (Cb and Hb change roles)
    int apply_A(const cd* IN, int lo, int m) {
        const int64_t off = (int64_t)lo * n;
        CHK(ew_copy(b, n, m, IN + off, n, Cb + off, n));
        CHK(project(Cb + off, m));
        CHK(apply_H_minus_eps(Cb + off, Hb + off, m, eps_d + lo));
        if (n_extra > 0) {
            CHK(extra_coefficients(HPe, Cb + off, m, eps_d + lo));
            CHK(zgemm(b, 'N', n, m, n_extra, MINUS_ONE, HPe, n, U, n_extra, ONE, Hb + off, n));
        }
        CHK(project(Hb + off, m));
        std::swap(Cb, Hb);
        return 0;
    }
    // Cb[:, active] = R TPA R r[:, active]
    int precondition(int lo, int m) {
        const int64_t off = (int64_t)lo * n;
        CHK(ew_copy(b, n, m, Rr() + off, n, Cb + off, n));
        CHK(project(Cb + off, m));
        CHK(ew_tpa(b, n, m, Cb + off, n, Hb + off, n, kb->d_kin, mk_d + lo, junk_d + lo));
        CHK(project(Hb + off, m));
        std::swap(Cb, Hb);
        return 0;
    }
    int fetch_norms(std::vector<double>& h) {
        CHK(host_fetch(b, h.data(), res_d, (size_t)n_occ * sizeof(double)));
        for (double v : h)
            if (!std::isfinite(v)) {
                dftk_set_error("sternheimer: non-finite residual norm");
                return DFTK_MI_NUM_NONFINITE;
            }
        return 0;
    }
};
}   // namespace

int sternheimer_run(dftk_mi_kblock* kb, int n_occ, const cd* psi_occ, int64_t ld_occ, const double* eps_h, int n_extra,
                    const cd* psi_extra, int64_t ld_extra, const cd* rhs, int64_t ld_rhs, const double* tol_h, int miniter,
                    int maxiter, const cd* dpsi0, int64_t ld_dpsi0, cd* dpsi, int64_t ld_dpsi, int* n_iter_out,
                    double* resid_h, int* converged_out) {
    dftk_mi_basis* b = kb->basis;
    if (batching()) {
        dftk_set_error("sternheimer: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    Solver s;
    s.kb = kb;
    s.b = b;
    s.n = kb->n_G;
    s.n_occ = n_occ;
    s.n_extra = n_extra;
    s.nc = n_occ + n_extra;
    const int64_t n = s.n;
    const size_t col = (size_t)n;

    WsCarver ws;
    ws.take(&s.Phi, col * s.nc);
    ws.take(&s.HPe, col * n_extra);
    ws.take(&s.Bq, n_extra > 0 ? col * n_occ : 0);
    ws.take(&s.XR, 2 * col * n_occ);
    ws.take(&s.Cb, col * n_occ);
    ws.take(&s.Hb, col * n_occ);
    ws.take(&s.Pb, col * n_occ);
    ws.take(&s.S, 2 * (size_t)s.nc * n_occ);
    ws.take(&s.U, (size_t)n_extra * n_occ);
    ws.take(&s.dbl, 7 * (size_t)n_occ + (size_t)n_extra + 1);
    CHK(scratch_grow(b, b->resp_ws, ws.bytes()));
    ws.bind(b->resp_ws);
    s.eps_d = s.dbl;
    s.gam[0] = s.eps_d + n_occ;
    s.gam[1] = s.gam[0] + n_occ;
    s.pc_d = s.gam[1] + n_occ;
    s.res_d = s.pc_d + n_occ;
    s.mk_d = s.res_d + n_occ;
    s.junk_d = s.mk_d + n_occ;
    s.ee_d = s.junk_d + n_occ;       // n_extra + 1 values (the spare one takes the mean kinetic energy before the broadcast)

    // ---- set-up ------------------------------------------------------------------------------------------------------
    HIPCHK(hipMemcpyAsync(s.eps_d, eps_h, (size_t)n_occ * sizeof(double), hipMemcpyHostToDevice, b->stream));
    CHK(ew_copy(b, n, n_occ, psi_occ, ld_occ, s.Phi, n));
    if (n_extra > 0) {
        CHK(ew_copy(b, n, n_extra, psi_extra, ld_extra, s.Pe(), n));
        // H psi_extra and eps_extra = diag(psi_extra' H psi_extra) (the extra bands are Rayleigh-Ritz vectors)
        CHK(dftk_mi_apply_H_parts(kb, 7, n_extra, reinterpret_cast<const dftk_mi_cplx*>(s.Pe()), n,
                                  reinterpret_cast<dftk_mi_cplx*>(s.HPe), n));
        CHK(ew_coldots(b, n, n_extra, s.Pe(), n, s.HPe, n, s.ee_d));
    }
    // b = -Q rhs
    cd* const bq = n_extra > 0 ? s.Bq : s.Rr();
    CHK(zgemm(b, 'C', n_occ, n_occ, n, ONE, s.Phi, n, rhs, ld_rhs, ZERO, s.S, n_occ));
    CHK(resp_axpby(b, n, n_occ, -1.0, nullptr, rhs, ld_rhs, 0.0, bq, n));
    CHK(zgemm(b, 'N', n, n_occ, n_occ, ONE, s.Phi, n, s.S, n_occ, ONE, bq, n));
    // r = bb = R (b - H psi_extra (inv .* psi_extra' b))
    if (n_extra > 0) {
        CHK(s.extra_coefficients(s.Pe(), s.Bq, n_occ, s.eps_d));
        CHK(ew_copy(b, n, n_occ, s.Bq, n, s.Rr(), n));
        CHK(zgemm(b, 'N', n, n_occ, n_extra, MINUS_ONE, s.HPe, n, s.U, n_extra, ONE, s.Rr(), n));
    }
    CHK(s.project(s.Rr(), n_occ));
    // x = R dpsi0 (r -= A x) or 0
    if (dpsi0) {
        CHK(ew_copy(b, n, n_occ, dpsi0, ld_dpsi0, s.X(), n));
        CHK(s.project(s.X(), n_occ));
        CHK(s.apply_A(s.X(), 0, n_occ));
        CHK(resp_axpby(b, n, n_occ, -1.0, nullptr, s.Cb, n, 1.0, s.Rr(), n));
    } else {
        CHK(ew_fill_zero(b, s.X(), col * n_occ));
    }
    // TPA with the mean kinetic energy of the first occupied column for all columns (chi0.jl:214-217)
    CHK(ew_weighted_colsums(b, n, 1, s.Phi, n, kb->d_kin, s.ee_d + n_extra));
    CHK(resp_broadcast(b, n_occ, s.ee_d + n_extra, s.mk_d));
    int cur = 0;      // gam[cur] = gamma of this iteration
    CHK(s.precondition(0, n_occ));
    CHK(ew_coldots(b, n, n_occ, s.Rr(), n, s.Cb, n, s.gam[cur]));
    CHK(ew_copy(b, n, n_occ, s.Cb, n, s.Pb, n));
    CHK(ew_colnorms(b, n, n_occ, s.Rr(), n, s.res_d));
    std::vector<double> res(n_occ);
    CHK(s.fetch_norms(res));

    // ---- preconditioned block CG with locking (cg.jl:78-125): one host synchronisation per iteration ------------------------
    int n_iter = 0;
    bool converged = false;
    while (n_iter < maxiter) {
        n_iter += 1;
        int lo = -1, hi = -1;
        for (int c = 0; c < n_occ; ++c)
            if (!(res[c] <= tol_h[c])) {
                if (lo < 0) lo = c;
                hi = c;
            }
        if (n_iter >= miniter && lo < 0) {
            converged = true;
            break;
        }
        if (lo < 0) {   // all converged before miniter: the reference's findfirst(!, ...) has nothing to work on
            lo = 0;
            hi = n_occ - 1;
        }
        const int m = hi - lo + 1;
        const int64_t off = (int64_t)lo * n;
        CHK(s.apply_A(s.Pb, lo, m));                                                      // c = A p
        CHK(ew_coldots(b, n, m, s.Pb + off, n, s.Cb + off, n, s.pc_d + lo));
        CHK(resp_update_xr(b, n, m, s.gam[cur] + lo, s.pc_d + lo, s.Pb + off, n, s.Cb + off, n, s.X() + off, n,
                           s.Rr() + off, n));                                             // x += p alpha, r -= c alpha
        if (m == n_occ) {
            CHK(s.project(s.XR, 2 * n_occ));                                              // x and r are adjacent: one pair
        } else {
            CHK(s.project(s.X() + off, m));
            CHK(s.project(s.Rr() + off, m));
        }
        CHK(ew_colnorms(b, n, m, s.Rr() + off, n, s.res_d + lo));
        CHK(s.precondition(lo, m));                                                       // c = R TPA R r
        CHK(ew_coldots(b, n, m, s.Rr() + off, n, s.Cb + off, n, s.gam[1 - cur] + lo));
        CHK(resp_update_p(b, n, m, s.gam[1 - cur] + lo, s.gam[cur] + lo, s.Cb + off, n, s.Pb + off, n));   // p = c + p beta
        CHK(s.project(s.Pb + off, m));
        cur = 1 - cur;
        CHK(s.fetch_norms(res));                                                          // THE host synchronisation
    }

    // ---- back-substitution for the extra bands, result -------------------------------------------------------------------
    if (n_extra > 0) {
        CHK(s.apply_H_minus_eps(s.X(), s.Hb, n_occ, s.eps_d));
        CHK(resp_axpby(b, n, n_occ, 1.0, nullptr, s.Bq, n, -1.0, s.Hb, n));               // b - (H - eps) x
        CHK(s.extra_coefficients(s.Pe(), s.Hb, n_occ, s.eps_d));
        CHK(ew_copy(b, n, n_occ, s.X(), n, dpsi, ld_dpsi));
        CHK(zgemm(b, 'N', n, n_occ, n_extra, ONE, s.Pe(), n, s.U, n_extra, ONE, dpsi, ld_dpsi));
    } else {
        CHK(ew_copy(b, n, n_occ, s.X(), n, dpsi, ld_dpsi));
    }
    for (int c = 0; c < n_occ; ++c) resid_h[c] = res[c];
    *n_iter_out = n_iter;
    *converged_out = converged ? 1 : 0;
    return 0;
}

extern "C" int dftk_mi_sternheimer(dftk_mi_kblock* kb, int n_occ, const dftk_mi_cplx* psi_occ_d, int64_t ld_occ,
                                   const double* eps_h, int n_extra, const dftk_mi_cplx* psi_extra_d, int64_t ld_extra,
                                   const dftk_mi_cplx* rhs_d, int64_t ld_rhs, const double* tol_h, int miniter, int maxiter,
                                   const dftk_mi_cplx* dpsi0_d, int64_t ld_dpsi0, dftk_mi_cplx* dpsi_d, int64_t ld_dpsi,
                                   int* n_iter, double* resid_h, int* converged) {
    if (!kb || n_occ < 0 || n_extra < 0 || miniter < 0 || maxiter < 0 || !n_iter || !converged) return DFTK_MI_EINVAL;
    *n_iter = 0;
    *converged = 1;
    if (n_occ == 0) return 0;          // nothing to solve for (chi0.jl:216: "the (rare) cases when psi_k is empty")
    if (kb->sh_comm) {
        dftk_set_error("sternheimer: plane-wave sharded k-blocks are not supported");
        return DFTK_MI_EINVAL;
    }
    const int64_t n = kb->n_G;
    if (!psi_occ_d || !eps_h || !rhs_d || !tol_h || !dpsi_d || !resid_h || ld_occ < n || ld_rhs < n || ld_dpsi < n ||
        (n_extra > 0 && (!psi_extra_d || ld_extra < n)) || (dpsi0_d && ld_dpsi0 < n) || (int64_t)n_occ + n_extra > n) {
        dftk_set_error("sternheimer: invalid argument (null block, leading dimension below n_G = %lld, or more columns "
                       "than plane waves)", (long long)n);
        return DFTK_MI_EINVAL;
    }
    HIPCHK(hipSetDevice(kb->basis->device));
    return sternheimer_run(kb, n_occ, reinterpret_cast<const cd*>(psi_occ_d), ld_occ, eps_h, n_extra,
                           reinterpret_cast<const cd*>(psi_extra_d), ld_extra, reinterpret_cast<const cd*>(rhs_d), ld_rhs,
                           tol_h, miniter, maxiter, reinterpret_cast<const cd*>(dpsi0_d), ld_dpsi0,
                           reinterpret_cast<cd*>(dpsi_d), ld_dpsi, n_iter, resid_h, converged);
}

// compute_drho's accumulation at q = 0 (src/densities.jl:60-108):
//   drho(r) += 2 w_occ[n] Re(conj(psi_n(r)) dpsi_n(r)) + w_docc[n] |psi_n(r)|^2
extern "C" int dftk_mi_density_response_accumulate(dftk_mi_kblock* kb, int n_bands, const dftk_mi_cplx* psi_d, int64_t ld_psi,
                                                   const dftk_mi_cplx* dpsi_d, int64_t ld_dpsi, const double* w_occ_h,
                                                   const double* w_docc_h, double* drho_d) {
    if (!kb || !psi_d || !dpsi_d || !w_occ_h || !w_docc_h || !drho_d || n_bands < 0 || ld_psi < kb->n_G ||
        ld_dpsi < kb->n_G)
        return DFTK_MI_EINVAL;
    if (kb->sh_comm) {
        dftk_set_error("density_response_accumulate: plane-wave sharded k-blocks are not supported");
        return DFTK_MI_EINVAL;
    }
    if (batching()) {
        dftk_set_error("density_response_accumulate: not available inside a batched multi-k call");
        return DFTK_MI_EINVAL;
    }
    if (n_bands == 0) return 0;
    HIPCHK(hipSetDevice(kb->basis->device));
    return launch_density_response(kb, n_bands, reinterpret_cast<const cd*>(psi_d), ld_psi,
                                   reinterpret_cast<const cd*>(dpsi_d), ld_dpsi, w_occ_h, w_docc_h, drho_d);
}

// apply_kernel of TermHartree + TermXc (src/terms/hartree.jl:68-81, src/terms/xc.jl:245-330, LDA, no spin) in one call
extern "C" int dftk_mi_apply_kernel(dftk_mi_kblock* cube_kb, const double* rho_d, const double* drho_d,
                                    const double* poisson_green_d, int xc_functionals, double* dV_d) {
    if (!cube_kb || !drho_d || !dV_d || (xc_functionals & ~7) || (xc_functionals && !rho_d) || cube_kb->sh_comm)
        return DFTK_MI_EINVAL;
    HIPCHK(hipSetDevice(cube_kb->basis->device));
    return apply_kernel_lda(cube_kb, rho_d, drho_d, poisson_green_d, xc_functionals, dV_d);
}
