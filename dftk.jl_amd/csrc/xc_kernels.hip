// xc_kernels.hip -- the local-potential pipeline of energy_hamiltonian on the device:
//   Hartree   src/terms/hartree.jl:50-59   rho -> FFT -> * 4 pi / |G|^2 -> E_H = 1/2 Re <V_H(G), rho(G)> -> irfft
//   XC (LDA)  src/terms/xc.jl:84-160       e_xc(rho), v_xc(rho) point by point (Slater exchange, VWN5 / PW92
//                                          correlation: the closed forms libxc evaluates for lda_x, lda_c_vwn, lda_c_pw)
//   sum       src/terms/operators.jl:213-222   V = V_loc + V_H + v_xc, handed to the k-blocks as ONE potential
//   energies  src/terms/local.jl:15-16 (E_loc = sum rho V_loc dvol), xc.jl:113 (E_xc = sum e_xc dvol)
// One pass over the cube for XC + the sum + two energy reductions; the Poisson multiply and the Hartree energy
// ride on the Fourier-space pass between the two cube FFTs (the library's own pruned pipeline with a full "sphere").
// Reductions: one partial per workgroup, summed on the host in a fixed order (bitwise reproducible).
#include "common.h"
#include <cmath>
#include <vector>

namespace dftk_xc {   // (named: kernels of an anonymous namespace lose their names in rocprofv3 traces)
const int XC_BLOCKS = 1024;

__global__ __launch_bounds__(256) void k_real_to_complex(int64_t n, const double* __restrict__ x, cd* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = make_double2(x[i], 0.0);
}

// c <- green * c ; partial[block] = sum green |c_old|^2
__global__ __launch_bounds__(256) void k_poisson(int64_t n, cd* __restrict__ c, const double* __restrict__ green,
                                                 double* __restrict__ partial) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const cd v = c[i];
        const double g = green[i];
        acc += g * (v.x * v.x + v.y * v.y);
        c[i] = make_double2(g * v.x, g * v.y);
    }
    const double s = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// closed forms; eps = energy per particle, returns e = rho * eps and v = d e / d rho
__device__ __forceinline__ void lda_x(double rho, double& e, double& v) {
    const double cx = -0.73855876638202240588;   // -3/4 (3/pi)^(1/3)
    const double r13 = cbrt(rho);
    e = cx * rho * r13;
    v = (4.0 / 3.0) * cx * r13;
}
__device__ __forceinline__ void lda_c_vwn(double rho, double& e, double& v) {
    const double A = 0.0310907, b = 3.72744, c = 12.9352, x0 = -0.10498;
    const double rs = cbrt(3.0 / (4.0 * M_PI * rho));
    const double x = sqrt(rs);
    const double X = x * x + b * x + c, X0 = x0 * x0 + b * x0 + c;
    const double Q = sqrt(4.0 * c - b * b);
    const double at = atan(Q / (2.0 * x + b));
    const double eps = A * (log(x * x / X) + 2.0 * b / Q * at -
                            b * x0 / X0 * (log((x - x0) * (x - x0) / X) + 2.0 * (b + 2.0 * x0) / Q * at));
    const double dat = -2.0 * Q / (Q * Q + (2.0 * x + b) * (2.0 * x + b));
    const double deps_dx = A * (2.0 / x - (2.0 * x + b) / X + 2.0 * b / Q * dat -
                                b * x0 / X0 * (2.0 / (x - x0) - (2.0 * x + b) / X + 2.0 * (b + 2.0 * x0) / Q * dat));
    e = rho * eps;
    v = eps - rs / 3.0 * deps_dx / (2.0 * x);
}
__device__ __forceinline__ void lda_c_pw(double rho, double& e, double& v) {
    const double a = 0.031091, a1 = 0.21370, b1 = 7.5957, b2 = 3.5876, b3 = 1.6382, b4 = 0.49294;
    const double rs = cbrt(3.0 / (4.0 * M_PI * rho));
    const double sq = sqrt(rs);
    const double den = 2.0 * a * (b1 * sq + b2 * rs + b3 * rs * sq + b4 * rs * rs);
    const double lg = log1p(1.0 / den);
    const double eps = -2.0 * a * (1.0 + a1 * rs) * lg;
    const double dden = 2.0 * a * (b1 / (2.0 * sq) + b2 + 1.5 * b3 * sq + 2.0 * b4 * rs);
    // d lg / d rs = -dden / (den^2 + den), as two quotients: den^2 overflows for rho < 2e-234 (den ~ rs^2)
    const double deps = -2.0 * a * a1 * lg + 2.0 * a * (1.0 + a1 * rs) * (dden / den) / (den + 1.0);
    e = rho * eps;
    v = eps - rs / 3.0 * deps;
}

// ---- GGA (PBE): e(rho, sigma) with forward-mode derivatives d/d rho, d/d sigma carried through the closed forms
// (libxc's gga_x_pbe / gga_c_pbe on lda_c_pw_mod; Perdew, Burke, Ernzerhof 1996).  A dual number (v, d/d rho, d/d sigma) makes
// the potential terms exact derivatives of exactly the energy expression -- no hand-derived formulas.
// Dual<N>: a value and N derivative slots, every slot through the same operations.  D3 carries (d/d rho, d/d sigma) or
// (d/d rho_up, d/d rho_down), D4 (d/d rho_up, d/d rho_down, d/d sigma_tot).
// No fused multiply-adds from here to k_gga_spin: the compiler folds the seeds (1, 0) and (0, 1) of two derivative
// slots and then contracts the two slots differently, which breaks the exchange symmetry V_up(a, b) = V_down(b, a) of the
// collinear forms in the last bit.  With separate roundings every folding is exact and all slots round alike.
#pragma clang fp contract(off)
template <int N>
struct Dual {
    double v, d[N];
    template <class F>
    static __device__ __forceinline__ Dual make(double v, F slot) {      // value v, slot k = slot(k)
        Dual r;
        r.v = v;
#pragma unroll
        for (int k = 0; k < N; ++k) r.d[k] = slot(k);
        return r;
    }
    friend __device__ __forceinline__ Dual operator+(Dual a, Dual b) {
        return make(a.v + b.v, [&](int k) { return a.d[k] + b.d[k]; });
    }
    friend __device__ __forceinline__ Dual operator-(Dual a, Dual b) {
        return make(a.v - b.v, [&](int k) { return a.d[k] - b.d[k]; });
    }
    friend __device__ __forceinline__ Dual operator*(Dual a, Dual b) {
        return make(a.v * b.v, [&](int k) { return a.d[k] * b.v + a.v * b.d[k]; });
    }
    friend __device__ __forceinline__ Dual operator/(Dual a, Dual b) {
        const double q = a.v / b.v;
        return make(q, [&](int k) { return (a.d[k] - q * b.d[k]) / b.v; });
    }
    friend __device__ __forceinline__ Dual operator*(double c, Dual a) {
        return make(c * a.v, [&](int k) { return c * a.d[k]; });
    }
    friend __device__ __forceinline__ Dual operator+(double c, Dual a) { a.v = c + a.v; return a; }
    friend __device__ __forceinline__ Dual dchain(Dual a, double f, double df) {      // f(a) with f' = df
        return make(f, [&](int k) { return df * a.d[k]; });
    }
    friend __device__ __forceinline__ Dual dsqrt(Dual a) { const double r = sqrt(a.v); return dchain(a, r, 0.5 / r); }
    friend __device__ __forceinline__ Dual dcbrt(Dual a) { const double r = cbrt(a.v); return dchain(a, r, r / (3.0 * a.v)); }
    friend __device__ __forceinline__ Dual dlog1p(Dual a) { return dchain(a, log1p(a.v), 1.0 / (1.0 + a.v)); }
    friend __device__ __forceinline__ Dual dexpm1(Dual a) { const double e = expm1(a.v); return dchain(a, e, e + 1.0); }
    friend __device__ __forceinline__ Dual dexp(Dual a) { const double e = exp(a.v); return dchain(a, e, e); }
};
typedef Dual<2> D3;
typedef Dual<3> D4;
template <class T>
__device__ __forceinline__ T dc(double c) { return T{c, {}}; }      // a constant
// the PW92 fit G(rs; A, a1, b1 .. b4) = -2 A (1 + a1 rs) log1p(1 / (2 A (b1 sqrt(rs) + b2 rs + b3 rs^(3/2) + b4 rs^2)))
template <class T>
__device__ __forceinline__ T pw92_G(T rs, T sq, double A, double a1, double b1, double b2, double b3, double b4) {
    const T den = 2.0 * A * (b1 * sq + b2 * rs + b3 * (rs * sq) + b4 * (rs * rs));
    return (-2.0 * A) * ((1.0 + a1 * rs) * dlog1p(dc<T>(1.0) / den));
}

__device__ __forceinline__ D3 gga_x_pbe(D3 rho, D3 sigma) {
    const double kappa = 0.8040, mu = 0.2195149727645171;
    const double cx = -0.73855876638202240588;                       // -3/4 (3/pi)^(1/3)
    const D3 kf = dcbrt(3.0 * M_PI * M_PI * rho);
    const D3 s2 = sigma / (4.0 * (kf * kf * rho * rho));
    const D3 r13 = dcbrt(rho);
    return cx * (rho * r13) * ((1.0 + kappa) + (-kappa * kappa) * (dc<D3>(1.0) / (kappa + mu * s2)));
}
__device__ __forceinline__ D3 gga_c_pbe(D3 rho, D3 sigma) {
    const double beta = 0.06672455060314922, gamma = 0.031090690869654895;   // (1 - ln 2) / pi^2
    const D3 rs = dcbrt(dc<D3>(3.0 / (4.0 * M_PI)) / rho);
    const D3 sq = dsqrt(rs);
    const D3 eps = pw92_G(rs, sq, 0.0310907, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294);   // lda_c_pw_mod
    const D3 kf = dcbrt(3.0 * M_PI * M_PI * rho);
    const D3 t2 = (M_PI / 16.0) * (sigma / (kf * rho * rho));
    const D3 A = dc<D3>(beta / gamma) / dexpm1((-1.0 / gamma) * eps);
    const D3 f1 = t2 + A * (t2 * t2);
    const D3 H = gamma * dlog1p((beta / gamma) * (f1 / (1.0 + A * f1)));
    return rho * (eps + H);
}

// e, de/drho, de/dsigma per grid point; points with rho <= threshold contribute nothing (libxc-style threshold)
// core (optional): the core density of a non-linear core correction, the forms are evaluated at rho + core
__global__ __launch_bounds__(256) void k_gga(int64_t n, const double* __restrict__ rho, const double* __restrict__ core,
                                             const double* __restrict__ sigma, int fun_mask, double threshold,
                                             double* __restrict__ e, double* __restrict__ vrho, double* __restrict__ vsigma) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        D3 acc = dc<D3>(0.0);
        const double r = core ? rho[i] + core[i] : rho[i];
        if (r > threshold) {
            const D3 dr = D3{r, {1.0, 0.0}}, dsg = D3{sigma[i], {0.0, 1.0}};
            if (fun_mask & DFTK_MI_XC_GGA_X_PBE) acc = acc + gga_x_pbe(dr, dsg);
            if (fun_mask & DFTK_MI_XC_GGA_C_PBE) acc = acc + gga_c_pbe(dr, dsg);
        }
        e[i] = acc.v;
        vrho[i] = acc.d[0];
        vsigma[i] = acc.d[1];
    }
}
// ---- collinear spin, LDA: e(rho_up, rho_down) with forward-mode derivatives; the two derivative slots of D3 carry
// d/d rho_up and d/d rho_down here.  Closed forms as libxc's polarised lda_x (spin-scaling relation), lda_c_pw (PW92 eq. 8
// interpolation in zeta, f''(0) = 1.709921) and lda_xc_teter93 (Goedecker, Teter, Hutter 1996: Pade coefficients linear in
// f(zeta)).  The unpolarised lda_xc_teter93 is the same form at rho_up = rho_down.
__device__ __forceinline__ D3 dpow43(D3 a) { return a * dcbrt(a); }
__device__ __forceinline__ D3 spin_fzeta(D3 ra, D3 rb, D3 rt) {
    const D3 xa = 2.0 * (ra / rt), xb = 2.0 * (rb / rt);
    return (1.0 / (2.5198420997897464 - 2.0)) * (dpow43(xa) + dpow43(xb) + dc<D3>(-2.0));   // 2^(4/3) - 2
}
__device__ __forceinline__ D3 lda_x_spin(D3 ra, D3 rb) {
    const double cx = -0.73855876638202240588 * 1.2599210498948732;   // -3/4 (3/pi)^(1/3) 2^(1/3)
    return cx * (dpow43(ra) + dpow43(rb));
}
__device__ __forceinline__ D3 lda_c_pw_spin(D3 ra, D3 rb) {
    const D3 rt = ra + rb;
    const D3 fz = spin_fzeta(ra, rb, rt);
    const D3 z = (ra - rb) / rt;
    const D3 z2 = z * z, z4 = z2 * z2;
    const D3 rs = dcbrt(dc<D3>(3.0 / (4.0 * M_PI)) / rt);
    const D3 sq = dsqrt(rs);
    const D3 e0 = pw92_G(rs, sq, 0.031091, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294);
    const D3 e1 = pw92_G(rs, sq, 0.015545, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517);
    const D3 mac = pw92_G(rs, sq, 0.016887, 0.11125, 10.357, 3.6231, 0.88026, 0.49671);   // = -alpha_c
    return rt * (e0 - (1.0 / 1.709921) * (mac * fz * (dc<D3>(1.0) - z4)) + (e1 - e0) * (fz * z4));
}
__device__ __forceinline__ D3 lda_xc_teter93_spin(D3 ra, D3 rb) {
    const double a[4] = {0.4581652932831429, 2.217058676663745, 0.7405551735357053, 0.01968227878617998};
    const double da[4] = {0.119086804055547, 0.6157402568883345, 0.1574201515892867, 0.003532336663397157};
    const double bb[4] = {1.0, 4.504130959426697, 1.110667363742916, 0.02359291751427506};
    const double db[4] = {0.0, 0.2673612973836267, 0.2052004607777787, 0.004200005045691381};
    const D3 rt = ra + rb;
    const D3 fz = spin_fzeta(ra, rb, rt);
    const D3 rs = dcbrt(dc<D3>(3.0 / (4.0 * M_PI)) / rt);
    const D3 num = (a[0] + da[0] * fz) + rs * ((a[1] + da[1] * fz) + rs * ((a[2] + da[2] * fz) + rs * (a[3] + da[3] * fz)));
    const D3 den = rs * ((bb[0] + db[0] * fz) + rs * ((bb[1] + db[1] * fz) + rs * ((bb[2] + db[2] * fz) + rs * (bb[3] + db[3] * fz))));
    return dc<D3>(-1.0) * (rt * (num / den));
}
__device__ __forceinline__ D3 lda_spin_sum(double rho_up, double rho_dn, int fun_mask) {
    const double floor_ = 1e-20;                       // a spin channel is never evaluated below this density
    const D3 ra = D3{rho_up > floor_ ? rho_up : floor_, {1.0, 0.0}}, rb = D3{rho_dn > floor_ ? rho_dn : floor_, {0.0, 1.0}};
    D3 acc = dc<D3>(0.0);
    if (rho_up + rho_dn <= 2.0 * floor_) return acc;
    if (fun_mask & DFTK_MI_XC_LDA_X) acc = acc + lda_x_spin(ra, rb);
    if (fun_mask & DFTK_MI_XC_LDA_C_PW) acc = acc + lda_c_pw_spin(ra, rb);
    if (fun_mask & DFTK_MI_XC_LDA_XC_TETER93) acc = acc + lda_xc_teter93_spin(ra, rb);
    return acc;
}

// ---- collinear spin, GGA (PBE): e(rho_up, rho_down, sigma_uu, sigma_ud, sigma_dd), sigma_st = grad rho_s . grad rho_t.
// Exchange by the spin-scaling relation e_x = 1/2 [e_x0(2 rho_up, 4 sigma_uu) + e_x0(2 rho_down, 4 sigma_dd)] on the
// unpolarised gga_x_pbe above: one D3 per channel, slots (d/d rho_s, d/d sigma_ss), and de/dsigma_ud = 0.
// Correlation depends on (rho_up, rho_down, sigma_tot = sigma_uu + 2 sigma_ud + sigma_dd): D4 is D3 with one more slot,
// de/dsigma_uu = de/dsigma_dd = de/dsigma_tot, de/dsigma_ud = 2 de/dsigma_tot.  Closed form as libxc's polarised gga_c_pbe:
// eps_c(rs, zeta) is the PW92 interpolation with the lda_c_pw_mod parameters (the a = 0.0310907 of gga_c_pbe above, more
// digits for the other two fits and f''(0)), phi = ((1 + zeta)^(2/3) + (1 - zeta)^(2/3)) / 2, t^2 = pi sigma_tot /
// (16 phi^2 k_F rho^2), A = (beta / gamma) / expm1(-eps_c / (gamma phi^3)), H = gamma phi^3 log1p(...): gga_c_pbe
// term by term where phi = 1.
__device__ __forceinline__ D4 gga_c_pbe_spin(D4 ra, D4 rb, D4 sigma) {
    const double beta = 0.06672455060314922, gamma = 0.031090690869654895;   // (1 - ln 2) / pi^2
    const D4 rt = ra + rb;
    const D4 xa = 2.0 * (ra / rt), xb = 2.0 * (rb / rt);                     // 1 + zeta, 1 - zeta
    const D4 ca = dcbrt(xa), cb = dcbrt(xb);
    const D4 fz = (1.0 / (2.5198420997897464 - 2.0)) * (xa * ca + xb * cb + dc<D4>(-2.0));
    const D4 phi = 0.5 * (ca * ca + cb * cb);
    const D4 z = (ra - rb) / rt;
    const D4 z2 = z * z, z4 = z2 * z2;
    const D4 rs = dcbrt(dc<D4>(3.0 / (4.0 * M_PI)) / rt);
    const D4 sq = dsqrt(rs);
    const D4 e0 = pw92_G(rs, sq, 0.0310907, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294);
    const D4 e1 = pw92_G(rs, sq, 0.01554535, 0.20548, 14.1189, 6.1977, 3.3662, 0.62517);
    const D4 mac = pw92_G(rs, sq, 0.0168869, 0.11125, 10.357, 3.6231, 0.88026, 0.49671);   // = -alpha_c
    const D4 eps = e0 - (1.0 / 1.709920934161365617563962776245) * (mac * fz * (dc<D4>(1.0) - z4)) + (e1 - e0) * (fz * z4);
    const D4 phi2 = phi * phi, phi3 = phi2 * phi;
    const D4 kf = dcbrt(3.0 * M_PI * M_PI * rt);
    const D4 t2 = (M_PI / 16.0) * (sigma / (phi2 * (kf * rt * rt)));
    const D4 A = dc<D4>(beta / gamma) / dexpm1((-1.0 / gamma) * (eps / phi3));
    const D4 f1 = t2 + A * (t2 * t2);
    const D4 H = gamma * (phi3 * dlog1p((beta / gamma) * (f1 / (1.0 + A * f1))));
    return rt * (eps + H);
}
// Floors as lda_spin_sum: a channel enters as max(rho_s, 1e-20) and the derivatives are those of the clamped variables;
// rho_up + rho_down <= max(threshold, 2e-20) gives zeros; sigma_uu, sigma_dd and sigma_tot enter as max(., 0).
// core (optional): the TOTAL core density of a non-linear core correction, half of it joins each channel
__global__ __launch_bounds__(256) void k_gga_spin(int64_t n, const double* __restrict__ up, const double* __restrict__ dn,
                                                  const double* __restrict__ core,
                                                  const double* __restrict__ suu, const double* __restrict__ sud,
                                                  const double* __restrict__ sdd, int fun_mask, double threshold,
                                                  double* __restrict__ e, double* __restrict__ vup, double* __restrict__ vdn,
                                                  double* __restrict__ vsuu, double* __restrict__ vsud,
                                                  double* __restrict__ vsdd) {
    const double floor_ = 1e-20;
    const double cut = threshold > 2.0 * floor_ ? threshold : 2.0 * floor_;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double a = up[i], b = dn[i];
        if (core) {
            const double hc = 0.5 * core[i];
            a += hc;
            b += hc;
        }
        double ev = 0.0, va = 0.0, vb = 0.0, wuu = 0.0, wud = 0.0, wdd = 0.0;
        if (a + b > cut) {
            const double ra = a > floor_ ? a : floor_, rb = b > floor_ ? b : floor_;
            const double s_uu = suu[i], s_ud = sud[i], s_dd = sdd[i];
            const double p_uu = s_uu > 0.0 ? s_uu : 0.0, p_dd = s_dd > 0.0 ? s_dd : 0.0;
            if (fun_mask & DFTK_MI_XC_GGA_X_PBE) {
                const D3 xu = 0.5 * gga_x_pbe(D3{2.0 * ra, {2.0, 0.0}}, D3{4.0 * p_uu, {0.0, 4.0}});
                const D3 xd = 0.5 * gga_x_pbe(D3{2.0 * rb, {2.0, 0.0}}, D3{4.0 * p_dd, {0.0, 4.0}});
                ev += xu.v + xd.v;
                va += xu.d[0];
                vb += xd.d[0];
                wuu += xu.d[1];
                wdd += xd.d[1];
            }
            if (fun_mask & DFTK_MI_XC_GGA_C_PBE) {
                const double st = (s_uu + s_dd) + 2.0 * s_ud;      // (symmetric in the channels to the last bit)
                const D4 c = gga_c_pbe_spin(D4{ra, {1.0, 0.0, 0.0}}, D4{rb, {0.0, 1.0, 0.0}},
                                            D4{st > 0.0 ? st : 0.0, {0.0, 0.0, 1.0}});
                ev += c.v;
                va += c.d[0];
                vb += c.d[1];
                wuu += c.d[2];
                wud += 2.0 * c.d[2];
                wdd += c.d[2];
            }
        }
        e[i] = ev;
        vup[i] = va;
        vdn[i] = vb;
        vsuu[i] = wuu;
        vsud[i] = wud;
        vsdd[i] = wdd;
    }
}

// ---- meta-GGA (SCAN): e(rho, sigma, tau), slots (d/d rho, d/d sigma, d/d tau) of D4.  Closed forms of Sun, Ruzsinszky,
// Perdew, PRL 115, 036402 (2015) as libxc's unpolarised mgga_x_scan / mgga_c_scan:
//   p = s^2 = sigma / (4 k_F^2 rho^2),  alpha = (tau - sigma / (8 rho)) / tau_unif,  tau_unif = 3/10 k_F^2 rho
// sigma is not clamped against 8 rho tau: alpha may be negative, the forms are smooth there.
__device__ __forceinline__ D4 dinv_root4(D4 a) { return dc<D4>(1.0) / dsqrt(dsqrt(a)); }      // a^(-1/4)
// the switching function: exp(-c1 alpha / (1 - alpha)) below alpha = 1, -d exp(c2 / (1 - alpha)) above, 0 with zero slope at 1.
// Next to 1 the exponential underflows to 0 while the slope of its argument stays finite (|1 - alpha| >= 2^-53): no 0 * inf.
__device__ __forceinline__ D4 scan_switch(D4 alpha, double c1, double c2, double d) {
    const D4 oma = dc<D4>(1.0) - alpha;
    if (alpha.v < 1.0) return dexp((-c1) * (alpha / oma));
    if (alpha.v > 1.0) return (-d) * dexp(dc<D4>(c2) / oma);
    return dc<D4>(0.0);
}
__device__ __forceinline__ void scan_variables(D4 rho, D4 sigma, D4 tau, D4& p, D4& alpha) {
    const D4 kf = dcbrt(3.0 * M_PI * M_PI * rho);
    const D4 kf2r = kf * kf * rho;
    p = sigma / (4.0 * (kf2r * rho));
    // tau - tau_W cancels (tau_W = 5/3 s^2 tau_unif: 167 tau_unif at s = 10) and the switching function is steep in alpha,
    // so the value of the difference takes the rounding error of the quotient tau_W = sigma / (8 rho) back in (one fma
    // gives the remainder exactly); the slots are those of the plain expression
    D4 num = tau - sigma / (8.0 * rho);
    const double r8 = 8.0 * rho.v, tw = sigma.v / r8;
    num.v = (tau.v - tw) - fma(-tw, r8, sigma.v) / r8;
    alpha = num / (0.3 * kf2r);
}
__device__ __forceinline__ D4 mgga_x_scan(D4 rho, D4 sigma, D4 tau) {
    const double cx = -0.73855876638202240588;                       // -3/4 (3/pi)^(1/3)
    const double k1 = 0.065, h0 = 1.174, a1 = 4.9479, mu = 10.0 / 81.0;
    const double b2 = 0.12083045973594572;                           // sqrt(5913 / 405000)
    const double b1 = (511.0 / 13500.0) / (2.0 * b2), b3 = 0.5;
    const double b4 = mu * mu / k1 - 1606.0 / 18225.0 - b1 * b1;
    D4 p, alpha;
    scan_variables(rho, sigma, tau, p, alpha);
    const D4 oma = dc<D4>(1.0) - alpha;
    const D4 w = b1 * p + b2 * (oma * dexp((-b3) * (oma * oma)));
    const D4 y = mu * p + b4 * ((p * p) * dexp((-b4 / mu) * p)) + w * w;
    const D4 h1 = (1.0 + k1) + (-k1 * k1) * (dc<D4>(1.0) / (k1 + y));
    // g_x = 1 - exp(-a1 / p^(1/4)); where the exponential underflows (sigma = 0 included) g_x is the constant 1: the dual of
    // p^(-1/4) would multiply an infinite slope by a zero there
    D4 gx = dc<D4>(1.0);
    if (a1 / sqrt(sqrt(p.v)) <= 708.0) gx = dc<D4>(1.0) - dexp((-a1) * dinv_root4(p));
    const D4 fx = scan_switch(alpha, 0.667, 0.8, 1.24);
    const D4 Fx = (h1 + fx * (dc<D4>(h0) - h1)) * gx;
    return cx * (rho * dcbrt(rho)) * Fx;
}
__device__ __forceinline__ D4 mgga_c_scan(D4 rho, D4 sigma, D4 tau) {
    const double gamma = 0.031090690869654895;                       // (1 - ln 2) / pi^2
    const double b1c = 0.0285764, b2c = 0.0889, b3c = 0.125541, chi = 0.12802585262625815;
    D4 p, alpha;
    scan_variables(rho, sigma, tau, p, alpha);
    const D4 rs = dcbrt(dc<D4>(3.0 / (4.0 * M_PI)) / rho);
    const D4 sq = dsqrt(rs);
    const D4 eps = pw92_G(rs, sq, 0.0310907, 0.21370, 7.5957, 3.5876, 1.6382, 0.49294);   // lda_c_pw_mod
    const D4 beta = 0.066725 * ((1.0 + 0.1 * rs) / (1.0 + 0.1778 * rs));
    const D4 kf = dcbrt(3.0 * M_PI * M_PI * rho);
    const D4 t2 = (M_PI / 16.0) * (sigma / (kf * rho * rho));
    const D4 w1 = dexpm1((-1.0 / gamma) * eps);
    const D4 A = beta / (gamma * w1);
    const D4 eps1 = eps + gamma * dlog1p(w1 * (dc<D4>(1.0) - dinv_root4(1.0 + 4.0 * (A * t2))));
    const D4 e0 = dc<D4>(-b1c) / (1.0 + (b2c * sq + b3c * rs));
    const D4 w0 = dexpm1((-1.0 / b1c) * e0);
    const D4 eps0 = e0 + b1c * dlog1p(w0 * (dc<D4>(1.0) - dinv_root4(1.0 + (4.0 * chi) * p)));
    const D4 fc = scan_switch(alpha, 0.64, 1.5, 0.7);
    return rho * (eps1 + fc * (eps0 - eps1));
}
// e, de/drho, de/dsigma, de/dtau per grid point; points with rho <= threshold give zeros, as in k_gga
// add: e, vrho, vsigma already hold the GGA part of the same points (k_gga) and are added to
__global__ __launch_bounds__(256) void k_mgga(int64_t n, const double* __restrict__ rho, const double* __restrict__ sigma,
                                              const double* __restrict__ tau, int fun_mask, double threshold, bool add,
                                              double* __restrict__ e, double* __restrict__ vrho, double* __restrict__ vsigma,
                                              double* __restrict__ vtau) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        D4 acc = dc<D4>(0.0);
        const double r = rho[i];
        if (r > threshold) {
            const D4 dr = D4{r, {1.0, 0.0, 0.0}}, dsg = D4{sigma[i], {0.0, 1.0, 0.0}}, dt = D4{tau[i], {0.0, 0.0, 1.0}};
            if (fun_mask & DFTK_MI_XC_MGGA_X_SCAN) acc = acc + mgga_x_scan(dr, dsg, dt);
            if (fun_mask & DFTK_MI_XC_MGGA_C_SCAN) acc = acc + mgga_c_scan(dr, dsg, dt);
        }
        e[i] = add ? e[i] + acc.v : acc.v;
        vrho[i] = add ? vrho[i] + acc.d[0] : acc.d[0];
        vsigma[i] = add ? vsigma[i] + acc.d[1] : acc.d[1];
        vtau[i] = acc.d[2];
    }
}

#pragma clang fp contract(fast)

// V = V_loc + V_H + v_xc ; partials: [0] sum e_xc, [1] sum rho V_loc
// core (optional): e_xc and v_xc are those of rho + core, the local energy (and V_H, computed elsewhere) those of rho
__global__ __launch_bounds__(256) void k_xc_sum(int64_t n, const double* __restrict__ rho, const double* __restrict__ core,
                                                const cd* __restrict__ vh_cube,
                                                double vh_scale, const double* __restrict__ vloc, int fun_mask,
                                                const double* __restrict__ e_extra, const double* __restrict__ v_extra,
                                                double* __restrict__ V, double* __restrict__ partial) {
    __shared__ double sh[4];
    double acc_xc = 0.0, acc_loc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double r = rho[i];
        const double rx = core ? r + core[i] : r;         // the argument of the XC forms
        double e = 0.0, v = 0.0;
        if (fun_mask != 0 && rx > 1e-300) {
            double ei, vi;
            if (fun_mask & DFTK_MI_XC_LDA_X) { lda_x(rx, ei, vi); e += ei; v += vi; }
            if (fun_mask & DFTK_MI_XC_LDA_C_VWN) { lda_c_vwn(rx, ei, vi); e += ei; v += vi; }
            if (fun_mask & DFTK_MI_XC_LDA_C_PW) { lda_c_pw(rx, ei, vi); e += ei; v += vi; }
            if (fun_mask & DFTK_MI_XC_LDA_XC_TETER93) {   // the polarised form at rho_up = rho_down = rho / 2
                const D3 t = lda_spin_sum(0.5 * rx, 0.5 * rx, DFTK_MI_XC_LDA_XC_TETER93);
                e += t.v;
                v += t.d[0];
            }
        }
        if (e_extra) {                       // GGA part: e(rho, sigma) and v_rho - 2 div(v_sigma grad rho), precomputed
            e += e_extra[i];
            v += v_extra[i];
        }
        acc_xc += e;
        double tot = v;
        if (vloc) {
            const double vl = vloc[i];
            acc_loc += r * vl;
            tot += vl;
        }
        if (vh_cube) tot += vh_scale * vh_cube[i].x;
        if (V) V[i] = tot;
    }
    const double s0 = block_sum<256>(acc_xc, sh);
    const double s1 = block_sum<256>(acc_loc, sh);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s0;
        partial[XC_BLOCKS + blockIdx.x] = s1;
    }
}
// rho_tot as a complex cube (input of the Hartree pass of a collinear model)
__global__ __launch_bounds__(256) void k_total_to_complex(int64_t n, const double* __restrict__ up, const double* __restrict__ dn,
                                                          cd* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        out[i] = make_double2(up[i] + dn[i], 0.0);
}
// V_s = V_loc + V_H[rho_tot] + v_xc,s(rho_up, rho_down), s = up, down ; partials: [0] sum e_xc, [1] sum rho_tot V_loc
// core (optional): the TOTAL core density; the XC forms see rho_s + core / 2, the local energy rho_tot alone
__global__ __launch_bounds__(256) void k_xc_sum_spin(int64_t n, const double* __restrict__ up, const double* __restrict__ dn,
                                                     const double* __restrict__ core,
                                                     const cd* __restrict__ vh_cube, double vh_scale,
                                                     const double* __restrict__ vloc, int fun_mask,
                                                     const double* __restrict__ e_extra, const double* __restrict__ v_extra,
                                                     double* __restrict__ V_up, double* __restrict__ V_dn,
                                                     double* __restrict__ partial) {
    __shared__ double sh[4];
    double acc_xc = 0.0, acc_loc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double ra = up[i], rb = dn[i];
        const double hc = core ? 0.5 * core[i] : 0.0;
        D3 e = core ? lda_spin_sum(ra + hc, rb + hc, fun_mask) : lda_spin_sum(ra, rb, fun_mask);
        if (e_extra) {                       // GGA part: e and v_rho,s - 2 div(...) of the two channels (v_extra: 2 cubes)
            e.v += e_extra[i];
            e.d[0] += v_extra[i];
            e.d[1] += v_extra[n + i];
        }
        acc_xc += e.v;
        double common = 0.0;
        if (vloc) {
            const double vl = vloc[i];
            acc_loc += (ra + rb) * vl;
            common += vl;
        }
        if (vh_cube) common += vh_scale * vh_cube[i].x;
        if (V_up) {
            V_up[i] = common + e.d[0];
            V_dn[i] = common + e.d[1];
        }
    }
    const double s0 = block_sum<256>(acc_xc, sh);
    const double s1 = block_sum<256>(acc_loc, sh);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s0;
        partial[XC_BLOCKS + blockIdx.x] = s1;
    }
}
// ---- second derivatives f_xc = d^2 (rho eps_xc) / d rho^2 of the three closed forms above (the XC kernel of
// apply_kernel, src/terms/xc.jl:245-330).  With v = eps - (rs / 3) eps' (eps' = d eps / d rs) and d rs / d rho = -rs / (3 rho):
//   f = d v / d rho = -rs / (3 rho) (2/3 eps' - rs / 3 eps'')
__device__ __forceinline__ double lda_x_fxc(double rho) {
    const double cx = -0.73855876638202240588;
    const double r13 = cbrt(rho);
    return (4.0 / 9.0) * cx / (r13 * r13);
}
__device__ __forceinline__ double fxc_from_rs(double rho, double rs, double d1, double d2) {
    return -(rs / 3.0) * (((2.0 / 3.0) * d1 - rs / 3.0 * d2) / rho);   // (rs / rho itself overflows for rho < 1e-231)
}
__device__ __forceinline__ double lda_c_vwn_fxc(double rho) {
    const double A = 0.0310907, b = 3.72744, c = 12.9352, x0 = -0.10498;
    const double rs = cbrt(3.0 / (4.0 * M_PI * rho));
    const double x = sqrt(rs);
    const double X = x * x + b * x + c, X0 = x0 * x0 + b * x0 + c;
    const double Q = sqrt(4.0 * c - b * b);
    const double t = 2.0 * x + b;
    const double dat = -Q / (2.0 * X);                 // d atan(Q / (2 x + b)) / dx  (Q^2 + (2 x + b)^2 = 4 X)
    const double ddat = Q * t / (2.0 * X * X);
    const double u1 = -t / X, u2 = -(2.0 / X - t * t / (X * X));      // d/dx, d2/dx2 of -log X
    // eps = A (g(x) - b x0 / X0 h(x)),  g = log(x^2 / X) + 2 b / Q atan,  h = log((x - x0)^2 / X) + 2 (b + 2 x0) / Q atan
    const double g1 = 2.0 / x + u1 + 2.0 * b / Q * dat;
    const double g2 = -2.0 / (x * x) + u2 + 2.0 * b / Q * ddat;
    const double h1 = 2.0 / (x - x0) + u1 + 2.0 * (b + 2.0 * x0) / Q * dat;
    const double h2 = -2.0 / ((x - x0) * (x - x0)) + u2 + 2.0 * (b + 2.0 * x0) / Q * ddat;
    const double E1 = A * (g1 - b * x0 / X0 * h1), E2 = A * (g2 - b * x0 / X0 * h2);   // d eps / dx, d2 eps / dx2
    const double d1 = E1 / (2.0 * x);                                                  // x = sqrt(rs)
    const double d2 = E2 / (4.0 * rs) - E1 / (4.0 * rs * x);
    return fxc_from_rs(rho, rs, d1, d2);
}
__device__ __forceinline__ double lda_c_pw_fxc(double rho) {
    const double a = 0.031091, a1 = 0.21370, b1 = 7.5957, b2 = 3.5876, b3 = 1.6382, b4 = 0.49294;
    const double rs = cbrt(3.0 / (4.0 * M_PI * rho));
    const double sq = sqrt(rs);
    const double den = 2.0 * a * (b1 * sq + b2 * rs + b3 * rs * sq + b4 * rs * rs);
    const double lg = log1p(1.0 / den);
    const double dden = 2.0 * a * (b1 / (2.0 * sq) + b2 + 1.5 * b3 * sq + 2.0 * b4 * rs);
    const double ddden = 2.0 * a * (-b1 / (4.0 * rs * sq) + 0.75 * b3 / sq + 2.0 * b4);
    // d lg / d rs = -dden / W, W = den^2 + den; written with q = dden / den and iw = 1 / (den + 1) because W overflows for
    // rho < 2e-234 (den ~ rs^2) and W^2 long before: dden / W = q iw, (2 den + 1) dden^2 / W^2 = (2 den + 1) iw q^2 iw
    // (pre ~ rs is multiplied in before the last iw: q q iw alone underflows there, where the product is still 1e-299)
    const double q = dden / den, iw = 1.0 / (den + 1.0);
    const double pre = 2.0 * a * (1.0 + a1 * rs);
    const double pq = pre * q;
    const double d1 = -2.0 * a * a1 * lg + pq * iw;
    const double d2 = 4.0 * a * a1 * q * iw + (pre * (ddden / den) - (2.0 * den + 1.0) * iw * q * pq) * iw;
    return fxc_from_rs(rho, rs, d1, d2);
}

// dV = vh_scale Re(vh_cube) + f_xc(rho) drho
__global__ __launch_bounds__(256) void k_fxc_sum(int64_t n, const double* __restrict__ rho, const double* __restrict__ drho,
                                                 const cd* __restrict__ vh_cube, double vh_scale, int fun_mask,
                                                 double* __restrict__ dV) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double f = 0.0;
        if (fun_mask != 0) {
            const double r = rho[i];
            if (r > 1e-300) {
                if (fun_mask & DFTK_MI_XC_LDA_X) f += lda_x_fxc(r);
                if (fun_mask & DFTK_MI_XC_LDA_C_VWN) f += lda_c_vwn_fxc(r);
                if (fun_mask & DFTK_MI_XC_LDA_C_PW) f += lda_c_pw_fxc(r);
            }
        }
        double tot = f * drho[i];
        if (vh_cube) tot += vh_scale * vh_cube[i].x;
        dV[i] = tot;
    }
}
}  // namespace dftk_xc
using namespace dftk_xc;

// out[i] = scale * Re(c[i]) (+ add_scale * add[i mod n_add]: the gradient cubes of the core density, n_add = 3 N, joined
// to the three gradient cubes of the density or, halved, to the six of two spin channels; n <= 2 n_add)
__global__ __launch_bounds__(256) void k_xc_real_part_scaled(int64_t n, const cd* __restrict__ c, double scale,
                                                             const double* __restrict__ add, double add_scale, int64_t n_add,
                                                             double* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double v = scale * c[i].x;
        out[i] = add ? v + add_scale * add[i < n_add ? i : i - n_add] : v;
    }
}
// out[a n + i] = v[i] * g[a n + i], a = 0, 1, 2 (as complex numbers)
__global__ __launch_bounds__(256) void k_product3_to_complex(int64_t n, const double* __restrict__ v, const double* __restrict__ g,
                                                             cd* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double vi = v[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a * n + i] = make_double2(vi * g[a * n + i], 0.0);
    }
}

// out = green * (a + b) ; partial[block] = sum green |a + b|^2   (the Poisson pass of a collinear density, from F[rho_s])
__global__ __launch_bounds__(256) void k_poisson_sum(int64_t n, const cd* __restrict__ a, const cd* __restrict__ b,
                                                     const double* __restrict__ green, cd* __restrict__ out,
                                                     double* __restrict__ partial) {
    __shared__ double sh[4];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const cd va = a[i], vb = b[i];
        const double x = va.x + vb.x, y = va.y + vb.y;
        const double g = green[i];
        acc += g * (x * x + y * y);
        out[i] = make_double2(g * x, g * y);
    }
    const double s = block_sum<256>(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
// g: d_a rho_up (a = 0, 1, 2), then d_a rho_down; sigma: uu, ud, dd
__global__ __launch_bounds__(256) void k_sigma_spin(int64_t n, const double* __restrict__ g, double* __restrict__ sigma) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double uu = 0.0, ud = 0.0, dd = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double u = g[a * n + i], d = g[(3 + a) * n + i];
            uu += u * u;
            ud += u * d;
            dd += d * d;
        }
        sigma[i] = uu;
        sigma[n + i] = ud;
        sigma[2 * n + i] = dd;
    }
}
// out[(3 s + a) n + i] = v_sigma,ss d_a rho_s + 1/2 v_sigma,ud d_a rho_s'  (as complex numbers; v: uu, ud, dd)
__global__ __launch_bounds__(256) void k_flux_spin_to_complex(int64_t n, const double* __restrict__ v, const double* __restrict__ g,
                                                              cd* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double vuu = v[i], hud = 0.5 * v[n + i], vdd = v[2 * n + i];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double u = g[a * n + i], d = g[(3 + a) * n + i];
            // explicit fma: left to the compiler, the two sums contract differently (fma(vuu, u, hud d) but fma(hud, u, vdd d))
            // and rho_up = rho_down no longer gives V_up = V_down to the last bit
            out[a * n + i] = make_double2(fma(vuu, u, hud * d), 0.0);
            out[(3 + a) * n + i] = make_double2(fma(vdd, d, hud * u), 0.0);
        }
    }
}

// the three energies of a collinear pipeline from its reduction partials ([0] e_xc, [1] rho_tot V_loc, [2] Hartree)
static int collinear_energies(dftk_mi_basis* b, int64_t N, const double* partial, bool hartree, double* energies_h) {
    std::vector<double> hp(3 * XC_BLOCKS, 0.0);
    CHK(host_fetch(b, hp.data(), partial, (hartree ? 3 : 2) * XC_BLOCKS * sizeof(double)));
    double s3[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < XC_BLOCKS; ++i) s3[k] += hp[(size_t)k * XC_BLOCKS + i];
    const double dvol = b->volume / (double)N;
    energies_h[0] = hartree ? 0.5 * b->volume / ((double)N * (double)N) * s3[2] : 0.0;
    energies_h[1] = s3[0] * dvol;
    energies_h[2] = s3[1] * dvol;
    return 0;
}

// rho: (up, down), sigma: (uu, ud, dd), vrho: (up, down), vsigma: (uu, ud, dd), n values each
int xc_gga_spin_pointwise(dftk_mi_basis* b, int64_t n, const double* rho, const double* sigma, int fun_mask,
                          double threshold, double* e, double* vrho, double* vsigma) {
    hipLaunchKernelGGL(k_gga_spin, dim3(XC_BLOCKS), dim3(256), 0, b->stream, n, rho, rho + n, (const double*)nullptr, sigma,
                       sigma + n, sigma + 2 * n,
                       fun_mask, threshold, e, vrho, vrho + n, vsigma, vsigma + n, vsigma + 2 * n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}

int xc_mgga_pointwise(dftk_mi_basis* b, int64_t n, const double* rho, const double* sigma, const double* tau, int fun_mask,
                      double threshold, double* e, double* vrho, double* vsigma, double* vtau) {
    hipLaunchKernelGGL(k_mgga, dim3(XC_BLOCKS), dim3(256), 0, b->stream, n, rho, sigma, tau, fun_mask, threshold, false, e,
                       vrho, vsigma, vtau);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}

int xc_gga_pointwise(dftk_mi_basis* b, int64_t n, const double* rho, const double* sigma, int fun_mask,
                     double threshold, double* e, double* vrho, double* vsigma) {
    hipLaunchKernelGGL(k_gga, dim3(XC_BLOCKS), dim3(256), 0, b->stream, n, rho, (const double*)nullptr, sigma, fun_mask,
                       threshold, e, vrho, vsigma);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
}

// cube_kernels.hip
int cube_forward_real(dftk_mi_kblock* cube_kb, const double* f, const double* g, cd* tmp, cd* c_out);
int cube_gradient_multiply(dftk_mi_kblock* cube_kb, const double* recip_h, int alpha, const cd* c, cd* out, bool accumulate);
int cube_backward_real(dftk_mi_kblock* cube_kb, const cd* c, cd* tmp, double scale, double* out);
int cube_sigma(dftk_mi_basis* b, int64_t N, const double* gx, const double* gy, const double* gz, double* sigma);
int cube_axpy_real(dftk_mi_basis* b, int64_t N, const double* a, double scale, const cd* c, double* out);

// Collinear-spin LDA pipeline: rho = (rho_up, rho_down), two cubes; Hartree of the TOTAL density, V_loc, and the spin-resolved
// XC potential summed into (V_up, V_down); energies = Hartree, Xc, AtomicLocal (rho_tot V_loc).
// core (optional, ONE cube): the XC forms see rho_s + core / 2 (non-linear core correction), everything else rho.
int local_potential_collinear(dftk_mi_kblock* cube_kb, const double* rho, const double* core, const double* vloc,
                              const double* green, int fun_mask, double* V_out, double* energies_h) {
    dftk_mi_basis* b = cube_kb->basis;
    const int64_t N = (int64_t)b->nx * b->ny * b->nz;
    if (cube_kb->n_G != N) {
        dftk_set_error("local_potential_collinear: the k-block must span the whole cube (n_G = %lld, N = %lld)",
                       (long long)cube_kb->n_G, (long long)N);
        return DFTK_MI_EINVAL;
    }
    if (fun_mask & ~(1 | 4 | 32)) {
        dftk_set_error("local_potential_collinear: spin-polarised forms exist for lda_x, lda_c_pw, lda_xc_teter93 only "
                       "(mask %d)", fun_mask);
        return DFTK_MI_EINVAL;
    }
    CHK(scratch_grow(b, b->dense_ws, 2 * (size_t)N * sizeof(cd) + 3 * XC_BLOCKS * sizeof(double)));
    cd* c1 = reinterpret_cast<cd*>(b->dense_ws.get());
    cd* c2 = c1 + N;
    double* partial = reinterpret_cast<double*>(c2 + N);
    const double *up = rho, *dn = rho + N;
    const cd* vh = nullptr;
    if (green) {
        hipLaunchKernelGGL(k_total_to_complex, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, up, dn, c1);
        CHK(launch_fft_from_cube(cube_kb, c1, c2));
        hipLaunchKernelGGL(k_poisson, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, c2, green, partial + 2 * XC_BLOCKS);
        CHK(launch_ifft_to_cube(cube_kb, c2, c1));
        vh = c1;
    }
    hipLaunchKernelGGL(k_xc_sum_spin, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, up, dn, core, vh, 1.0 / (double)N, vloc,
                       fun_mask, (const double*)nullptr, (const double*)nullptr, V_out, V_out ? V_out + N : (double*)nullptr,
                       partial);
    HIPCHK(hipGetLastError());
    if (!energies_h) return 0;      // potential only: asynchronous, like every call that returns no host data
    return collinear_energies(b, N, partial, green != nullptr, energies_h);
}

// Collinear-spin GGA pipeline (xc.jl:120-137 with LibxcDensities for two spin components): as local_potential_collinear, plus
//   grad rho_s = irfft(i G_a fft(rho_s)),  sigma_st = grad rho_s . grad rho_t,  point-wise PBE (k_gga_spin),
//   V_s += v_rho,s - 2 div(v_sigma,ss grad rho_s + 1/2 v_sigma,ud grad rho_s')
// F[rho_up], F[rho_down] are computed once (the Poisson pass works on their sum); the six gradient cubes and the six flux
// cubes go through one transform pipeline each.  17 cube FFTs in 5 pipelines, 35 launches with Hartree.
// core / grad_core (optional: one cube and its three gradient cubes): half of each joins rho_s and grad rho_s in the XC
// forms, sigma and the flux; no transform and no launch more.
int local_potential_collinear_gga(dftk_mi_kblock* cube_kb, const double* recip_h, const double* rho, const double* core,
                                  const double* grad_core, const double* vloc, const double* green, int fun_mask,
                                  double threshold, double* V_out, double* energies_h) {
    dftk_mi_basis* b = cube_kb->basis;
    const int64_t N = (int64_t)b->nx * b->ny * b->nz;
    if (cube_kb->n_G != N) {
        dftk_set_error("local_potential_collinear_gga: the k-block must span the whole cube (n_G = %lld, N = %lld)",
                       (long long)cube_kb->n_G, (long long)N);
        return DFTK_MI_EINVAL;
    }
    if (fun_mask & ~(1 | 4 | 32 | 24)) {
        dftk_set_error("local_potential_collinear_gga: spin-polarised forms exist for lda_x, lda_c_pw, lda_xc_teter93, "
                       "gga_x_pbe, gga_c_pbe only (mask %d)", fun_mask);
        return DFTK_MI_EINVAL;
    }
    const int gga_mask = fun_mask & 24;
    if (!gga_mask) return local_potential_collinear(cube_kb, rho, core, vloc, green, fun_mask, V_out, energies_h);
    // complex cubes: c1 | F[rho_up], F[rho_down] | six gradient / flux cubes; real cubes: 6 gradients, 3 sigma, e, 2 v_rho,
    // 3 v_sigma; then the reduction partials
    CHK(scratch_grow(b, b->dense_ws,
                     9 * (size_t)N * sizeof(cd) + 15 * (size_t)N * sizeof(double) + 3 * XC_BLOCKS * sizeof(double)));
    cd* c1 = reinterpret_cast<cd*>(b->dense_ws.get());
    cd* f2 = c1 + N;                                   // F[rho_up], F[rho_down]; later the two divergences
    cd* g6 = f2 + 2 * N;
    double* grad = reinterpret_cast<double*>(g6 + 6 * N);   // d_a rho_up (a = 0, 1, 2), d_a rho_down
    double* sigma = grad + 6 * N;                      // uu, ud, dd
    double* e_g = sigma + 3 * N;
    double* vrho = e_g + N;                            // up, down
    double* vsig = vrho + 2 * N;                       // uu, ud, dd
    double* partial = vsig + 3 * N;
    const double *up = rho, *dn = rho + N;
    const cd* vh = nullptr;
    hipLaunchKernelGGL(k_real_to_complex, dim3(XC_BLOCKS), dim3(256), 0, b->stream, 2 * N, rho, g6);
    CHK(launch_fft_from_cube(cube_kb, g6, f2, 2));                                     // f2[s] = F[rho_s] (unnormalised)
    for (int s = 0; s < 2; ++s)
        for (int a = 0; a < 3; ++a) CHK(cube_gradient_multiply(cube_kb, recip_h, a, f2 + s * N, g6 + (3 * s + a) * N, false));
    if (green) {
        hipLaunchKernelGGL(k_poisson_sum, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, (const cd*)f2, (const cd*)(f2 + N), green,
                           c1, partial + 2 * XC_BLOCKS);
        CHK(launch_ifft_to_cube(cube_kb, c1, c1));                                     // c1 = N * V_H(r): kept until the final sum
        vh = c1;
    }
    CHK(launch_ifft_to_cube(cube_kb, g6, g6, 6));                                      // in place: N grad rho_s
    hipLaunchKernelGGL(k_xc_real_part_scaled, dim3(XC_BLOCKS), dim3(256), 0, b->stream, 6 * N, (const cd*)g6, 1.0 / (double)N,
                       core ? grad_core : (const double*)nullptr, 0.5, 3 * N, grad);
    hipLaunchKernelGGL(k_sigma_spin, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, (const double*)grad, sigma);
    hipLaunchKernelGGL(k_gga_spin, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, up, dn, core, (const double*)sigma,
                       (const double*)(sigma + N), (const double*)(sigma + 2 * N), gga_mask, threshold, e_g, vrho, vrho + N, vsig,
                       vsig + N, vsig + 2 * N);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_flux_spin_to_complex, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, (const double*)vsig,
                       (const double*)grad, g6);
    CHK(launch_fft_from_cube(cube_kb, g6, g6, 6));                                     // in place
    for (int s = 0; s < 2; ++s)
        for (int a = 0; a < 3; ++a) CHK(cube_gradient_multiply(cube_kb, recip_h, a, g6 + (3 * s + a) * N, f2 + s * N, a > 0));
    CHK(launch_ifft_to_cube(cube_kb, f2, g6, 2));                                      // g6[s] = N div(flux_s)
    double* v_g = sigma;                                                               // (sigma is dead by now): two cubes
    CHK(cube_axpy_real(b, 2 * N, vrho, -2.0 / (double)N, g6, v_g));
    hipLaunchKernelGGL(k_xc_sum_spin, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, up, dn, core, vh, 1.0 / (double)N, vloc,
                       fun_mask & (1 | 4 | 32), (const double*)e_g, (const double*)v_g, V_out,
                       V_out ? V_out + N : (double*)nullptr, partial);
    HIPCHK(hipGetLastError());
    if (!energies_h) return 0;      // potential only: asynchronous (no fetch, no synchronisation)
    return collinear_energies(b, N, partial, green != nullptr, energies_h);
}

// cube_kb: a k-block whose "sphere" is the whole cube (mapping = 0 .. N-1), i.e. the library's cube FFT.
// fun_mask may carry LDA bits (1, 2, 4: point-wise in the final pass) and GGA bits (8, 16): for the latter
//   grad rho = irfft(i G_a fft(rho))            (LibxcDensities, xc.jl:356-409)
//   sigma = |grad rho|^2, (e, v_rho, v_sigma) = point-wise PBE forms (k_gga)
//   v_xc = v_rho - 2 div(v_sigma grad rho),  div f = irfft(sum_a i G_a fft(f_a))   (xc.jl:140-150, :576-584)
// with G in cartesian coordinates from recip_h (row-major recip_lattice).  8 cube FFTs in total.
// core / grad_core (optional: one cube and its three gradient cubes, non-linear core correction): the XC forms are evaluated
// at rho + core with grad rho + grad core in sigma and the flux; Hartree and the local energy see rho alone.  The core is
// one more operand of passes that run anyway: no transform and no launch more.
// Meta-GGA bits (64, 128; dftk_mi_local_potential_mgga): tau is one more operand of the point-wise pass (k_mgga, after k_gga
// where GGA bits are mixed in) and Vtau_out = de/dtau one more output of it; V_out gets v_rho - 2 div(v_sigma grad rho) of the
// summed forms through the same two pipelines.  No transform more.
int local_potential_lda(dftk_mi_kblock* cube_kb, const double* recip_h, const double* rho, const double* core,
                        const double* grad_core, const double* vloc, const double* green, int fun_mask, double threshold,
                        double* V_out, double* energies_h, const double* tau, double* Vtau_out) {
    dftk_mi_basis* b = cube_kb->basis;
    const int64_t N = (int64_t)b->nx * b->ny * b->nz;
    if (cube_kb->n_G != N) {
        dftk_set_error("local_potential: the k-block must span the whole cube (n_G = %lld, N = %lld)",
                       (long long)cube_kb->n_G, (long long)N);
        return DFTK_MI_EINVAL;
    }
    const int mgga_mask = fun_mask & 192;
    if (mgga_mask && (!tau || core)) {
        dftk_set_error("local_potential: a meta-GGA functional needs tau and has no core correction (mask %d)", fun_mask);
        return DFTK_MI_EINVAL;
    }
    const int pbe_mask = fun_mask & 24;
    const int gga_mask = pbe_mask | mgga_mask;       // everything that takes the gradient branch
    // complex cubes c1, c2 (+ three more and 7 real cubes for GGA) + reduction partials in the basis' dense workspace
    const size_t need = (gga_mask ? 5 : 2) * (size_t)N * sizeof(cd) + (gga_mask ? 7 : 0) * (size_t)N * sizeof(double) +
                        3 * XC_BLOCKS * sizeof(double);
    CHK(scratch_grow(b, b->dense_ws, need));
    cd* c1 = reinterpret_cast<cd*>(b->dense_ws.get());
    cd* c2 = c1 + N;
    cd* g3 = gga_mask ? c2 + N : nullptr;          // three cubes behind one another (one FFT pipeline for the three)
    double* rbase = reinterpret_cast<double*>(c2 + N + (gga_mask ? 3 * N : 0));
    double* partial = rbase + (gga_mask ? 7 * N : 0);
    double *e_g = nullptr, *v_g = nullptr;
    const cd* vh = nullptr;
    std::vector<double> hp(3 * XC_BLOCKS, 0.0);
    // F[rho] (unnormalised) is computed ONCE: the gradient multipliers read it, then the Poisson kernel works on it in place.
    // The three components of grad rho and of v_sigma grad rho go through ONE transform pipeline each (three cubes per
    // launch) instead of three: 18 launches fewer per call -- on the 36^3 ... 30 x 30 x 120 cubes of the k-point workloads
    // every launch of this chain is ~6 us whatever it does.
    if (gga_mask) {
        double* grad[3] = {rbase, rbase + N, rbase + 2 * N};
        double* sigma = rbase + 3 * N;
        e_g = rbase + 4 * N;
        double* vrho = rbase + 5 * N;
        double* vsig = rbase + 6 * N;
        CHK(cube_forward_real(cube_kb, rho, nullptr, c1, c2));                         // c2 = F[rho]
        for (int a = 0; a < 3; ++a) CHK(cube_gradient_multiply(cube_kb, recip_h, a, c2, g3 + a * N, false));   // i G_a F[rho]
        if (green) {
            hipLaunchKernelGGL(k_poisson, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, c2, green, partial + 2 * XC_BLOCKS);
            CHK(launch_ifft_to_cube(cube_kb, c2, c1));                                 // c1 = N * V_H(r): kept until the final sum
            vh = c1;
        }
        CHK(launch_ifft_to_cube(cube_kb, g3, g3, 3));                                  // in place: N grad rho (complex cubes)
        hipLaunchKernelGGL(k_xc_real_part_scaled, dim3(XC_BLOCKS), dim3(256), 0, b->stream, 3 * N, (const cd*)g3, 1.0 / (double)N,
                           core ? grad_core : (const double*)nullptr, 1.0, 3 * N,
                           grad[0]);                                                   // the three gradients are adjacent
        CHK(cube_sigma(b, N, grad[0], grad[1], grad[2], sigma));
        if (pbe_mask)
            hipLaunchKernelGGL(k_gga, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, rho, core, (const double*)sigma, pbe_mask,
                               threshold, e_g, vrho, vsig);
        if (mgga_mask) {
            // without a caller's cube for it (energies only) v_tau lands in c2's storage, dead until the divergence below
            double* vt = Vtau_out ? Vtau_out : reinterpret_cast<double*>(c2);
            hipLaunchKernelGGL(k_mgga, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, rho, (const double*)sigma, tau, mgga_mask,
                               threshold, pbe_mask != 0, e_g, vrho, vsig, vt);
        }
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_product3_to_complex, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, (const double*)vsig,
                           (const double*)grad[0], g3);                                // v_sigma d_a rho, a = 0, 1, 2
        CHK(launch_fft_from_cube(cube_kb, g3, g3, 3));                                 // in place
        for (int a = 0; a < 3; ++a) CHK(cube_gradient_multiply(cube_kb, recip_h, a, g3 + a * N, c2, a > 0));   // c2 (+)= i G_a ...
        CHK(launch_ifft_to_cube(cube_kb, c2, g3));                                     // g3[0] = N div(...)
        v_g = sigma;                                                                   // (sigma is dead by now)
        CHK(cube_axpy_real(b, N, vrho, -2.0 / (double)N, g3, v_g));
    } else if (green) {
        hipLaunchKernelGGL(k_real_to_complex, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, rho, c1);
        CHK(launch_fft_from_cube(cube_kb, c1, c2));                       // c2 = F[rho] (unnormalised)
        hipLaunchKernelGGL(k_poisson, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, c2, green, partial + 2 * XC_BLOCKS);
        CHK(launch_ifft_to_cube(cube_kb, c2, c1));                        // c1 = N * V_H(r)
        vh = c1;
    }
    hipLaunchKernelGGL(k_xc_sum, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, rho, core, vh, 1.0 / (double)N, vloc,
                       fun_mask & (7 | 32), (const double*)e_g, (const double*)v_g, V_out, partial);
    HIPCHK(hipGetLastError());
    if (!energies_h) return 0;      // potential only: asynchronous (no fetch, no synchronisation)
    HIPCHK(hipMemcpyAsync(hp.data(), partial, (green ? 3 : 2) * XC_BLOCKS * sizeof(double), hipMemcpyDeviceToHost,
                          b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    double s[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < XC_BLOCKS; ++i) s[k] += hp[(size_t)k * XC_BLOCKS + i];
    const double dvol = b->volume / (double)N;
    energies_h[0] = green ? 0.5 * b->volume / ((double)N * (double)N) * s[2] : 0.0;   // Hartree
    energies_h[1] = s[0] * dvol;                                                        // Xc
    energies_h[2] = s[1] * dvol;                                                        // AtomicLocal
    return 0;
}

// dV = v_c * drho + f_xc(rho) drho: the Hartree part through the Poisson multiplier between two cube FFTs (as the potential
// pipeline above, hartree.jl:68-81), the XC part point by point in the final pass.  Asynchronous on the basis' stream.
int apply_kernel_lda(dftk_mi_kblock* cube_kb, const double* rho, const double* drho, const double* green, int fun_mask,
                     double* dV_out) {
    dftk_mi_basis* b = cube_kb->basis;
    const int64_t N = (int64_t)b->nx * b->ny * b->nz;
    if (cube_kb->n_G != N) {
        dftk_set_error("apply_kernel: the k-block must span the whole cube (n_G = %lld, N = %lld)", (long long)cube_kb->n_G,
                       (long long)N);
        return DFTK_MI_EINVAL;
    }
    const cd* vh = nullptr;
    if (green) {
        CHK(scratch_grow(b, b->dense_ws, 2 * (size_t)N * sizeof(cd) + XC_BLOCKS * sizeof(double)));
        cd* c1 = reinterpret_cast<cd*>(b->dense_ws.get());
        cd* c2 = c1 + N;
        double* partial = reinterpret_cast<double*>(c2 + N);
        hipLaunchKernelGGL(k_real_to_complex, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, drho, c1);
        CHK(launch_fft_from_cube(cube_kb, c1, c2));
        hipLaunchKernelGGL(k_poisson, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, c2, green, partial);
        CHK(launch_ifft_to_cube(cube_kb, c2, c1));                        // c1 = N * dV_H(r)
        vh = c1;
    }
    hipLaunchKernelGGL(k_fxc_sum, dim3(XC_BLOCKS), dim3(256), 0, b->stream, N, rho, drho, vh, 1.0 / (double)N, fun_mask & 7,
                       dV_out);
    HIPCHK(hipGetLastError());
    return 0;
}
