// hgh_forms.h -- the closed forms of the HGH pseudopotentials and the small index helpers shared by the set-up, force,
// stress, cube and mixing kernels (gfx950 and host).  Everything is __host__ __device__ inline and needs no HIP runtime
// call: tools/host_stress_check.cpp includes this header and checks the derivatives against finite differences without
// a GPU.  Each form exists ONCE here; a consumer that needs only the value ignores the derivative (dead after inlining).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

// ------------------------------------------------------------------------------------------------ index helpers
// G_axis(n)[i]: [0 .. floor((n-1)/2), -ceil((n-1)/2) .. -1]   (src/fft.jl:24-31)
__host__ __device__ inline int signed_freq(int i, int n) { return i <= (n - 1) / 2 ? i : i - n; }

// cube entries whose -G partner is not on the grid (the Nyquist planes of even axes; enforce_real!, symmetry.jl:318-337)
__host__ __device__ inline bool unpaired_nyquist(int ix, int iy, int iz, int nx, int ny, int nz) {
    return ((nx % 2 == 0) && ix == nx / 2) || ((ny % 2 == 0) && iy == ny / 2) || ((nz % 2 == 0) && iz == nz / 2);
}

struct Mat3 {        // recip_lattice, column-major (b[3 j + i] = B_ij); passed to kernels by value
    double b[9];
};
__host__ __device__ inline Mat3 make_mat3(const double* recip) {
    Mat3 B;
    for (int i = 0; i < 9; ++i) B.b[i] = recip[i];
    return B;
}
// q = B p
__host__ __device__ inline void recip_times(const Mat3& B, double px, double py, double pz, double* qx, double* qy,
                                            double* qz) {
    *qx = px * B.b[0] + py * B.b[3] + pz * B.b[6];
    *qy = px * B.b[1] + py * B.b[4] + pz * B.b[7];
    *qz = px * B.b[2] + py * B.b[5] + pz * B.b[8];
}

struct ProjCol {         // one column of P
    double rx, ry, rz;   // atom position (reduced)
    double rp;           // r_l of the species
    int l, m, i, chan;   // angular momentum, magnetic index, radial index (1-based); chan: the channel's row of a table
                         // of radial values (dftk_mi_build_projectors_radial), 0 for the closed forms
};

// (re + i im) <- (-i)^l (re + i im):  1, -i, -1, i
__host__ __device__ inline void rotate_minus_i_pow(int l, double* re, double* im) {
    const double r = *re, i = *im;
    switch (l & 3) {
        case 0: break;
        case 1: *re = i; *im = -r; break;
        case 2: *re = -r; *im = -i; break;
        default: *re = -i; *im = r; break;
    }
}

// ------------------------------------------------------------------------------------------------ projectors
// eval_psp_projector_fourier (PspHgh.jl:140-164, divided by p^l) as a function of t2 = (p r_l)^2, and its t2 derivative.
// false (and NaN) for a channel that is not tabulated.
__host__ __device__ inline bool hgh_radial(int l, int i, double rp, double t2, double* R, double* dR) {
    const double common = 4.0 * pow(M_PI, 1.25) * sqrt(ldexp(1.0, l + 1) * rp * rp * rp) * exp(-t2 / 2.0);
    double c, poly = 1.0, dpoly = 0.0;
    switch (l * 4 + i) {
        case 0 * 4 + 1: c = 1.0; break;
        case 0 * 4 + 2: c = 2.0 / sqrt(15.0); poly = 3.0 - t2; dpoly = -1.0; break;
        case 0 * 4 + 3: c = 4.0 / (3.0 * sqrt(105.0)); poly = 15.0 - 10.0 * t2 + t2 * t2; dpoly = -10.0 + 2.0 * t2; break;
        case 1 * 4 + 1: c = rp / sqrt(3.0); break;
        case 1 * 4 + 2: c = 2.0 * rp / sqrt(105.0); poly = 5.0 - t2; dpoly = -1.0; break;
        case 1 * 4 + 3: c = 4.0 * rp / (3.0 * sqrt(1155.0)); poly = 35.0 - 14.0 * t2 + t2 * t2; dpoly = -14.0 + 2.0 * t2; break;
        case 2 * 4 + 1: c = rp * rp / sqrt(15.0); break;
        case 2 * 4 + 2: c = 2.0 * rp * rp / (3.0 * sqrt(105.0)); poly = 7.0 - t2; dpoly = -1.0; break;
        case 3 * 4 + 1: c = rp * rp * rp / sqrt(105.0); break;
        default: *R = *dR = nan(""); return false;
    }
    *R = common * c * poly;
    *dR = common * c * (dpoly - 0.5 * poly);
    return true;
}

// r^l Y_lm, real form (spherical_harmonics.jl:31-66), and its gradient g[3]
__host__ __device__ inline double solid_harmonic(int l, int m, double x, double y, double z, double* g) {
    const double pi = M_PI;
    g[0] = g[1] = g[2] = 0.0;
    if (l == 0) return sqrt(1.0 / (4.0 * pi));
    if (l == 1) {
        const double c = sqrt(3.0 / (4.0 * pi));
        if (m == -1) { g[1] = c; return c * y; }
        if (m == 0) { g[2] = c; return c * z; }
        g[0] = c;
        return c * x;
    }
    if (l == 2) {
        const double c = sqrt(15.0 / (4.0 * pi));
        switch (m) {
            case -2: g[0] = c * y; g[1] = c * x; return c * x * y;
            case -1: g[1] = c * z; g[2] = c * y; return c * y * z;
            case 0: {
                const double d = sqrt(5.0 / (16.0 * pi));
                g[0] = -2.0 * d * x; g[1] = -2.0 * d * y; g[2] = 4.0 * d * z;
                return d * (2.0 * z * z - x * x - y * y);
            }
            case 1: g[0] = c * z; g[2] = c * x; return c * x * z;
            default: {
                const double d = sqrt(15.0 / (16.0 * pi));
                g[0] = 2.0 * d * x; g[1] = -2.0 * d * y;
                return d * (x * x - y * y);
            }
        }
    }
    switch (m) {
        case -3: {
            const double a = sqrt(35.0 / (32.0 * pi));
            g[0] = a * 6.0 * x * y; g[1] = a * (3.0 * x * x - 3.0 * y * y);
            return a * (3.0 * x * x - y * y) * y;
        }
        case -2: {
            const double a = sqrt(105.0 / (4.0 * pi));
            g[0] = a * y * z; g[1] = a * x * z; g[2] = a * x * y;
            return a * x * y * z;
        }
        case -1: {
            const double a = sqrt(21.0 / (32.0 * pi));
            g[0] = -2.0 * a * x * y; g[1] = a * (4.0 * z * z - x * x - 3.0 * y * y); g[2] = 8.0 * a * y * z;
            return a * y * (4.0 * z * z - x * x - y * y);
        }
        case 0: {
            const double a = sqrt(7.0 / (16.0 * pi));
            g[0] = -6.0 * a * x * z; g[1] = -6.0 * a * y * z; g[2] = a * (6.0 * z * z - 3.0 * x * x - 3.0 * y * y);
            return a * z * (2.0 * z * z - 3.0 * x * x - 3.0 * y * y);
        }
        case 1: {
            const double a = sqrt(21.0 / (32.0 * pi));
            g[0] = a * (4.0 * z * z - 3.0 * x * x - y * y); g[1] = -2.0 * a * x * y; g[2] = 8.0 * a * x * z;
            return a * x * (4.0 * z * z - x * x - y * y);
        }
        case 2: {
            const double a = sqrt(105.0 / (16.0 * pi));
            g[0] = 2.0 * a * x * z; g[1] = -2.0 * a * y * z; g[2] = a * (x * x - y * y);
            return a * (x * x - y * y) * z;
        }
        default: {
            const double a = sqrt(35.0 / (32.0 * pi));
            g[0] = a * (3.0 * x * x - 3.0 * y * y); g[1] = -6.0 * a * x * y;
            return a * (x * x - 3.0 * y * y) * x;
        }
    }
}

// real amplitudes of the six strain derivatives (xx, yy, zz, zy, zx, yx) of R_li(|q|) Y_lm(q) / sqrt(Omega), without the
// 1 / sqrt(Omega) itself:  -1/2 delta_ab R Y - 2 r_l^2 (dR/dt2) q_a q_b Y - 1/2 R (q_a dY/dq_b + q_b dY/dq_a)
__host__ __device__ inline void hgh_dproj_amplitudes(int l, int m, int i, double rp, double qx, double qy, double qz,
                                                     double* out) {
    const double t2 = (qx * qx + qy * qy + qz * qz) * rp * rp;
    double R, dR, gY[3];
    hgh_radial(l, i, rp, t2, &R, &dR);
    const double Y = solid_harmonic(l, m, qx, qy, qz, gY);
    const double q[3] = {qx, qy, qz};
    const int ia[6] = {0, 1, 2, 2, 2, 1}, ib[6] = {0, 1, 2, 1, 0, 0};
    const double cr = 2.0 * rp * rp * dR * Y;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int a = ia[t], b = ib[t];
        out[t] = (a == b ? -0.5 * R * Y : 0.0) - cr * q[a] * q[b] - 0.5 * R * (q[a] * gY[b] + q[b] * gY[a]);
    }
}

// ------------------------------------------------------------------------------------------------ local part
// eval_psp_local_fourier (PspHgh.jl:110-124); par = {rloc, Zion, c1..c4}, t2 = (p rloc)^2.  The polynomial and its t2
// derivative:
__host__ __device__ inline double hgh_local_poly(const double* par, double t2) {
    return par[2] + par[3] * (3.0 - t2) + par[4] * (15.0 - 10.0 * t2 + t2 * t2) +
           par[5] * (105.0 - 105.0 * t2 + 21.0 * t2 * t2 - t2 * t2 * t2);
}
__host__ __device__ inline double hgh_local_dpoly(const double* par, double t2) {
    return -par[3] + par[4] * (-10.0 + 2.0 * t2) + par[5] * (-105.0 + 42.0 * t2 - 3.0 * t2 * t2);
}
// The form factor is written in TWO arithmetic orders over that polynomial, and both stay.  The local potential and the
// forces use (1), the stress kernel uses (2), which factors the Gaussian out so that the derivative shares it.  They
// agree to rounding, not to the last bit; the results of each consumer are pinned bit for bit against earlier builds, so
// neither order may replace the other.
//   (1) the value alone, as the reference spells it; 0 at t2 = 0 (compensating background)
__host__ __device__ inline double hgh_local_ff(const double* par, double t2) {
    const double rloc = par[0], Zion = par[1];
    if (!(t2 > 0.0)) return 0.0;
    const double P = hgh_local_poly(par, t2);
    return 4.0 * M_PI * rloc * rloc * (-Zion + sqrt(M_PI / 2.0) * rloc * t2 * P) * exp(-t2 / 2.0) / t2;
}
//   (2) value and d ff / d t2, t2 > 0
__host__ __device__ inline void hgh_local_ff_deriv(const double* par, double t2, double* ff, double* dff) {
    const double rloc = par[0], Zion = par[1];
    const double P = hgh_local_poly(par, t2), dP = hgh_local_dpoly(par, t2);
    const double A = 4.0 * M_PI * rloc * rloc * exp(-t2 / 2.0), Bc = sqrt(M_PI / 2.0) * rloc;
    const double inner = -Zion / t2 + Bc * P;
    *ff = A * inner;
    *dff = A * (Zion / (t2 * t2) + Bc * dP - 0.5 * inner);
}
