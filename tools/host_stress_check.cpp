// host_stress_check -- the closed forms of csrc/hgh_forms.h on the host, without a GPU: the header is all
// __host__ __device__ inline and calls no HIP runtime function.  Every tabulated HGH channel's six strain derivatives
// dP_ab, and the derivative of the local form factor, are compared with central
// differences of the functions they differentiate:
//   d/d eps_ab [ R_li(|q'|) Y_lm(q') / sqrt(1 + tr eps) ],  q' = (I - eps) q,  eps = t/2 (e_a e_b' + e_b e_a'), t = +-1e-5
// (truncation ~ t^2 f''' / 6 ~ 1e-10 of the values, round-off ~ 1e-16 / t ~ 1e-11: the bound is 1e-8 of the channel's
// largest derivative).  exit 0 + "host_stress_check OK" when every case holds.
#include "../dftk.jl_amd/csrc/hgh_forms.h"
#include <cstdio>

static double strained(int l, int m, int i, double rp, const double* q, const double eps[3][3]) {
    double p[3];
    for (int a = 0; a < 3; ++a) {
        p[a] = q[a];
        for (int b = 0; b < 3; ++b) p[a] -= eps[a][b] * q[b];
    }
    double R, dR, g[3];
    hgh_radial(l, i, rp, (p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) * rp * rp, &R, &dR);
    return R * solid_harmonic(l, m, p[0], p[1], p[2], g) / sqrt(1.0 + eps[0][0] + eps[1][1] + eps[2][2]);
}

int main() {
    const int ia[6] = {0, 1, 2, 2, 2, 1}, ib[6] = {0, 1, 2, 1, 0, 0};
    const int nl[4] = {3, 3, 2, 1};
    const double qs[3][3] = {{0.7, -0.4, 1.1}, {-2.3, 0.2, 0.9}, {0.05, 3.1, -1.7}};
    const double rps[2] = {0.45, 0.31};
    const double t = 1e-5;
    int failures = 0, cases = 0;
    for (int l = 0; l < 4; ++l)
        for (int i = 1; i <= nl[l]; ++i)
            for (int m = -l; m <= l; ++m)
                for (int iq = 0; iq < 3; ++iq)
                    for (int ir = 0; ir < 2; ++ir) {
                        double an[6], fd[6], scale = 0.0, err = 0.0;
                        hgh_dproj_amplitudes(l, m, i, rps[ir], qs[iq][0], qs[iq][1], qs[iq][2], an);
                        for (int c = 0; c < 6; ++c) {
                            double e[3][3] = {{0}}, f[3][3] = {{0}};
                            e[ia[c]][ib[c]] += t / 2; e[ib[c]][ia[c]] += t / 2;
                            f[ia[c]][ib[c]] -= t / 2; f[ib[c]][ia[c]] -= t / 2;
                            fd[c] = (strained(l, m, i, rps[ir], qs[iq], e) - strained(l, m, i, rps[ir], qs[iq], f)) / (2 * t);
                            scale = fmax(scale, fabs(fd[c]));
                            err = fmax(err, fabs(fd[c] - an[c]));
                        }
                        cases += 1;
                        if (!(err <= 1e-8 * scale)) {
                            failures += 1;
                            printf("l=%d m=%d i=%d q#%d rp=%.2f: error %.3e of %.3e FAILED\n", l, m, i, iq, rps[ir], err, scale);
                        }
                    }
    // q = 0: only the -1/2 delta_ab P term of the l = 0 channels is left
    {
        double an[6], R, dR;
        hgh_dproj_amplitudes(0, 0, 2, 0.45, 0.0, 0.0, 0.0, an);
        hgh_radial(0, 2, 0.45, 0.0, &R, &dR);
        const double want = -0.5 * R * sqrt(1.0 / (4.0 * M_PI));
        cases += 1;
        if (!(fabs(an[0] - want) <= 1e-15 * fabs(want) && an[0] == an[1] && an[1] == an[2] && an[3] == 0.0 && an[4] == 0.0 && an[5] == 0.0)) {
            failures += 1;
            printf("q = 0 FAILED\n");
        }
        hgh_dproj_amplitudes(1, 0, 1, 0.45, 0.0, 0.0, 0.0, an);
        for (int c = 0; c < 6; ++c)
            if (an[c] != 0.0) { failures += 1; printf("q = 0, l = 1 FAILED\n"); break; }
    }
    // local form factor: {rloc, Zion, c1..c4}
    const double par[6] = {0.44, 4.0, -7.3, 1.2, -0.3, 0.05};
    for (double p = 0.5; p < 12.0; p += 0.37) {
        double ff, dff, fp, fm, d;
        const double r2 = par[0] * par[0];
        hgh_local_ff_deriv(par, p * p * r2, &ff, &dff);
        hgh_local_ff_deriv(par, (p + t) * (p + t) * r2, &fp, &d);
        hgh_local_ff_deriv(par, (p - t) * (p - t) * r2, &fm, &d);
        const double fd = (fp - fm) / (2 * t), an = dff * 2.0 * p * r2;
        cases += 1;
        if (!(fabs(fd - an) <= 1e-8 * (fabs(fd) + 1.0))) {
            failures += 1;
            printf("local form factor at p=%.2f: fd %.10e analytic %.10e FAILED\n", p, fd, an);
        }
    }
    if (failures) {
        printf("host_stress_check: %d of %d case(s) FAILED\n", failures, cases);
        return 1;
    }
    printf("host_stress_check OK (%d cases)\n", cases);
    return 0;
}
