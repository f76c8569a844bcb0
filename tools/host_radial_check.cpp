// host_radial_check.cpp -- g_l(x) = j_l(x) / x^l of csrc/radial_forms.h on the host, without a GPU.
//
// Both branches (even power series below the switch point, closed form above it) are driven on a grid that straddles
// every switch point and compared with a long-double evaluation: the ascending series in 64-bit-mantissa arithmetic
// below x = 8 (terms stay below 2^6 g_l(0) there), the upward recurrence j_{n+1} = (2n+1)/x j_n - j_{n-1} from j_0 and j_1
// above it (stable for x > n).  The bound is 4 units of
// 2^-52 g_l(0): the measured error of either branch is below 1 unit within the range of the other.
// The host part is compiled with AddressSanitizer and UBSan.
#include "radial_forms.h"
#include <cmath>
#include <cstdio>
#include <vector>

static long double ref_series(int l, long double x) {
    long double t = 1.0L;
    for (int k = 1; k <= l; ++k) t /= (long double)(2 * k + 1);
    const long double h = -0.5L * x * x;
    long double sum = 0.0L;
    for (int k = 0; k < 80; ++k) {
        sum += t;
        t *= h / ((long double)(k + 1) * (long double)(2 * l + 2 * k + 3));
    }
    return sum;
}

static long double ref_upward(int l, long double x) {
    const long double sn = sinl(x), cs = cosl(x);
    long double jm = sn / x, j = sn / (x * x) - cs / x;       // j_0, j_1
    if (l == 0) return jm;
    for (int n = 1; n < l; ++n) {
        const long double jp = (long double)(2 * n + 1) / x * j - jm;
        jm = j;
        j = jp;
    }
    for (int k = 0; k < l; ++k) j /= x;
    return j;
}

int main() {
    int bad = 0;
    double worst[4] = {0, 0, 0, 0};
    for (int l = 0; l <= RADIAL_LMAX; ++l) {
        const double xs = radial_switch_point(l), g0 = radial_g_at_zero(l);
        std::vector<double> pts = {0.0, 1e-300, 5e-16, 1e-8, 1e-3, nextafter(xs, 0.0), xs, nextafter(xs, 10.0)};
        for (int i = 1; i <= 4000; ++i) pts.push_back(0.0025 * i);                  // (0, 10]: both sides of every x_l
        for (int i = 0; i < 400; ++i) pts.push_back(10.0 + 17.3 * i + 0.01 * i * i);   // up to several thousand
        for (double x : pts) {
            const long double ref = x < 8.0 ? ref_series(l, (long double)x) : ref_upward(l, (long double)x);
            const double got = radial_g_l(l, x);
            const double err = (double)fabsl((long double)got - ref) / (g0 * 0x1p-52);
            if (err > worst[l]) worst[l] = err;
            if (!(err <= 4.0)) {
                if (bad < 10) std::printf("l=%d x=%.17g: got %.17g, ref %.17Lg (%.2f units)\n", l, x, got, ref, err);
                ++bad;
            }
        }
        // both branches at the switch point itself
        double s, c;
        sincos(xs, &s, &c);
        const double a = l == 0 ? radial_g_closed<0>(xs, s, c) : l == 1 ? radial_g_closed<1>(xs, s, c)
                       : l == 2 ? radial_g_closed<2>(xs, s, c) : radial_g_closed<3>(xs, s, c);
        const double b = l == 0 ? radial_g_series<0>(xs) : l == 1 ? radial_g_series<1>(xs)
                       : l == 2 ? radial_g_series<2>(xs) : radial_g_series<3>(xs);
        if (!(std::fabs(a - b) <= 4.0 * g0 * 0x1p-52)) {
            std::printf("l=%d: branches differ at the switch point: %.17g vs %.17g\n", l, a, b);
            ++bad;
        }
        if (radial_g_l(l, 0.0) != g0) {
            std::printf("l=%d: g_l(0) = %.17g\n", l, radial_g_l(l, 0.0));
            ++bad;
        }
    }
    std::printf("host_radial_check: worst error in units of 2^-52 g_l(0): l=0 %.2f, l=1 %.2f, l=2 %.2f, l=3 %.2f\n",
                worst[0], worst[1], worst[2], worst[3]);
    if (bad) {
        std::printf("host_radial_check: %d FAILURES\n", bad);
        return 1;
    }
    std::printf("host_radial_check OK\n");
    return 0;
}
