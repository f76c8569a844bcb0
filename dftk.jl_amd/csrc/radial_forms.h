// radial_forms.h -- g_l(x) = j_l(x) / x^l for l = 0..3, the kernel of the modified Hankel transform of numeric (UPF)
// pseudopotentials (src/common/hankel.jl: the 1 / p^l factor folded into the Bessel function).  __host__ __device__
// inline, no HIP runtime call: tools/host_radial_check.cpp includes this header alone and runs without a GPU.
//
// Above the switch point x_l the closed form from ONE sincos; below it the even power series
//     g_l(x) = 1 / (2l+1)!! * sum_k (-x^2 / 2)^k / (k! (2l+3)(2l+5)...(2l+2k+1))
// (RADIAL_SERIES_TERMS terms, Horner from the back).  The closed forms cancel like x^-2l at small x (the reference's
// spherical_bessels.jl has the same forms without a series); the series is exact to rounding there and g_l(0) =
// 1 / (2l+1)!! needs no special case.  Switch points: where the two branches' largest errors against 40-digit values
// meet, in units of 2^-52 g_l(0) (DESIGN.md 3.18 has the table): both stay below 1 unit around x_l.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

#define RADIAL_SERIES_TERMS 16
#define RADIAL_LMAX 3

__host__ __device__ inline double radial_switch_point(int l) {
    switch (l) {
        case 0: return 1.0;
        case 1: return 2.0;
        case 2: return 3.0;
        default: return 4.0;
    }
}

// 1 / (2l+1)!!
__host__ __device__ inline double radial_g_at_zero(int l) {
    switch (l) {
        case 0: return 1.0;
        case 1: return 1.0 / 3.0;
        case 2: return 1.0 / 15.0;
        default: return 1.0 / 105.0;
    }
}

template <int L>
__host__ __device__ inline double radial_g_series(double x) {
    const double h = -0.5 * x * x;
    double acc = 0.0;
#pragma unroll
    for (int k = RADIAL_SERIES_TERMS; k >= 1; --k) acc = (1.0 + acc) * h / (double)(k * (2 * L + 2 * k + 1));
    return radial_g_at_zero(L) * (1.0 + acc);
}

// the closed forms, from sin x and cos x; x > 0
template <int L>
__host__ __device__ inline double radial_g_closed(double x, double s, double c) {
    if (L == 0) return s / x;
    if (L == 1) return (s - x * c) / (x * x * x);
    const double x2 = x * x;
    if (L == 2) return ((3.0 - x2) * s - 3.0 * x * c) / (x2 * x2 * x);
    return ((15.0 - 6.0 * x2) * s - (15.0 - x2) * x * c) / (x2 * x2 * x2 * x);
}

template <int L>
__host__ __device__ inline double radial_g(double x) {
    if (x < radial_switch_point(L)) return radial_g_series<L>(x);
    double s, c;
    sincos(x, &s, &c);
    return radial_g_closed<L>(x, s, c);
}

__host__ __device__ inline double radial_g_l(int l, double x) {
    switch (l) {
        case 0: return radial_g<0>(x);
        case 1: return radial_g<1>(x);
        case 2: return radial_g<2>(x);
        default: return radial_g<3>(x);
    }
}
