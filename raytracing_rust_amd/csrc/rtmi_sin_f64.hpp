// rtmi_sin_f64.hpp — the f64 render mode's sine for |x| < 2^40: sin(x) evaluated to about 90 bits and rounded once.
//
// The reference takes f64::sin from the platform's libm (texture.rs:41, :68), which the f64 oracle restates with glibc's
// sin.  glibc's is within 0.55 ULP, the device library's within 1 ULP of it, so a texture value that goes through a sine
// came out an ULP apart on a few pixels in a hundred.  This one is evaluated in double-double arithmetic (relative error
// about 2^-90) and rounded once.  That is no proof of correct rounding: sin(x) within 2^-90 of the midpoint of two doubles
// would round either way, about one argument in 2^37, which no test here can see.  It is the double nearest to sin(x)
// on every argument tested (25 118, tests/test_sin_f64.py); glibc's is that double too except where sin(x) lies within
// 0.05 ULP of a midpoint (measured there: 0.7 arguments in 1000).
//
// Plain C++ with fma and no contraction (-ffp-contract=off), for the device and for the host: the test compiles it with
// g++ and compares it with mpmath.  From 2^40 on, and for infinities and NaN, the caller's library sine answers.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RTMI_SIN_HD __host__ __device__ inline
#else
#define RTMI_SIN_HD inline
#endif

namespace rtmi_sin64 {

struct DD { double hi, lo; }; // hi + lo, |lo| <= ulp(hi) / 2

RTMI_SIN_HD DD two_sum(double a, double b) { // a + b exactly (Knuth)
    const double s = a + b, bb = s - a;
    return DD{s, (a - (s - bb)) + (b - bb)};
}
RTMI_SIN_HD DD fast_two_sum(double a, double b) { // a + b exactly, given |a| >= |b| or a == 0 (Dekker)
    const double s = a + b;
    return DD{s, b - (s - a)};
}
RTMI_SIN_HD DD two_prod(double a, double b) { // a * b exactly
    const double p = a * b;
    return DD{p, ::fma(a, b, -p)};
}
RTMI_SIN_HD DD dd_add(DD a, DD b) { // relative error about 2^-104, under cancellation too
    DD s = two_sum(a.hi, b.hi);
    const DD t = two_sum(a.lo, b.lo);
    s = fast_two_sum(s.hi, s.lo + t.hi);
    return fast_two_sum(s.hi, s.lo + t.lo);
}
RTMI_SIN_HD DD dd_mul(DD a, DD b) { // relative error about 2^-102
    const DD p = two_prod(a.hi, b.hi);
    return fast_two_sum(p.hi, p.lo + (a.hi * b.lo + a.lo * b.hi));
}

// sum over k of z^k c[k], c[k] = (-1)^k / (2k + 1)! for the sine (times r) and (-1)^k / (2k)! for the cosine: the Taylor
// series; the first terms left out, z^12 / 25! and z^13 / 26! at |r| <= pi/4 + 2^-12, are below 2^-92
RTMI_SIN_HD DD sin_series(DD z) {
    const DD c[12] = {{0x1.0000000000000p+0, 0.0},
                      {-0x1.5555555555555p-3, -0x1.5555555555555p-57},
                      {0x1.1111111111111p-7, 0x1.1111111111111p-63},
                      {-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73},
                      {0x1.71de3a556c734p-19, -0x1.c154f8ddc6c00p-73},
                      {-0x1.ae64567f544e4p-26, 0x1.c062e06d1f209p-80},
                      {0x1.6124613a86d09p-33, 0x1.f28e0cc748ebep-87},
                      {-0x1.ae7f3e733b81fp-41, -0x1.1d8656b0ee8cbp-97},
                      {0x1.952c77030ad4ap-49, 0x1.ac981465ddc6cp-103},
                      {-0x1.2f49b46814157p-57, -0x1.2650f61dbdcb4p-112},
                      {0x1.71b8ef6dcf572p-66, -0x1.d043ae40c4647p-120},
                      {-0x1.761b41316381ap-75, 0x1.3423c7d91404fp-130}};
    DD s = c[11];
    for (int k = 10; k >= 0; k--) s = dd_add(dd_mul(s, z), c[k]);
    return s;
}
RTMI_SIN_HD DD cos_series(DD z) {
    const DD c[13] = {{0x1.0000000000000p+0, 0.0},
                      {-0x1.0000000000000p-1, 0.0},
                      {0x1.5555555555555p-5, 0x1.5555555555555p-59},
                      {-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65},
                      {0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-76},
                      {-0x1.27e4fb7789f5cp-22, -0x1.cbbc05b4fa99ap-76},
                      {0x1.1eed8eff8d898p-29, -0x1.2aec959e14c06p-83},
                      {-0x1.93974a8c07c9dp-37, -0x1.05d6f8a2efd1fp-92},
                      {0x1.ae7f3e733b81fp-45, 0x1.1d8656b0ee8cbp-101},
                      {-0x1.6827863b97d97p-53, -0x1.eec01221a8b0bp-107},
                      {0x1.e542ba4020225p-62, 0x1.ea72b4afe3c2fp-120},
                      {-0x1.0ce396db7f853p-70, 0x1.aebcdbd20331cp-124},
                      {0x1.f2cf01972f578p-80, -0x1.9ada5fcc1ab14p-135}};
    DD s = c[12];
    for (int k = 11; k >= 0; k--) s = dd_add(dd_mul(s, z), c[k]);
    return s;
}

constexpr double SIN_CR_LIMIT = 0x1p40;

// sin(x) for |x| < 2^40, evaluated in double-double and rounded to nearest once.
// k = rint(x 2/pi), r = x - k pi/2 with pi/2 as four doubles (212 bits): k p1 is taken as an exact product, x - hi(k p1) is exact (Sterbenz: the two are within a factor 2 for k != 0), and the rest is
// summed in double-double, whose absolute error is 2^-104 of the largest term, 2^-13 at most.  The r of a double below
// 2^40 is never below 2^-30 or so, so r carries 90 bits or more.  |r| <= pi/4 + 2^-12 from the rounding of x 2/pi.
RTMI_SIN_HD double sin_cr(double x) {
    if (x == 0.0) return x; // keeps the sign of -0
    const double P1 = 0x1.921fb54442d18p+0, P2 = 0x1.1a62633145c07p-54, P3 = -0x1.f1976b7ed8fbcp-110, P4 = 0x1.4cf98e804177dp-164;
    const double k = ::rint(x * 0x1.45f306dc9c883p-1);
    DD r{x, 0.0};
    if (k != 0.0) {
        const DD a = two_prod(k, P1), b = two_prod(k, P2), c = two_prod(k, P3);
        r = DD{x - a.hi, 0.0};
        r = dd_add(r, two_sum(-a.lo, -b.hi));
        r = dd_add(r, two_sum(-b.lo, -c.hi));
        r = dd_add(r, two_sum(-c.lo, -(k * P4)));
    }
    const int64_t q = (int64_t)k & 3;
    const DD z = dd_mul(r, r);
    const DD s = (q & 1) ? cos_series(z) : dd_mul(r, sin_series(z));
    const double y = s.hi + s.lo;
    return (q & 2) ? -y : y;
}

} // namespace rtmi_sin64
