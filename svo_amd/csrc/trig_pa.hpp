// sin, cos and acos in plain arithmetic (+, -, *, /, sqrt and fma, each one IEEE
// operation; double-double inside), for the values that must be the same bits on
// the host and on the device: the final fit's rotation vector and Frame::pose()
// (RansacSeq::fit / pose_cam_to_world on the host, sqpnp_select_kernel on the
// device). The two maths libraries' acos / sin / cos are each within an ulp or
// two of the truth but not of each other (tests/test_sqpnp_fit_gpu.py: a mirror
// pose at |rvec| = 3.018 rad came out 1 ulp apart in every entry of rvec); these
// run the same operations on both sides. They carry ~100 bits, so the result is
// the correctly rounded one but for arguments within ~1e-30 of a rounding
// boundary -- what the host's library returns on nearly every argument.
#pragma once

#include <hip/hip_runtime.h>
#include <cmath>

namespace svo {
namespace la {
namespace pa {

#define SVO_PA __host__ __device__ inline

struct DD {
    double hi, lo;
};

SVO_PA DD two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
SVO_PA DD quick_two_sum(double a, double b) {  // |a| >= |b|
    const double s = a + b;
    return {s, b - (s - a)};
}
SVO_PA DD two_prod(double a, double b) {
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
SVO_PA DD add(DD a, DD b) {
    const DD s = two_sum(a.hi, b.hi), t = two_sum(a.lo, b.lo);
    const DD u = quick_two_sum(s.hi, s.lo + t.hi);
    return quick_two_sum(u.hi, u.lo + t.lo);
}
SVO_PA DD neg(DD a) { return {-a.hi, -a.lo}; }
SVO_PA DD mul(DD a, DD b) {
    const DD p = two_prod(a.hi, b.hi);
    return quick_two_sum(p.hi, p.lo + (a.hi * b.lo + a.lo * b.hi));
}
SVO_PA DD div_d(DD a, double b) {  // a / b for a double b
    const double q = a.hi / b;
    const DD p = two_prod(q, b);
    const double r = ((a.hi - p.hi) - p.lo) + a.lo;
    return quick_two_sum(q, r / b);
}
SVO_PA DD sqrt_dd(DD x) {  // x >= 0
    if (!(x.hi > 0)) return {0.0, 0.0};
    const double y = sqrt(x.hi);
    const DD y2 = two_prod(y, y);
    const double r = ((x.hi - y2.hi) - y2.lo) + x.lo;
    return quick_two_sum(y, r / (2 * y));
}

constexpr double kPio2a = 1.5707963267948966, kPio2b = 6.123233995736766e-17, kPio2c = -1.4973849048591698e-33;

// sin and cos of x (0 <= x <= 8) as double-doubles: x - k pi/2 with pi/2 to three
// doubles, then the Taylor series to r^27 / r^28 (|r| <= pi/4 + : below 1e-31)
SVO_PA void sincos_dd(double x, DD* sn, DD* cs) {
    const double S[13][2] = {{-0.16666666666666666, -9.25185853854297e-18}, {0.008333333333333333, 1.1564823173178714e-19},
                             {-0.0001984126984126984, -1.7209558293420705e-22}, {2.7557319223985893e-06, -1.858393274046472e-22},
                             {-2.505210838544172e-08, 1.448814070935912e-24}, {1.6059043836821613e-10, 1.2585294588752098e-26},
                             {-7.647163731819816e-13, -7.03872877733453e-30}, {2.8114572543455206e-15, 1.6508842730861433e-31},
                             {-8.22063524662433e-18, -2.2141894119604265e-34}, {1.9572941063391263e-20, -1.3643503830087908e-36},
                             {-3.868170170630684e-23, 8.843177655482344e-40}, {6.446950284384474e-26, -1.9330404233703465e-42},
                             {-9.183689863795546e-29, -1.4303150396787322e-45}};
    const double C[14][2] = {{-0.5, 0.0}, {0.041666666666666664, 2.3129646346357427e-18},
                             {-0.001388888888888889, 5.300543954373577e-20}, {2.48015873015873e-05, 2.1511947866775882e-23},
                             {-2.755731922398589e-07, -2.3767714622250297e-23}, {2.08767569878681e-09, -1.20734505911326e-25},
                             {-1.1470745597729725e-11, -2.0655512752830745e-28}, {4.779477332387385e-14, 4.399205485834081e-31},
                             {-1.5619206968586225e-16, -1.1910679660273754e-32}, {4.110317623312165e-19, 1.4412973378659527e-36},
                             {-8.896791392450574e-22, 7.911402614872376e-38}, {1.6117375710961184e-24, -3.6846573564509766e-41},
                             {-2.4795962632247976e-27, 1.2953730964765229e-43}, {3.279889237069838e-30, 1.5117542744029879e-46}};
    const int k = (int)(x * 0.6366197723675814 + 0.5);
    const DD p = two_prod((double)k, kPio2a);
    DD r = add(two_sum(x, -p.hi), DD{-p.lo, 0.0});
    r = add(r, neg(two_prod((double)k, kPio2b)));
    r = add(r, DD{-((double)k * kPio2c), 0.0});
    const DD r2 = mul(r, r);
    DD ps{S[12][0], S[12][1]}, pc{C[13][0], C[13][1]};
    for (int i = 11; i >= 0; i--) ps = add(mul(ps, r2), DD{S[i][0], S[i][1]});
    for (int i = 12; i >= 0; i--) pc = add(mul(pc, r2), DD{C[i][0], C[i][1]});
    const DD s = add(r, mul(mul(ps, r2), r));  // r + r^3 (..)
    const DD c = add(DD{1.0, 0.0}, mul(pc, r2));
    switch (k & 3) {
        case 0: *sn = s, *cs = c; break;
        case 1: *sn = c, *cs = neg(s); break;
        case 2: *sn = neg(s), *cs = neg(c); break;
        default: *sn = neg(c), *cs = s; break;
    }
}

// sin(x), cos(x) rounded to double; outside [0, 8] (no rotation vector of a fit
// is that long: rodrigues_inv returns at most pi) the library's
SVO_PA void sincos(double x, double* sn, double* cs) {
    if (!(x >= 0 && x <= 8)) {
        *sn = sin(x);
        *cs = cos(x);
        return;
    }
    DD s, c;
    sincos_dd(x, &s, &c);
    *sn = s.hi + s.lo;
    *cs = c.hi + c.lo;
}

// acos(c), -1 <= c <= 1, rounded to double: h with sin h = sqrt((1 - |c|) / 2), 0 <=
// h <= pi/4 (Newton from a series start: the error squares each step down to the
// double-double's), acos |c| = 2 h, and pi - 2 h for c < 0
SVO_PA double acos(double c) {
    if (c != c) return c;
    const double a = fabs(c);
    if (a >= 1) return c > 0 ? 0.0 : 2 * kPio2a;
    const DD om = two_sum(1.0, -a);  // exact
    const DD q = sqrt_dd(DD{0.5 * om.hi, 0.5 * om.lo});
    const double q2 = q.hi * q.hi;
    DD h{q.hi * (1 + q2 * (1.0 / 6 + q2 * (3.0 / 40 + q2 * (15.0 / 336)))), 0.0};
    for (int it = 0; it < 5; it++) {
        DD s, cs;
        sincos_dd(h.hi, &s, &cs);
        // sin(h.hi + h.lo) = s + h.lo cs (h.lo below 1e-16 of h: the next term is below 1e-32)
        const DD sh = add(s, mul(cs, DD{h.lo, 0.0}));
        const DD d = div_d(add(q, neg(sh)), cs.hi);
        h = add(h, d);
    }
    DD th{2 * h.hi, 2 * h.lo};
    if (c < 0) {
        const DD pi = add(DD{2 * kPio2a, 2 * kPio2b}, DD{2 * kPio2c, 0.0});
        th = add(pi, neg(th));
    }
    return th.hi + th.lo;
}

#undef SVO_PA

}  // namespace pa
}  // namespace la
}  // namespace svo
