// chx_dual2.h — a second-order dual number for chx_dkd_ring_sensitivity (Segment.ring_sensitivity): the value, two first-order
// parts and the mixed part, x = v + a e1 + b e2 + ab e1 e2 with e1^2 = e2^2 = 0. A drift-kick-drift map evaluated in Dual2 with
// e1 along a phase-space direction and e2 along a setting gives the map (v), a column of its Jacobian (a), its derivative with
// respect to the setting (b) and the derivative of that column with respect to the setting (ab) in one walk.
// Everything chx_dual.h has for Dual, __host__ __device__ (tests/host/dual2_check.hip runs all of it without a GPU). The value
// and the first-order parts are the operations of Dual in Dual's order, so v and a (and b) carry the bits a Dual evaluation gives.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "chx_dual.h"

struct Dual2 {
    double v, a, b, ab;
};
#define CHX_D2 __host__ __device__ __forceinline__
CHX_D2 Dual2 mk2(double v, double a, double b, double ab) { Dual2 r; r.v = v; r.a = a; r.b = b; r.ab = ab; return r; }
// f(x) from f, f' and f'' at x.v, for the functions whose Dual form is f' * x.d
CHX_D2 Dual2 chain2(Dual2 x, double f0, double f1, double f2) { return mk2(f0, f1 * x.a, f1 * x.b, f1 * x.ab + f2 * (x.a * x.b)); }

CHX_D2 Dual2 operator+(Dual2 x, Dual2 y) { return mk2(x.v + y.v, x.a + y.a, x.b + y.b, x.ab + y.ab); }
CHX_D2 Dual2 operator-(Dual2 x, Dual2 y) { return mk2(x.v - y.v, x.a - y.a, x.b - y.b, x.ab - y.ab); }
CHX_D2 Dual2 operator*(Dual2 x, Dual2 y) {
    return mk2(x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b, (x.ab * y.v + x.v * y.ab) + (x.a * y.b + x.b * y.a));
}
CHX_D2 Dual2 operator/(Dual2 x, Dual2 y) {      // x = q y: x.ab = q.ab y.v + q.a y.b + q.b y.a + q.v y.ab
    const double q = x.v / y.v;
    const double qa = (x.a - q * y.a) / y.v, qb = (x.b - q * y.b) / y.v;
    return mk2(q, qa, qb, (x.ab - q * y.ab - (qa * y.b + qb * y.a)) / y.v);
}
CHX_D2 Dual2 operator-(Dual2 x) { return mk2(-x.v, -x.a, -x.b, -x.ab); }
CHX_D2 Dual2 operator+(Dual2 x, double y) { return mk2(x.v + y, x.a, x.b, x.ab); }
CHX_D2 Dual2 operator+(double x, Dual2 y) { return mk2(x + y.v, y.a, y.b, y.ab); }
CHX_D2 Dual2 operator-(Dual2 x, double y) { return mk2(x.v - y, x.a, x.b, x.ab); }
CHX_D2 Dual2 operator-(double x, Dual2 y) { return mk2(x - y.v, -y.a, -y.b, -y.ab); }
CHX_D2 Dual2 operator*(Dual2 x, double y) { return mk2(x.v * y, x.a * y, x.b * y, x.ab * y); }
CHX_D2 Dual2 operator*(double x, Dual2 y) { return mk2(x * y.v, x * y.a, x * y.b, x * y.ab); }
CHX_D2 Dual2 operator/(Dual2 x, double y) { return mk2(x.v / y, x.a / y, x.b / y, x.ab / y); }
CHX_D2 Dual2 operator/(double x, Dual2 y) {     // q y = x: 0 = q.ab y.v + q.a y.b + q.b y.a + q.v y.ab
    const double q = x / y.v;
    const double qa = -q * y.a / y.v, qb = -q * y.b / y.v;
    return mk2(q, qa, qb, (-q * y.ab - (qa * y.b + qb * y.a)) / y.v);
}

CHX_D2 double val(Dual2 x) { return x.v; }
CHX_D2 double tan_of(Dual2 x) { return x.a; }
template <> __device__ __forceinline__ Dual2 cst<Dual2>(double c) { return mk2(c, 0.0, 0.0, 0.0); }   // (the primary's attributes)

CHX_D2 Dual2 m_sqrt(Dual2 x) {                  // s s = x: 2 s s.ab + 2 s.a s.b = x.ab
    const double s = sqrt(x.v);
    const double sa = 0.5 * x.a / s, sb = 0.5 * x.b / s;
    return mk2(s, sa, sb, (0.5 * x.ab - sa * sb) / s);
}
CHX_D2 Dual2 m_sin(Dual2 x) { const double s = sin(x.v), c = cos(x.v); return chain2(x, s, c, -s); }
CHX_D2 Dual2 m_cos(Dual2 x) { const double s = sin(x.v), c = cos(x.v); return chain2(x, c, -s, -c); }
CHX_D2 Dual2 m_tan(Dual2 x) { const double t = tan(x.v), f1 = 1.0 + t * t; return chain2(x, t, f1, 2.0 * t * f1); }
CHX_D2 Dual2 m_sinh(Dual2 x) { const double s = sinh(x.v), c = cosh(x.v); return chain2(x, s, c, s); }
CHX_D2 Dual2 m_cosh(Dual2 x) { const double s = sinh(x.v), c = cosh(x.v); return chain2(x, c, s, c); }
CHX_D2 Dual2 m_log1p(Dual2 x) {
    const double p = 1.0 + x.v;
    const double la = x.a / p, lb = x.b / p;
    return mk2(log1p(x.v), la, lb, x.ab / p - la * lb);
}
CHX_D2 Dual2 m_asin(Dual2 x) {                  // f' = 1 / r, f'' = v / r^3 with r = sqrt(1 - v^2)
    const double r = sqrt(1.0 - x.v * x.v);
    const double fa = x.a / r, fb = x.b / r;
    return mk2(asin(x.v), fa, fb, x.ab / r + x.v * (fa * fb) / r);
}
CHX_D2 Dual2 m_atan2(Dual2 y, Dual2 x) {
    const double r2 = x.v * x.v + y.v * y.v;
    const double ta = (x.v * y.a - y.v * x.a) / r2, tb = (x.v * y.b - y.v * x.b) / r2;
    // d/de2 of (x y.a - y x.a) / r2: the numerator's e2 part over r2, less ta times r2's e2 part over r2
    const double num = (x.v * y.ab - y.v * x.ab) + (x.b * y.a - y.b * x.a);
    const double r2b = 2.0 * (x.v * x.b + y.v * y.b);
    return mk2(atan2(y.v, x.v), ta, tb, (num - ta * r2b) / r2);
}
CHX_D2 Dual2 m_atan(Dual2 x) {                  // f' = 1 / p, f'' = -2 v / p^2 with p = 1 + v^2
    const double p = 1.0 + x.v * x.v;
    const double fa = x.a / p, fb = x.b / p;
    return mk2(atan(x.v), fa, fb, x.ab / p - 2.0 * x.v * (fa * fb));
}
CHX_D2 Dual2 m_asinh(Dual2 x) {                 // f' = 1 / r, f'' = -v / r^3 with r = sqrt(1 + v^2)
    const double r = sqrt(1.0 + x.v * x.v);
    const double fa = x.a / r, fb = x.b / r;
    return mk2(asinh(x.v), fa, fb, x.ab / r - x.v * (fa * fb) / r);
}
// Dual's convention: sign(0) = 0
CHX_D2 Dual2 m_abs(Dual2 x) { return x.v < 0.0 ? -x : (x.v > 0.0 ? x : mk2(0.0, 0.0, 0.0, 0.0)); }
// ---- the Dual2 forms of the two closed forms that csrc/chx_nonlinear.hip gives Dual by name --------------------------------------
// cos(sqrt(w) len) and sin(sqrt(w) len) / sqrt(w) by their series inside |w len^2| < 1e-4 (quad_cs_series of chx_nonlinear.hip)
CHX_D2 bool quad_cs_series(Dual2 w, Dual2 len, Dual2& cx, Dual2& sx) {
    const Dual2 u = w * len * len;
    if (!(fabs(u.v) < 1e-4)) return false;
    cx = 1.0 - u * (1.0 / 2.0 - u * (1.0 / 24.0 - u * (1.0 / 720.0 - u * (1.0 / 40320.0))));
    sx = len * (1.0 - u * (1.0 / 6.0 - u * (1.0 / 120.0 - u * (1.0 / 5040.0 - u * (1.0 / 362880.0)))));
    return true;
}
// (sqrt(a^2 + b) - a) / b = 1 / (2a) - b / (8a^3) + b^2 / (16a^5) - ...: at b == 0 g_aa = 1 / a^3, g_ab = 3 / (8a^4), g_bb = 1 / (8a^5)
CHX_D2 Dual2 sqrta2minusbdiva(Dual2 a, Dual2 b) {
    if (b.v != 0.0) return (m_sqrt(a * a + b) - a) / b;
    const double a2 = a.v * a.v, a3 = a2 * a.v;
    return mk2(1.0 / (2.0 * a.v), -a.a / (2.0 * a.v * a.v) - b.a / (8.0 * a.v * a.v * a.v), -a.b / (2.0 * a.v * a.v) - b.b / (8.0 * a.v * a.v * a.v),
               -a.ab / (2.0 * a2) - b.ab / (8.0 * a3) + a.a * a.b / a3 + 3.0 * (a.a * b.b + a.b * b.a) / (8.0 * a2 * a2) +
                   b.a * b.b / (8.0 * a3 * a2));
}
#undef CHX_D2
