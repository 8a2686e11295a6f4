// dual2_check.hip — csrc/chx_dual2.h and the (seed, knob) parts of csrc/chx_optics_dev.h without a GPU, under the address and
// undefined-behaviour sanitizers:
//   hipcc --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all
//         -I cheetah_amd/csrc -o dual2_check tests/host/dual2_check.hip
//  * every Dual2 operator and function, and the two closed forms with a Dual2 form of their own, at drawn arguments: all four
//    parts against closed forms in long double, the value and
//    both first-order parts bit for bit against Dual (whose device-only functions are compiled for the host here as well);
//  * the lane maps of chx_dkd_ring_sensitivity and the system of the orbit's derivative against a long-double elimination.
// Prints one "<part>: ok" line per part and returns 0, or says what failed and returns 1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// chx_dual.h marks Dual's functions __device__ only: for this program, and nowhere else, they are host functions too
#undef __device__
#define __device__ __attribute__((device)) __attribute__((host))
#include "chx_dual2.h"
#include "chx_optics_dev.h"

using namespace chx_optics;
typedef long double ld;

static int failures = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAILED: ");      \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            ++failures;                   \
        }                                 \
    } while (0)

static unsigned long long rng_state = 12345;
static double uniform(double lo, double hi) {   // a fixed linear congruential sequence
    rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return lo + (hi - lo) * ((double)(rng_state >> 11) * 0x1p-53);
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct L4 {
    ld v, a, b, ab;
};
// |got - want| <= 64 * 2^-52 * (the sum of the absolute terms the part is made of): a handful of roundings per term
static void expect_close(const char* what, Dual2 got, L4 want, L4 scale) {
    const ld eps = 64 * 0x1p-52L;
    EXPECT(fabsl(got.v - want.v) <= eps * scale.v, "%s value %.17g want %.17Lg", what, got.v, want.v);
    EXPECT(fabsl(got.a - want.a) <= eps * scale.a, "%s e1 part %.17g want %.17Lg", what, got.a, want.a);
    EXPECT(fabsl(got.b - want.b) <= eps * scale.b, "%s e2 part %.17g want %.17Lg", what, got.b, want.b);
    EXPECT(fabsl(got.ab - want.ab) <= eps * scale.ab, "%s mixed part %.17g want %.17Lg (scale %.3Lg)", what, got.ab, want.ab, scale.ab);
}
// the value and each first-order part are what Dual gives for (v, that part)
static void expect_bits(const char* what, Dual2 got, Dual with_a, Dual with_b) {
    EXPECT(same_bits(got.v, with_a.v) && same_bits(got.v, with_b.v), "%s value bits %.17g vs Dual %.17g", what, got.v, with_a.v);
    EXPECT(same_bits(got.a, with_a.d), "%s e1 bits %.17g vs Dual %.17g", what, got.a, with_a.d);
    EXPECT(same_bits(got.b, with_b.d), "%s e2 bits %.17g vs Dual %.17g", what, got.b, with_b.d);
}
static Dual2 draw(double lo, double hi) { return mk2(uniform(lo, hi), uniform(-2, 2), uniform(-2, 2), uniform(-2, 2)); }
static Dual da(Dual2 x) { return mk(x.v, x.a); }
static Dual db(Dual2 x) { return mk(x.v, x.b); }

struct Unary {
    const char* name;
    Dual2 (*f2)(Dual2);
    Dual (*f1)(Dual);
    ld (*d0)(ld);
    ld (*d1)(ld);
    ld (*d2)(ld);
    double lo, hi;
};
static const Unary unary[] = {
    {"sqrt", m_sqrt, m_sqrt, [](ld x) { return sqrtl(x); }, [](ld x) { return 0.5L / sqrtl(x); }, [](ld x) { return -0.25L / (x * sqrtl(x)); }, 0.1, 9.0},
    {"sin", m_sin, m_sin, [](ld x) { return sinl(x); }, [](ld x) { return cosl(x); }, [](ld x) { return -sinl(x); }, -3.0, 3.0},
    {"cos", m_cos, m_cos, [](ld x) { return cosl(x); }, [](ld x) { return -sinl(x); }, [](ld x) { return -cosl(x); }, -3.0, 3.0},
    {"tan", m_tan, m_tan, [](ld x) { return tanl(x); }, [](ld x) { return 1 + tanl(x) * tanl(x); },
     [](ld x) { return 2 * tanl(x) * (1 + tanl(x) * tanl(x)); }, -1.2, 1.2},
    {"sinh", m_sinh, m_sinh, [](ld x) { return sinhl(x); }, [](ld x) { return coshl(x); }, [](ld x) { return sinhl(x); }, -2.0, 2.0},
    {"cosh", m_cosh, m_cosh, [](ld x) { return coshl(x); }, [](ld x) { return sinhl(x); }, [](ld x) { return coshl(x); }, -2.0, 2.0},
    {"log1p", m_log1p, m_log1p, [](ld x) { return log1pl(x); }, [](ld x) { return 1 / (1 + x); }, [](ld x) { return -1 / ((1 + x) * (1 + x)); }, -0.5, 3.0},
    {"asin", m_asin, m_asin, [](ld x) { return asinl(x); }, [](ld x) { return 1 / sqrtl(1 - x * x); },
     [](ld x) { return x / ((1 - x * x) * sqrtl(1 - x * x)); }, -0.9, 0.9},
    {"atan", m_atan, m_atan, [](ld x) { return atanl(x); }, [](ld x) { return 1 / (1 + x * x); },
     [](ld x) { return -2 * x / ((1 + x * x) * (1 + x * x)); }, -4.0, 4.0},
    {"asinh", m_asinh, m_asinh, [](ld x) { return asinhl(x); }, [](ld x) { return 1 / sqrtl(1 + x * x); },
     [](ld x) { return -x / ((1 + x * x) * sqrtl(1 + x * x)); }, -4.0, 4.0},
    {"abs", m_abs, m_abs, [](ld x) { return fabsl(x); }, [](ld x) { return x < 0 ? -1.0L : (x > 0 ? 1.0L : 0.0L); }, [](ld) { return 0.0L; }, -3.0, 3.0},
    {"negate", [](Dual2 x) { return -x; }, [](Dual x) { return -x; }, [](ld x) { return -x; }, [](ld) { return -1.0L; }, [](ld) { return 0.0L; }, -3.0, 3.0},
};

static void check_unary() {
    for (const Unary& u : unary) {
        for (int t = 0; t < 200; ++t) {
            const Dual2 x = draw(u.lo, u.hi);
            const Dual2 got = u.f2(x);
            const ld f0 = u.d0(x.v), f1 = u.d1(x.v), f2 = u.d2(x.v);
            const L4 want{f0, f1 * x.a, f1 * x.b, f1 * x.ab + f2 * (ld)x.a * x.b};
            // the libm value may be a few units off the long-double one; the scale of a part is the sum of its terms
            const L4 scale{fabsl(f0) + 1e-300L, fabsl(f1 * x.a), fabsl(f1 * x.b), fabsl(f1 * x.ab) + fabsl(f2 * x.a * x.b)};
            expect_close(u.name, got, want, scale);
            expect_bits(u.name, got, u.f1(da(x)), u.f1(db(x)));
        }
        // abs at 0: Dual's convention, all parts 0
    }
    const Dual2 z = m_abs(mk2(0.0, 1.0, 2.0, 3.0));
    EXPECT(z.v == 0 && z.a == 0 && z.b == 0 && z.ab == 0, "abs at 0");
    std::printf("unary functions: ok\n");
}

static void check_binary() {
    for (int t = 0; t < 400; ++t) {
        const Dual2 x = draw(-3, 3);
        Dual2 y = draw(0.3, 3);
        if (t & 1) y = -y;
        const double s = (t & 2) ? uniform(0.3, 3) : -uniform(0.3, 3);
        const ld xv = x.v, xa = x.a, xb = x.b, xab = x.ab, yv = y.v, ya = y.a, yb = y.b, yab = y.ab;
        expect_close("add", x + y, {xv + yv, xa + ya, xb + yb, xab + yab}, {fabsl(xv) + fabsl(yv), fabsl(xa) + fabsl(ya), fabsl(xb) + fabsl(yb), fabsl(xab) + fabsl(yab)});
        expect_close("sub", x - y, {xv - yv, xa - ya, xb - yb, xab - yab}, {fabsl(xv) + fabsl(yv), fabsl(xa) + fabsl(ya), fabsl(xb) + fabsl(yb), fabsl(xab) + fabsl(yab)});
        expect_close("mul", x * y, {xv * yv, xa * yv + xv * ya, xb * yv + xv * yb, xab * yv + xa * yb + xb * ya + xv * yab},
                     {fabsl(xv * yv), fabsl(xa * yv) + fabsl(xv * ya), fabsl(xb * yv) + fabsl(xv * yb),
                      fabsl(xab * yv) + fabsl(xa * yb) + fabsl(xb * ya) + fabsl(xv * yab)});
        {   // x / y = x * r with r = 1 / y: r' = -1 / y^2, r'' = 2 / y^3
            const ld r = 1 / yv, ra = -ya / (yv * yv), rb = -yb / (yv * yv), rab = -yab / (yv * yv) + 2 * ya * yb / (yv * yv * yv);
            const L4 want{xv * r, xa * r + xv * ra, xb * r + xv * rb, xab * r + xa * rb + xb * ra + xv * rab};
            const L4 scale{fabsl(xv * r), fabsl(xa * r) + fabsl(xv * ra), fabsl(xb * r) + fabsl(xv * rb),
                           fabsl(xab * r) + fabsl(xa * rb) + fabsl(xb * ra) + fabsl(xv * yab / (yv * yv)) + fabsl(2 * xv * ya * yb / (yv * yv * yv))};
            expect_close("div", x / y, want, scale);
            expect_close("double / Dual2", s / y, {s * r, s * ra, s * rb, s * rab},
                         {fabsl(s * r), fabsl(s * ra), fabsl(s * rb), fabsl(s * yab / (yv * yv)) + fabsl(2 * s * ya * yb / (yv * yv * yv))});
        }
        expect_close("Dual2 + double", x + s, {xv + s, xa, xb, xab}, {fabsl(xv) + fabsl((ld)s), fabsl(xa), fabsl(xb), fabsl(xab)});
        expect_close("double + Dual2", s + x, {xv + s, xa, xb, xab}, {fabsl(xv) + fabsl((ld)s), fabsl(xa), fabsl(xb), fabsl(xab)});
        expect_close("Dual2 - double", x - s, {xv - s, xa, xb, xab}, {fabsl(xv) + fabsl((ld)s), fabsl(xa), fabsl(xb), fabsl(xab)});
        expect_close("double - Dual2", s - x, {s - xv, -xa, -xb, -xab}, {fabsl(xv) + fabsl((ld)s), fabsl(xa), fabsl(xb), fabsl(xab)});
        expect_close("Dual2 * double", x * s, {xv * s, xa * s, xb * s, xab * s}, {fabsl(xv * s), fabsl(xa * s), fabsl(xb * s), fabsl(xab * s)});
        expect_close("double * Dual2", s * x, {xv * s, xa * s, xb * s, xab * s}, {fabsl(xv * s), fabsl(xa * s), fabsl(xb * s), fabsl(xab * s)});
        expect_close("Dual2 / double", x / s, {xv / s, xa / s, xb / s, xab / s}, {fabsl(xv / s), fabsl(xa / s), fabsl(xb / s), fabsl(xab / s)});
        expect_bits("add", x + y, da(x) + da(y), db(x) + db(y));
        expect_bits("sub", x - y, da(x) - da(y), db(x) - db(y));
        expect_bits("mul", x * y, da(x) * da(y), db(x) * db(y));
        expect_bits("div", x / y, da(x) / da(y), db(x) / db(y));
        expect_bits("Dual2 + double", x + s, da(x) + s, db(x) + s);
        expect_bits("double + Dual2", s + x, s + da(x), s + db(x));
        expect_bits("Dual2 - double", x - s, da(x) - s, db(x) - s);
        expect_bits("double - Dual2", s - x, s - da(x), s - db(x));
        expect_bits("Dual2 * double", x * s, da(x) * s, db(x) * s);
        expect_bits("double * Dual2", s * x, s * da(x), s * db(x));
        expect_bits("Dual2 / double", x / s, da(x) / s, db(x) / s);
        expect_bits("double / Dual2", s / y, s / da(y), s / db(y));
        {   // atan2(p, q): t_p = q / r2, t_q = -p / r2, t_pp = -2 p q / r2^2 = -t_qq, t_pq = (p^2 - q^2) / r2^2
            const Dual2 p = x, q = y;
            const ld r2 = xv * xv + yv * yv;
            const ld tp = yv / r2, tq = -xv / r2, tpp = -2 * xv * yv / (r2 * r2), tpq = (xv * xv - yv * yv) / (r2 * r2);
            const L4 want{atan2l(xv, yv), tp * xa + tq * ya, tp * xb + tq * yb,
                          tp * xab + tq * yab + tpp * xa * xb - tpp * ya * yb + tpq * (xa * yb + xb * ya)};
            const L4 scale{fabsl(want.v) + 1e-300L, fabsl(tp * xa) + fabsl(tq * ya), fabsl(tp * xb) + fabsl(tq * yb),
                           // (the terms of the quotient rule the code adds up: products of two first-order parts over r2)
                           fabsl(tp * xab) + fabsl(tq * yab) + (fabsl(xa * xb) + fabsl(ya * yb) + fabsl(xa * yb) + fabsl(xb * ya)) / r2};
            expect_close("atan2", m_atan2(p, q), want, scale);
            expect_bits("atan2", m_atan2(p, q), m_atan2(da(p), da(q)), m_atan2(db(p), db(q)));
        }
    }
    const Dual2 c = cst<Dual2>(2.5);
    EXPECT(c.v == 2.5 && c.a == 0 && c.b == 0 && c.ab == 0 && val(c) == 2.5 && tan_of(mk2(1, 2, 3, 4)) == 2.0, "cst, val, tan_of");
    std::printf("operators, atan2, cst, val, tan_of: ok\n");
}

// chx_nonlinear.hip's Dual form of the b == 0 limit (a copy: the original stands among device code that this program cannot include)
static Dual sqrta2minusbdiva_dual(Dual a, Dual b) { return mk(1.0 / (2.0 * a.v), -a.d / (2.0 * a.v * a.v) - b.d / (8.0 * a.v * a.v * a.v)); }

// the two closed forms csrc/chx_nonlinear.hip treats by name. sqrta2minusbdiva against the derivatives of its own power series
// g = sum k_n b^n / a^(2n + 1), k = 1/2, -1/8, 1/16, -5/128, 7/256 (the binomial series of sqrt(1 + x)), at b == 0 — the branch of
// limits; quad_cs_series against cos(k len) and sin(k len) / k, k = sqrt(w), at w == 0 and
// inside the series' range, e1 along w and e2 along len
static void check_named_forms() {
    const ld kn[5] = {0.5L, -0.125L, 0.0625L, -5.0L / 128, 7.0L / 256};
    for (int t = 0; t < 300; ++t) {
        const Dual2 a = draw(0.8, 3.0);
        Dual2 b = draw(-1e-3, 1e-3);
        b.v = 0.0;                                // (b != 0 is made of the operators checked above)
        const Dual2 got = sqrta2minusbdiva(a, b);
        ld g = 0, ga = 0, gb = 0, gaa = 0, gab = 0, gbb = 0;
        for (int n = 0; n < 5; ++n) {
            const ld p = 2 * n + 1, c = kn[n] * powl(a.v, -p), ca = -p * kn[n] * powl(a.v, -p - 1), caa = p * (p + 1) * kn[n] * powl(a.v, -p - 2);
            const ld bn = powl(b.v, n), bn1 = n >= 1 ? n * powl(b.v, n - 1) : 0, bn2 = n >= 2 ? n * (n - 1) * powl(b.v, n - 2) : 0;
            g += c * bn, ga += ca * bn, gb += c * bn1, gaa += caa * bn, gab += ca * bn1, gbb += c * bn2;
        }
        const L4 want{g, ga * a.a + gb * b.a, ga * a.b + gb * b.b,
                      ga * a.ab + gb * b.ab + gaa * a.a * a.b + gab * ((ld)a.a * b.b + (ld)a.b * b.a) + gbb * b.a * b.b};
        const ld loose = 64 * 0x1p-52L * 8;       // (parts of order one to eight)
        EXPECT(fabsl(got.v - want.v) <= loose && fabsl(got.a - want.a) <= loose * 10 && fabsl(got.b - want.b) <= loose * 10 &&
                   fabsl(got.ab - want.ab) <= loose * 100,
               "sqrta2minusbdiva at a = %.17g, b = %.17g: (%.17g %.17g %.17g %.17g) want (%.17Lg %.17Lg %.17Lg %.17Lg)", a.v, b.v, got.v, got.a, got.b,
               got.ab, want.v, want.a, want.b, want.ab);
        if (b.v == 0.0) expect_bits("sqrta2minusbdiva", got, sqrta2minusbdiva_dual(da(a), da(b)), sqrta2minusbdiva_dual(db(a), db(b)));
    }
    for (int t = 0; t < 200; ++t) {
        const double w0 = t % 4 == 0 ? 0.0 : uniform(1e-6, 9e-3), l0 = uniform(0.02, 0.1);       // u = w len^2 < 1e-4
        Dual2 cx, sx;
        EXPECT(quad_cs_series(mk2(w0, 1.0, 0.0, 0.0), mk2(l0, 0.0, 1.0, 0.0), cx, sx), "the series refuses u = %.3g", w0 * l0 * l0);
        const ld L = l0, k = sqrtl((ld)w0), S = sinl(k * L), C = cosl(k * L);
        L4 wc, ws;
        if (w0 == 0.0) {
            wc = {1, -L * L / 2, 0, -L};
            ws = {L, -L * L * L / 6, 1, -L * L / 2};
        } else {
            wc = {C, -L * S / (2 * k), -k * S, -(S + k * L * C) / (2 * k)};
            ws = {S / k, (L * C - S / k) / (2 * w0), C, -L * S / (2 * k)};
        }
        const ld tol = 1e-12L;                    // (the series' first term left out: u^5 / 10!)
        EXPECT(fabsl(cx.v - wc.v) <= tol && fabsl(cx.a - wc.a) <= tol && fabsl(cx.b - wc.b) <= tol && fabsl(cx.ab - wc.ab) <= tol,
               "quad_cs_series cx at w = %.3g, len = %.3g: mixed %.17g want %.17Lg", w0, l0, cx.ab, wc.ab);
        EXPECT(fabsl(sx.v - ws.v) <= tol && fabsl(sx.a - ws.a) <= tol && fabsl(sx.b - ws.b) <= tol && fabsl(sx.ab - ws.ab) <= tol,
               "quad_cs_series sx at w = %.3g, len = %.3g: mixed %.17g want %.17Lg", w0, l0, sx.ab, ws.ab);
    }
    Dual2 cx, sx;
    EXPECT(!quad_cs_series(mk2(1.0, 0, 0, 0), mk2(0.1, 0, 0, 0), cx, sx), "the series takes u = 1e-2");
    std::printf("named closed forms: ok\n");
}

// a composition as the maps make them, against the long-double second derivative by closed form:
// f(p, t) = sqrt(1 + p^2) * sin(t p) / (1 + t): d2 f / dp dt in the mixed part for e1 = p, e2 = t
static void check_composition() {
    for (int t = 0; t < 200; ++t) {
        const double p0 = uniform(-1.5, 1.5), t0 = uniform(0.2, 2.0);
        const Dual2 p = mk2(p0, 1.0, 0.0, 0.0), th = mk2(t0, 0.0, 1.0, 0.0);
        const Dual2 f = m_sqrt(1.0 + p * p) * m_sin(th * p) / (1.0 + th);
        const ld P = p0, T = t0, R = sqrtl(1 + P * P), S = sinl(T * P), C = cosl(T * P);
        const ld f_p = (P / R * S + R * T * C) / (1 + T);
        const ld f_t = R * P * C / (1 + T) - R * S / ((1 + T) * (1 + T));
        const ld f_pt = (P / R * P * C + R * C - R * T * P * S) / (1 + T) - (P / R * S + R * T * C) / ((1 + T) * (1 + T));
        const ld tol = 256 * 0x1p-52L * (1 + fabsl(f_pt));
        EXPECT(fabsl(f.v - R * S / (1 + T)) <= tol && fabsl(f.a - f_p) <= tol && fabsl(f.b - f_t) <= tol && fabsl(f.ab - f_pt) <= tol,
               "composition at p = %.17g, t = %.17g: mixed %.17g want %.17Lg", p0, t0, f.ab, f_pt);
    }
    std::printf("composition: ok\n");
}

static void check_lane_maps() {
    const int64_t Bs[] = {1, 2, 9, 64}, Ks[] = {1, 3, 9, 17, 100};
    for (int64_t B : Bs)
        for (int64_t K : Ks) {
            const int64_t wgs = pair_workgroups(B, K);
            EXPECT(wgs * kSeeds >= B * K && (wgs - 1) * kSeeds < B * K, "pair_workgroups(%lld, %lld) = %lld", (long long)B, (long long)K, (long long)wgs);
            std::vector<int> seen((size_t)(B * K), 0);
            for (int64_t wg = 0; wg < wgs; ++wg)
                for (int lane = 0; lane < kLanes; ++lane) {
                    bool live;
                    int64_t seed, knob;
                    pair_of_group(wg, group_of_lane(lane), B, K, live, seed, knob);
                    EXPECT(seed >= 0 && seed < B && knob >= 0 && knob < K, "pair_of_group out of range at B = %lld, K = %lld", (long long)B, (long long)K);
                    if (seed < 0 || seed >= B || knob < 0 || knob >= K) continue;
                    const int64_t pair = wg * kSeeds + group_of_lane(lane);
                    EXPECT(live == (pair < B * K), "live flag of pair %lld", (long long)pair);
                    if (live) {
                        EXPECT(seed * K + knob == pair, "pair %lld maps to (%lld, %lld)", (long long)pair, (long long)seed, (long long)knob);
                        if (tangent_of_lane(lane) == 0) ++seen[(size_t)(seed * K + knob)];
                    } else {
                        EXPECT(seed == B - 1 && knob == K - 1, "a group past the end does not repeat the last pair");
                    }
                }
            for (int64_t i = 0; i < B * K; ++i) EXPECT(seen[(size_t)i] == 1, "pair %lld is worked on %d times", (long long)i, seen[(size_t)i]);
        }
    std::printf("lane maps: ok\n");
}

// Gaussian elimination with complete pivoting in long double
static bool reference_solve(int n, std::vector<ld> a, std::vector<ld> b, std::vector<ld>& x) {
    std::vector<int> col(n);
    for (int i = 0; i < n; ++i) col[i] = i;
    for (int k = 0; k < n; ++k) {
        int pr = k, pc = k;
        ld big = 0;
        for (int r = k; r < n; ++r)
            for (int c = k; c < n; ++c)
                if (fabsl(a[r * n + c]) > big) big = fabsl(a[r * n + c]), pr = r, pc = c;
        if (big == 0) return false;
        for (int c = 0; c < n; ++c) std::swap(a[k * n + c], a[pr * n + c]);
        std::swap(b[k], b[pr]);
        for (int r = 0; r < n; ++r) std::swap(a[r * n + k], a[r * n + pc]);
        std::swap(col[k], col[pc]);
        for (int r = k + 1; r < n; ++r) {
            const ld f = a[r * n + k] / a[k * n + k];
            for (int c = k; c < n; ++c) a[r * n + c] -= f * a[k * n + c];
            b[r] -= f * b[k];
        }
    }
    std::vector<ld> y(n);
    for (int k = n - 1; k >= 0; --k) {
        ld s = b[k];
        for (int c = k + 1; c < n; ++c) s -= a[k * n + c] * y[c];
        y[k] = s / a[k * n + k];
    }
    x.assign(n, 0);
    for (int k = 0; k < n; ++k) x[col[k]] = y[k];
    return true;
}

static void check_orbit_sensitivity() {
    for (int mode = 1; mode <= 2; ++mode) {
        const int n = closed_count(mode);
        for (int t = 0; t < 100; ++t) {
            double M[36], dfdt[6], a[36], w[6];
            for (double& m : M) m = uniform(-1, 1);
            for (double& f : dfdt) f = uniform(-1, 1);
            std::vector<ld> A((size_t)(n * n)), rhs((size_t)n), want;
            for (int i = 0; i < n; ++i) {
                for (int m = 0; m < n; ++m) A[(size_t)(i * n + m)] = (i == m ? 1.0L : 0.0L) - M[i * 6 + m];
                rhs[(size_t)i] = dfdt[i];
            }
            EXPECT(reference_solve(n, A, rhs, want), "the reference could not solve a drawn system");
            const bool ok = orbit_sensitivity(n, M, dfdt, a, w);
            // the residual in long double, against n 2^-52 |A| |w| times a growth of 64 (partial pivoting on drawn matrices)
            ld worst = 0, size = 0;
            for (int i = 0; i < n; ++i) {
                ld r = -rhs[(size_t)i], s = fabsl(rhs[(size_t)i]);
                for (int m = 0; m < n; ++m) r += A[(size_t)(i * n + m)] * w[m], s += fabsl(A[(size_t)(i * n + m)] * w[m]);
                worst = fmaxl(worst, fabsl(r));
                size = fmaxl(size, s);
            }
            EXPECT(ok && worst <= 64 * n * 0x1p-52L * size, "orbit_sensitivity residual %.3Lg against %.3Lg", worst, 64 * n * 0x1p-52L * size);
            for (int i = n; i < 6; ++i) EXPECT(w[i] == 0.0, "a held coordinate moves");
            (void)want;
        }
        // M_n = I: no closed orbit's derivative, NaN on the closed coordinates and 0 on the held ones
        double M[36] = {0}, dfdt[6] = {1, 1, 1, 1, 1, 1}, a[36], w[6];
        for (int i = 0; i < 6; ++i) M[i * 6 + i] = 1.0;
        EXPECT(!orbit_sensitivity(n, M, dfdt, a, w), "a singular system is solved");
        for (int i = 0; i < 6; ++i) EXPECT(i < n ? w[i] != w[i] : w[i] == 0.0, "singular system: coordinate %d", i);
    }
    std::printf("orbit sensitivity system: ok\n");
}

int main() {
    check_unary();
    check_binary();
    check_composition();
    check_named_forms();
    check_lane_maps();
    check_orbit_sensitivity();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    return 0;
}
