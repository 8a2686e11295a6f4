// tunes_check.hip — the host-callable logic of csrc/chx_tunes_dev.h against long-double evaluations, without a GPU:
//   hipcc --cuda-host-only -O2 -std=c++17 -ffp-contract=off -I cheetah_amd/csrc -o tunes_check tests/host/tunes_check.hip
// Prints one "<part>: ok" line per part and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chx_tunes_dev.h"

using namespace chx_tune;
typedef long double ld;

static const ld kPiL = 3.14159265358979323846264338327950288L;
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

static double uniform(unsigned long long& state) {   // a fixed linear congruential sequence in [0, 1)
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(state >> 11) * 0x1p-53;
}

// v_n of the definition for a two-line signal with an offset, in long double rounded to double
static std::vector<double> signal(int T, double nu1, double nu2, double a2, double offset) {
    std::vector<ld> u(T), w(T);
    ld sw = 0, swu = 0;
    for (int n = 0; n < T; ++n) {
        u[n] = (ld)(double)(1e-3L * cosl(2 * kPiL * nu1 * n + 0.3L) + a2 * cosl(2 * kPiL * nu2 * n + 1.1L) + offset);
        const ld s = sinl(kPiL * (n + 0.5L) / T);
        w[n] = s * s;
        sw += w[n];
        swu += w[n] * u[n];
    }
    std::vector<double> v(T);
    for (int n = 0; n < T; ++n) v[n] = (double)(w[n] * (u[n] - swu / sw));
    return v;
}

struct Sums {
    ld fr, fi, gr, gi, hr, hi;
};
static Sums sums(const std::vector<double>& v, ld nu) {
    Sums s = {0, 0, 0, 0, 0, 0};
    for (size_t n = 0; n < v.size(); ++n) {
        ld t = nu * (ld)n;
        t -= floorl(t);
        const ld c = cosl(2 * kPiL * t), sn = sinl(2 * kPiL * t), a = v[n], dn = (ld)n;
        s.fr += a * c;
        s.fi -= a * sn;
        s.gr += dn * a * c;
        s.gi -= dn * a * sn;
        s.hr += dn * dn * a * c;
        s.hi -= dn * dn * a * sn;
    }
    return s;
}
static ld slope_l(const Sums& s) { return s.fr * s.gi - s.fi * s.gr; }
static ld power_l(const Sums& s) { return s.fr * s.fr + s.fi * s.fi; }

static void check_grid() {
    for (int T = 8; T <= 4096; ++T) {
        const int p = coarse_log2(T), P = 1 << p;
        int c = 1;
        while (c < T) c *= 2;
        EXPECT(P == 2 * c, "coarse_log2(%d) = %d", T, p);
        EXPECT(4 * T <= 2 * P && P <= 8192 && p >= 4, "grid of T = %d: P = %d", T, P);
    }
    for (int p = 4; p <= 13; ++p) {
        std::vector<char> seen(1 << p, 0);
        for (int k = 0; k < (1 << p); ++k) {
            const int q = fft_pos(k, p);
            EXPECT(q >= 0 && q < (1 << p) && !seen[q], "fft_pos(%d, %d) = %d", k, p, q);
            if (q >= 0 && q < (1 << p)) seen[q] = 1;
        }
    }
    if (!failures) std::printf("grid: ok\n");
}

// the coarse stage as the kernel runs it (every item of a stage, then the next stage) against the real signal's spectrum
static void coarse_stage(const std::vector<double>& v, int p, std::vector<vec2<float>>& z) {
    const int P = 1 << p;
    double sa = 0;
    for (double x : v) sa += std::fabs(x);
    z.assign(P, vec2<float>{0.0f, 0.0f});
    float* zf = reinterpret_cast<float*>(z.data());
    for (size_t n = 0; n < v.size(); ++n) zf[n] = (float)(v[n] / sa);
    if (p & 1)
        for (int j = 0; j < P / 2; ++j) fft_r2_item(z.data(), p, j);
    for (int l = p & ~1; l >= 2; l -= 2)
        for (int i = 0; i < P / 4; ++i) fft_r4_item(z.data(), l, i);
}

static void check_transform() {
    const int before = failures;
    unsigned long long seed = 12345;
    for (int p = 4; p <= 13; ++p) {
        const int P = 1 << p;
        for (int T : {P / 2, P / 4 + 1, (3 * P) / 8 + 1}) {
            if (T < 8) continue;
            EXPECT(coarse_log2(T) == p, "T = %d does not have p = %d", T, p);
            std::vector<double> v(T);
            double sa = 0;
            for (int n = 0; n < T; ++n) {
                v[n] = uniform(seed) - 0.5 + 0.7 * std::cos(2 * M_PI * 0.2137 * n);
                sa += std::fabs(v[n]);
            }
            std::vector<vec2<float>> z;
            coarse_stage(v, p, z);
            std::vector<ld> ct(2 * P), st(2 * P);
            for (int m = 0; m < 2 * P; ++m) {
                ct[m] = cosl(2 * kPiL * m / (2 * P));
                st[m] = sinl(2 * kPiL * m / (2 * P));
            }
            std::vector<ld> A(P + 1);
            ld amax = 0;
            for (int k = 0; k <= P; ++k) {
                ld re = 0, im = 0;
                for (int n = 0; n < T; ++n) {
                    const int m = (int)(((long long)k * n) & (2 * P - 1));
                    re += v[n] / sa * ct[m];
                    im -= v[n] / sa * st[m];
                }
                A[k] = re * re + im * im;
                if (A[k] > amax) amax = A[k];
            }
            ld worst = 0;
            for (int k = 0; k <= P; ++k) {
                const ld e = fabsl((ld)coarse_power(z.data(), p, k) - A[k]);
                if (e > worst) worst = e;
            }
            // float32 butterflies: a few 2^-24 of the largest value per stage, 7 stages at most
            EXPECT(worst <= 2e-5L * amax, "transform p = %d, T = %d: |A - A_ref| = %Lg of max %Lg", p, T, worst, amax);
        }
    }
    if (failures == before) std::printf("transform: ok\n");
}

// the whole path on the host (float32 coarse argmax, float64 choice among its neighbours, bracket, Newton steps) against the
// definition in long double (argmax over the whole grid, bisection)
static void check_path() {
    const int before = failures;
    unsigned long long seed = 777;
    int most_steps = 0;
    for (int T : {8, 9, 16, 64, 100, 257, 1024, 4096}) {
        const int p = coarse_log2(T), P = 1 << p;
        for (int rep = 0; rep < (T > 1000 ? 2 : 6); ++rep) {
            const double nu1 = 0.05 + 0.4 * uniform(seed), nu2 = 0.05 + 0.4 * uniform(seed);
            const std::vector<double> v = signal(T, nu1, nu2, 2e-4 * uniform(seed), 0.01 * (uniform(seed) - 0.5));
            // the definition
            int kref = 0;
            ld aref = -1;
            std::vector<ld> ct(2 * P), st(2 * P);                  // the grid's phases k n / (2 P) are exact: a table
            for (int m = 0; m < 2 * P; ++m) {
                ct[m] = cosl(2 * kPiL * m / (2 * P));
                st[m] = sinl(2 * kPiL * m / (2 * P));
            }
            for (int k = 0; k <= P; ++k) {
                ld re = 0, im = 0;
                for (int n = 0; n < T; ++n) {
                    const int m = (int)(((long long)k * n) & (2 * P - 1));
                    re += v[n] * ct[m];
                    im -= v[n] * st[m];
                }
                const ld a = re * re + im * im;
                if (a > aref) {
                    aref = a;
                    kref = k;
                }
            }
            // the kernel's path
            std::vector<vec2<float>> z;
            coarse_stage(v, p, z);
            int k0 = 0;
            float a0 = -1.0f;
            for (int k = 0; k <= P; ++k) {
                const float a = coarse_power(z.data(), p, k);
                if (a > a0) {
                    a0 = a;
                    k0 = k;
                }
            }
            double A[5], g[5];
            for (int d = 0; d < 5; ++d) {
                int k = k0 - 2 + d;
                k = k < 0 ? 0 : (k > P ? P : k);
                const Sums s = sums(v, (ld)k / (2 * P));
                A[d] = (double)power_l(s);
                g[d] = slope((double)s.fr, (double)s.fi, (double)s.gr, (double)s.gi);
            }
            const int dp = pick_peak(A, k0, P), ks = k0 - 2 + dp;
            EXPECT(ks == kref, "T = %d nu = %.6f: peak %d (coarse %d), definition %d", T, nu1, ks, k0, kref);
            if (ks != kref) continue;
            const bool refine = has_bracket(ks, P, g[dp - 1], g[dp + 1]);
            EXPECT(refine, "T = %d nu = %.6f: no bracket around an interior peak", T, nu1);
            if (!refine) continue;
            ld lo = (ld)(ks - 1) / (2 * P), hi = (ld)(ks + 1) / (2 * P);
            Root r = root_begin((double)lo, (double)hi, (double)ks / (2 * P));
            int steps = 0;
            for (; steps < kMaxIter; ++steps) {
                const Sums s = sums(v, r.x);
                const double gx = (double)slope_l(s);
                const double dg = curvature((double)s.fr, (double)s.fi, (double)s.gr, (double)s.gi, (double)s.hr, (double)s.hi);
                const bool done = root_step(r, gx, dg);
                EXPECT(r.x >= r.lo && r.x <= r.hi && r.lo >= (double)lo && r.hi <= (double)hi, "T = %d: iterate %.17g outside [%.17g, %.17g]",
                       T, r.x, r.lo, r.hi);
                if (done) break;
            }
            for (int i = 0; i < 100; ++i) {
                const ld mid = 0.5L * (lo + hi);
                if (slope_l(sums(v, mid)) > 0) lo = mid;
                else hi = mid;
            }
            const ld root = 0.5L * (lo + hi);
            EXPECT(steps < 12, "T = %d nu = %.6f: %d Newton steps", T, nu1, steps + 1);
            EXPECT(fabsl((ld)r.x - root) <= 0x1p-47L, "T = %d nu = %.6f: root %.17g, bisection %.17Lg", T, nu1, r.x, root);
            if (steps + 1 > most_steps) most_steps = steps + 1;
        }
    }
    if (failures == before) std::printf("path: ok (at most %d Newton steps)\n", most_steps);
}

// root_step with derivatives that are useless: it must fall back to bisection and end within the cap; a derivative that is too
// large makes Newton steps that are too short, and ending on such a step is as exact as the derivative is
static void check_root_fallback() {
    const int before = failures;
    const double root = 0.3 + 1.0 / 3000.0;
    auto g = [&](double x) { return -(x - root) * (1.0 + 50.0 * (x - root) * (x - root)); };
    const double dgs[] = {1.0, 0.0, -1e-30, -1e3, -30.0, NAN, -1.0};
    for (double dg : dgs) {
        Root r = root_begin(0.25, 0.3125, 0.28125);
        int steps = 0;
        bool done = false;
        for (; steps < kMaxIter && !done; ++steps) {
            done = root_step(r, g(r.x), dg);
            EXPECT(r.x >= r.lo && r.x <= r.hi && r.lo >= 0.25 && r.hi <= 0.3125, "dg = %g: iterate %.17g outside the bracket", dg, r.x);
        }
        EXPECT(done, "dg = %g: not done after %d steps", dg, steps);
        // g' = -1 at the root. A search that ends on its bracket is within 2^-48; one that ends on a Newton step |g / dg| <= 2^-48
        // has |g| <= |dg| 2^-48 and stands |g / g'| from the root: with the true derivative that is the same bound (twice, for slack)
        const double bound = dg < -1.0 ? -dg * 0x1p-47 : 0x1p-47;
        EXPECT(std::fabs(r.x - root) <= bound, "dg = %g: %.17g instead of %.17g", dg, r.x, root);
    }
    {   // an exact zero ends the search where it is
        Root r = root_begin(0.0, 1.0, 0.5);
        EXPECT(root_step(r, 0.0, -1.0) && r.x == 0.5, "g == 0 does not end the search");
    }
    if (failures == before) std::printf("root: ok\n");
}

static void check_edges() {
    const int before = failures;
    {
        const double A[5] = {9.0, 1.0, 2.0, 2.0, 9.0};       // ties go to the lowest k; k0 +- 2 are never chosen
        EXPECT(pick_peak(A, 10, 64) == 2, "tie between k0 and k0 + 1");
        const double B[5] = {0.0, 3.0, 3.0, 1.0, 0.0};
        EXPECT(pick_peak(B, 10, 64) == 1, "tie between k0 - 1 and k0");
        EXPECT(pick_peak(B, 0, 64) == 2, "k0 = 0: k = -1 is outside the grid");
        const double C[5] = {0.0, 1.0, 2.0, 5.0, 0.0};
        EXPECT(pick_peak(C, 64, 64) == 2, "k0 = P: k = P + 1 is outside the grid");
        const double Z[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        EXPECT(pick_peak(Z, 5, 64) == 1, "all zero: the lowest k");
    }
    EXPECT(has_bracket(5, 64, 1.0, -1.0), "an interior peak with slopes towards it");
    EXPECT(!has_bracket(0, 64, 1.0, -1.0) && !has_bracket(64, 64, 1.0, -1.0), "the ends of the grid are not refined");
    EXPECT(!has_bracket(5, 64, 0.0, -1.0) && !has_bracket(5, 64, 1.0, 0.0) && !has_bracket(5, 64, -1.0, 1.0) &&
               !has_bracket(5, 64, NAN, -1.0),
           "a bracket needs g > 0 below and g < 0 above");
    EXPECT(!lost_in_window(0, 100) && lost_in_window(1, 100) && lost_in_window(100, 100) && !lost_in_window(101, 100) &&
               !lost_in_window(-1, 100),
           "the loss rule");
    {   // the alternating signal: the peak is the last grid point, exactly 1/2
        const int T = 64, p = coarse_log2(T), P = 1 << p;
        std::vector<double> v(T);
        ld sw = 0, swu = 0;
        for (int n = 0; n < T; ++n) {
            const ld s = sinl(kPiL * (n + 0.5L) / T);
            sw += s * s;
            swu += s * s * ((n & 1) ? -1 : 1);
        }
        for (int n = 0; n < T; ++n) {
            const ld s = sinl(kPiL * (n + 0.5L) / T);
            v[n] = (double)(s * s * (((n & 1) ? -1 : 1) - swu / sw));
        }
        std::vector<vec2<float>> z;
        coarse_stage(v, p, z);
        int k0 = 0;
        float a0 = -1.0f;
        for (int k = 0; k <= P; ++k) {
            const float a = coarse_power(z.data(), p, k);
            if (a > a0) {
                a0 = a;
                k0 = k;
            }
        }
        EXPECT(k0 == P, "alternating signal: coarse peak %d of %d", k0, P);
    }
    if (failures == before) std::printf("edges: ok\n");
}

int main() {
    check_grid();
    check_transform();
    check_path();
    check_root_fallback();
    check_edges();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("all: ok\n");
    return 0;
}
