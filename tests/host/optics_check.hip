// optics_check.hip — the host-callable parts of csrc/chx_optics_dev.h against long-double eliminations, without a GPU, under the
// address and undefined-behaviour sanitizers:
//   hipcc --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all
//         -I cheetah_amd/csrc -o optics_check tests/host/optics_check.hip
// Prints one "<part>: ok" line per part and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

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

static double uniform(unsigned long long& state) {   // a fixed linear congruential sequence in [0, 1)
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(state >> 11) * 0x1p-53;
}

// the reference: Gaussian elimination with COMPLETE pivoting in long double (another order of operations, 11 more bits)
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

// the growth the bound allows: n 2^-52 times the row-sum norm of a times that of its inverse times 64 — the error of partial
// pivoting is n eps cond times a growth factor that is of order one on drawn matrices; the inverse from the reference
static ld condition(int n, const std::vector<ld>& a) {
    ld na = 0, ni = 0;
    for (int r = 0; r < n; ++r) {
        ld s = 0;
        for (int c = 0; c < n; ++c) s += fabsl(a[r * n + c]);
        na = fmaxl(na, s);
    }
    std::vector<std::vector<ld>> inv(n);
    for (int c = 0; c < n; ++c) {
        std::vector<ld> e(n, 0);
        e[c] = 1;
        reference_solve(n, a, e, inv[c]);
    }
    for (int r = 0; r < n; ++r) {
        ld s = 0;
        for (int c = 0; c < n; ++c) s += fabsl(inv[c][r]);
        ni = fmaxl(ni, s);
    }
    return na * ni;
}

static void check_layout() {
    const int before = failures;
    EXPECT(kLanes == 64 && kGroup * kSeeds == kLanes, "a workgroup is one wave");
    std::vector<int> seen(kSeeds * 6, 0);
    for (int lane = 0; lane < kLanes; ++lane) {
        const int g = group_of_lane(lane), m = tangent_of_lane(lane);
        EXPECT(g >= 0 && g < kSeeds && m >= 0 && m < kGroup, "lane %d -> group %d tangent %d", lane, g, m);
        EXPECT(g == group_of_lane(lane - m), "the lanes of a group are consecutive");
        if (m < 6) ++seen[g * 6 + m];
    }
    for (int i = 0; i < kSeeds * 6; ++i) EXPECT(seen[i] == 1, "every (seed, tangent) has one lane");
    for (int64_t B : {1LL, 7LL, 8LL, 9LL, 65LL, 257LL, 4096LL, (1LL << 33) + 3}) {
        const int64_t wg = workgroups(B);
        EXPECT(wg * kSeeds >= B && (wg - 1) * kSeeds < B, "workgroups(%lld) = %lld", (long long)B, (long long)wg);
        int64_t live_count = 0;
        for (int pick = 0; pick < 2; ++pick) {
            const int64_t w = pick == 0 ? 0 : wg - 1;
            for (int g = 0; g < kSeeds; ++g) {
                bool live;
                const int64_t seed = seed_of_group(w, g, B, live);
                EXPECT(seed >= 0 && seed < B, "B %lld: group %d of workgroup %lld reads seed %lld", (long long)B, g, (long long)w, (long long)seed);
                EXPECT(live == (w * kSeeds + g < B), "B %lld: live", (long long)B);
                EXPECT(!live || seed == w * kSeeds + g, "B %lld: a live group has its own seed", (long long)B);
                if (pick == 1 && live) ++live_count;
            }
        }
        EXPECT(live_count == B - (wg - 1) * kSeeds, "B %lld: %lld live groups in the last workgroup", (long long)B, (long long)live_count);
    }
    if (failures == before) std::printf("layout: ok\n");
}

static void check_solver() {
    const int before = failures;
    unsigned long long st = 12345;
    double worst = 0;
    for (int n : {1, 4, 6}) {
        for (int draw = 0; draw < 200; ++draw) {
            std::vector<double> a(36, 7.0), b(6, 7.0);           // (rows 6 apart, as the kernel holds them)
            std::vector<ld> al(n * n), bl(n), xl;
            for (int r = 0; r < n; ++r) {
                for (int c = 0; c < n; ++c) al[r * n + c] = a[r * 6 + c] = 2.0 * uniform(st) - 1.0;
                bl[r] = b[r] = 2.0 * uniform(st) - 1.0;
            }
            if (draw % 3 == 0)                                   // a small leading entry: the pivot must come from below
                al[0] = a[0] = 1e-300 * (uniform(st) - 0.5);
            const std::vector<double> a0 = a;
            EXPECT(reference_solve(n, al, bl, xl), "the reference solves draw %d", draw);
            const bool ok = solve(n, a.data(), 6, b.data());
            EXPECT(ok, "n %d draw %d is regular", n, draw);
            const ld bound = 64 * n * 0x1p-52L * condition(n, al);
            ld scale = 0;
            for (int k = 0; k < n; ++k) scale = fmaxl(scale, fabsl(xl[k]));
            for (int k = 0; k < n; ++k) {
                const ld err = fabsl((ld)b[k] - xl[k]) / scale;
                worst = fmax(worst, (double)(err / bound));
                EXPECT(err <= bound, "n %d draw %d: x[%d] = %.17g, reference %.17Lg, error %.3Lg of the bound", n, draw, k, b[k], xl[k], err / bound);
            }
            for (int r = n; r < 6; ++r) EXPECT(b[r] == 7.0, "n %d: b[%d] is not touched", n, r);
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c)
                    if (r >= n || c >= n) EXPECT(a[r * 6 + c] == 7.0, "n %d: a[%d][%d] is not touched", n, r, c);
        }
    }
    std::printf("solver: largest error / bound %.3g\n", worst);
    if (failures == before) std::printf("solver: ok\n");
}

static void check_singular() {
    const int before = failures;
    for (int n : {4, 6}) {
        // two equal rows; a zero matrix; a NaN entry; an infinite entry: no solution, every x NaN, nothing else touched
        for (int what = 0; what < 4; ++what) {
            std::vector<double> a(36, 0.0), b(6, 3.0);
            unsigned long long st = 99 + what;
            for (int r = 0; r < n; ++r)
                for (int c = 0; c < n; ++c) a[r * 6 + c] = what == 1 ? 0.0 : 2.0 * uniform(st) - 1.0;
            if (what == 0)
                for (int c = 0; c < n; ++c) a[(n - 1) * 6 + c] = a[1 * 6 + c];
            if (what == 2) a[2 * 6 + 1] = NAN;
            if (what == 3) a[1 * 6 + 0] = INFINITY;
            const bool ok = solve(n, a.data(), 6, b.data());
            // (two equal rows see the same operations until one of them is the pivot row; the other is then a - 1 * a = 0 exactly
            // and stays 0: the zero pivot is met in floating point too)
            EXPECT(!ok, "n %d case %d has no solution", n, what);
            for (int k = 0; k < n; ++k) EXPECT(std::isnan(b[k]), "n %d case %d: x[%d] is NaN", n, what, k);
            for (int k = n; k < 6; ++k) EXPECT(b[k] == 3.0, "n %d case %d: b[%d] is not touched", n, what, k);
        }
    }
    if (failures == before) std::printf("singular: ok\n");
}

static void check_systems() {
    const int before = failures;
    unsigned long long st = 777;
    for (int draw = 0; draw < 50; ++draw) {
        double M[36], f[6], x[6], a[36], step[6], eta[6] = {5, 5, 5, 5, 5, 5};
        for (int i = 0; i < 36; ++i) M[i] = 2.0 * uniform(st) - 1.0;
        for (int i = 0; i < 6; ++i) f[i] = 1e-3 * (uniform(st) - 0.5), x[i] = 1e-3 * (uniform(st) - 0.5), step[i] = 5;
        for (int mode : {1, 2}) {
            const int n = closed_count(mode);
            EXPECT(n == (mode == 2 ? 6 : 4), "closed_count");
            EXPECT(newton_step(n, M, f, x, a, step), "the Newton system of draw %d is regular", draw);
            // (M_c - I) step + (f - x)_c = 0 in long double, to n eps cond relative to |f - x|
            std::vector<ld> al(n * n), bl(n), xl;
            for (int i = 0; i < n; ++i) {
                for (int m = 0; m < n; ++m) al[i * n + m] = (ld)M[i * 6 + m] - (i == m ? 1 : 0);
                bl[i] = -((ld)f[i] - (ld)x[i]);
            }
            reference_solve(n, al, bl, xl);
            const ld bound = 64 * n * 0x1p-52L * condition(n, al);
            ld scale = 0;
            for (int k = 0; k < n; ++k) scale = fmaxl(scale, fabsl(xl[k]));
            for (int k = 0; k < n; ++k) EXPECT(fabsl((ld)step[k] - xl[k]) <= bound * scale, "mode %d draw %d: step[%d]", mode, draw, k);
            if (mode == 1) EXPECT(step[4] == 5 && step[5] == 5, "the held coordinates have no step");
        }
        EXPECT(dispersion(M, a, eta), "the dispersion system of draw %d is regular", draw);
        std::vector<ld> al(16), bl(4), xl;
        for (int i = 0; i < 4; ++i) {
            for (int m = 0; m < 4; ++m) al[i * 4 + m] = (i == m ? 1 : 0) - (ld)M[i * 6 + m];
            bl[i] = M[i * 6 + 5];
        }
        reference_solve(4, al, bl, xl);
        const ld bound = 64 * 4 * 0x1p-52L * condition(4, al);
        ld scale = 0;
        for (int k = 0; k < 4; ++k) scale = fmaxl(scale, fabsl(xl[k]));
        for (int k = 0; k < 4; ++k) EXPECT(fabsl((ld)eta[k] - xl[k]) <= bound * scale, "draw %d: eta[%d]", draw, k);
        EXPECT(eta[4] == 5 && eta[5] == 5, "eta has four entries");
    }
    // the identity has no closed orbit of its own and no dispersion: NaN, nothing raised
    double I6[36] = {0}, f[6] = {1, 2, 3, 4, 5, 6}, x[6] = {0}, a[36], step[6], eta[4];
    for (int i = 0; i < 6; ++i) I6[i * 6 + i] = 1.0;
    EXPECT(!newton_step(4, I6, f, x, a, step) && std::isnan(step[0]) && std::isnan(step[3]), "M = I: no step");
    EXPECT(!dispersion(I6, a, eta) && std::isnan(eta[0]) && std::isnan(eta[3]), "M = I: no dispersion");
    // the closing error: the largest of the first n, NaN from any of them
    const double g[6] = {1.0, 2.5, -4.0, 0.5, 100.0, NAN}, z[6] = {0, 0, 0, 0, 0, 0};
    EXPECT(closing_error(4, g, z) == 4.0, "closing_error over four");
    EXPECT(closing_error(5, g, z) == 100.0, "closing_error over five");
    EXPECT(std::isnan(closing_error(6, g, z)), "closing_error with a NaN at the end");
    const double h[6] = {1.0, NAN, 3.0, 0.5, 0, 0};
    EXPECT(std::isnan(closing_error(4, h, z)), "closing_error with a NaN in the middle");
    if (failures == before) std::printf("systems: ok\n");
}

int main() {
    check_layout();
    check_solver();
    check_singular();
    check_systems();
    if (failures == 0) std::printf("all: ok\n");
    return failures == 0 ? 0 : 1;
}
