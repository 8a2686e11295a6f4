// chx_tunes_dev.h — the index and termination logic of chx_tunes.hip (TurnByTurn.tunes), host-callable: the coarse transform's
// butterfly items and output positions, the spectrum of the real signal from the packed complex transform, the choice of the
// peak and its bracket, and the safeguarded Newton step. tests/host/tunes_check.hip runs all of it against long-double
// evaluations without a GPU; the kernel runs the same functions, one item per lane.
//
// The coarse grid nu_k = k / (2 P), k = 0 .. P, of a real signal x_0 .. x_{T-1} zero-padded to 2 P samples is the first half of
// its 2 P-point transform. Packed as z_m = x_{2m} + i x_{2m+1} that is ONE complex transform of P points, Z, and
//   X_k = E_k + exp(-2 pi i k / (2 P)) O_k,  E_k = (Z_k + conj Z_{P-k}) / 2,  O_k = (Z_k - conj Z_{P-k}) / (2 i)   (indices mod P).
// The transform runs in place, decimation in frequency: one radix-2 stage first when log2 P is odd, then radix-4 stages (the
// butterflies of chx_fft_reg.h) on blocks of L = 4^m, ..., 16, 4 points. Output k lands at fft_pos(k): the halves of the radix-2
// stage hold the even and the odd k, inside them the base-4 digits of k are reversed.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "chx_fft_reg.h"

namespace chx_tune {

constexpr double kStop = 0x1p-48;   // the root search ends when its bracket or its step is this small
constexpr int kMaxIter = 96;        // ... or after this many steps: every step halves the bracket or the step (root_step)

// log2 P of the coarse transform, P = 2 * 2^ceil(log2 T)
__host__ __device__ inline int coarse_log2(int T) {
    int p = 0;
    while ((1 << p) < T) ++p;
    return p + 1;
}

// exp(-2 pi i num / 2^den_log2) = c + i s, 0 <= num < 2^13 (the fraction is exact in float32)
__host__ __device__ inline void twiddle(int num, int den_log2, float& c, float& s) {
    const float x = (float)num / (float)(1 << den_log2);
#ifdef __HIP_DEVICE_COMPILE__
    float sn;
    sincospif(2.0f * x, &sn, &c);
    s = -sn;
#else
    c = (float)cos(6.283185307179586 * (double)x);
    s = (float)-sin(6.283185307179586 * (double)x);
#endif
}

// item j < P / 2 of the radix-2 stage over all P = 2^p points
__host__ __device__ inline void fft_r2_item(vec2<float>* z, int p, int j) {
    const int half = 1 << (p - 1);
    const vec2<float> a = z[j], b = z[j + half];
    float c, s;
    twiddle(j, p, c, s);
    z[j] = a + b;
    z[j + half] = chx_fft::cmul(a - b, c, s);
}

// item i < P / 4 of the radix-4 stage on blocks of L = 2^l points (l even, >= 2)
__host__ __device__ inline void fft_r4_item(vec2<float>* z, int l, int i) {
    const int q = 1 << (l - 2);
    const int j = i & (q - 1);
    const int base = ((i >> (l - 2)) << l) + j;
    vec2<float> a0 = z[base], a1 = z[base + q], a2 = z[base + 2 * q], a3 = z[base + 3 * q];
    chx_fft::dft4<false>(a0, a1, a2, a3);
    if (j) {
        float c, s;
        twiddle(j, l, c, s);
        a1 = chx_fft::cmul(a1, c, s);
        twiddle(2 * j, l, c, s);
        a2 = chx_fft::cmul(a2, c, s);
        twiddle(3 * j, l, c, s);
        a3 = chx_fft::cmul(a3, c, s);
    }
    z[base] = a0;
    z[base + q] = a1;
    z[base + 2 * q] = a2;
    z[base + 3 * q] = a3;
}

// where output k < P of the in-place transform of P = 2^p points stands
__host__ __device__ inline int fft_pos(int k, int p) {
    int off = 0, bits = p;
    if (p & 1) {
        off = (k & 1) << (p - 1);
        k >>= 1;
        bits = p - 1;
    }
    int r = 0;
    for (int b = 0; b < bits; b += 2) {
        r = (r << 2) | (k & 3);
        k >>= 2;
    }
    return off + r;
}

// |X_k|^2, k = 0 .. P, of the real signal behind the packed transform z (as the stages left it)
__host__ __device__ inline float coarse_power(const vec2<float>* z, int p, int k) {
    const int P = 1 << p;
    const vec2<float> a = z[fft_pos(k & (P - 1), p)], b = z[fft_pos((P - k) & (P - 1), p)];
    const vec2<float> e = {0.5f * (a.x + b.x), 0.5f * (a.y - b.y)};
    const vec2<float> o = {0.5f * (a.y + b.y), -0.5f * (a.x - b.x)};
    float c, s;
    twiddle(k, p + 1, c, s);
    const vec2<float> x = e + chx_fft::cmul(o, c, s);
    return x.x * x.x + x.y * x.y;
}

// g = F_r G_i - F_i G_r (dA / dnu = 4 pi g) and g' = 2 pi (|G|^2 - F_r H_r - F_i H_i), from F = sum v e, G = sum n v e,
// H = sum n^2 v e with e = exp(-2 pi i nu n): F' = -2 pi i G, G' = -2 pi i H
__host__ __device__ inline double slope(double fr, double fi, double gr, double gi) { return fr * gi - fi * gr; }
__host__ __device__ inline double curvature(double fr, double fi, double gr, double gi, double hr, double hi) {
    return 6.283185307179586 * ((gr * gr + gi * gi) - fr * hr - fi * hi);
}

// The peak among the float64 values A[0..4] at k0 - 2 .. k0 + 2, k0 the argmax of the float32 coarse stage: the lowest k of k0 - 1,
// k0, k0 + 1 inside 0 .. P with the largest A (the float32 stage decides between distant k, float64 between neighbours, which
// is where two values can lie within float32's error of each other). Returns its index 1 .. 3 into A.
__host__ __device__ inline int pick_peak(const double (&A)[5], int k0, int P) {
    int best = 2;
    double bestA = -1.0;
    for (int d = 1; d <= 3; ++d) {
        const int k = k0 - 2 + d;
        if (k < 0 || k > P) continue;
        if (A[d] > bestA) {
            bestA = A[d];
            best = d;
        }
    }
    return best;
}

// refine only an interior peak whose neighbours' slopes point at it
__host__ __device__ inline bool has_bracket(int k, int P, double g_below, double g_above) {
    return k > 0 && k < P && g_below > 0.0 && g_above < 0.0;
}

// Root of g in a bracket with g(lo) > 0 > g(hi). x is the iterate to evaluate next, dx the size of the last step.
struct Root {
    double lo, hi, x, dx;
};
__host__ __device__ inline Root root_begin(double lo, double hi, double x) { return Root{lo, hi, x, hi - lo}; }
// One step from g(x) and dg = g'(x): the bracket takes x, the Newton point is the next iterate when
// g falls there, the point lies in the bracket (a Newton step below the spacing of doubles leaves x where it is, at the bracket's
// end: that is convergence) and the step is at most half the last one; otherwise the bracket's middle. Every iterate stays inside the bracket, and every step halves the bracket or the step. Returns true when r.x is the
// answer: g(x) == 0, or the bracket or the step to the new r.x is <= kStop.
__host__ __device__ inline bool root_step(Root& r, double g, double dg) {
    if (g == 0.0) return true;
    if (g > 0.0) r.lo = r.x;
    else r.hi = r.x;
    const double width = r.hi - r.lo;
    double xn = r.x - g / dg;
    const bool newton = dg < 0.0 && xn >= r.lo && xn <= r.hi && fabs(xn - r.x) <= 0.5 * r.dx;
    if (!newton) xn = r.lo + 0.5 * width;
    const double step = fabs(xn - r.x);
    r.dx = step;
    r.x = xn;
    return width <= kStop || step <= kStop;
}

// the row's loss rule: lost on a turn up to the window's last record
__host__ __device__ inline bool lost_in_window(int32_t lost_turn, int64_t last_turn) {
    return lost_turn > 0 && (int64_t)lost_turn <= last_turn;
}

}  // namespace chx_tune
