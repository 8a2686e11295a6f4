// chx_tunes.hip — per-particle tunes from turn-by-turn records (TurnByTurn.tunes): for every recorded row and every requested
// plane the interpolated peak of the Hann-windowed spectrum of T consecutive records (NAFF's first line) and its amplitude.
// The definition is in include/chx.h and DESIGN.md; the index and termination logic in chx_tunes_dev.h (host-checked).
//
// One workgroup of 256 lanes per row. Lane t owns the samples n = t + 256 j, j < 16, of every requested plane in registers:
// the row's record (7 contiguous values) is read once for all planes. Per plane:
//   1. windowed mean and v_n = w_n (u_n - mean) in float64; sum |v_n| scales the coarse stage into float32's range;
//   2. the coarse stage: v packed as P complex float32 values in LDS (64 KB at T = 4096), transformed in place, |X_k|^2 from
//      pairs of outputs, argmax with the lowest k on ties -> k0;
//   3. float64 direct sums F, G at k0 - 2 .. k0 + 2 in one pass over the lane's samples: the peak k* among k0 - 1 .. k0 + 1 (float32
//      decides between distant k, float64 between neighbours) and the slopes at its two neighbours;
//   4. the root of the slope by safeguarded Newton steps (F, G, H at one frequency per step), and F at the root for the amplitude.
// Every sum: the lane's samples in order, chx_wave_sum, the four waves in order — the same bits in every call. The reduction
// scratch lies on the first bytes of the transform's buffer; barriers separate the two uses. No workspace, no host
// synchronisation. -ffp-contract=off: every fma is written out.
#include "chx_common.h"
#include "chx_tunes_dev.h"

namespace {

using namespace chx_tune;

constexpr int kJ = CHX_TUNES_T_MAX / CHX_BLOCK;   // samples per lane
constexpr int kPMax = 2 * CHX_TUNES_T_MAX;        // complex points of the largest coarse transform
static_assert(kJ * CHX_BLOCK == CHX_TUNES_T_MAX && (CHX_TUNES_T_MAX & (CHX_TUNES_T_MAX - 1)) == 0, "whole samples per lane");
static_assert(kPMax * sizeof(vec2<float>) <= 65536, "the coarse transform fits the static LDS limit");
static_assert(CHX_TUNES_T_MIN >= 8, "P >= 16: every transform has a radix-4 stage");

// sums of K doubles per lane over the workgroup, delivered to EVERY lane (the control flow that follows is uniform)
template <int K>
__device__ __forceinline__ void block_sum_all(double (&v)[K], double* red /* [4 K] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = chx_wave_sum(v[k]);
    __syncthreads();                              // whoever read the scratch (or the transform under it) is done
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
}

// F (ORDER 0), F and G (1) or F, G and H (2) at NF frequencies: out[f] = (F_r, F_i, G_r, G_i, H_r, H_i)
template <int NF, int ORDER>
__device__ __forceinline__ void spectral_sums(const double (&v)[kJ], int Tn, const double (&nus)[NF],
                                              double (&out)[NF * 2 * (ORDER + 1)], double* red) {
    constexpr int W = 2 * (ORDER + 1);
#pragma unroll
    for (int i = 0; i < NF * W; ++i) out[i] = 0.0;
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
        const int n = (int)threadIdx.x + j * CHX_BLOCK;
        if (n < Tn) {
            const double dn = (double)n;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const double t = nus[f] * dn;
                const double fr = t - __builtin_rint(t);          // the phase in turns, reduced exactly
                double s, c;
                sincospi(2.0 * fr, &s, &c);
                double a = v[j];
                out[f * W] = __builtin_fma(a, c, out[f * W]);
                out[f * W + 1] = __builtin_fma(-a, s, out[f * W + 1]);
                if constexpr (ORDER >= 1) {
                    a *= dn;
                    out[f * W + 2] = __builtin_fma(a, c, out[f * W + 2]);
                    out[f * W + 3] = __builtin_fma(-a, s, out[f * W + 3]);
                }
                if constexpr (ORDER >= 2) {
                    a *= dn;
                    out[f * W + 4] = __builtin_fma(a, c, out[f * W + 4]);
                    out[f * W + 5] = __builtin_fma(-a, s, out[f * W + 5]);
                }
            }
        }
    }
    block_sum_all<NF * W>(out, red);
}

template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void tunes_kernel(const T* __restrict__ probe, const int32_t* __restrict__ lost, int64_t S,
                                                         int64_t r0, int Tn, int64_t last_turn, int columns,
                                                         double* __restrict__ nu_out, double* __restrict__ amp_out) {
    __shared__ vec2<float> zbuf[kPMax];
    double* red = reinterpret_cast<double*>(zbuf);
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const int C = __builtin_popcount(columns);
    const double nan = __builtin_nan("");
    double* nu_row = nu_out + row * C;
    double* amp_row = amp_out + row * C;

    if (lost && lost_in_window(lost[row], last_turn)) {       // (uniform)
        if (tid < C) {
            nu_row[tid] = nan;
            amp_row[tid] = nan;
        }
        return;
    }

    // the samples of all requested planes and the window, n = tid + 256 j
    T u[3][kJ];
    double w[kJ];
    double sw[1] = {0.0};
#pragma unroll
    for (int j = 0; j < kJ; ++j) {
        const int n = tid + j * CHX_BLOCK;
        w[j] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c][j] = (T)0;
        if (n < Tn) {
            const T* __restrict__ rec = probe + ((r0 + n) * S + row) * 7;
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (columns >> c & 1) u[c][j] = rec[2 * c];
            const double sn = sinpi(((double)n + 0.5) / (double)Tn);
            w[j] = sn * sn;
            sw[0] += w[j];
        }
    }
    block_sum_all<1>(sw, red);

    const int p = coarse_log2(Tn), P = 1 << p;
    int ci = 0;
    for (int c = 0; c < 3; ++c) {
        if (!(columns >> c & 1)) continue;
        const int slot = ci++;

        double x[kJ];
        double s1[2] = {0.0, 0.0};                                // sum w u, and the count of samples that are not finite
#pragma unroll
        for (int j = 0; j < kJ; ++j) {
            const T uv = c == 0 ? u[0][j] : (c == 1 ? u[1][j] : u[2][j]);
            x[j] = (double)uv;
            if (!(__builtin_fabs(x[j]) <= 1.79769313486231570815e308)) s1[1] += 1.0;
            s1[0] = __builtin_fma(w[j], x[j], s1[0]);
        }
        block_sum_all<2>(s1, red);
        if (s1[1] > 0.0) {                                        // a sample that is not finite
            if (tid == 0) {
                nu_row[slot] = nan;
                amp_row[slot] = nan;
            }
            continue;
        }
        const double mean = s1[0] / sw[0];
        double v[kJ];
        double sa[1] = {0.0};
#pragma unroll
        for (int j = 0; j < kJ; ++j) {
            v[j] = w[j] * (x[j] - mean);
            sa[0] += __builtin_fabs(v[j]);
        }
        block_sum_all<1>(sa, red);
        if (!(sa[0] > 0.0)) {                                     // v = 0: the spectrum is 0 everywhere
            if (tid == 0) {
                nu_row[slot] = nan;
                amp_row[slot] = 0.0;
            }
            continue;
        }

        // the coarse stage in float32: |v / sum |v|| <= 1 and no output exceeds 1
        const double inv = 1.0 / sa[0];
        float* zf = reinterpret_cast<float*>(zbuf);
        __syncthreads();                                          // the scratch under zbuf has been read
#pragma unroll
        for (int j = 0; j < kJ; ++j) {
            const int n = tid + j * CHX_BLOCK;
            if (n < 2 * P) zf[n] = n < Tn ? (float)(v[j] * inv) : 0.0f;
        }
        for (int n = kJ * CHX_BLOCK + tid; n < 2 * P; n += CHX_BLOCK) zf[n] = 0.0f;
        __syncthreads();
        if (p & 1) {
            for (int j = tid; j < P / 2; j += CHX_BLOCK) fft_r2_item(zbuf, p, j);
            __syncthreads();
        }
        for (int l = p & ~1; l >= 2; l -= 2) {
            for (int i = tid; i < P / 4; i += CHX_BLOCK) fft_r4_item(zbuf, l, i);
            __syncthreads();
        }
        float bestA = -1.0f;
        int bestK = 0;
        for (int k = tid; k <= P; k += CHX_BLOCK) {               // (ascending: the lane keeps its lowest k on ties)
            const float a = coarse_power(zbuf, p, k);
            if (a > bestA) {
                bestA = a;
                bestK = k;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float oa = __shfl_xor(bestA, off, 64);
            const int ok = __shfl_xor(bestK, off, 64);
            if (oa > bestA || (oa == bestA && ok < bestK)) {
                bestA = oa;
                bestK = ok;
            }
        }
        __syncthreads();                                          // every wave has read the transform: its first bytes are scratch
        if ((tid & 63) == 0) {
            zf[2 * (tid >> 6)] = bestA;
            reinterpret_cast<int*>(zf)[2 * (tid >> 6) + 1] = bestK;
        }
        __syncthreads();
        int k0 = reinterpret_cast<const int*>(zf)[1];
        {
            float a0 = zf[0];
#pragma unroll
            for (int wv = 1; wv < 4; ++wv) {
                const float oa = zf[2 * wv];
                const int ok = reinterpret_cast<const int*>(zf)[2 * wv + 1];
                if (oa > a0 || (oa == a0 && ok < k0)) {
                    a0 = oa;
                    k0 = ok;
                }
            }
        }

        // float64 around k0: the peak and the slopes beside it
        const double dnu = 1.0 / (double)(2 * P);
        double nus[5], fg[20];
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            int k = k0 - 2 + d;
            k = k < 0 ? 0 : (k > P ? P : k);                      // (outside the grid: computed, never chosen)
            nus[d] = (double)k * dnu;
        }
        spectral_sums<5, 1>(v, Tn, nus, fg, red);
        double A[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) A[d] = fg[4 * d] * fg[4 * d] + fg[4 * d + 1] * fg[4 * d + 1];
        const int dp = pick_peak(A, k0, P);
        const int ks = k0 - 2 + dp;
        double Ap = A[1], gm = 0.0, gp = 0.0;
#pragma unroll
        for (int d = 1; d <= 3; ++d) {
            if (d == dp) {
                Ap = A[d];
                gm = slope(fg[4 * (d - 1)], fg[4 * (d - 1) + 1], fg[4 * (d - 1) + 2], fg[4 * (d - 1) + 3]);
                gp = slope(fg[4 * (d + 1)], fg[4 * (d + 1) + 1], fg[4 * (d + 1) + 2], fg[4 * (d + 1) + 3]);
            }
        }
        if (!(Ap > 0.0)) {                                        // the largest value of the grid is 0 (or not a number)
            if (tid == 0) {
                nu_row[slot] = nan;
                amp_row[slot] = Ap == 0.0 ? 0.0 : nan;
            }
            continue;
        }
        double nuhat = (double)ks * dnu;
        if (has_bracket(ks, P, gm, gp)) {
            Root r = root_begin((double)(ks - 1) * dnu, (double)(ks + 1) * dnu, nuhat);
            for (int it = 0; it < kMaxIter; ++it) {
                const double nu1[1] = {r.x};
                double fgh[6];
                spectral_sums<1, 2>(v, Tn, nu1, fgh, red);
                if (root_step(r, slope(fgh[0], fgh[1], fgh[2], fgh[3]), curvature(fgh[0], fgh[1], fgh[2], fgh[3], fgh[4], fgh[5])))
                    break;
            }
            nuhat = r.x;
        }
        const double nu1[1] = {nuhat};
        double f[2];
        spectral_sums<1, 0>(v, Tn, nu1, f, red);
        if (tid == 0) {
            nu_row[slot] = nuhat;
            amp_row[slot] = 2.0 * hypot(f[0], f[1]) / sw[0];
        }
    }
}

}  // namespace

extern "C" int chx_tunes(const void* probe, const int32_t* lost, int64_t R, int64_t S, int64_t r0, int64_t T, int64_t last_turn,
                         int columns, int dtype, double* nu, double* amp, void* stream) {
    if (!probe || !nu || !amp || R < 1 || S < 1 || S > 0x7fffffffLL || r0 < 0 || T < CHX_TUNES_T_MIN || T > CHX_TUNES_T_MAX ||
        r0 > R - T || columns < 1 || columns > 7)
        return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CHX_F32)
        hipLaunchKernelGGL(tunes_kernel<float>, dim3((unsigned)S), dim3(CHX_BLOCK), 0, s, (const float*)probe, lost, S, r0, (int)T,
                           last_turn, columns, nu, amp);
    else
        hipLaunchKernelGGL(tunes_kernel<double>, dim3((unsigned)S), dim3(CHX_BLOCK), 0, s, (const double*)probe, lost, S, r0, (int)T,
                           last_turn, columns, nu, amp);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}
