// chx_grid1d_dev.h — device code shared by the kicks that bin the beam's charge on M nodes in tau (chx_wake.hip,
// chx_csr.hip, chx_lsc.hip): the node coordinate, 64-bit fixed-point deposits, fixed-order reductions, the two particle passes that
// find the row's tau range (F1, wake_range_kernel) and deposit the line density (F2, wake_deposit_kernel), and the particle passes
// of the single-channel kicks (CSR, LSC): the gather-kick F4 (node_kick_kernel) and the backward passes B1 (node_bwd_range_kernel),
// B2 (node_bwd_deposit_kernel) and B4 (node_bwd_particles_kernel), which take the doubles per state row as an argument, and the
// low-pass stage of the calls with a cutoff (grid_filter_kernel) between F2 and a kick's node pass and, backward, in front of its last
// particle pass. Per batch row, every grid quantity in fp64. The host side of the same layer (argument check, workspace, launchers)
// is chx_grid1d_host.h.
#pragma once
#include "chx_common.h"

#include <math.h>

namespace {

constexpr int kWB = CHX_BLOCK;                // threads per workgroup
constexpr int kMaxG = 1024;                   // workgroups per row of a particle pass (the merge: thread t takes t, t + 256, ...)
constexpr int kPart = 8;                      // doubles per workgroup partial
constexpr int kHdr = CHX_WAKE_STATE_HEADER;   // state row header: valid, tau_lo, D, S[3] (fixed-point scales), tau_hi, free slot
constexpr int kNodeBlock = 64;                // nodes per workgroup of the convolution kernels (one per lane)
constexpr double kCoulomb = 8.9875517923e9;   // k_e = 1 / (4 pi eps0), V m / C

inline int wake_groups(int64_t N) {
    const int64_t g = (N + 2047) / 2048;
    return (int)(g < 1 ? 1 : g > kMaxG ? kMaxG : g);
}
inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// Node coordinate of a particle: u = clamp((tau - lo) / D, 0, M - 1) (0 when D = 0), k = min(floor(u), M - 2), f = u - k;
// `in` = the clamp passed u through (du/dtau = 1/D). NaN tau: f = NaN at node 0.
__device__ __forceinline__ void wake_node(double tau, double lo, double D, int M, int& k, double& f, bool& in) {
    in = false;
    if (isnan(tau)) { k = 0; f = tau; return; }
    double u = 0.0;
    if (D > 0.0) {
        const double ur = (tau - lo) / D;
        in = ur >= 0.0 && ur <= (double)(M - 1);
        u = in ? ur : (ur < 0.0 ? 0.0 : (double)(M - 1));
    }
    int kk = (int)floor(u);
    if (kk > M - 2) kk = M - 2;
    k = kk;
    f = u - (double)kk;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}

// Workgroup reduction in a fixed pattern: lo = min, hi = max, s[K] = sums; valid in thread 0.
template <int K>
__device__ __forceinline__ void block_reduce(double& lo, double& hi, double (&s)[K], double* red /* [4][K + 2] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    lo = wave_min(lo);
    hi = wave_max(hi);
#pragma unroll
    for (int c = 0; c < K; ++c) s[c] = chx_wave_sum(s[c]);
    if (lane == 0) {
        red[wave * (K + 2)] = lo;
        red[wave * (K + 2) + 1] = hi;
#pragma unroll
        for (int c = 0; c < K; ++c) red[wave * (K + 2) + 2 + c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < kWB / 64; ++v) {
            lo = fmin(lo, red[v * (K + 2)]);
            hi = fmax(hi, red[v * (K + 2) + 1]);
#pragma unroll
            for (int c = 0; c < K; ++c) s[c] += red[v * (K + 2) + 2 + c];
        }
    }
    __syncthreads();
}

// Fixed-point scale of a channel whose contributions sum (in magnitude) to at most `bound`: 2^(62 - e) with bound < 2^e, so
// every partial sum stays below 2^62 (+ N/2 of rounding) < 2^63. 1 for an empty channel; 0 for a non-finite bound (the
// channel's nodes then read back as NaN).
__device__ __forceinline__ double fixed_scale(double bound) {
    if (!isfinite(bound)) return 0.0;
    if (bound <= 0.0) return 1.0;
    int e;
    frexp(bound, &e);
    int x = 62 - e;
    if (x > 1000) x = 1000;
    return ldexp(1.0, x);
}
__device__ __forceinline__ unsigned long long to_fixed(double v, double S) { return (unsigned long long)__double2ll_rn(v * S); }
__device__ __forceinline__ double from_fixed(unsigned long long v, double S) {
    return S == 0.0 ? __longlong_as_double(0x7ff8000000000000LL) : (double)(long long)v / S;
}

// The row header from the G partials of F1 (every workgroup of F2 computes the same one: a fixed order). hdr in LDS.
__device__ void wake_row_header(const double* __restrict__ part, int G, int M, double* hdr, double* red) {
    const int t = threadIdx.x;
    double lo = INFINITY, hi = -INFINITY, s[3] = {0.0, 0.0, 0.0};
    for (int g = t; g < G; g += kWB) {
        const double* p = part + (int64_t)g * kPart;
        lo = fmin(lo, p[0]); hi = fmax(hi, p[1]); s[0] += p[2]; s[1] += p[3]; s[2] += p[4];
    }
    block_reduce<3>(lo, hi, s, red);
    if (t == 0) {
        const bool valid = hi >= lo;
        hdr[0] = valid ? 1.0 : 0.0;
        hdr[1] = valid ? lo : 0.0;
        hdr[2] = valid ? (hi - lo) / (double)(M - 1) : 0.0;
        for (int c = 0; c < 3; ++c) hdr[3 + c] = fixed_scale(s[c]);
        hdr[6] = valid ? hi : 0.0;
        hdr[7] = 0.0;
    }
    __syncthreads();
}

// p0c = beta gamma m c^2 of a reference energy as `Beam.p0c` (energy and mass in eV), and gamma = energy / mass.
__device__ __forceinline__ double ref_p0c(double energy, double mass, double& gamma) {
    gamma = energy / mass;
    const double beta = fabs(gamma) > 0.0 ? sqrt(fmax(1.0 - 1.0 / (gamma * gamma), 0.0)) : 1.0;
    return beta * gamma * mass;
}

template <typename T> struct RowPtrs {
    const T* x; const T* q; const T* w;
};
template <typename T>
__device__ __forceinline__ RowPtrs<T> row_ptrs(const T* x, const T* q, const T* w, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N,
                                               int64_t b) {
    RowPtrs<T> r;
    r.x = x + (Bx == 1 ? 0 : b) * N * 7;
    r.q = q + (Bq == 1 ? 0 : b) * N;
    r.w = w + (Bw == 1 ? 0 : b) * N;
    return r;
}

// ---- F1: per-workgroup partials over the surviving particles: tau min / max, sum c (and sum c|x|, sum c|y| when has_t); zeroes
// the row's fixed-point grid of grid_row integers ----------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kWB) void wake_range_kernel(const T* __restrict__ x, const T* __restrict__ q, const T* __restrict__ w,
                                                        int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int G, int M, int has_t,
                                                        int64_t grid_row, double* __restrict__ part,
                                                        unsigned long long* __restrict__ grid) {
    __shared__ double red[4 * 5];
    const int64_t b = blockIdx.y;
    const int g = blockIdx.x;
    unsigned long long* gr = grid + b * grid_row;
    for (int64_t i = (int64_t)g * kWB + threadIdx.x; i < grid_row; i += (int64_t)G * kWB) gr[i] = 0ull;
    const RowPtrs<T> r = row_ptrs(x, q, w, Bx, Bq, Bw, N, b);
    const int64_t chunk = (N + G - 1) / G, n0 = g * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
    double lo = INFINITY, hi = -INFINITY, s[3] = {0.0, 0.0, 0.0};
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kWB) {
        const double wn = (double)r.w[n], tau = (double)r.x[n * 7 + 4];
        if (wn > 0.0 && isfinite(tau)) {
            const double c = fabs((double)r.q[n]) * wn;
            lo = fmin(lo, tau);
            hi = fmax(hi, tau);
            s[0] += c;
            if (has_t) {
                s[1] += c * fabs((double)r.x[n * 7]);
                s[2] += c * fabs((double)r.x[n * 7 + 2]);
            }
        }
    }
    block_reduce<3>(lo, hi, s, red);
    if (threadIdx.x == 0) {
        double* p = part + (b * G + g) * kPart;
        p[0] = lo; p[1] = hi; p[2] = s[0]; p[3] = s[1]; p[4] = s[2]; p[5] = p[6] = p[7] = 0.0;
    }
}

// ---- F2: the row header (written to the first kHdr doubles of the row's state, state_row doubles per row) and the fixed-point
// deposit of channels ch0 ... ch0 + nch - 1 (Q, X, Y) into the row's grid (grid_row integers per row, channel c at c M) -------------
template <typename T>
__global__ __launch_bounds__(kWB) void wake_deposit_kernel(const T* __restrict__ x, const T* __restrict__ q, const T* __restrict__ w,
                                                          int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int G, int M, int ch0,
                                                          int nch, int64_t state_row, int64_t grid_row,
                                                          const double* __restrict__ part, double* __restrict__ state,
                                                          unsigned long long* __restrict__ grid) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long hist[];   // [nch][M]
    __shared__ double hdr[kHdr];
    __shared__ double red[4 * 5];
    const int64_t b = blockIdx.y;
    const int g = blockIdx.x;
    wake_row_header(part + b * G * kPart, G, M, hdr, red);
    if (g == 0 && threadIdx.x < kHdr) state[b * state_row + threadIdx.x] = hdr[threadIdx.x];
    if (hdr[0] == 0.0) return;                       // no surviving particle: nothing to deposit
    const double lo = hdr[1], D = hdr[2];
    const double S0 = hdr[3 + ch0], S1 = nch > 1 ? hdr[3 + ch0 + 1] : 0.0, S2 = nch > 2 ? hdr[3 + ch0 + 2] : 0.0;
    for (int i = threadIdx.x; i < nch * M; i += kWB) hist[i] = 0ull;
    __syncthreads();
    const RowPtrs<T> r = row_ptrs(x, q, w, Bx, Bq, Bw, N, b);
    const int64_t chunk = (N + G - 1) / G, n0 = g * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kWB) {
        const double wn = (double)r.w[n], tau = (double)r.x[n * 7 + 4];
        if (!(wn > 0.0 && isfinite(tau))) continue;
        const double c = fabs((double)r.q[n]) * wn;
        int k;
        double f;
        bool in;
        wake_node(tau, lo, D, M, k, f, in);
        const double a0 = (1.0 - f) * c, a1 = f * c;
        if (ch0 == 0) {
            atomicAdd(&hist[k], to_fixed(a0, S0));
            atomicAdd(&hist[k + 1], to_fixed(a1, S0));
        }
        if (ch0 + nch == 3) {                        // transverse channels X, Y: the last two slots
            const double xn = (double)r.x[n * 7], yn = (double)r.x[n * 7 + 2];
            const int sx = nch - 2;
            const double Sx = sx == 0 ? S0 : S1, Sy = sx == 0 ? S1 : S2;
            atomicAdd(&hist[sx * M + k], to_fixed(a0 * xn, Sx));
            atomicAdd(&hist[sx * M + k + 1], to_fixed(a1 * xn, Sx));
            atomicAdd(&hist[(sx + 1) * M + k], to_fixed(a0 * yn, Sy));
            atomicAdd(&hist[(sx + 1) * M + k + 1], to_fixed(a1 * yn, Sy));
        }
    }
    __syncthreads();
    unsigned long long* gr = grid + b * grid_row + ch0 * M;
    for (int i = threadIdx.x; i < nch * M; i += kWB) {
        const unsigned long long v = hist[i];
        if (v) atomicAdd(&gr[i], v);
    }
}

// ---- the low-pass stage between F2 and a kick's node pass, and between a kick's adjoint node pass and its last particle pass: one
// workgroup per (row, channel, tile of kWB nodes) smooths the channel's M values with the Gaussian of rms width s = cutoff / (2 pi h)
// nodes, from `src` into `dst`,
//   R = max(1, min(ceil(4 s), M - 1)), g_d = exp(-d^2 / 2 s^2) / sum_{|e| <= R} g_e, D'_j = sum_{|d| <= R} g_d D_refl(j - d),
// refl(i) = -1 - i for i < 0 and 2 M - 1 - i for i >= M (the row mirrored about its two ends; R <= M - 1, so once is enough). The matrix
// is symmetric (the adjoint is the same stage), its columns sum to 1 (the charge is kept) and no weight is negative (|D'| <= max |D|:
// the fixed-point scale still holds). The weights (formed once per workgroup) and the tile's window j0 - R ... j0 + kWB - 1 + R, already
// mirrored, sit in LDS; D'_j is one thread's sum g_0 D_j + sum_{d = 1 ... R} g_d (D_(j-d) + D_(j+d)) in that order. kFixed: the
// fixed-point grids (channel c scaled by the header's S[c]), else the float64 cotangents. A row without a grid (no survivor, h = 0),
// a cutoff that is not > 0 or not finite, a channel whose scale is 0 (non-finite deposits) and weights that are the identity
// (g_1 = 0) are copied bit for bit.
constexpr double kTwoPi = 6.283185307179586;

template <bool kFixed>
__global__ __launch_bounds__(kWB) void grid_filter_kernel(const double* __restrict__ cutoff, int64_t Bc, int M, int channels,
                                                          const double* __restrict__ state, int64_t state_row,
                                                          const void* __restrict__ src, void* __restrict__ dst) {
    extern __shared__ __attribute__((aligned(16))) double flt[];             // g[M], red[kWB / 64], norm, win[nodes of the tile + 2 R]
    const int64_t b = blockIdx.y;
    const int c = blockIdx.z, t = threadIdx.x, j0 = blockIdx.x * kWB, j = j0 + t;
    const int64_t row = (b * channels + c) * M;
    const unsigned long long* sx = (const unsigned long long*)src + row;
    const double* sd = (const double*)src + row;
    unsigned long long* dx = (unsigned long long*)dst + row;
    double* dd = (double*)dst + row;
    const double* st = state + b * state_row;
    const double h = st[2], lc = cutoff[Bc == 1 ? 0 : b], S = kFixed ? st[3 + c] : 1.0;
    double* g = flt;
    double* red = flt + M;
    double* win = flt + M + kWB / 64 + 1;
    bool copy = st[0] == 0.0 || !(h > 0.0) || !(lc > 0.0) || !isfinite(lc) || S == 0.0;     // the same in every thread
    int R = 0;
    if (!copy) {
        const double s = lc / (kTwoPi * h);
        R = (int)fmax(1.0, fmin(ceil(4.0 * s), (double)(M - 1)));
        double part = 0.0;
        for (int d = t; d <= R; d += kWB) {
            const double r = (double)d / s, v = d == 0 ? 1.0 : exp(-0.5 * r * r);
            g[d] = v;
            part += d == 0 ? v : 2.0 * v;
        }
        part = chx_wave_sum(part);
        if ((t & 63) == 0) red[t >> 6] = part;
        __syncthreads();
        if (t == 0) {
            double n = 0.0;
            for (int v = 0; v < kWB / 64; ++v) n += red[v];
            red[kWB / 64] = n;
        }
        __syncthreads();
        copy = g[1] == 0.0;
    }
    if (copy) {
        if (j < M) {
            if (kFixed) dx[j] = sx[j];
            else dd[j] = sd[j];
        }
        return;
    }
    const double norm = red[kWB / 64];
    const int nodes = M - j0 < kWB ? M - j0 : kWB;
    for (int i = t; i < nodes + 2 * R; i += kWB) {
        int m = j0 - R + i;
        m = m < 0 ? -1 - m : (m >= M ? 2 * M - 1 - m : m);
        win[i] = kFixed ? from_fixed(sx[m], S) : sd[m];
    }
    __syncthreads();
    if (j >= M) return;
    const double* w0 = win + t + R;
    double acc = g[0] * w0[0];
    for (int d = 1; d <= R; ++d) acc += g[d] * (w0[-d] + w0[d]);
    acc /= norm;
    if (kFixed) dx[j] = to_fixed(acc, S);
    else dd[j] = acc;
}

// ---- the particle passes of the kicks whose state row is [header | M node kicks | ...] with the row's scale in the header's last
// slot (chx_csr.hip, chx_lsc.hip): the gather-kick F4 and the backward passes B1, B2, B4; state_row doubles per row ---------------

// The row kicks at all: surviving particles and a node spacing h > 0.
__device__ __forceinline__ bool node_live(const double* st) { return st[0] != 0.0 && st[2] > 0.0; }

// F4, one thread per particle: gather of the node kicks times the row's scale, delta updated in fp64, rounded once.
template <typename T>
__global__ __launch_bounds__(kWB) void node_kick_kernel(const T* __restrict__ x, int64_t Bx, int64_t N, int M,
                                                        const double* __restrict__ state, int64_t state_row, T* __restrict__ out) {
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * kWB + threadIdx.x;
    if (n >= N) return;
    const T* xr = x + ((Bx == 1 ? 0 : b) * N + n) * 7;
    T* o = out + (b * N + n) * 7;
    T v[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) v[c] = xr[c];
    const double* st = state + b * state_row;
    if (node_live(st)) {
        int k;
        double f;
        bool in;
        wake_node((double)v[4], st[1], st[2], M, k, f, in);
        // no field (a scale of 0; both nodes 0: no charge) leaves delta's bits as they are, NaN tau included
        const double sc = st[kHdr - 1], n0 = st[kHdr + k], n1 = st[kHdr + k + 1];
        if (sc != 0.0 && (n0 != 0.0 || n1 != 0.0)) {
            const double dv = sc * ((1.0 - f) * n0 + f * n1);
            if (dv != 0.0) v[5] = (T)((double)v[5] + dv);
        }
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) o[c] = v[c];
}

// B1: bound of the gather's cotangents a = scale g_delta; partials of d(scale) = sum g_delta dE(u); zeroes the cotangents' grid.
template <typename T>
__global__ __launch_bounds__(kWB) void node_bwd_range_kernel(const T* __restrict__ x, int64_t Bx, int64_t N, int G, int M,
                                                             const double* __restrict__ state, int64_t state_row,
                                                             const T* __restrict__ gout, double* __restrict__ bpart,
                                                             unsigned long long* __restrict__ ggrid) {
    __shared__ double red[4 * 4];
    const int64_t b = blockIdx.y;
    const int g = blockIdx.x;
    unsigned long long* gr = ggrid + b * M;
    for (int64_t i = (int64_t)g * kWB + threadIdx.x; i < M; i += (int64_t)G * kWB) gr[i] = 0ull;
    const double* st = state + b * state_row;
    const double* node = st + kHdr;
    const int64_t chunk = (N + G - 1) / G, n0 = g * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
    double lo = 0.0, hi = 0.0, s[2] = {0.0, 0.0};
    if (node_live(st)) {
        const double sc = st[kHdr - 1];
        const T* xb = x + (Bx == 1 ? 0 : b) * N * 7;
        const T* gb = gout + b * N * 7;
        for (int64_t n = n0 + threadIdx.x; n < n1; n += kWB) {
            int k;
            double f;
            bool in;
            wake_node((double)xb[n * 7 + 4], st[1], st[2], M, k, f, in);
            if (isnan(f)) continue;
            const double g5 = (double)gb[n * 7 + 5];
            s[0] += fabs(sc * g5);
            s[1] += g5 * ((1.0 - f) * node[k] + f * node[k + 1]);
        }
    }
    block_reduce<2>(lo, hi, s, red);
    if (threadIdx.x == 0) {
        double* p = bpart + (b * G + g) * kPart;
        p[0] = s[0]; p[1] = s[1]; p[2] = p[3] = p[4] = p[5] = p[6] = p[7] = 0.0;
    }
}

// B2: fixed-point deposit of the gather's cotangents, as F2 (hist: M integers of dynamic LDS); workgroup 0 writes d(scale) and
// the backward header (valid, S of the cotangent deposit).
template <typename T>
__global__ __launch_bounds__(kWB) void node_bwd_deposit_kernel(const T* __restrict__ x, int64_t Bx, int64_t N, int G, int M,
                                                               const double* __restrict__ state, int64_t state_row,
                                                               const T* __restrict__ gout, const double* __restrict__ bpart,
                                                               double* __restrict__ bhdr, double* __restrict__ d_scale,
                                                               unsigned long long* __restrict__ ggrid) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long hist[];   // [M]
    __shared__ double red[4 * 4];
    __shared__ double S;
    const int64_t b = blockIdx.y;
    const int g = blockIdx.x;
    const double* st = state + b * state_row;
    double lo = 0.0, hi = 0.0, s[2] = {0.0, 0.0};
    for (int gg = threadIdx.x; gg < G; gg += kWB) {
        const double* p = bpart + (b * G + gg) * kPart;
        s[0] += p[0]; s[1] += p[1];
    }
    block_reduce<2>(lo, hi, s, red);
    if (threadIdx.x == 0) {
        S = fixed_scale(s[0]);
        if (g == 0) {
            d_scale[b] = s[1];
            bhdr[b * kHdr] = st[0];
            bhdr[b * kHdr + 1] = S;
        }
    }
    __syncthreads();
    if (!node_live(st)) return;
    const double S0 = S;
    for (int i = threadIdx.x; i < M; i += kWB) hist[i] = 0ull;
    __syncthreads();
    const T* xb = x + (Bx == 1 ? 0 : b) * N * 7;
    const T* gb = gout + b * N * 7;
    const double sc = st[kHdr - 1];
    const int64_t chunk = (N + G - 1) / G, n0 = g * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kWB) {
        int k;
        double f;
        bool in;
        wake_node((double)xb[n * 7 + 4], st[1], st[2], M, k, f, in);
        if (isnan(f)) continue;
        const double a = sc * (double)gb[n * 7 + 5];
        atomicAdd(&hist[k], to_fixed((1.0 - f) * a, S0));
        atomicAdd(&hist[k + 1], to_fixed(f * a, S0));
    }
    __syncthreads();
    unsigned long long* gr = ggrid + b * M;
    for (int i = threadIdx.x; i < M; i += kWB) {
        const unsigned long long v = hist[i];
        if (v) atomicAdd(&gr[i], v);
    }
}

// B4, one thread per particle: adjoint of the deposit (adj[B][M]: cotangents of the deposits) and of the node coordinate. A device
// function under node_bwd_particles_kernel, so that a kick with more to do in this pass wraps it in a kernel of its own.
template <typename T>
__device__ __forceinline__ void node_bwd_particle(const T* __restrict__ x, const T* __restrict__ q, const T* __restrict__ w,
                                                  int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int M,
                                                  const double* __restrict__ state, int64_t state_row,
                                                  const double* __restrict__ adj, const T* __restrict__ gout, T* __restrict__ dX,
                                                  T* __restrict__ dC) {
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * kWB + threadIdx.x;
    if (n >= N) return;
    const RowPtrs<T> r = row_ptrs(x, q, w, Bx, Bq, Bw, N, b);
    const T* gr = gout + (b * N + n) * 7;
    double gv[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) gv[c] = (double)gr[c];
    const double* st = state + b * state_row;
    double dc = 0.0;
    if (node_live(st)) {
        const double tau = (double)r.x[n * 7 + 4];
        int k;
        double f;
        bool in;
        wake_node(tau, st[1], st[2], M, k, f, in);
        const double* node = st + kHdr;
        const double* ad = adj + b * M;
        const double sc = st[kHdr - 1];
        double df = sc * gv[5] * (node[k + 1] - node[k]);
        const double wn = (double)r.w[n];
        if (wn > 0.0 && isfinite(tau)) {
            const double c = fabs((double)r.q[n]) * wn;
            dc = (1.0 - f) * ad[k] + f * ad[k + 1];
            df += c * (ad[k + 1] - ad[k]);
        }
        if (in) gv[4] += df / st[2];
    }
    T* o = dX + (b * N + n) * 7;
#pragma unroll
    for (int c = 0; c < 7; ++c) o[c] = (T)gv[c];
    if (dC) dC[b * N + n] = (T)dc;
}

template <typename T>
__global__ __launch_bounds__(kWB) void node_bwd_particles_kernel(const T* __restrict__ x, const T* __restrict__ q,
                                                                 const T* __restrict__ w, int64_t Bx, int64_t Bq, int64_t Bw,
                                                                 int64_t N, int M, const double* __restrict__ state,
                                                                 int64_t state_row, const double* __restrict__ adj,
                                                                 const T* __restrict__ gout, T* __restrict__ dX, T* __restrict__ dC) {
    node_bwd_particle(x, q, w, Bx, Bq, Bw, N, M, state, state_row, adj, gout, dX, dC);
}

// Lane l's double, broadcast to the whole wave (the Toeplitz sums over the nodes: one source tile of 64 nodes per load).
__device__ __forceinline__ double readlane_d(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

}  // namespace
