// chx_wake.hip — short-range wakefield kick (Wakefield element): the beam's charge (and dipole moment) is deposited on M nodes
// in tau, convolved causally with the sampled point-charge wake, interpolated back to every particle and applied as a kick to
// delta (longitudinal) and px, py (transverse dipole). Per batch row, every grid quantity in fp64:
//   F1. wake_range_kernel     per-workgroup partials over the surviving particles (w > 0, finite tau): tau min / max and the
//                             bounds sum c, sum c|x|, sum c|y| (c = |q| w); zeroes the row's fixed-point grid
//   F2. wake_deposit_kernel   every workgroup merges the row's partials in a fixed order (node spacing, fixed-point scales);
//                             node-based linear deposit into LDS histograms of 64-bit integers (ds_add_u64), flushed with
//                             integer global atomics: integer addition is associative, so the grid is bitwise reproducible
//   F3. wake_conv_kernel      one workgroup per (row, 64 nodes): the wake sampled at the node spacing into LDS, the causal
//                             convolution over the deposited nodes, its four waves splitting the sources and merged in order
//   F4. wake_kick_kernel      one thread per particle: gather of the node kicks, delta / px / py updated in fp64, rounded once
// Backward (same pattern): B1 bounds of the cotangents and the per-row partials of d(scale); B2 deposit of the gather's
// cotangents; B3 the anti-causal correlation (adjoint of the convolution) and B4 the correlation for the sampled wakes' gradient;
// B5 one pass over the particles (adjoint of the deposit and of the node coordinate); B6 the tables' gradient (adjoint of the
// sampling), one thread per table entry. F1 and F2 live in chx_grid1d_dev.h; the argument check, the workspace, the dtype dispatch
// and the launcher of F1 and F2 in chx_grid1d_host.h, all shared with the CSR and LSC kicks (chx_csr.hip, chx_lsc.hip). The
// three-channel passes F4, B1, B2 and B5 are this file's own.
#include "chx_grid1d_host.h"

namespace {

__host__ __device__ inline int64_t state_row(int M) { return CHX_WAKE_STATE_DOUBLES(M); }

// Three deposit channels (Q, X, Y); the workspace's own block: dsamp[B][2][M], the cotangents of the sampled wakes (longitudinal,
// transverse).
Grid1dWs wake_ws(void* base, int64_t B, int64_t N, int M) { return grid1d_ws(base, B, N, M, 3, (size_t)(B * 2 * M) * 8); }

// Position of node n in the table: p = n D / h; false beyond the last entry (the wake is 0 there), else entry j and fraction t
// of the linear interpolation (1 - t) T[j] + t T[j + 1] (a table of one entry: j = 0, t = 0).
__device__ __forceinline__ bool wake_table_pos(int n, double D, double h, int64_t L, int64_t& j, double& t) {
    const double p = ((double)n * D) / h;
    if (!(p <= (double)(L - 1))) return false;
    if (L == 1) { j = 0; t = 0.0; return true; }
    int64_t jj = (int64_t)floor(p);
    if (jj > L - 2) jj = L - 2;
    j = jj;
    t = p - (double)jj;
    return true;
}

__device__ __forceinline__ double wake_sample(const double* __restrict__ T, int64_t L, int n, double D, double h) {
    int64_t j;
    double t;
    if (!wake_table_pos(n, D, h, L, j, t)) return 0.0;
    const double v = L == 1 ? T[0] : (1.0 - t) * T[j] + t * T[j + 1];
    return n == 0 ? 0.5 * v : v;     // the self term (beam loading): half the wake at s = 0
}


// ---- F3 ----------------------------------------------------------------------------------------------------------------------
// One workgroup per (row, 64 nodes k0 ... k0 + 63): the sampled wakes W~[n], n < k0 + 64, in LDS behind 64 zeros (a source m > k
// reads a zero); wave v takes the source tiles m0 = 64 (v + 4 i); a tile's 64 deposits are loaded one per lane and broadcast with
// readlane. The four waves' sums are added in order by wave 0.
__global__ __launch_bounds__(kWB) void wake_conv_kernel(const double* __restrict__ wl, int64_t Ll, const double* __restrict__ wt,
                                                       int64_t Lt, const double* __restrict__ hp, int M,
                                                       const unsigned long long* __restrict__ grid, double* __restrict__ state) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // Wl~[64 + M], Wt~[64 + M], acc[4][3][64]
    const int64_t b = blockIdx.y;
    const int k0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* st = state + b * state_row(M);
    const double valid = st[0], D = st[2], h = hp[0];
    double* wsl = lds;
    double* wst = lds + 64 + M;
    double* acc = lds + 2 * (64 + M);
    const int nmax = k0 + kNodeBlock < M ? k0 + kNodeBlock : M;
    for (int i = threadIdx.x; i < 64 + nmax; i += kWB) {
        const int n = i - 64;
        wsl[i] = (n < 0 || Ll == 0) ? 0.0 : wake_sample(wl, Ll, n, D, h);
        wst[i] = (n < 0 || Lt == 0) ? 0.0 : wake_sample(wt, Lt, n, D, h);
    }
    __syncthreads();
    const unsigned long long* gq = grid + b * 3 * M;
    const double SQ = st[3], SX = st[4], SY = st[5];
    const int k = k0 + lane;
    double v = 0.0, ux = 0.0, uy = 0.0;
    if (valid != 0.0) {
        for (int m0 = wave * 64; m0 <= nmax - 1; m0 += kWB) {
            const int m = m0 + lane;
            const double q = (Ll && m < M) ? from_fixed(gq[m], SQ) : 0.0;
            const double xm = (Lt && m < M) ? from_fixed(gq[M + m], SX) : 0.0;
            const double ym = (Lt && m < M) ? from_fixed(gq[2 * M + m], SY) : 0.0;
            const int base = 64 + k - m0;           // W~ index of source m0 + j: base - j >= 1 for every j <= 63
            if (Ll) {
#pragma unroll 16
                for (int j = 0; j < 64; ++j) v += wsl[base - j] * readlane_d(q, j);
            }
            if (Lt) {
#pragma unroll 16
                for (int j = 0; j < 64; ++j) {
                    const double wj = wst[base - j];
                    ux += wj * readlane_d(xm, j);
                    uy += wj * readlane_d(ym, j);
                }
            }
        }
    }
    acc[(wave * 3 + 0) * 64 + lane] = v;
    acc[(wave * 3 + 1) * 64 + lane] = ux;
    acc[(wave * 3 + 2) * 64 + lane] = uy;
    __syncthreads();
    if (wave == 0 && k < M) {
        double s[3];
        for (int c = 0; c < 3; ++c)
            s[c] = ((acc[(0 * 3 + c) * 64 + lane] + acc[(1 * 3 + c) * 64 + lane]) + acc[(2 * 3 + c) * 64 + lane]) +
                   acc[(3 * 3 + c) * 64 + lane];
        double* node = st + kHdr;
        node[k] = -s[0];                            // V: a positive wake takes energy
        node[M + k] = s[1];
        node[2 * M + k] = s[2];
        double* dep = node + 3 * M;                 // the deposits as doubles (for the backward pass)
        const bool ok = valid != 0.0;
        dep[k] = (ok && Ll) ? from_fixed(gq[k], SQ) : 0.0;
        dep[M + k] = (ok && Lt) ? from_fixed(gq[M + k], SX) : 0.0;
        dep[2 * M + k] = (ok && Lt) ? from_fixed(gq[2 * M + k], SY) : 0.0;
    }
}

// ---- F4 ----------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kWB) void wake_kick_kernel(const T* __restrict__ x, int64_t Bx, int64_t N, int M,
                                                       const double* __restrict__ scale, const double* __restrict__ state,
                                                       T* __restrict__ out) {
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * kWB + threadIdx.x;
    if (n >= N) return;
    const T* xr = x + ((Bx == 1 ? 0 : b) * N + n) * 7;
    T* o = out + (b * N + n) * 7;
    T v[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) v[c] = xr[c];
    const double* st = state + b * state_row(M);
    if (st[0] != 0.0) {
        int k;
        double f;
        bool in;
        wake_node((double)v[4], st[1], st[2], M, k, f, in);
        const double* node = st + kHdr;
        const double s = scale[b], g = 1.0 - f;
        const double V = g * node[k] + f * node[k + 1];
        const double Ux = g * node[M + k] + f * node[M + k + 1];
        const double Uy = g * node[2 * M + k] + f * node[2 * M + k + 1];
        v[5] = (T)((double)v[5] + s * V);
        v[1] = (T)((double)v[1] + s * Ux);
        v[3] = (T)((double)v[3] + s * Uy);
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) o[c] = v[c];
}

// ---- B1: bounds of the gather's cotangents a = scale g_delta, bx = scale g_px, by = scale g_py; partials of d(scale) ----------
template <typename T>
__global__ __launch_bounds__(kWB) void wake_bwd_range_kernel(const T* __restrict__ x, int64_t Bx, int64_t N, int G, int M,
                                                            const double* __restrict__ scale, const double* __restrict__ state,
                                                            const T* __restrict__ gout, double* __restrict__ bpart,
                                                            unsigned long long* __restrict__ ggrid) {
    __shared__ double red[4 * 6];
    const int64_t b = blockIdx.y;
    const int g = blockIdx.x;
    unsigned long long* gr = ggrid + b * 3 * M;
    for (int64_t i = (int64_t)g * kWB + threadIdx.x; i < 3 * (int64_t)M; i += (int64_t)G * kWB) gr[i] = 0ull;
    const double* st = state + b * state_row(M);
    const double* node = st + kHdr;
    const int64_t chunk = (N + G - 1) / G, n0 = g * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
    const double sc = scale[b];
    double lo = 0.0, hi = 0.0, s[4] = {0.0, 0.0, 0.0, 0.0};
    if (st[0] != 0.0) {
        const T* xb = x + (Bx == 1 ? 0 : b) * N * 7;
        const T* gb = gout + b * N * 7;
        for (int64_t n = n0 + threadIdx.x; n < n1; n += kWB) {
            int k;
            double f;
            bool in;
            wake_node((double)xb[n * 7 + 4], st[1], st[2], M, k, f, in);
            if (isnan(f)) continue;
            const double g5 = (double)gb[n * 7 + 5], g1 = (double)gb[n * 7 + 1], g3 = (double)gb[n * 7 + 3], e = 1.0 - f;
            s[0] += fabs(sc * g5);
            s[1] += fabs(sc * g1);
            s[2] += fabs(sc * g3);
            s[3] += g5 * (e * node[k] + f * node[k + 1]) + g1 * (e * node[M + k] + f * node[M + k + 1]) +
                    g3 * (e * node[2 * M + k] + f * node[2 * M + k + 1]);
        }
    }
    block_reduce<4>(lo, hi, s, red);
    if (threadIdx.x == 0) {
        double* p = bpart + (b * G + g) * kPart;
        p[0] = s[0]; p[1] = s[1]; p[2] = s[2]; p[3] = s[3]; p[4] = p[5] = p[6] = p[7] = 0.0;
    }
}

// ---- B2: deposit of the gather's cotangents (GV, GUx, GUy), fixed point like F2; workgroup 0 writes d(scale) -----------------
template <typename T>
__global__ __launch_bounds__(kWB) void wake_bwd_deposit_kernel(const T* __restrict__ x, int64_t Bx, int64_t N, int G, int M, int ch0,
                                                              int nch, const double* __restrict__ scale,
                                                              const double* __restrict__ state, const T* __restrict__ gout,
                                                              const double* __restrict__ bpart, double* __restrict__ bhdr,
                                                              double* __restrict__ d_scale, unsigned long long* __restrict__ ggrid) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long hist[];
    __shared__ double red[4 * 6];
    __shared__ double S[4];
    const int64_t b = blockIdx.y;
    const int g = blockIdx.x;
    const double* st = state + b * state_row(M);
    double lo = 0.0, hi = 0.0, s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int gg = threadIdx.x; gg < G; gg += kWB) {
        const double* p = bpart + (b * G + gg) * kPart;
        s[0] += p[0]; s[1] += p[1]; s[2] += p[2]; s[3] += p[3];
    }
    block_reduce<4>(lo, hi, s, red);
    if (threadIdx.x == 0) {
        for (int c = 0; c < 3; ++c) S[c] = fixed_scale(s[c]);
        if (g == 0) {
            d_scale[b] = s[3];
            double* bh = bhdr + b * kHdr;
            bh[0] = st[0];
            for (int c = 0; c < 3; ++c) bh[1 + c] = S[c];
        }
    }
    __syncthreads();
    if (st[0] == 0.0) return;
    const double S0 = S[ch0], S1 = nch > 1 ? S[ch0 + 1] : 0.0, S2 = nch > 2 ? S[ch0 + 2] : 0.0;
    for (int i = threadIdx.x; i < nch * M; i += kWB) hist[i] = 0ull;
    __syncthreads();
    const T* xb = x + (Bx == 1 ? 0 : b) * N * 7;
    const T* gb = gout + b * N * 7;
    const double sc = scale[b];
    const int64_t chunk = (N + G - 1) / G, n0 = g * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kWB) {
        int k;
        double f;
        bool in;
        wake_node((double)xb[n * 7 + 4], st[1], st[2], M, k, f, in);
        if (isnan(f)) continue;
        const double e = 1.0 - f;
        if (ch0 == 0) {
            const double a = sc * (double)gb[n * 7 + 5];
            atomicAdd(&hist[k], to_fixed(e * a, S0));
            atomicAdd(&hist[k + 1], to_fixed(f * a, S0));
        }
        if (ch0 + nch == 3) {
            const int sx = nch - 2;
            const double Sx = sx == 0 ? S0 : S1, Sy = sx == 0 ? S1 : S2;
            const double bx = sc * (double)gb[n * 7 + 1], by = sc * (double)gb[n * 7 + 3];
            atomicAdd(&hist[sx * M + k], to_fixed(e * bx, Sx));
            atomicAdd(&hist[sx * M + k + 1], to_fixed(f * bx, Sx));
            atomicAdd(&hist[(sx + 1) * M + k], to_fixed(e * by, Sy));
            atomicAdd(&hist[(sx + 1) * M + k + 1], to_fixed(f * by, Sy));
        }
    }
    __syncthreads();
    unsigned long long* gr = ggrid + (b * 3 + ch0) * M;
    for (int i = threadIdx.x; i < nch * M; i += kWB) {
        const unsigned long long v = hist[i];
        if (v) atomicAdd(&gr[i], v);
    }
}

// ---- B3: adjoint of the causal convolution, GQ_m = -sum_{k >= m} Wl~[k - m] GV_k, GX_m = sum Wt~[k - m] GUx_k, GY likewise ----
// One workgroup per (row, 64 sources m0 ... m0 + 63); the sampled wakes for every lag in LDS with 64 zeros IN FRONT (lane m of a
// tile k0 < m reads a zero); wave v takes the tiles k0 = m0 + 64 (v + 4 i).
__global__ __launch_bounds__(kWB) void wake_bwd_conv_kernel(const double* __restrict__ wl, int64_t Ll, const double* __restrict__ wt,
                                                           int64_t Lt, const double* __restrict__ hp, int M,
                                                           const double* __restrict__ state, const double* __restrict__ bhdr,
                                                           const unsigned long long* __restrict__ ggrid, double* __restrict__ adj) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // Wl~[64 + M], Wt~[64 + M], acc[4][3][64]
    const int64_t b = blockIdx.y;
    const int m0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* st = state + b * state_row(M);
    const double* bh = bhdr + b * kHdr;
    const double valid = st[0], D = st[2], h = hp[0];
    double* wsl = lds;
    double* wst = lds + 64 + M;
    double* acc = lds + 2 * (64 + M);
    for (int i = threadIdx.x; i < 64 + M; i += kWB) {
        const int n = i - 64;
        wsl[i] = (n < 0 || Ll == 0) ? 0.0 : wake_sample(wl, Ll, n, D, h);
        wst[i] = (n < 0 || Lt == 0) ? 0.0 : wake_sample(wt, Lt, n, D, h);
    }
    __syncthreads();
    const unsigned long long* gg = ggrid + b * 3 * M;
    const double SV = bh[1], SX = bh[2], SY = bh[3];
    const int m = m0 + lane;
    double v = 0.0, gx = 0.0, gy = 0.0;
    if (valid != 0.0) {
        for (int k0 = m0 + wave * 64; k0 < M; k0 += kWB) {
            const int k = k0 + lane;
            const double a = (Ll && k < M) ? from_fixed(gg[k], SV) : 0.0;
            const double bx = (Lt && k < M) ? from_fixed(gg[M + k], SX) : 0.0;
            const double by = (Lt && k < M) ? from_fixed(gg[2 * M + k], SY) : 0.0;
            const int base = 64 + k0 - m;           // W~ index of target k0 + j: base + j, >= 1 for every j >= 0
            if (Ll) {
#pragma unroll 16
                for (int j = 0; j < 64; ++j) {
                    const int idx = base + j;
                    v += (idx < 64 + M ? wsl[idx] : 0.0) * readlane_d(a, j);
                }
            }
            if (Lt) {
#pragma unroll 16
                for (int j = 0; j < 64; ++j) {
                    const int idx = base + j;
                    const double wj = idx < 64 + M ? wst[idx] : 0.0;
                    gx += wj * readlane_d(bx, j);
                    gy += wj * readlane_d(by, j);
                }
            }
        }
    }
    acc[(wave * 3 + 0) * 64 + lane] = v;
    acc[(wave * 3 + 1) * 64 + lane] = gx;
    acc[(wave * 3 + 2) * 64 + lane] = gy;
    __syncthreads();
    if (wave == 0 && m < M) {
        double* ad = adj + b * 3 * M;
        for (int c = 0; c < 3; ++c) {
            const double s = ((acc[(0 * 3 + c) * 64 + lane] + acc[(1 * 3 + c) * 64 + lane]) + acc[(2 * 3 + c) * 64 + lane]) +
                             acc[(3 * 3 + c) * 64 + lane];
            ad[c * M + m] = c == 0 ? -s : s;
        }
    }
}

// ---- B4: cotangents of the sampled wakes, dWl~_j = -sum_m GV_{m + j} Q_m, dWt~_j = sum_m GUx_{m + j} X_m + GUy_{m + j} Y_m -------
// One workgroup per (row, 64 lags j0 ... j0 + 63): the node cotangents as doubles in LDS with 128 zeros BEHIND them; wave v takes
// the source tiles m = 64 (v + 4 i) < M - j0.
__global__ __launch_bounds__(kWB) void wake_bwd_table_samples_kernel(int has_l, int has_t, int M, const double* __restrict__ state,
                                                                    const double* __restrict__ bhdr,
                                                                    const unsigned long long* __restrict__ ggrid,
                                                                    double* __restrict__ dsamp) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // G[3][M + 128], acc[4][2][64]
    const int64_t b = blockIdx.y;
    const int j0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* st = state + b * state_row(M);
    const double* bh = bhdr + b * kHdr;
    const int ML = M + 128;                    // zeros behind: index m + j <= M + 125 for every tile taken
    double* G = lds;
    double* acc = lds + 3 * ML;
    const unsigned long long* gg = ggrid + b * 3 * M;
    const double valid = st[0];
    for (int i = threadIdx.x; i < 3 * ML; i += kWB) {
        const int c = i / ML, n = i - c * ML;
        const bool on = valid != 0.0 && n < M && (c == 0 ? has_l : has_t);
        G[i] = on ? from_fixed(gg[c * M + n], bh[1 + c]) : 0.0;
    }
    __syncthreads();
    const double* dep = st + kHdr + 3 * M;
    const int j = j0 + lane;
    double dl = 0.0, dt = 0.0;
    if (valid != 0.0) {
        for (int mt = wave * 64; mt < M - j0; mt += kWB) {
            const int m = mt + lane;
            const double qm = (has_l && m < M) ? dep[m] : 0.0;
            const double xm = (has_t && m < M) ? dep[M + m] : 0.0;
            const double ym = (has_t && m < M) ? dep[2 * M + m] : 0.0;
            const int base = mt + j;                // G index of source mt + i
            if (has_l) {
#pragma unroll 16
                for (int i = 0; i < 64; ++i) dl += G[base + i] * readlane_d(qm, i);
            }
            if (has_t) {
#pragma unroll 16
                for (int i = 0; i < 64; ++i) dt += G[ML + base + i] * readlane_d(xm, i) + G[2 * ML + base + i] * readlane_d(ym, i);
            }
        }
    }
    acc[(wave * 2 + 0) * 64 + lane] = dl;
    acc[(wave * 2 + 1) * 64 + lane] = dt;
    __syncthreads();
    if (wave == 0 && j < M) {
        double* ds = dsamp + b * 2 * M;
        for (int c = 0; c < 2; ++c) {
            const double s = ((acc[(0 * 2 + c) * 64 + lane] + acc[(1 * 2 + c) * 64 + lane]) + acc[(2 * 2 + c) * 64 + lane]) +
                             acc[(3 * 2 + c) * 64 + lane];
            ds[c * M + j] = c == 0 ? -s : s;
        }
    }
}

// ---- B5: one pass over the particles ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kWB) void wake_bwd_particles_kernel(const T* __restrict__ x, const T* __restrict__ q,
                                                                const T* __restrict__ w, int64_t Bx, int64_t Bq, int64_t Bw,
                                                                int64_t N, int M, int has_t, const double* __restrict__ scale,
                                                                const double* __restrict__ state, const double* __restrict__ adj,
                                                                const T* __restrict__ gout, T* __restrict__ dX, T* __restrict__ dC) {
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * kWB + threadIdx.x;
    if (n >= N) return;
    const RowPtrs<T> r = row_ptrs(x, q, w, Bx, Bq, Bw, N, b);
    const T* gr = gout + (b * N + n) * 7;
    double gv[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) gv[c] = (double)gr[c];
    const double* st = state + b * state_row(M);
    double dc = 0.0;
    if (st[0] != 0.0) {
        const double tau = (double)r.x[n * 7 + 4];
        int k;
        double f;
        bool in;
        wake_node(tau, st[1], st[2], M, k, f, in);
        const double* node = st + kHdr;
        const double* ad = adj + b * 3 * M;
        const double sc = scale[b], e = 1.0 - f;
        double df = sc * gv[5] * (node[k + 1] - node[k]) + sc * gv[1] * (node[M + k + 1] - node[M + k]) +
                    sc * gv[3] * (node[2 * M + k + 1] - node[2 * M + k]);
        const double wn = (double)r.w[n];
        if (wn > 0.0 && isfinite(tau)) {
            const double c = fabs((double)r.q[n]) * wn;
            dc = e * ad[k] + f * ad[k + 1];
            double dfd = ad[k + 1] - ad[k];
            if (has_t) {
                const double xn = (double)r.x[n * 7], yn = (double)r.x[n * 7 + 2];
                const double GX = e * ad[M + k] + f * ad[M + k + 1], GY = e * ad[2 * M + k] + f * ad[2 * M + k + 1];
                dc += xn * GX + yn * GY;
                gv[0] += c * GX;
                gv[2] += c * GY;
                dfd += xn * (ad[M + k + 1] - ad[M + k]) + yn * (ad[2 * M + k + 1] - ad[2 * M + k]);
            }
            df += c * dfd;
        }
        if (in) gv[4] += df / st[2];
    }
    T* o = dX + (b * N + n) * 7;
#pragma unroll
    for (int c = 0; c < 7; ++c) o[c] = (T)gv[c];
    if (dC) dC[b * N + n] = (T)dc;
}

// ---- B6: the tables' gradient: entry j collects (1 - t) and t of every node sampled next to it, over all rows ---------------------
__global__ __launch_bounds__(kWB) void wake_bwd_tables_kernel(int64_t B, int M, int64_t L, int c, const double* __restrict__ hp,
                                                             const double* __restrict__ state, const double* __restrict__ dsamp,
                                                             double* __restrict__ dT) {
    const int64_t j = (int64_t)blockIdx.x * kWB + threadIdx.x;
    if (j >= L) return;
    const double h = hp[0];
    double s = 0.0;
    for (int64_t b = 0; b < B; ++b) {
        const double* st = state + b * state_row(M);
        if (st[0] == 0.0) continue;
        const double D = st[2];
        int nlo = 0, nhi = M - 1;
        if (D > 0.0) {                        // p = n D / h in [j - 1, j + 1] (+ margins for the rounding of p)
            const double a = ((double)(j - 1) * h) / D - 2.0, z = ((double)(j + 1) * h) / D + 2.0;
            if (z < 0.0 || a > (double)(M - 1)) continue;
            nlo = a < 0.0 ? 0 : (int)a;
            nhi = z > (double)(M - 1) ? M - 1 : (int)z;
        }
        const double* ds = dsamp + (b * 2 + c) * M;
        for (int n = nlo; n <= nhi; ++n) {
            int64_t jn;
            double t;
            if (!wake_table_pos(n, D, h, L, jn, t)) continue;
            const double g = n == 0 ? 0.5 * ds[n] : ds[n];
            if (jn == j) s += (L == 1 ? 1.0 : 1.0 - t) * g;
            else if (jn + 1 == j) s += t * g;
        }
    }
    dT[j] = s;
}

// The table conditions of the wake on top of check_grid1d.
int check_wake(const void* x, const void* q, const void* w, const double* scale, const double* wl, int64_t Ll, const double* wt,
               int64_t Lt, const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int32_t M, int dtype,
               const double* state) {
    if (!scale || !h || Ll < 0 || Lt < 0 || (Ll == 0 && Lt == 0) || (Ll > 0 && !wl) || (Lt > 0 && !wt)) return CHX_ERR_INVALID_ARG;
    return check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
}

inline size_t conv_lds(int M) { return ((size_t)2 * (64 + M) + 4 * 3 * 64) * sizeof(double); }
inline size_t samples_lds(int M) { return ((size_t)3 * (M + 128) + 4 * 2 * 64) * sizeof(double); }

template <typename T>
int wake_kick_t(const T* x, const T* q, const T* w, const double* scale, const double* wl, int64_t Ll, const double* wt, int64_t Lt,
                const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int M, T* out, double* state,
                const Grid1dWs& ws, hipStream_t s) {
    const int has_l = Ll > 0, has_t = Lt > 0;
    const int ch0 = has_l ? 0 : 1, nch = has_t ? 3 - ch0 : 1;
    if (!lds_ok(wake_conv_kernel, conv_lds(M))) return CHX_ERR_LAUNCH;
    int st = launch_deposit(x, q, w, B, Bx, Bq, Bw, N, M, ch0, nch, 3, state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(wake_conv_kernel, dim3((unsigned)((M + kNodeBlock - 1) / kNodeBlock), (unsigned)B), dim3(kWB), conv_lds(M), s,
                       wl, Ll, wt, Lt, h, M, ws.grid, state);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(wake_kick_kernel<T>, dim3((unsigned)((N + kWB - 1) / kWB), (unsigned)B), dim3(kWB), 0, s, x, Bx, N, M, scale,
                       state, out);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

template <typename T>
int wake_kick_bwd_t(const T* x, const T* q, const T* w, const double* scale, const double* wl, int64_t Ll, const double* wt,
                    int64_t Lt, const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int M, const double* state,
                    const T* gout, T* dX, T* dC, double* d_scale, double* d_wl, double* d_wt, const Grid1dWs& ws, hipStream_t s) {
    const int G = wake_groups(N);
    const int has_l = Ll > 0, has_t = Lt > 0;
    const int ch0 = has_l ? 0 : 1, nch = has_t ? 3 - ch0 : 1;
    const unsigned nb = (unsigned)((M + kNodeBlock - 1) / kNodeBlock);
    if (!lds_ok(wake_bwd_deposit_kernel<T>, (size_t)nch * M * 8) || !lds_ok(wake_bwd_conv_kernel, conv_lds(M)) ||
        !lds_ok(wake_bwd_table_samples_kernel, samples_lds(M)))
        return CHX_ERR_LAUNCH;
    hipLaunchKernelGGL(wake_bwd_range_kernel<T>, dim3((unsigned)G, (unsigned)B), dim3(kWB), 0, s, x, Bx, N, G, M, scale, state, gout,
                       ws.bpart, ws.ggrid);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(wake_bwd_deposit_kernel<T>, dim3((unsigned)G, (unsigned)B), dim3(kWB), (size_t)nch * M * 8, s, x, Bx, N, G, M,
                       ch0, nch, scale, state, gout, ws.bpart, ws.bhdr, d_scale, ws.ggrid);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(wake_bwd_conv_kernel, dim3(nb, (unsigned)B), dim3(kWB), conv_lds(M), s, wl, Ll, wt, Lt, h, M, state, ws.bhdr,
                       ws.ggrid, ws.adj);
    CHX_CHECK_LAUNCH();
    if (d_wl || d_wt) {
        hipLaunchKernelGGL(wake_bwd_table_samples_kernel, dim3(nb, (unsigned)B), dim3(kWB), samples_lds(M), s, has_l, has_t, M, state,
                           ws.bhdr, ws.ggrid, ws.extra);
        CHX_CHECK_LAUNCH();
        if (d_wl && has_l) {
            hipLaunchKernelGGL(wake_bwd_tables_kernel, dim3((unsigned)((Ll + kWB - 1) / kWB)), dim3(kWB), 0, s, B, M, Ll, 0, h, state,
                               ws.extra, d_wl);
            CHX_CHECK_LAUNCH();
        }
        if (d_wt && has_t) {
            hipLaunchKernelGGL(wake_bwd_tables_kernel, dim3((unsigned)((Lt + kWB - 1) / kWB)), dim3(kWB), 0, s, B, M, Lt, 1, h, state,
                               ws.extra, d_wt);
            CHX_CHECK_LAUNCH();
        }
    }
    const int st = launch_adj_filter(B, M, 3, state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(wake_bwd_particles_kernel<T>, dim3((unsigned)((N + kWB - 1) / kWB), (unsigned)B), dim3(kWB), 0, s, x, q, w, Bx,
                       Bq, Bw, N, M, has_t, scale, state, ws.adj_last, gout, dX, dC);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace

// Every entry point has a twin that takes cutoff[Bcut] in front of the workspace (the low-pass stage of chx_grid1d_dev.h, launched by
// launch_deposit and launch_adj_filter); the call without the suffix is the twin with a null cutoff.
extern "C" size_t chx_wake_workspace_bytes(int64_t B, int64_t N, int32_t M) { return wake_ws(nullptr, B, N, M).bytes; }
extern "C" size_t chx_wake_workspace_bytes_cut(int64_t B, int64_t N, int32_t M) {
    return cutoff_ws_bytes(wake_ws(nullptr, B, N, M), B, M, 3);
}

extern "C" int chx_wake_kick_cut(const void* x, const void* q, const void* w, const double* scale, const double* wl, int64_t Ll,
                                 const double* wt, int64_t Lt, const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                                 int64_t N, int32_t M, int dtype, void* out, double* state, const double* cutoff, int64_t Bcut,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    const int st = check_wake(x, q, w, scale, wl, Ll, wt, Lt, h, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!out) return CHX_ERR_INVALID_ARG;
    if (!chx_aligned16(out)) return CHX_ERR_MISALIGNED;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(wake_ws(workspace, B, N, M), workspace, B, M, 3, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return wake_kick_t<T>((const T*)x, (const T*)q, (const T*)w, scale, wl, Ll, wt, Lt, h, B, Bx, Bq, Bw, N, M, (T*)out, state, ws,
                              (hipStream_t)stream);
    });
}

extern "C" int chx_wake_kick(const void* x, const void* q, const void* w, const double* scale, const double* wl, int64_t Ll,
                             const double* wt, int64_t Lt, const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                             int64_t N, int32_t M, int dtype, void* out, double* state, void* workspace, size_t workspace_bytes,
                             void* stream) {
    return chx_wake_kick_cut(x, q, w, scale, wl, Ll, wt, Lt, h, B, Bx, Bq, Bw, N, M, dtype, out, state, nullptr, 1, workspace,
                             workspace_bytes, stream);
}

extern "C" int chx_wake_kick_bwd_cut(const void* x, const void* q, const void* w, const double* scale, const double* wl, int64_t Ll,
                                     const double* wt, int64_t Lt, const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                                     int64_t N, int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC,
                                     double* d_scale, double* d_wl, double* d_wt, const double* cutoff, int64_t Bcut,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    const int st = check_wake(x, q, w, scale, wl, Ll, wt, Lt, h, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!d_out || !dX || !d_scale) return CHX_ERR_INVALID_ARG;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(wake_ws(workspace, B, N, M), workspace, B, M, 3, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return wake_kick_bwd_t<T>((const T*)x, (const T*)q, (const T*)w, scale, wl, Ll, wt, Lt, h, B, Bx, Bq, Bw, N, M, state,
                                  (const T*)d_out, (T*)dX, (T*)dC, d_scale, d_wl, d_wt, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_wake_kick_bwd(const void* x, const void* q, const void* w, const double* scale, const double* wl, int64_t Ll,
                                 const double* wt, int64_t Lt, const double* h, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                                 int64_t N, int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC,
                                 double* d_scale, double* d_wl, double* d_wt, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    return chx_wake_kick_bwd_cut(x, q, w, scale, wl, Ll, wt, Lt, h, B, Bx, Bq, Bw, N, M, dtype, state, d_out, dX, dC, d_scale, d_wl,
                                 d_wt, nullptr, 1, workspace, workspace_bytes, stream);
}
