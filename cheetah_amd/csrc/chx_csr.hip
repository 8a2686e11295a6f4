// chx_csr.hip — steady-state coherent synchrotron radiation kick (CSRKick element): the 1-D energy change of an ultra-relativistic
// bunch on a circular arc (Derbenev et al., TESLA-FEL 95-05; Saldin, Schneidmiller, Yurkov, NIM A 398 (1997) 373), with the line
// density piecewise linear between M nodes in tau and the kernel (z - z')^(-1/3) integrated exactly over every interval. Per batch
// row, every grid quantity in fp64:
//   F1. wake_range_kernel     (chx_grid1d_dev.h) partials of the surviving particles' tau range and charge; zeroes the grid
//   F2. wake_deposit_kernel   (chx_grid1d_dev.h) the row header and the fixed-point node deposit D_k (one channel)
//   F3. csr_toeplitz_kernel   one workgroup per (row, 64 nodes): b_j = a_(j-1) - a_j formed into LDS, the anti-causal sum
//                             S_k = sum_j b_j D_(k+j) over the nodes behind, its four waves splitting the sources, merged in order
//   F4. node_kick_kernel      (chx_grid1d_dev.h) one thread per particle: gather of the node kicks times the row's scale (formed
//                             by F3 from the energy, L and theta pointers), delta updated in fp64, rounded once
// Backward (same pattern): B1 node_bwd_range_kernel, bounds of the gather's cotangents and the per-row partials of d(scale); B2
// node_bwd_deposit_kernel, their fixed-point deposit; B3 csr_bwd_toeplitz_kernel, the causal correlation (adjoint of the anti-causal
// sum); B4 node_bwd_particles_kernel, one pass over the particles (adjoint of the deposit and of the node coordinate). Only F3 and
// B3 are this file's: the particle passes, the argument check, the workspace and the launchers are chx_grid1d_dev.h and
// chx_grid1d_host.h, shared with chx_wake.hip and chx_lsc.hip.
// The second half of the file is the same kick with the entrance transient (TransientCSRKick element): F3 and B3 with the table of
// the slippage length reached inside the bend, and B4 wrapped to sum the cotangent of that length. The third part is the kick in the
// drift behind the bend (CSRDriftKick element): F3 and B3 with the table of the radiation that left the bend and catches up.
#include "chx_dual.h"
#include "chx_grid1d_host.h"

namespace {

__host__ __device__ inline int64_t csr_state_row(int M) { return CHX_CSR_STATE_DOUBLES(M); }

Grid1dWs csr_ws(void* base, int64_t B, int64_t N, int M) { return grid1d_ws(base, B, N, M, 1, 0); }

// The row's scale |Z| L^(1/3) |theta|^(2/3) / p0c in fp64; p0c = beta gamma m c^2 as `Beam.p0c`.
template <typename T>
__device__ __forceinline__ double csr_scale(const T* energy, int64_t Be, const T* length, int64_t Bl, const T* angle, int64_t Ba,
                                            double mass, double absz, int64_t b) {
    const double e = (double)energy[Be == 1 ? 0 : b], L = (double)length[Bl == 1 ? 0 : b], th = (double)angle[Ba == 1 ? 0 : b];
    double gamma;
    const double p0c = ref_p0c(e, mass, gamma);
    const double lf = L > 0.0 ? cbrt(L) : (L == 0.0 ? 0.0 : __longlong_as_double(0x7ff8000000000000LL));
    const double c = cbrt(fabs(th));
    return absz * lf * (c * c) / p0c;
}

// a_j = (j+1)^(2/3) - j^(2/3) without the cancellation.
__device__ __forceinline__ double csr_a(int j) {
    const double x = (double)j, y = x + 1.0, cx = cbrt(x), cy = cbrt(y), cxy = cbrt(x * y);
    return (2.0 * x + 1.0) / (y * cy + cxy * cxy + x * cx);
}

// LDS table bt[i] = b_(i - 128) for lags 0 <= i - 128 < nlag, zero elsewhere (i < M + 256); scratch at[nlag] for a_j. Every lag
// j < nlag the workgroup reads must be inside the table; lags beyond M - 1 only meet zero deposits.
__device__ void csr_b_table(int M, int nlag, double* bt, double* at) {
    for (int j = threadIdx.x; j < nlag; j += kWB) at[j] = csr_a(j);
    __syncthreads();
    for (int i = threadIdx.x; i < M + 256; i += kWB) {
        const int j = i - 128;
        bt[i] = (j < 0 || j >= nlag) ? 0.0 : (j == 0 ? -1.0 : at[j - 1] - at[j]);
    }
    __syncthreads();
}

inline size_t toeplitz_lds(int M) { return ((size_t)2 * M + 256 + 4 * 64) * sizeof(double); }

// A wave's share of the anti-causal sum of node k0 + lane: the source tiles m0 = k0 + 64 (wave + 4 i) < mend; a tile's 64 deposits
// are loaded one per lane and broadcast with readlane. Lag m - k of source m0 + j: bt index 128 + m0 + j - k in [65, M + 190].
__device__ __forceinline__ double toeplitz_fwd_sum(const double* bt, const unsigned long long* __restrict__ gq, double SQ, int k0,
                                                   int mend, int M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = k0 + lane;
    double v = 0.0;
    for (int m0 = k0 + wave * 64; m0 < mend; m0 += kWB) {
        const int m = m0 + lane;
        const double d = m < M ? from_fixed(gq[m], SQ) : 0.0;
        const int base = 128 + m0 - k;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) v += bt[base + j] * readlane_d(d, j);
    }
    return v;
}

// A wave's share of the adjoint (causal) sum of source m0 + lane: the target tiles k0 = 64 (wave + 4 i) < mmax that reach up to node
// kmin or beyond (the tiles in front of it only meet lags whose coefficient is zero). Lag m - k of target k0 + j: bt index
// 128 + m - k0 - j in [65, M + 190] (k0 <= m0).
__device__ __forceinline__ double toeplitz_bwd_sum(const double* bt, const unsigned long long* __restrict__ gg, double SV, int m0,
                                                   int mmax, int kmin, int M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = m0 + lane;
    double v = 0.0;
    for (int k0 = wave * 64; k0 < mmax; k0 += kWB) {
        if (k0 + 63 < kmin) continue;
        const int k = k0 + lane;
        const double a = k < M ? from_fixed(gg[k], SV) : 0.0;
        const int base = 128 + m - k0;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) v += bt[base - j] * readlane_d(a, j);
    }
    return v;
}

// ---- F3 ----------------------------------------------------------------------------------------------------------------------
// One workgroup per (row, 64 nodes k0 ... k0 + 63); workgroup 0 stores the row's scale in the last header slot, where F4 and the
// backward pass read it; wave v takes the source tiles m0 = k0 + 64 (v + 4 i) < M (toeplitz_fwd_sum).
template <typename T>
__global__ __launch_bounds__(kWB) void csr_toeplitz_kernel(int M, const T* __restrict__ energy, int64_t Be,
                                                           const T* __restrict__ length, int64_t Bl, const T* __restrict__ angle,
                                                           int64_t Ba, double mass, double absz,
                                                           const unsigned long long* __restrict__ grid, double* __restrict__ state) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // bt[M + 256], at[M], acc[4][64]
    const int64_t b = blockIdx.y;
    const int k0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* st = state + b * csr_state_row(M);
    double* bt = lds;
    double* acc = lds + 2 * M + 256;
    const bool live = node_live(st);
    if (blockIdx.x == 0 && threadIdx.x == 0) st[kHdr - 1] = csr_scale(energy, Be, length, Bl, angle, Ba, mass, absz, b);
    if (live) csr_b_table(M, M - k0, bt, lds + M + 256);
    const unsigned long long* gq = grid + b * M;
    const double SQ = st[3], h = st[2];
    const int k = k0 + lane;
    acc[wave * 64 + lane] = live ? toeplitz_fwd_sum(bt, gq, SQ, k0, M, M) : 0.0;
    __syncthreads();
    if (wave == 0 && k < M) {
        const double s = ((acc[lane] + acc[64 + lane]) + acc[128 + lane]) + acc[192 + lane];
        // 3^(2/3) k_e h^(-4/3): the node energy change per unit |Z| L^(1/3) |theta|^(2/3)
        st[kHdr + k] = live ? cbrt(9.0) * kCoulomb / (h * cbrt(h)) * s : 0.0;
    }
}

// ---- B3: adjoint of F3, GD_m = 3^(2/3) k_e h^(-4/3) sum_{k <= m} b_(m-k) GV_k ------------------------------------------------------
// One workgroup per (row, 64 sources m0 ... m0 + 63); wave v takes the target tiles k0 = 64 (v + 4 i) <= m0 + 63 (toeplitz_bwd_sum).
__global__ __launch_bounds__(kWB) void csr_bwd_toeplitz_kernel(int M, const double* __restrict__ state, const double* __restrict__ bhdr,
                                                               const unsigned long long* __restrict__ ggrid, double* __restrict__ adj) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // bt[M + 256], at[M], acc[4][64]
    const int64_t b = blockIdx.y;
    const int m0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* st = state + b * csr_state_row(M);
    double* bt = lds;
    double* acc = lds + 2 * M + 256;
    const int mmax = m0 + kNodeBlock < M ? m0 + kNodeBlock : M;     // sources m < mmax: lags up to mmax - 1
    const bool live = node_live(st);
    if (live) csr_b_table(M, mmax, bt, lds + M + 256);
    const unsigned long long* gg = ggrid + b * M;
    const double SV = bhdr[b * kHdr + 1], h = st[2];
    const int m = m0 + lane;
    acc[wave * 64 + lane] = live ? toeplitz_bwd_sum(bt, gg, SV, m0, mmax, 0, M) : 0.0;
    __syncthreads();
    if (wave == 0 && m < M) {
        const double s = ((acc[lane] + acc[64 + lane]) + acc[128 + lane]) + acc[192 + lane];
        adj[b * M + m] = live ? cbrt(9.0) * kCoulomb / (h * cbrt(h)) * s : 0.0;
    }
}

template <typename T>
int csr_kick_t(const T* x, const T* q, const T* w, const T* energy, const T* length, const T* angle, double mass, double absz,
               int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl, int64_t Ba, int64_t N, int M, T* out,
               double* state, const Grid1dWs& ws, hipStream_t s) {
    if (!lds_ok(csr_toeplitz_kernel<T>, toeplitz_lds(M))) return CHX_ERR_LAUNCH;
    int st = launch_deposit(x, q, w, B, Bx, Bq, Bw, N, M, 0, 1, 1, csr_state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(csr_toeplitz_kernel<T>, grid_nodes(M, B), dim3(kWB), toeplitz_lds(M), s, M, energy, Be, length, Bl, angle, Ba,
                       mass, absz, ws.grid, state);
    CHX_CHECK_LAUNCH();
    return launch_node_kick(x, B, Bx, N, M, csr_state_row(M), state, out, s);
}

template <typename T>
int csr_kick_bwd_t(const T* x, const T* q, const T* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int M,
                   const double* state, const T* gout, T* dX, T* dC, double* d_scale, const Grid1dWs& ws, hipStream_t s) {
    if (!lds_ok(csr_bwd_toeplitz_kernel, toeplitz_lds(M))) return CHX_ERR_LAUNCH;
    int st = launch_node_bwd_deposit(x, B, Bx, N, M, csr_state_row(M), state, gout, d_scale, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(csr_bwd_toeplitz_kernel, grid_nodes(M, B), dim3(kWB), toeplitz_lds(M), s, M, state, ws.bhdr, ws.ggrid, ws.adj);
    CHX_CHECK_LAUNCH();
    st = launch_adj_filter(B, M, 1, csr_state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(node_bwd_particles_kernel<T>, grid_particles(N, B), dim3(kWB), 0, s, x, q, w, Bx, Bq, Bw, N, M, state,
                       csr_state_row(M), ws.adj_last, gout, dX, dC);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

// ==== the entrance transient (TransientCSRKick element) ===========================================================================
// Saldin, Schneidmiller, Yurkov, NIM A 398 (1997) 373: an arc length d into a bend of radius R behind a long straight the slippage
// length is z_L = d^3 / (24 R^2), x = z_L / h = d^3 theta^2 / (24 L^2 h) nodes, and
//   S_k(x) = sum_j a~_j(x) (D_(k+j+1) - D_(k+j)) - (2/3) x^(-1/3) [D~(k + x) - D~(k + 4x)],   a~_j = min(j+1, x)^(2/3) - min(j, x)^(2/3)
// with D~ the linear interpolation of the deposits (0 beyond node M). As a Toeplitz table: b_j = a~_(j-1) - a~_j, then
// -(2/3) x^(-1/3) (1 - f, f) at the lags (p, p + 1) and +(2/3) x^(-1/3) (1 - f4, f4) at (p4, p4 + 1), p = floor(x), p4 = floor(4x).
// For x >= M the table is the steady state's. F3 and B3 below; the particle passes are the shared ones. State row: the header with
// the row's scale in its last slot | M node kicks | x | a free slot | M deposits D_k.
constexpr int kCsrMaxBlocks = CHX_WAKE_MAX_BINS / kNodeBlock;

__host__ __device__ inline int64_t csrt_state_row(int M) { return CHX_CSR_TRANSIENT_STATE_DOUBLES(M); }
__host__ __device__ inline int csrt_x_slot(int M) { return kHdr + M; }
__host__ __device__ inline int csrt_dep_slot(int M) { return kHdr + M + 2; }

// The workspace's own block: xpart[B][kCsrMaxBlocks], the partials of d(x), one per workgroup of B3.
Grid1dWs csrt_ws(void* base, int64_t B, int64_t N, int M) { return grid1d_ws(base, B, N, M, 1, (size_t)(B * kCsrMaxBlocks) * 8); }

// The row's x = d^3 theta^2 / (24 L^2 h) in fp64: 0 (no kick) where L, theta or d is 0, NaN for a negative L or d.
template <typename T>
__device__ __forceinline__ double csrt_x(const T* length, int64_t Bl, const T* angle, int64_t Ba, const T* distance, int64_t Bd,
                                         double h, int64_t b) {
    const double L = (double)length[Bl == 1 ? 0 : b], th = (double)angle[Ba == 1 ? 0 : b], d = (double)distance[Bd == 1 ? 0 : b];
    if (L == 0.0 || th == 0.0 || d == 0.0) return 0.0;
    if (L > 0.0 && d > 0.0) return d * d * d * th * th / (24.0 * L * L * h);
    return __longlong_as_double(0x7ff8000000000000LL);
}

// x > 0 taken apart: p = floor(x) and p4 = floor(4x) clamped to M in double (x may be 1e30) with the fractions f, f4 (only used
// below the clamp), cx = (2/3) x^(-1/3), and nl = min(M, p4 + 2): the lags j >= nl have b_j = 0.
struct CsrLags {
    int p, p4, nl;
    double f, f4, cx;
};
__device__ __forceinline__ CsrLags csr_lags(double x, int M) {
    CsrLags g;
    const double pd = fmin(floor(x), (double)M), p4d = fmin(floor(4.0 * x), (double)M);
    g.p = (int)pd;
    g.p4 = (int)p4d;
    g.f = x - pd;
    g.f4 = 4.0 * x - p4d;
    g.nl = g.p4 + 2 < M ? g.p4 + 2 : M;
    g.cx = 2.0 / (3.0 * cbrt(x));
    return g;
}

// LDS table bt[i] = b_(i - 128)(x) for lags 0 <= i - 128 < nlag, zero elsewhere (i < M + 256); scratch at[nlag] for a~_j: csr_a(j)
// for the full intervals j < p and the same cancellation-free form, (x - p)(x + p) / (x^(4/3) + (x p)^(2/3) + p^(4/3)), for the
// partial one. Where x and 4x lie between the same two nodes (x < 1/4) the two interpolations are taken together, (f - f4) and
// (f4 - f), so that b stays accurate as x -> 0, where it goes as x^(2/3).
__device__ void csrt_b_table(int M, int nlag, double x, const CsrLags& g, double* bt, double* at) {
    for (int j = threadIdx.x; j < nlag; j += kWB) {
        double a = 0.0;
        if (j < g.p) {
            a = csr_a(j);
        } else if (j == g.p) {
            const double pp = (double)j, cxp = cbrt(x * pp);
            a = (x - pp) * (x + pp) / (x * cbrt(x) + cxp * cxp + pp * cbrt(pp));
        }
        at[j] = a;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < M + 256; i += kWB) {
        const int j = i - 128;
        double bj = 0.0;
        if (j >= 0 && j < nlag) {
            bj = j == 0 ? (g.p > 0 ? -1.0 : -at[0]) : at[j - 1] - at[j];
            if (g.p4 == g.p) {
                if (j == g.p) bj += g.cx * (g.f - g.f4);
                else if (j == g.p + 1) bj += g.cx * (g.f4 - g.f);
            } else {
                if (j == g.p) bj -= g.cx * (1.0 - g.f);
                else if (j == g.p + 1) bj -= g.cx * g.f;
                if (j == g.p4) bj += g.cx * (1.0 - g.f4);
                else if (j == g.p4 + 1) bj += g.cx * g.f4;
            }
        }
        bt[i] = bj;
    }
    __syncthreads();
}

// ---- F3 of the transient: csr_toeplitz_kernel with the table of the row's x; workgroup 0 stores the row's scale and x in the state
// row, where F4 and the backward pass read them. The source tiles behind the last non-zero lag are skipped.
template <typename T>
__global__ __launch_bounds__(kWB) void csrt_toeplitz_kernel(int M, const T* __restrict__ energy, int64_t Be,
                                                            const T* __restrict__ length, int64_t Bl, const T* __restrict__ angle,
                                                            int64_t Ba, const T* __restrict__ distance, int64_t Bd, double mass,
                                                            double absz, const unsigned long long* __restrict__ grid,
                                                            double* __restrict__ state) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // bt[M + 256], at[M], acc[4][64]
    const int64_t b = blockIdx.y;
    const int k0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* st = state + b * csrt_state_row(M);
    double* bt = lds;
    double* acc = lds + 2 * M + 256;
    const bool live = node_live(st);
    const double SQ = st[3], h = st[2];
    const double x = live ? csrt_x(length, Bl, angle, Ba, distance, Bd, h, b) : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[kHdr - 1] = csr_scale(energy, Be, length, Bl, angle, Ba, mass, absz, b);
        st[csrt_x_slot(M)] = x;
        st[csrt_x_slot(M) + 1] = 0.0;
    }
    const bool ok = live && x > 0.0;
    const CsrLags g = csr_lags(ok ? x : 1.0, M);
    if (ok) csrt_b_table(M, M - k0 < g.nl ? M - k0 : g.nl, x, g, bt, lds + M + 256);
    const unsigned long long* gq = grid + b * M;
    const int k = k0 + lane;
    const int mend = k0 + 63 + g.nl < M ? k0 + 63 + g.nl : M;       // sources m >= mend: lags >= nl for every node of the block
    acc[wave * 64 + lane] = ok ? toeplitz_fwd_sum(bt, gq, SQ, k0, mend, M) : 0.0;
    __syncthreads();
    if (wave == 0 && k < M) {
        const double s = ((acc[lane] + acc[64 + lane]) + acc[128 + lane]) + acc[192 + lane];
        st[kHdr + k] = ok ? cbrt(9.0) * kCoulomb / (h * cbrt(h)) * s : (live && x != x ? x : 0.0);
        st[csrt_dep_slot(M) + k] = live ? from_fixed(gq[k], SQ) : 0.0;
    }
}

// ---- B3 of the transient: csr_bwd_toeplitz_kernel with the table of the row's x, and the workgroup's partial of d(x) = sum_k GV_k
// 3^(2/3) k_e h^(-4/3) dS_k/dx over its 64 nodes, dS_k/dx = (2/9) x^(-4/3) [D~(k + x) - D~(k + 4x)] + (8/3) x^(-1/3) (D_(k+p4+1) -
// D_(k+p4)) (the derivative of the partial a~ cancels against the interpolation's slope at k + x).
__global__ __launch_bounds__(kWB) void csrt_bwd_toeplitz_kernel(int M, const double* __restrict__ state,
                                                                const double* __restrict__ bhdr,
                                                                const unsigned long long* __restrict__ ggrid,
                                                                double* __restrict__ adj, double* __restrict__ xpart) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // bt[M + 256], at[M], acc[4][64]
    const int64_t b = blockIdx.y;
    const int m0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* st = state + b * csrt_state_row(M);
    double* bt = lds;
    double* acc = lds + 2 * M + 256;
    const int mmax = m0 + kNodeBlock < M ? m0 + kNodeBlock : M;     // sources m < mmax: lags up to mmax - 1
    const bool live = node_live(st);
    const double x = st[csrt_x_slot(M)];
    const bool ok = live && x > 0.0;
    const CsrLags g = csr_lags(ok ? x : 1.0, M);
    if (ok) csrt_b_table(M, mmax < g.nl ? mmax : g.nl, x, g, bt, lds + M + 256);
    const unsigned long long* gg = ggrid + b * M;
    const double SV = bhdr[b * kHdr + 1], h = st[2];
    const int m = m0 + lane;
    acc[wave * 64 + lane] = ok ? toeplitz_bwd_sum(bt, gg, SV, m0, mmax, m0 - g.nl + 1, M) : 0.0;
    __syncthreads();
    if (wave == 0) {
        const double nan_x = live && x != x ? x : 0.0;
        double xp = 0.0;
        if (m < M) {
            const double s = ((acc[lane] + acc[64 + lane]) + acc[128 + lane]) + acc[192 + lane];
            const double factor = cbrt(9.0) * kCoulomb / (h * cbrt(h));
            adj[b * M + m] = ok ? factor * s : nan_x;
            xp = nan_x;
            if (ok && m + g.p < M) {                                // beyond: every deposit dS_m/dx meets is zero
                const double* D = st + csrt_dep_slot(M);
                const int i = m + g.p, i4 = m + g.p4;
                const double d0 = D[i], d1 = i + 1 < M ? D[i + 1] : 0.0;
                const double e0 = i4 < M ? D[i4] : 0.0, e1 = i4 + 1 < M ? D[i4 + 1] : 0.0;
                const double diff = g.p4 == g.p ? (g.f - g.f4) * (d1 - d0)
                                                : ((1.0 - g.f) * d0 + g.f * d1) - (i4 < M ? (1.0 - g.f4) * e0 + g.f4 * e1 : 0.0);
                const double dsdx = g.cx / (3.0 * x) * diff + 4.0 * g.cx * (e1 - e0);
                xp = from_fixed(gg[m], SV) * factor * dsdx;
            }
        }
        xp = chx_wave_sum(xp);
        if (lane == 0) xpart[b * kCsrMaxBlocks + blockIdx.x] = xp;
    }
}

// ---- B4 of the transient: one pass over the particles; the first thread of a row adds the workgroups' partials of d(x) in order
template <typename T>
__global__ __launch_bounds__(kWB) void csrt_bwd_particles_kernel(const T* __restrict__ x, const T* __restrict__ q,
                                                                 const T* __restrict__ w, int64_t Bx, int64_t Bq, int64_t Bw,
                                                                 int64_t N, int M, const double* __restrict__ state,
                                                                 const double* __restrict__ adj, const double* __restrict__ xpart,
                                                                 const T* __restrict__ gout, T* __restrict__ dX, T* __restrict__ dC,
                                                                 double* __restrict__ d_x) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int nb = (M + kNodeBlock - 1) / kNodeBlock;
        double s = 0.0;
        for (int i = 0; i < nb; ++i) s += xpart[(int64_t)blockIdx.y * kCsrMaxBlocks + i];
        d_x[blockIdx.y] = s;
    }
    node_bwd_particle(x, q, w, Bx, Bq, Bw, N, M, state, csrt_state_row(M), adj, gout, dX, dC);
}

template <typename T>
int csrt_kick_t(const T* x, const T* q, const T* w, const T* energy, const T* length, const T* angle, const T* distance, double mass,
                double absz, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl, int64_t Ba, int64_t Bd, int64_t N,
                int M, T* out, double* state, const Grid1dWs& ws, hipStream_t s) {
    if (!lds_ok(csrt_toeplitz_kernel<T>, toeplitz_lds(M))) return CHX_ERR_LAUNCH;
    int st = launch_deposit(x, q, w, B, Bx, Bq, Bw, N, M, 0, 1, 1, csrt_state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(csrt_toeplitz_kernel<T>, grid_nodes(M, B), dim3(kWB), toeplitz_lds(M), s, M, energy, Be, length, Bl, angle, Ba,
                       distance, Bd, mass, absz, ws.grid, state);
    CHX_CHECK_LAUNCH();
    return launch_node_kick(x, B, Bx, N, M, csrt_state_row(M), state, out, s);
}

template <typename T>
int csrt_kick_bwd_t(const T* x, const T* q, const T* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int M,
                    const double* state, const T* gout, T* dX, T* dC, double* d_scale, double* d_x, const Grid1dWs& ws,
                    hipStream_t s) {
    if (!lds_ok(csrt_bwd_toeplitz_kernel, toeplitz_lds(M))) return CHX_ERR_LAUNCH;
    int st = launch_node_bwd_deposit(x, B, Bx, N, M, csrt_state_row(M), state, gout, d_scale, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(csrt_bwd_toeplitz_kernel, grid_nodes(M, B), dim3(kWB), toeplitz_lds(M), s, M, state, ws.bhdr, ws.ggrid, ws.adj,
                       ws.extra);
    CHX_CHECK_LAUNCH();
    st = launch_adj_filter(B, M, 1, csrt_state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(csrt_bwd_particles_kernel<T>, grid_particles(N, B), dim3(kWB), 0, s, x, q, w, Bx, Bq, Bw, N, M, state, ws.adj_last,
                       ws.extra, gout, dX, dC, d_x);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

// ==== the drift behind a bend (CSRDriftKick element) ==============================================================================
// Stupakov and Emma, EPAC 2002, case D: a bunch a distance x behind the exit face of a bend of radius R and angle phi sees the
// radiation emitted inside that bend. With xh = x / R, kappa = 24 h / R, the retarded angle psi(u) the root of
// psi^3 (psi + 4 xh) / (psi + xh) = 24 u / R and y = u(phi) / h = phi^3 (phi + 4 xh) / (kappa (phi + xh)) nodes,
//   S_k = (1 / (2 h^2)) { sum_j [G(psi_(j+1)) - G(psi_j)] (D_(k+j+1) - D_(k+j)) - kappa / (3 (phi + 2 xh)) D~(k + y) }
//   G(psi) = psi^2 / 2 + xh^2 psi / (psi + xh) - xh^2 log1p(psi / xh),   psi_j = min(psi(j h), phi)
// (the deposits beyond node M are 0, as in the kicks above), delta_k += (|Z| k_e L / p0c) S_k. As a Toeplitz table: b_0 = -g_0,
// b_j = g_(j-1) - g_j with g_j = G(psi_(j+1)) - G(psi_j), then -beta (1 - f, f) at the lags (p, p + 1), p = floor(y), f = y - p,
// beta = kappa / (3 (phi + 2 xh)). At xh = 0 and y >= M this is the steady state's table. F3 and B3 below; the particle passes are
// the shared ones. State row: the header with the row's scale |Z| L / p0c in its last slot | M node kicks | xh, phi, kappa, a free
// slot | M deposits D_k.
constexpr int kCsrdPar = 4;                    // doubles per workgroup partial of B3: d(xh), d(phi), d(kappa), a free slot

__host__ __device__ inline int64_t csrd_state_row(int M) { return CHX_CSR_DRIFT_STATE_DOUBLES(M); }
__host__ __device__ inline int csrd_par_slot(int M) { return kHdr + M; }
__host__ __device__ inline int csrd_dep_slot(int M) { return kHdr + M + 4; }

// The workspace's own block: part[B][kCsrMaxBlocks][kCsrdPar], the partials of the shape numbers' cotangents, one per workgroup of B3.
Grid1dWs csrd_ws(void* base, int64_t B, int64_t N, int M) {
    return grid1d_ws(base, B, N, M, 1, (size_t)(B * kCsrMaxBlocks * kCsrdPar) * 8);
}

// The row's scale |Z| L / p0c and its shape numbers xh = x |theta| / L_b, phi = |theta|, kappa = 24 h |theta| / L_b in fp64: all 0
// (no kick) where L, L_b or theta is 0, NaN for a negative L, L_b or x.
struct CsrdRow {
    double scale, xh, phi, kappa;
};
template <typename T>
__device__ __forceinline__ CsrdRow csrd_row(const T* energy, int64_t Be, const T* length, int64_t Bl, const T* bend_length, int64_t Bbl,
                                            const T* bend_angle, int64_t Bba, const T* distance, int64_t Bd, double mass, double absz,
                                            double h, int64_t b) {
    const double e = (double)energy[Be == 1 ? 0 : b], L = (double)length[Bl == 1 ? 0 : b];
    const double Lb = (double)bend_length[Bbl == 1 ? 0 : b], th = (double)bend_angle[Bba == 1 ? 0 : b];
    const double d = (double)distance[Bd == 1 ? 0 : b];
    CsrdRow r = {0.0, 0.0, 0.0, 0.0};
    if (L == 0.0 || Lb == 0.0 || th == 0.0) return r;
    if (L > 0.0 && Lb > 0.0 && d >= 0.0) {
        double gamma;
        r.scale = absz * L / ref_p0c(e, mass, gamma);
        r.phi = fabs(th);
        r.xh = d * r.phi / Lb;
        r.kappa = 24.0 * h * r.phi / Lb;
    } else {
        r.scale = r.xh = r.phi = r.kappa = __longlong_as_double(0x7ff8000000000000LL);
    }
    return r;
}

// The table's arithmetic is written once for double (F3, B3's table) and Dual (B3's derivatives). The entries G(psi_j) grow with j
// while their second differences b_j shrink, so a table that differs in the last bit of its entries differs by far more than that
// in the node sums of a long table (1e-12 of the largest kick and more at M = 4096). The double instance is therefore a fixed
// sequence of IEEE additions, multiplications and divisions (libchx is built without contraction into fused multiply-adds) that
// gives the same bits wherever it is restated: no library cbrt for Newton's start and no library log1p, which differ by an ulp
// from one platform to the next (a start one ulp apart ends on a neighbouring fixed point of the iteration in hundreds of entries).

// log1p(x) for x > -1/2 from IEEE operations and the exact frexp: 1 + x = m 2^e with m in [sqrt(1/2), sqrt(2)),
// log m = 2 s (1 + z / 3 + ... + z^11 / 23), s = (m - 1) / (m + 1), z = s^2 <= 0.0295, ln 2 in two parts, and the rounding of 1 + x
// put back to first order.
__device__ __forceinline__ double csrd_log1p(double x) {
    const double u = 1.0 + x;
    int e;
    double m = frexp(u, &e);
    if (m < 0.70710678118654757) {
        m = 2.0 * m;
        e -= 1;
    }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 1.0 / 23.0;
    for (int n = 10; n >= 0; --n) p = 1.0 / (double)(2 * n + 1) + z * p;
    return (double)e * 6.93147180369123816490e-01 + (2.0 * s * p + ((double)e * 1.90821492927058770002e-10 + (x - (u - 1.0)) / u));
}
__device__ __forceinline__ Dual csrd_log1p(Dual x) { return mk(csrd_log1p(x.v), x.d / (1.0 + x.v)); }

// G(psi; xh). Below psi / xh = 1/4 the closed form cancels to O(r^3): there the series xh^2 sum_(n=3)^(32) (-1)^(n+1) (1 - 1/n) r^n,
// in Horner's form (summed from the small terms to the large ones).
template <typename S>
__device__ __forceinline__ S csrd_G(S psi, S xh) {
    if (val(xh) == 0.0) return 0.5 * psi * psi;
    const S r = psi / xh;
    if (val(r) < 0.25) {
        S acc = cst<S>(-(1.0 - 1.0 / 32.0));
        for (int n = 31; n >= 3; --n) {
            const double c = 1.0 - 1.0 / (double)n;
            acc = ((n & 1) ? c : -c) + r * acc;
        }
        return xh * xh * (r * r * r * acc);
    }
    return (0.5 * psi * psi + xh * xh * psi / (psi + xh)) - xh * xh * csrd_log1p(r);
}

// One Newton step for the root of psi^3 (psi + 4 xh) / (psi + xh) = c, over a common denominator (one division). The left side
// is convex in psi, so the steps from above the root come down to it monotonically.
template <typename S>
__device__ __forceinline__ S csrd_newton(S psi, S c, S xh) {
    const S a = psi + xh;
    const S n = psi * psi * psi * (psi + 4.0 * xh) - c * a;
    const S w = psi * (psi + 2.0 * xh);
    return psi - n * a / (3.0 * w * w);
}

// The root for c > 0: it lies in [(c / 4)^(1/3), c^(1/3)]; 12 steps from the power of two at or above the upper end (c = m 2^e
// with m < 1: 2^ceil(e / 3)), the same count in every lane.
__device__ __forceinline__ double csrd_root(double c, double xh) {
    int e;
    frexp(c, &e);
    double psi = ldexp(1.0, e >= 0 ? (e + 2) / 3 : -((-e) / 3));
    for (int i = 0; i < 12; ++i) psi = csrd_newton(psi, c, xh);
    return psi;
}

// t_i = G(psi_i), psi_i = min(psi(i h), phi) (phi itself for i > p = floor(y)), t_0 = 0. One more Newton step from the converged
// root, taken in S, carries the root's implicit derivative.
template <typename S>
__device__ __forceinline__ S csrd_t(int i, int p, S xh, S phi, S kappa) {
    if (i <= 0) return cst<S>(0.0);
    if (i > p) return csrd_G(phi, xh);
    const double psi0 = csrd_root((double)i * val(kappa), val(xh));
    S psi = csrd_newton(cst<S>(psi0), (double)i * kappa, xh);
    if (val(psi) > val(phi)) psi = phi;
    return csrd_G(psi, xh);
}

// y > 0 taken apart: p = floor(y) clamped to M in double (y may be 1e30) with the fraction f (only used below the clamp), and
// nl = min(M, p + 2): the lags j >= nl have b_j = 0.
struct CsrdLags {
    int p, nl;
};
__device__ __forceinline__ CsrdLags csrd_lags(double y, int M) {
    CsrdLags g;
    g.p = (int)fmin(floor(y), (double)M);
    g.nl = g.p + 2 < M ? g.p + 2 : M;
    return g;
}
template <typename S>
__device__ __forceinline__ S csrd_y(S xh, S phi, S kappa) {
    return phi * phi * phi * (phi + 4.0 * xh) / (kappa * (phi + xh));
}
template <typename S>
__device__ __forceinline__ S csrd_beta(S xh, S phi, S kappa) {
    return kappa / (3.0 * (phi + 2.0 * xh));
}
// b_j from t_(j-1), t_j, t_(j+1) and the boundary term's interpolation weights.
template <typename S>
__device__ __forceinline__ S csrd_b(int j, int p, S tm, S t0, S tp, S beta, S y) {
    S bj = (t0 - tm) - (tp - t0);
    if (j == p) bj = bj - beta * (1.0 - (y - (double)p));
    else if (j == p + 1) bj = bj - beta * (y - (double)p);
    return bj;
}

// LDS table bt[i] = b_(i - 128) for lags 0 <= i - 128 < nlag <= nl, zero elsewhere (i < M + 256); scratch at[nlag] for t_(j+1).
__device__ void csrd_b_table(int M, int nlag, const CsrdRow& r, const CsrdLags& g, double* bt, double* at) {
    for (int j = threadIdx.x; j < nlag; j += kWB) at[j] = csrd_t<double>(j + 1, g.p, r.xh, r.phi, r.kappa);
    __syncthreads();
    const double beta = csrd_beta(r.xh, r.phi, r.kappa), y = csrd_y(r.xh, r.phi, r.kappa);
    for (int i = threadIdx.x; i < M + 256; i += kWB) {
        const int j = i - 128;
        double bj = 0.0;
        if (j >= 0 && j < nlag) bj = csrd_b<double>(j, g.p, j > 1 ? at[j - 2] : 0.0, j > 0 ? at[j - 1] : 0.0, at[j], beta, y);
        bt[i] = bj;
    }
    __syncthreads();
}

// toeplitz_fwd_sum with the sources in fp64 (B3: the deposits the forward pass left in the state row).
__device__ __forceinline__ double toeplitz_fwd_sum_d(const double* bt, const double* __restrict__ D, int k0, int mend, int M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = k0 + lane;
    double v = 0.0;
    for (int m0 = k0 + wave * 64; m0 < mend; m0 += kWB) {
        const int m = m0 + lane;
        const double d = m < M ? D[m] : 0.0;
        const int base = 128 + m0 - k;
#pragma unroll 16
        for (int j = 0; j < 64; ++j) v += bt[base + j] * readlane_d(d, j);
    }
    return v;
}

// ---- F3 of the drift: csr_toeplitz_kernel with the row's table; workgroup 0 stores the row's scale and shape numbers in the state
// row, where F4 and the backward pass read them. The source tiles behind the last non-zero lag are skipped.
template <typename T>
__global__ __launch_bounds__(kWB) void csrd_toeplitz_kernel(int M, const T* __restrict__ energy, int64_t Be,
                                                            const T* __restrict__ length, int64_t Bl,
                                                            const T* __restrict__ bend_length, int64_t Bbl,
                                                            const T* __restrict__ bend_angle, int64_t Bba,
                                                            const T* __restrict__ distance, int64_t Bd, double mass, double absz,
                                                            const unsigned long long* __restrict__ grid,
                                                            double* __restrict__ state) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // bt[M + 256], at[M], acc[4][64]
    const int64_t b = blockIdx.y;
    const int k0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* st = state + b * csrd_state_row(M);
    double* bt = lds;
    double* acc = lds + 2 * M + 256;
    const bool live = node_live(st);
    const double SQ = st[3], h = st[2];
    const CsrdRow r = csrd_row(energy, Be, length, Bl, bend_length, Bbl, bend_angle, Bba, distance, Bd, mass, absz, live ? h : 0.0, b);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[kHdr - 1] = r.scale;
        st[csrd_par_slot(M)] = r.xh;
        st[csrd_par_slot(M) + 1] = r.phi;
        st[csrd_par_slot(M) + 2] = r.kappa;
        st[csrd_par_slot(M) + 3] = 0.0;
    }
    const bool ok = live && r.kappa > 0.0;
    const CsrdLags g = csrd_lags(ok ? csrd_y(r.xh, r.phi, r.kappa) : 1.0, M);
    if (ok) csrd_b_table(M, M - k0 < g.nl ? M - k0 : g.nl, r, g, bt, lds + M + 256);
    const unsigned long long* gq = grid + b * M;
    const int k = k0 + lane;
    const int mend = k0 + 63 + g.nl < M ? k0 + 63 + g.nl : M;       // sources m >= mend: lags >= nl for every node of the block
    acc[wave * 64 + lane] = ok ? toeplitz_fwd_sum(bt, gq, SQ, k0, mend, M) : 0.0;
    __syncthreads();
    if (wave == 0 && k < M) {
        const double s = ((acc[lane] + acc[64 + lane]) + acc[128 + lane]) + acc[192 + lane];
        st[kHdr + k] = ok ? kCoulomb / (2.0 * h * h) * s : (live && r.kappa != r.kappa ? r.kappa : 0.0);
        st[csrd_dep_slot(M) + k] = live ? from_fixed(gq[k], SQ) : 0.0;
    }
}

// ---- B3 of the drift: csr_bwd_toeplitz_kernel with the row's table, and the workgroup's partials of the shape numbers'
// cotangents: d(p) = (k_e / (2 h^2)) sum_j (db_j / dp) C_j over its 64 lags j, C_j = sum_k GV_k D_(k+j) the correlation of the node
// kicks' cotangents with the deposits (the same Toeplitz sum, the cotangents as its table); wave v < 3 takes the derivative with
// respect to xh, phi, kappa as dual numbers through the root and G, the lags p and p + 1 of the boundary term held fixed.
__global__ __launch_bounds__(kWB) void csrd_bwd_toeplitz_kernel(int M, const double* __restrict__ state,
                                                                const double* __restrict__ bhdr,
                                                                const unsigned long long* __restrict__ ggrid,
                                                                double* __restrict__ adj, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // bt[M + 256], at[M], acc[4][64]
    const int64_t b = blockIdx.y;
    const int m0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* st = state + b * csrd_state_row(M);
    double* bt = lds;
    double* acc = lds + 2 * M + 256;
    const int mmax = m0 + kNodeBlock < M ? m0 + kNodeBlock : M;     // sources m < mmax: lags up to mmax - 1
    const bool live = node_live(st);
    CsrdRow r;
    r.scale = st[kHdr - 1];
    r.xh = st[csrd_par_slot(M)];
    r.phi = st[csrd_par_slot(M) + 1];
    r.kappa = st[csrd_par_slot(M) + 2];
    const bool ok = live && r.kappa > 0.0;
    const double nan_row = live && r.kappa != r.kappa ? r.kappa : 0.0;
    const CsrdLags g = csrd_lags(ok ? csrd_y(r.xh, r.phi, r.kappa) : 1.0, M);
    if (ok) csrd_b_table(M, mmax < g.nl ? mmax : g.nl, r, g, bt, lds + M + 256);
    const unsigned long long* gg = ggrid + b * M;
    const double SV = bhdr[b * kHdr + 1], h = st[2];
    const double factor = kCoulomb / (2.0 * h * h);
    const int m = m0 + lane;
    acc[wave * 64 + lane] = ok ? toeplitz_bwd_sum(bt, gg, SV, m0, mmax, m0 - g.nl + 1, M) : 0.0;
    __syncthreads();
    if (wave == 0 && m < M) {
        const double s = ((acc[lane] + acc[64 + lane]) + acc[128 + lane]) + acc[192 + lane];
        adj[b * M + m] = ok ? factor * s : nan_row;
    }
    // the lags j = m0 + lane of this workgroup; those from nl on have b_j = 0 for every value of the shape numbers
    const bool lags = ok && m0 < g.nl;
    __syncthreads();
    if (lags) {
        for (int i = threadIdx.x; i < M + 256; i += kWB) {
            const int k = i - 128;
            bt[i] = (k >= 0 && k < M) ? from_fixed(gg[k], SV) : 0.0;
        }
    }
    __syncthreads();
    acc[wave * 64 + lane] = lags ? toeplitz_fwd_sum_d(bt, st + csrd_dep_slot(M), m0, M, M) : 0.0;
    __syncthreads();
    if (wave < 3) {
        double dp = wave == 0 ? nan_row : 0.0;
        if (lags && m < g.nl) {
            const double cj = ((acc[lane] + acc[64 + lane]) + acc[128 + lane]) + acc[192 + lane];
            const Dual xh = mk(r.xh, wave == 0 ? 1.0 : 0.0), phi = mk(r.phi, wave == 1 ? 1.0 : 0.0),
                       kappa = mk(r.kappa, wave == 2 ? 1.0 : 0.0);
            const Dual bj = csrd_b<Dual>(m, g.p, csrd_t<Dual>(m - 1, g.p, xh, phi, kappa), csrd_t<Dual>(m, g.p, xh, phi, kappa),
                                         csrd_t<Dual>(m + 1, g.p, xh, phi, kappa), csrd_beta(xh, phi, kappa), csrd_y(xh, phi, kappa));
            dp = factor * bj.d * cj;
        }
        dp = chx_wave_sum(dp);
        if (lane == 0) part[(b * kCsrMaxBlocks + blockIdx.x) * kCsrdPar + wave] = dp;
    }
}

// ---- B4 of the drift: one pass over the particles; the first thread of a row adds the workgroups' partials in order
template <typename T>
__global__ __launch_bounds__(kWB) void csrd_bwd_particles_kernel(const T* __restrict__ x, const T* __restrict__ q,
                                                                 const T* __restrict__ w, int64_t Bx, int64_t Bq, int64_t Bw,
                                                                 int64_t N, int M, const double* __restrict__ state,
                                                                 const double* __restrict__ adj, const double* __restrict__ part,
                                                                 const T* __restrict__ gout, T* __restrict__ dX, T* __restrict__ dC,
                                                                 double* __restrict__ d_xh, double* __restrict__ d_phi,
                                                                 double* __restrict__ d_kappa) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int nb = (M + kNodeBlock - 1) / kNodeBlock;
        double s[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < nb; ++i)
            for (int c = 0; c < 3; ++c) s[c] += part[((int64_t)blockIdx.y * kCsrMaxBlocks + i) * kCsrdPar + c];
        d_xh[blockIdx.y] = s[0];
        d_phi[blockIdx.y] = s[1];
        d_kappa[blockIdx.y] = s[2];
    }
    node_bwd_particle(x, q, w, Bx, Bq, Bw, N, M, state, csrd_state_row(M), adj, gout, dX, dC);
}

template <typename T>
int csrd_kick_t(const T* x, const T* q, const T* w, const T* energy, const T* length, const T* bend_length, const T* bend_angle,
                const T* distance, double mass, double absz, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl,
                int64_t Bbl, int64_t Bba, int64_t Bd, int64_t N, int M, T* out, double* state, const Grid1dWs& ws, hipStream_t s) {
    if (!lds_ok(csrd_toeplitz_kernel<T>, toeplitz_lds(M))) return CHX_ERR_LAUNCH;
    int st = launch_deposit(x, q, w, B, Bx, Bq, Bw, N, M, 0, 1, 1, csrd_state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(csrd_toeplitz_kernel<T>, grid_nodes(M, B), dim3(kWB), toeplitz_lds(M), s, M, energy, Be, length, Bl, bend_length,
                       Bbl, bend_angle, Bba, distance, Bd, mass, absz, ws.grid, state);
    CHX_CHECK_LAUNCH();
    return launch_node_kick(x, B, Bx, N, M, csrd_state_row(M), state, out, s);
}

template <typename T>
int csrd_kick_bwd_t(const T* x, const T* q, const T* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int M,
                    const double* state, const T* gout, T* dX, T* dC, double* d_scale, double* d_xh, double* d_phi, double* d_kappa,
                    const Grid1dWs& ws, hipStream_t s) {
    if (!lds_ok(csrd_bwd_toeplitz_kernel, toeplitz_lds(M))) return CHX_ERR_LAUNCH;
    int st = launch_node_bwd_deposit(x, B, Bx, N, M, csrd_state_row(M), state, gout, d_scale, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(csrd_bwd_toeplitz_kernel, grid_nodes(M, B), dim3(kWB), toeplitz_lds(M), s, M, state, ws.bhdr, ws.ggrid, ws.adj,
                       ws.extra);
    CHX_CHECK_LAUNCH();
    st = launch_adj_filter(B, M, 1, csrd_state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(csrd_bwd_particles_kernel<T>, grid_particles(N, B), dim3(kWB), 0, s, x, q, w, Bx, Bq, Bw, N, M, state, ws.adj_last,
                       ws.extra, gout, dX, dC, d_xh, d_phi, d_kappa);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace

// Every entry point has a twin that takes cutoff[Bcut] in front of the workspace (the low-pass stage of chx_grid1d_dev.h, launched by
// launch_deposit and launch_adj_filter); the call without the suffix is the twin with a null cutoff.
extern "C" size_t chx_csr_workspace_bytes(int64_t B, int64_t N, int32_t M) { return csr_ws(nullptr, B, N, M).bytes; }
extern "C" size_t chx_csr_workspace_bytes_cut(int64_t B, int64_t N, int32_t M) {
    return cutoff_ws_bytes(csr_ws(nullptr, B, N, M), B, M, 1);
}

extern "C" int chx_csr_kick_cut(const void* x, const void* q, const void* w, const void* energy, const void* length,
                                const void* angle, double mass_eV, double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                                int64_t Be, int64_t Bl, int64_t Ba, int64_t N, int32_t M, int dtype, void* out, double* state,
                                const double* cutoff, int64_t Bcut, void* workspace, size_t workspace_bytes, void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!energy || !length || !angle || !(mass_eV > 0.0) || !chx_bcast_ok(Be, B) || !chx_bcast_ok(Bl, B) || !chx_bcast_ok(Ba, B) ||
        !out)
        return CHX_ERR_INVALID_ARG;
    if (!chx_aligned16(out)) return CHX_ERR_MISALIGNED;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(csr_ws(workspace, B, N, M), workspace, B, M, 1, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return csr_kick_t<T>((const T*)x, (const T*)q, (const T*)w, (const T*)energy, (const T*)length, (const T*)angle, mass_eV,
                             abs_charge, B, Bx, Bq, Bw, Be, Bl, Ba, N, M, (T*)out, state, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_csr_kick(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* angle,
                            double mass_eV, double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be,
                            int64_t Bl, int64_t Ba, int64_t N, int32_t M, int dtype, void* out, double* state, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return chx_csr_kick_cut(x, q, w, energy, length, angle, mass_eV, abs_charge, B, Bx, Bq, Bw, Be, Bl, Ba, N, M, dtype, out, state,
                            nullptr, 1, workspace, workspace_bytes, stream);
}

extern "C" int chx_csr_kick_bwd_cut(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                                    int64_t N, int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC,
                                    double* d_scale, const double* cutoff, int64_t Bcut, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!d_out || !dX || !d_scale) return CHX_ERR_INVALID_ARG;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(csr_ws(workspace, B, N, M), workspace, B, M, 1, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return csr_kick_bwd_t<T>((const T*)x, (const T*)q, (const T*)w, B, Bx, Bq, Bw, N, M, state, (const T*)d_out, (T*)dX, (T*)dC,
                                 d_scale, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_csr_kick_bwd(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                                int64_t N, int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC,
                                double* d_scale, void* workspace, size_t workspace_bytes, void* stream) {
    return chx_csr_kick_bwd_cut(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state, d_out, dX, dC, d_scale, nullptr, 1, workspace,
                                workspace_bytes, stream);
}

extern "C" size_t chx_csr_transient_workspace_bytes(int64_t B, int64_t N, int32_t M) { return csrt_ws(nullptr, B, N, M).bytes; }
extern "C" size_t chx_csr_transient_workspace_bytes_cut(int64_t B, int64_t N, int32_t M) {
    return cutoff_ws_bytes(csrt_ws(nullptr, B, N, M), B, M, 1);
}

extern "C" int chx_csr_transient_kick_cut(const void* x, const void* q, const void* w, const void* energy, const void* length,
                                          const void* angle, const void* distance, double mass_eV, double abs_charge, int64_t B,
                                          int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl, int64_t Ba, int64_t Bd,
                                          int64_t N, int32_t M, int dtype, void* out, double* state, const double* cutoff,
                                          int64_t Bcut, void* workspace, size_t workspace_bytes, void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!energy || !length || !angle || !distance || !(mass_eV > 0.0) || !chx_bcast_ok(Be, B) || !chx_bcast_ok(Bl, B) ||
        !chx_bcast_ok(Ba, B) || !chx_bcast_ok(Bd, B) || !out)
        return CHX_ERR_INVALID_ARG;
    if (!chx_aligned16(out)) return CHX_ERR_MISALIGNED;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(csrt_ws(workspace, B, N, M), workspace, B, M, 1, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return csrt_kick_t<T>((const T*)x, (const T*)q, (const T*)w, (const T*)energy, (const T*)length, (const T*)angle,
                              (const T*)distance, mass_eV, abs_charge, B, Bx, Bq, Bw, Be, Bl, Ba, Bd, N, M, (T*)out, state, ws,
                              (hipStream_t)stream);
    });
}

extern "C" int chx_csr_transient_kick(const void* x, const void* q, const void* w, const void* energy, const void* length,
                                      const void* angle, const void* distance, double mass_eV, double abs_charge, int64_t B,
                                      int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl, int64_t Ba, int64_t Bd, int64_t N,
                                      int32_t M, int dtype, void* out, double* state, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    return chx_csr_transient_kick_cut(x, q, w, energy, length, angle, distance, mass_eV, abs_charge, B, Bx, Bq, Bw, Be, Bl, Ba, Bd,
                                      N, M, dtype, out, state, nullptr, 1, workspace, workspace_bytes, stream);
}

extern "C" int chx_csr_transient_kick_bwd_cut(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq,
                                              int64_t Bw, int64_t N, int32_t M, int dtype, const double* state, const void* d_out,
                                              void* dX, void* dC, double* d_scale, double* d_x, const double* cutoff, int64_t Bcut,
                                              void* workspace, size_t workspace_bytes, void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!d_out || !dX || !d_scale || !d_x) return CHX_ERR_INVALID_ARG;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(csrt_ws(workspace, B, N, M), workspace, B, M, 1, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return csrt_kick_bwd_t<T>((const T*)x, (const T*)q, (const T*)w, B, Bx, Bq, Bw, N, M, state, (const T*)d_out, (T*)dX, (T*)dC,
                                  d_scale, d_x, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_csr_transient_kick_bwd(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq,
                                          int64_t Bw, int64_t N, int32_t M, int dtype, const double* state, const void* d_out,
                                          void* dX, void* dC, double* d_scale, double* d_x, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    return chx_csr_transient_kick_bwd_cut(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state, d_out, dX, dC, d_scale, d_x, nullptr, 1,
                                          workspace, workspace_bytes, stream);
}

extern "C" size_t chx_csr_drift_workspace_bytes(int64_t B, int64_t N, int32_t M) { return csrd_ws(nullptr, B, N, M).bytes; }
extern "C" size_t chx_csr_drift_workspace_bytes_cut(int64_t B, int64_t N, int32_t M) {
    return cutoff_ws_bytes(csrd_ws(nullptr, B, N, M), B, M, 1);
}

extern "C" int chx_csr_drift_kick_cut(const void* x, const void* q, const void* w, const void* energy, const void* length,
                                      const void* bend_length, const void* bend_angle, const void* distance, double mass_eV,
                                      double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl,
                                      int64_t Bbl, int64_t Bba, int64_t Bd, int64_t N, int32_t M, int dtype, void* out,
                                      double* state, const double* cutoff, int64_t Bcut, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!energy || !length || !bend_length || !bend_angle || !distance || !(mass_eV > 0.0) || !chx_bcast_ok(Be, B) ||
        !chx_bcast_ok(Bl, B) || !chx_bcast_ok(Bbl, B) || !chx_bcast_ok(Bba, B) || !chx_bcast_ok(Bd, B) || !out)
        return CHX_ERR_INVALID_ARG;
    if (!chx_aligned16(out)) return CHX_ERR_MISALIGNED;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(csrd_ws(workspace, B, N, M), workspace, B, M, 1, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return csrd_kick_t<T>((const T*)x, (const T*)q, (const T*)w, (const T*)energy, (const T*)length, (const T*)bend_length,
                              (const T*)bend_angle, (const T*)distance, mass_eV, abs_charge, B, Bx, Bq, Bw, Be, Bl, Bbl, Bba, Bd, N, M,
                              (T*)out, state, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_csr_drift_kick(const void* x, const void* q, const void* w, const void* energy, const void* length,
                                  const void* bend_length, const void* bend_angle, const void* distance, double mass_eV,
                                  double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl,
                                  int64_t Bbl, int64_t Bba, int64_t Bd, int64_t N, int32_t M, int dtype, void* out, double* state,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    return chx_csr_drift_kick_cut(x, q, w, energy, length, bend_length, bend_angle, distance, mass_eV, abs_charge, B, Bx, Bq, Bw,
                                  Be, Bl, Bbl, Bba, Bd, N, M, dtype, out, state, nullptr, 1, workspace, workspace_bytes, stream);
}

extern "C" int chx_csr_drift_kick_bwd_cut(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq,
                                          int64_t Bw, int64_t N, int32_t M, int dtype, const double* state, const void* d_out,
                                          void* dX, void* dC, double* d_scale, double* d_xh, double* d_phi, double* d_kappa,
                                          const double* cutoff, int64_t Bcut, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!d_out || !dX || !d_scale || !d_xh || !d_phi || !d_kappa) return CHX_ERR_INVALID_ARG;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(csrd_ws(workspace, B, N, M), workspace, B, M, 1, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return csrd_kick_bwd_t<T>((const T*)x, (const T*)q, (const T*)w, B, Bx, Bq, Bw, N, M, state, (const T*)d_out, (T*)dX, (T*)dC,
                                  d_scale, d_xh, d_phi, d_kappa, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_csr_drift_kick_bwd(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                                      int64_t N, int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC,
                                      double* d_scale, double* d_xh, double* d_phi, double* d_kappa, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return chx_csr_drift_kick_bwd_cut(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state, d_out, dX, dC, d_scale, d_xh, d_phi, d_kappa,
                                      nullptr, 1, workspace, workspace_bytes, stream);
}
