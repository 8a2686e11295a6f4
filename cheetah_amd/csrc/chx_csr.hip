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

// ---- F3 ----------------------------------------------------------------------------------------------------------------------
// One workgroup per (row, 64 nodes k0 ... k0 + 63); workgroup 0 stores the row's scale in the last header slot, where F4 and the
// backward pass read it; wave v takes the source tiles m0 = k0 + 64 (v + 4 i) < M; a tile's 64 deposits
// are loaded one per lane and broadcast with readlane. Lag m - k of source m0 + j: bt index 128 + m0 + j - k in [65, M + 190].
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
    double v = 0.0;
    if (live) {
        for (int m0 = k0 + wave * 64; m0 < M; m0 += kWB) {
            const int m = m0 + lane;
            const double d = m < M ? from_fixed(gq[m], SQ) : 0.0;
            const int base = 128 + m0 - k;
#pragma unroll 16
            for (int j = 0; j < 64; ++j) v += bt[base + j] * readlane_d(d, j);
        }
    }
    acc[wave * 64 + lane] = v;
    __syncthreads();
    if (wave == 0 && k < M) {
        const double s = ((acc[lane] + acc[64 + lane]) + acc[128 + lane]) + acc[192 + lane];
        // 3^(2/3) k_e h^(-4/3): the node energy change per unit |Z| L^(1/3) |theta|^(2/3)
        st[kHdr + k] = live ? cbrt(9.0) * kCoulomb / (h * cbrt(h)) * s : 0.0;
    }
}

// ---- B3: adjoint of F3, GD_m = 3^(2/3) k_e h^(-4/3) sum_{k <= m} b_(m-k) GV_k ------------------------------------------------------
// One workgroup per (row, 64 sources m0 ... m0 + 63); wave v takes the target tiles k0 = 64 (v + 4 i) <= m0 + 63. Lag m - k of
// target k0 + j: bt index 128 + m - k0 - j in [2, M + 190].
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
    double v = 0.0;
    if (live) {
        for (int k0 = wave * 64; k0 < mmax; k0 += kWB) {
            const int k = k0 + lane;
            const double a = k < M ? from_fixed(gg[k], SV) : 0.0;
            const int base = 128 + m - k0;
#pragma unroll 16
            for (int j = 0; j < 64; ++j) v += bt[base - j] * readlane_d(a, j);
        }
    }
    acc[wave * 64 + lane] = v;
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
    hipLaunchKernelGGL(node_bwd_particles_kernel<T>, grid_particles(N, B), dim3(kWB), 0, s, x, q, w, Bx, Bq, Bw, N, M, state,
                       csr_state_row(M), ws.adj, gout, dX, dC);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace

extern "C" size_t chx_csr_workspace_bytes(int64_t B, int64_t N, int32_t M) { return csr_ws(nullptr, B, N, M).bytes; }

extern "C" int chx_csr_kick(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* angle,
                            double mass_eV, double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl,
                            int64_t Ba, int64_t N, int32_t M, int dtype, void* out, double* state, void* workspace,
                            size_t workspace_bytes, void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!energy || !length || !angle || !(mass_eV > 0.0) || !chx_bcast_ok(Be, B) || !chx_bcast_ok(Bl, B) || !chx_bcast_ok(Ba, B) ||
        !out)
        return CHX_ERR_INVALID_ARG;
    if (!chx_aligned16(out)) return CHX_ERR_MISALIGNED;
    const Grid1dWs ws = csr_ws(workspace, B, N, M);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return csr_kick_t<T>((const T*)x, (const T*)q, (const T*)w, (const T*)energy, (const T*)length, (const T*)angle, mass_eV,
                             abs_charge, B, Bx, Bq, Bw, Be, Bl, Ba, N, M, (T*)out, state, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_csr_kick_bwd(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N,
                                int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale,
                                void* workspace, size_t workspace_bytes, void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!d_out || !dX || !d_scale) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = csr_ws(workspace, B, N, M);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return csr_kick_bwd_t<T>((const T*)x, (const T*)q, (const T*)w, B, Bx, Bq, Bw, N, M, state, (const T*)d_out, (T*)dX, (T*)dC,
                                 d_scale, ws, (hipStream_t)stream);
    });
}
