// chx_lsc.hip — longitudinal space-charge kick (LSCKick element): the on-axis field of a uniformly charged disc of radius a moving
// with Lorentz factor gamma, E_z(tau) = (2 k_e / a^2) int lambda(tau') g(tau' - tau) dtau', g(u) = sgn(u) - u / sqrt(u^2 + (a/gamma)^2),
// with the line density piecewise linear between M nodes in tau and g integrated exactly against every hat function. With
// rho = a / (gamma h): P(v) = v / (|v| + sqrt(v^2 + rho^2)) + asinh(v / rho) (the second antiderivative of g over -rho^2 / 2, in its
// cancellation-free form), c^_0 = 0, c^_(-j) = -c^_j, c^_j = -(P(j+1) - 2 P(j) + P(j-1)) / 2. Per batch row, every grid quantity in fp64:
//   F1. wake_range_kernel     (chx_grid1d_dev.h) partials of the surviving particles' tau range and charge; zeroes the grid
//   F2. wake_deposit_kernel   (chx_grid1d_dev.h) the row header and the fixed-point node deposit D_k (one channel)
//   F3. lsc_toeplitz_kernel   one workgroup per (row, 64 nodes): P and c^_j for the lags 0 ... M - 1 formed into LDS, the two-sided sum
//                             V_k = sum_j c^_j D_(k+j) over the source tiles on both sides of the block with the lag's sign, its four
//                             waves splitting the tiles, merged in order; workgroup 0 stores the row's scale S and rho
//   F4. node_kick_kernel      (chx_grid1d_dev.h) one thread per particle: gather of the node sums times S, delta rounded once
// Backward (the CSR kick's pattern): B1 node_bwd_range_kernel, bounds of the gather's cotangents and the per-row partials of d(S);
// B2 node_bwd_deposit_kernel, their fixed-point deposit; B3 lsc_bwd_toeplitz_kernel, the adjoint correlation (two-sided, the
// opposite sign) with c^ for the deposits' cotangents and with d c^ / d rho against the forward's deposits for d(rho); B4
// lsc_bwd_particles_kernel, one pass over the particles (node_bwd_particle of chx_grid1d_dev.h) that also sums d(rho). Only F3, B3
// and that sum are this file's: the particle passes, the argument check, the workspace and the launchers are chx_grid1d_dev.h and
// chx_grid1d_host.h, shared with chx_wake.hip and chx_csr.hip.
#include "chx_grid1d_host.h"

namespace {

constexpr int kMaxBlocks = CHX_WAKE_MAX_BINS / kNodeBlock;

__host__ __device__ inline int64_t lsc_state_row(int M) { return CHX_LSC_STATE_DOUBLES(M); }
// state row: [0, kHdr) the header with S in its last slot | [kHdr, kHdr + M) node sums V_k | rho | a free slot | M deposits D_k
__host__ __device__ inline int lsc_rho_slot(int M) { return kHdr + M; }
__host__ __device__ inline int lsc_dep_slot(int M) { return kHdr + M + 2; }

// The workspace's own block: rpart[B][kMaxBlocks], the partials of d(rho), one per workgroup of B3.
Grid1dWs lsc_ws(void* base, int64_t B, int64_t N, int M) { return grid1d_ws(base, B, N, M, 1, (size_t)(B * kMaxBlocks) * 8); }

// The row's scale S = |Z| 2 k_e L / (gamma^2 h^2 p0c) and rho = a / (gamma h) in fp64; p0c = beta gamma m c^2 as `Beam.p0c`. A radius
// that is not > 0 or not finite gives NaN for both (a line charge has no finite on-axis field).
template <typename T>
__device__ __forceinline__ void lsc_scales(const T* energy, int64_t Be, const T* length, int64_t Bl, const T* radius, int64_t Ba,
                                           double mass, double absz, double h, int64_t b, double& S, double& rho) {
    const double e = (double)energy[Be == 1 ? 0 : b], L = (double)length[Bl == 1 ? 0 : b], a = (double)radius[Ba == 1 ? 0 : b];
    double gamma;
    const double p0c = ref_p0c(e, mass, gamma);
    if (a > 0.0 && isfinite(a)) {
        S = absz * 2.0 * kCoulomb * L / (gamma * gamma * h * h * p0c);
        rho = a / (gamma * h);
    } else {
        S = rho = __longlong_as_double(0x7ff8000000000000LL);
    }
}

// LDS tables ct[j] = c^_j for 0 < j < M, zero elsewhere (j < M + 64), and dt[j] = d c^_j / d rho likewise when dt is given; scratch
// pt[M + 1] for P(0 ... M). d P / d rho = -v rho / (s (v + s)^2) - v / (rho s), s = sqrt(v^2 + rho^2).
__device__ void lsc_tables(int M, double rho, double* ct, double* dt, double* pt) {
    for (int i = threadIdx.x; i <= M; i += kWB) {
        const double v = (double)i, s = sqrt(v * v + rho * rho);
        pt[i] = v / (v + s) + asinh(v / rho);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < M + 64; j += kWB) ct[j] = (j == 0 || j >= M) ? 0.0 : -0.5 * (pt[j + 1] - 2.0 * pt[j] + pt[j - 1]);
    __syncthreads();
    if (!dt) return;
    for (int i = threadIdx.x; i <= M; i += kWB) {
        const double v = (double)i, s = sqrt(v * v + rho * rho);
        pt[i] = -v * rho / (s * ((v + s) * (v + s))) - v / (rho * s);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < M + 64; j += kWB) dt[j] = (j == 0 || j >= M) ? 0.0 : -0.5 * (pt[j + 1] - 2.0 * pt[j] + pt[j - 1]);
    __syncthreads();
}

inline size_t lsc_lds(int M, int tables) { return ((size_t)tables * (M + 64) + (M + 2) + (size_t)tables * 4 * 64) * sizeof(double); }

__device__ __forceinline__ bool lsc_rho_ok(double rho) { return rho > 0.0 && isfinite(rho); }

// ---- F3 ----------------------------------------------------------------------------------------------------------------------
// One workgroup per (row, 64 nodes k0 ... k0 + 63); wave v takes the source tiles m0 = 64 (v + 4 i) < M on both sides of the block; a
// tile's 64 deposits are loaded one per lane and broadcast with readlane. Lag m - k of source m0 + j: a tile behind the block
// (m0 > k0) reads ct[m0 - k + j] in [1, M + 62], a tile ahead of it (m0 < k0) reads -ct[k - m0 - j] in [1, M + 62], and the block's
// own tile takes the sign per term. Workgroup 0 stores S and rho in the state row, where F4 and the backward pass read them.
template <typename T>
__global__ __launch_bounds__(kWB) void lsc_toeplitz_kernel(int M, const T* __restrict__ energy, int64_t Be,
                                                           const T* __restrict__ length, int64_t Bl, const T* __restrict__ radius,
                                                           int64_t Ba, double mass, double absz,
                                                           const unsigned long long* __restrict__ grid, double* __restrict__ state) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // ct[M + 64], pt[M + 2], acc[4][64]
    const int64_t b = blockIdx.y;
    const int k0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* st = state + b * lsc_state_row(M);
    double* ct = lds;
    double* pt = lds + M + 64;
    double* acc = pt + M + 2;
    const bool live = node_live(st);
    const double SQ = st[3], h = st[2];
    double S = 0.0, rho = 0.0;
    if (live) lsc_scales(energy, Be, length, Bl, radius, Ba, mass, absz, h, b, S, rho);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[kHdr - 1] = S;
        st[lsc_rho_slot(M)] = rho;
        st[lsc_rho_slot(M) + 1] = 0.0;
    }
    const bool ok = live && lsc_rho_ok(rho);
    if (ok) lsc_tables(M, rho, ct, nullptr, pt);
    const unsigned long long* gq = grid + b * M;
    const int k = k0 + lane;
    double v = 0.0;
    if (ok) {
        for (int m0 = wave * 64; m0 < M; m0 += kWB) {
            const int m = m0 + lane;
            const double d = m < M ? from_fixed(gq[m], SQ) : 0.0;
            if (m0 > k0) {
                const int base = m0 - k;
#pragma unroll 16
                for (int j = 0; j < 64; ++j) v += ct[base + j] * readlane_d(d, j);
            } else if (m0 < k0) {
                const int base = k - m0;
#pragma unroll 16
                for (int j = 0; j < 64; ++j) v -= ct[base - j] * readlane_d(d, j);
            } else {
#pragma unroll 16
                for (int j = 0; j < 64; ++j) {
                    const int lag = j - lane;
                    v += (lag >= 0 ? ct[lag] : -ct[-lag]) * readlane_d(d, j);
                }
            }
        }
    }
    acc[wave * 64 + lane] = v;
    __syncthreads();
    if (wave == 0 && k < M) {
        const double s = ((acc[lane] + acc[64 + lane]) + acc[128 + lane]) + acc[192 + lane];
        st[kHdr + k] = ok ? s : (live ? rho : 0.0);                         // a live row without a radius: NaN
        st[lsc_dep_slot(M) + k] = live ? from_fixed(gq[k], SQ) : 0.0;
    }
}

// ---- B3: adjoint of F3, GD_m = sum_k sgn(m - k) c^_|m-k| GV_k, and the workgroup's partial of d(rho) = sum_m D_m sum_k sgn(m - k)
// (d c^ / d rho)_|m-k| GV_k. One workgroup per (row, 64 sources m0 ... m0 + 63); wave v takes the target tiles k0 = 64 (v + 4 i) < M.
__global__ __launch_bounds__(kWB) void lsc_bwd_toeplitz_kernel(int M, const double* __restrict__ state, const double* __restrict__ bhdr,
                                                               const unsigned long long* __restrict__ ggrid, double* __restrict__ adj,
                                                               double* __restrict__ rpart) {
    extern __shared__ __attribute__((aligned(16))) double lds[];            // ct[M + 64], dt[M + 64], pt[M + 2], acc[2][4][64]
    const int64_t b = blockIdx.y;
    const int m0 = blockIdx.x * kNodeBlock;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* st = state + b * lsc_state_row(M);
    double* ct = lds;
    double* dt = lds + M + 64;
    double* pt = dt + M + 64;
    double* acc = pt + M + 2;
    const bool live = node_live(st);
    const double rho = st[lsc_rho_slot(M)];
    const bool ok = live && lsc_rho_ok(rho);
    if (ok) lsc_tables(M, rho, ct, dt, pt);
    const unsigned long long* gg = ggrid + b * M;
    const double SV = bhdr[b * kHdr + 1];
    const int m = m0 + lane;
    double v = 0.0, r = 0.0;
    if (ok) {
        for (int k0 = wave * 64; k0 < M; k0 += kWB) {
            const int k = k0 + lane;
            const double a = k < M ? from_fixed(gg[k], SV) : 0.0;
            if (k0 < m0) {
                const int base = m - k0;
#pragma unroll 16
                for (int j = 0; j < 64; ++j) {
                    const double aj = readlane_d(a, j);
                    v += ct[base - j] * aj;
                    r += dt[base - j] * aj;
                }
            } else if (k0 > m0) {
                const int base = k0 - m;
#pragma unroll 16
                for (int j = 0; j < 64; ++j) {
                    const double aj = readlane_d(a, j);
                    v -= ct[base + j] * aj;
                    r -= dt[base + j] * aj;
                }
            } else {
#pragma unroll 16
                for (int j = 0; j < 64; ++j) {
                    const int lag = lane - j;
                    const double aj = readlane_d(a, j);
                    v += (lag >= 0 ? ct[lag] : -ct[-lag]) * aj;
                    r += (lag >= 0 ? dt[lag] : -dt[-lag]) * aj;
                }
            }
        }
    }
    acc[wave * 64 + lane] = v;
    acc[256 + wave * 64 + lane] = r;
    __syncthreads();
    if (wave == 0) {
        double rp = 0.0;
        if (m < M) {
            const double s = ((acc[lane] + acc[64 + lane]) + acc[128 + lane]) + acc[192 + lane];
            const double sr = ((acc[256 + lane] + acc[320 + lane]) + acc[384 + lane]) + acc[448 + lane];
            adj[b * M + m] = ok ? s : (live ? rho : 0.0);
            rp = ok ? st[lsc_dep_slot(M) + m] * sr : (live ? rho : 0.0);
        }
        rp = chx_wave_sum(rp);
        if (lane == 0) rpart[b * kMaxBlocks + blockIdx.x] = rp;
    }
}

// ---- B4: one pass over the particles; the first thread of a row adds the workgroups' partials of d(rho) in order ------------------
template <typename T>
__global__ __launch_bounds__(kWB) void lsc_bwd_particles_kernel(const T* __restrict__ x, const T* __restrict__ q,
                                                                const T* __restrict__ w, int64_t Bx, int64_t Bq, int64_t Bw,
                                                                int64_t N, int M, const double* __restrict__ state,
                                                                const double* __restrict__ adj, const double* __restrict__ rpart,
                                                                const T* __restrict__ gout, T* __restrict__ dX, T* __restrict__ dC,
                                                                double* __restrict__ d_rho) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int nb = (M + kNodeBlock - 1) / kNodeBlock;
        double s = 0.0;
        for (int i = 0; i < nb; ++i) s += rpart[(int64_t)blockIdx.y * kMaxBlocks + i];
        d_rho[blockIdx.y] = s;
    }
    node_bwd_particle(x, q, w, Bx, Bq, Bw, N, M, state, lsc_state_row(M), adj, gout, dX, dC);
}

template <typename T>
int lsc_kick_t(const T* x, const T* q, const T* w, const T* energy, const T* length, const T* radius, double mass, double absz,
               int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl, int64_t Ba, int64_t N, int M, T* out,
               double* state, const Grid1dWs& ws, hipStream_t s) {
    if (!lds_ok(lsc_toeplitz_kernel<T>, lsc_lds(M, 1))) return CHX_ERR_LAUNCH;
    int st = launch_deposit(x, q, w, B, Bx, Bq, Bw, N, M, 0, 1, 1, lsc_state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(lsc_toeplitz_kernel<T>, grid_nodes(M, B), dim3(kWB), lsc_lds(M, 1), s, M, energy, Be, length, Bl, radius, Ba,
                       mass, absz, ws.grid, state);
    CHX_CHECK_LAUNCH();
    return launch_node_kick(x, B, Bx, N, M, lsc_state_row(M), state, out, s);
}

template <typename T>
int lsc_kick_bwd_t(const T* x, const T* q, const T* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int M,
                   const double* state, const T* gout, T* dX, T* dC, double* d_scale, double* d_rho, const Grid1dWs& ws,
                   hipStream_t s) {
    if (!lds_ok(lsc_bwd_toeplitz_kernel, lsc_lds(M, 2))) return CHX_ERR_LAUNCH;
    int st = launch_node_bwd_deposit(x, B, Bx, N, M, lsc_state_row(M), state, gout, d_scale, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(lsc_bwd_toeplitz_kernel, grid_nodes(M, B), dim3(kWB), lsc_lds(M, 2), s, M, state, ws.bhdr, ws.ggrid, ws.adj,
                       ws.extra);
    CHX_CHECK_LAUNCH();
    st = launch_adj_filter(B, M, 1, lsc_state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(lsc_bwd_particles_kernel<T>, grid_particles(N, B), dim3(kWB), 0, s, x, q, w, Bx, Bq, Bw, N, M, state, ws.adj_last,
                       ws.extra, gout, dX, dC, d_rho);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace

// Every entry point has a twin that takes cutoff[Bcut] in front of the workspace (the low-pass stage of chx_grid1d_dev.h, launched by
// launch_deposit and launch_adj_filter); the call without the suffix is the twin with a null cutoff.
extern "C" size_t chx_lsc_workspace_bytes(int64_t B, int64_t N, int32_t M) { return lsc_ws(nullptr, B, N, M).bytes; }
extern "C" size_t chx_lsc_workspace_bytes_cut(int64_t B, int64_t N, int32_t M) {
    return cutoff_ws_bytes(lsc_ws(nullptr, B, N, M), B, M, 1);
}

extern "C" int chx_lsc_kick_cut(const void* x, const void* q, const void* w, const void* energy, const void* length,
                                const void* radius, double mass_eV, double abs_charge, int64_t B, int64_t Bx, int64_t Bq,
                                int64_t Bw, int64_t Be, int64_t Bl, int64_t Ba, int64_t N, int32_t M, int dtype, void* out,
                                double* state, const double* cutoff, int64_t Bcut, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!energy || !length || !radius || !(mass_eV > 0.0) || !chx_bcast_ok(Be, B) || !chx_bcast_ok(Bl, B) || !chx_bcast_ok(Ba, B) ||
        !out)
        return CHX_ERR_INVALID_ARG;
    if (!chx_aligned16(out)) return CHX_ERR_MISALIGNED;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(lsc_ws(workspace, B, N, M), workspace, B, M, 1, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return lsc_kick_t<T>((const T*)x, (const T*)q, (const T*)w, (const T*)energy, (const T*)length, (const T*)radius, mass_eV,
                             abs_charge, B, Bx, Bq, Bw, Be, Bl, Ba, N, M, (T*)out, state, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_lsc_kick(const void* x, const void* q, const void* w, const void* energy, const void* length, const void* radius,
                            double mass_eV, double abs_charge, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be,
                            int64_t Bl, int64_t Ba, int64_t N, int32_t M, int dtype, void* out, double* state, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return chx_lsc_kick_cut(x, q, w, energy, length, radius, mass_eV, abs_charge, B, Bx, Bq, Bw, Be, Bl, Ba, N, M, dtype, out,
                            state, nullptr, 1, workspace, workspace_bytes, stream);
}

extern "C" int chx_lsc_kick_bwd_cut(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                                    int64_t N, int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC,
                                    double* d_scale, double* d_rho, const double* cutoff, int64_t Bcut, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!d_out || !dX || !d_scale || !d_rho) return CHX_ERR_INVALID_ARG;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(lsc_ws(workspace, B, N, M), workspace, B, M, 1, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return lsc_kick_bwd_t<T>((const T*)x, (const T*)q, (const T*)w, B, Bx, Bq, Bw, N, M, state, (const T*)d_out, (T*)dX, (T*)dC,
                                 d_scale, d_rho, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_lsc_kick_bwd(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw,
                                int64_t N, int32_t M, int dtype, const double* state, const void* d_out, void* dX, void* dC,
                                double* d_scale, double* d_rho, void* workspace, size_t workspace_bytes, void* stream) {
    return chx_lsc_kick_bwd_cut(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state, d_out, dX, dC, d_scale, d_rho, nullptr, 1, workspace,
                                workspace_bytes, stream);
}
