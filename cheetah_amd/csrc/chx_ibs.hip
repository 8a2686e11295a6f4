// chx_ibs.hip — intrabeam scattering (IBSKick element): the growth of the slice energy spread by multiple small-angle Coulomb
// scattering inside the bunch, Bane's high-energy approximation of the Bjorken-Mtingwa rate (EPAC 2002) without dispersion and
// with beta = 1, the bunch average N / sigma_s replaced by the local line density. Per batch row, in fp64, from the reference energy,
// the length L, the Coulomb logarithm Lambda, the rms sizes sigma_x, sigma_y and the geometric emittances eps_x, eps_y
// (gamma = E / mc^2, r_c = Z^2 r_e m_e / m):
//   alpha = (sigma_x eps_y) / (sigma_y eps_x),   g(alpha) = sqrt(alpha) / AGM(1, alpha)   (8 steps of (a, b) <- ((a + b) / 2, sqrt(a b)))
//   K = sqrt(pi) r_c^2 Lambda L g(alpha) / (4 gamma^3 sqrt(eps_x eps_y sigma_x sigma_y) |Z| e)
//   V_k = (K / h) D_k                            the variance of delta at node k; D_k, h: the family's deposit and node spacing
// and per particle at its node coordinate (k, f), V(u) = (1 - f) V_k + f V_(k+1):  delta' = delta + sqrt(V(u)) xi.
// xi is one standard normal per (kick, call, batch row, particle): Philox4x32-10 (chx_philox.h) with key (seed, stream) and counter
// (particle n, b + 2^31, call_lo, call_hi); B <= 65535, so bit 31 of the second word keeps this kick's draws apart from those of
// chx_sr.hip at the same key and call index. The call index is read from device memory, so a captured graph follows it. Nothing of
// xi is stored: the backward pass draws it again.
//   F1. wake_range_kernel     (chx_grid1d_dev.h) partials of the surviving particles' tau range and charge; zeroes the grid
//   F2. wake_deposit_kernel   (chx_grid1d_dev.h) the row header and the fixed-point node deposit D_k (one channel)
//   F3. ibs_node_kernel       one thread per node: K / h formed from the settings (into the header's last slot), V_k and D_k stored
//   F4. ibs_kick_kernel       one thread per particle: gather of V(u), the draw, delta updated in fp64 and rounded once
// Backward, with the per-particle weight a_n = g_delta xi / (2 sqrt(V(u))) (0 where V(u) is not > 0), the family's pattern:
//   B1. ibs_bwd_range_kernel     the bound sum |a_n| of the cotangents' deposit; zeroes the cotangents' grid
//   B2. ibs_bwd_deposit_kernel   the fixed-point deposit GV_k = sum_n a_n hat_k(u_n)
//   B3. ibs_bwd_node_kernel      one workgroup per row: the deposits' cotangents (K / h) GV_k and d(K / h) = sum_k GV_k D_k
//   B4. ibs_bwd_particles_kernel one thread per particle: d(tau) through V(u) and through the deposit's adjoint, dC, d(delta) passes
// Every sum in a fixed order, no float atomics: bitwise reproducible. The deposit, the argument check, the workspace and the node
// coordinate are chx_grid1d_dev.h and chx_grid1d_host.h, shared with chx_wake.hip, chx_csr.hip and chx_lsc.hip.
#include "chx_grid1d_host.h"
#include "chx_philox.h"

namespace {

constexpr double kElectronRadius = 2.8179403205e-15;     // r_e, m (as chx_sr.hip)
constexpr double kElectronMass = 510998.95069;           // m_e c^2, eV (as chx_sr.hip)
constexpr double kUnitCharge = 1.602176634e-19;          // e, C
constexpr double kSqrtPi = 1.7724538509055160273;
constexpr int kSettings = 7;                             // energy, length, coulomb_log, sigma_x, sigma_y, eps_x, eps_y

__host__ __device__ inline int64_t ibs_state_row(int M) { return CHX_IBS_STATE_DOUBLES(M); }
// state row: [0, kHdr) the header with K / h in its last slot | [kHdr, kHdr + M) node variances V_k | M deposits D_k
__host__ __device__ inline int ibs_dep_slot(int M) { return kHdr + M; }

Grid1dWs ibs_ws(void* base, int64_t B, int64_t N, int M) { return grid1d_ws(base, B, N, M, 1, 0); }

struct IbsKey {
    uint32_t seed, stream;
};

// The settings as the entry point gets them: device arrays of the beam's dtype, each of 1 or B rows.
template <typename T> struct IbsSettings {
    const T* p[kSettings];
    int64_t rows[kSettings];
};

__device__ __forceinline__ void ibs_words(IbsKey key, uint64_t call, int64_t b, int64_t n, uint32_t (&w)[4]) {
    philox4x32_10((uint32_t)n, (uint32_t)b | 0x80000000u, (uint32_t)call, (uint32_t)(call >> 32), key.seed, key.stream, w);
}
__device__ __forceinline__ double ibs_normal(IbsKey key, uint64_t call, int64_t b, int64_t n) {
    uint32_t w[4];
    ibs_words(key, call, b, n, w);
    return philox_normal_of(w);
}

// The row's K in fp64. A row in which any of Lambda, sigma_x, sigma_y, eps_x, eps_y is not > 0 or not finite gives NaN.
template <typename T>
__device__ double ibs_strength(const IbsSettings<T>& s, double mass, double absz, int64_t b) {
    double v[kSettings];
#pragma unroll
    for (int i = 0; i < kSettings; ++i) v[i] = (double)s.p[i][s.rows[i] == 1 ? 0 : b];
    bool ok = true;
#pragma unroll
    for (int i = 2; i < kSettings; ++i) ok = ok && v[i] > 0.0 && isfinite(v[i]);
    if (!ok) return __longlong_as_double(0x7ff8000000000000LL);
    const double gamma = v[0] / mass, L = v[1], lambda = v[2], sx = v[3], sy = v[4], ex = v[5], ey = v[6];
    const double alpha = (sx * ey) / (sy * ex);
    double a = 1.0, c = alpha;
    for (int i = 0; i < 8; ++i) {
        const double m = 0.5 * (a + c);
        c = sqrt(a * c);
        a = m;
    }
    const double g = sqrt(alpha) / a;
    const double rc = absz * absz * kElectronRadius * kElectronMass / mass;
    return kSqrtPi * (rc * rc) * lambda * L * g / (4.0 * (gamma * gamma * gamma) * sqrt(ex * ey * sx * sy) * absz * kUnitCharge);
}

// V(u) of a particle from the row's node variances; false where there is no kick (both nodes 0, or V(u) = 0): delta keeps its bits.
// A NaN (a NaN tau, an invalid row) is a kick.
__device__ __forceinline__ bool ibs_variance(const double* st, int M, double tau, int& k, double& f, bool& in, double& V) {
    wake_node(tau, st[1], st[2], M, k, f, in);
    const double v0 = st[kHdr + k], v1 = st[kHdr + k + 1];
    V = 0.0;
    if (v0 == 0.0 && v1 == 0.0) return false;
    V = (1.0 - f) * v0 + f * v1;
    return V != 0.0;
}

// The backward pass's weight of a particle: the cotangent of V(u), a = g_delta xi / (2 sqrt(V(u))); 0 where V(u) is not > 0.
__device__ __forceinline__ double ibs_weight(const double* st, int M, double tau, double g5, IbsKey key, uint64_t call, int64_t b,
                                             int64_t n, int& k, double& f, bool& in) {
    double V;
    if (!ibs_variance(st, M, tau, k, f, in, V) || !(V > 0.0)) return 0.0;
    return g5 * ibs_normal(key, call, b, n) / (2.0 * sqrt(V));
}

// ---- F3 ----------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kWB) void ibs_node_kernel(int M, IbsSettings<T> set, double mass, double absz,
                                                       const unsigned long long* __restrict__ grid, double* __restrict__ state) {
    __shared__ double scale;
    const int64_t b = blockIdx.y;
    double* st = state + b * ibs_state_row(M);
    const bool live = node_live(st);
    const double SQ = st[3];
    if (threadIdx.x == 0) {
        scale = live ? ibs_strength(set, mass, absz, b) / st[2] : 0.0;
        if (blockIdx.x == 0) st[kHdr - 1] = scale;
    }
    __syncthreads();
    const int k = blockIdx.x * kWB + threadIdx.x;
    if (k < M) {
        const double d = live ? from_fixed(grid[b * M + k], SQ) : 0.0;
        st[kHdr + k] = live ? scale * d : 0.0;
        st[ibs_dep_slot(M) + k] = d;
    }
}

// ---- F4 ----------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kWB) void ibs_kick_kernel(const T* __restrict__ x, int64_t Bx, int64_t N, int M,
                                                       const double* __restrict__ state, IbsKey key,
                                                       const int64_t* __restrict__ call_index, T* __restrict__ out) {
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * kWB + threadIdx.x;
    if (n >= N) return;
    const T* xr = x + ((Bx == 1 ? 0 : b) * N + n) * 7;
    T* o = out + (b * N + n) * 7;
    T v[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) v[c] = xr[c];
    const double* st = state + b * ibs_state_row(M);
    if (node_live(st)) {
        int k;
        double f, V;
        bool in;
        if (ibs_variance(st, M, (double)v[4], k, f, in, V))
            v[5] = (T)((double)v[5] + sqrt(V) * ibs_normal(key, (uint64_t)call_index[0], b, n));
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) o[c] = v[c];
}

// ---- B1 ----------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kWB) void ibs_bwd_range_kernel(const T* __restrict__ x, int64_t Bx, int64_t N, int G, int M,
                                                            const double* __restrict__ state, const T* __restrict__ gout, IbsKey key,
                                                            const int64_t* __restrict__ call_index, double* __restrict__ bpart,
                                                            unsigned long long* __restrict__ ggrid) {
    __shared__ double red[4 * 3];
    const int64_t b = blockIdx.y;
    const int g = blockIdx.x;
    unsigned long long* gr = ggrid + b * M;
    for (int64_t i = (int64_t)g * kWB + threadIdx.x; i < M; i += (int64_t)G * kWB) gr[i] = 0ull;
    const double* st = state + b * ibs_state_row(M);
    const int64_t chunk = (N + G - 1) / G, n0 = g * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
    double lo = 0.0, hi = 0.0, s[1] = {0.0};
    if (node_live(st)) {
        const uint64_t call = (uint64_t)call_index[0];
        const T* xb = x + (Bx == 1 ? 0 : b) * N * 7;
        const T* gb = gout + b * N * 7;
        for (int64_t n = n0 + threadIdx.x; n < n1; n += kWB) {
            int k;
            double f;
            bool in;
            s[0] += fabs(ibs_weight(st, M, (double)xb[n * 7 + 4], (double)gb[n * 7 + 5], key, call, b, n, k, f, in));
        }
    }
    block_reduce<1>(lo, hi, s, red);
    if (threadIdx.x == 0) {
        double* p = bpart + (b * G + g) * kPart;
        p[0] = s[0]; p[1] = p[2] = p[3] = p[4] = p[5] = p[6] = p[7] = 0.0;
    }
}

// ---- B2: as F2 (hist: M integers of dynamic LDS); workgroup 0 writes the backward header (valid, S of the cotangent deposit) -------
template <typename T>
__global__ __launch_bounds__(kWB) void ibs_bwd_deposit_kernel(const T* __restrict__ x, int64_t Bx, int64_t N, int G, int M,
                                                              const double* __restrict__ state, const T* __restrict__ gout,
                                                              IbsKey key, const int64_t* __restrict__ call_index,
                                                              const double* __restrict__ bpart, double* __restrict__ bhdr,
                                                              unsigned long long* __restrict__ ggrid) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long hist[];   // [M]
    __shared__ double red[4 * 3];
    __shared__ double S;
    const int64_t b = blockIdx.y;
    const int g = blockIdx.x;
    const double* st = state + b * ibs_state_row(M);
    double lo = 0.0, hi = 0.0, s[1] = {0.0};
    for (int gg = threadIdx.x; gg < G; gg += kWB) s[0] += bpart[(b * G + gg) * kPart];
    block_reduce<1>(lo, hi, s, red);
    if (threadIdx.x == 0) {
        S = fixed_scale(s[0]);
        if (g == 0) {
            bhdr[b * kHdr] = st[0];
            bhdr[b * kHdr + 1] = S;
        }
    }
    __syncthreads();
    if (!node_live(st)) return;
    const double S0 = S;
    for (int i = threadIdx.x; i < M; i += kWB) hist[i] = 0ull;
    __syncthreads();
    const uint64_t call = (uint64_t)call_index[0];
    const T* xb = x + (Bx == 1 ? 0 : b) * N * 7;
    const T* gb = gout + b * N * 7;
    const int64_t chunk = (N + G - 1) / G, n0 = g * chunk, n1 = n0 + chunk < N ? n0 + chunk : N;
    for (int64_t n = n0 + threadIdx.x; n < n1; n += kWB) {
        int k;
        double f;
        bool in;
        const double a = ibs_weight(st, M, (double)xb[n * 7 + 4], (double)gb[n * 7 + 5], key, call, b, n, k, f, in);
        if (a == 0.0) continue;                      // NaN tau included: its V(u) is not > 0
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

// ---- B3: one workgroup per row; thread t takes the nodes t, t + 256, ... in order, then the workgroup's fixed tree ------------------
__global__ __launch_bounds__(kWB) void ibs_bwd_node_kernel(int M, const double* __restrict__ state, const double* __restrict__ bhdr,
                                                           const unsigned long long* __restrict__ ggrid, double* __restrict__ adj,
                                                           double* __restrict__ d_scale) {
    __shared__ double red[4 * 3];
    const int64_t b = blockIdx.x;
    const double* st = state + b * ibs_state_row(M);
    const bool live = node_live(st);
    const double sc = st[kHdr - 1], SV = bhdr[b * kHdr + 1];
    double lo = 0.0, hi = 0.0, s[1] = {0.0};
    for (int k = threadIdx.x; k < M; k += kWB) {
        const double gv = live ? from_fixed(ggrid[b * M + k], SV) : 0.0;
        adj[b * M + k] = live ? sc * gv : 0.0;
        s[0] += gv * st[ibs_dep_slot(M) + k];
    }
    block_reduce<1>(lo, hi, s, red);
    if (threadIdx.x == 0) d_scale[b] = s[0];
}

// ---- B4 ----------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kWB) void ibs_bwd_particles_kernel(const T* __restrict__ x, const T* __restrict__ q,
                                                                const T* __restrict__ w, int64_t Bx, int64_t Bq, int64_t Bw,
                                                                int64_t N, int M, const double* __restrict__ state,
                                                                const double* __restrict__ adj, const T* __restrict__ gout,
                                                                IbsKey key, const int64_t* __restrict__ call_index,
                                                                T* __restrict__ dX, T* __restrict__ dC) {
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * kWB + threadIdx.x;
    if (n >= N) return;
    const RowPtrs<T> r = row_ptrs(x, q, w, Bx, Bq, Bw, N, b);
    const T* gr = gout + (b * N + n) * 7;
    double gv[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) gv[c] = (double)gr[c];
    const double* st = state + b * ibs_state_row(M);
    double dc = 0.0;
    if (node_live(st)) {
        const double tau = (double)r.x[n * 7 + 4];
        int k;
        double f;
        bool in;
        const double a = ibs_weight(st, M, tau, gv[5], key, (uint64_t)call_index[0], b, n, k, f, in);
        const double* ad = adj + b * M;
        double df = a != 0.0 ? a * (st[kHdr + k + 1] - st[kHdr + k]) : 0.0;
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

// ---- the draw itself -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWB) void ibs_normals_kernel(IbsKey key, uint64_t call, int64_t N, uint32_t* __restrict__ words,
                                                          double* __restrict__ xi) {
    const int64_t b = blockIdx.y, n = (int64_t)blockIdx.x * kWB + threadIdx.x;
    if (n >= N) return;
    uint32_t w[4];
    ibs_words(key, call, b, n, w);
    uint4* dst = reinterpret_cast<uint4*>(words) + (b * N + n);
    *dst = make_uint4(w[0], w[1], w[2], w[3]);
    xi[b * N + n] = philox_normal_of(w);
}

inline dim3 grid_node_threads(int M, int64_t B) { return dim3((unsigned)((M + kWB - 1) / kWB), (unsigned)B); }

template <typename T>
int ibs_kick_t(const T* x, const T* q, const T* w, const IbsSettings<T>& set, double mass, double absz, IbsKey key,
               const int64_t* call_index, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int M, T* out, double* state,
               const Grid1dWs& ws, hipStream_t s) {
    int st = launch_deposit(x, q, w, B, Bx, Bq, Bw, N, M, 0, 1, 1, ibs_state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(ibs_node_kernel<T>, grid_node_threads(M, B), dim3(kWB), 0, s, M, set, mass, absz, ws.grid, state);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(ibs_kick_kernel<T>, grid_particles(N, B), dim3(kWB), 0, s, x, Bx, N, M, state, key, call_index, out);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

template <typename T>
int ibs_kick_bwd_t(const T* x, const T* q, const T* w, IbsKey key, const int64_t* call_index, int64_t B, int64_t Bx, int64_t Bq,
                   int64_t Bw, int64_t N, int M, const double* state, const T* gout, T* dX, T* dC, double* d_scale,
                   const Grid1dWs& ws, hipStream_t s) {
    const int G = wake_groups(N);
    const size_t lds = (size_t)M * 8;
    if (!lds_ok(ibs_bwd_deposit_kernel<T>, lds)) return CHX_ERR_LAUNCH;
    hipLaunchKernelGGL(ibs_bwd_range_kernel<T>, grid_groups(N, B), dim3(kWB), 0, s, x, Bx, N, G, M, state, gout, key, call_index,
                       ws.bpart, ws.ggrid);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(ibs_bwd_deposit_kernel<T>, grid_groups(N, B), dim3(kWB), lds, s, x, Bx, N, G, M, state, gout, key, call_index,
                       ws.bpart, ws.bhdr, ws.ggrid);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(ibs_bwd_node_kernel, dim3((unsigned)B), dim3(kWB), 0, s, M, state, ws.bhdr, ws.ggrid, ws.adj, d_scale);
    CHX_CHECK_LAUNCH();
    const int st = launch_adj_filter(B, M, 1, ibs_state_row(M), state, ws, s);
    if (st != CHX_OK) return st;
    hipLaunchKernelGGL(ibs_bwd_particles_kernel<T>, grid_particles(N, B), dim3(kWB), 0, s, x, q, w, Bx, Bq, Bw, N, M, state,
                       ws.adj_last, gout, key, call_index, dX, dC);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace

// Every entry point has a twin that takes cutoff[Bcut] in front of the workspace (the low-pass stage of chx_grid1d_dev.h, launched by
// launch_deposit and launch_adj_filter); the call without the suffix is the twin with a null cutoff.
extern "C" size_t chx_ibs_workspace_bytes(int64_t B, int64_t N, int32_t M) { return ibs_ws(nullptr, B, N, M).bytes; }
extern "C" size_t chx_ibs_workspace_bytes_cut(int64_t B, int64_t N, int32_t M) {
    return cutoff_ws_bytes(ibs_ws(nullptr, B, N, M), B, M, 1);
}

extern "C" int chx_ibs_kick_cut(const void* x, const void* q, const void* w, const void* energy, const void* length,
                                const void* coulomb_log, const void* sigma_x, const void* sigma_y, const void* eps_x,
                                const void* eps_y, double mass_eV, double abs_charge, uint32_t seed, uint32_t rng_stream,
                                const int64_t* call_index, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl,
                                int64_t Bc, int64_t Bsx, int64_t Bsy, int64_t Bex, int64_t Bey, int64_t N, int32_t M, int dtype,
                                void* out, double* state, const double* cutoff, int64_t Bcut, void* workspace,
                                size_t workspace_bytes, void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    const void* ptrs[kSettings] = {energy, length, coulomb_log, sigma_x, sigma_y, eps_x, eps_y};
    const int64_t rows[kSettings] = {Be, Bl, Bc, Bsx, Bsy, Bex, Bey};
    for (int i = 0; i < kSettings; ++i)
        if (!ptrs[i] || !chx_bcast_ok(rows[i], B)) return CHX_ERR_INVALID_ARG;
    if (!(mass_eV > 0.0) || !call_index || !out) return CHX_ERR_INVALID_ARG;
    if (!chx_aligned16(out)) return CHX_ERR_MISALIGNED;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(ibs_ws(workspace, B, N, M), workspace, B, M, 1, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        IbsSettings<T> set;
        for (int i = 0; i < kSettings; ++i) {
            set.p[i] = (const T*)ptrs[i];
            set.rows[i] = rows[i];
        }
        return ibs_kick_t<T>((const T*)x, (const T*)q, (const T*)w, set, mass_eV, abs_charge, IbsKey{seed, rng_stream}, call_index, B,
                             Bx, Bq, Bw, N, M, (T*)out, state, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_ibs_kick(const void* x, const void* q, const void* w, const void* energy, const void* length,
                            const void* coulomb_log, const void* sigma_x, const void* sigma_y, const void* eps_x, const void* eps_y,
                            double mass_eV, double abs_charge, uint32_t seed, uint32_t rng_stream, const int64_t* call_index,
                            int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t Be, int64_t Bl, int64_t Bc, int64_t Bsx,
                            int64_t Bsy, int64_t Bex, int64_t Bey, int64_t N, int32_t M, int dtype, void* out, double* state,
                            void* workspace, size_t workspace_bytes, void* stream) {
    return chx_ibs_kick_cut(x, q, w, energy, length, coulomb_log, sigma_x, sigma_y, eps_x, eps_y, mass_eV, abs_charge, seed,
                            rng_stream, call_index, B, Bx, Bq, Bw, Be, Bl, Bc, Bsx, Bsy, Bex, Bey, N, M, dtype, out, state, nullptr,
                            1, workspace, workspace_bytes, stream);
}

extern "C" int chx_ibs_kick_bwd_cut(const void* x, const void* q, const void* w, uint32_t seed, uint32_t rng_stream,
                                    const int64_t* call_index, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int32_t M,
                                    int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale,
                                    const double* cutoff, int64_t Bcut, void* workspace, size_t workspace_bytes, void* stream) {
    const int st = check_grid1d(x, q, w, B, Bx, Bq, Bw, N, M, dtype, state);
    if (st != CHX_OK) return st;
    if (!call_index || !d_out || !dX || !d_scale) return CHX_ERR_INVALID_ARG;
    if (!cutoff_ok(cutoff, Bcut, B)) return CHX_ERR_INVALID_ARG;
    const Grid1dWs ws = with_cutoff(ibs_ws(workspace, B, N, M), workspace, B, M, 1, cutoff, Bcut);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return ibs_kick_bwd_t<T>((const T*)x, (const T*)q, (const T*)w, IbsKey{seed, rng_stream}, call_index, B, Bx, Bq, Bw, N, M,
                                 state, (const T*)d_out, (T*)dX, (T*)dC, d_scale, ws, (hipStream_t)stream);
    });
}

extern "C" int chx_ibs_kick_bwd(const void* x, const void* q, const void* w, uint32_t seed, uint32_t rng_stream,
                                const int64_t* call_index, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int32_t M,
                                int dtype, const double* state, const void* d_out, void* dX, void* dC, double* d_scale,
                                void* workspace, size_t workspace_bytes, void* stream) {
    return chx_ibs_kick_bwd_cut(x, q, w, seed, rng_stream, call_index, B, Bx, Bq, Bw, N, M, dtype, state, d_out, dX, dC, d_scale,
                                nullptr, 1, workspace, workspace_bytes, stream);
}

extern "C" int chx_ibs_normals(uint32_t seed, uint32_t rng_stream, uint64_t call, int64_t B, int64_t N, uint32_t* words_out,
                               double* xi_out, void* stream) {
    if (B < 1 || B > 65535 || N < 1 || N > 0x7fffffffLL || !words_out || !xi_out) return CHX_ERR_INVALID_ARG;
    if (!chx_aligned16(words_out)) return CHX_ERR_MISALIGNED;
    hipLaunchKernelGGL(ibs_normals_kernel, grid_particles(N, B), dim3(kWB), 0, (hipStream_t)stream, IbsKey{seed, rng_stream}, call, N,
                       words_out, xi_out);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}
