// chx_density.hip — seeded density modulation (ParticleBeam.with_density_modulation): the beam's longitudinal density times
// 1 + sum_m A_m cos(2 pi tau / lambda_m + phi_m), K <= 8 modes, by moving every particle's tau to the root tau' of
//   tau' + sum_m c_m sin(2 pi (tau' nu_m + phi_t,m)) = tau,    nu_m = 1 / lambda_m, phi_t,m = phi_m / fl(2 pi), c_m = A_m / (fl(2 pi) nu_m)
// (exact for a uniform envelope; the map is monotone, and its root unique, only for sum |A_m| < 1). Per batch row the settings
// amplitudes, wavelengths, phases [1 or B][K] are fp64 whatever the beam dtype, and so is all arithmetic; tau' is rounded once on the
// store. The phase of mode m at t, in turns as chx_laser.hip reduces it:
//   w = fl(fl(t nu_m) + phi_t,m)    product and sum rounded separately, never one fma
//   f = w - rint(w)                 exact, |f| <= 1/2;  (sin theta_m, cos theta_m) = sincospi(2 f)
// Solver: at most kIterations steps from t = tau: with g = t + sum c_m sin theta_m - tau and D = 1 + sum A_m cos theta_m the bracket
// [lo, hi], from tau -+ sum |c_m|, takes t on the side of the sign of g, and the step is Newton's t - g / D where that stays inside
// the bracket, the bracket's middle otherwise. A particle is done after a Newton step no longer than tol = 2^-30 of the row's shortest wavelength:
// Newton's error is squared by every step (times pi sum |A_m| / D < 63), so behind such a step it is below 10^-16 wavelengths. A
// function of the particle and its row alone: deterministic whatever the launch. Plain Newton needs 3 to 8 steps (sum |A_m| from
// 0.02 to 0.9); the middle is taken where the root lies next to the bracket's end (sin = -+1 there) and Newton's overshoot leaves
// it, and each such step halves the distance: a root within eps of the end (in units of the bracket) costs about
// log2(sum |A_m| / sqrt(2 eps)) of them, 20 before eps falls below fp64's rounding. Hence the cap of 32.
// Every column but tau keeps its bits; a row whose A_m are all 0 keeps every bit; a non-finite tau stays as it is; in a row with
// sum |A_m| >= 1 (or NaN) every finite tau becomes NaN.
//   F. density_kernel       one workgroup per (row tile, batch row), the tile's rows through LDS (chx_apply_tiles.h's tile shapes)
//   B1. density_bwd_kernel  the same pass (the root is solved again from x) with the cotangents' tile beside it: dX, and the
//                           workgroup's partial of the cotangents of (A_m, nu_m, phi_t,m)
//   B2. density_rows_kernel one workgroup per batch row adds the partials in a fixed order: bitwise reproducible, no float atomics
//                           (laser_rows_kernel's order; 24 sums per row, hence a sibling)
#include "chx_apply_tiles.h"

namespace {

constexpr double kTwoPi = 6.283185307179586;             // fl(2 pi)
constexpr int kModes = CHX_DENSITY_MAX_MODES;
constexpr int kSums = 3 * kModes;                        // cotangents of A_m, nu_m, phi_t,m
constexpr int kIterations = 32;

template <typename T> struct density_cfg { static constexpr int TP = tile_cfg<T>::PPT * CHX_BLOCK; };
// tiles per batch row of the float64 shape (the smaller tile): what the workspace is sized for in either dtype
inline int64_t density_max_tiles(int64_t N) { return (N + density_cfg<double>::TP - 1) / density_cfg<double>::TP; }

struct DensityRows {
    const double *amplitude, *wavelength, *phase;
    int64_t Ba, Bw, Bp;
    int K;
};

// The row's factors in LDS: A, nu, phi_t, c per mode (0 beyond K), then W = sum |c_m|, sum |A_m|, tol = 2^-30 / max |nu_m| and "some
// A_m != 0".
struct DensityRow {
    double A[kModes], nu[kModes], pt[kModes], c[kModes];
    double W, sumA, tol;
    int any;
};

__device__ __forceinline__ void density_row_factors(const DensityRows& r, int64_t b, DensityRow* f) {
    double W = 0.0, sumA = 0.0, numax = 0.0;
    int any = 0;
    for (int m = 0; m < kModes; ++m) {
        const bool on = m < r.K;
        const double A = on ? r.amplitude[(r.Ba == 1 ? 0 : b) * r.K + m] : 0.0;
        const double nu = on ? 1.0 / r.wavelength[(r.Bw == 1 ? 0 : b) * r.K + m] : 0.0;
        const double pt = on ? r.phase[(r.Bp == 1 ? 0 : b) * r.K + m] / kTwoPi : 0.0;
        const double c = on ? A / (kTwoPi * nu) : 0.0;
        f->A[m] = A;
        f->nu[m] = nu;
        f->pt[m] = pt;
        f->c[m] = c;
        W += fabs(c);
        sumA += fabs(A);
        numax = fmax(numax, fabs(nu));                     // (a negative wavelength on the device: the same periods)
        any |= (A != 0.0);                                 // a NaN amplitude included
    }
    f->W = W;
    f->sumA = sumA;
    f->tol = 0x1p-30 / numax;
    f->any = any;
}

// g + tau = t + sum c_m sin theta_m and D = 1 + sum A_m cos theta_m at t, the modes added in the order m = 0 .. K - 1
__device__ __forceinline__ void density_eval(const DensityRow& f, int K, double t, double& gt, double& D) {
    gt = t;
    D = 1.0;
    for (int m = 0; m < K; ++m) {
        const double w = __dadd_rn(__dmul_rn(t, f.nu[m]), f.pt[m]);
        const double frac = w - rint(w);
        double s, c;
        sincospi(2.0 * frac, &s, &c);
        gt += f.c[m] * s;
        D += f.A[m] * c;
    }
}

__device__ __forceinline__ double density_root(const DensityRow& f, int K, double tau) {
    double lo = tau - f.W, hi = tau + f.W, t = tau;
    for (int it = 0; it < kIterations; ++it) {
        double gt, D;
        density_eval(f, K, t, gt, D);
        const double g = gt - tau;
        if (g < 0.0) lo = t; else hi = t;
        double tn = t - g / D;
        const bool inside = tn >= lo && tn <= hi;
        if (!inside) tn = 0.5 * (lo + hi);
        const bool done = inside && fabs(tn - t) <= f.tol;
        t = tn;
        if (done) break;
    }
    return t;
}

// ---- F ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void density_kernel(const T* __restrict__ x, DensityRows settings, int64_t B, int64_t Bx,
                                                            int64_t N, T* __restrict__ out, int in_vec_ok) {
    constexpr int TP = density_cfg<T>::TP, PPT = tile_cfg<T>::PPT;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    __shared__ DensityRow row;
    const int64_t b = blockIdx.y, n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const T* gin = x + (in_row * N + n0) * 7;
    T* gout = out + (b * N + n0) * 7;
    const bool in_vec = CHX_TILE_VEC_OK(T, in_vec_ok, in_row, N), out_vec = CHX_TILE_VEC_OK(T, 1, b, N);
    if (threadIdx.x == 0) density_row_factors(settings, b, &row);
    tile_load<T, TP>(gin, lds, np * 7, in_vec, !(Bx == 1 && B > 1));
    __syncthreads();
    if (row.any) {                                                 // a row with every A_m = 0 keeps every bit
        const bool unique = row.sumA < 1.0;
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int p = threadIdx.x + k * CHX_BLOCK;
            if (p < np) {
                const double tau = (double)lds[p * 7 + 4];
                if (isfinite(tau)) lds[p * 7 + 4] = (T)(unique ? density_root(row, settings.K, tau) : nan);
            }
        }
    }
    __syncthreads();
    tile_store<T, TP>(gout, lds, np * 7, out_vec, true);
}

// ---- B1 --------------------------------------------------------------------------------------------------------------------------
// By the implicit function, with G the cotangent of tau', theta_m the phase of mode m at tau' and D = 1 + sum A_m cos theta_m:
// dX = d_out in every column but tau's, which gets G / D; the row's cotangents sum G_A,m = -G sin theta_m / (2 pi nu_m D),
// G_nu,m = G (A_m sin theta_m / (2 pi nu_m^2) - A_m tau' cos theta_m / nu_m) / D, G_phit,m = -G A_m cos theta_m / (nu_m D). A particle
// whose tau' is not finite has no gradient: its tau column gets 0 and it adds nothing (a non-finite tau that the forward pass hands
// on included).
template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void density_bwd_kernel(const T* __restrict__ x, DensityRows settings, int64_t B, int64_t Bx,
                                                                int64_t N, const T* __restrict__ gout, T* __restrict__ dX,
                                                                double* __restrict__ partials, int64_t max_tiles, int in_vec_ok,
                                                                int g_vec_ok) {
    constexpr int TP = density_cfg<T>::TP, PPT = tile_cfg<T>::PPT;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    __shared__ __attribute__((aligned(16))) T gl[TP * 7];
    __shared__ DensityRow row;
    __shared__ double red[4 * kSums];
    const int64_t b = blockIdx.y, n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const bool in_vec = CHX_TILE_VEC_OK(T, in_vec_ok, in_row, N), g_vec = CHX_TILE_VEC_OK(T, g_vec_ok, b, N),
               out_vec = CHX_TILE_VEC_OK(T, 1, b, N);
    if (threadIdx.x == 0) density_row_factors(settings, b, &row);
    tile_load<T, TP>(x + (in_row * N + n0) * 7, lds, np * 7, in_vec, !(Bx == 1 && B > 1));
    tile_load<T, TP>(gout + (b * N + n0) * 7, gl, np * 7, g_vec, true);
    __syncthreads();
    const int K = settings.K;
    const bool unique = row.sumA < 1.0;
    double acc[kSums];
#pragma unroll
    for (int j = 0; j < kSums; ++j) acc[j] = 0.0;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = threadIdx.x + k * CHX_BLOCK;
        if (p < np) {
            const double tau = (double)lds[p * 7 + 4];
            if (isfinite(tau) && unique) {
                const double t = density_root(row, K, tau);
                double s[kModes], c[kModes], D = 1.0;
#pragma unroll
                for (int m = 0; m < kModes; ++m) {
                    s[m] = 0.0;
                    c[m] = 0.0;
                    if (m < K) {
                        const double w = __dadd_rn(__dmul_rn(t, row.nu[m]), row.pt[m]);
                        const double frac = w - rint(w);
                        sincospi(2.0 * frac, &s[m], &c[m]);
                        D += row.A[m] * c[m];
                    }
                }
                const double GD = (double)gl[p * 7 + 4] / D;
                gl[p * 7 + 4] = (T)GD;
#pragma unroll
                for (int m = 0; m < kModes; ++m) {
                    if (m < K) {
                        const double A = row.A[m], nu = row.nu[m];
                        acc[m] -= GD * s[m] / (kTwoPi * nu);
                        acc[kModes + m] += GD * (A * s[m] / (kTwoPi * nu * nu) - A * t * c[m] / nu);
                        acc[2 * kModes + m] -= GD * A * c[m] / nu;
                    }
                }
            } else {
                gl[p * 7 + 4] = (T)0.0;
            }
        }
    }
    chx_block_sum<kSums>(acc, red);                               // its barriers also order the tile's writes before the store
    if (threadIdx.x == 0) {
        double* dst = partials + (b * max_tiles + blockIdx.x) * kSums;
#pragma unroll
        for (int j = 0; j < kSums; ++j) dst[j] = acc[j];
    }
    tile_store<T, TP>(dX + (b * N + n0) * 7, gl, np * 7, out_vec, true);
}

// ---- B2: thread t adds the partials t, t + 256, ... of its row in order, then the workgroup's fixed tree ---------------------------
__global__ __launch_bounds__(CHX_BLOCK) void density_rows_kernel(const double* __restrict__ partials, int64_t max_tiles,
                                                                 int64_t tiles, double* __restrict__ d_rows) {
    __shared__ double red[4 * kSums];
    const int64_t b = blockIdx.x;
    double acc[kSums];
#pragma unroll
    for (int j = 0; j < kSums; ++j) acc[j] = 0.0;
    for (int64_t t = threadIdx.x; t < tiles; t += CHX_BLOCK) {
        const double* src = partials + (b * max_tiles + t) * kSums;
#pragma unroll
        for (int j = 0; j < kSums; ++j) acc[j] += src[j];
    }
    chx_block_sum<kSums>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < kSums; ++j) d_rows[b * kSums + j] = acc[j];
    }
}

// B rows are grid.y; N as chx_laser_kick's
bool density_shape_ok(int64_t B, int64_t N) { return B >= 1 && B <= 65535 && N >= 1 && N <= 0xffffffffLL; }

bool density_args_ok(const void* x, const DensityRows& s, int64_t K, int64_t B, int64_t Bx, int64_t N) {
    return density_shape_ok(B, N) && x && s.amplitude && s.wavelength && s.phase && K >= 1 && K <= kModes && chx_bcast_ok(Bx, B) &&
           chx_bcast_ok(s.Ba, B) && chx_bcast_ok(s.Bw, B) && chx_bcast_ok(s.Bp, B);
}

template <typename T>
dim3 density_grid(int64_t B, int64_t N) {
    return dim3((unsigned)((N + density_cfg<T>::TP - 1) / density_cfg<T>::TP), (unsigned)B);
}

}  // namespace

extern "C" size_t chx_density_workspace_bytes(int64_t B, int64_t N) {
    return density_shape_ok(B, N) ? (size_t)(B * density_max_tiles(N)) * kSums * sizeof(double) : 0;
}

extern "C" int chx_density_modulate(const void* x, const double* amplitudes, const double* wavelengths, const double* phases, int64_t K,
                                    int64_t B, int64_t Bx, int64_t Ba, int64_t Bw, int64_t Bp, int64_t N, int dtype, void* out,
                                    void* stream) {
    const DensityRows s{amplitudes, wavelengths, phases, Ba, Bw, Bp, (int)K};
    if (!density_args_ok(x, s, K, B, Bx, N) || !out) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!chx_aligned16(out)) return CHX_ERR_MISALIGNED;
    return dispatch_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL(density_kernel<T>, density_grid<T>(B, N), dim3(CHX_BLOCK), 0, (hipStream_t)stream, (const T*)x, s, B, Bx, N,
                           (T*)out, (int)chx_aligned16(x));
        CHX_CHECK_LAUNCH();
        return CHX_OK;
    });
}

extern "C" int chx_density_modulate_bwd(const void* x, const double* amplitudes, const double* wavelengths, const double* phases,
                                        int64_t K, int64_t B, int64_t Bx, int64_t Ba, int64_t Bw, int64_t Bp, int64_t N, int dtype,
                                        const void* d_out, void* dX, double* d_rows, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    const DensityRows s{amplitudes, wavelengths, phases, Ba, Bw, Bp, (int)K};
    if (!density_args_ok(x, s, K, B, Bx, N) || !d_out || !dX || !d_rows) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!chx_aligned16(dX)) return CHX_ERR_MISALIGNED;
    if (!workspace || workspace_bytes < chx_density_workspace_bytes(B, N)) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        const dim3 grid = density_grid<T>(B, N);
        const int64_t max_tiles = density_max_tiles(N);
        hipLaunchKernelGGL(density_bwd_kernel<T>, grid, dim3(CHX_BLOCK), 0, (hipStream_t)stream, (const T*)x, s, B, Bx, N,
                           (const T*)d_out, (T*)dX, (double*)workspace, max_tiles, (int)chx_aligned16(x), (int)chx_aligned16(d_out));
        CHX_CHECK_LAUNCH();
        hipLaunchKernelGGL(density_rows_kernel, dim3((unsigned)B), dim3(CHX_BLOCK), 0, (hipStream_t)stream,
                           (const double*)workspace, max_tiles, (int64_t)grid.x, d_rows);
        CHX_CHECK_LAUNCH();
        return CHX_OK;
    });
}
