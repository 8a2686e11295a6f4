// chx_laser.hip — laser energy modulation in an undulator (LaserModulator element; Huang et al., PRSTAB 7, 074401 (2004), eq. 8):
// a laser resonant with the undulator radiation modulates the energy at the optical wavelength, following the laser's transverse
// profile and pulse envelope, as one zero-length kick. Per batch row, in fp64 whatever the beam dtype, from the reference energy
// (gamma0 = E0 / mc^2, P0 = beta0 gamma0, formed as chx_sr.hip forms them), the amplitude A (eV), the wavelength lambda, the phase
// phi, the rms size sigma_r of the laser intensity, the laser axis (x0, y0), the rms length sigma_t of the intensity envelope and
// its centre tau0:
//   a = A / (P0 mc^2),  nu = 1 / lambda,  phi_t = phi / fl(2 pi),  g = 1 / (4 sigma_r^2),  h = 1 / (4 sigma_t^2)   (h = 0: no envelope)
// and per particle, in fp64, rounded once on the store, with u = x - x0, v = y - y0, w = tau - tau0:
//   t = fl(fl(tau nu) + phi_t)       the phase in turns: product and sum rounded separately, never one fma
//   f = t - rint(t)                  exact, |f| <= 1/2
//   Ex = exp(-g (u^2 + v^2) - h w^2)
//   delta' = delta + a Ex sin(2 pi f)          sincospi(2 f)
// Every other column keeps its bits, and so does every column of a row with a = 0. A particle whose x, y, tau or delta is not
// finite gets NaN in delta' (a non-finite delta stays what it is) and nothing else of it changes.
//   F. laser_kick_kernel      one workgroup per (row tile, batch row): the tile's rows through LDS (coalesced 16-byte transfers of
//                             the 7-strided rows, chx_apply_tiles.h's tile shapes), a lane takes whole rows
//   B1. laser_kick_bwd_kernel the same pass with the cotangents' tile beside it: dX, and the workgroup's partial of the cotangents
//                             of the eight row factors (a, nu, phi_t, g, x0, y0, h, tau0)
//   B2. laser_rows_kernel     one workgroup per batch row adds the partials in a fixed order: bitwise reproducible, no float
//                             atomics (sr_rows_kernel's order; eight sums into one [B][8] array, hence a sibling)
#include "chx_apply_tiles.h"

namespace {

constexpr double kTwoPi = 6.283185307179586;             // fl(2 pi)
constexpr int kRowFactors = 8;                           // a, nu, phi_t, g, x0, y0, h, tau0

template <typename T> struct laser_cfg { static constexpr int TP = tile_cfg<T>::PPT * CHX_BLOCK; };
// tiles per batch row of the float64 shape (the smaller tile): what the workspace is sized for in either dtype
inline int64_t laser_max_tiles(int64_t N) { return (N + laser_cfg<double>::TP - 1) / laser_cfg<double>::TP; }

// The energy and the eight settings as device arrays of the beam's dtype, each of 1 or B rows; pulse_sigma may be null.
enum { L_ENERGY, L_AMPLITUDE, L_WAVELENGTH, L_PHASE, L_SIGMA, L_X0, L_Y0, L_PULSE_SIGMA, L_PULSE_CENTER, L_SETTINGS };
template <typename T>
struct LaserRows {
    const T* p[L_SETTINGS];
    int64_t rows[L_SETTINGS];
};

template <typename T>
__device__ __forceinline__ void laser_row_factors(const LaserRows<T>& r, double mass, int64_t b, double* f) {
    double v[L_SETTINGS];
#pragma unroll
    for (int k = 0; k < L_SETTINGS; ++k) v[k] = r.p[k] ? (double)r.p[k][r.rows[k] == 1 ? 0 : b] : 0.0;
    const double gamma = v[L_ENERGY] / mass;
    const double beta = fabs(gamma) > 0.0 ? sqrt(fmax(1.0 - 1.0 / (gamma * gamma), 0.0)) : 1.0;
    const double P0 = beta * gamma;
    f[0] = v[L_AMPLITUDE] / (P0 * mass);
    f[1] = 1.0 / v[L_WAVELENGTH];
    f[2] = v[L_PHASE] / kTwoPi;
    f[3] = 1.0 / (4.0 * (v[L_SIGMA] * v[L_SIGMA]));
    f[4] = v[L_X0];
    f[5] = v[L_Y0];
    f[6] = r.p[L_PULSE_SIGMA] ? 1.0 / (4.0 * (v[L_PULSE_SIGMA] * v[L_PULSE_SIGMA])) : 0.0;
    f[7] = v[L_PULSE_CENTER];
}

struct LaserParticle {
    double u, v, w, r2, Ex, s, c;
    bool finite;                          // x, y, tau and delta are finite
};

__device__ __forceinline__ LaserParticle laser_particle(double x, double y, double tau, double delta, const double* f) {
    LaserParticle q;
    q.u = x - f[4];
    q.v = y - f[5];
    q.w = tau - f[7];
    q.r2 = q.u * q.u + q.v * q.v;
    const double t = __dadd_rn(__dmul_rn(tau, f[1]), f[2]);
    const double frac = t - rint(t);
    q.Ex = exp(-f[3] * q.r2 - f[6] * (q.w * q.w));
    sincospi(2.0 * frac, &q.s, &q.c);
    q.finite = isfinite(x) && isfinite(y) && isfinite(tau) && isfinite(delta);
    return q;
}

// ---- F ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void laser_kick_kernel(const T* __restrict__ x, LaserRows<T> settings, double mass, int64_t B,
                                                               int64_t Bx, int64_t N, T* __restrict__ out, int in_vec_ok) {
    constexpr int TP = laser_cfg<T>::TP, PPT = tile_cfg<T>::PPT;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    __shared__ double row[kRowFactors];
    const int64_t b = blockIdx.y, n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const T* gin = x + (in_row * N + n0) * 7;
    T* gout = out + (b * N + n0) * 7;
    const bool in_vec = CHX_TILE_VEC_OK(T, in_vec_ok, in_row, N), out_vec = CHX_TILE_VEC_OK(T, 1, b, N);
    if (threadIdx.x == 0) laser_row_factors(settings, mass, b, row);
    tile_load<T, TP>(gin, lds, np * 7, in_vec, !(Bx == 1 && B > 1));
    __syncthreads();
    double f[kRowFactors];
#pragma unroll
    for (int k = 0; k < kRowFactors; ++k) f[k] = row[k];
    if (f[0] != 0.0) {                                             // a NaN amplitude included; a row with a = 0 keeps every bit
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int p = threadIdx.x + k * CHX_BLOCK;
            if (p < np) {
                const double px = (double)lds[p * 7 + 0], py = (double)lds[p * 7 + 2], tau = (double)lds[p * 7 + 4],
                             delta = (double)lds[p * 7 + 5];
                const LaserParticle q = laser_particle(px, py, tau, delta, f);
                const double nan = __longlong_as_double(0x7ff8000000000000LL);
                lds[p * 7 + 5] = (T)(q.finite ? delta + f[0] * q.Ex * q.s : (isfinite(delta) ? nan : delta));
            }
        }
    }
    __syncthreads();
    tile_store<T, TP>(gout, lds, np * 7, out_vec, true);
}

// ---- B1 --------------------------------------------------------------------------------------------------------------------------
// With G the cotangent of delta' and S = a Ex: dX = d_out in every column, and x's adds -2 g u G S s, y's -2 g v G S s, tau's
// G S (2 pi nu c - 2 h w s). The row's cotangents sum G_a = G Ex s, G_nu = 2 pi tau G S c, G_phit = 2 pi G S c,
// G_g = -G S s (u^2 + v^2), G_x0 = 2 g u G S s, G_y0 = 2 g v G S s, G_h = -G S s w^2, G_tau0 = 2 h w G S s. A particle whose delta'
// is not finite has no gradient: its delta column gets 0 and it adds nothing (chx_sr_kick_bwd's rule); in a row with a = 0, whose
// forward pass hands every bit on, it hands delta's cotangent on as well.
template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void laser_kick_bwd_kernel(const T* __restrict__ x, LaserRows<T> settings, double mass,
                                                                   int64_t B, int64_t Bx, int64_t N, const T* __restrict__ gout,
                                                                   T* __restrict__ dX, double* __restrict__ partials,
                                                                   int64_t max_tiles, int in_vec_ok, int g_vec_ok) {
    constexpr int TP = laser_cfg<T>::TP, PPT = tile_cfg<T>::PPT;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    __shared__ __attribute__((aligned(16))) T gl[TP * 7];
    __shared__ double row[kRowFactors];
    __shared__ double red[4 * kRowFactors];
    const int64_t b = blockIdx.y, n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const bool in_vec = CHX_TILE_VEC_OK(T, in_vec_ok, in_row, N), g_vec = CHX_TILE_VEC_OK(T, g_vec_ok, b, N),
               out_vec = CHX_TILE_VEC_OK(T, 1, b, N);
    if (threadIdx.x == 0) laser_row_factors(settings, mass, b, row);
    tile_load<T, TP>(x + (in_row * N + n0) * 7, lds, np * 7, in_vec, !(Bx == 1 && B > 1));
    tile_load<T, TP>(gout + (b * N + n0) * 7, gl, np * 7, g_vec, true);
    __syncthreads();
    double f[kRowFactors];
#pragma unroll
    for (int k = 0; k < kRowFactors; ++k) f[k] = row[k];
    const double a = f[0], nu = f[1], g = f[3], h = f[6];
    double acc[kRowFactors] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = threadIdx.x + k * CHX_BLOCK;
        if (p < np) {
            const double px = (double)lds[p * 7 + 0], py = (double)lds[p * 7 + 2], tau = (double)lds[p * 7 + 4],
                         delta = (double)lds[p * 7 + 5];
            const LaserParticle q = laser_particle(px, py, tau, delta, f);
            if (q.finite) {
                const double G = (double)gl[p * 7 + 5];
                const double GS = G * (a * q.Ex), GSs = GS * q.s, GSc = GS * q.c;
                gl[p * 7 + 0] = (T)((double)gl[p * 7 + 0] - 2.0 * g * q.u * GSs);
                gl[p * 7 + 2] = (T)((double)gl[p * 7 + 2] - 2.0 * g * q.v * GSs);
                gl[p * 7 + 4] = (T)((double)gl[p * 7 + 4] + (kTwoPi * nu * GSc - 2.0 * h * q.w * GSs));
                acc[0] += G * q.Ex * q.s;
                acc[1] += kTwoPi * tau * GSc;
                acc[2] += kTwoPi * GSc;
                acc[3] -= GSs * q.r2;
                acc[4] += 2.0 * g * q.u * GSs;
                acc[5] += 2.0 * g * q.v * GSs;
                acc[6] -= GSs * (q.w * q.w);
                acc[7] += 2.0 * h * q.w * GSs;
            } else if (a != 0.0) {
                gl[p * 7 + 5] = (T)0.0;
            }
        }
    }
    chx_block_sum<kRowFactors>(acc, red);                         // its barriers also order the tile's writes before the store
    if (threadIdx.x == 0) {
        double* dst = partials + (b * max_tiles + blockIdx.x) * kRowFactors;
#pragma unroll
        for (int k = 0; k < kRowFactors; ++k) dst[k] = acc[k];
    }
    tile_store<T, TP>(dX + (b * N + n0) * 7, gl, np * 7, out_vec, true);
}

// ---- B2: thread t adds the partials t, t + 256, ... of its row in order, then the workgroup's fixed tree ---------------------------
__global__ __launch_bounds__(CHX_BLOCK) void laser_rows_kernel(const double* __restrict__ partials, int64_t max_tiles, int64_t tiles,
                                                               double* __restrict__ d_rows) {
    __shared__ double red[4 * kRowFactors];
    const int64_t b = blockIdx.x;
    double acc[kRowFactors] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t t = threadIdx.x; t < tiles; t += CHX_BLOCK) {
        const double* src = partials + (b * max_tiles + t) * kRowFactors;
#pragma unroll
        for (int k = 0; k < kRowFactors; ++k) acc[k] += src[k];
    }
    chx_block_sum<kRowFactors>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kRowFactors; ++k) d_rows[b * kRowFactors + k] = acc[k];
    }
}

// B rows are grid.y; N as chx_sr_kick's
bool laser_shape_ok(int64_t B, int64_t N) { return B >= 1 && B <= 65535 && N >= 1 && N <= 0xffffffffLL; }

struct LaserArgs {
    const void* p[L_SETTINGS];
    int64_t rows[L_SETTINGS];
};

bool laser_settings_ok(const void* x, const LaserArgs& s, double mass, int64_t B, int64_t Bx, int64_t N) {
    if (!laser_shape_ok(B, N) || !x || !(mass > 0.0) || !chx_bcast_ok(Bx, B)) return false;
    for (int k = 0; k < L_SETTINGS; ++k) {
        if (!s.p[k] && k != L_PULSE_SIGMA) return false;
        if (!chx_bcast_ok(s.rows[k], B)) return false;
    }
    return true;
}

template <typename T>
LaserRows<T> laser_rows_of(const LaserArgs& s) {
    LaserRows<T> r;
    for (int k = 0; k < L_SETTINGS; ++k) {
        r.p[k] = (const T*)s.p[k];
        r.rows[k] = s.rows[k];
    }
    return r;
}

template <typename T>
dim3 laser_grid(int64_t B, int64_t N) { return dim3((unsigned)((N + laser_cfg<T>::TP - 1) / laser_cfg<T>::TP), (unsigned)B); }

template <typename T>
int laser_kick_t(const T* x, const LaserArgs& s, double mass, int64_t B, int64_t Bx, int64_t N, T* out, hipStream_t st) {
    hipLaunchKernelGGL(laser_kick_kernel<T>, laser_grid<T>(B, N), dim3(CHX_BLOCK), 0, st, x, laser_rows_of<T>(s), mass, B, Bx, N, out,
                       (int)chx_aligned16(x));
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

template <typename T>
int laser_kick_bwd_t(const T* x, const LaserArgs& s, double mass, int64_t B, int64_t Bx, int64_t N, const T* gout, T* dX,
                     double* d_rows, double* partials, hipStream_t st) {
    const dim3 grid = laser_grid<T>(B, N);
    const int64_t max_tiles = laser_max_tiles(N);
    hipLaunchKernelGGL(laser_kick_bwd_kernel<T>, grid, dim3(CHX_BLOCK), 0, st, x, laser_rows_of<T>(s), mass, B, Bx, N, gout, dX,
                       partials, max_tiles, (int)chx_aligned16(x), (int)chx_aligned16(gout));
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(laser_rows_kernel, dim3((unsigned)B), dim3(CHX_BLOCK), 0, st, partials, max_tiles, (int64_t)grid.x, d_rows);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace

#define CHX_LASER_ARGS                                                                                                             \
    LaserArgs{{energy, amplitude, wavelength, phase, laser_sigma, offset_x, offset_y, pulse_sigma, pulse_center},                  \
              {Be, Ba, Bw, Bp, Bs, Bx0, By0, Bps, Bpc}}

extern "C" size_t chx_laser_workspace_bytes(int64_t B, int64_t N) {
    return laser_shape_ok(B, N) ? (size_t)(B * laser_max_tiles(N)) * kRowFactors * sizeof(double) : 0;
}

extern "C" int chx_laser_kick(const void* x, const void* energy, const void* amplitude, const void* wavelength, const void* phase,
                              const void* laser_sigma, const void* offset_x, const void* offset_y, const void* pulse_sigma,
                              const void* pulse_center, double mass_eV, int64_t B, int64_t Bx, int64_t Be, int64_t Ba, int64_t Bw,
                              int64_t Bp, int64_t Bs, int64_t Bx0, int64_t By0, int64_t Bps, int64_t Bpc, int64_t N, int dtype,
                              void* out, void* stream) {
    const LaserArgs s = CHX_LASER_ARGS;
    if (!laser_settings_ok(x, s, mass_eV, B, Bx, N) || !out) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!chx_aligned16(out)) return CHX_ERR_MISALIGNED;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return laser_kick_t<T>((const T*)x, s, mass_eV, B, Bx, N, (T*)out, (hipStream_t)stream);
    });
}

extern "C" int chx_laser_kick_bwd(const void* x, const void* energy, const void* amplitude, const void* wavelength, const void* phase,
                                  const void* laser_sigma, const void* offset_x, const void* offset_y, const void* pulse_sigma,
                                  const void* pulse_center, double mass_eV, int64_t B, int64_t Bx, int64_t Be, int64_t Ba,
                                  int64_t Bw, int64_t Bp, int64_t Bs, int64_t Bx0, int64_t By0, int64_t Bps, int64_t Bpc, int64_t N,
                                  int dtype, const void* d_out, void* dX, double* d_rows, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    const LaserArgs s = CHX_LASER_ARGS;
    if (!laser_settings_ok(x, s, mass_eV, B, Bx, N) || !d_out || !dX || !d_rows) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!chx_aligned16(dX)) return CHX_ERR_MISALIGNED;
    if (!workspace || workspace_bytes < chx_laser_workspace_bytes(B, N)) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return laser_kick_bwd_t<T>((const T*)x, s, mass_eV, B, Bx, N, (const T*)d_out, (T*)dX, d_rows, (double*)workspace,
                                   (hipStream_t)stream);
    });
}
