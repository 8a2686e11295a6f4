// chx_sr.hip — incoherent synchrotron radiation of a bend's arc (SynchrotronRadiationKick element): the classical energy loss and
// the quantum excitation in its Gaussian approximation, as one zero-length kick. Per batch row, from the reference energy, the arc
// length L and the bend angle theta (gamma0 = E0 / mc^2, P0 = beta0 gamma0, r_c = Z^2 r_e m_e / m, lambda_c = hbar c / mc^2):
//   a = (2/3) r_c theta^2 / L,    b = 55 / (24 sqrt 3) r_c lambda_c |theta|^3 / L^2        (both 0 where L = 0 or theta = 0)
// and per particle, in fp64 whatever the beam dtype, rounded once on the store:
//   g = gamma0 + delta P0,  pi = sqrt(g^2 - 1),  g' = g - a P0^2 pi g - sqrt(b P0^3 g^7 / pi^3) xi
//   delta' = delta + (g' - g) / P0,  pi' = sqrt(g'^2 - 1),  px' = px pi' / pi,  py' = py pi' / pi
// xi is one standard normal per (kick, call, batch row, particle): Philox4x32-10 with key (seed, stream) and counter (particle n,
// flat batch row b, call_lo, call_hi), its four words turned into two uniforms on the 53-bit grid and one Box-Muller cosine branch
// (chx_philox.h).
// The call index is read from device memory, so a captured graph follows it. Nothing of xi is stored: the backward pass draws it
// again from the same counter.
//   F. sr_kick_kernel      one workgroup per (row tile, batch row): the tile's rows through LDS (coalesced 16-byte transfers of the
//                          7-strided rows, chx_apply_tiles.h's tile shapes), a lane takes whole rows; x, y, tau and the seventh
//                          column keep their bits, and so does every column of a row with a = b = 0
//   B1. sr_kick_bwd_kernel the same pass with the cotangents' tile beside it: dX, and the workgroup's partial of the cotangents of
//                          (gamma0, a, b) (P0 = sqrt(gamma0^2 - 1) folded into gamma0's)
//   B2. sr_rows_kernel     one workgroup per batch row adds the partials in a fixed order: bitwise reproducible, no float atomics
#include "chx_apply_tiles.h"
#include "chx_philox.h"

namespace {

constexpr double kElectronRadius = 2.8179403205e-15;     // r_e, m (CODATA 2022)
constexpr double kElectronMass = 510998.95069;           // m_e c^2, eV
constexpr double kHbarC = 1.973269804593025e-7;          // hbar c, eV m
constexpr double kQuantumFactor = 55.0 / (24.0 * 1.7320508075688772);   // 55 / (24 sqrt 3)

template <typename T> struct sr_cfg { static constexpr int TP = tile_cfg<T>::PPT * CHX_BLOCK; };
// tiles per batch row of the float64 shape (the smaller tile): what the workspace is sized for in either dtype
inline int64_t sr_max_tiles(int64_t N) { return (N + sr_cfg<double>::TP - 1) / sr_cfg<double>::TP; }

struct SrKey {
    uint32_t seed, stream;
};

__device__ __forceinline__ double sr_normal(SrKey key, uint64_t call, int64_t b, int64_t n) {
    uint32_t w[4];
    philox4x32_10((uint32_t)n, (uint32_t)b, (uint32_t)call, (uint32_t)(call >> 32), key.seed, key.stream, w);
    return philox_normal_of(w);
}

// The row's factors {gamma0, P0, a, b} in fp64; beta0 as `Beam.p0c` forms it. A negative L gives NaN.
template <typename T>
__device__ __forceinline__ void sr_row_factors(const T* energy, int64_t Be, const T* length, int64_t Bl, const T* angle, int64_t Ba,
                                               double mass, double absz, bool excite, int64_t b, double* f) {
    const double e = (double)energy[Be == 1 ? 0 : b], L = (double)length[Bl == 1 ? 0 : b], th = (double)angle[Ba == 1 ? 0 : b];
    const double gamma = e / mass;
    const double beta = fabs(gamma) > 0.0 ? sqrt(fmax(1.0 - 1.0 / (gamma * gamma), 0.0)) : 1.0;
    const double rc = absz * absz * kElectronRadius * kElectronMass / mass, lc = kHbarC / mass;
    double a = 0.0, q = 0.0;
    if (L != 0.0 && th != 0.0) {
        if (L > 0.0) {
            a = (2.0 / 3.0) * rc * (th * th) / L;
            q = kQuantumFactor * rc * lc * (fabs(th) * (th * th)) / (L * L);
        } else {
            a = q = __longlong_as_double(0x7ff8000000000000LL);
        }
    }
    f[0] = gamma;
    f[1] = beta * gamma;
    f[2] = a;
    f[3] = excite ? q : 0.0;
}

struct SrParticle {
    double g, pi, A, S, g1, pi1, ratio;   // A: the loss a P0^2 pi g; S: the rms sqrt(b P0^3 g^7 / pi^3), 0 without excitation
    bool ok;                              // finite coordinates and g' > 1: otherwise delta', px', py' are NaN
};

__device__ __forceinline__ SrParticle sr_particle(double delta, double px, double py, double gamma0, double P0, double a, double q,
                                                  double xi) {
    SrParticle s;
    s.g = gamma0 + delta * P0;
    s.pi = sqrt(s.g * s.g - 1.0);
    s.A = a * (P0 * P0) * s.pi * s.g;
    s.g1 = s.g - s.A;
    s.S = 0.0;
    if (q != 0.0) {
        const double g2 = s.g * s.g, g4 = g2 * g2;
        s.S = sqrt(q * (P0 * P0 * P0) * (g4 * g2 * s.g) / (s.pi * s.pi * s.pi));
        s.g1 -= s.S * xi;
    }
    s.pi1 = sqrt(s.g1 * s.g1 - 1.0);
    s.ratio = s.pi1 / s.pi;
    s.ok = isfinite(delta) && isfinite(px) && isfinite(py) && s.g1 > 1.0 && isfinite(s.g1) && isfinite(s.ratio);
    return s;
}

// ---- F ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void sr_kick_kernel(const T* __restrict__ x, const T* __restrict__ energy, int64_t Be,
                                                            const T* __restrict__ length, int64_t Bl, const T* __restrict__ angle,
                                                            int64_t Ba, double mass, double absz, int excite, SrKey key,
                                                            const int64_t* __restrict__ call_index, int64_t B, int64_t Bx, int64_t N,
                                                            T* __restrict__ out, int in_vec_ok) {
    constexpr int TP = sr_cfg<T>::TP, PPT = tile_cfg<T>::PPT;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    __shared__ double row[4];
    const int64_t b = blockIdx.y, n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const T* gin = x + (in_row * N + n0) * 7;
    T* gout = out + (b * N + n0) * 7;
    const bool in_vec = CHX_TILE_VEC_OK(T, in_vec_ok, in_row, N), out_vec = CHX_TILE_VEC_OK(T, 1, b, N);
    if (threadIdx.x == 0) sr_row_factors(energy, Be, length, Bl, angle, Ba, mass, absz, excite != 0, b, row);
    tile_load<T, TP>(gin, lds, np * 7, in_vec, !(Bx == 1 && B > 1));
    __syncthreads();
    const double gamma0 = row[0], P0 = row[1], a = row[2], q = row[3];
    if (a != 0.0 || q != 0.0) {                                    // NaN factors included; a row of zeros keeps every bit
        const uint64_t call = q != 0.0 ? (uint64_t)call_index[0] : 0ull;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int p = threadIdx.x + k * CHX_BLOCK;
            if (p < np) {
                const double px = (double)lds[p * 7 + 1], py = (double)lds[p * 7 + 3], delta = (double)lds[p * 7 + 5];
                const double xi = q != 0.0 ? sr_normal(key, call, b, n0 + p) : 0.0;
                const SrParticle s = sr_particle(delta, px, py, gamma0, P0, a, q, xi);
                const double nan = __longlong_as_double(0x7ff8000000000000LL);
                lds[p * 7 + 1] = (T)(s.ok ? px * s.ratio : nan);
                lds[p * 7 + 3] = (T)(s.ok ? py * s.ratio : nan);
                lds[p * 7 + 5] = (T)(s.ok ? delta + (s.g1 - s.g) / P0 : nan);
            }
        }
    }
    __syncthreads();
    tile_store<T, TP>(gout, lds, np * 7, out_vec, true);
}

// ---- B1 --------------------------------------------------------------------------------------------------------------------------
// With G the cotangents of (px', py', delta') and r = pi' / pi: G_r = G_px' px + G_py' py; G_g' = G_r g' / (pi pi') + G_delta' / P0;
// G_pi = -G_r r / pi - G_g' (a P0^2 g - (3/2) S xi / pi); G_g = G_g' (1 - a P0^2 pi - (7/2) S xi / g) - G_delta' / P0 + G_pi g / pi;
// d(px) = G_px' r, d(py) = G_py' r, d(delta) = G_delta' + G_g P0; the row's cotangents sum G_a = -G_g' P0^2 pi g,
// G_b = -G_g' xi S / (2 b), G_P0 = -G_delta' (g' - g) / P0^2 - G_g' (2 a P0 pi g + (3/2) S xi / P0) + G_g delta and
// G_gamma0 = G_g + G_P0 gamma0 / P0. A particle whose output is NaN has no gradient and adds nothing.
template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void sr_kick_bwd_kernel(const T* __restrict__ x, const T* __restrict__ energy, int64_t Be,
                                                                const T* __restrict__ length, int64_t Bl,
                                                                const T* __restrict__ angle, int64_t Ba, double mass, double absz,
                                                                int excite, SrKey key, const int64_t* __restrict__ call_index,
                                                                int64_t B, int64_t Bx, int64_t N, const T* __restrict__ gout,
                                                                T* __restrict__ dX, double* __restrict__ partials, int64_t max_tiles,
                                                                int in_vec_ok, int g_vec_ok) {
    constexpr int TP = sr_cfg<T>::TP, PPT = tile_cfg<T>::PPT;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    __shared__ __attribute__((aligned(16))) T gl[TP * 7];
    __shared__ double row[4];
    __shared__ double red[4 * 3];
    const int64_t b = blockIdx.y, n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const bool in_vec = CHX_TILE_VEC_OK(T, in_vec_ok, in_row, N), g_vec = CHX_TILE_VEC_OK(T, g_vec_ok, b, N),
               out_vec = CHX_TILE_VEC_OK(T, 1, b, N);
    if (threadIdx.x == 0) sr_row_factors(energy, Be, length, Bl, angle, Ba, mass, absz, excite != 0, b, row);
    tile_load<T, TP>(x + (in_row * N + n0) * 7, lds, np * 7, in_vec, !(Bx == 1 && B > 1));
    tile_load<T, TP>(gout + (b * N + n0) * 7, gl, np * 7, g_vec, true);
    __syncthreads();
    const double gamma0 = row[0], P0 = row[1], a = row[2], q = row[3];
    const uint64_t call = q != 0.0 ? (uint64_t)call_index[0] : 0ull;
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = threadIdx.x + k * CHX_BLOCK;
        if (p < np) {
            const double px = (double)lds[p * 7 + 1], py = (double)lds[p * 7 + 3], delta = (double)lds[p * 7 + 5];
            const double Gpx = (double)gl[p * 7 + 1], Gpy = (double)gl[p * 7 + 3], Gd = (double)gl[p * 7 + 5];
            const double xi = q != 0.0 ? sr_normal(key, call, b, n0 + p) : 0.0;
            const SrParticle s = sr_particle(delta, px, py, gamma0, P0, a, q, xi);
            double dpx = 0.0, dpy = 0.0, dd = 0.0;
            if (s.ok) {
                const double Sxi = s.S * xi;
                const double Gr = Gpx * px + Gpy * py;
                const double Gg1 = Gr * s.g1 / (s.pi * s.pi1) + Gd / P0;
                const double Gpi = -Gr * s.ratio / s.pi - Gg1 * (a * (P0 * P0) * s.g - 1.5 * Sxi / s.pi);
                const double Gg = Gg1 * (1.0 - a * (P0 * P0) * s.pi - 3.5 * Sxi / s.g) - Gd / P0 + Gpi * s.g / s.pi;
                const double GP0 = -Gd * (s.g1 - s.g) / (P0 * P0) - Gg1 * (2.0 * a * P0 * s.pi * s.g + 1.5 * Sxi / P0) + Gg * delta;
                dpx = Gpx * s.ratio;
                dpy = Gpy * s.ratio;
                dd = Gd + Gg * P0;
                acc[0] += Gg + GP0 * gamma0 / P0;
                acc[1] -= Gg1 * (P0 * P0) * s.pi * s.g;
                if (q != 0.0) acc[2] -= Gg1 * Sxi / (2.0 * q);
            }
            gl[p * 7 + 1] = (T)dpx;
            gl[p * 7 + 3] = (T)dpy;
            gl[p * 7 + 5] = (T)dd;
        }
    }
    chx_block_sum<3>(acc, red);                                   // its barriers also order the tile's writes before the store
    if (threadIdx.x == 0) {
        double* dst = partials + (b * max_tiles + blockIdx.x) * 3;
        dst[0] = acc[0]; dst[1] = acc[1]; dst[2] = acc[2];
    }
    tile_store<T, TP>(dX + (b * N + n0) * 7, gl, np * 7, out_vec, true);
}

// ---- B2: thread t adds the partials t, t + 256, ... of its row in order, then the workgroup's fixed tree ---------------------------
__global__ __launch_bounds__(CHX_BLOCK) void sr_rows_kernel(const double* __restrict__ partials, int64_t max_tiles, int64_t tiles,
                                                            double* __restrict__ d_gamma, double* __restrict__ d_a,
                                                            double* __restrict__ d_b) {
    __shared__ double red[4 * 3];
    const int64_t b = blockIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t t = threadIdx.x; t < tiles; t += CHX_BLOCK) {
        const double* src = partials + (b * max_tiles + t) * 3;
        acc[0] += src[0]; acc[1] += src[1]; acc[2] += src[2];
    }
    chx_block_sum<3>(acc, red);
    if (threadIdx.x == 0) {
        d_gamma[b] = acc[0]; d_a[b] = acc[1]; d_b[b] = acc[2];
    }
}

// ---- the draw itself -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CHX_BLOCK) void sr_normals_kernel(SrKey key, uint64_t call, int64_t N, uint32_t* __restrict__ words,
                                                               double* __restrict__ xi) {
    const int64_t b = blockIdx.y, n = (int64_t)blockIdx.x * CHX_BLOCK + threadIdx.x;
    if (n >= N) return;
    uint32_t w[4];
    philox4x32_10((uint32_t)n, (uint32_t)b, (uint32_t)call, (uint32_t)(call >> 32), key.seed, key.stream, w);
    uint4* dst = reinterpret_cast<uint4*>(words) + (b * N + n);
    *dst = make_uint4(w[0], w[1], w[2], w[3]);
    xi[b * N + n] = philox_normal_of(w);
}

// B rows are grid.y and the particle index is a 32-bit counter word
bool sr_shape_ok(int64_t B, int64_t N) { return B >= 1 && B <= 65535 && N >= 1 && N <= 0xffffffffLL; }

bool sr_settings_ok(const void* x, const void* energy, const void* length, const void* angle, double mass, const void* call_index,
                    int64_t B, int64_t Bx, int64_t Be, int64_t Bl, int64_t Ba, int64_t N) {
    return sr_shape_ok(B, N) && x && energy && length && angle && call_index && mass > 0.0 && chx_bcast_ok(Bx, B) &&
           chx_bcast_ok(Be, B) && chx_bcast_ok(Bl, B) && chx_bcast_ok(Ba, B);
}

template <typename T>
dim3 sr_grid(int64_t B, int64_t N) { return dim3((unsigned)((N + sr_cfg<T>::TP - 1) / sr_cfg<T>::TP), (unsigned)B); }

template <typename T>
int sr_kick_t(const T* x, const T* energy, const T* length, const T* angle, double mass, double absz, int excite, SrKey key,
              const int64_t* call_index, int64_t B, int64_t Bx, int64_t Be, int64_t Bl, int64_t Ba, int64_t N, T* out, hipStream_t s) {
    hipLaunchKernelGGL(sr_kick_kernel<T>, sr_grid<T>(B, N), dim3(CHX_BLOCK), 0, s, x, energy, Be, length, Bl, angle, Ba, mass, absz,
                       excite, key, call_index, B, Bx, N, out, (int)chx_aligned16(x));
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

template <typename T>
int sr_kick_bwd_t(const T* x, const T* energy, const T* length, const T* angle, double mass, double absz, int excite, SrKey key,
                  const int64_t* call_index, int64_t B, int64_t Bx, int64_t Be, int64_t Bl, int64_t Ba, int64_t N, const T* gout,
                  T* dX, double* d_gamma, double* d_a, double* d_b, double* partials, hipStream_t s) {
    const dim3 grid = sr_grid<T>(B, N);
    const int64_t max_tiles = sr_max_tiles(N);
    hipLaunchKernelGGL(sr_kick_bwd_kernel<T>, grid, dim3(CHX_BLOCK), 0, s, x, energy, Be, length, Bl, angle, Ba, mass, absz, excite,
                       key, call_index, B, Bx, N, gout, dX, partials, max_tiles, (int)chx_aligned16(x), (int)chx_aligned16(gout));
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(sr_rows_kernel, dim3((unsigned)B), dim3(CHX_BLOCK), 0, s, partials, max_tiles, (int64_t)grid.x, d_gamma, d_a,
                       d_b);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace

extern "C" size_t chx_sr_workspace_bytes(int64_t B, int64_t N) {
    return sr_shape_ok(B, N) ? (size_t)(B * sr_max_tiles(N)) * 3 * sizeof(double) : 0;
}

extern "C" int chx_sr_kick(const void* x, const void* energy, const void* length, const void* angle, double mass_eV,
                           double abs_charge, int quantum_excitation, uint32_t seed, uint32_t rng_stream, const int64_t* call_index,
                           int64_t B, int64_t Bx, int64_t Be, int64_t Bl, int64_t Ba, int64_t N, int dtype, void* out, void* stream) {
    if (!sr_settings_ok(x, energy, length, angle, mass_eV, call_index, B, Bx, Be, Bl, Ba, N) || !out) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!chx_aligned16(out)) return CHX_ERR_MISALIGNED;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return sr_kick_t<T>((const T*)x, (const T*)energy, (const T*)length, (const T*)angle, mass_eV, abs_charge, quantum_excitation,
                            SrKey{seed, rng_stream}, call_index, B, Bx, Be, Bl, Ba, N, (T*)out, (hipStream_t)stream);
    });
}

extern "C" int chx_sr_kick_bwd(const void* x, const void* energy, const void* length, const void* angle, double mass_eV,
                               double abs_charge, int quantum_excitation, uint32_t seed, uint32_t rng_stream,
                               const int64_t* call_index, int64_t B, int64_t Bx, int64_t Be, int64_t Bl, int64_t Ba, int64_t N,
                               int dtype, const void* d_out, void* dX, double* d_gamma, double* d_a, double* d_b, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!sr_settings_ok(x, energy, length, angle, mass_eV, call_index, B, Bx, Be, Bl, Ba, N) || !d_out || !dX || !d_gamma || !d_a ||
        !d_b)
        return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!chx_aligned16(dX)) return CHX_ERR_MISALIGNED;
    if (!workspace || workspace_bytes < chx_sr_workspace_bytes(B, N)) return CHX_ERR_WORKSPACE;
    return dispatch_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return sr_kick_bwd_t<T>((const T*)x, (const T*)energy, (const T*)length, (const T*)angle, mass_eV, abs_charge,
                                quantum_excitation, SrKey{seed, rng_stream}, call_index, B, Bx, Be, Bl, Ba, N, (const T*)d_out,
                                (T*)dX, d_gamma, d_a, d_b, (double*)workspace, (hipStream_t)stream);
    });
}

extern "C" int chx_sr_normals(uint32_t seed, uint32_t rng_stream, uint64_t call, int64_t B, int64_t N, uint32_t* words_out,
                              double* xi_out, void* stream) {
    if (!sr_shape_ok(B, N) || !words_out || !xi_out) return CHX_ERR_INVALID_ARG;
    if (!chx_aligned16(words_out)) return CHX_ERR_MISALIGNED;
    hipLaunchKernelGGL(sr_normals_kernel, dim3((unsigned)((N + CHX_BLOCK - 1) / CHX_BLOCK), (unsigned)B), dim3(CHX_BLOCK), 0,
                       (hipStream_t)stream, SrKey{seed, rng_stream}, call, N, words_out, xi_out);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}
