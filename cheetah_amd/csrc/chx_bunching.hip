// chx_bunching.hip — the bunching factor of a particle beam (ParticleBeam.bunching_factor): for every spatial frequency nu_k
// (turns per metre) F_k = sum_i a_i exp(-2 pi i nu_k tau_i) and Q = sum_i a_i, a_i = q_i w_i. A direct sum over N x K pairs:
// 8-16 bytes per particle read once per frequency tile, everything else arithmetic.
//
// Forward (bunching_partial_kernel): lanes own frequencies, particles are wave-uniform. A workgroup takes one (chunk of kChunk
// particles, tile of kKTile frequencies, batch row): it stages (tau, a) of the chunk in LDS as fp64 (tau replaced by 0 where
// a == 0: the select that keeps a lost particle's NaN out), each of its 4 waves walks its own quarter of the chunk (an LDS
// broadcast read per particle) and every lane keeps the running (re, im) of kKU frequencies in registers — one fma chain per
// frequency and wave, no cross-lane reduction. The 4 waves are added in order, the chunk's partial sums go to the workspace, and
// bunching_merge_kernel adds the chunks in a fixed order (wave w of a merging workgroup takes the chunks c = w mod 4 in
// increasing order, then the 4 waves in order) and forms Q likewise. Appending particles without weight adds only zeros to
// every one of these sums: the result keeps its bits.
// Backward (bunching_bwd_kernel): the transpose. Lanes own particles, nu_k and the cotangents are wave-uniform (scalar loads),
// every particle sums over K; no reduction.
//
// Phase: t = nu * tau in fp64 (turns), f = t - rint(t) exactly, |f| <= 1/2. A float32 beam evaluates sin, cos of 2 pi f with
// turn_sincos_f32 below (absolute error <= 2.5 * 2^-24, derived there and in DESIGN.md); a float64 beam with sincospi.
// -ffp-contract=off: every fma is written out.
#include "chx_common.h"

namespace {

constexpr int kChunk = CHX_BUNCHING_CHUNK;
constexpr int kSub = kChunk / 4;              // particles per wave
constexpr int kKU = 4;                        // frequencies per lane
constexpr int kKTile = 64 * kKU;
static_assert(kKTile == CHX_BUNCHING_K_TILE, "the frequency tile of include/chx.h");
static_assert(kChunk % CHX_BLOCK == 0 && 4 * kKTile * 2 <= kChunk * 2, "the wave partials reuse the staging buffer");
constexpr double kTwoPi = 6.283185307179586;

inline int64_t nchunks(int64_t N) { return (N + kChunk - 1) / kChunk; }
inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// sin(2 pi x), cos(2 pi x) for |x| <= 1/2 turn in float32. j = rint(4 x) picks the quadrant, y = x - j / 4 is exact (4 x, its
// rounding to an integer and the difference of two floats within a factor 2 of each other carry no rounding), |y| <= 1/8, and
// with z = y y the Taylor polynomials of sin(2 pi y) / y (through y^8) and cos(2 pi y) (through y^10) are run as fma chains.
// Error, u = 2^-24, |2 pi y| <= pi / 4, z <= 1/64:
//   sin: P = S0 + z p1, |p1| <= 41.4, P in [5.65, 6.29]. Relative to P: the last fma u, S0 as a float u, and three errors of
//        size u |p1 z| <= 0.647 u (p1's own rounding, the rounding of z, S1 as a float), 0.115 u each; everything deeper is
//        scaled by z^2 <= 2.5e-4 |S2| / P < 0.004 per rounding, < 0.02 u in all; y P rounds once more: (1 + 1 + 0.345 + 0.02 + 1) u
//        = 3.4 u of |sin| <= 0.7072, plus the series' remainder (pi/4)^11 / 11! = 1.8e-9 = 0.03 u: <= 2.45 u absolute.
//   cos: C = 1 + z p1, |p1| <= 19.74, C in [0.707, 1]: the last fma u / 2 (half an ulp below 1), three errors of size
//        u |p1 z| <= 0.309 u, deeper terms (|p2| z^2 <= 0.016 per rounding) < 0.06 u, remainder (pi/4)^12 / 12! = 1.2e-10:
//        <= 1.5 u absolute.
// Swapping and negating by quadrant is exact. Both within 2.5 * 2^-24 (E_SC of tests/test_gpu_bunching_factor.py).
__device__ __forceinline__ void turn_sincos_f32(float x, float& s, float& c) {
    const float j = __builtin_rintf(4.0f * x);
    const float y = __builtin_fmaf(j, -0.25f, x);
    const float z = y * y;
    float p = __builtin_fmaf(42.058693944897634f, z, -76.70585975306136f);
    p = __builtin_fmaf(p, z, 81.60524927607504f);
    p = __builtin_fmaf(p, z, -41.341702240399755f);
    p = __builtin_fmaf(p, z, 6.283185307179586f);
    const float sy = y * p;
    float r = __builtin_fmaf(-26.426256783374388f, z, 60.24464137187664f);
    r = __builtin_fmaf(r, z, -85.45681720669371f);
    r = __builtin_fmaf(r, z, 64.93939402266828f);
    r = __builtin_fmaf(r, z, -19.739208802178716f);
    const float cy = __builtin_fmaf(r, z, 1.0f);
    // angle = j quarter turns + 2 pi y, j in -2..2: j odd swaps sin and cos, the signs follow the quadrant
    const int ji = (int)j;
    const bool odd = ji & 1;
    const float ss = odd ? cy : sy, cc = odd ? sy : cy;
    const int q = ji & 3;                       // 0, 1, 2, 3 (-1 -> 3, -2 -> 2)
    s = (q == 2 || q == 3) ? -ss : ss;
    c = (q == 1 || q == 2) ? -cc : cc;
}

// sin, cos of 2 pi t for a phase t in turns (fp64), evaluated in the precision of the beam
template <typename T>
__device__ __forceinline__ void phase_sincos(double t, double& s, double& c) {
    const double f = t - __builtin_rint(t);
    if constexpr (sizeof(T) == 4) {
        float sf, cf;
        turn_sincos_f32((float)f, sf, cf);
        s = (double)sf;
        c = (double)cf;
    } else {
        sincospi(2.0 * f, &s, &c);
    }
}

// the fma chains of one wave over `cnt` staged particles, NU (wave-uniform) of the lane's kKU frequencies in use
template <typename T, int NU>
__device__ __forceinline__ void accumulate(const double2* __restrict__ sp, int cnt, const double (&nuv)[kKU], double (&re)[kKU],
                                           double (&im)[kKU]) {
    for (int i = 0; i < cnt; ++i) {
        const double2 ta = sp[i];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            double s, c;
            phase_sincos<T>(nuv[u] * ta.x, s, c);
            re[u] = __builtin_fma(ta.y, c, re[u]);
            im[u] = __builtin_fma(-ta.y, s, im[u]);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void bunching_partial_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                                    const T* __restrict__ q, const double* __restrict__ nu,
                                                                    int64_t Bx, int64_t Bw, int64_t Bq, int64_t Bnu, int64_t N,
                                                                    int64_t K, int64_t nchunk, double* __restrict__ part,
                                                                    double* __restrict__ qpart) {
    __shared__ double2 stage[kChunk];           // (tau, a) of the chunk; afterwards the 4 waves' partial sums
    __shared__ double red[4];
    const int64_t chunk = blockIdx.x, kt = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (uniform: a scalar loop count)
    const T* __restrict__ xb = x + (Bx == 1 ? 0 : b) * N * 7;
    const T* __restrict__ wb = w ? w + (Bw == 1 ? 0 : b) * N : nullptr;
    const T* __restrict__ qb = q ? q + (Bq == 1 ? 0 : b) * N : nullptr;
    const int64_t n0 = chunk * kChunk;
    double qa[1] = {0.0};
#pragma unroll
    for (int j = 0; j < kChunk / CHX_BLOCK; ++j) {
        const int i = threadIdx.x + j * CHX_BLOCK;
        const int64_t n = n0 + i;
        double tau = 0.0, a = 0.0;
        if (n < N) {
            a = (wb ? (double)wb[n] : 1.0) * (qb ? (double)qb[n] : 1.0);
            const double tv = (double)xb[n * 7 + 4];
            tau = a == 0.0 ? 0.0 : tv;           // a particle without weight contributes a * (cos 0, sin 0) = exactly 0
        }
        stage[i] = make_double2(tau, a);
        qa[0] += a;
    }
    chx_block_sum<1>(qa, red);                   // (its barriers also publish the staged chunk)
    if (kt == 0 && threadIdx.x == 0) qpart[b * nchunk + chunk] = qa[0];

    const int64_t k0 = kt * kKTile;
    const double* __restrict__ nub = nu + (Bnu == 1 ? 0 : b) * K;
    double nuv[kKU], re[kKU], im[kKU];
#pragma unroll
    for (int u = 0; u < kKU; ++u) {
        const int64_t k = k0 + 64 * u + lane;
        nuv[u] = k < K ? nub[k] : 0.0;
        re[u] = 0.0;
        im[u] = 0.0;
    }
    const int64_t left = N - n0 - (int64_t)wave * kSub;                 // particles of this wave's quarter
    const int cnt = left < 0 ? 0 : (left > kSub ? kSub : (int)left);
    const int64_t kleft = K - k0;
    const int nu_act = kleft >= kKTile ? kKU : (int)((kleft + 63) / 64);
    const double2* sp = stage + wave * kSub;
    switch (nu_act) {                                                    // (wave-uniform)
        case 1: accumulate<T, 1>(sp, cnt, nuv, re, im); break;
        case 2: accumulate<T, 2>(sp, cnt, nuv, re, im); break;
        case 3: accumulate<T, 3>(sp, cnt, nuv, re, im); break;
        default: accumulate<T, 4>(sp, cnt, nuv, re, im); break;
    }
    __syncthreads();                              // every wave has read its quarter: the staging buffer is free
    double2* m = stage;                           // [wave][kKTile]
#pragma unroll
    for (int u = 0; u < kKU; ++u) m[wave * kKTile + 64 * u + lane] = make_double2(re[u], im[u]);
    __syncthreads();
    const int64_t k = k0 + threadIdx.x;
    if (k < K) {
        const double2 p0 = m[threadIdx.x], p1 = m[kKTile + threadIdx.x], p2 = m[2 * kKTile + threadIdx.x],
                      p3 = m[3 * kKTile + threadIdx.x];
        double2* o = reinterpret_cast<double2*>(part) + (b * nchunk + chunk) * K + k;
        *o = make_double2(((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y);
    }
}

// grid (ceil(K / 64) + 1, B): workgroup j < ceil(K / 64) merges 64 frequencies — wave w adds the chunks c = w, w + 4, ... in
// order, then the waves are added in order; the last workgroup of a row forms Q from the chunks' weight sums
__global__ __launch_bounds__(CHX_BLOCK) void bunching_merge_kernel(const double* __restrict__ part, const double* __restrict__ qpart,
                                                                  int64_t K, int64_t nchunk, double* __restrict__ F,
                                                                  double* __restrict__ Q) {
    __shared__ double2 m[CHX_BLOCK];
    __shared__ double red[4];
    const int64_t b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == gridDim.x - 1) {
        double s[1] = {0.0};
        for (int64_t c = threadIdx.x; c < nchunk; c += CHX_BLOCK) s[0] += qpart[b * nchunk + c];
        chx_block_sum<1>(s, red);
        if (threadIdx.x == 0) Q[b] = s[0];
        return;
    }
    const int64_t k = (int64_t)blockIdx.x * 64 + lane;
    double re = 0.0, im = 0.0;
    if (k < K) {
        const double2* __restrict__ p = reinterpret_cast<const double2*>(part) + b * nchunk * K + k;
#pragma unroll 4
        for (int64_t c = wave; c < nchunk; c += 4) {
            const double2 v = p[c * K];
            re += v.x;
            im += v.y;
        }
    }
    m[threadIdx.x] = make_double2(re, im);
    __syncthreads();
    if (wave == 0 && k < K) {
        const double2 p0 = m[lane], p1 = m[64 + lane], p2 = m[128 + lane], p3 = m[192 + lane];
        reinterpret_cast<double2*>(F)[b * K + k] = make_double2(((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y);
    }
}

template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void bunching_bwd_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ q,
                                                                const double* __restrict__ nu, int64_t Bx, int64_t Bw, int64_t Bq,
                                                                int64_t Bnu, int64_t N, int64_t K, const double* __restrict__ dF,
                                                                const double* __restrict__ dQ, T* __restrict__ dTau,
                                                                T* __restrict__ dW, T* __restrict__ dQpart) {
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * CHX_BLOCK + threadIdx.x;
    if (n >= N) return;
    const double wv = w ? (double)w[(Bw == 1 ? 0 : b) * N + n] : 1.0;
    const double qv = q ? (double)q[(Bq == 1 ? 0 : b) * N + n] : 1.0;
    const double a = wv * qv;
    const double tv = (double)x[((Bx == 1 ? 0 : b) * N + n) * 7 + 4];
    const bool lost = a == 0.0 && !(__builtin_fabs(tv) <= 1.79769313486231570815e308);   // no weight and no position
    const double tau = lost ? 0.0 : tv;
    double st = 0.0, sa = 0.0;
    if (dF) {
        const double* __restrict__ nub = nu + (Bnu == 1 ? 0 : b) * K;
        const double2* __restrict__ g = reinterpret_cast<const double2*>(dF) + b * K;
        for (int64_t k = 0; k < K; ++k) {
            const double nk = nub[k];
            const double2 gk = g[k];
            double s, c;
            phase_sincos<T>(nk * tau, s, c);
            const double u = __builtin_fma(-gk.y, c, -(gk.x * s));
            st = __builtin_fma(nk, u, st);
            sa = __builtin_fma(gk.x, c, sa);
            sa = __builtin_fma(-gk.y, s, sa);
        }
    }
    const double da = (lost ? 0.0 : sa) + (dQ ? dQ[b] : 0.0);
    if (dTau) dTau[b * N + n] = a == 0.0 ? (T)0 : (T)(a * (kTwoPi * st));
    if (dW) dW[b * N + n] = (T)(da * qv);
    if (dQpart) dQpart[b * N + n] = (T)(da * wv);
}

int check_bunching(const void* x, const void* nu, int64_t B, int64_t Bx, int64_t Bw, int64_t Bq, int64_t Bnu, int64_t N, int64_t K,
                   int dtype) {
    if (!x || !nu || B < 1 || B > 65535 || N < 1 || N > 0x7fffffffLL || K < 1 || K > CHX_BUNCHING_K_MAX) return CHX_ERR_INVALID_ARG;
    if (!chx_bcast_ok(Bx, B) || !chx_bcast_ok(Bw, B) || !chx_bcast_ok(Bq, B) || !chx_bcast_ok(Bnu, B)) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    return CHX_OK;
}

struct BunchWs {
    double* part;    // [B][nchunk][K][2]
    double* qpart;   // [B][nchunk]
    size_t bytes;
};

BunchWs bunch_ws(void* base, int64_t B, int64_t N, int64_t K) {
    BunchWs w;
    char* p = (char*)base;
    const size_t npart = al256((size_t)B * (size_t)nchunks(N) * (size_t)K * 16);
    w.part = (double*)p;
    w.qpart = (double*)(p ? p + npart : nullptr);
    w.bytes = npart + al256((size_t)B * (size_t)nchunks(N) * 8);
    return w;
}

template <typename T>
int bunching_t(const T* x, const T* w, const T* q, const double* nu, int64_t B, int64_t Bx, int64_t Bw, int64_t Bq, int64_t Bnu,
               int64_t N, int64_t K, double* F, double* Q, const BunchWs& ws, hipStream_t s) {
    const int64_t nc = nchunks(N);
    hipLaunchKernelGGL(bunching_partial_kernel<T>, dim3((unsigned)nc, (unsigned)((K + kKTile - 1) / kKTile), (unsigned)B),
                       dim3(CHX_BLOCK), 0, s, x, w, q, nu, Bx, Bw, Bq, Bnu, N, K, nc, ws.part, ws.qpart);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(bunching_merge_kernel, dim3((unsigned)((K + 63) / 64 + 1), (unsigned)B), dim3(CHX_BLOCK), 0, s, ws.part,
                       ws.qpart, K, nc, F, Q);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace

extern "C" size_t chx_bunching_workspace_bytes(int64_t B, int64_t N, int64_t K) {
    if (B < 1 || B > 65535 || N < 1 || N > 0x7fffffffLL || K < 1 || K > CHX_BUNCHING_K_MAX) return 0;
    return bunch_ws(nullptr, B, N, K).bytes;
}

extern "C" int chx_bunching(const void* x, const void* w, const void* q, const double* nu, int64_t B, int64_t Bx, int64_t Bw,
                            int64_t Bq, int64_t Bnu, int64_t N, int64_t K, int dtype, double* F, double* Q, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!w) Bw = 1;
    if (!q) Bq = 1;
    int st = check_bunching(x, nu, B, Bx, Bw, Bq, Bnu, N, K, dtype);
    if (st != CHX_OK) return st;
    if (!F || !Q) return CHX_ERR_INVALID_ARG;
    const BunchWs ws = bunch_ws(workspace, B, N, K);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CHX_F32)
        return bunching_t<float>((const float*)x, (const float*)w, (const float*)q, nu, B, Bx, Bw, Bq, Bnu, N, K, F, Q, ws, s);
    return bunching_t<double>((const double*)x, (const double*)w, (const double*)q, nu, B, Bx, Bw, Bq, Bnu, N, K, F, Q, ws, s);
}

extern "C" int chx_bunching_bwd(const void* x, const void* w, const void* q, const double* nu, int64_t B, int64_t Bx, int64_t Bw,
                                int64_t Bq, int64_t Bnu, int64_t N, int64_t K, int dtype, const double* dF, const double* dQ,
                                void* dTau, void* dW, void* dQpart, void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace;
    (void)workspace_bytes;
    if (!w) Bw = 1;
    if (!q) Bq = 1;
    int st = check_bunching(x, nu, B, Bx, Bw, Bq, Bnu, N, K, dtype);
    if (st != CHX_OK) return st;
    if (!dF && !dQ) return CHX_ERR_INVALID_ARG;
    if (!dTau && !dW && !dQpart) return CHX_OK;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + CHX_BLOCK - 1) / CHX_BLOCK), (unsigned)B);
    if (dtype == CHX_F32)
        hipLaunchKernelGGL(bunching_bwd_kernel<float>, grid, dim3(CHX_BLOCK), 0, s, (const float*)x, (const float*)w, (const float*)q,
                           nu, Bx, Bw, Bq, Bnu, N, K, dF, dQ, (float*)dTau, (float*)dW, (float*)dQpart);
    else
        hipLaunchKernelGGL(bunching_bwd_kernel<double>, grid, dim3(CHX_BLOCK), 0, s, (const double*)x, (const double*)w,
                           (const double*)q, nu, Bx, Bw, Bq, Bnu, N, K, dF, dQ, (double*)dTau, (double*)dW, (double*)dQpart);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}
