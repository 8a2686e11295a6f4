// chx_slices.hip — slice statistics of a particle beam (ParticleBeam.slice_statistics): for every interval [e_k, e_k+1) of tau,
// the survival-weighted moments of chx_moments (W, W2, mu[6], unbiased cov[21]) and the charge sum q w of its particles.
//
// Membership is torch.histogram's with explicit edges (hist_bin, chx_cic_dev.h): tau outside [e_0, e_S] or NaN is in no slice,
// tau == e_S is in the last one. Everything is accumulated in fp64 without float atomics (bitwise reproducible):
//   1. slice_rank_kernel    one wave per tile of kSliceTile particles: the slice of every particle and its rank among the
//                           tile's earlier particles of that slice (ballot multisplit + per-wave LDS counters), the tile's
//                           per-slice counts -> off[b][k][tile]
//   2. slice_scan_kernel    one wave per slice: exclusive scan of its counts over the tiles
//   3. slice_start_kernel   one workgroup per row: slice starts and piece starts (a piece = kPiece consecutive particles of a slice)
//   4. slice_scatter_kernel idx[start_k + off + rank] = n: a stable counting sort — every slice is a contiguous range in the
//                           particles' original order
//   5. slice_piece_kernel   one workgroup per piece: W, W2, Σ q w, the mean and the CENTRED second moments of its particles
//   6. slice_finalize_kernel one thread per slice: the pieces merged in order with chx_merge_moments' arithmetic
// The backward pass is one sweep over the particles (slice_bwd_kernel) after a per-slice coefficient table (slice_bwd_table_kernel):
// a particle in slice k gets moments_bwd_kernel's gradient with that slice's moments and cotangent, plus the charge terms.
#include "chx_common.h"
#include "chx_cic_dev.h"

namespace {

constexpr int kSliceTile = 1024;              // particles per wave-tile of the ranking pass (16 per lane, all loaded up front)
constexpr int kSliceTileU = kSliceTile / 64;
constexpr int kPiece = 1024;                  // particles per piece of the reductions (4 per thread)
constexpr int kPieceU = kPiece / CHX_BLOCK;
constexpr int kSP = 30;                       // piece partials: W, W2, mean[6], centred M2[21], Q
constexpr int kTab = 40;                      // backward table: flag, mu[6], A[6], H[21], C0, C1, (4 unused), gq
constexpr uint32_t kNoSlice = 0xffffffffu;

inline int64_t ntiles(int64_t N) { return (N + kSliceTile - 1) / kSliceTile; }
inline int64_t npieces_max(int64_t N, int S) { return (N + kPiece - 1) / kPiece + S; }
__host__ __device__ inline size_t edge_lds_bytes(int S, size_t tsize) { return (((size_t)(S + 1) * tsize) + 15) & ~(size_t)15; }
inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

struct SliceWs {
    uint32_t* packed;   // [B][N] (slice << 16) | rank in tile, kNoSlice outside
    int* off;           // [B][S][ntile] counts, then their exclusive scan over the tiles
    int* totals;        // [B][S]
    int* start;         // [B][S + 1] first sorted position of every slice
    int* pstart;        // [B][S + 1] first piece of every slice
    int* idx;           // [B][N] particle indices sorted by slice (stable)
    double* part;       // [B][npmax][kSP]
    double* tab;        // [B][S][kTab] (backward)
    size_t bytes;
};

SliceWs slice_ws(void* base, int64_t B, int64_t N, int S) {
    SliceWs w;
    char* p = (char*)base;
    size_t o = 0;
    auto take = [&](size_t nbytes) { char* r = p ? p + o : nullptr; o += al256(nbytes); return r; };
    w.packed = (uint32_t*)take((size_t)(B * N) * 4);
    w.off = (int*)take((size_t)(B * S * ntiles(N)) * 4);
    w.totals = (int*)take((size_t)(B * S) * 4);
    w.start = (int*)take((size_t)(B * (S + 1)) * 4);
    w.pstart = (int*)take((size_t)(B * (S + 1)) * 4);
    w.idx = (int*)take((size_t)(B * N) * 4);
    w.part = (double*)take((size_t)(B * npieces_max(N, S) * kSP) * 8);
    w.tab = (double*)take((size_t)(B * S * kTab) * 8);
    w.bytes = o;
    return w;
}

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(v, d, 64);
        if (lane >= d) v += y;
    }
    return v;
}

// 1. Ranking. Lanes of a round of 64 consecutive particles that share a slice find each other by `nbits` ballots over the bits
// of the slice index (a multisplit: the same cost for any number of distinct slices); a lane's rank is the tile's earlier
// count of its slice (the wave's LDS counter) plus its peers in lower lanes; the lowest peer advances the counter.
template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void slice_rank_kernel(const T* __restrict__ x, int64_t Bx, const T* __restrict__ edges,
                                                              int64_t Be, int64_t N, int S, int nbits, int64_t ntile,
                                                              uint32_t* __restrict__ packed, int* __restrict__ off) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* e = (T*)smem;
    const int64_t b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* cnt = (int*)(smem + edge_lds_bytes(S, sizeof(T))) + wave * S;
    const T* eb = edges + (Be == 1 ? 0 : b) * (S + 1);
    for (int i = threadIdx.x; i <= S; i += CHX_BLOCK) e[i] = eb[i];
    for (int i = lane; i < S; i += 64) cnt[i] = 0;
    __syncthreads();
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    if (tile >= ntile) return;                            // (whole waves; nothing below synchronises the workgroup)
    const T* __restrict__ xb = x + (Bx == 1 ? 0 : b) * N * 7;
    const int64_t n0 = tile * kSliceTile;
    T v[kSliceTileU];
#pragma unroll
    for (int u = 0; u < kSliceTileU; ++u) {
        const int64_t n = n0 + u * 64 + lane;
        v[u] = xb[(n < N ? n : n0) * 7 + 4];
    }
    const uint64_t lower = (1ull << lane) - 1ull;
#pragma unroll
    for (int u = 0; u < kSliceTileU; ++u) {
        const int64_t n = n0 + u * 64 + lane;
        const bool in = n < N;
        const int k = in ? hist_bin<T>(e, S, v[u]) : -1;
        const bool valid = k >= 0;
        uint64_t peers = __ballot(valid);
        for (int i = 0; i < nbits; ++i) {
            const bool bit = (k >> i) & 1;
            const uint64_t bb = __ballot(bit);
            peers &= bit ? bb : ~bb;
        }
        int rank = 0;
        if (valid) rank = cnt[k] + __popcll(peers & lower);
        chx_wave_sync();                                  // every lane has read its counter before the leaders advance them
        if (valid && (peers & lower) == 0) cnt[k] = rank + __popcll(peers);
        chx_wave_sync();
        if (in) packed[b * N + n] = valid ? (((uint32_t)k << 16) | (uint32_t)rank) : kNoSlice;
    }
    for (int i = lane; i < S; i += 64) off[(b * S + i) * ntile + tile] = cnt[i];
}

// 2. one wave per (slice, row): off[b][k][:] -> its exclusive scan, totals[b][k]
__global__ __launch_bounds__(CHX_BLOCK) void slice_scan_kernel(int* __restrict__ off, int S, int64_t ntile, int* __restrict__ totals) {
    const int64_t b = blockIdx.y;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= S) return;
    int* o = off + (b * S + k) * ntile;
    int carry = 0;
    for (int64_t t0 = 0; t0 < ntile; t0 += 64) {
        const int64_t t = t0 + lane;
        const int c = t < ntile ? o[t] : 0;
        const int incl = wave_incl_scan(c, lane);
        if (t < ntile) o[t] = carry + incl - c;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) totals[b * S + k] = carry;
}

// 3. one workgroup per row: start[b][k] = sum of the counts of the slices before k, pstart[b][k] the same for ceil(count / kPiece)
__global__ __launch_bounds__(CHX_BLOCK) void slice_start_kernel(const int* __restrict__ totals, int S, int* __restrict__ start,
                                                               int* __restrict__ pstart) {
    __shared__ int wsum[2][4];
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int* tb = totals + b * S;
    int* sb = start + b * (S + 1);
    int* pb = pstart + b * (S + 1);
    const int C = (S + CHX_BLOCK - 1) / CHX_BLOCK;
    const int k0 = threadIdx.x * C;
    int sc = 0, sp = 0;
    for (int i = 0; i < C; ++i) {
        const int k = k0 + i;
        if (k < S) {
            const int c = tb[k];
            sc += c;
            sp += (c + kPiece - 1) / kPiece;
        }
    }
    const int ic = wave_incl_scan(sc, lane), ip = wave_incl_scan(sp, lane);
    if (lane == 63) { wsum[0][wave] = ic; wsum[1][wave] = ip; }
    __syncthreads();
    int ec = ic - sc, ep = ip - sp;
    for (int q = 0; q < wave; ++q) { ec += wsum[0][q]; ep += wsum[1][q]; }
    for (int i = 0; i < C; ++i) {
        const int k = k0 + i;
        if (k < S) {
            sb[k] = ec;
            pb[k] = ep;
            const int c = tb[k];
            ec += c;
            ep += (c + kPiece - 1) / kPiece;
        }
    }
    if (threadIdx.x == CHX_BLOCK - 1) { sb[S] = ec; pb[S] = ep; }
}

// 4. the stable counting sort's scatter
__global__ __launch_bounds__(CHX_BLOCK) void slice_scatter_kernel(const uint32_t* __restrict__ packed, const int* __restrict__ off,
                                                                 const int* __restrict__ start, int64_t N, int S, int64_t ntile,
                                                                 int* __restrict__ idx) {
    const int64_t b = blockIdx.y;
    const int64_t n = (int64_t)blockIdx.x * CHX_BLOCK + threadIdx.x;
    if (n >= N) return;
    const uint32_t u = packed[b * N + n];
    if (u == kNoSlice) return;
    const int k = (int)(u >> 16), r = (int)(u & 0xffffu);
    const int64_t pos = (int64_t)start[b * (S + 1) + k] + off[(b * S + k) * ntile + n / kSliceTile] + r;
    if (pos >= 0 && pos < N) idx[b * N + pos] = (int)n;      // (always true: the ranks of a slice are a permutation)
}

// block-wide sums of K doubles per thread, delivered to EVERY thread (DPP row sums, one LDS exchange of the 16 row sums; fixed order)
template <int K>
__device__ __forceinline__ void block_sum_all(double (&v)[K], double* red /* [16 * K] */) {
    const int lane = threadIdx.x & 63, row = (threadIdx.x >> 6) * 4 + (lane >> 4);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = chx_row16_sum(v[k]);
    if ((lane & 15) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[row * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += red[r * K + k];
        v[k] = t;
    }
    __syncthreads();
}

// 5. one workgroup per piece (a fixed range of at most kPiece particles of ONE slice in sorted order): its rows stay in
// registers for the two passes — sums, then second moments about the piece's own mean
template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void slice_piece_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ q,
                                                               int64_t Bx, int64_t Bw, int64_t Bq, int64_t N, int S,
                                                               const int* __restrict__ idx, const int* __restrict__ start,
                                                               const int* __restrict__ pstart, int64_t npmax, double* __restrict__ part) {
    __shared__ double red[16 * 21];
    const int64_t b = blockIdx.y;
    const int j = blockIdx.x;
    const int* pb = pstart + b * (S + 1);
    if (j >= pb[S]) return;                                 // (uniform: the row has fewer pieces than the grid)
    int lo = 0, hi = S;                                     // the slice k with pb[k] <= j < pb[k + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pb[mid] <= j) lo = mid;
        else hi = mid;
    }
    const int k = lo;
    const int* sb = start + b * (S + 1);
    const int64_t p0 = (int64_t)sb[k] + (int64_t)(j - pb[k]) * kPiece;
    const int64_t p1 = (p0 + kPiece < (int64_t)sb[k + 1]) ? p0 + kPiece : (int64_t)sb[k + 1];
    const T* __restrict__ xb = x + (Bx == 1 ? 0 : b) * N * 7;
    const T* __restrict__ wb = w ? w + (Bw == 1 ? 0 : b) * N : nullptr;
    const T* __restrict__ qb = q ? q + (Bq == 1 ? 0 : b) * N : nullptr;
    const int* __restrict__ ib = idx + b * N;
    double xv[kPieceU][6], wv[kPieceU], qv[kPieceU];
#pragma unroll
    for (int u = 0; u < kPieceU; ++u) {
        const int64_t p = p0 + u * CHX_BLOCK + threadIdx.x;
        const bool ok = p < p1;
        int64_t n = ib[ok ? p : p0];
        n = n < 0 ? 0 : (n >= N ? N - 1 : n);                // (always inside: idx holds particle indices)
#pragma unroll
        for (int c = 0; c < 6; ++c) xv[u][c] = (double)xb[n * 7 + c];
        wv[u] = ok ? (wb ? (double)wb[n] : 1.0) : 0.0;
        qv[u] = qb ? (double)qb[n] : 1.0;
    }
    double s[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i] = 0.0;
#pragma unroll
    for (int u = 0; u < kPieceU; ++u) {
        if (!(p0 + u * CHX_BLOCK + threadIdx.x < p1)) continue;
        s[0] += wv[u];
        s[1] += wv[u] * wv[u];
#pragma unroll
        for (int c = 0; c < 6; ++c) s[2 + c] += wv[u] * xv[u][c];
        s[8] += qv[u] * wv[u];
    }
    block_sum_all<9>(s, red);
    double mu[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) mu[c] = s[2 + c] / s[0];
    double m[21];
#pragma unroll
    for (int i = 0; i < 21; ++i) m[i] = 0.0;
#pragma unroll
    for (int u = 0; u < kPieceU; ++u) {
        if (!(p0 + u * CHX_BLOCK + threadIdx.x < p1)) continue;
        double d[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) d[c] = xv[u][c] - mu[c];
        int t = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double wd = wv[u] * d[a];
#pragma unroll
            for (int c = a; c < 6; ++c) m[t++] += wd * d[c];
        }
    }
    block_sum_all<21>(m, red);
    double* o = part + (b * npmax + j) * kSP;
    const int t = threadIdx.x;
    if (t < 2) o[t] = s[t];
    else if (t < 8) o[t] = mu[t - 2];
    else if (t < 29) {
#pragma unroll
        for (int i = 0; i < 21; ++i)
            if (t - 8 == i) o[t] = m[i];
    } else if (t == 29) o[29] = s[8];
}

// 6. one thread per (row, slice): the pieces merged in order (Chan et al.; the arithmetic of merge_moments_kernel with the
// centred sums themselves), pieces without weight skipped; a slice without weight gets the NaN pattern of chx_moments
__global__ void slice_finalize_kernel(const double* __restrict__ part, const int* __restrict__ pstart, int64_t npmax, int64_t B, int S,
                                      double* __restrict__ out, double* __restrict__ charge) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * S) return;
    const int64_t b = i / S;
    const int k = (int)(i - b * S);
    const int j0 = pstart[b * (S + 1) + k], j1 = pstart[b * (S + 1) + k + 1];
    const double* P = part + b * npmax * kSP;
    double W = 0.0, W2 = 0.0, Q = 0.0, mu[6] = {0, 0, 0, 0, 0, 0};
    for (int j = j0; j < j1; ++j) {
        const double* p = P + (int64_t)j * kSP;
        Q += p[29];
        if (!(p[0] > 0.0)) continue;
        W += p[0];
        W2 += p[1];
        for (int c = 0; c < 6; ++c) mu[c] += p[0] * p[2 + c];
    }
    for (int c = 0; c < 6; ++c) mu[c] /= W;
    double M[21];
    for (int t = 0; t < 21; ++t) M[t] = 0.0;
    for (int j = j0; j < j1; ++j) {
        const double* p = P + (int64_t)j * kSP;
        if (!(p[0] > 0.0)) continue;
        double d[6];
        for (int c = 0; c < 6; ++c) d[c] = p[2 + c] - mu[c];
        int t = 0;
        for (int a = 0; a < 6; ++a)
            for (int c = a; c < 6; ++c, ++t) M[t] += p[8 + t] + p[0] * d[a] * d[c];
    }
    double* o = out + i * CHX_MOM_NOUT;
    o[0] = W;
    o[1] = W2;
    for (int c = 0; c < 6; ++c) o[2 + c] = mu[c];
    const double cf = W - W2 / W;  // statistics.py:42
    for (int t = 0; t < 21; ++t) o[8 + t] = M[t] / cf;
    charge[i] = Q;
}

// Backward, per slice: with d = x - mu, hs = H d, H = Gsym / cf (Gsym = g + g^T on the upper-triangular cotangent g of the
// covariances), A = g_mu / W, moments_bwd_kernel's gradient regrouped:
//   dX = w (A + hs),  dW = C0 + w C1 + A.d + d.hs / 2,  C0 = g_W - S k / cf,  C1 = 2 g_W2 + 2 S / (cf W),
//   S = sum g_ab cov_ab, k = 1 + W2 / W^2. Charge: dQ = w g_q, dW += q g_q.
// A slice whose moment cotangent is all zero contributes exactly nothing (flag 0), and without a covariance cotangent the
// 1 / cf terms are left out — a loss that reads only populated slices gets no 0 * inf from empty or one-particle slices.
__global__ void slice_bwd_table_kernel(const double* __restrict__ out, const double* __restrict__ d_out, const double* __restrict__ d_charge,
                                       int64_t BS, double* __restrict__ tab) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BS) return;
    const double* o = out + i * CHX_MOM_NOUT;
    const double* g = d_out ? d_out + i * CHX_MOM_NOUT : nullptr;
    double* t = tab + i * kTab;
    for (int c = 0; c < kTab; ++c) t[c] = 0.0;
    t[kTab - 1] = d_charge ? d_charge[i] : 0.0;
    if (!g) return;
    bool any = false, any_cov = false;
    for (int c = 0; c < CHX_MOM_NOUT; ++c) {
        any = any || g[c] != 0.0;
        if (c >= 8) any_cov = any_cov || g[c] != 0.0;
    }
    if (!any) return;
    const double W = o[0], W2 = o[1];
    t[0] = 1.0;
    // (a slice whose members carry no weight has no mean, but its W and W2 are sums with a gradient like any other: dW = g_W +
    //  2 w g_W2. A centre of 0 keeps the A.d and d.H d terms, whose coefficients are 0 there, from turning into 0 * NaN)
    for (int c = 0; c < 6; ++c) t[1 + c] = W > 0.0 ? o[2 + c] : 0.0;
    for (int c = 0; c < 6; ++c) t[7 + c] = g[2 + c] == 0.0 ? 0.0 : g[2 + c] / W;
    t[34] = g[0];
    t[35] = 2.0 * g[1];
    if (any_cov) {
        const double icf = 1.0 / (W - W2 / W);
        double S = 0.0;
        for (int c = 0; c < 21; ++c) S += g[8 + c] * o[8 + c];
        int c = 0;
        for (int a = 0; a < 6; ++a)
            for (int e = a; e < 6; ++e, ++c) t[13 + c] = icf * (a == e ? 2.0 * g[8 + c] : g[8 + c]);
        const double kcf = 1.0 + W2 / (W * W);
        t[34] = g[0] - icf * S * kcf;
        t[35] = 2.0 * g[1] + 2.0 * icf * S / W;
    }
}

template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void slice_bwd_kernel(const T* __restrict__ x, const T* __restrict__ w, const T* __restrict__ q,
                                                             const T* __restrict__ edges, int64_t Bx, int64_t Bw, int64_t Bq, int64_t Be,
                                                             int64_t N, int S, const double* __restrict__ tab, T* __restrict__ dX,
                                                             T* __restrict__ dW, T* __restrict__ dQ) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* e = (T*)smem;
    const int64_t b = blockIdx.y;
    const T* eb = edges + (Be == 1 ? 0 : b) * (S + 1);
    for (int i = threadIdx.x; i <= S; i += CHX_BLOCK) e[i] = eb[i];
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * CHX_BLOCK + threadIdx.x;
    if (n >= N) return;
    const T* xr = x + ((Bx == 1 ? 0 : b) * N + n) * 7;
    const double wv = w ? (double)w[(Bw == 1 ? 0 : b) * N + n] : 1.0;
    const double qv = q ? (double)q[(Bq == 1 ? 0 : b) * N + n] : 1.0;
    const int k = hist_bin<T>(e, S, xr[4]);
    double gx[6] = {0, 0, 0, 0, 0, 0}, gw = 0.0, gq = 0.0;
    if (k >= 0) {
        const double* t = tab + (b * S + k) * kTab;
        gq = t[kTab - 1];
        if (t[0] != 0.0) {
            double d[6];
#pragma unroll
            for (int c = 0; c < 6; ++c) d[c] = (double)xr[c] - t[1 + c];
            double H[6][6];
            int c = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int f = a; f < 6; ++f, ++c) { H[a][f] = t[13 + c]; H[f][a] = t[13 + c]; }
            double lin = 0.0, quad = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double hs = 0.0;
#pragma unroll
                for (int f = 0; f < 6; ++f) hs += H[a][f] * d[f];
                gx[a] = wv * (t[7 + a] + hs);
                lin += t[7 + a] * d[a];
                quad += d[a] * hs;
            }
            gw = t[34] + wv * t[35] + lin + 0.5 * quad;
        }
        gw += qv * gq;
    }
    if (dX) {
        T* o = dX + (b * N + n) * 7;
#pragma unroll
        for (int c = 0; c < 6; ++c) o[c] = (T)gx[c];
        o[6] = (T)0;
    }
    if (dW) dW[b * N + n] = (T)gw;
    if (dQ) dQ[b * N + n] = (T)(wv * gq);
}

int check_slices(const void* x, const void* edges, int64_t B, int64_t Bx, int64_t Bw, int64_t Bq, int64_t Be, int64_t N, int32_t S,
                 int dtype) {
    if (!x || !edges || B < 1 || B > 65535 || N < 1 || N > 0x7fffffffLL || S < 1 || S > CHX_SLICES_MAX) return CHX_ERR_INVALID_ARG;
    if (!chx_bcast_ok(Bx, B) || !chx_bcast_ok(Bw, B) || !chx_bcast_ok(Bq, B) || !chx_bcast_ok(Be, B)) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    return CHX_OK;
}

template <typename T>
int slice_moments_t(const T* x, const T* w, const T* q, const T* edges, int64_t B, int64_t Bx, int64_t Bw, int64_t Bq, int64_t Be,
                    int64_t N, int S, double* out, double* charge, const SliceWs& ws, hipStream_t s) {
    const int64_t nt = ntiles(N), npmax = npieces_max(N, S);
    const int nbits = S > 1 ? 32 - __builtin_clz((unsigned)(S - 1)) : 0;
    const size_t lds = edge_lds_bytes(S, sizeof(T)) + (size_t)4 * S * sizeof(int);
    hipLaunchKernelGGL(slice_rank_kernel<T>, dim3((unsigned)((nt + 3) / 4), (unsigned)B), dim3(CHX_BLOCK), lds, s, x, Bx, edges, Be, N,
                       S, nbits, nt, ws.packed, ws.off);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(slice_scan_kernel, dim3((unsigned)((S + 3) / 4), (unsigned)B), dim3(CHX_BLOCK), 0, s, ws.off, S, nt, ws.totals);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(slice_start_kernel, dim3((unsigned)B), dim3(CHX_BLOCK), 0, s, ws.totals, S, ws.start, ws.pstart);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(slice_scatter_kernel, dim3((unsigned)((N + CHX_BLOCK - 1) / CHX_BLOCK), (unsigned)B), dim3(CHX_BLOCK), 0, s,
                       ws.packed, ws.off, ws.start, N, S, nt, ws.idx);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(slice_piece_kernel<T>, dim3((unsigned)npmax, (unsigned)B), dim3(CHX_BLOCK), 0, s, x, w, q, Bx, Bw, Bq, N, S,
                       ws.idx, ws.start, ws.pstart, npmax, ws.part);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(slice_finalize_kernel, dim3((unsigned)((B * S + 63) / 64)), dim3(64), 0, s, ws.part, ws.pstart, npmax, B, S, out,
                       charge);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace

extern "C" size_t chx_slice_moments_workspace_bytes(int64_t B, int64_t N, int32_t S) {
    if (B < 1 || N < 1 || S < 1 || S > CHX_SLICES_MAX) return 0;
    return slice_ws(nullptr, B, N, S).bytes;
}

extern "C" int chx_slice_moments(const void* x, const void* w, const void* q, const void* edges, int64_t B, int64_t Bx, int64_t Bw,
                                 int64_t Bq, int64_t Be, int64_t N, int32_t S, int dtype, double* out, double* charge, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!w) Bw = 1;
    if (!q) Bq = 1;
    int st = check_slices(x, edges, B, Bx, Bw, Bq, Be, N, S, dtype);
    if (st != CHX_OK) return st;
    if (!out || !charge) return CHX_ERR_INVALID_ARG;
    const SliceWs ws = slice_ws(workspace, B, N, S);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CHX_F32)
        return slice_moments_t<float>((const float*)x, (const float*)w, (const float*)q, (const float*)edges, B, Bx, Bw, Bq, Be, N, S, out,
                                      charge, ws, s);
    return slice_moments_t<double>((const double*)x, (const double*)w, (const double*)q, (const double*)edges, B, Bx, Bw, Bq, Be, N, S,
                                   out, charge, ws, s);
}

extern "C" int chx_slice_moments_bwd(const void* x, const void* w, const void* q, const void* edges, int64_t B, int64_t Bx, int64_t Bw,
                                     int64_t Bq, int64_t Be, int64_t N, int32_t S, int dtype, const double* out, const double* d_out,
                                     const double* d_charge, void* dX, void* dW, void* dQ, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    if (!w) Bw = 1;
    if (!q) Bq = 1;
    int st = check_slices(x, edges, B, Bx, Bw, Bq, Be, N, S, dtype);
    if (st != CHX_OK) return st;
    if (!out || (!d_out && !d_charge)) return CHX_ERR_INVALID_ARG;
    if (!dX && !dW && !dQ) return CHX_OK;
    const SliceWs ws = slice_ws(workspace, B, N, S);
    if (!workspace || workspace_bytes < ws.bytes) return CHX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(slice_bwd_table_kernel, dim3((unsigned)((B * S + 63) / 64)), dim3(64), 0, s, out, d_out, d_charge, B * S, ws.tab);
    CHX_CHECK_LAUNCH();
    const dim3 grid((unsigned)((N + CHX_BLOCK - 1) / CHX_BLOCK), (unsigned)B);
    if (dtype == CHX_F32)
        hipLaunchKernelGGL(slice_bwd_kernel<float>, grid, dim3(CHX_BLOCK), edge_lds_bytes(S, sizeof(float)), s, (const float*)x,
                           (const float*)w, (const float*)q, (const float*)edges, Bx, Bw, Bq, Be, N, S, ws.tab, (float*)dX, (float*)dW,
                           (float*)dQ);
    else
        hipLaunchKernelGGL(slice_bwd_kernel<double>, grid, dim3(CHX_BLOCK), edge_lds_bytes(S, sizeof(double)), s, (const double*)x,
                           (const double*)w, (const double*)q, (const double*)edges, Bx, Bw, Bq, Be, N, S, ws.tab, (double*)dX,
                           (double*)dW, (double*)dQ);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}
