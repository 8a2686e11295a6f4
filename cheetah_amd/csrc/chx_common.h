// chx_common.h — shared device/host helpers for the libchx HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "chx.h"

#define CHX_WAVE 64
#define CHX_BLOCK 256

#define CHX_CHECK_LAUNCH()                                   \
    do {                                                     \
        hipError_t e__ = hipGetLastError();                  \
        if (e__ != hipSuccess) return CHX_ERR_LAUNCH;        \
    } while (0)

static inline bool chx_bcast_ok(int64_t b, int64_t B) { return b == 1 || b == B; }
// f(T{}) with T = float or double as the dtype says: f is a generic lambda that casts the entry point's pointers to T.
template <typename F>
int dispatch_dtype(int dtype, F&& f) {
    return dtype == CHX_F32 ? f(float{}) : f(double{});
}
static __host__ __device__ inline bool chx_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// 16-byte vector type per element type: float -> 4 lanes, double -> 2 lanes.
template <typename T> struct chx_vec16;
template <> struct chx_vec16<float> { using type = float4; static constexpr int n = 4; };
template <> struct chx_vec16<double> { using type = double2; static constexpr int n = 2; };

// v + (v of the lane selected by the DPP control CTRL): a VALU move with a data-parallel-primitive lane pattern — no LDS
// round trip, unlike __shfl_xor (ds_bpermute_b32 + s_waitcnt per 32-bit half).
template <int CTRL>
__device__ __forceinline__ double chx_dpp_add(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    const int hi2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return v + __hiloint2double(hi2, lo2);
}

// Sum over the 64 lanes of a wavefront (all lanes receive the total). The four steps inside a row of 16 lanes are DPP
// moves (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror: after each step the lanes being paired
// already hold equal partial sums, so the mirrors act like xor 4 / xor 8); only the two steps across rows go through
// ds_bpermute. Measured motive (moments_onepass_kernel, 29 accumulators): 348 dependent ds_bpermute + s_waitcnt per wave
// were half of the kernel's 19.6 us.
__device__ __forceinline__ double chx_wave_sum(double v) {
    v = chx_dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
    v = chx_dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
    v = chx_dpp_add<0x141>(v);  // row_half_mirror
    v = chx_dpp_add<0x140>(v);  // row_mirror
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// The same sum, bit for bit, delivered in lane 63 ONLY (the other lanes hold partial sums): the two steps across rows as DPP
// row broadcasts (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3) instead of four dependent ds_bpermute —
// for passes that take many wave sums per wave and let one lane write them (the monitors of lattice_apply_kernel).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double chx_dpp_add_rows(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
    const int hi2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
    return v + __hiloint2double(hi2, lo2);
}
__device__ __forceinline__ double chx_wave_sum_lane63(double v) {
    v = chx_dpp_add<0xB1>(v);
    v = chx_dpp_add<0x4E>(v);
    v = chx_dpp_add<0x141>(v);
    v = chx_dpp_add<0x140>(v);
    v = chx_dpp_add_rows<0x142, 0xA>(v);   // row_bcast:15 -> rows 1 and 3: r1 + r0, r3 + r2
    v = chx_dpp_add_rows<0x143, 0xC>(v);   // row_bcast:31 -> rows 2 and 3: (r3 + r2) + (r1 + r0)
    return v;
}

// Sum over each row of 16 lanes only (every lane of a row receives its row's total): the DPP part of chx_wave_sum.
__device__ __forceinline__ double chx_row16_sum(double v) {
    v = chx_dpp_add<0xB1>(v);
    v = chx_dpp_add<0x4E>(v);
    v = chx_dpp_add<0x141>(v);
    v = chx_dpp_add<0x140>(v);
    return v;
}

// Block-wide sum of K doubles per thread (CHX_BLOCK threads = 4 waves). Result valid in thread 0.
template <int K>
__device__ __forceinline__ void chx_block_sum(double (&v)[K], double* smem /* [4*K] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = chx_wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) smem[wave * K + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            v[k] = smem[k] + smem[K + k] + smem[2 * K + k] + smem[3 * K + k];
    }
    __syncthreads();
}

// Block-wide sums of EIGHT doubles per thread, folded: instead of eight full wave sums (8 x (8 DPP moves + 4 ds_bpermute + 6
// adds) per wave) the lanes first split the eight values between them — after exchanging with lane ^ 1 a lane carries four of
// them (summed over the pair), after lane ^ 2 two (summed over its quad) — and only those two are summed over the four quads of
// the row of 16 (row_ror:8, row_ror:4). Lane p < 4 of every row then holds the row's totals of values {0,1}, {4,5}, {2,3}, {6,7}
// (p = 0..3) and leaves them in LDS; after one barrier threads k < 8 add the 16 rows of the workgroup: v[0] of thread k is the
// total of value k. ~60 instructions per wave instead of ~200. smem: 16 rows x 8 doubles.
template <int CTRL>
__device__ __forceinline__ double chx_dpp_get(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int lo2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    const int hi2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi2, lo2);
}
__device__ __forceinline__ void chx_block_sum8_folded(double (&v)[8], double* smem /* [16 * 8] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool b0 = lane & 1, b1 = lane & 2;
    double t[4], u[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double mine = b0 ? v[j + 4] : v[j], give = b0 ? v[j] : v[j + 4];
        t[j] = mine + chx_dpp_get<0xB1>(give);          // quad_perm [1,0,3,2]
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double mine = b1 ? t[j + 2] : t[j], give = b1 ? t[j] : t[j + 2];
        u[j] = mine + chx_dpp_get<0x4E>(give);          // quad_perm [2,3,0,1]
        u[j] += chx_dpp_get<0x128>(u[j]);               // row_ror:8
        u[j] += chx_dpp_get<0x124>(u[j]);               // row_ror:4
    }
    if ((lane & 15) < 4) {
        const int row = wave * 4 + (lane >> 4);
        const int first = 4 * (lane & 1) + (lane & 2);  // value index of u[0]
        smem[row * 8 + first] = u[0];
        smem[row * 8 + first + 1] = u[1];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc += smem[r * 8 + threadIdx.x];
        v[0] = acc;
    }
}

// THIRTY-TWO doubles per thread summed over the workgroup's rows of 16 lanes, folded the same way: after lane ^ 1 a lane carries 16
// of the values, after lane ^ 2 eight, and those eight are summed over the four quads of its row (row_ror:8, row_ror:4): ~216
// instructions per wave against 32 x 12 for full row sums. Lane p < 4 of a row ends with the row totals of values
// 16 (p & 1) + 8 (p >> 1) + j, j < 8, and stores them to smem[row][32] (row = wave * 4 + lane / 16). No barrier in here.
__device__ __forceinline__ void chx_row16_sum32_folded(double (&v)[32], double* smem /* [rows][32] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool b0 = lane & 1, b1 = lane & 2;
    double t[16], u[8];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const double mine = b0 ? v[j + 16] : v[j], give = b0 ? v[j] : v[j + 16];
        t[j] = mine + chx_dpp_get<0xB1>(give);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double mine = b1 ? t[j + 8] : t[j], give = b1 ? t[j] : t[j + 8];
        u[j] = mine + chx_dpp_get<0x4E>(give);
        u[j] += chx_dpp_get<0x128>(u[j]);
        u[j] += chx_dpp_get<0x124>(u[j]);
    }
    if ((lane & 15) < 4) {
        double* dst = smem + (wave * 4 + (lane >> 4)) * 32 + 16 * (lane & 1) + 4 * (lane & 2);
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j] = u[j];
    }
}

// SIXTEEN doubles per thread, the same folding (~108 instructions per wave): lane p < 4 of a row ends with the row totals of values
// 8 (p & 1) + 4 (p >> 1) + j, j < 4, and stores them to smem[row * stride + j...]. No barrier in here.
__device__ __forceinline__ void chx_row16_sum16_folded(double (&v)[16], double* smem /* [rows][stride] */, int stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool b0 = lane & 1, b1 = lane & 2;
    double t[8], u[4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const double mine = b0 ? v[j + 8] : v[j], give = b0 ? v[j] : v[j + 8];
        t[j] = mine + chx_dpp_get<0xB1>(give);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double mine = b1 ? t[j + 4] : t[j], give = b1 ? t[j] : t[j + 4];
        u[j] = mine + chx_dpp_get<0x4E>(give);
        u[j] += chx_dpp_get<0x128>(u[j]);
        u[j] += chx_dpp_get<0x124>(u[j]);
    }
    if ((lane & 15) < 4) {
        double* dst = smem + (wave * 4 + (lane >> 4)) * stride + 8 * (lane & 1) + 2 * (lane & 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j] = u[j];
    }
}

// ---- LDS tile staging: contiguous 16-byte vector transfers between global memory and an LDS
// tile (coalesced global_load/store_dwordx4); scalar fallback when the tile start is unaligned.
// Non-temporal 16-byte accesses (the `nt` cache policy of global_load/store_dwordx4): a streaming pass reads every
// byte once and writes every byte once, so nothing is gained by allocating the lines in L2. Measured on MI355X
// (benchmarks/apply_variants.hip, two buffers ping-ponged like a tracked lattice): 5.69 -> 6.71 TB/s at 1e6 particles,
// 5.44 -> 5.90 TB/s at 1.6e7. Not used where other workgroups re-read the same input (a beam shared by a batch).
typedef float chx_v2f __attribute__((ext_vector_type(2)));
typedef float chx_v4f __attribute__((ext_vector_type(4)));
typedef double chx_v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 chx_nt_load(const float4* p) {
    const chx_v4f v = __builtin_nontemporal_load(reinterpret_cast<const chx_v4f*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ double2 chx_nt_load(const double2* p) {
    const chx_v2d v = __builtin_nontemporal_load(reinterpret_cast<const chx_v2d*>(p));
    return make_double2(v.x, v.y);
}
__device__ __forceinline__ void chx_nt_store(float4 v, float4* p) {
    const chx_v4f w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<chx_v4f*>(p));
}
__device__ __forceinline__ void chx_nt_store(double2 v, double2* p) {
    const chx_v2d w = {v.x, v.y};
    __builtin_nontemporal_store(w, reinterpret_cast<chx_v2d*>(p));
}

// TP = particles per tile (compile time, for documentation of the call sites). The copy loops are deliberately left
// rolled: issuing all ceil(TP * 7 / (VN * 256)) = 4 loads of a lane before the first wait was measured SLOWER on MI355X
// (apply at 1e6 particles: 8.4 -> 9.4 us repeated, 9.3 -> 11.3 us ping-ponged) — with 8 workgroups per CU the memory
// system is already oversubscribed and the extra 16 VGPRs cost occupancy.
template <typename T, int TP>
__device__ __forceinline__ void tile_load(const T* __restrict__ g, T* __restrict__ lds, int n_elem,
                                          bool vec_ok, bool nt = false) {
    using V = typename chx_vec16<T>::type;
    constexpr int VN = chx_vec16<T>::n;
    if (vec_ok) {
        const int nvec = n_elem / VN;
        const V* __restrict__ gv = reinterpret_cast<const V*>(g);
        V* lv = reinterpret_cast<V*>(lds);
        if (nt) {
            for (int v = threadIdx.x; v < nvec; v += CHX_BLOCK) lv[v] = chx_nt_load(gv + v);
        } else {
            for (int v = threadIdx.x; v < nvec; v += CHX_BLOCK) lv[v] = gv[v];
        }
        for (int e = nvec * VN + threadIdx.x; e < n_elem; e += CHX_BLOCK) lds[e] = g[e];
    } else {
        for (int e = threadIdx.x; e < n_elem; e += CHX_BLOCK) lds[e] = g[e];
    }
}

template <typename T, int TP>
__device__ __forceinline__ void tile_store(T* __restrict__ g, const T* __restrict__ lds, int n_elem,
                                           bool vec_ok, bool nt = false) {
    using V = typename chx_vec16<T>::type;
    constexpr int VN = chx_vec16<T>::n;
    if (vec_ok) {
        const int nvec = n_elem / VN;
        V* __restrict__ gv = reinterpret_cast<V*>(g);
        const V* lv = reinterpret_cast<const V*>(lds);
        if (nt) {
            for (int v = threadIdx.x; v < nvec; v += CHX_BLOCK) chx_nt_store(lv[v], gv + v);
        } else {
            for (int v = threadIdx.x; v < nvec; v += CHX_BLOCK) gv[v] = lv[v];
        }
        for (int e = nvec * VN + threadIdx.x; e < n_elem; e += CHX_BLOCK) g[e] = lds[e];
    } else {
        for (int e = threadIdx.x; e < n_elem; e += CHX_BLOCK) g[e] = lds[e];
    }
}

// ---- the same staging per WAVE: a wave moves its own rows between global memory and its own LDS slice (64 rows of 28 / 56
// bytes are a whole number of 16-byte chunks), so no workgroup barrier is needed around the transfer — chx_wave_sync()
// orders the wave's LDS accesses — and the waves of a workgroup run independently.
__device__ __forceinline__ void chx_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T>
__device__ __forceinline__ void wave_tile_load(const T* __restrict__ g, T* __restrict__ wl, int n_elem, bool vec_ok,
                                                bool nt = false) {
    using V = typename chx_vec16<T>::type;
    constexpr int VN = chx_vec16<T>::n;
    const int lane = threadIdx.x & 63;
    if (vec_ok) {
        const int nvec = n_elem / VN;
        const V* __restrict__ gv = reinterpret_cast<const V*>(g);
        V* lv = reinterpret_cast<V*>(wl);
        if (nt) {
            for (int v = lane; v < nvec; v += 64) lv[v] = chx_nt_load(gv + v);
        } else {
            for (int v = lane; v < nvec; v += 64) lv[v] = gv[v];
        }
        for (int e = nvec * VN + lane; e < n_elem; e += 64) wl[e] = g[e];
    } else {
        for (int e = lane; e < n_elem; e += 64) wl[e] = g[e];
    }
}

template <typename T>
__device__ __forceinline__ void wave_tile_store(T* __restrict__ g, const T* __restrict__ wl, int n_elem, bool vec_ok,
                                                 bool nt = false) {
    using V = typename chx_vec16<T>::type;
    constexpr int VN = chx_vec16<T>::n;
    const int lane = threadIdx.x & 63;
    if (vec_ok) {
        const int nvec = n_elem / VN;
        V* __restrict__ gv = reinterpret_cast<V*>(g);
        const V* lv = reinterpret_cast<const V*>(wl);
        if (nt) {
            for (int v = lane; v < nvec; v += 64) chx_nt_store(lv[v], gv + v);
        } else {
            for (int v = lane; v < nvec; v += 64) gv[v] = lv[v];
        }
        for (int e = nvec * VN + lane; e < n_elem; e += 64) g[e] = wl[e];
    } else {
        for (int e = lane; e < n_elem; e += 64) g[e] = wl[e];
    }
}

// The same two transfers UNROLLED, for a wave's whole slice of WV 16-byte chunks (WV compile time) of which `valid_elem` elements
// exist: every chunk of a lane is requested before the first is waited for, then the few elements behind the last whole chunk (the
// ragged end of a batch row). Both pairs exist on purpose: the rolled one above takes any length and an unaligned slice (scalar
// fallback) and costs no registers beyond one chunk — what tile_load / tile_store were measured to want; this one needs the slice
// 16-byte aligned in global memory and is what apply_wave_kernel, apply_shared_wave_kernel and lattice_scan_wave_kernel were
// tuned with: a wave that stages on its own has no other wave's barrier to wait at, so the depth of its own requests is its overlap.
// Stores are non-temporal; loads when `nt`.
template <typename T, int WV>
__device__ __forceinline__ void wave_slice_load(const T* __restrict__ g, T* __restrict__ wl, int valid_elem, bool nt) {
    using V = typename chx_vec16<T>::type;
    constexpr int VN = chx_vec16<T>::n;
    const int lane = threadIdx.x & 63, vchunks = valid_elem / VN;
    const V* __restrict__ gv = reinterpret_cast<const V*>(g);
    V* lv = reinterpret_cast<V*>(wl);
#pragma unroll
    for (int c = 0; c < (WV + 63) / 64; ++c) {
        const int v = c * 64 + lane;
        if (v < vchunks) lv[v] = nt ? chx_nt_load(gv + v) : gv[v];
    }
    for (int e = vchunks * VN + lane; e < valid_elem; e += 64) wl[e] = g[e];
}

// TAIL_TEST: the scalar tail sits behind a test of its own for "the slice is whole" (the row loops of the shared-beam kernels were
// tuned with it; apply_wave_kernel, one slice per wave, without: either way costs the other a wave per SIMD in registers).
template <typename T, int WV, bool TAIL_TEST = true>
__device__ __forceinline__ void wave_slice_store(T* __restrict__ g, const T* __restrict__ wl, int valid_elem) {
    using V = typename chx_vec16<T>::type;
    constexpr int VN = chx_vec16<T>::n;
    const int lane = threadIdx.x & 63, vchunks = valid_elem / VN;
    V* __restrict__ gv = reinterpret_cast<V*>(g);
    const V* lv = reinterpret_cast<const V*>(wl);
#pragma unroll
    for (int c = 0; c < (WV + 63) / 64; ++c) {
        const int v = c * 64 + lane;
        if (v < vchunks) chx_nt_store(lv[v], gv + v);
    }
    if (!TAIL_TEST || vchunks < WV) {             // the last tile of a row: a few elements beyond the last whole chunk
        for (int e = vchunks * VN + lane; e < valid_elem; e += 64) g[e] = wl[e];
    }
}

// ---- tile coordinates: workgroup blockIdx.x takes tile t of batch row b of x[B][N][7], tiles of TP rows laid out per batch row so
// that a tile never straddles two rows (blockIdx.x = b * ceil(N / TP) + t).
template <int TP>
struct chx_tile {
    int64_t N, tiles_per_row, b, t, n0;   // n0: first row of the tile within its batch row
    // rows of the tile that exist (< TP only in the last tile of a batch row)
    __device__ __forceinline__ int np() const { return (int)((N - n0 < TP) ? (N - n0) : TP); }
    __device__ __forceinline__ bool full() const { return N - n0 >= TP; }
};
template <int TP>
__device__ __forceinline__ chx_tile<TP> chx_tile_coords(int64_t N) {
    const int64_t tiles_per_row = (N + TP - 1) / TP;
    const int64_t b = blockIdx.x / tiles_per_row;
    const int64_t t = blockIdx.x - b * tiles_per_row;
    return {N, tiles_per_row, b, t, t * TP};
}
// The vector path of tile_load / tile_store needs the tile start 16-byte aligned: the base (base_ok, checked on the host) and
// row * N * 7 * sizeof(T) for the tile's batch row (the input's row is 0 for one beam shared by the batch); n0 * 7 * sizeof(T) is
// a multiple of 16 by construction. A macro, not a function: behind a call the compiler orders and branches the prologue of
// every kernel that uses it differently (profiles/map7_refactor.md), and this text is what the kernels always held.
#define CHX_TILE_VEC_OK(T, base_ok, row, N) ((base_ok) && ((((row) * (N) * 7 * (int64_t)sizeof(T)) & 15) == 0))

// ---- column tiles: the in-place element passes of chx_track_elementwise between its first and its last one ---------------
// A full tile of TP rows (TP * 7 values, the same bytes in every pass) holds its rows transposed, [7][TP] instead of [TP][7].
// A lane then owns 16 bytes of consecutive rows in each of the seven columns, needs no LDS and no barrier, and a column that a
// map leaves as it was (px, py, delta and the 1 behind a drift) is a store the wave does not issue. Column 6 of every beam
// this library makes is the constant 1 and every element's map leaves it so: given one word of scratch per tile, the entering
// pass records where that holds and the column passes there do not read the column either (chx_coltile_pass, FLAGGED).
// Shared with benchmarks/apply_coltile.hip, which times exactly these bodies.
typedef unsigned chx_v4u __attribute__((ext_vector_type(4)));
template <typename T> struct chx_col16;   // V: 16 bytes of one column, P: two rows of it (one packed FMA per step in float32)
template <> struct chx_col16<float> { using V = chx_v4f; using P = chx_v2f; };
template <> struct chx_col16<double> { using V = chx_v2d; using P = chx_v2d; };

// ---- THE first-order map step: y = R x with R row-major 7x7. Row i is R_i0 * x_0 first, then six fused multiply-adds j = 1..6,
// in the storage dtype: the one spelling of that chain in the library, so that every kernel that sends a particle through a map
// — single pass, fused, element by element, column tiles, lattice stretches, scans, the chains of chx_nonlinear.hip and
// chx_spacecharge.hip, the moments of chx_moments.hip, the mapped deposits of chx_cic_dev.h — writes the same bits. X = T: one particle; X = chx_v2f with T = float: two
// particles side by side, every step ONE v_pk_fma_f32 (the map entry a scalar operand); X = double with T = float: float32-rounded
// maps on fp64 coordinates. R may live in SGPRs (uniform pointer).
// Row i for NX operands side by side: every map entry is fetched once and used for all of them (LaneRows, kMapByMatrixRow).
template <typename T, typename X, int NX>
__device__ __forceinline__ void chx_map7_row(const T* __restrict__ R, int i, const X (&x)[NX][7], X (&y)[NX][7]) {
#pragma unroll
    for (int n = 0; n < NX; ++n) y[n][i] = x[n][0] * R[i * 7];
#pragma unroll
    for (int j = 1; j < 7; ++j) {
        const X m = (X)R[i * 7 + j];
#pragma unroll
        for (int n = 0; n < NX; ++n) y[n][i] = __builtin_elementwise_fma(m, x[n][j], y[n][i]);
    }
}
// ROWS < 7: only the first rows of the map (the moments take six coordinates)
template <typename T, typename X, int ROWS = 7>
__device__ __forceinline__ void chx_map7(const T* __restrict__ R, const X (&x)[7], X (&y)[ROWS]) {
    X x1[1][7], y1[1][7];
#pragma unroll
    for (int j = 0; j < 7; ++j) x1[0][j] = x[j];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        chx_map7_row<T, X, 1>(R, i, x1, y1);
        y[i] = y1[0][i];
    }
}
// one row alone, Rrow = R + 7 i with i a run-time index (the coordinates a deposit takes of a mapped particle, chx_cic_dev.h)
template <typename T, typename X>
__device__ __forceinline__ X chx_map7_one_row(const T* __restrict__ Rrow, const X (&x)[7]) {
    X x1[1][7], y1[1][7];
#pragma unroll
    for (int j = 0; j < 7; ++j) x1[0][j] = x[j];
    chx_map7_row<T, X, 1>(Rrow, 0, x1, y1);
    return y1[0][0];
}
// in place
template <typename T, typename X>
__device__ __forceinline__ void chx_map7_inplace(const T* __restrict__ R, X (&x)[7]) {
    X y[7];
    chx_map7<T, X>(R, x, y);
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = y[j];
}

// One column pass over a full column tile at g, TP / (16 / sizeof(T)) lanes per workgroup. Column i goes back only if some lane
// of the wave holds a result whose bits differ from what it loaded: memory already holds exactly the bits a skipped store would
// have written, so the tile is bit for bit what storing everything leaves (NaN payloads, infinities and -0.0 included).
// g is read and written: no __restrict__. NT_LOAD: the beam does not stay in L2 from pass to pass, stream past it.
// FLAGGED: *flag (one word per tile, written by chx_coltile_edge, FLAG) says that column 6 of the tile, the affine coordinate, is
// all (T)1 in memory. The six loads of columns 0..5 leave first, then the flag is read (a uniform address: a scalar load behind
// the vector loads); where it is set the seventh load, 16 bytes per lane through the L2 queue that bounds the pass, is not
// issued and x[6] is the constant. The constant goes through an empty asm so that both arms run the same fma chain (no
// fma(r, 1, acc) folded into an add): identical inputs to identical instructions, identical bits. A wave whose column 6 comes
// out other than it went in (a map whose last row is not e6, a NaN or inf in another column against a zero of row 6) stores
// it as ever and clears the flag; a wave that saw no difference leaves the 1s in memory, which is what it would have stored.
// Two waves of a tile may both clear it, and a wave may read the flag before or after the other wave's clear: its own 16
// bytes per lane of column 6 are in memory either way. The flag is not set again within a call.
template <typename T, int TP, bool NT_LOAD, bool NT_STORE = true, bool FLAGGED = false>
__device__ __forceinline__ void chx_coltile_pass(T* g, const T* __restrict__ R, unsigned* flag = nullptr) {
    using V = typename chx_col16<T>::V;
    using P = typename chx_col16<T>::P;
    constexpr int LANES = TP / (16 / (int)sizeof(T));
    constexpr int NLOAD = FLAGGED ? 6 : 7;
    V* gv = reinterpret_cast<V*>(g) + threadIdx.x;
    V x[7], y[7];
#pragma unroll
    for (int j = 0; j < NLOAD; ++j) x[j] = NT_LOAD ? __builtin_nontemporal_load(gv + j * LANES) : gv[j * LANES];
    unsigned flagged = 0;
    if constexpr (FLAGGED) {
        flagged = *flag;
        T one = (T)1;
        asm("" : "+v"(one));
        x[6] = (V)one;
        if (!flagged) x[6] = NT_LOAD ? __builtin_nontemporal_load(gv + 6 * LANES) : gv[6 * LANES];
    }
    if constexpr (sizeof(T) == 4) {
        P lo[7], hi[7], ylo[7], yhi[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) { lo[j] = x[j].xy; hi[j] = x[j].zw; }
        chx_map7<T, P>(R, lo, ylo);
        chx_map7<T, P>(R, hi, yhi);
#pragma unroll
        for (int j = 0; j < 7; ++j) { y[j].xy = ylo[j]; y[j].zw = yhi[j]; }
    } else {
        chx_map7<T, P>(R, x, y);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const chx_v4u d = __builtin_bit_cast(chx_v4u, y[j]) ^ __builtin_bit_cast(chx_v4u, x[j]);
        if (__any((d.x | d.y | d.z | d.w) != 0u)) {
            if (NT_STORE) __builtin_nontemporal_store(y[j], gv + j * LANES);
            else gv[j * LANES] = y[j];
            if (FLAGGED && j == 6 && flagged && (threadIdx.x & 63) == 0) *flag = 0u;
        }
    }
}

// The rows of a tile that is not full (the last one of a batch row) stay [np][7] in every pass; a lane takes whole rows.
template <typename T>
__device__ __forceinline__ void chx_rowtile_pass(T* g, const T* __restrict__ R, int np) {
    for (int p = threadIdx.x; p < np; p += blockDim.x) {
        T x[7], y[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) x[j] = g[p * 7 + j];
        chx_map7<T, T>(R, x, y);
#pragma unroll
        for (int j = 0; j < 7; ++j) g[p * 7 + j] = y[j];
    }
}

// The pass that enters (TO_COLUMNS) or leaves the column layout, CHX_BLOCK lanes: the tile's bytes go through LDS as in every
// LDS-staged pass, the lane reads its rows in the layout the tile came in and writes them in the one it leaves in. A tile that is
// not full is [np][7] on both sides. The library runs it in place (gin == gout, in_vec true, nt_in false: the rows just written
// come from L2); with gin the input of the call an entering pass is a pass 0 that writes column tiles (in_vec / nt_in as in
// apply_tile_kernel), which benchmarks/apply_coltile.hip measured and the library does not use (chx_apply_tiles.h).
// gout must be 16-byte aligned (the column layout exists only on aligned batch rows, chx_coltile_ok): the store always takes the
// vector path, only the input side has an alignment argument.
// FLAG (entering only): the pass also says what it left there — *flag is written for the tile, every call, so that the flags need
// no initialising: 1 iff every value of column 6 the tile now holds has the bits of (T)1. Wave 0 reads that column back from the
// LDS image behind the last barrier (32 bytes per lane), one lane stores the word. The whole of column 6 goes to memory whatever
// the flag says. A tile that is not full stays rows, and its flag, which no pass reads, is 0.
template <typename T, int TP, bool TO_COLUMNS, bool FLAG = false>
__device__ __forceinline__ void chx_coltile_edge(const T* gin, T* gout, const T* __restrict__ R, T* lds, int np, bool in_vec,
                                                 bool nt_in, unsigned* flag = nullptr) {
    static_assert(TO_COLUMNS || !FLAG, "only the entering pass writes a flag");
    constexpr int PPT = TP / CHX_BLOCK;
    const bool full = np == TP;
    const bool in_cols = full && !TO_COLUMNS, out_cols = full && TO_COLUMNS;
    tile_load<T, TP>(gin, lds, np * 7, in_vec, nt_in);
    __syncthreads();
    T y[PPT][7];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = threadIdx.x + k * CHX_BLOCK;
        if (p < np) {
            T x[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) x[j] = in_cols ? lds[j * TP + p] : lds[p * 7 + j];
            chx_map7<T, T>(R, x, y[k]);
        }
    }
    if (full) __syncthreads();   // the layout changes: every lane has read its rows before another lane's results land on them
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = threadIdx.x + k * CHX_BLOCK;
        if (p < np) {
#pragma unroll
            for (int j = 0; j < 7; ++j) lds[out_cols ? j * TP + p : p * 7 + j] = y[k][j];
        }
    }
    __syncthreads();
    tile_store<T, TP>(gout, lds, np * 7, true, true);
    if constexpr (FLAG) {
        using V = typename chx_col16<T>::V;
        if (threadIdx.x < 64) {
            bool ones = full;
            if (full) {
                constexpr int NV = TP * (int)sizeof(T) / 16 / 64;   // 16-byte pieces of column 6 per lane of one wave
                const V* c6 = reinterpret_cast<const V*>(lds + 6 * TP);
                const V one = (V)(T)1;
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const chx_v4u d = __builtin_bit_cast(chx_v4u, c6[threadIdx.x + i * 64]) ^ __builtin_bit_cast(chx_v4u, one);
                    ones = ones && (d.x | d.y | d.z | d.w) == 0u;
                }
            }
            const bool all_ones = __all(ones);
            if (threadIdx.x == 0) *flag = all_ones ? 1u : 0u;
        }
    }
}

static inline int chx_grid_for(int64_t work_items, int per_block, int cap) {
    int64_t g = (work_items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}
