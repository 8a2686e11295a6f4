// apply_coltile.hip — what does an in-place element pass cost when it stores only the coordinates its map changed?
//
// chx_track_elementwise runs passes 1..E-1 in place. A drift changes x, y and tau of a row, a quadrupole x, px, y, py and tau,
// but in rows of 28 bytes every 128-byte line holds changed dwords, so every pass writes all 28 bytes per particle. Here the
// passes between the first and the last in-place pass keep every full 512-row tile transposed ([7][512], the same bytes, the
// same workgroup, the same XCD) and a wave stores a column only if one of its lanes holds other bits than it loaded
// (chx_common.h: column tiles — the bodies timed here are the ones chx_apply.hip launches). 100 passes back to back, fp32,
// HIP events, old and new alternating in one process, 5 runs each, every result compared bit for bit with the production
// structure (nt loads, nt stores, rows) after the same passes:
//   ab     at one size: variant (i) of apply_l2_resident.hip (rows, L2-allocating loads, nt stores: production MODE 3) against
//          the column passes (16 bytes per lane and column, nt / plain stores; 8 bytes per lane, 256 lanes), with the
//          benchmark's FODO cell (quadrupole, drift, quadrupole, drift), a map that changes columns 0..5 in every row
//          (nothing to skip) and the identity (nothing to store);
//   sweep  the FODO cell over the sizes around the production thresholds: the in-place pass production uses at that size
//          (libchx's chx_apply_affine7 in place, or variant (i) between 14.7 and 28 MiB) against the column passes with
//          L2-allocating or nt loads and nt or plain stores.
// Results: profiles/r08_coltile.md.
//
// r09 (profiles/r09_map_prologue.md): both tables gain two candidates beside the production kernels, which are kernel for kernel
// what chx_coltile.hip launches (k_edge_prod, k_col16_prod):
//   r09 pass       production edge passes, column pass with the map requested before the particles, in one piece (r09_map_request)
//   r09 pass+edge  the same in the edge passes too; kernel arguments fetched at once, no division for one beam
// Neither was faster than production beyond the spreads and neither is in the library; their bodies live here (r09_*).
// Built a second time with -mllvm -amdgpu-kernarg-preload-count=8 (the first 8 dwords of the kernel arguments arrive in scalar
// registers with the wave), every kernel of this file takes its arguments that way: the two builds, alternating, are the measurement
// behind that option for chx_coltile.hip.
//
// r10 (profiles/r10_const_column.md): whole calls, pass 0 included, of the production structure against
//   part 1         the pass that enters the layout writes one word per tile (column 6 all 1), the column passes read six columns
//                  where it is set (k_enter, k_col16_flag: kernel for kernel coltile_enter_kernel / coltile_pass_flag_kernel)
//   part 2         pass 0 writes the column tiles itself (k_enter_first), pass 1 is an ordinary column pass
//   part 1 + 2     both
// Part 1 is in the library; part 2 moved nothing beyond the spreads at any size and lives here only.
// us per pass = the whole call / 100; `r10 [rows]` for the three maps at one size, `r10sweep` for the FODO cell over the sizes.
//
// Build (after libchx.so) and run:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Icheetah_amd/csrc -Iinclude benchmarks/apply_coltile.hip \
//         -Lcheetah_amd -lchx -L/opt/rocm/lib -lhipfft -Wl,-rpath,$PWD/cheetah_amd -o apply_coltile
//   (the second build: the same line with -mllvm -amdgpu-kernarg-preload-count=8 and -o apply_coltile_preload)
//   ./apply_coltile ab [rows]; ./apply_coltile sweep; ./apply_coltile r10 [rows]; ./apply_coltile r10sweep
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "chx.h"
#include "chx_common.h"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

constexpr int TP = 512;  // rows per tile, as tile_cfg<float>

__device__ __forceinline__ void rows_in_lds(const float* __restrict__ R, float* lds, int np) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int p = threadIdx.x + k * CHX_BLOCK;
        if (p < np) {
            float x[7], y[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) x[j] = lds[p * 7 + j];
            chx_map7<float, float>(R, x, y);
#pragma unroll
            for (int j = 0; j < 7; ++j) lds[p * 7 + j] = y[j];
        }
    }
}

// rows through LDS: NT_LOAD = the production apply_tile_kernel<float,2,0> structure, else its MODE 3 (variant (i) of r07)
template <bool NT_LOAD>
__global__ __launch_bounds__(CHX_BLOCK) void k_rows(const float* x_in, const float* __restrict__ R, float* x_out, long N) {
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    const long n0 = (long)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    tile_load<float, TP>(x_in + n0 * 7, lds, np * 7, true, NT_LOAD);
    __syncthreads();
    rows_in_lds(R, lds, np);
    __syncthreads();
    tile_store<float, TP>(x_out + n0 * 7, lds, np * 7, true, true);
}

// ---- the production kernels (coltile_edge_kernel, coltile_pass_kernel of chx_coltile.hip) ----
template <bool TO_COLUMNS>
__global__ __launch_bounds__(CHX_BLOCK) void k_edge_prod(float* x, const float* __restrict__ R, int64_t BR, int64_t N) {
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    const int64_t tiles_per_row = (N + TP - 1) / TP;
    const int64_t b = blockIdx.x / tiles_per_row;
    const int64_t n0 = (blockIdx.x - b * tiles_per_row) * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    float* g = x + (b * N + n0) * 7;
    chx_coltile_edge<float, TP, TO_COLUMNS>(g, g, R + ((BR == 1) ? 0 : b) * 49, lds, np, true, false);
}

template <bool NT_LOAD, bool NT_STORE>
__global__ __launch_bounds__(TP / 4) void k_col16_prod(float* x, const float* __restrict__ R, int64_t BR, int64_t N) {
    const int64_t tiles_per_row = (N + TP - 1) / TP;
    const int64_t b = blockIdx.x / tiles_per_row;
    const int64_t n0 = (blockIdx.x - b * tiles_per_row) * TP;
    float* g = x + (b * N + n0) * 7;
    const float* __restrict__ Rb = R + ((BR == 1) ? 0 : b) * 49;
    if (N - n0 >= TP) chx_coltile_pass<float, TP, NT_LOAD, NT_STORE>(g, Rb);
    else chx_rowtile_pass<float>(g, Rb, (int)(N - n0));
}

// ---- r10: the kernels chx_coltile.hip launches when chx_track_elementwise is given scratch ----
template <bool NT_LOAD>
__global__ __launch_bounds__(TP / 4) void k_col16_flag(float* x, const float* __restrict__ R, unsigned* flags, int64_t N, int64_t BR) {
    const int64_t tiles_per_row = (N + TP - 1) / TP;
    const int64_t b = blockIdx.x / tiles_per_row;
    const int64_t n0 = (blockIdx.x - b * tiles_per_row) * TP;
    float* g = x + (b * N + n0) * 7;
    const float* __restrict__ Rb = R + ((BR == 1) ? 0 : b) * 49;
    if (N - n0 >= TP) chx_coltile_pass<float, TP, NT_LOAD, true, true>(g, Rb, flags + blockIdx.x);
    else chx_rowtile_pass<float>(g, Rb, (int)(N - n0));
}

// pass 1 in place: coltile_enter_kernel
__global__ __launch_bounds__(CHX_BLOCK) void k_enter(float* x, const float* __restrict__ R, unsigned* flags, int64_t N, int64_t BR) {
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    const int64_t tiles_per_row = (N + TP - 1) / TP;
    const int64_t b = blockIdx.x / tiles_per_row;
    const int64_t n0 = (blockIdx.x - b * tiles_per_row) * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    float* g = x + (b * N + n0) * 7;
    chx_coltile_edge<float, TP, true, true>(g, g, R + ((BR == 1) ? 0 : b) * 49, lds, np, true, false, flags + blockIdx.x);
}

// part 2, not in the library: pass 0 from the input of the call (shared by the batch rows when Bx == 1) straight into column tiles,
// with apply_tile_kernel's alignment handling. in_flags: bit 0 = x_in 16-byte aligned, bit 1 = nt loads.
__global__ __launch_bounds__(CHX_BLOCK) void k_enter_first(const float* x_in, const float* __restrict__ R, float* x_out, unsigned* flags,
                                                           int64_t N, int64_t BR, int64_t Bx, int in_flags) {
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    const int64_t tiles_per_row = (N + TP - 1) / TP;
    const int64_t b = blockIdx.x / tiles_per_row;
    const int64_t n0 = (blockIdx.x - b * tiles_per_row) * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const bool in_vec = (in_flags & 1) && (((in_row * N * 7 * (int64_t)sizeof(float)) & 15) == 0);
    chx_coltile_edge<float, TP, true, true>(x_in + (in_row * N + n0) * 7, x_out + (b * N + n0) * 7, R + ((BR == 1) ? 0 : b) * 49, lds, np, in_vec,
                                 (in_flags & 2) != 0, flags + blockIdx.x);
}

// ---- r09, measured and not taken: the map requested before the particles, in one piece (profiles/r09_map_prologue.md) ----
// ---- a wave-uniform map held in scalar registers ------------------------------------------------------------------------------
// An element pass is one generation of waves that all start together and all wait for the same 196 bytes: nothing hides the map's
// fetch, and left to itself the compiler asks for a float32 map in three or four pieces, each waited for where its first entry is
// used. r09_map_request() asks for all 49 entries at once (three s_load_dwordx16 and one s_load_dword), as early as the caller
// places it; r09_map_arrive() is the one wait: from there on the entries are register operands of the FMAs. Between the two the
// caller forms its addresses and issues its tile loads. R must be wave-uniform and not written by the kernel.
// A float64 map is 98 scalar registers of 102: it stays a pointer, and the compiler fetches it as before.
typedef float r09_v16f __attribute__((ext_vector_type(16)));
typedef float r09_v16f_a4 __attribute__((ext_vector_type(16), aligned(4)));
template <typename T> struct r09_map_regs {
    const T* __restrict__ p;
    __device__ __forceinline__ T operator[](int i) const { return p[i]; }
};
template <> struct r09_map_regs<float> {
    r09_v16f a, b, c;
    float d;
    __device__ __forceinline__ float operator[](int i) const { return i < 16 ? a[i] : (i < 32 ? b[i - 16] : (i < 48 ? c[i - 32] : d)); }
};
template <typename T>
__device__ __forceinline__ r09_map_regs<T> r09_map_request(const T* __restrict__ R) {
    if constexpr (sizeof(T) == 4) {
        r09_map_regs<float> m;
        m.a = *reinterpret_cast<const r09_v16f_a4*>(R);
        m.b = *reinterpret_cast<const r09_v16f_a4*>(R + 16);
        m.c = *reinterpret_cast<const r09_v16f_a4*>(R + 32);
        m.d = R[48];
        return m;
    } else {
        return r09_map_regs<T>{R};
    }
}
// The kernel arguments a kernel needs behind its first branch, named here so that they are fetched with the first ones (the compiler
// otherwise sinks their loads to the first use: one more dependent round trip before the tile's address exists).
template <typename... A>
__device__ __forceinline__ void r09_args_now(A... a) { (..., [](auto v) { asm volatile("" ::"s"(v)); }(a)); }
// (the scheduler may not move an instruction across the barrier: the requests stay above what follows, the wait below what precedes)
__device__ __forceinline__ void r09_map_requested() { __builtin_amdgcn_sched_barrier(0); }
template <typename T>
__device__ __forceinline__ void r09_map_arrive(r09_map_regs<T>& m) {
    if constexpr (sizeof(T) == 4) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" : "+s"(m.a), "+s"(m.b), "+s"(m.c), "+s"(m.d));
    }
}

// blockIdx.x = b * tiles_per_row + t -> (b, t). One beam (B == 1: every tile index is below tiles_per_row, which the host computed)
// takes the uniform branch around the division.
__device__ __forceinline__ void r09_tile_of_block(unsigned tiles_per_row, unsigned& b, unsigned& t) {
    b = 0;
    t = blockIdx.x;
    if (t >= tiles_per_row) {
        b = t / tiles_per_row;
        t -= b * tiles_per_row;
    }
}

// y = R x, the fma chain j = 0..6 of chx_map7 (chx_common.h), for one row (X = T) or two rows side by side (X = chx_col16<T>::P);
// R: a pointer to the 49 entries or a r09_map_regs
template <typename T, typename X, typename M>
__device__ __forceinline__ void r09_map7(const M& R, const X (&x)[7], X (&y)[7]) {
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        X acc = x[0] * R[i * 7];
#pragma unroll
        for (int j = 1; j < 7; ++j) acc = __builtin_elementwise_fma((X)R[i * 7 + j], x[j], acc);
        y[i] = acc;
    }
}

// One column pass over a full column tile at g, TPn / (16 / sizeof(T)) lanes per workgroup. Column i goes back only if some lane
// of the wave holds a result whose bits differ from what it loaded: memory already holds exactly the bits a skipped store would
// have written, so the tile is bit for bit what storing everything leaves (NaN payloads, infinities and -0.0 included).
// g is read and written: no __restrict__. NT_LOAD: the beam does not stay in L2 from pass to pass, stream past it.
// R was requested by the caller (r09_map_request): the seven loads leave while it is in flight, one wait before the first FMA.
template <typename T, int TPn, bool NT_LOAD, bool NT_STORE = true>
__device__ __forceinline__ void r09_coltile_pass(T* g, r09_map_regs<T>& R) {
    using V = typename chx_col16<T>::V;
    using P = typename chx_col16<T>::P;
    constexpr int LANES = TPn / (16 / (int)sizeof(T));
    V* gv = reinterpret_cast<V*>(g) + threadIdx.x;
    V x[7], y[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = NT_LOAD ? __builtin_nontemporal_load(gv + j * LANES) : gv[j * LANES];
    r09_map_arrive<T>(R);
    if constexpr (sizeof(T) == 4) {
        P lo[7], hi[7], ylo[7], yhi[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) { lo[j] = x[j].xy; hi[j] = x[j].zw; }
        r09_map7<T, P>(R, lo, ylo);
        r09_map7<T, P>(R, hi, yhi);
#pragma unroll
        for (int j = 0; j < 7; ++j) { y[j].xy = ylo[j]; y[j].zw = yhi[j]; }
    } else {
        r09_map7<T, P>(R, x, y);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const chx_v4u d = __builtin_bit_cast(chx_v4u, y[j]) ^ __builtin_bit_cast(chx_v4u, x[j]);
        if (__any((d.x | d.y | d.z | d.w) != 0u)) {
            if (NT_STORE) __builtin_nontemporal_store(y[j], gv + j * LANES);
            else gv[j * LANES] = y[j];
        }
    }
}

template <typename T, int TPn, bool TO_COLUMNS>
__device__ __forceinline__ void r09_coltile_edge(T* g, r09_map_regs<T>& R, T* lds, int np, bool vec_ok) {
    constexpr int PPT = TPn / CHX_BLOCK;
    const bool full = np == TPn;
    const bool in_cols = full && !TO_COLUMNS, out_cols = full && TO_COLUMNS;
    tile_load<T, TPn>(g, lds, np * 7, vec_ok, false);
    r09_map_arrive<T>(R);        // requested by the caller before the tile: in scalar registers across the barriers
    __syncthreads();
    T y[PPT][7];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = threadIdx.x + k * CHX_BLOCK;
        if (p < np) {
            T x[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) x[j] = in_cols ? lds[j * TPn + p] : lds[p * 7 + j];
            r09_map7<T, T>(R, x, y[k]);
        }
    }
    if (full) __syncthreads();   // the layout changes: every lane has read its rows before another lane's results land on them
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int p = threadIdx.x + k * CHX_BLOCK;
        if (p < np) {
#pragma unroll
            for (int j = 0; j < 7; ++j) lds[out_cols ? j * TPn + p : p * 7 + j] = y[k][j];
        }
    }
    __syncthreads();
    tile_store<T, TPn>(g, lds, np * 7, vec_ok, true);
}

template <bool TO_COLUMNS>
__global__ __launch_bounds__(CHX_BLOCK) void k_edge_r09(float* x, const float* __restrict__ R, int64_t BR, int64_t N, unsigned tiles_per_row) {
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    r09_args_now(x, N);
    unsigned b, t;
    r09_tile_of_block(tiles_per_row, b, t);
    r09_map_regs<float> Rb = r09_map_request<float>(R + ((BR == 1) ? 0 : (int64_t)b) * 49);
    r09_map_requested();
    const int64_t n0 = (int64_t)t * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    r09_coltile_edge<float, TP, TO_COLUMNS>(x + ((int64_t)b * N + n0) * 7, Rb, lds, np, true);
}

template <bool NT_LOAD, bool NT_STORE>
__global__ __launch_bounds__(TP / 4) void k_col16_r09(float* x, const float* __restrict__ R, int64_t BR, int64_t N, unsigned tiles_per_row) {
    r09_args_now(x, N);
    unsigned b, t;
    r09_tile_of_block(tiles_per_row, b, t);
    const float* __restrict__ Rp = R + ((BR == 1) ? 0 : (int64_t)b) * 49;
    const int64_t n0 = (int64_t)t * TP;
    if (N - n0 >= TP) {
        r09_map_regs<float> Rb = r09_map_request<float>(Rp);
        r09_map_requested();
        r09_coltile_pass<float, TP, NT_LOAD, NT_STORE>(x + ((int64_t)b * N + n0) * 7, Rb);
    } else {
        chx_rowtile_pass<float>(x + ((int64_t)b * N + n0) * 7, Rp, (int)(N - n0));
    }
}

// the other lane shape: 256 lanes, two rows and 8 bytes per lane and column
__global__ __launch_bounds__(TP / 2) void k_col8(float* x, const float* __restrict__ R, long N) {
    const long n0 = (long)blockIdx.x * TP;
    if (N - n0 < TP) {
        chx_rowtile_pass<float>(x + n0 * 7, R, (int)(N - n0));
        return;
    }
    chx_v2f* gv = reinterpret_cast<chx_v2f*>(x + n0 * 7) + threadIdx.x;
    chx_v2f a[7], y[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) a[j] = gv[j * (TP / 2)];
    chx_map7<float, chx_v2f>(R, a, y);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const bool changed = __float_as_uint(a[j].x) != __float_as_uint(y[j].x) || __float_as_uint(a[j].y) != __float_as_uint(y[j].y);
        if (__any(changed)) __builtin_nontemporal_store(y[j], gv + j * (TP / 2));
    }
}

struct Stats { float mean, lo, hi; };

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "ab";
    const int E = 100, reps = 5;
    hipEvent_t t0, t1;
    CK(hipEventCreate(&t0)); CK(hipEventCreate(&t1));

    // the benchmark's cell at 100 MeV: Quadrupole(0.2, k1 = 4.2), Drift(0.8), Quadrupole(0.2, k1 = -4.2), Drift(0.8)
    auto drift = [](double L, float* R) {
        const double g = 1e8 / 510998.95, ig2 = 1.0 / (g * g), b2 = 1.0 - ig2;
        for (int i = 0; i < 49; ++i) R[i] = (i / 7 == i % 7) ? 1.f : 0.f;
        R[0 * 7 + 1] = (float)L; R[2 * 7 + 3] = (float)L; R[4 * 7 + 5] = (float)(-L / b2 * ig2);
    };
    auto quad = [&](double L, double k1, float* R) {
        drift(L, R);
        const double k = std::sqrt(std::fabs(k1)), c = std::cos(k * L), s = std::sin(k * L) / k, ch = std::cosh(k * L),
                     sh = std::sinh(k * L) / k;
        const int f = k1 > 0 ? 0 : 2, d = k1 > 0 ? 2 : 0;  // focusing / defocusing plane
        R[f * 7 + f] = (float)c; R[f * 7 + f + 1] = (float)s; R[(f + 1) * 7 + f] = (float)(-k * k * s); R[(f + 1) * 7 + f + 1] = (float)c;
        R[d * 7 + d] = (float)ch; R[d * 7 + d + 1] = (float)sh; R[(d + 1) * 7 + d] = (float)(k * k * sh); R[(d + 1) * 7 + d + 1] = (float)ch;
    };
    std::vector<float> fodo(E * 49), dense(E * 49), ident(E * 49);
    for (int e = 0; e < E; ++e) {
        if (e % 2) drift(0.8, &fodo[e * 49]);
        else quad(0.2, e % 4 ? -4.2 : 4.2, &fodo[e * 49]);
        for (int i = 0; i < 7; ++i)
            for (int j = 0; j < 7; ++j) {
                ident[e * 49 + i * 7 + j] = i == j ? 1.f : 0.f;
                // rows 0..5 dense (every column of a particle changes), row 6 keeps the 1
                dense[e * 49 + i * 7 + j] = i == j ? 1.f : (i < 6 ? 1e-3f * (float)(((i * 3 + j * 5 + e) % 7) - 3) : 0.f);
            }
    }
    float *dR[3];
    const std::vector<float>* hR[3] = {&fodo, &dense, &ident};
    const char* map_name[3] = {"FODO cell", "all of columns 0-5 change", "identity"};
    for (int m = 0; m < 3; ++m) {
        CK(hipMalloc(&dR[m], E * 196));
        CK(hipMemcpy(dR[m], hR[m]->data(), E * 196, hipMemcpyHostToDevice));
    }

    auto run_size = [&](long N, bool sweep) {
        const unsigned tiles = (unsigned)((N + TP - 1) / TP);
        const long bytes = N * 28;
        std::vector<float> hx(N * 7);
        for (long i = 0; i < N * 7; ++i) hx[i] = i % 7 == 6 ? 1.f : ((float)((i * 2654435761u) % 1000) * 1e-3f - 0.4995f) * 1e-3f;
        float *x0, *ref, *buf;
        CK(hipMalloc(&x0, bytes)); CK(hipMalloc(&ref, bytes)); CK(hipMalloc(&buf, bytes));
        CK(hipMemcpy(x0, hx.data(), bytes, hipMemcpyHostToDevice));
        std::vector<float> ha(N * 7), hb(N * 7);

        using Launch = std::function<void(float*, const float*)>;  // passes 1..E-1 in place on the buffer, maps R[1..E-1]
        auto rows_chain = [&](bool nt) {
            return Launch([=](float* x, const float* R) {
                for (int e = 1; e < E; ++e) {
                    if (nt) hipLaunchKernelGGL(k_rows<true>, dim3(tiles), dim3(CHX_BLOCK), 0, 0, x, R + e * 49, x, N);
                    else hipLaunchKernelGGL(k_rows<false>, dim3(tiles), dim3(CHX_BLOCK), 0, 0, x, R + e * 49, x, N);
                }
            });
        };
        Launch lib_chain = [=](float* x, const float* R) {
            for (int e = 1; e < E; ++e)
                if (chx_apply_affine7(x, R + e * 49, x, 1, 1, 1, N, CHX_F32, nullptr) != CHX_OK) { printf("chx_apply_affine7 failed\n"); exit(1); }
        };
        // 0: L2 loads, nt stores; 1: L2 loads, plain stores; 2: nt loads, nt stores; 3: 8 bytes per lane; 4: nt loads, plain stores
        // gen 0: the production kernels; 1: production edge passes, r09 column pass; 2: r09 edge passes and column pass
        const unsigned tpr = tiles;
        auto col_chain = [&](int kind, int gen = 0) {
            return Launch([=](float* x, const float* R) {
                const int64_t Nl = N, one = 1;
                const dim3 g(tiles), b16(TP / 4);
                if (gen == 2) hipLaunchKernelGGL(k_edge_r09<true>, g, dim3(CHX_BLOCK), 0, 0, x, R + 49, one, Nl, tpr);
                else hipLaunchKernelGGL(k_edge_prod<true>, g, dim3(CHX_BLOCK), 0, 0, x, R + 49, one, Nl);
                for (int e = 2; e < E - 1; ++e) {
                    const float* Re = R + e * 49;
                    if (kind == 3) hipLaunchKernelGGL(k_col8, g, dim3(TP / 2), 0, 0, x, Re, N);
                    else if (gen == 0) {
                        if (kind == 0) hipLaunchKernelGGL((k_col16_prod<false, true>), g, b16, 0, 0, x, Re, one, Nl);
                        else if (kind == 1) hipLaunchKernelGGL((k_col16_prod<false, false>), g, b16, 0, 0, x, Re, one, Nl);
                        else if (kind == 2) hipLaunchKernelGGL((k_col16_prod<true, true>), g, b16, 0, 0, x, Re, one, Nl);
                        else hipLaunchKernelGGL((k_col16_prod<true, false>), g, b16, 0, 0, x, Re, one, Nl);
                    } else if (kind == 0) hipLaunchKernelGGL((k_col16_r09<false, true>), g, b16, 0, 0, x, Re, one, Nl, tpr);
                    else hipLaunchKernelGGL((k_col16_r09<true, true>), g, b16, 0, 0, x, Re, one, Nl, tpr);
                }
                if (gen == 2) hipLaunchKernelGGL(k_edge_r09<false>, g, dim3(CHX_BLOCK), 0, 0, x, R + (E - 1) * 49, one, Nl, tpr);
                else hipLaunchKernelGGL(k_edge_prod<false>, g, dim3(CHX_BLOCK), 0, 0, x, R + (E - 1) * 49, one, Nl);
            });
        };
        auto full_run = [&](const Launch& l, float* out, const float* R) {
            hipLaunchKernelGGL(k_rows<true>, dim3(tiles), dim3(CHX_BLOCK), 0, 0, x0, R, out, N);  // pass 0
            l(out, R);
        };
        auto mismatches = [&](const Launch& l, const float* R) {
            full_run(rows_chain(true), ref, R);
            full_run(l, buf, R);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(ha.data(), ref, bytes, hipMemcpyDeviceToHost));
            CK(hipMemcpy(hb.data(), buf, bytes, hipMemcpyDeviceToHost));
            long bad = 0;
            for (long i = 0; i < N * 7; ++i) bad += memcmp(&ha[i], &hb[i], 4) != 0;
            return bad;
        };
        // the variants of one table alternate: run r of every variant before run r + 1 of any; us per in-place pass
        auto time_all = [&](const std::vector<Launch>& ls, const float* R) {
            std::vector<Stats> st(ls.size(), Stats{0.f, 1e30f, 0.f});
            for (const Launch& l : ls) full_run(l, buf, R);  // warm-up
            CK(hipDeviceSynchronize());
            for (int r = 0; r < reps; ++r)
                for (size_t v = 0; v < ls.size(); ++v) {
                    hipLaunchKernelGGL(k_rows<true>, dim3(tiles), dim3(CHX_BLOCK), 0, 0, x0, R, buf, N);
                    CK(hipEventRecord(t0, 0));
                    ls[v](buf, R);
                    CK(hipEventRecord(t1, 0));
                    CK(hipEventSynchronize(t1));
                    float ms;
                    CK(hipEventElapsedTime(&ms, t0, t1));
                    const float us = ms * 1e3f / (E - 1);
                    st[v].mean += us / reps;
                    st[v].lo = us < st[v].lo ? us : st[v].lo;
                    st[v].hi = us > st[v].hi ? us : st[v].hi;
                }
            return st;
        };
        auto report = [&](const char* name, const Stats& s, long bad) {
            printf("  %-58s %7.3f us/pass (min %7.3f max %7.3f)  mismatches=%ld\n", name, s.mean, s.lo, s.hi, bad);
            fflush(stdout);
        };
        if (!sweep) {
            const char* names[7] = {"(i) rows, L2 loads, nt stores [production MODE 3]", "columns, 16 B/lane, L2 loads, nt stores",
                                    "columns, 16 B/lane, L2 loads, plain stores", "columns, 16 B/lane, nt loads, nt stores",
                                    "columns, 8 B/lane (256 lanes), L2 loads, nt stores",
                                    "r09 pass: columns, L2 loads, nt stores, map prologue in the column pass",
                                    "r09 pass+edge: the same in the edge passes too"};
            const std::vector<Launch> ls = {rows_chain(false), col_chain(0), col_chain(1), col_chain(2), col_chain(3), col_chain(0, 1),
                                            col_chain(0, 2)};
            for (int m = 0; m < 3; ++m) {
                printf("N=%ld rows fp32 (%.1f MiB), %d in-place passes, maps: %s\n", N, bytes / 1048576.0, E - 1, map_name[m]);
                const std::vector<Stats> st = time_all(ls, dR[m]);
                for (size_t v = 0; v < ls.size(); ++v) report(names[v], st[v], mismatches(ls[v], dR[m]));
            }
        } else {
            const bool l2_range = bytes > 14L * 1024 * 1024 + 700 * 1024 && bytes <= 28L * 1024 * 1024;
            const std::vector<Launch> ls = {l2_range ? rows_chain(false) : lib_chain, col_chain(0), col_chain(1), col_chain(2), col_chain(4),
                                            col_chain(0, 1), col_chain(0, 2), col_chain(2, 2)};
            printf("N=%ld rows fp32 (%.1f MiB), FODO cell\n", N, bytes / 1048576.0);
            const std::vector<Stats> st = time_all(ls, dR[0]);
            report(l2_range ? "production in-place pass: rows, MODE 3" : "production in-place pass: libchx chx_apply_affine7", st[0],
                   mismatches(ls[0], dR[0]));
            report("columns, L2 loads, nt stores", st[1], mismatches(ls[1], dR[0]));
            report("columns, L2 loads, plain stores", st[2], mismatches(ls[2], dR[0]));
            report("columns, nt loads, nt stores", st[3], mismatches(ls[3], dR[0]));
            report("columns, nt loads, plain stores", st[4], mismatches(ls[4], dR[0]));
            report("r09 pass: columns, L2 loads, nt stores", st[5], mismatches(ls[5], dR[0]));
            report("r09 pass+edge: columns, L2 loads, nt stores", st[6], mismatches(ls[6], dR[0]));
            report("r09 pass+edge: columns, nt loads, nt stores", st[7], mismatches(ls[7], dR[0]));
        }
        CK(hipFree(x0)); CK(hipFree(ref)); CK(hipFree(buf));
    };

    // r10: whole calls (pass 0 + E - 1 in-place passes), us per pass = call / E
    auto run_r10 = [&](long N, bool sweep) {
        const unsigned tiles = (unsigned)((N + TP - 1) / TP);
        const long bytes = N * 28;
        const bool nt = bytes > 28L * 1024 * 1024;   // kL2ResidentBytes
        std::vector<float> hx(N * 7);
        for (long i = 0; i < N * 7; ++i) hx[i] = i % 7 == 6 ? 1.f : ((float)((i * 2654435761u) % 1000) * 1e-3f - 0.4995f) * 1e-3f;
        float *x0, *ref, *buf;
        unsigned* flags;
        CK(hipMalloc(&x0, bytes)); CK(hipMalloc(&ref, bytes)); CK(hipMalloc(&buf, bytes)); CK(hipMalloc(&flags, tiles * 4));
        CK(hipMemcpy(x0, hx.data(), bytes, hipMemcpyHostToDevice));
        std::vector<float> ha(N * 7), hb(N * 7);
        const int64_t Nl = N, one = 1;
        const dim3 g(tiles), b16(TP / 4), b256(CHX_BLOCK);
        // 0: production; 1: part 1; 2: part 2; 3: parts 1 and 2
        auto call = [&](int v, float* out, const float* R) {
            const bool first = v >= 2, flagged = v == 1 || v == 3;
            int e = 1;
            if (first) hipLaunchKernelGGL(k_enter_first, g, b256, 0, 0, x0, R, out, flags, Nl, one, one, 3);
            else {
                if (chx_apply_affine7(x0, R, out, 1, 1, 1, N, CHX_F32, nullptr) != CHX_OK) { printf("chx_apply_affine7 failed\n"); exit(1); }
                if (flagged) hipLaunchKernelGGL(k_enter, g, b256, 0, 0, out, R + 49, flags, Nl, one);
                else hipLaunchKernelGGL(k_edge_prod<true>, g, b256, 0, 0, out, R + 49, one, Nl);
                e = 2;
            }
            for (; e < E - 1; ++e) {
                const float* Re = R + e * 49;
                if (flagged) {
                    if (nt) hipLaunchKernelGGL(k_col16_flag<true>, g, b16, 0, 0, out, Re, flags, Nl, one);
                    else hipLaunchKernelGGL(k_col16_flag<false>, g, b16, 0, 0, out, Re, flags, Nl, one);
                } else {
                    if (nt) hipLaunchKernelGGL((k_col16_prod<true, true>), g, b16, 0, 0, out, Re, one, Nl);
                    else hipLaunchKernelGGL((k_col16_prod<false, true>), g, b16, 0, 0, out, Re, one, Nl);
                }
            }
            hipLaunchKernelGGL(k_edge_prod<false>, g, b256, 0, 0, out, R + (E - 1) * 49, one, Nl);
        };
        const char* names[4] = {"production: row pass 0, edge pass, column passes", "part 1: flags, six-column passes",
                                "part 2: pass 0 writes column tiles", "parts 1 + 2"};
        for (int m = 0; m < (sweep ? 1 : 3); ++m) {
            printf("N=%ld rows fp32 (%.1f MiB), whole call of %d passes, maps: %s\n", N, bytes / 1048576.0, E, map_name[m]);
            const float* R = dR[m];
            Stats st[4];
            float runs[4][8];
            for (int v = 0; v < 4; ++v) { st[v] = Stats{0.f, 1e30f, 0.f}; call(v, buf, R); }
            CK(hipDeviceSynchronize());
            // The first call behind a synchronise costs 150 - 250 us more than the same call later, whichever variant it is (seen run by
            // run in profiles/r10_const_column.md): one untimed call takes it. The starting variant rotates from run to run, so
            // that whatever else depends on the position in the sequence does not always meet the same variant.
            call(3, buf, R);
            for (int r = 0; r < reps; ++r)
                for (int i = 0; i < 4; ++i) {
                    const int v = (i + r) % 4;
                    CK(hipEventRecord(t0, 0));
                    call(v, buf, R);
                    CK(hipEventRecord(t1, 0));
                    CK(hipEventSynchronize(t1));
                    float ms;
                    CK(hipEventElapsedTime(&ms, t0, t1));
                    const float us = ms * 1e3f / E;
                    runs[v][r] = us;
                    st[v].mean += us / reps;
                    st[v].lo = us < st[v].lo ? us : st[v].lo;
                    st[v].hi = us > st[v].hi ? us : st[v].hi;
                }
            // the row structure: nt loads, nt stores, rows, in every pass
            for (int e = 0; e < E; ++e) hipLaunchKernelGGL(k_rows<true>, g, b256, 0, 0, e ? ref : x0, R + e * 49, ref, N);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(ha.data(), ref, bytes, hipMemcpyDeviceToHost));
            for (int v = 0; v < 4; ++v) {
                CK(hipMemset(flags, v & 1 ? 0xff : 0, tiles * 4));
                call(v, buf, R);
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(hb.data(), buf, bytes, hipMemcpyDeviceToHost));
                long bad = 0;
                for (long i = 0; i < N * 7; ++i) bad += memcmp(&ha[i], &hb[i], 4) != 0;
                printf("  %-58s %7.3f us/pass (min %7.3f max %7.3f)  mismatches=%ld\n", names[v], st[v].mean, st[v].lo, st[v].hi, bad);
                printf("      runs in order:");
                for (int r = 0; r < reps; ++r) printf(" %.3f", runs[v][r]);
                printf("\n");
                fflush(stdout);
            }
        }
        CK(hipFree(x0)); CK(hipFree(ref)); CK(hipFree(buf)); CK(hipFree(flags));
    };

    if (!strcmp(mode, "r10")) run_r10(argc > 2 ? atol(argv[2]) : 1000000, false);
    else if (!strcmp(mode, "r10sweep")) {
        for (long N : {300000L, 500000L, 600000L, 800000L, 1000000L, 1048576L, 1300000L, 1600000L, 3000000L, 3600000L, 16000000L}) run_r10(N, true);
    } else
    if (!strcmp(mode, "ab")) run_size(argc > 2 ? atol(argv[2]) : 1000000, false);
    else if (!strcmp(mode, "sweep")) {
        if (argc > 2) run_size(atol(argv[2]), true);
        else
            for (long N : {20000L, 50000L, 100000L, 300000L, 500000L, 800000L, 1000000L, 1048576L, 1300000L, 1600000L, 3000000L, 16000000L}) run_size(N, true);
    } else {
        printf("usage: apply_coltile ab [rows] | sweep [rows] | r10 [rows] | r10sweep\n");
        return 2;
    }
    for (int m = 0; m < 3; ++m) CK(hipFree(dR[m]));
    return 0;
}
