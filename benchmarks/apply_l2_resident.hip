// apply_l2_resident.hip — can element-by-element passes read the beam from the XCDs' L2 instead of the Infinity Cache?
//
// chx_track_elementwise runs passes 1..E-1 in place on one buffer (28 MB at 1e6 fp32 rows: 3.5 MB per XCD, each XCD
// has 4 MiB of L2). The production tile kernel reads and writes non-temporally and lets any XCD take any tile, so every
// pass misses L2. This harness times 100 in-place passes back to back (HIP events) for:
//   (a) the production apply_tile_kernel<float,2,0> structure (nt loads, nt stores, one 512-row tile per workgroup);
//   (b) an XCD-affine persistent kernel: the tiles are split into 8 contiguous slices, a workgroup reads its XCC id and
//       claims tiles of that XCD's slice through a per-XCD atomic head, then steals from the other seven slices, so every
//       tile is done exactly once under any placement; nt loads, nt stores;
//   (c) (b) with default-policy (L2-allocating) loads;
//   (d) (c) with default-policy (write-back) stores;
//   (e) (c) with 16-byte sc1 (write-through) stores;
//   (f)-(h) no claims: (a)'s one tile per workgroup with the load / store policies of (c)-(e), grid rounded to a multiple
//       of 8; (i) = (f) on the bare tile grid; (j) = (i) with every tile moved to another XCD each pass (a control);
// every one checked bit for bit against (a) after the same number of passes. The affine kernel also runs on grids of
// 1, 7 and 9 workgroups (2 and 3 passes), which exercises the stealing path. Results: profiles/r07_l2_resident.md.
//
// Build and run (no arguments = everything; `apply_l2_resident acd [grid [rows]]` runs the listed variants, e.g. for a profiler):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Icheetah_amd/csrc -Iinclude \
//         benchmarks/apply_l2_resident.hip -o apply_l2_resident
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "chx_common.h"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

constexpr int TP = 512;           // rows per tile (PPT = 2), as tile_cfg<float>
constexpr int HEAD_STRIDE = 32;   // one head per 128-byte line
constexpr int HEAD_SET = 8 * HEAD_STRIDE;

__device__ __forceinline__ void apply7(const float* __restrict__ R, const float (&x)[7], float (&y)[7]) {
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        float acc = R[i * 7] * x[0];
#pragma unroll
        for (int j = 1; j < 7; ++j) acc = fmaf(R[i * 7 + j], x[j], acc);
        y[i] = acc;
    }
}

__device__ __forceinline__ void apply_lds_tile(const float* __restrict__ R, float* lds, int np) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int p = threadIdx.x + k * CHX_BLOCK;
        if (p < np) {
            float x[7], y[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) x[j] = lds[p * 7 + j];
            apply7(R, x, y);
#pragma unroll
            for (int j = 0; j < 7; ++j) lds[p * 7 + j] = y[j];
        }
    }
}

// (a) the production structure: one tile per workgroup, nt loads and stores (apply_tile_kernel<float,2,0>, B = 1)
__global__ __launch_bounds__(CHX_BLOCK) void k_prod(const float* x_in, const float* __restrict__ R, float* x_out, long N) {
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    const long n0 = (long)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    tile_load<float, TP>(x_in + n0 * 7, lds, np * 7, true, true);
    __syncthreads();
    apply_lds_tile(R, lds, np);
    __syncthreads();
    tile_store<float, TP>(x_out + n0 * 7, lds, np * 7, true, true);
}

typedef float v4f __attribute__((ext_vector_type(4)));

template <int SP>
__device__ __forceinline__ void store16(float4 a, float4* p) {
    if (SP == 0) chx_nt_store(a, p);
    else if (SP == 1) *p = a;
    else {
        const v4f d = {a.x, a.y, a.z, a.w};
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(reinterpret_cast<v4f*>(p)), "v"(d) : "memory");
    }
}

// LP: 0 = nt loads, 1 = default policy. SP: 0 = nt stores, 1 = default (write-back), 2 = sc1 (write-through).
template <int LP, int SP>
__global__ __launch_bounds__(CHX_BLOCK) void k_affine(float* x, const float* __restrict__ R, long N, unsigned* heads,
                                                      int parity) {
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    __shared__ long s_next;
    const long tiles = (N + TP - 1) / TP;
    unsigned* head = heads + parity * HEAD_SET;
    // the other set was last used by the previous pass, which has finished: zero it for the next one
    if (blockIdx.x == 0 && threadIdx.x < 8)
        __hip_atomic_store(heads + (parity ^ 1) * HEAD_SET + threadIdx.x * HEAD_STRIDE, 0u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    int xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
    int k = 0;  // slices given up so far (thread 0 only): own slice first, then the other seven in turn
    auto claim = [&]() -> long {
        while (k < 8) {
            const int s = (xcc + k) & 7;
            const long lo = tiles * s / 8, hi = tiles * (s + 1) / 8;
            // a drained slice is skipped on a plain read: an atomic on an exhausted head is the one that costs
            if (lo + (long)__hip_atomic_load(head + s * HEAD_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= hi) {
                ++k;
                continue;
            }
            const unsigned i = __hip_atomic_fetch_add(head + s * HEAD_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (lo + (long)i < hi) return lo + i;
            ++k;
        }
        return -1;
    };
    if (threadIdx.x == 0) s_next = claim();
    __syncthreads();
    long t = s_next;
    while (t >= 0) {
        const long n0 = t * TP;
        const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
        const int nvec = np * 7 / 4;
        float* g = x + n0 * 7;
        const float4* gv = reinterpret_cast<const float4*>(g);
        float4* lv = reinterpret_cast<float4*>(lds);
        for (int v = threadIdx.x; v < nvec; v += CHX_BLOCK) lv[v] = LP == 0 ? chx_nt_load(gv + v) : gv[v];
        for (int e = nvec * 4 + threadIdx.x; e < np * 7; e += CHX_BLOCK) lds[e] = g[e];
        __syncthreads();
        if (threadIdx.x == 0) s_next = claim();  // the next claim's latency hides behind this tile's arithmetic
        apply_lds_tile(R, lds, np);
        __syncthreads();
        t = s_next;
        for (int v = threadIdx.x; v < nvec; v += CHX_BLOCK) store16<SP>(lv[v], reinterpret_cast<float4*>(g) + v);
        for (int e = nvec * 4 + threadIdx.x; e < np * 7; e += CHX_BLOCK) g[e] = lds[e];
        __syncthreads();  // s_next is rewritten and lds refilled only after every lane has read them
    }
}

// (f)-(h) no claiming at all: the production one-tile-per-workgroup kernel with the load / store policy of (c)-(e) and the
// grid rounded up to a multiple of 8 (surplus workgroups exit). Tile t then always goes to workgroup t, and workgroups
// b and b + 8 share an XCD; whether tile t stays on ONE XCD from pass to pass depends on where the dispatcher deals
// workgroup 0, which workgroups 0..7 record in xcc_log[pass][8]. (i) is (f) without the rounding.
// shift != 0 (variant j, a control): workgroup b takes tile (b + shift) % tiles, so a tile moves to another XCD every pass.
template <int LP, int SP>
__global__ __launch_bounds__(CHX_BLOCK) void k_tile_pol(float* x, const float* __restrict__ R, long N, int* xcc_log, int shift) {
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    if (xcc_log && blockIdx.x < 8 && threadIdx.x == 0) {
        int xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
        xcc_log[blockIdx.x] = xcc;
    }
    const long tiles = (N + TP - 1) / TP;
    if ((long)blockIdx.x >= tiles) return;
    const long n0 = (((long)blockIdx.x + shift) % tiles) * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    const int nvec = np * 7 / 4;
    float* g = x + n0 * 7;
    const float4* gv = reinterpret_cast<const float4*>(g);
    float4* lv = reinterpret_cast<float4*>(lds);
    for (int v = threadIdx.x; v < nvec; v += CHX_BLOCK) lv[v] = LP == 0 ? chx_nt_load(gv + v) : gv[v];
    for (int e = nvec * 4 + threadIdx.x; e < np * 7; e += CHX_BLOCK) lds[e] = g[e];
    __syncthreads();
    apply_lds_tile(R, lds, np);
    __syncthreads();
    for (int v = threadIdx.x; v < nvec; v += CHX_BLOCK) store16<SP>(lv[v], reinterpret_cast<float4*>(g) + v);
    for (int e = nvec * 4 + threadIdx.x; e < np * 7; e += CHX_BLOCK) g[e] = lds[e];
}

struct Variant { char id; const char* name; void (*k)(float*, const float*, long, unsigned*, int); };

int main(int argc, char** argv) {
    const long N = argc > 3 ? atol(argv[3]) : 1000000;
    const int E = 100, reps = 5;
    const char* only = argc > 1 ? argv[1] : nullptr;
    const int grid_arg = argc > 2 ? atoi(argv[2]) : 0;
    int cus = 0;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));

    std::vector<float> hx(N * 7), hR(E * 49);
    for (long i = 0; i < N * 7; ++i) hx[i] = (float)((i * 2654435761u) % 1000) * 1e-3f - 0.5f;
    for (int e = 0; e < E; ++e)
        for (int i = 0; i < 7; ++i)
            for (int j = 0; j < 7; ++j)
                hR[e * 49 + i * 7 + j] = (i == j) ? 1.f : 1e-3f * (float)(((i * 3 + j * 5 + e) % 7) - 3);
    float *x0, *ref, *buf, *R;
    unsigned* heads;
    CK(hipMalloc(&x0, N * 28)); CK(hipMalloc(&ref, N * 28)); CK(hipMalloc(&buf, N * 28));
    CK(hipMalloc(&R, E * 196)); CK(hipMalloc(&heads, 2 * HEAD_SET * sizeof(unsigned)));
    CK(hipMemcpy(x0, hx.data(), N * 28, hipMemcpyHostToDevice));
    CK(hipMemcpy(R, hR.data(), E * 196, hipMemcpyHostToDevice));
    hipEvent_t t0, t1;
    CK(hipEventCreate(&t0)); CK(hipEventCreate(&t1));
    const unsigned tiles = (unsigned)((N + TP - 1) / TP);

    // (a) pass 0 x0 -> buf, passes 1..E-1 in place (chx_track_elementwise); also the bitwise reference for `passes`
    auto run_prod = [&](float* out, int passes) {
        hipLaunchKernelGGL(k_prod, dim3(tiles), dim3(CHX_BLOCK), 0, 0, x0, R, out, N);
        for (int e = 1; e < passes; ++e) hipLaunchKernelGGL(k_prod, dim3(tiles), dim3(CHX_BLOCK), 0, 0, out, R + e * 49, out, N);
    };
    // the affine kernels: pass 0 as (a), passes 1.. in place through the affine kernel, one memset of both head sets
    auto run_affine = [&](const Variant& v, int grid, int passes) {
        CK(hipMemsetAsync(heads, 0, 2 * HEAD_SET * sizeof(unsigned), 0));
        hipLaunchKernelGGL(k_prod, dim3(tiles), dim3(CHX_BLOCK), 0, 0, x0, R, buf, N);
        for (int e = 1; e < passes; ++e) hipLaunchKernelGGL(v.k, dim3(grid), dim3(CHX_BLOCK), 0, 0, buf, R + e * 49, N, heads, e & 1);
    };
    auto mismatches = [&](int passes) {
        run_prod(ref, passes);
        CK(hipDeviceSynchronize());
        std::vector<float> a(N * 7), b(N * 7);
        CK(hipMemcpy(a.data(), ref, N * 28, hipMemcpyDeviceToHost));
        CK(hipMemcpy(b.data(), buf, N * 28, hipMemcpyDeviceToHost));
        long bad = 0;
        for (long i = 0; i < N * 7; ++i) bad += memcmp(&a[i], &b[i], sizeof(float)) != 0;
        return bad;
    };
    auto time_runs = [&](auto launch) {
        launch();  // warm-up
        CK(hipDeviceSynchronize());
        float best = 1e30f, sum = 0.f;
        for (int r = 0; r < reps; ++r) {
            CK(hipMemcpyAsync(buf, x0, N * 28, hipMemcpyDeviceToDevice, 0));
            CK(hipEventRecord(t0, 0));
            launch();
            CK(hipEventRecord(t1, 0));
            CK(hipEventSynchronize(t1));
            float ms;
            CK(hipEventElapsedTime(&ms, t0, t1));
            sum += ms;
            best = ms < best ? ms : best;
        }
        return std::make_pair(sum / reps * 1e3f / E, best * 1e3f / E);  // us per pass: mean, best
    };

    const Variant vs[] = {{'b', "affine nt load, nt store", k_affine<0, 0>},
                          {'c', "affine L2 load, nt store", k_affine<1, 0>},
                          {'d', "affine L2 load, write-back store", k_affine<1, 1>},
                          {'e', "affine L2 load, sc1 store", k_affine<1, 2>}};
    printf("N=%ld rows fp32, %d passes in place, %d CUs, %u tiles of %d rows\n", N, E, cus, tiles, TP);
    if (!only || strchr(only, 'a')) {
        auto t = time_runs([&] { run_prod(buf, E); });
        printf("(a) production tile kernel             grid=%6u  %7.3f us/pass (best %7.3f)  %6.2f TB/s\n", tiles, t.first,
               t.second, 56.0 * N / (t.first * 1e-6) / 1e12);
        fflush(stdout);
    }
    for (const Variant& v : vs) {
        if (only && !strchr(only, v.id)) continue;
        std::vector<int> grids;
        if (grid_arg) grids = {grid_arg};
        else grids = {cus, cus * 2, cus * 4, cus * 6};
        for (int g : grids) {
            auto t = time_runs([&] { run_affine(v, g, E); });
            const long bad = mismatches(E);
            printf("(%c) %-35s grid=%6d  %7.3f us/pass (best %7.3f)  %6.2f TB/s  mismatches=%ld\n", v.id, v.name, g, t.first,
                   t.second, 56.0 * N / (t.first * 1e-6) / 1e12, bad);
            fflush(stdout);
        }
        if (!grid_arg && v.id == 'c') {
            for (int g : {1, 7, 9}) {  // few workgroups: most tiles are taken from other XCDs' slices
                for (int passes : {2, 3}) {
                    run_affine(v, g, passes);
                    printf("(%c) stealing check grid=%d passes=%d  mismatches=%ld\n", v.id, g, passes, mismatches(passes));
                }
            }
        }
    }
    // (f)-(i): placement only, no claims. Grid = tiles rounded up to a multiple of 8 (f-h) or the bare tile count (i)
    struct TileVariant { char id; const char* name; void (*k)(float*, const float*, long, int*, int); bool pad; int shift; };
    const TileVariant tvs[] = {{'f', "tile L2 load, nt store, grid%8=0", k_tile_pol<1, 0>, true, 0},
                               {'g', "tile L2 load, write-back, grid%8=0", k_tile_pol<1, 1>, true, 0},
                               {'h', "tile L2 load, sc1 store, grid%8=0", k_tile_pol<1, 2>, true, 0},
                               {'i', "tile L2 load, nt store, grid=tiles", k_tile_pol<1, 0>, false, 0},
                               {'j', "(i), tiles moved across XCDs", k_tile_pol<1, 0>, false, 1}};
    int* xlog;
    CK(hipMalloc(&xlog, E * 8 * sizeof(int)));
    for (const TileVariant& v : tvs) {
        if (only && !strchr(only, v.id)) continue;
        const unsigned g = v.pad ? (tiles + 7) / 8 * 8 : tiles;
        auto launch = [&](int passes) {
            hipLaunchKernelGGL(k_prod, dim3(tiles), dim3(CHX_BLOCK), 0, 0, x0, R, buf, N);
            for (int e = 1; e < passes; ++e)
                hipLaunchKernelGGL(v.k, dim3(g), dim3(CHX_BLOCK), 0, 0, buf, R + e * 49, N, xlog + e * 8, v.shift * e);
        };
        auto t = time_runs([&] { launch(E); });
        const long bad = mismatches(E);
        std::vector<int> hl(E * 8);
        CK(hipMemcpy(hl.data(), xlog, E * 8 * sizeof(int), hipMemcpyDeviceToHost));
        int moved = 0;  // passes whose workgroup 0 ran on another XCD than in the pass before
        for (int e = 2; e < E; ++e) moved += hl[e * 8] != hl[(e - 1) * 8];
        printf("(%c) %-35s grid=%6u  %7.3f us/pass (best %7.3f)  %6.2f TB/s  mismatches=%ld  wg0 changed XCD in %d of %d passes;"
               " XCC of wg 0..7 in passes 1-3: ", v.id, v.name, g, t.first, t.second, 56.0 * N / (t.first * 1e-6) / 1e12, bad,
               moved, E - 2);
        for (int e = 1; e <= 3; ++e) {
            for (int b = 0; b < 8; ++b) printf("%d", hl[e * 8 + b]);
            printf(" ");
        }
        printf("\n");
        fflush(stdout);
    }
    CK(hipFree(xlog));
    CK(hipFree(x0)); CK(hipFree(ref)); CK(hipFree(buf)); CK(hipFree(R)); CK(hipFree(heads));
    return 0;
}
