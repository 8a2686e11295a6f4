// chx_coltile.hip — the column-tiled in-place passes of chx_track_elementwise (passes 1..E-1; layout, flags and bodies: chx_common.h,
// column tiles). A translation unit of its own because it is compiled with kernel-argument preloading
// (-mllvm -amdgpu-kernarg-preload-count=8, see the Makefile): the 32 bytes of (x, R, BR, N) arrive in scalar registers with the
// wave instead of through a scalar load that every wave of a 2 - 5 us pass waits for before it can ask for anything else.
// Measured on MI355X, 1e6 fp32 rows, FODO cell (benchmarks/apply_coltile.hip built with and without the option, alternating;
// profiles/r09_map_prologue.md): 5.38 -> 4.88 us per pass, bench.py 0.529 - 0.568 -> 0.511 - 0.518 ms per step.
// r10: given scratch (one word per tile), pass 1 records which tiles hold nothing but 1 in column 6 and the column passes do not read
// that column there (coltile_enter_kernel, coltile_pass_flag_kernel; chx_common.h: chx_coltile_pass, FLAGGED). Measured the same way,
// whole 100-pass calls (profiles/r10_const_column.md): 4.96 -> 4.76 us per pass, bench.py 0.505 - 0.525 -> 0.485 - 0.498 ms per step.
#include "chx_common.h"
#include "chx_apply_tiles.h"

namespace {

// ---- column-tiled in-place passes (chx_common.h: column tiles) -----------------------------------------------------------
// Same tiling as apply_tile_kernel: workgroup blockIdx.x takes tile t of batch row b in every pass.
template <typename T> struct coltile_cfg {
    static constexpr int TP = tile_cfg<T>::PPT * CHX_BLOCK;          // rows per tile
    static constexpr int LANES = TP / (16 / (int)sizeof(T));         // lanes of a column pass: 16 bytes of every column each
};

// pass 1 (TO_COLUMNS) and pass E-1 of a call: [TP][7] -> [7][TP] and back, through LDS
template <typename T, bool TO_COLUMNS>
__global__ __launch_bounds__(CHX_BLOCK) void coltile_edge_kernel(T* x, const T* __restrict__ R, int64_t BR, int64_t N) {
    constexpr int TP = coltile_cfg<T>::TP;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    const chx_tile<TP> tc = chx_tile_coords<TP>(N);
    const int np = tc.np();
    T* g = x + (tc.b * N + tc.n0) * 7;
    chx_coltile_edge<T, TP, TO_COLUMNS>(g, g, R + ((BR == 1) ? 0 : tc.b) * 49, lds, np, true, false);
}

// passes 2..E-2: no LDS, no barrier, only the columns the map changed are stored
template <typename T, bool NT_LOAD>
__global__ __launch_bounds__(coltile_cfg<T>::LANES) void coltile_pass_kernel(T* x, const T* __restrict__ R, int64_t BR, int64_t N) {
    constexpr int TP = coltile_cfg<T>::TP;
    const chx_tile<TP> tc = chx_tile_coords<TP>(N);
    T* g = x + (tc.b * N + tc.n0) * 7;
    const T* __restrict__ Rb = R + ((BR == 1) ? 0 : tc.b) * 49;
    if (tc.full()) chx_coltile_pass<T, TP, NT_LOAD>(g, Rb);
    else chx_rowtile_pass<T>(g, Rb, (int)(N - tc.n0));
}

// ---- the same with one word of scratch per tile (chx_track_elementwise_scratch_bytes): flags[blockIdx.x] != 0 says that column
// 6 of the tile is all 1 in memory, and the pass does not read it (chx_common.h: chx_coltile_pass, FLAGGED). Kernels of their own,
// not a test of flags == nullptr in the ones above: the flagged full-tile path has no branch for the case it never sees, and a
// call without scratch runs the object code it always ran. The ten dwords of (x, R, flags, N, BR) are preloaded like the eight
// of the kernels above (the Makefile's preload count).
template <typename T, bool NT_LOAD>
__global__ __launch_bounds__(coltile_cfg<T>::LANES) void coltile_pass_flag_kernel(T* x, const T* __restrict__ R, unsigned* flags,
                                                                                  int64_t N, int64_t BR) {
    constexpr int TP = coltile_cfg<T>::TP;
    const chx_tile<TP> tc = chx_tile_coords<TP>(N);
    T* g = x + (tc.b * N + tc.n0) * 7;
    const T* __restrict__ Rb = R + ((BR == 1) ? 0 : tc.b) * 49;
    if (tc.full()) chx_coltile_pass<T, TP, NT_LOAD, true, true>(g, Rb, flags + blockIdx.x);
    else chx_rowtile_pass<T>(g, Rb, (int)(N - tc.n0));
}

// pass 1 with scratch: coltile_edge_kernel<T, true> that also writes the tile's flag (chx_common.h: chx_coltile_edge with FLAG, in place)
template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void coltile_enter_kernel(T* x, const T* __restrict__ R, unsigned* flags, int64_t N, int64_t BR) {
    constexpr int TP = coltile_cfg<T>::TP;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    const chx_tile<TP> tc = chx_tile_coords<TP>(N);
    const int np = tc.np();
    T* g = x + (tc.b * N + tc.n0) * 7;
    chx_coltile_edge<T, TP, true, true>(g, g, R + ((BR == 1) ? 0 : tc.b) * 49, lds, np, true, false, flags + blockIdx.x);
}

// Passes 1..E-1 of chx_track_elementwise through the column layout: needs E >= 3 and every batch row of x 16-byte aligned.
template <typename T>
bool coltile_ok(const void* x, int64_t E, int64_t B, int64_t N) {
    const int64_t bytes = B * N * 7 * (int64_t)sizeof(T);
    return E >= 3 && chx_aligned16(x) && (B == 1 || (N * 7 * (int64_t)sizeof(T)) % 16 == 0) &&
           bytes >= kColTileMinBytes;
}

template <typename T>
size_t coltile_scratch_bytes(int64_t B, int64_t N) {
    if (B < 1 || N < 1 || B * N * 7 * (int64_t)sizeof(T) < kColTileMinBytes) return 0;
    constexpr int TP = coltile_cfg<T>::TP;
    return (size_t)(((N + TP - 1) / TP) * B) * sizeof(unsigned);
}

// flags: nullptr (seven loads in every pass, the kernels and the object code of a call without scratch) or one word per tile
template <typename T>
int launch_coltile_passes(void* x, const void* R, unsigned* flags, int64_t E, int64_t B, int64_t BR, int64_t N, hipStream_t s) {
    constexpr int TP = coltile_cfg<T>::TP;
    const int64_t tiles = ((N + TP - 1) / TP) * B;
    if (tiles > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
    const bool nt_load = B * N * 7 * (int64_t)sizeof(T) > kL2ResidentBytes;
    const T* Rp = (const T*)R;
    const int64_t estride = BR * 49;
    const dim3 grid((unsigned)tiles), lanes(coltile_cfg<T>::LANES);
    if (flags) hipLaunchKernelGGL((coltile_enter_kernel<T>), grid, dim3(CHX_BLOCK), 0, s, (T*)x, Rp + estride, flags, N, BR);
    else hipLaunchKernelGGL((coltile_edge_kernel<T, true>), grid, dim3(CHX_BLOCK), 0, s, (T*)x, Rp + estride, BR, N);
    for (int64_t e = 2; e < E - 1; ++e) {
        if (flags) {
            if (nt_load) hipLaunchKernelGGL((coltile_pass_flag_kernel<T, true>), grid, lanes, 0, s, (T*)x, Rp + e * estride, flags, N, BR);
            else hipLaunchKernelGGL((coltile_pass_flag_kernel<T, false>), grid, lanes, 0, s, (T*)x, Rp + e * estride, flags, N, BR);
        } else {
            if (nt_load) hipLaunchKernelGGL((coltile_pass_kernel<T, true>), grid, lanes, 0, s, (T*)x, Rp + e * estride, BR, N);
            else hipLaunchKernelGGL((coltile_pass_kernel<T, false>), grid, lanes, 0, s, (T*)x, Rp + e * estride, BR, N);
        }
    }
    hipLaunchKernelGGL((coltile_edge_kernel<T, false>), grid, dim3(CHX_BLOCK), 0, s, (T*)x, Rp + (E - 1) * estride, BR, N);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace

bool chx_coltile_ok(const void* x, int64_t E, int64_t B, int64_t N, int dtype) {
    return dtype == CHX_F32 ? coltile_ok<float>(x, E, B, N) : coltile_ok<double>(x, E, B, N);
}

size_t chx_coltile_scratch_bytes(int64_t B, int64_t N, int dtype) {
    return dtype == CHX_F32 ? coltile_scratch_bytes<float>(B, N) : coltile_scratch_bytes<double>(B, N);
}

int chx_coltile_passes(void* x, const void* R, void* flags, int64_t E, int64_t B, int64_t BR, int64_t N, int dtype, hipStream_t s) {
    return dtype == CHX_F32 ? launch_coltile_passes<float>(x, R, (unsigned*)flags, E, B, BR, N, s)
                            : launch_coltile_passes<double>(x, R, (unsigned*)flags, E, B, BR, N, s);
}
