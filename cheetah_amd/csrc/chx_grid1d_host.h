// chx_grid1d_host.h — host code shared by the entry points of the kicks that bin the beam's charge on M nodes in tau (chx_wake.hip,
// chx_csr.hip, chx_lsc.hip): the argument check, the workspace layout, the float / double dispatch and the launchers of the particle
// passes of chx_grid1d_dev.h and of the low-pass stage of the calls with a cutoff. A kick adds its own conditions, its own block of
// the workspace and its Toeplitz launch in between.
#pragma once
#include "chx_grid1d_dev.h"

namespace {

// The conditions every entry point of the family puts on the particles, the batch sizes, the grid and the state.
int check_grid1d(const void* x, const void* q, const void* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int32_t M,
                 int dtype, const double* state) {
    if (!x || !q || !w || !state || B < 1 || B > 65535 || N < 1 || N > 0x7fffffffLL || M < 2 || M > CHX_WAKE_MAX_BINS)
        return CHX_ERR_INVALID_ARG;
    if (!chx_bcast_ok(Bx, B) || !chx_bcast_ok(Bq, B) || !chx_bcast_ok(Bw, B)) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!chx_aligned16(x)) return CHX_ERR_MISALIGNED;
    return CHX_OK;
}

// The workspace of a kick with `channels` deposit channels (1, or the wake's 3: Q, X, Y) and a block of its own behind the common
// arrays. bytes = 0 for sizes no entry point accepts.
struct Grid1dWs {
    double* part;               // [B][G][kPart] forward partials
    unsigned long long* grid;   // [B][channels][M] fixed-point deposit
    double* bpart;              // [B][G][kPart] backward partials
    double* bhdr;               // [B][kHdr] backward header: valid, S per channel of the cotangent deposit
    unsigned long long* ggrid;  // [B][channels][M] fixed-point cotangents of the node kicks
    double* adj;                // [B][channels][M] cotangents of the deposits
    double* extra;              // the caller's block of extra_bytes
    size_t bytes;
    const double* adj_last;     // what a kick's last backward pass reads: adj, or the filtered cotangents of a call with a cutoff
    // a call with a cutoff (with_cutoff): the cutoff wavelengths (m) of the low-pass stage, [Bc] with Bc = 1 or B, and its block
    // behind everything else, [B][channels][M] of 8 bytes: the raw deposit, then the filtered cotangents. Null: no stage
    const double* cutoff;
    int64_t Bc;
    unsigned long long* raw;
};

Grid1dWs grid1d_ws(void* base, int64_t B, int64_t N, int M, int channels, size_t extra_bytes) {
    Grid1dWs w = {};
    if (B < 1 || N < 1 || M < 2 || M > CHX_WAKE_MAX_BINS) return w;
    char* p = (char*)base;
    size_t o = 0;
    auto take = [&](size_t nbytes) { char* r = p ? p + o : nullptr; o += al256(nbytes); return r; };
    const int G = wake_groups(N);
    w.part = (double*)take((size_t)(B * G * kPart) * 8);
    w.grid = (unsigned long long*)take((size_t)(B * channels * M) * 8);
    w.bpart = (double*)take((size_t)(B * G * kPart) * 8);
    w.bhdr = (double*)take((size_t)(B * kHdr) * 8);
    w.ggrid = (unsigned long long*)take((size_t)(B * channels * M) * 8);
    w.adj = (double*)take((size_t)(B * channels * M) * 8);
    w.extra = (double*)take(extra_bytes);
    w.bytes = o;
    w.adj_last = w.adj;
    return w;
}

// The workspace of a call that takes a cutoff: `ws` with the stage's block behind it. Without a cutoff (null) it is `ws` itself.
inline size_t cutoff_ws_bytes(const Grid1dWs& ws, int64_t B, int M, int channels) {
    return ws.bytes ? ws.bytes + al256((size_t)(B * channels * M) * 8) : 0;
}
inline Grid1dWs with_cutoff(Grid1dWs ws, void* base, int64_t B, int M, int channels, const double* cutoff, int64_t Bc) {
    if (!cutoff || !ws.bytes) return ws;
    ws.raw = base ? (unsigned long long*)((char*)base + ws.bytes) : nullptr;
    ws.bytes = cutoff_ws_bytes(ws, B, M, channels);
    ws.adj_last = (const double*)ws.raw;
    ws.cutoff = cutoff;
    ws.Bc = Bc;
    return ws;
}
inline bool cutoff_ok(const double* cutoff, int64_t Bc, int64_t B) { return !cutoff || chx_bcast_ok(Bc, B); }

// Dynamic LDS above 64 KiB (M > ~2700 nodes) must be requested per kernel (gfx950: 160 KiB per workgroup).
template <typename K>
bool lds_ok(K kern, size_t bytes) {
    return bytes <= 64 * 1024 ||
           hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

inline dim3 grid_groups(int64_t N, int64_t B) { return dim3((unsigned)wake_groups(N), (unsigned)B); }       // F1, F2, B1, B2
inline dim3 grid_particles(int64_t N, int64_t B) { return dim3((unsigned)((N + kWB - 1) / kWB), (unsigned)B); }
inline dim3 grid_nodes(int M, int64_t B) { return dim3((unsigned)((M + kNodeBlock - 1) / kNodeBlock), (unsigned)B); }

// The low-pass stage of a call with a cutoff, every channel of the row: the raw deposit into the grid the node pass reads (kFixed), or
// the cotangents `adj` into what the last particle pass reads. Nothing without a cutoff.
template <bool kFixed>
int launch_filter(int64_t B, int M, int channels, int64_t state_row, const double* state, const void* src, void* dst,
                  const Grid1dWs& ws, hipStream_t s) {
    if (!ws.cutoff) return CHX_OK;
    const size_t lds = ((size_t)M + kWB / 64 + 1 + kWB + 2 * (size_t)(M - 1)) * 8;    // weights, sums, the widest window
    if (!lds_ok(grid_filter_kernel<kFixed>, lds)) return CHX_ERR_LAUNCH;
    hipLaunchKernelGGL(grid_filter_kernel<kFixed>, dim3((unsigned)((M + kWB - 1) / kWB), (unsigned)B, (unsigned)channels), dim3(kWB),
                       lds, s, ws.cutoff, ws.Bc, M, channels, state, state_row, src, dst);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}
// Between a kick's adjoint node pass (which wrote ws.adj) and its last particle pass (which reads ws.adj_last).
inline int launch_adj_filter(int64_t B, int M, int channels, int64_t state_row, const double* state, const Grid1dWs& ws,
                             hipStream_t s) {
    return launch_filter<false>(B, M, channels, state_row, state, ws.adj, ws.raw, ws, s);
}

// F1 and F2 (and the low-pass stage of a call with a cutoff): channels ch0 ... ch0 + nch - 1 of the `channels` the row's grid holds;
// state_row doubles per state row.
template <typename T>
int launch_deposit(const T* x, const T* q, const T* w, int64_t B, int64_t Bx, int64_t Bq, int64_t Bw, int64_t N, int M, int ch0,
                   int nch, int channels, int64_t state_row, double* state, const Grid1dWs& ws, hipStream_t s) {
    const int G = wake_groups(N);
    const size_t lds = (size_t)nch * M * 8;
    unsigned long long* dep = ws.cutoff ? ws.raw : ws.grid;          // with a cutoff the stage forms ws.grid from the raw deposit
    if (!lds_ok(wake_deposit_kernel<T>, lds)) return CHX_ERR_LAUNCH;
    hipLaunchKernelGGL(wake_range_kernel<T>, grid_groups(N, B), dim3(kWB), 0, s, x, q, w, Bx, Bq, Bw, N, G, M, (int)(ch0 + nch == 3),
                       (int64_t)channels * M, ws.part, dep);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(wake_deposit_kernel<T>, grid_groups(N, B), dim3(kWB), lds, s, x, q, w, Bx, Bq, Bw, N, G, M, ch0, nch, state_row,
                       (int64_t)channels * M, ws.part, state, dep);
    CHX_CHECK_LAUNCH();
    return launch_filter<true>(B, M, channels, state_row, state, ws.raw, ws.grid, ws, s);
}

// F4 of the single-channel kicks.
template <typename T>
int launch_node_kick(const T* x, int64_t B, int64_t Bx, int64_t N, int M, int64_t state_row, const double* state, T* out,
                     hipStream_t s) {
    hipLaunchKernelGGL(node_kick_kernel<T>, grid_particles(N, B), dim3(kWB), 0, s, x, Bx, N, M, state, state_row, out);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

// B1 and B2 of the single-channel kicks (B4 is one launch: node_bwd_particles_kernel, or the kick's own kernel around it).
template <typename T>
int launch_node_bwd_deposit(const T* x, int64_t B, int64_t Bx, int64_t N, int M, int64_t state_row, const double* state,
                            const T* gout, double* d_scale, const Grid1dWs& ws, hipStream_t s) {
    const int G = wake_groups(N);
    const size_t lds = (size_t)M * 8;
    if (!lds_ok(node_bwd_deposit_kernel<T>, lds)) return CHX_ERR_LAUNCH;
    hipLaunchKernelGGL(node_bwd_range_kernel<T>, grid_groups(N, B), dim3(kWB), 0, s, x, Bx, N, G, M, state, state_row, gout, ws.bpart,
                       ws.ggrid);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(node_bwd_deposit_kernel<T>, grid_groups(N, B), dim3(kWB), lds, s, x, Bx, N, G, M, state, state_row,
                       gout, ws.bpart, ws.bhdr, d_scale, ws.ggrid);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

}  // namespace
