// chx_apply_tiles.h — tile shapes and size thresholds of the apply kernels, shared by chx_apply.hip and chx_coltile.hip.
#pragma once
#include "chx_common.h"

template <typename T> struct tile_cfg;
template <> struct tile_cfg<float> { static constexpr int PPT = 2; };   // 512 rows, 14 KiB LDS
template <> struct tile_cfg<double> { static constexpr int PPT = 1; };  // 256 rows, 14 KiB LDS

// Beams up to this size take the wave-staged MODE-0 kernel (launch_tiles).
constexpr int64_t kSmallBeamBytes = (int64_t)14 * 1024 * 1024 + 700 * 1024;
// In-place element passes on beams up to this size run as MODE 3 (launch_inplace_pass): 7/8 of the 8 x 4 MiB of L2.
constexpr int64_t kL2ResidentBytes = (int64_t)28 * 1024 * 1024;
// Calls of chx_track_elementwise with E >= 3 on beams from this size on run passes 1..E-1 column-tiled (launch_coltile_passes).
// Measured on MI355X, fp32, FODO cell, us per in-place pass, production pass -> column passes (benchmarks/apply_coltile.hip,
// profiles/r08_coltile.md): 3e5 rows 3.60 -> 3.01, 5e5 6.14 -> 3.48, 1e6 7.37 -> 5.38, 1.6e6 14.5 -> 10.6, 1.6e7 142 -> 113;
// at 1e5 rows and below both sit on the launch floor (2.6 - 3.0 us, inside each other's spread) and the row passes stay.
constexpr int64_t kColTileMinBytes = (int64_t)8 * 1024 * 1024;

// Pass 0 of such a call stays the row pass above at every size: a pass 0 that writes the column tiles itself (chx_coltile_edge from
// x_in, which makes pass 1 an ordinary column pass) was measured in benchmarks/apply_coltile.hip (r10, part 2), us per pass of a
// whole 100-pass call with / without it: 1e6 rows 4.88 / 4.84, 1.3e6 8.03 / 7.90, 3e6 18.77 / 18.86, 1.6e7 102.9 / 103.2
// (profiles/r10_const_column.md): inside the spreads everywhere, so there is no size threshold for it here.

// chx_coltile.hip: passes 1..E-1 of chx_track_elementwise through the column layout (needs chx_coltile_ok). flags: NULL, or
// chx_coltile_scratch_bytes() bytes, one word per tile (column 6 of the tile is all 1: the column passes do not read it).
bool chx_coltile_ok(const void* x, int64_t E, int64_t B, int64_t N, int dtype);
size_t chx_coltile_scratch_bytes(int64_t B, int64_t N, int dtype);
int chx_coltile_passes(void* x, const void* R, void* flags, int64_t E, int64_t B, int64_t BR, int64_t N, int dtype, hipStream_t s);
