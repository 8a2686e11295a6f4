// chx_quiet.hip — quiet-start deviates: the Halton sequence in up to eight prime bases, as uniforms in (0, 1) or as standard-normal
// deviates, for beams whose sampling noise lies far below 1 / sqrt(N) (ParticleBeam.from_distribution(quiet_start=True)).
// Row n of out[N][D] has the index i = offset + 1 + n (index 0 is never used, so 0 < u < 1); column d is the radical inverse of i in
// the base bases[d]. Bit-defined: in unsigned 64-bit integers the digits of i are peeled off in base b, r = r b + digit and p = p b per
// digit, and u = (double)r / (double)p is ONE IEEE division. For i < 2^40 and b <= 19 both r and p stay below 2^53, so both
// conversions are exact and u has the same bits on any machine. The bases are compile-time constants of the digit loop (one
// instantiation per prime up to 19), so its divisions are multiply-shifts: 64-bit division by a run-time value is emulated.
// Normal deviates, in fp64: s = min(u, 1 - u) (1 - u is exact for u >= 1/2), z = -+ sqrt(2) erfcinv(2 s), negative for u < 1/2 and
// exactly 0 at u = 1/2. A float32 output is the fp64 value rounded once on the store.
// One launch, one row per lane and step of a grid-stride loop, a lane stores its whole row contiguously. Nothing depends on the
// launch geometry: rows [a, b) of one call equal a call with offset + a.
#include "chx_common.h"

namespace {

constexpr int kMaxDims = CHX_QUIET_MAX_DIMS;
constexpr int64_t kIndexEnd = (int64_t)1 << 40;           // indices stay below 2^40
constexpr double kSqrt2 = 1.4142135623730951;             // fl(sqrt 2)

struct QuietBases { int b[kMaxDims]; };

// r and p are carried as doubles: integers below 2^53, so every r B + digit and p B is exact and they are the integers of the
// definition, converted. Digits above 2^32 are peeled off in 64 bits, the rest in 32 (B is a constant: multiply and shift).
template <unsigned B>
__device__ __forceinline__ double radical_inverse(uint64_t i) {
    double r = 0.0, p = 1.0;
    while (i >> 32) {
        const uint64_t q = i / B;
        r = r * (double)B + (double)(unsigned)(i - q * B);
        p *= (double)B;
        i = q;
    }
    unsigned j = (unsigned)i;
    while (j) {
        const unsigned q = j / B;
        r = r * (double)B + (double)(j - q * B);
        p *= (double)B;
        j = q;
    }
    return r / p;
}

__device__ __forceinline__ double radical_inverse_in(int base, uint64_t i) {
    switch (base) {                                           // uniform over the launch
        case 2: return radical_inverse<2>(i);
        case 3: return radical_inverse<3>(i);
        case 5: return radical_inverse<5>(i);
        case 7: return radical_inverse<7>(i);
        case 11: return radical_inverse<11>(i);
        case 13: return radical_inverse<13>(i);
        case 17: return radical_inverse<17>(i);
        default: return radical_inverse<19>(i);
    }
}

__device__ __forceinline__ double normal_of(double u) {
    if (u == 0.5) return 0.0;
    const bool low = u < 0.5;
    const double s = low ? u : 1.0 - u;
    const double z = kSqrt2 * erfcinv(2.0 * s);
    return low ? -z : z;
}

template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void quiet_sequence_kernel(QuietBases bases, int D, int64_t N, int64_t offset, int normal,
                                                                   T* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * CHX_BLOCK;
    for (int64_t n = (int64_t)blockIdx.x * CHX_BLOCK + threadIdx.x; n < N; n += stride) {
        const uint64_t i = (uint64_t)(offset + 1 + n);
        T* row = out + n * D;
#pragma unroll
        for (int d = 0; d < kMaxDims; ++d) {
            if (d < D) {
                const double u = radical_inverse_in(bases.b[d], i);
                row[d] = (T)(normal ? normal_of(u) : u);
            }
        }
    }
}

bool quiet_base_ok(int b) { return b == 2 || b == 3 || b == 5 || b == 7 || b == 11 || b == 13 || b == 17 || b == 19; }

}  // namespace

extern "C" int chx_quiet_sequence(const int* bases, int64_t D, int64_t N, int64_t offset, int normal, int dtype, void* out,
                                  void* stream) {
    if (!bases || !out || D < 1 || D > kMaxDims || N < 1 || offset < 0 || offset >= kIndexEnd || N >= kIndexEnd - offset)
        return CHX_ERR_INVALID_ARG;
    QuietBases qb;
    for (int d = 0; d < kMaxDims; ++d) qb.b[d] = 2;
    for (int d = 0; d < (int)D; ++d) {
        if (!quiet_base_ok(bases[d])) return CHX_ERR_INVALID_ARG;
        for (int e = 0; e < d; ++e)
            if (bases[e] == bases[d]) return CHX_ERR_INVALID_ARG;       // two columns in one base would be equal
        qb.b[d] = bases[d];
    }
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    const int grid = chx_grid_for(N, CHX_BLOCK, 1 << 16);
    return dispatch_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL(quiet_sequence_kernel<T>, dim3((unsigned)grid), dim3(CHX_BLOCK), 0, (hipStream_t)stream, qb, (int)D, N,
                           offset, normal, (T*)out);
        CHX_CHECK_LAUNCH();
        return CHX_OK;
    });
}
