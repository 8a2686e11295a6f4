// chx_optics_dev.h — the host-callable parts of chx_dkd_ring_jacobian and chx_dkd_ring_sensitivity (Segment.ring_optics,
// ring_sensitivity; the kernels stand in chx_nonlinear.hip next to the templates they evaluate): which lane carries which seed,
// knob and tangent, the linear systems of the closed-orbit Newton step, of the orbit's derivative and of the dispersion, and the
// small dense solver they go through. tests/host/optics_check.hip runs all of it against
// long-double eliminations without a GPU, built with the address and undefined-behaviour sanitizers; the kernel runs the same
// functions, one seed per group of lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace chx_optics {

// A seed is a group of kGroup consecutive lanes: lane m of the group carries the tangent e_m for m < 6, lanes 6 and 7 carry none
// (they walk the same orbit and store nothing). kSeeds groups make the one wave of a workgroup.
constexpr int kGroup = 8;
constexpr int kSeeds = 8;
constexpr int kLanes = kGroup * kSeeds;

__host__ __device__ inline int group_of_lane(int lane) { return lane / kGroup; }
__host__ __device__ inline int tangent_of_lane(int lane) { return lane % kGroup; }
// workgroups for B seeds (B >= 1)
__host__ __device__ inline int64_t workgroups(int64_t B) { return (B + kSeeds - 1) / kSeeds; }
// the seed a group works on: the last seed again for the groups past the end of the last workgroup (they store nothing)
__host__ __device__ inline int64_t seed_of_group(int64_t workgroup, int group, int64_t B, bool& live) {
    const int64_t seed = workgroup * kSeeds + group;
    live = seed < B;
    return live ? seed : B - 1;
}

// a x = b for the n x n matrix a (row-major, rows `lda` apart), n <= 6, by Gaussian elimination with partial pivoting; a is
// destroyed, b becomes x. false — and b all NaN — when a pivot is zero or not finite or the solution is not finite: a singular
// system and a system with a NaN or an infinity in it end the same way. The work does not depend on the values beyond the
// choice of the pivot rows.
__host__ __device__ inline bool solve(int n, double* a, int lda, double* b) {
    bool ok = true;
    for (int k = 0; k < n; ++k) {
        int p = k;
        double big = fabs(a[k * lda + k]);
        for (int r = k + 1; r < n; ++r) {
            const double v = fabs(a[r * lda + k]);
            if (v > big) {
                big = v;
                p = r;
            }
        }
        if (!(big > 0.0) || !(big <= 1.79769313486231570815e308)) {          // zero, NaN or infinite
            ok = false;
            break;
        }
        if (p != k) {
            for (int c = 0; c < n; ++c) {
                const double t = a[k * lda + c];
                a[k * lda + c] = a[p * lda + c];
                a[p * lda + c] = t;
            }
            const double t = b[k];
            b[k] = b[p];
            b[p] = t;
        }
        const double piv = a[k * lda + k];
        for (int r = k + 1; r < n; ++r) {
            const double f = a[r * lda + k] / piv;
            for (int c = k + 1; c < n; ++c) a[r * lda + c] = a[r * lda + c] - f * a[k * lda + c];
            b[r] = b[r] - f * b[k];
        }
    }
    if (ok) {
        for (int k = n - 1; k >= 0; --k) {
            double s = b[k];
            for (int c = k + 1; c < n; ++c) s = s - a[k * lda + c] * b[c];
            b[k] = s / a[k * lda + k];
        }
        for (int k = 0; k < n; ++k) ok = ok && fabs(b[k]) <= 1.79769313486231570815e308;
    }
    if (!ok) {
        for (int k = 0; k < n; ++k) b[k] = NAN;
    }
    return ok;
}

// the closed coordinates of a search: the first four (mode 1: delta and tau are held) or all six (mode 2)
__host__ __device__ inline int closed_count(int mode) { return mode == 2 ? 6 : 4; }

// The Newton step of the closed orbit on the first n coordinates: (M_c - I) step = -(f - x)_c from the 6 x 6 matrix M[i * 6 + m] =
// d f_i / d x_m, the image f and the point x. The step is left in `step` (NaN when there is none); a[36] is scratch.
__host__ __device__ inline bool newton_step(int n, const double* M, const double* f, const double* x, double* a, double* step) {
    for (int i = 0; i < n; ++i) {
        for (int m = 0; m < n; ++m) a[i * 6 + m] = M[i * 6 + m] - (i == m ? 1.0 : 0.0);
        step[i] = -(f[i] - x[i]);
    }
    return solve(n, a, 6, step);
}

// the dispersion of the 4-D motion, (I - M_4) eta = M[:4, 5], from the same solver
__host__ __device__ inline bool dispersion(const double* M, double* a, double* eta) {
    for (int i = 0; i < 4; ++i) {
        for (int m = 0; m < 4; ++m) a[i * 6 + m] = (i == m ? 1.0 : 0.0) - M[i * 6 + m];
        eta[i] = M[i * 6 + 5];
    }
    return solve(4, a, 6, eta);
}

// |f - x| over the first n coordinates, NaN when one of them is
__host__ __device__ inline double closing_error(int n, const double* f, const double* x) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) {
        const double d = fabs(f[i] - x[i]);
        if (d > r || d != d) r = d;                // (a NaN takes over and stays: no later d is > NaN)
    }
    return r;
}

// ---- chx_dkd_ring_sensitivity: a group of kGroup lanes works on a (seed, knob) PAIR, pair = seed * K + knob, as a group of
// chx_dkd_ring_jacobian works on a seed. Lane m < 6 of the group carries e1 = e_m in phase space, every lane e2 = the knob.
// workgroups for B seeds and K knobs (B >= 1, K >= 1)
__host__ __device__ inline int64_t pair_workgroups(int64_t B, int64_t K) { return (B * K + kSeeds - 1) / kSeeds; }
// the (seed, knob) a group works on: the last pair again for the groups past the end of the last workgroup (they store nothing)
__host__ __device__ inline void pair_of_group(int64_t workgroup, int group, int64_t B, int64_t K, bool& live, int64_t& seed, int64_t& knob) {
    int64_t pair = workgroup * kSeeds + group;
    live = pair < B * K;
    if (!live) pair = B * K - 1;
    seed = pair / K;
    knob = pair % K;
}

// How the closed orbit moves with a knob: x = f(x, theta) on the first n coordinates gives (I - M_n) w = (d f / d theta)_n — the
// matrix of the Newton step with the other sign — from M[i * 6 + m] = d f_i / d x_m and dfdt[6]. w[6] is left 0 on the held
// coordinates and NaN on the closed ones when there is no solution; a[36] is scratch.
__host__ __device__ inline bool orbit_sensitivity(int n, const double* M, const double* dfdt, double* a, double* w) {
    for (int i = 0; i < 6; ++i) w[i] = 0.0;
    for (int i = 0; i < n; ++i) {
        for (int m = 0; m < n; ++m) a[i * 6 + m] = (i == m ? 1.0 : 0.0) - M[i * 6 + m];
        w[i] = dfdt[i];
    }
    return solve(n, a, 6, w);
}

}  // namespace chx_optics
