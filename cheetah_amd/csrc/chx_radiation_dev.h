// chx_radiation_dev.h — the host-callable parts of chx_dkd_ring_radiation (Segment.radiation_integrals; the kernel stands in
// chx_nonlinear.hip next to dkd_ring_jacobian_kernel, whose layout it has): the 8-point Gauss-Legendre rule on (0, 1), what a
// lane adds to the sums a point inside a bend needs, dispersion, beta, alpha and curly H from those sums, and a Dipole's
// contribution to the seven integrals with its edge terms. tests/host/radiation_check.hip runs all of it against closed-form
// sector-bend values without a GPU, built with the address and undefined-behaviour sanitizers; the kernel runs the same functions.
//
// The definitions (include/chx.h): for a point s inside a Dipole, A(s) is the 6 x 6 Jacobian from the ring's start to s,
//   eta(s)  = rel_beta (A[:4, :4] eta0 + A[:4, 5])        rel_beta = p0c / E0: the library's delta is dE / p0c, the integrals are
//                                                         defined on d x / d (dp / p); eta' is d px / d delta (canonical)
//   beta_u, alpha_u = propagate_twiss of the diagonal 2 x 2 block of A(s) with beta0_u, alpha0_u (the projected functions)
//   H_u     = (eta_u^2 + (beta_u eta_u' + alpha_u eta_u)^2) / beta_u
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "chx_optics_dev.h"

namespace chx_radiation {

constexpr int kNodes = 8;        // Gauss-Legendre points per Dipole: exact to degree 15, error of order theta^16 / 16! for a bend angle theta
constexpr int kTerms = 12;       // sums over the group's lanes per point: eta (4), and per plane A11 beta0 - A12 alpha0, A21 beta0 - A22 alpha0, A12, A22
constexpr int kIntegrals = 7;    // I1, I2, I3, I4x, I4y, I5x, I5y

// node j of the 8-point rule on (0, 1), ascending, and its weight (the weights sum to 1)
__host__ __device__ inline double gl8_node(int j) {
    switch (j) {
        case 0: return 0.01985507175123188415821957;
        case 1: return 0.10166676129318663020422303;
        case 2: return 0.23723379504183550709113047;
        case 3: return 0.40828267875217509753026193;
        case 4: return 0.59171732124782490246973807;
        case 5: return 0.76276620495816449290886953;
        case 6: return 0.89833323870681336979577697;
        default: return 0.98014492824876811584178043;
    }
}
__host__ __device__ inline double gl8_weight(int j) {
    switch (j) {
        case 0: case 7: return 0.05061426814518812957626567;
        case 1: case 6: return 0.11119051722668723527217800;
        case 2: case 5: return 0.15685332293894364366898110;
        default: return 0.18134189168918099148257522;
    }
}

// What lane m of a group (column m of A: col[i] = A[i][m], i < 4; lanes 6 and 7 hold no column) adds to the kTerms sums. Terms a
// lane has no part in are exact zeros, so a plane without a periodic solution (beta0_u NaN) is NaN in its own four sums only.
__host__ __device__ inline void lane_terms(int m, const double* col, const double* eta0, const double* beta0, const double* alpha0, double* t) {
    _Pragma("unroll") for (int i = 0; i < 4; ++i) t[i] = m < 4 ? eta0[m] * col[i] : (m == 5 ? col[i] : 0.0);
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {
        const double a = col[2 * u], b = col[2 * u + 1];           // rows 2u and 2u + 1 of the column
        const bool first = m == 2 * u, second = m == 2 * u + 1;
        t[4 + 4 * u] = first ? beta0[u] * a : (second ? -(alpha0[u] * a) : 0.0);
        t[5 + 4 * u] = first ? beta0[u] * b : (second ? -(alpha0[u] * b) : 0.0);
        t[6 + 4 * u] = second ? a : 0.0;
        t[7 + 4 * u] = second ? b : 0.0;
    }
}

// the sum over a group's kGroup lanes in the order of the kernel's butterfly (lane ^ 1, ^ 2, ^ 4): every lane ends with these bits
__host__ __device__ inline double group_sum(const double* v) {
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

struct Node {
    double eta[4];               // (eta_x, eta_x', eta_y, eta_y') with the factor rel_beta
    double beta[2], alpha[2], H[2];
};

// eta alone (the faces of a bend: the edge terms need nothing else)
__host__ __device__ inline void eta_from_sums(const double* s, double rel_beta, double* eta) {
    _Pragma("unroll") for (int i = 0; i < 4; ++i) eta[i] = rel_beta * s[i];
}

__host__ __device__ inline void node_from_sums(const double* s, const double* beta0, double rel_beta, Node& n) {
    eta_from_sums(s, rel_beta, n.eta);
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {
        const double U = s[4 + 4 * u], W = s[5 + 4 * u], a12 = s[6 + 4 * u], a22 = s[7 + 4 * u];
        n.beta[u] = (U * U + a12 * a12) / beta0[u];
        n.alpha[u] = -(U * W + a12 * a22) / beta0[u];
        const double e = n.eta[2 * u], g = n.beta[u] * n.eta[2 * u + 1] + n.alpha[u] * e;
        n.H[u] = (e * e + g * g) / n.beta[u];
    }
}

// all of a point from the 4 x 6 block A[i * 6 + m] at once (the host's way to the numbers the lanes of a group reach together)
__host__ __device__ inline void node_from_block(const double* A, const double* eta0, const double* beta0, const double* alpha0, double rel_beta,
                                                Node& n) {
    double t[chx_optics::kGroup][kTerms], s[kTerms];
    _Pragma("unroll") for (int m = 0; m < chx_optics::kGroup; ++m) {
        double col[4];
        _Pragma("unroll") for (int i = 0; i < 4; ++i) col[i] = m < 6 ? A[i * 6 + m] : 0.0;
        lane_terms(m, col, eta0, beta0, alpha0, t[m]);
    }
    _Pragma("unroll") for (int k = 0; k < kTerms; ++k) {
        double v[chx_optics::kGroup];
        _Pragma("unroll") for (int m = 0; m < chx_optics::kGroup; ++m) v[m] = t[m][k];
        s[k] = group_sum(v);
    }
    node_from_sums(s, beta0, rel_beta, n);
}

// the dispersion in the bending plane of a magnet tilted by t
__host__ __device__ inline double eta_bend(const double* eta, double cos_t, double sin_t) { return eta[0] * cos_t + eta[2] * sin_t; }

// the quadrature sums of one Dipole, a node after the other in ascending order
struct BendSums {
    double s1, s4x, s4y, s5x, s5y;
};
__host__ __device__ inline BendSums bend_sums_zero() { return BendSums{0.0, 0.0, 0.0, 0.0, 0.0}; }
__host__ __device__ inline void bend_sums_add(BendSums& b, double w, double cos_t, double sin_t, const Node& n) {
    b.s1 = b.s1 + w * eta_bend(n.eta, cos_t, sin_t);
    b.s4x = b.s4x + w * n.eta[0];
    b.s4y = b.s4y + w * n.eta[2];
    b.s5x = b.s5x + w * n.H[0];
    b.s5y = b.s5y + w * n.H[1];
}

// The contribution of a Dipole of length L and curvature h = angle / L, tilted by t, to (I1, I2, I3, I4x, I4y, I5x, I5y). ch = h tan e1
// and cj = h tan e2 are the tracking's edge constants (zero where the face's fringe is off): a rectangular magnet's path length does
// not grow with x, which takes h^2 eta tan e off I4 at each face (eta_in, eta_out: the bending-plane dispersion at the faces).
// L == 0 or h == 0 (no angle): zeros.
__host__ __device__ inline void bend_contribution(double L, double h, double cos_t, double sin_t, double ch, double cj, double eta_in, double eta_out,
                                                  const BendSums& b, double* out) {
    if (L == 0.0 || h == 0.0) {
        _Pragma("unroll") for (int k = 0; k < kIntegrals; ++k) out[k] = 0.0;
        return;
    }
    const double h2 = h * h, h3a = fabs(h) * h2, edge = ch * eta_in + cj * eta_out;
    out[0] = L * h * b.s1;
    out[1] = L * h2;
    out[2] = L * h3a;
    out[3] = L * (h2 * h) * cos_t * b.s4x - h * cos_t * edge;
    out[4] = L * (h2 * h) * sin_t * b.s4y - h * sin_t * edge;
    out[5] = L * h3a * b.s5x;
    out[6] = L * h3a * b.s5y;
}

}  // namespace chx_radiation
