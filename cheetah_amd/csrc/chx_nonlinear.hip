// chx_nonlinear.hip — per-particle non-linear tracking for gfx950.
//
//  * drift-kick-drift (Bmad-X) tracking of Drift, Quadrupole, Dipole, TransverseDeflectingCavity, Sextupole, RFCavity and Multipole:
//    cheetah/accelerator/drift.py:106-154, quadrupole.py:168-251, dipole.py:183-370,
//    transverse_deflecting_cavity.py:122-209 on top of cheetah/utils/bmadx.py;
//  * second-order (MAD-convention T tensor) tracking: element.py:195-228 with the tensors of
//    track_methods.py:80-296 (base_ttensor) dressed per element in drift.py:68-84,
//    quadrupole.py:113-146, dipole.py:397-428 and sextupole.py:91-116.
//
// Both are one streaming pass over particles[B][N][7] (56 B/particle fp32, 112 B fp64) through the same
// LDS tile staging as chx_apply.hip; the per-particle arithmetic runs in fp64 whatever the storage
// dtype is (transcendental-heavy but far below the HBM time of the pass on 256 CUs).
#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <type_traits>
#include <utility>
#include <vector>

#include "chx_common.h"
#include "chx_dual.h"
#include "chx_dual2.h"
#include "chx_optics_dev.h"
#include "chx_radiation_dev.h"

// parameters per drift-kick-drift kind (include/chx.h), -1 for anything else: what every entry point below counts with
static __host__ __device__ int dkd_num_params(int kind) {
    switch (kind) {
        case CHX_DKD_DRIFT: return 1;
        case CHX_DKD_QUADRUPOLE: return 5;
        case CHX_DKD_DIPOLE: return 9;
        case CHX_DKD_TDC: return 7;
        case CHX_DKD_SEXTUPOLE: return 5;
        case CHX_DKD_RFCAVITY: return 4;
        case CHX_DKD_MULTIPOLE: return 6;
    }
    return -1;
}

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kC = 299792458.0;  // scipy.constants.speed_of_light

// ---------------------------------------------------------------------------------------------
// Bmad-X helpers (utils/bmadx.py). Templates over S = double (tracking) or Dual (chx_dkd_track_bwd).
// ---------------------------------------------------------------------------------------------
template <typename S> __device__ __forceinline__ S sinc1(S x) { return val(x) == 0.0 ? cst<S>(1.0) : m_sin(x) / x; }  // bmadx.py:318
template <typename S> __device__ __forceinline__ S cosc1(S x) { const S s = sinc1<S>(0.5 * x); return -0.5 * s * s; }  // :323
template <typename S> __device__ __forceinline__ S sqrt_one(S x) { return x / (m_sqrt(1.0 + x) + 1.0); }              // :255

template <typename S>
struct Bmad {
    S x, px, y, py, z, pz;
};

// bmadx.py:7-31
template <typename S>
__device__ __forceinline__ void to_bmad(S tau, S delta, S E, double mc2, S p0c, S& z, S& pz) {
    const S en = E + delta * p0c;
    const S p = m_sqrt(en * en - mc2 * mc2);
    const S beta = p / en;
    z = -beta * tau;
    pz = (p - p0c) / p0c;
}
// bmadx.py:34-56
template <typename S>
__device__ __forceinline__ void from_bmad(S z, S pz, S p0c, double mc2, S& tau, S& delta) {
    const S ref = m_sqrt(p0c * p0c + mc2 * mc2);
    const S p = (1.0 + pz) * p0c;
    const S en = m_sqrt(p * p + mc2 * mc2);
    const S beta = p / en;
    tau = -z / beta;
    delta = (en - ref) / p0c;
}
// bmadx.py:117-147 / 150-181
template <typename S>
__device__ __forceinline__ void offset_set(S xo, S yo, S s, S c, Bmad<S>& q) {
    const S xi = q.x - xo, yi = q.y - yo;
    const S x = xi * c + yi * s, y = -xi * s + yi * c;
    const S px = q.px * c + q.py * s, py = -q.px * s + q.py * c;
    q.x = x; q.y = y; q.px = px; q.py = py;
}
template <typename S>
__device__ __forceinline__ void offset_unset(S xo, S yo, S s, S c, Bmad<S>& q) {
    const S xi = q.x * c - q.y * s, yi = q.x * s + q.y * c;
    const S px = q.px * c - q.py * s, py = q.px * s + q.py * c;
    q.x = xi + xo; q.y = yi + yo; q.px = px; q.py = py;
}
// bmadx.py:263-298
template <typename S>
__device__ __forceinline__ void track_a_drift(S L, Bmad<S>& q, S p0c, double mc2) {
    const S P = 1.0 + q.pz;
    const S Px = q.px / P, Py = q.py / P;
    const S Pxy2 = Px * Px + Py * Py;
    const S Pl = m_sqrt(1.0 - Pxy2);
    const S pc = p0c * P;
    const S dz =
        L * (sqrt_one<S>((mc2 * mc2 * (2.0 * q.pz + q.pz * q.pz)) / (pc * pc + mc2 * mc2)) + sqrt_one<S>(-Pxy2) / Pl);
    q.x = q.x + L * Px / Pl;
    q.y = q.y + L * Py / Pl;
    q.z = q.z + dz;
}
// bmadx.py:184-216
template <typename S>
__device__ __forceinline__ S low_energy_z_correction(S pz, S p0c, double mc2, S ds) {
    const S pc = (1.0 + pz) * p0c;
    const S beta = pc / m_sqrt(pc * pc + mc2 * mc2);
    const S e_tot = m_sqrt(p0c * p0c + mc2 * mc2);
    const S beta0 = p0c / e_tot;
    const S b0pz = beta0 * pz;
    const S evaluation = mc2 * (b0pz * b0pz);
    const S me = mc2 / e_tot, me2 = me * me, b02 = beta0 * beta0;
    if (val(evaluation) < 3e-7 * val(e_tot))
        return ds * pz * (1.0 - 3.0 * (pz * b02) / 2.0 + pz * pz * b02 * (2.0 * b02 - me2 / 2.0)) * me2;
    return ds * (beta - beta0) / beta0;
}
// bmadx.py:219-252 with k1 real: kx = sqrt(-k1) is real (k1 < 0), imaginary (k1 > 0) or zero
template <typename S>
struct QuadCoef {
    S a11, a12, a21, a22, c1, c2, c3;
};
// cx = cos(sqrt(w) len) and sx = sin(sqrt(w) len) / sqrt(w) are entire functions of u = w len^2: cx = sum (-u)^n / (2n)!,
// sx = len sum (-u)^n / (2n + 1)!. The closed forms below keep the VALUES to the last digit down to w == 0, which they treat as
// a constant — but a tangent through them loses its digits near 0 (d sx / d w = (len cos - sx) / (2 w): a difference of order
// u over u, 3e-5 off at k1 = 1e-12) and all of itself at 0, where d cx / d w = -len^2 / 2 and d sx / d w = -len^3 / 6. So the
// dual-number evaluation, and it alone, takes the series inside |u| < 1e-4 (first term left out: u^5 / 10!, below 1e-26; the
// closed forms' tangents are good to 2^-52 / |u| <= 3e-12 outside). The reference's autograd returns NaN at k1 == 0 (a complex
// square root at 0); the limit is the definition.
__device__ __forceinline__ bool quad_cs_series(Dual w, Dual len, Dual& cx, Dual& sx) {
    const Dual u = w * len * len;
    if (!(fabs(u.v) < 1e-4)) return false;
    cx = 1.0 - u * (1.0 / 2.0 - u * (1.0 / 24.0 - u * (1.0 / 720.0 - u * (1.0 / 40320.0))));
    sx = len * (1.0 - u * (1.0 / 6.0 - u * (1.0 / 120.0 - u * (1.0 / 5040.0 - u * (1.0 / 362880.0)))));
    return true;
}
template <typename S>
__device__ __forceinline__ QuadCoef<S> quad_from_cs(S k1, S len, S rel_p, S cx, S sx) {
    QuadCoef<S> q;
    q.a11 = cx;
    q.a12 = sx / rel_p;
    q.a21 = k1 * sx * rel_p;
    q.a22 = cx;
    q.c1 = k1 * (-cx * sx + len) / 4.0;
    q.c2 = -k1 * (sx * sx) / (2.0 * rel_p);
    q.c3 = -(cx * sx + len) / (4.0 * (rel_p * rel_p));
    return q;
}
template <typename S>
__device__ __forceinline__ QuadCoef<S> quad_coefficients(S k1, S len, S rel_p) {
    S cx, sx;
    const S w = -k1;
    if constexpr (std::is_same<S, Dual>::value || std::is_same<S, Dual2>::value) {
        if (quad_cs_series(w, len, cx, sx)) return quad_from_cs<S>(k1, len, rel_p, cx, sx);
    }
    if (val(w) > 0.0) {
        const S k = m_sqrt(w);
        cx = m_cos(k * len);
        sx = m_sin(k * len) / k;
    } else if (val(w) < 0.0) {
        const S k = m_sqrt(-w);
        cx = m_cosh(k * len);
        sx = m_sinh(k * len) / k;
    } else {
        cx = cst<S>(1.0);
        sx = len;
    }
    return quad_from_cs<S>(k1, len, rel_p, cx, sx);
}
// utils/autograd.py:669-670 (value) and :672-700 (derivatives, with the b == 0 limits -1/(2a^2), -1/(8a^3))
__device__ __forceinline__ double sqrta2minusbdiva(double a, double b) {
    return b != 0.0 ? (sqrt(a * a + b) - a) / b : 1.0 / (2.0 * a);
}
__device__ __forceinline__ F32 sqrta2minusbdiva(F32 a, F32 b) {
    return b.v != 0.0f ? mkf((sqrtf(a.v * a.v + b.v) - a.v) / b.v) : mkf(1.0f / (2.0f * a.v));
}
__device__ __forceinline__ Dual sqrta2minusbdiva(Dual a, Dual b) {
    if (b.v != 0.0) return (m_sqrt(a * a + b) - a) / b;
    return mk(1.0 / (2.0 * a.v), -a.d / (2.0 * a.v * a.v) - b.d / (8.0 * a.v * a.v * a.v));
}

// sin and cos of 2 pi u for a phase u in TURNS: r = u - rint(u) is exact and |r| <= 1/2, sincospi(2 r) has no reduction of its own
// left to do (as in chx_laser.hip, chx_bunching.hip, chx_density.hip) — and u = 0, 1/4, 1/2 ... give exact zeros and ones.
__device__ __forceinline__ void turn_sincos(double u, double& s, double& c) {
    const double r = u - __builtin_rint(u);
    sincospi(2.0 * r, &s, &c);
}
__device__ __forceinline__ void turn_sincos(F32 u, F32& s, F32& c) {
    const float r = u.v - __builtin_rintf(u.v);
    sincospif(2.0f * r, &s.v, &c.v);
}
__device__ __forceinline__ void turn_sincos(Dual u, Dual& s, Dual& c) {
    double sv, cv;
    turn_sincos(u.v, sv, cv);
    s = mk(sv, 2.0 * kPi * cv * u.d);
    c = mk(cv, -2.0 * kPi * sv * u.d);
}
__device__ __forceinline__ void turn_sincos(Dual2 u, Dual2& s, Dual2& c) {
    double sv, cv;
    turn_sincos(u.v, sv, cv);
    s = chain2(u, sv, 2.0 * kPi * cv, -(2.0 * kPi) * (2.0 * kPi) * sv);
    c = chain2(u, cv, -2.0 * kPi * sv, -(2.0 * kPi) * (2.0 * kPi) * cv);
}

// ---------------------------------------------------------------------------------------------
// per-batch-row constants (computed once per workgroup by lane 0, shared through LDS)
// ---------------------------------------------------------------------------------------------
enum { C_E = 0, C_P0C, C_SIN, C_COS, C_XO, C_YO, C_A, C_B, C_C, C_D, C_E2, C_F, C_G, C_H, C_I, C_J, C_N };

template <typename S>
__device__ void dkd_constants(int kind, const S* par, S E, double mc2, double nq, int fringe, S* c) {
    const S zero = cst<S>(0.0), one = cst<S>(1.0);
    c[C_E] = E;
    const S p0c = m_sqrt(E * E - mc2 * mc2);
    c[C_P0C] = p0c;
    c[C_SIN] = zero; c[C_COS] = one; c[C_XO] = zero; c[C_YO] = zero;
    if (kind == CHX_DKD_DRIFT) {
        c[C_A] = par[0];
    } else if (kind == CHX_DKD_QUADRUPOLE) {
        const S L = par[0], k1 = par[1], tilt = par[2];
        c[C_SIN] = m_sin(tilt); c[C_COS] = m_cos(tilt);
        c[C_XO] = par[3]; c[C_YO] = par[4];
        c[C_A] = L;
        c[C_B] = k1 * L;  // b1 (quadrupole.py:199)
    } else if (kind == CHX_DKD_DIPOLE) {
        const S L = par[0], angle = par[1], e1 = par[2], e2 = par[3];
        const S tilt = par[4], fint = par[5], fintx = par[6];
        const S gap = par[7], gapx = par[8];
        c[C_SIN] = m_sin(tilt); c[C_COS] = m_cos(tilt);
        const S g = angle / L;
        c[C_A] = L; c[C_B] = angle; c[C_C] = g;
        c[C_D] = sinc1<S>(angle); c[C_E2] = cosc1<S>(angle); c[C_F] = m_cos(angle); c[C_G] = m_sin(angle);
        // linear fringe kicks (dipole.py:355-366): hx, hy at entrance and exit
        const S hg1 = 0.5 * gap, hg2 = 0.5 * gapx;
        const S s1 = m_sin(e1), s2 = m_sin(e2);
        c[C_H] = (fringe & 1) ? g * m_tan(e1) : zero;
        c[C_I] = (fringe & 1) ? -g * m_tan(e1 - 2.0 * fint * hg1 * g * (1.0 + s1 * s1) / m_cos(e1)) : zero;
        c[C_J] = (fringe & 2) ? g * m_tan(e2) : zero;
        c[C_N] = (fringe & 2) ? -g * m_tan(e2 - 2.0 * fintx * hg2 * g * (1.0 + s2 * s2) / m_cos(e2)) : zero;
    } else if (kind == CHX_DKD_SEXTUPOLE) {
        const S L = par[0], k2 = par[1], tilt = par[2];
        c[C_SIN] = m_sin(tilt); c[C_COS] = m_cos(tilt);
        c[C_XO] = par[3]; c[C_YO] = par[4];
        c[C_A] = L;
        c[C_B] = k2 * L;  // the integrated strength: every one of the n kicks applies 1 / n of it
    } else if (kind == CHX_DKD_RFCAVITY) {
        const S L = par[0], V = par[1], phase = par[2], freq = par[3];
        c[C_A] = L;
        c[C_B] = V * fabs(nq);               // the energy a particle gains on the crest, in eV
        turn_sincos(phase, c[C_C], c[C_D]);  // S0 = sin(2 pi phase), C0 = cos(2 pi phase): phase = 0 and 0.5 are exact zero crossings
        c[C_E2] = freq;
    } else if (kind == CHX_DKD_MULTIPOLE) {
        // `fringe` carries the order m = 0 .. 3 of the kick (include/chx.h). 1 / m! goes into the strengths here, so the kick is
        // C_B Re (x + i y)^m - C_C Im (x + i y)^m with no factorial left in it; m itself in a slot of its own (wave-uniform)
        const S L = par[0], knl = par[1], ksl = par[2], tilt = par[3];
        c[C_SIN] = m_sin(tilt); c[C_COS] = m_cos(tilt);
        c[C_XO] = par[4]; c[C_YO] = par[5];
        c[C_A] = L;
        const int m = fringe & 3;
        const double inv_fact = m < 2 ? 1.0 : (m == 2 ? 0.5 : 1.0 / 6.0);
        c[C_B] = knl * inv_fact;  // the integrated strengths: every one of the n kicks applies 1 / n of them
        c[C_C] = ksl * inv_fact;
        c[C_D] = cst<S>((double)m);
    } else {  // CHX_DKD_TDC
        const S L = par[0], V = par[1], phase = par[2], freq = par[3];
        const S tilt = par[4];
        c[C_SIN] = m_sin(tilt); c[C_COS] = m_cos(tilt);
        c[C_XO] = par[5]; c[C_YO] = par[6];
        c[C_A] = L;
        c[C_B] = V * -1.0 * nq / p0c;        // transverse_deflecting_cavity.py:156
        c[C_C] = 2.0 * kPi * freq / kC;      // k_rf
        c[C_D] = phase; c[C_E2] = freq;
    }
}

// dipole.py:246-336
template <typename S>
__device__ __forceinline__ void dipole_body(const S* c, Bmad<S>& q, S p0c, double mc2) {
    const S L = c[C_A], angle = c[C_B], g = c[C_C], sinc_a = c[C_D], cosc_a = c[C_E2];
    const S cos_a = c[C_F], sin_a = c[C_G];
    const S px_norm = m_sqrt((1.0 + q.pz) * (1.0 + q.pz) - q.py * q.py);
    const S phi1 = m_asin(q.px / px_norm);
    const S gp = g / px_norm;
    const S gx1 = 1.0 + g * q.x;
    const S sap = m_sin(angle + phi1), cap = m_cos(angle + phi1);
    const S t = gx1 * L * sinc_a;
    const S alpha = 2.0 * gx1 * sap * L * sinc_a - gp * (t * t);
    const S x2_t1 = q.x * cos_a + L * L * g * cosc_a;
    const S x2_t2 = m_sqrt(cap * cap + gp * alpha);
    const S x2_t3 = cap;
    const S x2 = (fabs(val(angle) + val(phi1)) < kPi / 2.0) ? x2_t1 + alpha / (x2_t2 + x2_t3)
                                                            : x2_t1 + alpha * sqrta2minusbdiva(x2_t3, gp * alpha);
    const S Lcu = x2 - L * L * g * cosc_a - q.x * cos_a;
    const S Lcv = -L * sinc_a - q.x * sin_a;
    const S theta_p = 2.0 * (angle + phi1 - kPi / 2.0 - m_atan2(Lcv, Lcu));
    const S Lc = m_sqrt(Lcu * Lcu + Lcv * Lcv);
    const S Lp = Lc / sinc1<S>(theta_p / 2.0);
    const S P = p0c * (1.0 + q.pz);
    const S E = m_sqrt(P * P + mc2 * mc2);
    const S E0 = m_sqrt(p0c * p0c + mc2 * mc2);
    const S beta = P / E, beta0 = p0c / E0;
    q.x = x2;
    q.px = px_norm * m_sin(angle + phi1 - theta_p);
    q.y = q.y + q.py * Lp / px_norm;
    q.z = q.z + (beta * L / beta0) - ((1.0 + q.pz) * Lp / px_norm);
}

template <int KIND, typename S>
__device__ __forceinline__ void dkd_particle(const S* c, Bmad<S>& q, double mc2, int num_steps) {
    const S p0c = c[C_P0C];
    if (KIND == CHX_DKD_DRIFT) {
        track_a_drift<S>(c[C_A], q, p0c, mc2);
    } else if (KIND == CHX_DKD_QUADRUPOLE) {
        const S L = c[C_A], b1 = c[C_B];
        const S step = L / (double)num_steps;
        offset_set<S>(c[C_XO], c[C_YO], c[C_SIN], c[C_COS], q);
        // pz does not change inside the magnet, so the per-step coefficients are the same for every step
        const S rel_p = 1.0 + q.pz;
        const S k1 = b1 / (L * rel_p);
        const QuadCoef<S> tx = quad_coefficients<S>(-k1, step, rel_p);
        const QuadCoef<S> ty = quad_coefficients<S>(k1, step, rel_p);
        const S dzc = low_energy_z_correction<S>(q.pz, p0c, mc2, step);
        for (int s = 0; s < num_steps; ++s) {
            q.z = q.z + tx.c1 * (q.x * q.x) + tx.c2 * q.x * q.px + tx.c3 * (q.px * q.px) + ty.c1 * (q.y * q.y) +
                  ty.c2 * q.y * q.py + ty.c3 * (q.py * q.py);
            const S xn = tx.a11 * q.x + tx.a12 * q.px, pxn = tx.a21 * q.x + tx.a22 * q.px;
            const S yn = ty.a11 * q.y + ty.a12 * q.py, pyn = ty.a21 * q.y + ty.a22 * q.py;
            q.x = xn; q.px = pxn; q.y = yn; q.py = pyn;
            q.z = q.z + dzc;
        }
        offset_unset<S>(c[C_XO], c[C_YO], c[C_SIN], c[C_COS], q);
    } else if (KIND == CHX_DKD_DIPOLE) {
        const S zero = cst<S>(0.0);
        offset_set<S>(zero, zero, c[C_SIN], c[C_COS], q);
        q.px = q.px + q.x * c[C_H];
        q.py = q.py + q.y * c[C_I];
        dipole_body<S>(c, q, p0c, mc2);
        q.px = q.px + q.x * c[C_J];
        q.py = q.py + q.y * c[C_N];
        offset_unset<S>(zero, zero, c[C_SIN], c[C_COS], q);
    } else if (KIND == CHX_DKD_SEXTUPOLE) {
        // Bmad's exact drifts around thin kicks (the reference has no drift-kick-drift Sextupole; track_a_drift and the offsets
        // are its building blocks): n kicks of k2 L / n between n + 1 drifts of L / 2n, L / n, ..., L / n, L / 2n. Every piece
        // is symplectic and leaves pz alone, so the element does.
        const S h = c[C_A] / (2.0 * (double)num_steps), kappa = c[C_B] / (double)num_steps;
        offset_set<S>(c[C_XO], c[C_YO], c[C_SIN], c[C_COS], q);
        track_a_drift<S>(h, q, p0c, mc2);
        for (int s = 0; s < num_steps; ++s) {
            q.px = q.px - 0.5 * kappa * (q.x * q.x - q.y * q.y);
            q.py = q.py + kappa * q.x * q.y;
            track_a_drift<S>(s + 1 < num_steps ? 2.0 * h : h, q, p0c, mc2);
        }
        offset_unset<S>(c[C_XO], c[C_YO], c[C_SIN], c[C_COS], q);
    } else if (KIND == CHX_DKD_MULTIPOLE) {
        // The Sextupole's frame with the kick of one order m: d px - i d py = -(knl + i ksl) / n (x + i y)^m / m!. The power by m
        // complex multiplications from 1, no pow and no branch on a value: the dual-number evaluation has the right tangent at
        // x = y = 0 and at knl = ksl = 0 (m is wave-uniform). length = 0: the drifts add 0 to x, y and z.
        const S h = c[C_A] / (2.0 * (double)num_steps), bn = c[C_B] / (double)num_steps, an = c[C_C] / (double)num_steps;
        const int m = (int)val(c[C_D]);
        offset_set<S>(c[C_XO], c[C_YO], c[C_SIN], c[C_COS], q);
        track_a_drift<S>(h, q, p0c, mc2);
        for (int s = 0; s < num_steps; ++s) {
            S re = cst<S>(1.0), im = cst<S>(0.0);
            for (int k = 0; k < m; ++k) {
                const S r = re * q.x - im * q.y;
                im = re * q.y + im * q.x;
                re = r;
            }
            q.px = q.px - (bn * re - an * im);
            q.py = q.py + (bn * im + an * re);
            track_a_drift<S>(s + 1 < num_steps ? 2.0 * h : h, q, p0c, mc2);
        }
        offset_unset<S>(c[C_XO], c[C_YO], c[C_SIN], c[C_COS], q);
    } else if (KIND == CHX_DKD_RFCAVITY) {
        // Bmad's rfcavity (bmad_standard) from the building blocks of the TDC branch below: half a drift, the energy kick
        // dE = |n_q| V sin(2 pi (phase0 - f t)) at the particle's own time offset t, half a drift. The kick depends on z alone and
        // changes pz alone, so it is symplectic; the reference energy stays (the storage-ring convention). The phase f t is
        // reduced in turns before any sine is taken; sin(a - b) by the addition theorem from the element's S0, C0.
        const S half = c[C_A] / 2.0, volt = c[C_B], S0 = c[C_C], C0 = c[C_D], freq = c[C_E2];
        track_a_drift<S>(half, q, p0c, mc2);
        const S pc_old = (1.0 + q.pz) * p0c;
        const S E_old = m_sqrt(pc_old * pc_old + mc2 * mc2);
        const S beta_old = pc_old / E_old;
        const S time = -q.z / (beta_old * kC);  // bmadx.py:301-310
        S sn, cs;
        turn_sincos(freq * time, sn, cs);
        const S dE = volt * (S0 * cs - C0 * sn);
        const S E_new = E_old + dE;
        const S pc = m_sqrt(E_new * E_new - mc2 * mc2);          // (E_new < m: NaN, and the particle is lost by the loss rule)
        const S beta = pc / E_new;
        // pz = (pc - p0c) / p0c as an increment, pc^2 - pc_old^2 = dE (2 E_old + dE): no digits of pz are lost to the size of the
        // energy (one rounding of the kick, not three of the momentum), and dE = 0 leaves pz as it is
        q.pz = q.pz + dE * (2.0 * E_old + dE) / ((pc + pc_old) * p0c);
        q.z = q.z * beta / beta_old;
        track_a_drift<S>(half, q, p0c, mc2);
    } else {  // TDC, transverse_deflecting_cavity.py:147-193
        const S half = c[C_A] / 2.0, volt = c[C_B], k_rf = c[C_C], phase0 = c[C_D], freq = c[C_E2];
        offset_set<S>(c[C_XO], c[C_YO], c[C_SIN], c[C_COS], q);
        track_a_drift<S>(half, q, p0c, mc2);
        const S pc_old = (1.0 + q.pz) * p0c;
        const S beta_old = pc_old / m_sqrt(pc_old * pc_old + mc2 * mc2);
        const S time = -q.z / (beta_old * kC);  // bmadx.py:301-310
        const S phase = 2.0 * kPi * (phase0 - time * freq);
        q.px = q.px + volt * m_sin(phase);
        const S E_old = pc_old / beta_old;
        const S E_new = E_old + volt * m_cos(phase) * k_rf * q.x * p0c;
        const S pc = m_sqrt(E_new * E_new - mc2 * mc2);
        const S beta = pc / E_new;
        q.pz = (pc - p0c) / p0c;
        q.z = q.z * beta / beta_old;
        track_a_drift<S>(half, q, p0c, mc2);
        offset_unset<S>(c[C_XO], c[C_YO], c[C_SIN], c[C_COS], q);
    }
}

// cheetah coordinates -> Bmad -> element -> cheetah (out[0..5])
template <int KIND, typename S>
__device__ __forceinline__ void dkd_map(const S* c, const S (&in)[6], double mc2, int num_steps, S (&out)[6]) {
    Bmad<S> q;
    q.x = in[0]; q.px = in[1]; q.y = in[2]; q.py = in[3];
    to_bmad<S>(in[4], in[5], c[C_E], mc2, c[C_P0C], q.z, q.pz);
    dkd_particle<KIND, S>(c, q, mc2, num_steps);
    out[0] = q.x; out[1] = q.px; out[2] = q.y; out[3] = q.py;
    from_bmad<S>(q.z, q.pz, c[C_P0C], mc2, out[4], out[5]);
}

// C: the scalar the per-particle map is evaluated in — double (default, whatever the storage dtype) or F32 (float32 beams with
// `precision = storage`: the reference's own arithmetic width, HBM-bound instead of fp64-VALU-bound).
template <typename C> struct dkd_scalar;
template <> struct dkd_scalar<double> {
    __device__ static __forceinline__ double from(double v) { return v; }
    __device__ static __forceinline__ double to(double v) { return v; }
};
template <> struct dkd_scalar<F32> {
    __device__ static __forceinline__ F32 from(double v) { return mkf((float)v); }
    __device__ static __forceinline__ double to(F32 v) { return (double)v.v; }
};

template <typename T, int KIND, typename C = double>
__global__ __launch_bounds__(CHX_BLOCK) void dkd_kernel(const T* __restrict__ x_in, const T* __restrict__ params,
                                                        const T* __restrict__ energy, double mc2, double nq,
                                                        int num_steps, int fringe, int P, int64_t B, int64_t Bx,
                                                        int64_t Bp, int64_t Be, int64_t N, T* __restrict__ x_out,
                                                        T* __restrict__ energy_out, int in_vec_ok, int out_vec_ok) {
    constexpr int TP = CHX_BLOCK;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    __shared__ double cst_[C_N + 1];
    __shared__ C cstc_[C_N + 1];

    const chx_tile<TP> tc = chx_tile_coords<TP>(N);
    const int64_t b = tc.b, t = tc.t, n0 = tc.n0;
    const int np = tc.np();
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const bool in_vec = CHX_TILE_VEC_OK(T, in_vec_ok, in_row, N), out_vec = CHX_TILE_VEC_OK(T, out_vec_ok, b, N);

    if (threadIdx.x == 0) {
        const T Eb = energy[(Be == 1) ? 0 : b];
        double par[CHX_MAX_PARAMS];
        for (int k = 0; k < P; ++k) par[k] = (double)params[((Bp == 1) ? 0 : b) * P + k];
        dkd_constants<double>(KIND, par, (double)Eb, mc2, nq, fringe, cst_);      // per-row constants: always in double
        for (int k = 0; k <= C_N; ++k) cstc_[k] = dkd_scalar<C>::from(cst_[k]);
        if (t == 0 && energy_out) {
            // ref_energy of bmad_to_cheetah_z_pz (bmadx.py:49), in the storage dtype like the reference
            const T m = (T)mc2;
            const T p0 = sqrt(Eb * Eb - m * m);
            energy_out[b] = sqrt(p0 * p0 + m * m);
        }
    }
    tile_load<T, TP>(x_in + (in_row * N + n0) * 7, lds, np * 7, in_vec, !(Bx == 1 && B > 1));
    __syncthreads();

    const int p = threadIdx.x;
    if (p < np) {
        C in[6], out[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) in[j] = dkd_scalar<C>::from((double)lds[p * 7 + j]);
        dkd_map<KIND, C>(cstc_, in, mc2, num_steps, out);
#pragma unroll
        for (int j = 0; j < 6; ++j) lds[p * 7 + j] = (T)dkd_scalar<C>::to(out[j]);
        lds[p * 7 + 6] = (T)1;
    }
    __syncthreads();
    tile_store<T, TP>(x_out + (b * N + n0) * 7, lds, np * 7, out_vec, true);
}

// ---- float32 beams, MIXED arithmetic (Drift, Quadrupole, Sextupole): the default of float32 beams ---------------------------
// Where does a float32 evaluation of the Bmad-X maps lose its digits? Not in the transverse map (x, px, y, py move by parts in
// 1e3 per element; seven significant digits of each step are what the float32 STORAGE keeps anyway) — in the longitudinal pair:
// pz = (p - p0c) / p0c and delta = (E - E_ref) / p0c subtract numbers that agree to three or four digits (bmadx.py:7-56), the
// low-energy correction subtracts beta - beta0 ~ 1e-8 (bmadx.py:184-216), and z collects increments of 1e-9 into a value of
// 1e-5. Measured over the 100 elements of the benchmark lattice: tau off by 1e-2 of its scale, delta by 4e-4 in float32
// arithmetic (the reference's own float32 run: 8e-3 / 4e-5), 5e-7 / 7e-14 in float64 arithmetic — at 2-3 times the kernel time,
// because then the per-particle cos / sin / cosh / sinh of the quadrupole and five square roots run in fp64 as well.
// Here: the (tau, delta) <-> (z, pz) conversions, the z accumulator, the low-energy correction and the misalignment shift run in
// fp64 — one square root and one reciprocal per particle, both from the hardware seeds (delta' is formed from the particle's
// own energy: pz does not change inside these two elements, so the round trip through p is the identity) — everything else in
// float32, including the increments of z (a RELATIVE error of 1e-7 on an increment is 1e-16 of z's scale).
enum { C_ETOT = C_N + 1, C_BETA0, C_ME2, C_INVP0C, C_INVBETA0, C_MIXED_N };
// the extra constants of the mixed evaluation, behind dkd_constants' (lane 0 of a workgroup / of a prepare kernel)
__device__ __forceinline__ void dkd_mixed_constants(double* cst_, double mc2) {
    const double p0c = cst_[C_P0C];
    const double e_tot = sqrt(p0c * p0c + mc2 * mc2);
    cst_[C_ETOT] = e_tot;
    cst_[C_BETA0] = p0c / e_tot;
    cst_[C_ME2] = (mc2 / e_tot) * (mc2 / e_tot);
    cst_[C_INVP0C] = 1.0 / p0c;
    cst_[C_INVBETA0] = e_tot / p0c;
}
// fp64 square root and reciprocal from the hardware seeds (v_rsq_f64 / v_rcp_f64, ~2^-26) and Newton steps in fused multiply-adds:
// a few ulp of a double, a third of the instructions of the correctly rounded library forms. What they feed is rounded to float32
// at the end of the element (2^-24): the extra 2^-51 is invisible there.
__device__ __forceinline__ double dkd_sqrt_fast(double a) {
    double y = __builtin_amdgcn_rsq(a);
    y = y * fma(-0.5 * a, y * y, 1.5);
    y = y * fma(-0.5 * a, y * y, 1.5);
    double s = a * y;
    s = fma(0.5 * y, fma(-s, s, a), s);
    return a == 0.0 ? 0.0 : s;
}
__device__ __forceinline__ double dkd_rcp_fast(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(r, fma(-d, r, 1.0), r);
    r = fma(r, fma(-d, r, 1.0), r);
    return r;
}
// one particle through one element, v = (x, px, y, py, tau, delta) in float32 before and after
template <int KIND>
__device__ __forceinline__ void dkd_mixed_particle(const double* __restrict__ cst_, double mc2, int num_steps, float (&v)[6]) {
    // A quadrupole that is shifted off the axis (quadrupole.py:199-215 subtracts the misalignment before its map): the shifted
    // coordinate may be hundreds of beam sizes, float32 steps on it lose digits of the BEAM's scale and its path-length terms
    // dwarf tau — such an element is evaluated in float64 like dkd_kernel<float, ., double> (workgroup-uniform decision).
    // A shifted sextupole likewise: its kick is quadratic in the shifted coordinate. A shifted Multipole as a shifted Sextupole.
    if ((KIND == CHX_DKD_QUADRUPOLE || KIND == CHX_DKD_SEXTUPOLE || KIND == CHX_DKD_MULTIPOLE) && (cst_[C_XO] != 0.0 || cst_[C_YO] != 0.0)) {
        double in[6], out[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) in[j] = (double)v[j];
        dkd_map<KIND, double>(cst_, in, mc2, num_steps, out);
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] = (float)out[j];
        return;
    }
    const double E = cst_[C_E], p0c = cst_[C_P0C];
    float x = v[0], px = v[1], y = v[2], py = v[3];
    const double tau = (double)v[4], delta = (double)v[5];
    // (tau, delta) -> (z, pz), bmadx.py:7-31, fp64
    const double inv_p0c = cst_[C_INVP0C];
    const double en = E + delta * p0c;
    const double pc = dkd_sqrt_fast(en * en - mc2 * mc2);
    const double r = dkd_rcp_fast(pc * en);
    const double beta = (pc * pc) * r, inv_beta = (en * en) * r;          // pc / en and en / pc from one reciprocal
    double z = -beta * tau;
    const double pz = (pc - p0c) * inv_p0c;
    const float pzf = (float)pz, mc2f = (float)mc2, p0cf = (float)p0c;
    const float relp = 1.0f + pzf;
    if (KIND == CHX_DKD_DRIFT) {                                  // bmadx.py:263-298
        const float L = (float)cst_[C_A];
        const float ir = __builtin_amdgcn_rcpf(relp);
        const float Px = px * ir, Py = py * ir;
        const float Pxy2 = Px * Px + Py * Py;
        const float Pl = __builtin_amdgcn_sqrtf(1.0f - Pxy2);
        const float iPl = __builtin_amdgcn_rcpf(Pl);
        const float pcf = p0cf * relp, m2 = mc2f * mc2f;
        const float a = (m2 * (2.0f * pzf + pzf * pzf)) * __builtin_amdgcn_rcpf(pcf * pcf + m2);
        const float so_a = a * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(1.0f + a) + 1.0f);          // sqrt_one(a)
        const float so_b = -Pxy2 * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(1.0f - Pxy2) + 1.0f);   // sqrt_one(-Pxy2)
        x = x + L * Px * iPl;
        y = y + L * Py * iPl;
        z = z + (double)(L * (so_a + so_b * iPl));
    } else if (KIND == CHX_DKD_SEXTUPOLE || KIND == CHX_DKD_MULTIPOLE) {   // drifts as in the branch above around float32 kicks
        const double sn = cst_[C_SIN], cs = cst_[C_COS];          // (here xo = yo = 0: the rotations as in the quadrupole's branch)
        const bool upright = sn == 0.0 && cs == 1.0;
        if (!upright) {
            const float xr = (float)((double)x * cs + (double)y * sn), yr = (float)(-(double)x * sn + (double)y * cs);
            const float pxr = (float)((double)px * cs + (double)py * sn), pyr = (float)(-(double)px * sn + (double)py * cs);
            x = xr; y = yr; px = pxr; py = pyr;
        }
        const float h = (float)cst_[C_A] / (2.0f * (float)num_steps), kappa = (float)cst_[C_B] / (float)num_steps;
        // (a Multipole: kappa = knl / (m! n), skew = ksl / (m! n), and the order m — see dkd_particle)
        const float skew = KIND == CHX_DKD_MULTIPOLE ? (float)cst_[C_C] / (float)num_steps : 0.0f;
        const int order = KIND == CHX_DKD_MULTIPOLE ? (int)cst_[C_D] : 2;
        // pz does not change inside the magnet: 1 / (1 + pz) and the energy term of dz are the same for every drift
        const float ir = __builtin_amdgcn_rcpf(relp);
        const float pcf = p0cf * relp, m2 = mc2f * mc2f;
        const float a = (m2 * (2.0f * pzf + pzf * pzf)) * __builtin_amdgcn_rcpf(pcf * pcf + m2);
        const float so_a = a * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(1.0f + a) + 1.0f);          // sqrt_one(a)
        for (int s = 0; s <= num_steps; ++s) {
            if (s > 0 && KIND == CHX_DKD_SEXTUPOLE) {
                px = px - 0.5f * kappa * (x * x - y * y);
                py = py + kappa * x * y;
            } else if (s > 0) {
                float re = 1.0f, im = 0.0f;
                for (int k = 0; k < order; ++k) {
                    const float r = re * x - im * y;
                    im = re * y + im * x;
                    re = r;
                }
                px = px - (kappa * re - skew * im);
                py = py + (kappa * im + skew * re);
            }
            const float L = (s == 0 || s == num_steps) ? h : 2.0f * h;
            const float Px = px * ir, Py = py * ir;
            const float Pxy2 = Px * Px + Py * Py;
            const float Pl = __builtin_amdgcn_sqrtf(1.0f - Pxy2);
            const float iPl = __builtin_amdgcn_rcpf(Pl);
            const float so_b = -Pxy2 * __builtin_amdgcn_rcpf(Pl + 1.0f);                                // sqrt_one(-Pxy2)
            x = x + L * Px * iPl;
            y = y + L * Py * iPl;
            z = z + (double)(L * (so_a + so_b * iPl));            // every increment of z into the fp64 accumulator
        }
        if (!upright) {
            const double xi = (double)x * cs - (double)y * sn, yi = (double)x * sn + (double)y * cs;
            const float pxr = (float)((double)px * cs - (double)py * sn), pyr = (float)((double)px * sn + (double)py * cs);
            x = (float)xi; y = (float)yi; px = pxr; py = pyr;
        }
    } else {                                                      // quadrupole.py:168-251, bmadx.py:219-252
        const double xo = cst_[C_XO], yo = cst_[C_YO], sn = cst_[C_SIN], cs = cst_[C_COS];
        // (here xo = yo = 0.) An upright quadrupole — sin(tilt) = 0, cos(tilt) = 1 — is rotated by the identity: x * 1 + y * 0 is
        // x again, so the two rotations are left out (wave-uniform), value for value the same result
        const bool upright = sn == 0.0 && cs == 1.0;
        if (!upright) {   // offset_set: the shift by the misalignment in fp64 (it may be hundreds of beam sizes), the rotation with it
            const double xi = (double)x - xo, yi = (double)y - yo;
            const float xr = (float)(xi * cs + yi * sn), yr = (float)(-xi * sn + yi * cs);
            const float pxr = (float)((double)px * cs + (double)py * sn), pyr = (float)(-(double)px * sn + (double)py * cs);
            x = xr; y = yr; px = pxr; py = pyr;
        }
        const float L = (float)cst_[C_A], b1 = (float)cst_[C_B];
        const float step = L / (float)num_steps;
        const F32 k1 = mkf(b1 * __builtin_amdgcn_rcpf(L * relp));
        const QuadCoef<F32> tx = quad_coefficients<F32>(-k1, mkf(step), mkf(relp));
        const QuadCoef<F32> ty = quad_coefficients<F32>(k1, mkf(step), mkf(relp));
        // low_energy_z_correction (bmadx.py:184-216) in fp64: beta - beta0 cancels to 1e-8
        double dzc;
        {
            const double e_tot = cst_[C_ETOT], beta0 = cst_[C_BETA0], me2 = cst_[C_ME2];
            const double b0pz = beta0 * pz, b02 = beta0 * beta0, ds = (double)step;
            if (mc2 * (b0pz * b0pz) < 3e-7 * e_tot)
                dzc = ds * pz * (1.0 - 3.0 * (pz * b02) / 2.0 + pz * pz * b02 * (2.0 * b02 - me2 / 2.0)) * me2;
            else
                dzc = ds * (beta - beta0) * cst_[C_INVBETA0];     // (beta of this particle: pc / en above)
        }
        for (int s = 0; s < num_steps; ++s) {
            const float dz = tx.c1.v * (x * x) + tx.c2.v * x * px + tx.c3.v * (px * px) + ty.c1.v * (y * y) + ty.c2.v * y * py +
                             ty.c3.v * (py * py);
            const float xn = tx.a11.v * x + tx.a12.v * px, pxn = tx.a21.v * x + tx.a22.v * px;
            const float yn = ty.a11.v * y + ty.a12.v * py, pyn = ty.a21.v * y + ty.a22.v * py;
            x = xn; px = pxn; y = yn; py = pyn;
            z = z + (double)dz + dzc;
        }
        if (!upright) {   // offset_unset
            const double xi = (double)x * cs - (double)y * sn, yi = (double)x * sn + (double)y * cs;
            const float pxr = (float)((double)px * cs - (double)py * sn), pyr = (float)((double)px * sn + (double)py * cs);
            x = (float)(xi + xo); y = (float)(yi + yo); px = pxr; py = pyr;
        }
    }
    // (z, pz) -> (tau, delta), bmadx.py:34-56: pz is unchanged, so p = pc and the particle's energy is `en` again
    const double ref = cst_[C_ETOT];
    v[0] = x; v[1] = px; v[2] = y; v[3] = py;
    v[4] = (float)(-z * inv_beta);
    v[5] = (float)((en - ref) * inv_p0c);
}

// (the kernel's text, shared by dkd_mixed_kernel and dkd_mixed_multipole_kernel; `fringe` is what dkd_constants receives)
template <int KIND>
__device__ __forceinline__ void dkd_mixed_tile(const float* __restrict__ x_in, const float* __restrict__ params,
                                               const float* __restrict__ energy, double mc2, double nq, int num_steps, int fringe,
                                               int P, int64_t B, int64_t Bx, int64_t Bp, int64_t Be, int64_t N,
                                               float* __restrict__ x_out, float* __restrict__ energy_out,
                                               int in_vec_ok, int out_vec_ok) {
    constexpr int TP = CHX_BLOCK;
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    __shared__ double cst_[C_MIXED_N];
    const chx_tile<TP> tc = chx_tile_coords<TP>(N);
    const int64_t b = tc.b, t = tc.t, n0 = tc.n0;
    const int np = tc.np();
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const bool in_vec = CHX_TILE_VEC_OK(float, in_vec_ok, in_row, N), out_vec = CHX_TILE_VEC_OK(float, out_vec_ok, b, N);
    tile_load<float, TP>(x_in + (in_row * N + n0) * 7, lds, np * 7, in_vec, !(Bx == 1 && B > 1));   // rows first: the constants
    if (threadIdx.x == 0) {                                                                          // are formed under the loads
        const float Eb = energy[(Be == 1) ? 0 : b];
        double par[CHX_MAX_PARAMS];
        for (int k = 0; k < P; ++k) par[k] = (double)params[((Bp == 1) ? 0 : b) * P + k];
        dkd_constants<double>(KIND, par, (double)Eb, mc2, nq, fringe, cst_);
        dkd_mixed_constants(cst_, mc2);
        if (t == 0 && energy_out) {
            const float m = (float)mc2;
            const float p0 = sqrtf(Eb * Eb - m * m);
            energy_out[b] = sqrtf(p0 * p0 + m * m);
        }
    }
    __syncthreads();
    const int p = threadIdx.x;
    if (p < np) {
        float v[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] = lds[p * 7 + j];
        dkd_mixed_particle<KIND>(cst_, mc2, num_steps, v);
#pragma unroll
        for (int j = 0; j < 6; ++j) lds[p * 7 + j] = v[j];
        lds[p * 7 + 6] = 1.0f;
    }
    __syncthreads();
    tile_store<float, TP>(x_out + (b * N + n0) * 7, lds, np * 7, out_vec, true);
}

template <int KIND>
__global__ __launch_bounds__(CHX_BLOCK) void dkd_mixed_kernel(const float* __restrict__ x_in, const float* __restrict__ params,
                                                              const float* __restrict__ energy, double mc2, double nq, int num_steps,
                                                              int P, int64_t B, int64_t Bx, int64_t Bp, int64_t Be, int64_t N,
                                                              float* __restrict__ x_out, float* __restrict__ energy_out,
                                                              int in_vec_ok, int out_vec_ok) {
    dkd_mixed_tile<KIND>(x_in, params, energy, mc2, nq, num_steps, 3, P, B, Bx, Bp, Be, N, x_out, energy_out, in_vec_ok, out_vec_ok);
}

// a Multipole in mixed arithmetic: the same with the order as an argument (the kinds above read no fringe bits)
__global__ __launch_bounds__(CHX_BLOCK) void dkd_mixed_multipole_kernel(const float* __restrict__ x_in, const float* __restrict__ params,
                                                                        const float* __restrict__ energy, double mc2, double nq,
                                                                        int num_steps, int order, int P, int64_t B, int64_t Bx, int64_t Bp,
                                                                        int64_t Be, int64_t N, float* __restrict__ x_out,
                                                                        float* __restrict__ energy_out, int in_vec_ok, int out_vec_ok) {
    dkd_mixed_tile<CHX_DKD_MULTIPOLE>(x_in, params, energy, mc2, nq, num_steps, order, P, B, Bx, Bp, Be, N, x_out, energy_out, in_vec_ok,
                                      out_vec_ok);
}

// Backward of the above. dx[n][m] = sum_i dY[n][i] d out_i / d in_m (six passes, coordinate m seeded), and per
// parameter k (then the energy) the workgroup's sum over its particles of dY . d out / d theta_k, written to
// partials[b][tile][k] — summed by the caller (no atomics: deterministic, and 10 same-address atomics per workgroup
// would serialise). Forward-mode costs (6 + P + 1) evaluations per particle; the pass stays far cheaper than the
// reference's autograd graph through ~100 tensor ops per element.
template <typename T, int KIND>
__global__ __launch_bounds__(CHX_BLOCK) void dkd_bwd_kernel(const T* __restrict__ x_in, const T* __restrict__ params,
                                                            const T* __restrict__ energy, const T* __restrict__ dY,
                                                            double mc2, double nq, int num_steps, int fringe, int P,
                                                            int64_t B, int64_t Bx, int64_t Bp, int64_t Be, int64_t N,
                                                            T* __restrict__ dx, double* __restrict__ partials) {
    constexpr int TP = CHX_BLOCK;
    __shared__ Dual cd[C_N + 1];
    __shared__ double red[CHX_BLOCK / 64];

    const chx_tile<TP> tc = chx_tile_coords<TP>(N);
    const int64_t b = tc.b, t = tc.t, in_row = (Bx == 1) ? 0 : b;
    const int64_t n = tc.n0 + threadIdx.x;
    const bool live = n < N;
    const T Eb = energy[(Be == 1) ? 0 : b];
    const T* par = params + ((Bp == 1) ? 0 : b) * P;

    double xv[6], g[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        xv[j] = live ? (double)x_in[(in_row * N + n) * 7 + j] : 0.0;
        g[j] = live ? (double)dY[(b * N + n) * 7 + j] : 0.0;
    }

    auto constants = [&](int seed) {  // seed in [0, P): parameter, P: energy, -1: none
        if (threadIdx.x == 0) {
            Dual pd[CHX_MAX_PARAMS];
            for (int k = 0; k < P; ++k) pd[k] = mk((double)par[k], k == seed ? 1.0 : 0.0);
            dkd_constants<Dual>(KIND, pd, mk((double)Eb, seed == P ? 1.0 : 0.0), mc2, nq, fringe, cd);
        }
        __syncthreads();
    };

    if (dx) {
        constants(-1);
        if (live) {
#pragma unroll 1
            for (int m = 0; m < 6; ++m) {
                Dual in[6], out[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) in[j] = mk(xv[j], j == m ? 1.0 : 0.0);
                dkd_map<KIND, Dual>(cd, in, mc2, num_steps, out);
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 6; ++j) acc += g[j] * out[j].d;
                dx[(b * N + n) * 7 + m] = (T)acc;
            }
            dx[(b * N + n) * 7 + 6] = (T)0;
        }
        __syncthreads();
    }
    if (partials) {
#pragma unroll 1
        for (int k = 0; k <= P; ++k) {
            constants(k);
            double acc = 0.0;
            if (live) {
                Dual in[6], out[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) in[j] = mk(xv[j], 0.0);
                dkd_map<KIND, Dual>(cd, in, mc2, num_steps, out);
#pragma unroll
                for (int j = 0; j < 6; ++j) acc += g[j] * out[j].d;
            }
            acc = chx_wave_sum(acc);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
            __syncthreads();
            if (threadIdx.x == 0) {
                double tot = 0.0;
                for (int w = 0; w < CHX_BLOCK / 64; ++w) tot += red[w];
                partials[(b * tc.tiles_per_row + t) * (P + 1) + k] = tot;
            }
            __syncthreads();
        }
    }
}

// ---- the one-turn map of a ring of drift-kick-drift items with its 6 x 6 Jacobian, and the closed orbit (chx_dkd_ring_jacobian) -----
// One lane per (seed, tangent direction): the lane carries the phase-space point and ONE tangent through all E items as six Dual
// numbers in registers, dkd_map<KIND, Dual> item after item — the instantiations dkd_bwd_kernel compiles, in float64 whatever the
// settings' dtype. A seed is a group of chx_optics::kGroup = 8 consecutive lanes (tangents e_0 .. e_5, two lanes without one),
// eight seeds are the one wave of a workgroup: nothing of a seed leaves its wave, the only barrier is the wave's own.
// The item's constants come from the 56-double block dkd_chain_prepare_kernel leaves (what a turn of chx_dkd_turns reads) through
// wave-uniform scalar loads and become Dual with a zero tangent per lane as the item is reached: their values stay in scalar
// registers, no LDS round trip and no barrier per item (DESIGN.md has the register figures).
// After a pass the group gathers M (lane m holds column m) in LDS; lane 0 of the group takes the Newton step of the closed orbit on
// the closed coordinates (chx_optics_dev.h), every lane of the group adds it. `passes` is the same for every seed: a seed that
// has converged keeps stepping (by rounding-size steps), a seed that cannot converge is NaN in its own rows, and two calls give
// the same bits. The last pass starts from the final point and is the one whose image, matrix and per-item records are stored.
constexpr int kRingCstStride = 56, kRingMeta = 54;          // kDkdCstStride, kDkdMeta below (asserted equal at the entry point)

// What dkd_ring_radiation_kernel and dkd_ring_sensitivity_kernel do per item, each stated once; S = Dual or Dual2.
// dkd_ring_jacobian_kernel has the same WRITTEN OUT, as it always had: on any of these helpers its registers are allocated otherwise,
// and the NaNs a lost seed of a plain map (mode 0) leaves in the records along the ring — the one place where a ring kernel stores
// NaNs as the maps made them — came out with the other sign bit (profiles/dkd_entry_points.md). A new kind: a line there, a line here.
__device__ __forceinline__ Dual ring_constant(Dual, double c, const double*, int) { return mk(c, 0.0); }
__device__ __forceinline__ Dual2 ring_constant(Dual2, double c, const double* dc, int k) { return mk2(c, 0.0, dc[k], 0.0); }
__device__ __forceinline__ double ring_row(Dual v) { return v.v; }
__device__ __forceinline__ double ring_row(Dual2 v) { return v.b; }
__device__ __forceinline__ double ring_column(Dual v) { return v.d; }
__device__ __forceinline__ double ring_column(Dual2 v) { return v.ab; }
// an item's constants (block c of cst) as S, its kind and step count. Dual2: the knob's tangent dc[kSensStride] in the e2 part.
template <typename S>
__device__ __forceinline__ void ring_item_load(const double* __restrict__ c, const double* __restrict__ dc, S (&cd)[C_N + 1], int& kind, int& steps) {
    const int32_t* w = reinterpret_cast<const int32_t*>(c + kRingMeta);
    kind = w[0];
    steps = w[1];
#pragma unroll
    for (int k = 0; k <= C_N; ++k) cd[k] = ring_constant(S{}, c[k], dc, k);
}
// the map of an item of any ring kind. BEND as in dkd_items: false compiles no Dipole in (the caller has dealt with that kind).
template <bool BEND, typename S>
__device__ __forceinline__ void dkd_map_kind(int kind, const S* cd, const S (&v)[6], double mc2, int steps, S (&out)[6]) {
    if (kind == CHX_DKD_DRIFT) dkd_map<CHX_DKD_DRIFT, S>(cd, v, mc2, steps, out);
    else if (kind == CHX_DKD_QUADRUPOLE) dkd_map<CHX_DKD_QUADRUPOLE, S>(cd, v, mc2, steps, out);
    else if (BEND && kind == CHX_DKD_DIPOLE) dkd_map<CHX_DKD_DIPOLE, S>(cd, v, mc2, steps, out);
    else if (kind == CHX_DKD_SEXTUPOLE) dkd_map<CHX_DKD_SEXTUPOLE, S>(cd, v, mc2, steps, out);
    else if (kind == CHX_DKD_RFCAVITY) dkd_map<CHX_DKD_RFCAVITY, S>(cd, v, mc2, steps, out);
    else dkd_map<CHX_DKD_MULTIPOLE, S>(cd, v, mc2, steps, out);
}
// record `row` of the records along the ring: the lane of tangent m < 6 stores column m of the matrix, lane 0 the orbit row as well
template <typename S>
__device__ __forceinline__ void ring_record_store(const S (&v)[6], int m, int64_t row, double* __restrict__ matrix_along, double* __restrict__ orbit_along) {
#pragma unroll
    for (int i = 0; i < 6; ++i) matrix_along[row * 36 + i * 6 + m] = ring_column(v[i]);
    if (m == 0) {
#pragma unroll
        for (int i = 0; i < 6; ++i) orbit_along[row * 6 + i] = ring_row(v[i]);
    }
}
// a point with a coordinate that is not finite (NaN, or beyond the largest double): its seed is lost
template <typename S>
__device__ __forceinline__ bool ring_lost(const S (&v)[6]) {
    bool lost = false;
#pragma unroll
    for (int i = 0; i < 6; ++i) lost = lost || !(fabs(val(v[i])) <= 1.79769313486231570815e308);
    return lost;
}

struct RingJacobianOut {
    double* orbit;          // [B][6]
    double* image;          // [B][6]
    double* matrix;         // [B][6][6]
    double* residual;       // [B]
    double* dispersion;     // [B][4]
    double* orbit_along;    // [B][E + 1][6] or null
    double* matrix_along;   // [B][E + 1][6][6] or null
    void* s_along;          // [E + 1] in the settings' dtype or null
};

__global__ __launch_bounds__(chx_optics::kLanes) void dkd_ring_jacobian_kernel(const double* __restrict__ cst, int E, double mc2,
                                                                              const double* __restrict__ start, int64_t B, int mode,
                                                                              int passes, int s_is_f32, RingJacobianOut o) {
    using namespace chx_optics;
    __shared__ double sM[kSeeds][36];
    __shared__ double sA[kSeeds][36];
    __shared__ double sF[kSeeds][6];
    __shared__ double sStep[kSeeds][6];
    const int lane = threadIdx.x, g = group_of_lane(lane), m = tangent_of_lane(lane);
    bool live;
    const int64_t seed = seed_of_group(blockIdx.x, g, B, live);
    const bool column = live && m < 6;                        // the lane stores column m of its seed's matrices
    const int n = closed_count(mode);

    if (blockIdx.x == 0 && lane == 0 && o.s_along) {          // the path length behind every item, added in the settings' dtype
        if (s_is_f32) {
            float* s_out = (float*)o.s_along;
            float s = 0.0f;
            s_out[0] = s;
            for (int e = 0; e < E; ++e) s_out[e + 1] = s = s + (float)cst[(int64_t)e * kRingCstStride + C_A];
        } else {
            double* s_out = (double*)o.s_along;
            double s = 0.0;
            s_out[0] = s;
            for (int e = 0; e < E; ++e) s_out[e + 1] = s = s + cst[(int64_t)e * kRingCstStride + C_A];
        }
    }

    double x[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) x[j] = start[seed * 6 + j];

#pragma unroll 1
    for (int pass = 0; pass < passes; ++pass) {
        const bool last = pass == passes - 1;
        const bool along = last && o.matrix_along != nullptr;
        Dual v[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] = mk(x[j], j == m ? 1.0 : 0.0);
        if (along && column) {
            double* Ma = o.matrix_along + seed * (int64_t)(E + 1) * 36;
#pragma unroll
            for (int i = 0; i < 6; ++i) Ma[i * 6 + m] = v[i].d;
            if (m == 0) {
                double* xa = o.orbit_along + seed * (int64_t)(E + 1) * 6;
#pragma unroll
                for (int i = 0; i < 6; ++i) xa[i] = v[i].v;
            }
        }
#pragma unroll 1
        for (int e = 0; e < E; ++e) {
            const double* __restrict__ c = cst + (int64_t)e * kRingCstStride;
            const int32_t* w = reinterpret_cast<const int32_t*>(c + kRingMeta);
            const int kind = w[0], steps = w[1];
            Dual cd[C_N + 1], out[6];
#pragma unroll
            for (int k = 0; k <= C_N; ++k) cd[k] = mk(c[k], 0.0);
            if (kind == CHX_DKD_DRIFT) dkd_map<CHX_DKD_DRIFT, Dual>(cd, v, mc2, steps, out);
            else if (kind == CHX_DKD_QUADRUPOLE) dkd_map<CHX_DKD_QUADRUPOLE, Dual>(cd, v, mc2, steps, out);
            else if (kind == CHX_DKD_DIPOLE) dkd_map<CHX_DKD_DIPOLE, Dual>(cd, v, mc2, steps, out);
            else if (kind == CHX_DKD_SEXTUPOLE) dkd_map<CHX_DKD_SEXTUPOLE, Dual>(cd, v, mc2, steps, out);
            else if (kind == CHX_DKD_RFCAVITY) dkd_map<CHX_DKD_RFCAVITY, Dual>(cd, v, mc2, steps, out);
            else dkd_map<CHX_DKD_MULTIPOLE, Dual>(cd, v, mc2, steps, out);
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = out[j];
            if (along && column) {
                double* Ma = o.matrix_along + (seed * (int64_t)(E + 1) + e + 1) * 36;
#pragma unroll
                for (int i = 0; i < 6; ++i) Ma[i * 6 + m] = v[i].d;
                if (m == 0) {
                    double* xa = o.orbit_along + (seed * (int64_t)(E + 1) + e + 1) * 6;
#pragma unroll
                    for (int i = 0; i < 6; ++i) xa[i] = v[i].v;
                }
            }
        }
        // the group's matrix and image in LDS: lane m < 6 holds column m
        if (m < 6) {
#pragma unroll
            for (int i = 0; i < 6; ++i) sM[g][i * 6 + m] = v[i].d;
        }
        if (m == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) sF[g][i] = v[i].v;
        }
        __syncthreads();
        if (!last) {
            if (m == 0) newton_step(n, sM[g], sF[g], x, sA[g], sStep[g]);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (j < n) x[j] = x[j] + sStep[g][j];
            __syncthreads();
            continue;
        }
        // a seed whose image is not finite (beyond the dynamic aperture, a search that ran away) is NaN in ALL its rows — the
        // coordinates a lost particle happens to keep (delta, say) and their unit derivatives would read as results. Every lane
        // of the group sees the same values. (The seed of a plain map, mode 0, is handed back as it came.)
        bool lost = false;
#pragma unroll
        for (int i = 0; i < 6; ++i) lost = lost || !(fabs(v[i].v) <= 1.79769313486231570815e308);
        if (column) {
#pragma unroll
            for (int i = 0; i < 6; ++i) o.matrix[seed * 36 + i * 6 + m] = lost ? NAN : v[i].d;
            double xm = x[0];
#pragma unroll
            for (int j = 1; j < 6; ++j) xm = m == j ? x[j] : xm;
            o.orbit[seed * 6 + m] = (lost && mode != 0) ? NAN : xm;
            o.image[seed * 6 + m] = lost ? NAN : sF[g][m];
        }
        if (live && m == 0) {
            o.residual[seed] = lost ? NAN : closing_error(n, sF[g], x);
            dispersion(sM[g], sA[g], sStep[g]);
            if (lost) {
                for (int i = 0; i < 4; ++i) sStep[g][i] = NAN;
            }
        }
        __syncthreads();
        if (live && m < 4) o.dispersion[seed * 4 + m] = sStep[g][m];
    }
}

// ---- the synchrotron-radiation integrals of such a ring on its closed orbit (chx_dkd_ring_radiation) ----------------------------
// The Jacobian kernel's layout and one pass of it: a group of kGroup lanes per seed, lane m < 6 carries the orbit and the tangent
// e_m through all items, the constants come from the same 56-double blocks through wave-uniform loads. At a Dipole the group first
// evaluates the map from the item's entrance to the kNodes Gauss-Legendre points inside the body — dkd_map<CHX_DKD_DIPOLE, Dual>
// itself on a copy of the constants with C_A, C_B, C_D, C_E2, C_F, C_G rebuilt for the part f L, f theta and C_J = C_N = 0 (no exit
// fringe) — and then, through the same call site with the constants as they are, the whole item: ONE inlined bend, no second
// definition. After a partial map lane m holds column m of A(s); the kTerms sums of chx_radiation_dev.h are butterflies over the
// group's lanes (nothing of a seed leaves its wave, every lane ends with the same bits), the algebra from there is that header's.
// Every lane of a group accumulates the same float64 numbers in the same fixed order; lane k < 7 stores integral k. No atomics.
struct RingRadiationIn {
    const double* orbit;    // [B][6]
    const double* beta0;    // [B][2]
    const double* alpha0;   // [B][2]
    const double* eta0;     // [B][4]
};

__device__ __forceinline__ double group_butterfly(double v) {
    v = v + __shfl_xor(v, 1, chx_optics::kGroup);
    v = v + __shfl_xor(v, 2, chx_optics::kGroup);
    v = v + __shfl_xor(v, 4, chx_optics::kGroup);
    return v;
}

// the kTerms sums of the group for the point whose tangents the lanes hold in p[0..3].d
__device__ __forceinline__ void group_terms(int m, const Dual (&p)[6], const double* eta0, const double* beta0, const double* alpha0, double* s) {
    const double col[4] = {p[0].d, p[1].d, p[2].d, p[3].d};
    double t[chx_radiation::kTerms];
    chx_radiation::lane_terms(m, col, eta0, beta0, alpha0, t);
#pragma unroll
    for (int k = 0; k < chx_radiation::kTerms; ++k) s[k] = group_butterfly(t[k]);
}

__global__ __launch_bounds__(chx_optics::kLanes) void dkd_ring_radiation_kernel(const double* __restrict__ cst, int E, double mc2, RingRadiationIn in,
                                                                               int64_t B, double* __restrict__ integrals,
                                                                               double* __restrict__ along) {
    using namespace chx_optics;
    using namespace chx_radiation;
    const int lane = threadIdx.x, g = group_of_lane(lane), m = tangent_of_lane(lane);
    bool live;
    const int64_t seed = seed_of_group(blockIdx.x, g, B, live);
    const bool stores = live && m < kIntegrals;               // the lane stores integral m of its seed

    double eta0[4], beta0[2], alpha0[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) eta0[j] = in.eta0[seed * 4 + j];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        beta0[j] = in.beta0[seed * 2 + j];
        alpha0[j] = in.alpha0[seed * 2 + j];
    }
    Dual v[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = mk(in.orbit[seed * 6 + j], j == m ? 1.0 : 0.0);
    double total[kIntegrals];
#pragma unroll
    for (int k = 0; k < kIntegrals; ++k) total[k] = 0.0;

#pragma unroll 1
    for (int e = 0; e < E; ++e) {
        const double* __restrict__ c = cst + (int64_t)e * kRingCstStride;
        int kind, steps;
        Dual cd[C_N + 1], out[6];
        ring_item_load<Dual>(c, nullptr, cd, kind, steps);
        double part[kIntegrals];
#pragma unroll
        for (int k = 0; k < kIntegrals; ++k) part[k] = 0.0;
        if (kind == CHX_DKD_DIPOLE) {
            const double L = c[C_A], theta = c[C_B], h = c[C_C], cos_t = c[C_COS], sin_t = c[C_SIN];
            const double rel_beta = c[C_P0C] / c[C_E];
            const bool bends = L != 0.0 && theta != 0.0;      // (wave-uniform) else zeros and the item alone
            double s[kTerms], eta[4], eta_in = 0.0;
            BendSums sums = bend_sums_zero();
            if (bends) {
                group_terms(m, v, eta0, beta0, alpha0, s);
                eta_from_sums(s, rel_beta, eta);
                eta_in = eta_bend(eta, cos_t, sin_t);
            }
#pragma unroll 1
            for (int j = bends ? 0 : kNodes; j <= kNodes; ++j) {
                const bool inside = j < kNodes;               // a point inside the body; j == kNodes: the whole item
                Dual cj[C_N + 1];
#pragma unroll
                for (int k = 0; k <= C_N; ++k) cj[k] = cd[k];
                if (inside) {
                    const double f = gl8_node(j), Lf = f * L, tf = f * theta;
                    cj[C_A] = mk(Lf, 0.0);
                    cj[C_B] = mk(tf, 0.0);
                    cj[C_D] = mk(sinc1<double>(tf), 0.0);
                    cj[C_E2] = mk(cosc1<double>(tf), 0.0);
                    cj[C_F] = mk(cos(tf), 0.0);
                    cj[C_G] = mk(sin(tf), 0.0);
                    cj[C_J] = mk(0.0, 0.0);
                    cj[C_N] = mk(0.0, 0.0);
                }
                dkd_map<CHX_DKD_DIPOLE, Dual>(cj, v, mc2, steps, out);
                if (inside) {
                    Node node;
                    group_terms(m, out, eta0, beta0, alpha0, s);
                    node_from_sums(s, beta0, rel_beta, node);
                    bend_sums_add(sums, gl8_weight(j), cos_t, sin_t, node);
                }
            }
            if (bends) {
                group_terms(m, out, eta0, beta0, alpha0, s);
                eta_from_sums(s, rel_beta, eta);
                bend_contribution(L, h, cos_t, sin_t, c[C_H], c[C_J], eta_in, eta_bend(eta, cos_t, sin_t), sums, part);
            }
        } else {
            dkd_map_kind<false, Dual>(kind, cd, v, mc2, steps, out);
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] = out[j];
#pragma unroll
        for (int k = 0; k < kIntegrals; ++k) total[k] = total[k] + part[k];
        if (along && stores) {                                // (a store per entry under its lane's mask: no register is indexed by the lane)
#pragma unroll
            for (int k = 0; k < kIntegrals; ++k)
                if (m == k) along[(seed * (int64_t)E + e) * kIntegrals + k] = part[k];
        }
    }
    // a seed whose orbit is NaN or whose image is not finite is NaN in ALL its rows, as in chx_dkd_ring_jacobian (every lane of the
    // group sees the same values; the lane that stored a number along the ring is the one that takes it back)
    const bool lost = ring_lost(v);
    if (stores) {
#pragma unroll
        for (int k = 0; k < kIntegrals; ++k)
            if (m == k) integrals[seed * kIntegrals + k] = lost ? NAN : total[k];
        if (along && lost) {
            for (int e = 0; e < E; ++e) along[(seed * (int64_t)E + e) * kIntegrals + m] = NAN;
        }
    }
}

// ---- the derivative of all that with respect to settings of the ring (chx_dkd_ring_sensitivity) ---------------------------------
// A group of lanes per (seed, knob) pair, eight pairs a wave. The lane carries six Dual2 numbers: e1 = e_m in phase space (lane
// m < 6 of the group), e2 = (w in phase space, the knob's direction in the settings). The items' constants are the values the
// Jacobian kernel reads (wave-uniform scalar loads) with the tangent dkd_ring_sensitivity_prepare_kernel left for the group's
// knob in the e2 part (kSensStride doubles per (knob, item), zeros for the items the knob does not touch); their e1 and mixed
// parts are literal zeros. Pass 1 (w = 0): the e2 parts of the image are d f / d theta, the e1 parts M; lane 0 of the group
// solves (I - M_n) w = (d f / d theta)_n (chx_optics_dev.h). Pass 2 (with w): the e2 parts are d orbit / d theta along the ring,
// the mixed parts column m of d matrix / d theta — the total derivative, the orbit moving with the knob. Mode 0 is pass 1
// alone. Two passes whatever the values, nothing of a pair leaves its wave, no atomics: two calls give the same bits.
constexpr int kSensStride = C_N + 1;
struct RingSensitivityOut {
    double* d_orbit;          // [B][K][6]
    double* d_image;          // [B][K][6]
    double* d_matrix;         // [B][K][6][6]
    double* d_dispersion;     // [B][K][4]
    double* d_orbit_along;    // [B][K][E + 1][6] or null
    double* d_matrix_along;   // [B][K][E + 1][6][6] or null
};

__global__ __launch_bounds__(chx_optics::kLanes) void dkd_ring_sensitivity_kernel(const double* __restrict__ cst, const double* __restrict__ dcst,
                                                                                 int E, double mc2, const double* __restrict__ orbit, int64_t B,
                                                                                 int64_t K, int mode, RingSensitivityOut o) {
    using namespace chx_optics;
    __shared__ double sM[kSeeds][36];
    __shared__ double sA[kSeeds][36];
    __shared__ double sF[kSeeds][6];
    __shared__ double sW[kSeeds][6];
    __shared__ double sD[kSeeds][36];
    const int lane = threadIdx.x, g = group_of_lane(lane), m = tangent_of_lane(lane);
    bool live;
    int64_t seed, knob;
    pair_of_group(blockIdx.x, g, B, K, live, seed, knob);
    const int64_t pair = seed * K + knob;
    const bool column = live && m < 6;                        // the lane stores column m of its pair's matrices
    const int n = closed_count(mode);
    const int passes = mode == 0 ? 1 : 2;
    const double* __restrict__ dc_knob = dcst + knob * (int64_t)E * kSensStride;

    double x[6], w[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        x[j] = orbit[seed * 6 + j];
        w[j] = 0.0;
    }

#pragma unroll 1
    for (int pass = 0; pass < passes; ++pass) {
        const bool last = pass == passes - 1;
        const bool along = last && o.d_matrix_along != nullptr;
        Dual2 v[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] = mk2(x[j], j == m ? 1.0 : 0.0, w[j], 0.0);
        if (along && column) ring_record_store(v, m, pair * (int64_t)(E + 1), o.d_matrix_along, o.d_orbit_along);
#pragma unroll 1
        for (int e = 0; e < E; ++e) {
            int kind, steps;
            Dual2 cd[C_N + 1], out[6];
            ring_item_load<Dual2>(cst + (int64_t)e * kRingCstStride, dc_knob + (int64_t)e * kSensStride, cd, kind, steps);
            dkd_map_kind<true, Dual2>(kind, cd, v, mc2, steps, out);
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = out[j];
            if (along && column) ring_record_store(v, m, pair * (int64_t)(E + 1) + e + 1, o.d_matrix_along, o.d_orbit_along);
        }
        if (!last) {
            // the group's matrix and d f / d theta in LDS: lane m < 6 holds column m, every lane the same e2 parts
            if (m < 6) {
#pragma unroll
                for (int i = 0; i < 6; ++i) sM[g][i * 6 + m] = v[i].a;
            }
            if (m == 0) {
#pragma unroll
                for (int i = 0; i < 6; ++i) sF[g][i] = v[i].b;
            }
            __syncthreads();
            if (m == 0) orbit_sensitivity(n, sM[g], sF[g], sA[g], sW[g]);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 6; ++j) w[j] = sW[g][j];
            continue;
        }
        // a pair whose orbit or image is not finite is NaN in ALL its rows, as its seed is in chx_dkd_ring_jacobian's
        const bool lost = ring_lost(v) || ring_lost(x);
        if (column) {
#pragma unroll
            for (int i = 0; i < 6; ++i) o.d_matrix[pair * 36 + i * 6 + m] = lost ? NAN : v[i].ab;
            double wm = w[0], fm = v[0].b;
#pragma unroll
            for (int j = 1; j < 6; ++j) {
                wm = m == j ? w[j] : wm;
                fm = m == j ? v[j].b : fm;
            }
            o.d_orbit[pair * 6 + m] = lost ? NAN : wm;
            o.d_image[pair * 6 + m] = lost ? NAN : fm;
            // (the rows along the ring were stored during the walk, before `lost` was known, each by the lane that stores it here
            // or by lane 0 of the same wave: stores of one wave to one address retire in program order, so the NaN stays)
            if (lost && along) {
                for (int e = 0; e <= E; ++e) {
                    double* Ma = o.d_matrix_along + (pair * (int64_t)(E + 1) + e) * 36;
#pragma unroll
                    for (int i = 0; i < 6; ++i) Ma[i * 6 + m] = NAN;
                    o.d_orbit_along[(pair * (int64_t)(E + 1) + e) * 6 + m] = NAN;
                }
            }
        }
        // the dispersion's derivative: (I - M_4) eta = M[:4, 5] gives (I - M_4) d eta = d M[:4, 5] + d M_4 eta, by the same solver
        if (m < 6) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                sM[g][i * 6 + m] = v[i].a;
                sD[g][i * 6 + m] = v[i].ab;
            }
        }
        __syncthreads();
        if (live && m == 0) {
            double eta[4], rhs[4];
            dispersion(sM[g], sA[g], eta);
            for (int i = 0; i < 4; ++i) {
                rhs[i] = sD[g][i * 6 + 5];
                for (int k = 0; k < 4; ++k) rhs[i] = rhs[i] + sD[g][i * 6 + k] * eta[k];
            }
            for (int i = 0; i < 4; ++i)
                for (int k = 0; k < 4; ++k) sA[g][i * 6 + k] = (i == k ? 1.0 : 0.0) - sM[g][i * 6 + k];
            solve(4, sA[g], 6, rhs);
            for (int i = 0; i < 4; ++i) o.d_dispersion[pair * 4 + i] = lost ? NAN : rhs[i];
        }
    }
}

template <typename T, int KIND, typename C = double>
int launch_dkd(const void* x_in, const void* params, const void* energy, double mc2, double nq, int num_steps,
               int fringe, int P, int64_t B, int64_t Bx, int64_t Bp, int64_t Be, int64_t N, void* x_out,
               void* energy_out, hipStream_t s) {
    const int64_t tiles = ((N + CHX_BLOCK - 1) / CHX_BLOCK) * B;
    if (tiles > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
    hipLaunchKernelGGL((dkd_kernel<T, KIND, C>), dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s, (const T*)x_in,
                       (const T*)params, (const T*)energy, mc2, nq, num_steps, fringe, P, B, Bx, Bp, Be, N,
                       (T*)x_out, (T*)energy_out, (int)chx_aligned16(x_in), (int)chx_aligned16(x_out));
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

template <typename T, typename C = double>
int dispatch_dkd(int kind, const void* x_in, const void* params, const void* energy, double mc2, double nq,
                 int num_steps, int fringe, int64_t B, int64_t Bx, int64_t Bp, int64_t Be, int64_t N,
                 void* x_out, void* energy_out, hipStream_t s) {
    const int P = dkd_num_params(kind);
    switch (kind) {
        case CHX_DKD_DRIFT:
            return launch_dkd<T, CHX_DKD_DRIFT, C>(x_in, params, energy, mc2, nq, num_steps, fringe, P, B, Bx, Bp, Be,
                                                N, x_out, energy_out, s);
        case CHX_DKD_QUADRUPOLE:
            return launch_dkd<T, CHX_DKD_QUADRUPOLE, C>(x_in, params, energy, mc2, nq, num_steps, fringe, P, B, Bx, Bp,
                                                     Be, N, x_out, energy_out, s);
        case CHX_DKD_DIPOLE:
            return launch_dkd<T, CHX_DKD_DIPOLE, C>(x_in, params, energy, mc2, nq, num_steps, fringe, P, B, Bx, Bp, Be,
                                                 N, x_out, energy_out, s);
        case CHX_DKD_TDC:
            return launch_dkd<T, CHX_DKD_TDC, C>(x_in, params, energy, mc2, nq, num_steps, fringe, P, B, Bx, Bp, Be, N,
                                              x_out, energy_out, s);
        case CHX_DKD_SEXTUPOLE:
            return launch_dkd<T, CHX_DKD_SEXTUPOLE, C>(x_in, params, energy, mc2, nq, num_steps, fringe, P, B, Bx, Bp, Be,
                                                    N, x_out, energy_out, s);
        case CHX_DKD_RFCAVITY:
            return launch_dkd<T, CHX_DKD_RFCAVITY, C>(x_in, params, energy, mc2, nq, num_steps, fringe, P, B, Bx, Bp, Be,
                                                   N, x_out, energy_out, s);
        case CHX_DKD_MULTIPOLE:
            return launch_dkd<T, CHX_DKD_MULTIPOLE, C>(x_in, params, energy, mc2, nq, num_steps, fringe, P, B, Bx, Bp, Be,
                                                    N, x_out, energy_out, s);
    }
    return CHX_ERR_INVALID_ARG;
}

}  // namespace

// The exported query keeps the answers it gave before CHX_DKD_RFCAVITY and CHX_DKD_MULTIPOLE existed (callers of ABI 9 probe the
// kinds with it, and 6 and 8 were "no such kind"); the entry points count the cavity's four parameters and the multipole's six
// through dkd_num_params.
extern "C" int chx_dkd_num_params(int kind) {
    return kind == CHX_DKD_RFCAVITY || kind == CHX_DKD_MULTIPOLE ? -1 : dkd_num_params(kind);
}

extern "C" int chx_dkd_track(int kind, const void* x_in, const void* params, const void* energy, double mass_eV,
                             double n_charges, int32_t num_steps, int32_t fringe_at, int64_t B, int64_t Bx,
                             int64_t Bp, int64_t Be, int64_t N, int dtype, void* x_out, void* energy_out,
                             void* stream) {
    return chx_dkd_track_p(kind, x_in, params, energy, mass_eV, n_charges, num_steps, fringe_at, B, Bx, Bp, Be, N, dtype, 0, x_out,
                           energy_out, stream);
}

extern "C" int chx_dkd_track_p(int kind, const void* x_in, const void* params, const void* energy, double mass_eV,
                               double n_charges, int32_t num_steps, int32_t fringe_at, int64_t B, int64_t Bx, int64_t Bp,
                               int64_t Be, int64_t N, int dtype, int storage_precision, void* x_out, void* energy_out,
                               void* stream) {
    if (dkd_num_params(kind) < 0) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (B < 0 || N < 0) return CHX_ERR_INVALID_ARG;
    if (B == 0 || N == 0) return CHX_OK;
    if (!x_in || !params || !energy || !x_out) return CHX_ERR_INVALID_ARG;
    if (!chx_bcast_ok(Bx, B) || !chx_bcast_ok(Bp, B) || !chx_bcast_ok(Be, B)) return CHX_ERR_INVALID_ARG;
    if ((kind == CHX_DKD_QUADRUPOLE || kind == CHX_DKD_SEXTUPOLE || kind == CHX_DKD_MULTIPOLE) && num_steps < 1) return CHX_ERR_INVALID_ARG;
    if ((kind == CHX_DKD_SEXTUPOLE || kind == CHX_DKD_MULTIPOLE) && num_steps >= (1 << 25)) return CHX_ERR_INVALID_ARG;        // (the chain's and the ring's cap)
    if (fringe_at < 0 || fringe_at > 3) return CHX_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CHX_F32 && storage_precision == 2 &&
        (kind == CHX_DKD_DRIFT || kind == CHX_DKD_QUADRUPOLE || kind == CHX_DKD_SEXTUPOLE || kind == CHX_DKD_MULTIPOLE)) {
        // mixed arithmetic (see dkd_mixed_kernel); the other kinds — Dipole, TDC, RFCavity — keep the fp64 evaluation
        const int64_t tiles = ((N + CHX_BLOCK - 1) / CHX_BLOCK) * B;
        if (tiles > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
        const int P = dkd_num_params(kind);
        if (kind == CHX_DKD_DRIFT)
            hipLaunchKernelGGL(dkd_mixed_kernel<CHX_DKD_DRIFT>, dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s, (const float*)x_in,
                               (const float*)params, (const float*)energy, mass_eV, n_charges, num_steps, P, B, Bx, Bp, Be, N,
                               (float*)x_out, (float*)energy_out, (int)chx_aligned16(x_in), (int)chx_aligned16(x_out));
        else if (kind == CHX_DKD_MULTIPOLE)          // (fringe_at: the order)
            hipLaunchKernelGGL(dkd_mixed_multipole_kernel, dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s, (const float*)x_in,
                               (const float*)params, (const float*)energy, mass_eV, n_charges, num_steps, fringe_at, P, B, Bx, Bp, Be, N,
                               (float*)x_out, (float*)energy_out, (int)chx_aligned16(x_in), (int)chx_aligned16(x_out));
        else if (kind == CHX_DKD_SEXTUPOLE)
            hipLaunchKernelGGL(dkd_mixed_kernel<CHX_DKD_SEXTUPOLE>, dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s, (const float*)x_in,
                               (const float*)params, (const float*)energy, mass_eV, n_charges, num_steps, P, B, Bx, Bp, Be, N,
                               (float*)x_out, (float*)energy_out, (int)chx_aligned16(x_in), (int)chx_aligned16(x_out));
        else
            hipLaunchKernelGGL(dkd_mixed_kernel<CHX_DKD_QUADRUPOLE>, dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s, (const float*)x_in,
                               (const float*)params, (const float*)energy, mass_eV, n_charges, num_steps, P, B, Bx, Bp, Be, N,
                               (float*)x_out, (float*)energy_out, (int)chx_aligned16(x_in), (int)chx_aligned16(x_out));
        CHX_CHECK_LAUNCH();
        return CHX_OK;
    }
    if (dtype == CHX_F32 && storage_precision == 1)
        return dispatch_dkd<float, F32>(kind, x_in, params, energy, mass_eV, n_charges, num_steps, fringe_at, B, Bx, Bp, Be, N, x_out,
                                        energy_out, s);
    return dtype == CHX_F32 ? dispatch_dkd<float>(kind, x_in, params, energy, mass_eV, n_charges, num_steps, fringe_at,
                                                  B, Bx, Bp, Be, N, x_out, energy_out, s)
                            : dispatch_dkd<double>(kind, x_in, params, energy, mass_eV, n_charges, num_steps,
                                                   fringe_at, B, Bx, Bp, Be, N, x_out, energy_out, s);
}

namespace {
constexpr int kDkdSChunk = 64;
struct DkdLengthPtrs {
    const void* p[kDkdSChunk];
};
// s_out = (((s_in + l_0) + l_1) + ...) in T: the additions the reference makes one element at a time (element.py `s=incoming.s +
// self.length`), so that the path length carries the same rounding
template <typename T>
__global__ void dkd_path_length_kernel(DkdLengthPtrs args, int n, const T* __restrict__ s_in, T* __restrict__ s_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    T s = *s_in;
    for (int e = 0; e < n; ++e) s = s + *(const T*)args.p[e];
    *s_out = s;
}

// ---- a RUN of Drifts, Quadrupoles, Dipoles and Sextupoles on one beam, particles kept in registers (chx_dkd_chain) ---------------------
// The per-element kernels above are bound by their arithmetic (a quadrupole in mixed arithmetic: ~450 instructions per particle),
// yet every one of them also moves its 56 bytes per particle through HBM and waits for them at both ends. A run of E elements of
// one arithmetic mode is two launches:
//   dkd_chain_prepare_kernel  a workgroup per element: its reference energy (the float32 round trip of bmadx.py:49 applied once
//                             per element in front of it, as the element-by-element kernels hand it on), dkd_constants in fp64,
//                             the energy it leaves (`energies[e]`);
//   dkd_chain_kernel<MODE>    a particle per lane through all elements; the element's constants are wave-uniform scalar loads;
//                             between two elements the coordinates are rounded to float32 — exactly what the store and the
//                             load of two separate launches do: the same bits as E calls of chx_dkd_track_p.
constexpr int kDkdChainMax = 192;          // elements per launch pair (kernel-argument space: 20 bytes each)
constexpr int kDkdCstStride = 56;          // doubles per element: C_MIXED_N constants — or the 49 entries of a first-order map in the
constexpr int kDkdMeta = 54;               // beam's dtype —, and at kDkdMeta the kind and the step count as two ints
constexpr int kDkdLinear = 4;              // CHX_DKD_LINEAR: a merged run of linear elements between two others
struct DkdChainArgs {
    const void* params[kDkdChainMax];      // (a linear run: its composed map R[7][7])
    const void* length[kDkdChainMax];      // the item's length if it is not the first parameter (a linear run's summed length), else null
    int32_t meta[kDkdChainMax];            // kind | fringe_at << 4 | num_steps << 6
};

template <typename T>
__device__ __forceinline__ T dkd_energy_round_trip(T E, T m) {       // ref_energy of bmadx.py:49, storage dtype
    const T p0 = sqrt(E * E - m * m);
    return sqrt(p0 * p0 + m * m);
}

// the path length behind the run (a workgroup of its own in the kernels that prepare the constants): s = ((s_in + l_0) + l_1) + ...
// in the beam's dtype like the reference's element-by-element additions (every kind's first parameter is its length; s_out may
// be s_in)
template <typename T>
__device__ __forceinline__ void dkd_chain_path_length(const DkdChainArgs& args, int E, const T* s_in, T* s_out) {
    __shared__ T len[kDkdChainMax];
    for (int k = threadIdx.x; k < E; k += blockDim.x) len[k] = args.length[k] ? *(const T*)args.length[k] : ((const T*)args.params[k])[0];
    __syncthreads();
    if (threadIdx.x == 0) {
        T sum = *s_in;
        for (int k = 0; k < E; ++k) sum = sum + len[k];
        *s_out = sum;
    }
}

// what one lane leaves in a drift-kick-drift item's slot of the constants (out[kDkdCstStride]) for the reference energy Ee in
// front of the item: dkd_constants in fp64 whatever the beam's dtype, the extra constants of the mixed evaluation, and at
// kDkdMeta the kind and the step count. ONE definition for the chain (dkd_chain_prepare_kernel) and the ring
// (dkd_turns_constants_kernel): the bits of a turn of the ring are those of a pass of the chain by construction.
template <typename T>
__device__ __forceinline__ void dkd_item_constants(int kind, int fringe, int steps, const T* __restrict__ pe, T Ee, double mc2, double nq,
                                                   double* __restrict__ out) {
    int32_t* w = reinterpret_cast<int32_t*>(out + kDkdMeta);
    w[0] = kind;
    w[1] = steps;
    const int P = dkd_num_params(kind);
    double par[CHX_MAX_PARAMS];
    for (int k = 0; k < P; ++k) par[k] = (double)pe[k];
    double c[C_MIXED_N];
    for (int k = 0; k < C_MIXED_N; ++k) c[k] = 0.0;
    dkd_constants<double>(kind, par, (double)Ee, mc2, nq, fringe, c);
    dkd_mixed_constants(c, mc2);
    for (int k = 0; k < C_MIXED_N; ++k) out[k] = c[k];
}

template <typename T>
__global__ void dkd_chain_prepare_kernel(DkdChainArgs args, int E, const T* __restrict__ energy_in, double mc2, double nq,
                                         double* __restrict__ cst, T* __restrict__ energies, const T* s_in, T* s_out) {
    const int e = blockIdx.x;
    if (e == E) {                                             // one workgroup more: the path length behind the run
        dkd_chain_path_length<T>(args, E, s_in, s_out);
        return;
    }
    const int kind = args.meta[e] & 15, fringe = (args.meta[e] >> 4) & 3, steps = args.meta[e] >> 6;
    double* out = cst + (int64_t)e * kDkdCstStride;
    if (kind == kDkdLinear && threadIdx.x < 49) reinterpret_cast<T*>(out)[threadIdx.x] = ((const T*)args.params[e])[threadIdx.x];
    if (threadIdx.x != 0) return;
    // the reference energy in front of element e: every drift-kick-drift element in front of it leaves the float round trip of
    // what it received (bmadx.py:49); a linear run hands its energy on
    const T m = (T)mc2;
    T Ee = *energy_in;
    for (int k = 0; k < e; ++k) {
        if ((args.meta[k] & 15) == kDkdLinear) continue;
        const T En = dkd_energy_round_trip<T>(Ee, m);
        if (En == Ee) break;              // a fixed point: every later round trip returns it again
        Ee = En;
    }
    if (kind == kDkdLinear) {
        int32_t* w = reinterpret_cast<int32_t*>(out + kDkdMeta);
        w[0] = kind;
        w[1] = steps;
        energies[e] = Ee;
        return;
    }
    dkd_item_constants<T>(kind, fringe, steps, (const T*)args.params[e], Ee, mc2, nq, out);
    energies[e] = dkd_energy_round_trip<T>(Ee, m);
}

struct DkdKindsBlock {
    int32_t k[256];
};
__global__ void dkd_store_kinds_kernel(DkdKindsBlock b, int n, int32_t* __restrict__ out) {
    if ((int)threadIdx.x < n) out[threadIdx.x] = b.k[threadIdx.x];
}

// energies[e] = the reference energy behind item e of such a run, nothing else (chx_dkd_energy_chain: a caller that builds the
// maps of the linear runs in between needs the energy in front of each of them)
template <typename T>
__global__ void dkd_energy_chain_kernel(const int32_t* __restrict__ kinds_dev, int E, const T* __restrict__ energy_in, double mc2,
                                        T* __restrict__ energies) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const T m = (T)mc2;
    T Ee = *energy_in;
    for (int e = 0; e < E; ++e) {
        if (kinds_dev[e] != kDkdLinear) Ee = dkd_energy_round_trip<T>(Ee, m);
        energies[e] = Ee;
    }
}

// MODE: chx_dkd_track_p's storage_precision — 0 fp64 evaluation, 1 float32 evaluation, 2 mixed
template <int MODE, int KIND>
__device__ __forceinline__ void dkd_chain_step(const double* __restrict__ c, double mc2, int num_steps, float (&v)[6]) {
    if (MODE == 2 && KIND != CHX_DKD_DIPOLE && KIND != CHX_DKD_RFCAVITY) {          // (a Dipole or an RFCavity in mixed mode: the fp64 evaluation, as chx_dkd_track_p does)
        dkd_mixed_particle<KIND>(c, mc2, num_steps, v);
    } else if (MODE == 0 || MODE == 2) {
        double in[6], out[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) in[j] = (double)v[j];
        dkd_map<KIND, double>(c, in, mc2, num_steps, out);
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] = (float)out[j];
    } else {
        F32 cf[C_N + 1], in[6], out[6];
#pragma unroll
        for (int k = 0; k <= C_N; ++k) cf[k] = dkd_scalar<F32>::from(c[k]);
#pragma unroll
        for (int j = 0; j < 6; ++j) in[j] = mkf(v[j]);
        dkd_map<KIND, F32>(cf, in, mc2, num_steps, out);
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] = out[j].v;
    }
}

// float64 beams (MODE is not read): the map in fp64 like dkd_kernel<double, ., double>
template <int MODE, int KIND>
__device__ __forceinline__ void dkd_chain_step(const double* __restrict__ c, double mc2, int num_steps, double (&v)[6]) {
    double out[6];
    dkd_map<KIND, double>(c, v, mc2, num_steps, out);
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = out[j];
}

// six coordinates from one register array to another. Which spelling leaves the better register allocation is the compiler's
// whim, not a property of the arithmetic: with hipcc of ROCm 7.2 the fp64 ring keeps 4 waves per SIMD only with the block copy,
// the float32 chain with Dipoles keeps its 8 only with the element copy. Nothing in the build guards this: after a ROCm update,
// regenerate the table of profiles/turn_frame.md and choose again.
template <typename T>
__device__ __forceinline__ void dkd_copy6(const T (&from)[6], T (&to)[6]) {
    if constexpr (sizeof(T) == 8) {
        __builtin_memcpy(to, from, sizeof(to));
    } else {
#pragma unroll
        for (int j = 0; j < 6; ++j) to[j] = from[j];
    }
}

// THE ITEM LOOP of a run of drift-kick-drift items, shared by the chain kernels (LINEAR = true) and the float64 ring (false; the
// float32 ring, dkd_turns_kernel, has the loop written out and says why): the
// items' constants at cst[e][kDkdCstStride] are wave-uniform scalar loads; lane and lane6 hold the lane's particle, six coordinates
// and the seventh column, into which every drift-kick-drift item writes 1.
// BEND: the run contains Dipoles (their body — asin, atan2, a dozen square roots — costs registers the other runs keep)
// SEXT: the run contains Sextupoles (a run without one is the instantiation it was before they existed: the branch is not compiled)
// RF: the run contains RFCavities, likewise; such a run always has BEND = SEXT = true as well (one more kernel per arithmetic
//     mode, not four)
// MP: the run contains Multipoles, likewise; such a run always has BEND = SEXT = RF = true as well (again one more kernel per
//     arithmetic mode)
// LINEAR: items of kind kDkdLinear may stand in the run (a chain; a ring has none, and its code has no such branch)
// A new element kind is one line of the dispatch below.
// The loop runs on a copy of x that is the function's own: a function is optimised before it is inlined into its caller, and
// there the lane's registers are memory behind a reference — a loop over them comes out in another shape than a loop over locals,
// at 3 to 6 VGPRs more per ring kernel and a wave per SIMD fewer in six of them (profiles/turn_frame.md).
template <int MODE, bool BEND, bool SEXT, bool RF, bool MP, bool LINEAR, typename T>
__device__ __forceinline__ void dkd_items(const double* __restrict__ cst, int E, double mc2, T (&lane)[6], T& lane6) {
    T v[6], v6 = lane6;
    dkd_copy6(lane, v);
    for (int e = 0; e < E; ++e) {
        const double* __restrict__ c = cst + (int64_t)e * kDkdCstStride;
        const int32_t* w = reinterpret_cast<const int32_t*>(c + kDkdMeta);
        const int kind = w[0], steps = w[1];
        if (LINEAR && kind == kDkdLinear) {
            // a merged run of linear elements: chx_map7 on all seven coordinates, as chx_apply_affine7 does it (R in the beam's dtype)
            const T in[7] = {v[0], v[1], v[2], v[3], v[4], v[5], v6};
            T y[7];
            chx_map7<T, T>(reinterpret_cast<const T*>(c), in, y);
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = y[j];
            v6 = y[6];
            continue;
        }
        if (kind == CHX_DKD_DRIFT) dkd_chain_step<MODE, CHX_DKD_DRIFT>(c, mc2, steps, v);
        else if (SEXT && kind == CHX_DKD_SEXTUPOLE) dkd_chain_step<MODE, CHX_DKD_SEXTUPOLE>(c, mc2, steps, v);
        else if (RF && kind == CHX_DKD_RFCAVITY) dkd_chain_step<MODE, CHX_DKD_RFCAVITY>(c, mc2, steps, v);
        else if (MP && kind == CHX_DKD_MULTIPOLE) dkd_chain_step<MODE, CHX_DKD_MULTIPOLE>(c, mc2, steps, v);
        else if (!BEND || kind == CHX_DKD_QUADRUPOLE) dkd_chain_step<MODE, CHX_DKD_QUADRUPOLE>(c, mc2, steps, v);
        else dkd_chain_step<MODE, CHX_DKD_DIPOLE>(c, mc2, steps, v);
        v6 = (T)1;
    }
    dkd_copy6(v, lane);
    lane6 = v6;
}

// a particle per lane through all items of the run, MODE / BEND / SEXT / RF / MP as in dkd_items (x_out may be x_in: a tile is read whole
// before it is written)
template <int MODE, bool BEND, bool SEXT, bool RF, bool MP, typename T>
__device__ __forceinline__ void dkd_chain_tile(const T* x_in, const double* __restrict__ cst, int E, double mc2, T* x_out, int64_t N,
                                               int in_vec_ok, int out_vec_ok) {
    constexpr int TP = CHX_BLOCK;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    const int64_t n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    tile_load<T, TP>(x_in + n0 * 7, lds, np * 7, in_vec_ok != 0, true);
    __syncthreads();
    const int p = threadIdx.x;
    T v[6], v6 = p < np ? lds[p * 7 + 6] : (T)1;
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = p < np ? lds[p * 7 + j] : (T)0;
    dkd_items<MODE, BEND, SEXT, RF, MP, true, T>(cst, E, mc2, v, v6);
    if (p < np) {
#pragma unroll
        for (int j = 0; j < 6; ++j) lds[p * 7 + j] = v[j];
        lds[p * 7 + 6] = v6;
    }
    __syncthreads();
    tile_store<T, TP>(x_out + n0 * 7, lds, np * 7, out_vec_ok != 0, true);
}

template <int MODE, bool BEND, bool SEXT, bool RF, bool MP>
__global__ __launch_bounds__(CHX_BLOCK) void dkd_chain_kernel(const float* x_in, const double* __restrict__ cst, int E, double mc2,
                                                              float* x_out, int64_t N, int in_vec_ok, int out_vec_ok) {
    dkd_chain_tile<MODE, BEND, SEXT, RF, MP, float>(x_in, cst, E, mc2, x_out, N, in_vec_ok, out_vec_ok);
}

template <bool BEND, bool SEXT, bool RF, bool MP>
__global__ __launch_bounds__(CHX_BLOCK) void dkd_chain_kernel_f64(const double* x_in, const double* __restrict__ cst, int E, double mc2,
                                                                  double* x_out, int64_t N, int in_vec_ok, int out_vec_ok) {
    dkd_chain_tile<0, BEND, SEXT, RF, MP, double>(x_in, cst, E, mc2, x_out, N, in_vec_ok, out_vec_ok);
}

// ---- the host rules of the entry points over a list of drift-kick-drift items (chx_dkd_chain_mixed, chx_dkd_turns, the three
// chx_dkd_ring_*), each stated once, in front of the first of them (TurnsCall and turns_call_ok stand with the *_turns entry points)
// an item the fused kernels take: one of the six ring kinds, its parameters, a step count that fits the meta word, fringe bits
bool dkd_item_ok(int kind, const void* params, int num_steps, int fringe_at) {
    const bool ring_kind = kind == CHX_DKD_DRIFT || kind == CHX_DKD_QUADRUPOLE || kind == CHX_DKD_DIPOLE || kind == CHX_DKD_SEXTUPOLE ||
                           kind == CHX_DKD_RFCAVITY || kind == CHX_DKD_MULTIPOLE;
    return ring_kind && params && num_steps >= 1 && num_steps < (1 << 25) && fringe_at >= 0 && fringe_at <= 3;
}
// which kinds a run contains: what chooses the compiled variant of its kernel (dkd_items)
struct DkdKinds {
    bool bend = false, sext = false, rf = false, mp = false;
    void add(int kind) {
        bend = bend || kind == CHX_DKD_DIPOLE;
        sext = sext || kind == CHX_DKD_SEXTUPOLE;
        rf = rf || kind == CHX_DKD_RFCAVITY;
        mp = mp || kind == CHX_DKD_MULTIPOLE;
    }
};
// all E items of a ring are good (false: the entry point refuses), and the kinds among them
bool dkd_items_ok(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at, int64_t E, DkdKinds* has = nullptr) {
    for (int64_t e = 0; e < E; ++e) {
        if (!dkd_item_ok(kinds[e], params[e], num_steps[e], fringe_at[e])) return false;
        if (has) has->add(kinds[e]);
    }
    return true;
}
// the compiled variants <BEND, SEXT, RF, MP> of a kernel over dkd_items: launch(BEND, SEXT, RF, MP) is called once, the flags as
// std::bool_constant values. A run with a Multipole has every kind compiled in, a run with a cavity every kind but that.
template <typename Launch>
void dkd_variant(const DkdKinds& k, Launch&& launch) {
    constexpr std::true_type T{};
    constexpr std::false_type F{};
    if (k.mp) launch(T, T, T, T);
    else if (k.rf) launch(T, T, T, F);
    else if (k.bend && k.sext) launch(T, T, F, F);
    else if (k.bend) launch(T, F, F, F);
    else if (k.sext) launch(F, T, F, F);
    else launch(F, F, F, F);
}
// likewise the arithmetic mode of a float32 beam (chx_dkd_track_p's storage_precision): launch(MODE)
template <typename Launch>
void dkd_mode_variant(int mode, Launch&& launch) {
    if (mode == 2) launch(std::integral_constant<int, 2>{});
    else if (mode == 1) launch(std::integral_constant<int, 1>{});
    else launch(std::integral_constant<int, 0>{});
}
// items [done, done + n) of a list as the argument of the kernels that prepare the constants (a linear run: kDkdLinear alone in its
// meta word); the slots behind n are zeroed. lengths may be null: every kind's first parameter is its length.
DkdChainArgs dkd_chain_args(const int32_t* kinds, const void* const* params, const void* const* lengths, const int32_t* num_steps,
                            const int32_t* fringe_at, int64_t done, int n) {
    DkdChainArgs a;
    for (int e = 0; e < kDkdChainMax; ++e) {
        const bool lin = e < n && kinds[done + e] == kDkdLinear;
        a.params[e] = e < n ? params[done + e] : nullptr;
        a.length[e] = e < n && lengths ? lengths[done + e] : nullptr;
        a.meta[e] = e >= n ? 0 : (lin ? kDkdLinear : (kinds[done + e] | (fringe_at[done + e] << 4) | (num_steps[done + e] << 6)));
    }
    return a;
}
// dkd_chain_prepare_kernel in the settings' dtype: `blocks` is n, or n + 1 with the path length (s_in and s_out given)
int dkd_prepare_launch(int dtype, unsigned blocks, const DkdChainArgs& a, int n, const void* energy_in, double mass_eV, double n_charges,
                       void* cst, void* energies, const void* s_in, void* s_out, hipStream_t s) {
    if (dtype == CHX_F32)
        hipLaunchKernelGGL(dkd_chain_prepare_kernel<float>, dim3(blocks), dim3(64), 0, s, a, n, (const float*)energy_in, mass_eV, n_charges,
                           (double*)cst, (float*)energies, (const float*)s_in, (float*)s_out);
    else
        hipLaunchKernelGGL(dkd_chain_prepare_kernel<double>, dim3(blocks), dim3(64), 0, s, a, n, (const double*)energy_in, mass_eV, n_charges,
                           (double*)cst, (double*)energies, (const double*)s_in, (double*)s_out);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}
// the workspace of the three chx_dkd_ring_* entry points, the constants of ONE turn: cst[E][kDkdCstStride] (double) | energies[E]
// (the settings' dtype, room for doubles, rounded up to 16 bytes) as byte offsets, and the size ...
size_t round_up16(size_t n) { return (n + 15) & ~(size_t)15; }
struct DkdRingLayout { size_t cst, energies, total; };
DkdRingLayout dkd_ring_layout(int64_t E) {
    const size_t energies = (size_t)E * kDkdCstStride * sizeof(double);
    return {0, energies, energies + round_up16((size_t)E * sizeof(double))};
}
// ... and its launch (the walk of the reference energy a first turn of chx_dkd_turns makes); cst: where the ring kernels read
int dkd_ring_prepare(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at, int64_t E,
                     int dtype, const void* energy_in, double mass_eV, double n_charges, void* workspace, hipStream_t s, const double*& cst) {
    const DkdRingLayout l = dkd_ring_layout(E);
    cst = (const double*)((const char*)workspace + l.cst);
    return dkd_prepare_launch(dtype, (unsigned)E, dkd_chain_args(kinds, params, nullptr, num_steps, fringe_at, 0, (int)E), (int)E, energy_in,
                              mass_eV, n_charges, (char*)workspace + l.cst, (char*)workspace + l.energies, nullptr, nullptr, s);
}
}  // namespace

// A run of drift-kick-drift elements on ONE beam with scalar settings. float32 Drifts and Quadrupoles of one arithmetic mode: two
// launches, the particles in registers for the whole run (dkd_chain_kernel; x_tmp holds the elements' constants). Otherwise E
// launches of chx_dkd_track_p from one call: the reference energy is handed from element to element on the device (energies[e] =
// what element e leaves), the particle rows ping-pong between x_out and x_tmp so that the last element writes x_out. Either way
// the same results as E separate calls, bit for bit.
extern "C" int chx_dkd_chain(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at,
                             const int32_t* storage_precision, int64_t E, const void* x_in, const void* energy_in, double mass_eV,
                             double n_charges, int64_t N, int dtype, void* x_out, void* x_tmp, void* energies, const void* s_in,
                             void* s_out, void* stream) {
    return chx_dkd_chain_mixed(kinds, params, nullptr, num_steps, fringe_at, storage_precision, E, x_in, energy_in, mass_eV, n_charges, N,
                               dtype, x_out, x_tmp, energies, s_in, s_out, stream);
}

// energies[e] (dtype) = the reference energy behind item e of a run: a drift-kick-drift element leaves the round trip E ->
// sqrt(p0c^2 + m^2) of what it received in dtype (bmadx.py:49), an item of kind CHX_DKD_LINEAR hands its energy on. One launch.
extern "C" int chx_dkd_energy_chain(const int32_t* kinds, int64_t E, const void* energy_in, double mass_eV, int dtype, void* energies,
                                    void* kinds_scratch, void* stream) {
    if (!kinds || E < 1 || E > 65535 || !energy_in || !energies || !kinds_scratch) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    hipStream_t s = (hipStream_t)stream;
    // the kinds travel as kernel arguments in blocks (no host buffer has to outlive the call)
    for (int64_t done = 0; done < E; done += 256) {
        DkdKindsBlock b;
        const int n = (int)std::min<int64_t>(256, E - done);
        for (int e = 0; e < 256; ++e) b.k[e] = e < n ? kinds[done + e] : 0;
        hipLaunchKernelGGL(dkd_store_kinds_kernel, dim3(1), dim3(256), 0, s, b, n, (int32_t*)kinds_scratch + done);
        CHX_CHECK_LAUNCH();
    }
    if (dtype == CHX_F32)
        hipLaunchKernelGGL(dkd_energy_chain_kernel<float>, dim3(1), dim3(1), 0, s, (const int32_t*)kinds_scratch, (int)E,
                           (const float*)energy_in, mass_eV, (float*)energies);
    else
        hipLaunchKernelGGL(dkd_energy_chain_kernel<double>, dim3(1), dim3(1), 0, s, (const int32_t*)kinds_scratch, (int)E,
                           (const double*)energy_in, mass_eV, (double*)energies);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

// The same run with merged runs of linear elements in between: kinds[e] = CHX_DKD_LINEAR marks params[e] as a [7][7] first-order
// map (dtype) applied with the arithmetic of chx_apply_affine7, lengths[e] as the device scalar with that run's summed length
// (lengths may be NULL when no item is linear; an entry of a drift-kick-drift element may be NULL: its first parameter). A lattice
// whose drifts are tracked linearly and whose magnets with the Bmad-X maps is still one pass over the beam.
extern "C" int chx_dkd_chain_mixed(const int32_t* kinds, const void* const* params, const void* const* lengths, const int32_t* num_steps,
                                   const int32_t* fringe_at, const int32_t* storage_precision, int64_t E, const void* x_in,
                                   const void* energy_in, double mass_eV, double n_charges, int64_t N, int dtype, void* x_out,
                                   void* x_tmp, void* energies, const void* s_in, void* s_out, void* stream) {
    if (!kinds || !params || !num_steps || !fringe_at || !storage_precision || E < 1 || E > 65535) return CHX_ERR_INVALID_ARG;
    if ((s_in == nullptr) != (s_out == nullptr)) return CHX_ERR_INVALID_ARG;
    if (!x_in || !energy_in || !x_out || !energies || (E > 1 && !x_tmp) || N < 1) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (x_out == x_in || x_tmp == x_in || x_tmp == x_out) return CHX_ERR_INVALID_ARG;
    const size_t esz = dtype == CHX_F32 ? 4 : 8;
    int64_t first = -1;                               // the first drift-kick-drift element: its arithmetic mode is the run's
    for (int64_t e = 0; e < E; ++e) {
        if (!params[e]) return CHX_ERR_INVALID_ARG;
        if (kinds[e] == kDkdLinear) {
            if (s_out && !(lengths && lengths[e])) return CHX_ERR_INVALID_ARG;
        } else if (first < 0) {
            first = e;
        }
    }
    // Drifts, Quadrupoles, Dipoles, Sextupoles, RFCavities, Multipoles (float32: of one arithmetic mode) and linear runs, the constants (448 bytes per item) in x_tmp:
    // the particles stay in registers (dkd_chain_kernel, dkd_chain_kernel_f64), two launches per 192 items, the same bits
    static const bool fused_off = [] { const char* v = getenv("CHX_DKD_CHAIN_FUSED"); return v && v[0] == '0'; }();
    // (a longer run takes several such pairs, the later ones in place on x_out: a workgroup holds its whole tile in registers
    // before it writes)
    const int64_t per_pass = std::min<int64_t>(kDkdChainMax, N * 7 * (int64_t)esz / (kDkdCstStride * (int64_t)sizeof(double)));
    bool fuse = !fused_off && E >= 2 && per_pass >= 2 && chx_aligned16(x_tmp) && first >= 0;
    DkdKinds has;
    for (int64_t e = 0; fuse && e < E; ++e) {      // (float64 beams ignore storage_precision, like chx_dkd_track_p)
        if (kinds[e] == kDkdLinear) continue;
        fuse = dkd_item_ok(kinds[e], params[e], num_steps[e], fringe_at[e]) &&
               (dtype == CHX_F64 || (storage_precision[e] == storage_precision[first] && storage_precision[e] >= 0 && storage_precision[e] <= 2));
        has.add(kinds[e]);
    }
    if (fuse) {
        hipStream_t s = (hipStream_t)stream;
        const int64_t tiles = (N + CHX_BLOCK - 1) / CHX_BLOCK;
        if (tiles > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
        const int mode = storage_precision[first];
        const dim3 grid((unsigned)tiles), wg(CHX_BLOCK);
        for (int64_t done = 0; done < E; done += per_pass) {
            const int n = (int)std::min<int64_t>(per_pass, E - done);
            const DkdChainArgs a = dkd_chain_args(kinds, params, lengths, num_steps, fringe_at, done, n);
            const void* e_from = done == 0 ? energy_in : (const void*)((const char*)energies + (size_t)(done - 1) * esz);
            void* e_to = (char*)energies + (size_t)done * esz;
            const void* s_from = done == 0 ? s_in : s_out;
            const unsigned blocks = (unsigned)(n + (s_out ? 1 : 0));
            const void* src = done == 0 ? x_in : x_out;
            const int in_ok = (int)chx_aligned16(src), out_ok = (int)chx_aligned16(x_out);
            const int st = dkd_prepare_launch(dtype, blocks, a, n, e_from, mass_eV, n_charges, x_tmp, e_to, s_from, s_out, s);
            if (st != CHX_OK) return st;
            if (dtype == CHX_F64) {
                dkd_variant(has, [&](auto B, auto S, auto R, auto M) {
                    hipLaunchKernelGGL((dkd_chain_kernel_f64<B.value, S.value, R.value, M.value>), grid, wg, 0, s, (const double*)src,
                                       (const double*)x_tmp, n, mass_eV, (double*)x_out, N, in_ok, out_ok);
                });
            } else {
                dkd_mode_variant(mode, [&](auto MODE) {
                    dkd_variant(has, [&](auto B, auto S, auto R, auto M) {
                        hipLaunchKernelGGL((dkd_chain_kernel<MODE.value, B.value, S.value, R.value, M.value>), grid, wg, 0, s, (const float*)src,
                                           (const double*)x_tmp, n, mass_eV, (float*)x_out, N, in_ok, out_ok);
                    });
                });
            }
            CHX_CHECK_LAUNCH();
        }
    } else {
        const void* src = x_in;
        const void* e_src = energy_in;
        for (int64_t e = 0; e < E; ++e) {
            void* dst = ((E - 1 - e) & 1) ? x_tmp : x_out;          // the last element lands in x_out
            void* e_dst = (char*)energies + (size_t)e * esz;
            int st;
            if (kinds[e] == kDkdLinear) {
                st = chx_apply_affine7(src, params[e], dst, 1, 1, 1, N, dtype, stream);
                if (st == CHX_OK && hipMemcpyAsync(e_dst, e_src, esz, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
                    st = CHX_ERR_LAUNCH;
            } else {
                st = chx_dkd_track_p(kinds[e], src, params[e], e_src, mass_eV, n_charges, num_steps[e], fringe_at[e], 1, 1, 1, 1, N, dtype,
                                     storage_precision[e], dst, e_dst, stream);
            }
            if (st != CHX_OK) return st;
            src = dst;
            e_src = e_dst;
        }
    }
    // the path length behind the run: every kind's first parameter is its length (the fused form has it from its first launch)
    for (int64_t done = 0; s_out && !fuse && done < E; done += kDkdSChunk) {
        DkdLengthPtrs a;
        const int n = (int)((E - done < kDkdSChunk) ? (E - done) : kDkdSChunk);
        for (int e = 0; e < kDkdSChunk; ++e)
            a.p[e] = e >= n ? nullptr : ((lengths && lengths[done + e]) ? lengths[done + e] : params[done + e]);
        const void* from = done == 0 ? s_in : s_out;
        if (dtype == CHX_F32)
            hipLaunchKernelGGL(dkd_path_length_kernel<float>, dim3(1), dim3(1), 0, (hipStream_t)stream, a, n, (const float*)from, (float*)s_out);
        else
            hipLaunchKernelGGL(dkd_path_length_kernel<double>, dim3(1), dim3(1), 0, (hipStream_t)stream, a, n, (const double*)from,
                               (double*)s_out);
        CHX_CHECK_LAUNCH();
    }
    return CHX_OK;
}

namespace {
// ---- a RUN of second-order elements on one float32 beam, particles kept in registers (chx_second_order_chain) ---------------
// E launches of second_order_pk_kernel move 56 B per particle and element through HBM for ~50 useful multiply-adds; a run of
// elements needs none of that traffic: Segment.track only hands out the beam behind the run. Two launches for the whole run:
//   so_chain_coeff_kernel  (a workgroup per element) folds T_ijk + T_ikj of every element into its 7 x 28 coefficients, finds
//                          which of them are non-zero and files the element under one of three evaluation schemes;
//   so_chain_kernel        every lane carries two particles through all elements; the coefficients are wave-uniform and come
//                          through scalar loads: no LDS, no barrier inside the loop.
// The schemes differ only in WHICH exact zeros are skipped (a skipped term is 0 * q, an exact no-op on a finite beam), never in
// the order of the remaining multiply-adds: per element the result is second_order_pk_kernel's, value for value.
//   scheme 0: the 27 coefficients an upright Quadrupole can have (a Drift's 15 are among them): 13 products + 27 multiply-adds;
//   scheme 1: the 55 of upright Dipoles (edges, gradient), RBends and Sextupoles: 22 products + 55 multiply-adds;
//   scheme 2: anything else (tilted, misaligned, custom maps): groups of four coefficients, skipped when all four are zero.
constexpr int kSoChainMax = 224;           // elements per launch pair (kernel-argument space: a map and a length pointer each)
constexpr int kSoCoefStride = 256;         // floats per element in the scratch: 196 coefficients, 2 group-mask words, the scheme,
constexpr int kSoPacked = 200;             // one unused; from kSoPacked on the coefficients of the element's pattern, back to back
struct SoChainPtrs {
    const void* T[kSoChainMax];
    const void* length[kSoChainMax];
    unsigned char linear[kSoChainMax];     // 1: T[e] is a 7 x 7 first-order map (a merged run of linear elements between two others)
};
// bit c of row i = coefficient (i, c) of the folded map, c = the pair (j <= k) in the order 00 01 .. 06 11 12 .. 66
struct SoPatternQuad {
    static constexpr unsigned int rows[7] = {0x1860u, 0x1860u, 0x330000u, 0x330000u, 0x7046083u, 0x4000000u, 0x8000000u};
};
struct SoPatternBend {
    static constexpr unsigned int rows[7] = {0x60478e3u, 0x60478e3u, 0x33030cu, 0x33030cu, 0x70478e3u, 0x4000000u, 0x8000000u};
};
constexpr int kSoJ[28] = {0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 6};
constexpr int kSoK[28] = {0, 1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6, 2, 3, 4, 5, 6, 3, 4, 5, 6, 4, 5, 6, 5, 6, 6};

template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void so_chain_coeff_kernel(SoChainPtrs maps, int E, T* __restrict__ coef, const T* s_in, T* s_out) {
    const int e = blockIdx.x;
    if (e == E) {
        // one workgroup more: the path length behind the run, s = ((s_in + l_0) + l_1) + ... in the beam's dtype like the reference's
        // element-by-element additions (s_out may be s_in)
        static_assert(kSoChainMax <= CHX_BLOCK, "one lane per length");
        __shared__ T len[kSoChainMax];
        if (threadIdx.x < E) len[threadIdx.x] = *(const T*)maps.length[threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            T sum = *s_in;
            for (int k = 0; k < E; ++k) sum = sum + len[k];
            *s_out = sum;
        }
        return;
    }
    const T* Tt = (const T*)maps.T[e];
    T* out = coef + (int64_t)e * kSoCoefStride;
    if (maps.linear[e]) {                      // scheme 3: the 49 entries of a first-order map, applied like chx_apply_affine7
        if (threadIdx.x < 49) out[kSoPacked + threadIdx.x] = Tt[threadIdx.x];
        if (threadIdx.x == 0) {
            unsigned int* w = reinterpret_cast<unsigned int*>(out + 196);
            w[0] = 0u; w[1] = 0u; w[2] = 3u; w[3] = 0u;
        }
        return;
    }
    T u = (T)0;
    int i = 0, c = 0;
    if (threadIdx.x < 7 * 28) {
        i = threadIdx.x / 28;
        c = threadIdx.x - i * 28;
        const int j = kSoJ[c], k = kSoK[c];
        const T* Tb = Tt + i * 49;
        u = (j == k) ? Tb[j * 7 + k] : Tb[j * 7 + k] + Tb[k * 7 + j];
        out[threadIdx.x] = u;
    }
    __shared__ unsigned int any4[64];          // group g = coefficients 4g .. 4g + 3
    __shared__ unsigned int outside[2];        // a non-zero coefficient outside pattern 0 / 1
    if (threadIdx.x < 64) any4[threadIdx.x] = 0u;
    if (threadIdx.x < 2) outside[threadIdx.x] = 0u;
    __syncthreads();
    if (threadIdx.x < 7 * 28 && u != (T)0) {
        atomicOr(&any4[threadIdx.x >> 2], 1u);
        if (!((SoPatternQuad::rows[i] >> c) & 1u)) atomicOr(&outside[0], 1u);
        if (!((SoPatternBend::rows[i] >> c) & 1u)) atomicOr(&outside[1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const unsigned long long m = __ballot(threadIdx.x < 49 && any4[threadIdx.x] != 0u);
        if (threadIdx.x == 0) {
            unsigned int* w = reinterpret_cast<unsigned int*>(out + 196);        // three 32-bit words behind the coefficients
            w[0] = (unsigned int)(m & 0xffffffffull);
            w[1] = (unsigned int)(m >> 32);
            w[2] = outside[0] == 0u ? 0u : (outside[1] == 0u ? 1u : 2u);
            w[3] = 0u;
        }
    }
    // the pattern's coefficients back to back (row by row, ascending c): three or four wide scalar loads per element and wave
    // instead of seventeen narrow ones — the scalar memory path of a CU serves its 32 waves one request at a time
    if (threadIdx.x < 7 * 28 && outside[1] == 0u) {
        const unsigned int* rows = outside[0] == 0u ? SoPatternQuad::rows : SoPatternBend::rows;
        if ((rows[i] >> c) & 1u) {
            int n = __popc(rows[i] & ((1u << c) - 1u));
            for (int r = 0; r < i; ++r) n += __popc(rows[r]);
            out[kSoPacked + n] = u;
        }
    }
}

// one element, coefficients of a fixed pattern: every product once, every row its multiply-adds in ascending c
template <class P>
struct SoPatternSize {
    static constexpr int count() {
        int n = 0;
        for (int i = 0; i < 7; ++i)
            for (int c = 0; c < 28; ++c) n += (P::rows[i] >> c) & 1u;
        return n;
    }
};
template <class P>
__device__ __forceinline__ void so_load_pattern(const float* __restrict__ U, float (&u)[SoPatternSize<P>::count()]) {
#pragma unroll
    for (int n = 0; n < SoPatternSize<P>::count(); ++n) u[n] = U[kSoPacked + n];
}
template <class P>
__device__ __forceinline__ void so_eval_pattern(const float (&u)[SoPatternSize<P>::count()], chx_v2f (&x)[7], chx_v2f probe) {
    constexpr unsigned int cols = P::rows[0] | P::rows[1] | P::rows[2] | P::rows[3] | P::rows[4] | P::rows[5] | P::rows[6];
    chx_v2f q[28];
#pragma unroll
    for (int c = 0; c < 28; ++c)
        if ((cols >> c) & 1u) q[c] = x[kSoJ[c]] * x[kSoK[c]];
    chx_v2f y[7];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        chx_v2f acc = probe;
#pragma unroll
        for (int c = 0; c < 28; ++c)
            if ((P::rows[i] >> c) & 1u) {
                const float uu = u[n++];
                acc = __builtin_elementwise_fma(chx_v2f{uu, uu}, q[c], acc);
            }
        y[i] = acc;
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = y[j];
}
template <class P>
__device__ __forceinline__ void so_step_pattern(const float* __restrict__ U, chx_v2f (&x)[7], chx_v2f probe) {
    float u[SoPatternSize<P>::count()];
    so_load_pattern<P>(U, u);
    so_eval_pattern<P>(u, x, probe);
}

// a first-order map between two second-order elements: chx_map7 (R_i0 x_0, then six multiply-adds), both particles of
// the lane at once — the values chx_apply_affine7 writes
__device__ __forceinline__ void so_step_linear(const float* __restrict__ U, chx_v2f (&x)[7]) {
    float r[49];
#pragma unroll
    for (int k = 0; k < 49; ++k) r[k] = U[kSoPacked + k];
    chx_map7_inplace<float, chx_v2f>(r, x);
}

__device__ __forceinline__ void so_step_groups(const float* __restrict__ U, chx_v2f (&x)[7], chx_v2f probe) {
    const unsigned long long g = (unsigned long long)reinterpret_cast<const unsigned int*>(U + 196)[0] |
                                 ((unsigned long long)reinterpret_cast<const unsigned int*>(U + 196)[1] << 32);
    chx_v2f y[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        chx_v2f acc = probe;
        if ((g >> (i * 7)) & 0x7full) {                            // wave-uniform: a row without coefficients is skipped whole
            float u[28];
#pragma unroll
            for (int c = 0; c < 28; ++c) u[c] = U[i * 28 + c];
#pragma unroll
            for (int m = 0; m < 7; ++m) {
                if (!((g >> (i * 7 + m)) & 1ull)) continue;       // wave-uniform
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const int c = 4 * m + q4;
                    const chx_v2f q = x[kSoJ[c]] * x[kSoK[c]];
                    acc = __builtin_elementwise_fma(chx_v2f{u[c], u[c]}, q, acc);
                }
            }
        }
        y[i] = acc;
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = y[j];
}

// ---- the same for float64 beams: one particle per lane, fp64 multiply-adds. second_order_kernel<double> sums a row densely
// (U_i0 q_0, then 27 multiply-adds); leaving out the terms whose coefficient is an exact zero changes no value of a finite beam
// (fma(0, q, acc) = acc), a non-finite coordinate turns the whole particle into NaN there (0 * inf) and here (the probe).
template <class P>
__device__ __forceinline__ void so_step_pattern(const double* __restrict__ U, double (&x)[7], double probe) {
    constexpr unsigned int cols = P::rows[0] | P::rows[1] | P::rows[2] | P::rows[3] | P::rows[4] | P::rows[5] | P::rows[6];
    double q[28];
#pragma unroll
    for (int c = 0; c < 28; ++c)
        if ((cols >> c) & 1u) q[c] = x[kSoJ[c]] * x[kSoK[c]];
    double y[7];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double acc = probe;
#pragma unroll
        for (int c = 0; c < 28; ++c)
            if ((P::rows[i] >> c) & 1u) acc = fma(U[kSoPacked + n++], q[c], acc);
        y[i] = acc;
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = y[j];
}

__device__ __forceinline__ void so_step_groups(const double* __restrict__ U, double (&x)[7], double probe) {
    const unsigned long long g = (unsigned long long)reinterpret_cast<const unsigned int*>(U + 196)[0] |
                                 ((unsigned long long)reinterpret_cast<const unsigned int*>(U + 196)[1] << 32);
    double y[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double acc = probe;
#pragma unroll
        for (int m = 0; m < 7; ++m) {
            if (!((g >> (i * 7 + m)) & 1ull)) continue;           // wave-uniform
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int c = 4 * m + q4;
                acc = fma(U[i * 28 + c], x[kSoJ[c]] * x[kSoK[c]], acc);
            }
        }
        y[i] = acc;
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = y[j];
}

__device__ __forceinline__ void so_step_linear(const double* __restrict__ U, double (&x)[7]) { chx_map7_inplace<double, double>(U + kSoPacked, x); }

// THE ITEM LOOP of a run of second-order items, shared by so_chain_kernel_f64 (X = double, one particle per lane) and the float32
// ring (X = chx_v2f, two particles; so_chain_kernel and so_turns_kernel_f64 have the loop written out and say why). The coefficients at coef[e][kSoCoefStride] are wave-uniform scalar loads, and so
// is the scheme that picks the evaluation. A new scheme is one line of the dispatch below. (The loop runs on a copy of the
// lane's registers that is the function's own: see dkd_items.)
template <typename T, typename X>
__device__ __forceinline__ void so_items(const T* __restrict__ coef, int E, X (&lane)[7]) {
    X x[7];
    __builtin_memcpy(x, lane, sizeof(x));
    for (int e = 0; e < E; ++e) {
        const T* __restrict__ U = coef + (int64_t)e * kSoCoefStride;
        const unsigned int scheme = reinterpret_cast<const unsigned int*>(U + 196)[2];
        // 0 * x is NaN exactly for a non-finite x and +0 otherwise: every row's sum STARTS from this value, so a particle that
        // left the finite range comes out as NaN in all seven coordinates (second_order_pk_kernel's rule) and nothing changes
        // for the others (+0 + a = a)
        X probe = X{};
#pragma unroll
        for (int j = 0; j < 7; ++j) probe = __builtin_elementwise_fma(X{}, x[j], probe);
        if (scheme == 0u) so_step_pattern<SoPatternQuad>(U, x, probe);
        else if (scheme == 1u) so_step_pattern<SoPatternBend>(U, x, probe);
        else if (scheme == 3u) so_step_linear(U, x);
        else so_step_groups(U, x, probe);
    }
    __builtin_memcpy(lane, x, sizeof(x));
}

// the float32 chain: so_items' loop written out in the kernel. At its cap of 64 VGPRs (8 waves per SIMD) the kernel takes no
// other shape without a cost: on so_items it spilled 6 VGPRs (loop on references) or grew by 11 instructions and 1 to 2 % in time
// (loop on a copy; profiles/turn_frame.md). A new scheme in so_items is added here too.
__global__ __launch_bounds__(CHX_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8)))
void so_chain_kernel(const float* x_in, const float* __restrict__ coef, int E, float* x_out, int64_t N, int in_vec_ok,
                     int out_vec_ok) {                  // (x_out may be x_in: a tile is read whole before it is written)
    constexpr int TP = 2 * CHX_BLOCK;
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    const int64_t n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    tile_load<float, TP>(x_in + n0 * 7, lds, np * 7, in_vec_ok != 0, true);
    __syncthreads();
    const int p0 = threadIdx.x, p1 = threadIdx.x + CHX_BLOCK;
    const bool on0 = p0 < np, on1 = p1 < np;
    chx_v2f x[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = chx_v2f{on0 ? lds[p0 * 7 + j] : 0.0f, on1 ? lds[p1 * 7 + j] : 0.0f};
    for (int e = 0; e < E; ++e) {
        const float* __restrict__ U = coef + (int64_t)e * kSoCoefStride;
        const unsigned int scheme = reinterpret_cast<const unsigned int*>(U + 196)[2];
        // 0 * x is NaN exactly for a non-finite x and +0 otherwise: every row's sum STARTS from this value, so a particle that
        // left the finite range comes out as NaN in all seven coordinates (second_order_pk_kernel's rule) and nothing changes
        // for the others (+0 + a = a)
        chx_v2f probe = chx_v2f{0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 7; ++j) probe = __builtin_elementwise_fma(chx_v2f{0.0f, 0.0f}, x[j], probe);
        if (scheme == 0u) so_step_pattern<SoPatternQuad>(U, x, probe);
        else if (scheme == 1u) so_step_pattern<SoPatternBend>(U, x, probe);
        else if (scheme == 3u) so_step_linear(U, x);
        else so_step_groups(U, x, probe);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        if (on0) lds[p0 * 7 + j] = x[j].x;
        if (on1) lds[p1 * 7 + j] = x[j].y;
    }
    __syncthreads();
    tile_store<float, TP>(x_out + n0 * 7, lds, np * 7, out_vec_ok != 0, true);
}

__global__ __launch_bounds__(CHX_BLOCK) void so_chain_kernel_f64(const double* x_in, const double* __restrict__ coef, int E, double* x_out,
                                                                 int64_t N, int in_vec_ok, int out_vec_ok) {
    constexpr int TP = CHX_BLOCK;              // (x_out may be x_in: a tile is read whole before it is written)
    __shared__ __attribute__((aligned(16))) double lds[TP * 7];
    const int64_t n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
    tile_load<double, TP>(x_in + n0 * 7, lds, np * 7, in_vec_ok != 0, true);
    __syncthreads();
    const int p = threadIdx.x;
    double x[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = p < np ? lds[p * 7 + j] : 0.0;
    so_items<double, double>(coef, E, x);
    if (p < np) {
#pragma unroll
        for (int j = 0; j < 7; ++j) lds[p * 7 + j] = x[j];
    }
    __syncthreads();
    tile_store<double, TP>(x_out + n0 * 7, lds, np * 7, out_vec_ok != 0, true);
}

// ---- the same chain TURN AFTER TURN (chx_second_order_turns): for turn { for item { ... } } over the one coefficient block, the
// particles in registers for a whole chunk of turns [first_turn, first_turn + num_turns). A ring at 1e3 - 1e4 particles is
// launch-bound turn by turn (two launches and a round trip of the beam per turn); here a turn costs its multiply-adds.
//   alive    lost[h] of a lane's particle h: 0 = alive, else the 1-based turn of loss (seeded from lost_turn[N], written back). At
//            the end of a turn a live particle is lost when one of its six coordinates is non-finite or |x| > a_x or |y| > a_y
//            (aperture[2], read through its address). Its coordinates of that moment go to the particle's row of the LDS tile
//            and stand there until the tile is stored: a lane cannot skip a step its other particle (or its neighbours) take,
//            so the registers of a lost particle go on being stepped, but nothing reads them again — the record and the probe
//            SELECT on the flag (no 0 * NaN anywhere), the final write-back leaves the row alone. A wave without a live
//            particle skips the item loop (wave-uniform branch).
//   records  on turn t = next_record, next_record + record_every, ...: the 14 float64 sums (count, sum w, sum w x_j, sum w x_j^2,
//            j < 6; w = (double)charge * (double)survival or 1) over the workgroup's live particles, formed one after the other —
//            a wave sum each, no accumulator lives across the item loop — and written to partials[record][tile][14]; the first
//            K rows of the beam to probe[record][K][7] (a lost row: its frozen values). so_turns_reduce_kernel adds the tiles
//            in a fixed order: no float atomics, bitwise reproducible.
constexpr int kSoTurnSums = 14;
template <typename T>
struct SoTurnsArgs {
    const T* x_in;                     // may be x_out (a tile is read whole before it is written)
    T* x_out;
    const T* charges;                  // [N] or NULL
    const T* survival;                 // [N] or NULL
    const T* aperture;                 // [2] or NULL
    int32_t* lost_turn;                // [N], in / out
    double* partials;                  // [records of this launch][tiles][14]
    T* probe;                          // [records][K][7], the row of this launch's first record
    int64_t N, K, next_record, record_every;
    int E, first_turn, num_turns, in_vec_ok, out_vec_ok;
};

// the 14 sums of one recorded turn over the workgroup: PP particles per lane, x as doubles
template <int PP>
__device__ __forceinline__ void so_turn_record(const double (&w)[PP], const double (&xd)[PP][6], const bool (&live)[PP],
                                               double* red /* [4][14] */, double* __restrict__ out /* [14] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kSoTurnSums; ++k) {
        double v = 0.0;
#pragma unroll
        for (int h = 0; h < PP; ++h) {
            double t;
            if (k == 0) t = 1.0;
            else if (k == 1) t = w[h];
            else if (k < 8) t = w[h] * xd[h][k - 2];
            else t = (w[h] * xd[h][k - 8]) * xd[h][k - 8];
            v += live[h] ? t : 0.0;                                // a select: a lost particle's NaN never meets a 0
        }
        v = chx_wave_sum(v);
        if (lane == 0) red[wave * kSoTurnSums + k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kSoTurnSums) {
        const int k = threadIdx.x;
        out[k] = ((red[k] + red[kSoTurnSums + k]) + red[2 * kSoTurnSums + k]) + red[3 * kSoTurnSums + k];
    }
    __syncthreads();                                               // red is free for the next recorded turn
}

template <typename T>
__device__ __forceinline__ bool so_turn_outside(const T (&c)[6], T ax, T ay) {      // (no aperture: ax = ay = +inf, never exceeded)
    int bad = 0;                                                   // straight-line: every test is evaluated, none branches
#pragma unroll
    for (int j = 0; j < 6; ++j) bad |= (int)!__builtin_isfinite(c[j]);
    bad |= (int)(__builtin_elementwise_abs(c[0]) > ax) | (int)(__builtin_elementwise_abs(c[2]) > ay);
    return bad != 0;
}

// THE TURN FRAME of the ring kernels (so_turns_kernel and dkd_turns_kernel_f64 run on it; so_turns_kernel_f64 and dkd_turns_kernel
// hold the same text written out and say why): the tile load, the loss flags, the aperture, the turn loop with its wave-uniform skip,
// the loss test and the freezing of a lost row in LDS, the record and the probe rows, the write-back — the rules above, once,
// for PP particles per lane. What a lane holds and what a turn does to it is the Ring's business:
//   ring.load(lds, p, on)   the lane's rows p[h] of the LDS tile into its registers (on[h] false: a lane past the end of the beam)
//   ring.get(h, j)          coordinate j < 7 of the lane's particle h
//   ring.turn(k)            turn k of the call (0-based) on the registers
// ring and a are taken by reference: the frame is inlined into its kernel, and the kernel's own arguments stay what the
// compiler sees (see so_turns_kernel for why that matters).
template <typename T, int PP, class Ring>
__device__ __forceinline__ void turns_frame(Ring& ring, const SoTurnsArgs<T>& a) {
    constexpr int TP = PP * CHX_BLOCK;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    __shared__ double red[4 * kSoTurnSums];
    const int64_t n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((a.N - n0 < TP) ? (a.N - n0) : TP);
    tile_load<T, TP>(a.x_in + n0 * 7, lds, np * 7, a.in_vec_ok != 0, true);
    __syncthreads();
    int p[PP], lost[PP];
    bool on[PP];
#pragma unroll
    for (int h = 0; h < PP; ++h) {
        p[h] = (int)threadIdx.x + h * CHX_BLOCK;
        on[h] = p[h] < np;
    }
    ring.load(lds, p, on);
#pragma unroll
    for (int h = 0; h < PP; ++h) lost[h] = on[h] ? a.lost_turn[n0 + p[h]] : -1;      // (a lane past the end of the beam: never alive)
    T ax = (T)__builtin_inf(), ay = (T)__builtin_inf();
    if (a.aperture) { ax = a.aperture[0]; ay = a.aperture[1]; }
    int64_t next_record = a.next_record;
    int rec = 0;
    const int end_turn = a.first_turn + a.num_turns;
    for (int t = a.first_turn; t < end_turn; ++t) {
        bool alive = false;
#pragma unroll
        for (int h = 0; h < PP; ++h) alive = alive || lost[h] == 0;
        if (__any(alive)) {
            ring.turn(t - a.first_turn);
#pragma unroll
            for (int h = 0; h < PP; ++h) {
                T c[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) c[j] = ring.get(h, j);
                if (so_turn_outside<T>(c, ax, ay) && lost[h] == 0) {
                    lost[h] = t;
#pragma unroll
                    for (int j = 0; j < 7; ++j) lds[p[h] * 7 + j] = ring.get(h, j);              // frozen here
                }
            }
        }
        if (t == next_record) {
            double w[PP], xd[PP][6];
            bool live[PP];
#pragma unroll
            for (int h = 0; h < PP; ++h) {
                live[h] = lost[h] == 0;
                const int64_t n = n0 + p[h];
                w[h] = 1.0;
                if (on[h] && a.charges) w[h] = (double)a.charges[n];
                if (on[h] && a.survival) w[h] = w[h] * (double)a.survival[n];
#pragma unroll
                for (int j = 0; j < 6; ++j) xd[h][j] = (double)ring.get(h, j);
                if (n < a.K) {
                    T* dst = a.probe + ((int64_t)rec * a.K + n) * 7;
#pragma unroll
                    for (int j = 0; j < 7; ++j) dst[j] = live[h] ? ring.get(h, j) : lds[p[h] * 7 + j];
                }
            }
            so_turn_record<PP>(w, xd, live, red, a.partials + ((int64_t)rec * gridDim.x + blockIdx.x) * kSoTurnSums);
            next_record += a.record_every;
            ++rec;
        }
    }
#pragma unroll
    for (int h = 0; h < PP; ++h) {
        if (lost[h] == 0) {
#pragma unroll
            for (int j = 0; j < 7; ++j) lds[p[h] * 7 + j] = ring.get(h, j);
        }
        if (on[h]) a.lost_turn[n0 + p[h]] = lost[h];
    }
    __syncthreads();
    tile_store<T, TP>(a.x_out + n0 * 7, lds, np * 7, a.out_vec_ok != 0, true);
}

// the float32 second-order ring: two particles per lane, rows p and p + CHX_BLOCK of a tile of 2 * CHX_BLOCK; a turn is so_items
// over the one coefficient block
struct SoRing {
    const float* __restrict__ coef;
    int E;
    chx_v2f x[7];
    __device__ __forceinline__ void load(const float* lds, const int (&p)[2], const bool (&on)[2]) {
#pragma unroll
        for (int j = 0; j < 7; ++j) x[j] = chx_v2f{on[0] ? lds[p[0] * 7 + j] : 0.0f, on[1] ? lds[p[1] * 7 + j] : 0.0f};
    }
    __device__ __forceinline__ float get(int h, int j) const { return h == 0 ? x[j].x : x[j].y; }
    __device__ __forceinline__ void turn(int) { so_items<float, chx_v2f>(coef, E, x); }
};

// (coef is a kernel argument of its own, __restrict__: only then does the compiler know that the stores of the records cannot
// touch the coefficients and fetch them through scalar loads as so_chain_kernel does — inside the argument block they came
// through 130 vector loads per item loop, and the kernel took 1.7 us per item step at 1e6 particles instead of the chain's 1.3)
__global__ __launch_bounds__(CHX_BLOCK) void so_turns_kernel(const float* __restrict__ coef, SoTurnsArgs<float> a) {
    SoRing ring{coef, a.E};
    turns_frame<float, 2>(ring, a);
}

// float64 beams: the frame's text written out, with the item loop in the kernel. On turns_frame this kernel kept its registers and
// its waves per SIMD, but its item loop compiled to twelve more v_mul_f64 and it ran 1.3 to 1.8 % slower at 1e5 and 1e6 particles
// (profiles/turn_frame.md). A change to the loss, record or probe rules of turns_frame is made here too.
__global__ __launch_bounds__(CHX_BLOCK) void so_turns_kernel_f64(const double* __restrict__ coef, SoTurnsArgs<double> a) {
    constexpr int TP = CHX_BLOCK;
    __shared__ __attribute__((aligned(16))) double lds[TP * 7];
    __shared__ double red[4 * kSoTurnSums];
    const int64_t n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((a.N - n0 < TP) ? (a.N - n0) : TP);
    tile_load<double, TP>(a.x_in + n0 * 7, lds, np * 7, a.in_vec_ok != 0, true);
    __syncthreads();
    const int p = threadIdx.x;
    const bool on = p < np;
    double x[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = on ? lds[p * 7 + j] : 0.0;
    int lost = on ? a.lost_turn[n0 + p] : -1;
    double ax = __builtin_inf(), ay = __builtin_inf();
    if (a.aperture) { ax = a.aperture[0]; ay = a.aperture[1]; }
    int64_t next_record = a.next_record;
    int rec = 0;
    const int end_turn = a.first_turn + a.num_turns;
    for (int t = a.first_turn; t < end_turn; ++t) {
        if (__any(lost == 0)) {
            for (int e = 0; e < a.E; ++e) {
                const double* __restrict__ U = coef + (int64_t)e * kSoCoefStride;
                const unsigned int scheme = reinterpret_cast<const unsigned int*>(U + 196)[2];
                double probe = 0.0;
#pragma unroll
                for (int j = 0; j < 7; ++j) probe = fma(0.0, x[j], probe);
                if (scheme == 0u) so_step_pattern<SoPatternQuad>(U, x, probe);
                else if (scheme == 1u) so_step_pattern<SoPatternBend>(U, x, probe);
                else if (scheme == 3u) so_step_linear(U, x);
                else so_step_groups(U, x, probe);
            }
            double c[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) c[j] = x[j];
            if (so_turn_outside<double>(c, ax, ay) && lost == 0) {
                lost = t;
#pragma unroll
                for (int j = 0; j < 7; ++j) lds[p * 7 + j] = x[j];                                  // frozen here
            }
        }
        if (t == next_record) {
            double w[1], xd[1][6];
            const bool live[1] = {lost == 0};
            const int64_t n = n0 + p;
            w[0] = 1.0;
            if (on && a.charges) w[0] = a.charges[n];
            if (on && a.survival) w[0] = w[0] * a.survival[n];
#pragma unroll
            for (int j = 0; j < 6; ++j) xd[0][j] = x[j];
            if (n < a.K) {
                double* dst = a.probe + ((int64_t)rec * a.K + n) * 7;
#pragma unroll
                for (int j = 0; j < 7; ++j) dst[j] = live[0] ? x[j] : lds[p * 7 + j];
            }
            so_turn_record<1>(w, xd, live, red, a.partials + ((int64_t)rec * gridDim.x + blockIdx.x) * kSoTurnSums);
            next_record += a.record_every;
            ++rec;
        }
    }
    if (lost == 0) {
#pragma unroll
        for (int j = 0; j < 7; ++j) lds[p * 7 + j] = x[j];
    }
    if (on) a.lost_turn[n0 + p] = lost;
    __syncthreads();
    tile_store<double, TP>(a.x_out + n0 * 7, lds, np * 7, a.out_vec_ok != 0, true);
}

// sums[record][14] = the tiles of partials[record][tiles][14] added in a fixed order: 16 strided slices of tiles, then the slices
__global__ __launch_bounds__(CHX_BLOCK) void so_turns_reduce_kernel(const double* __restrict__ partials, int64_t tiles,
                                                                    double* __restrict__ sums) {
    constexpr int SLICES = 16;
    static_assert(SLICES * kSoTurnSums <= CHX_BLOCK, "a lane per (slice, sum)");
    __shared__ double part[SLICES * kSoTurnSums];
    const double* __restrict__ src = partials + (int64_t)blockIdx.x * tiles * kSoTurnSums;
    if (threadIdx.x < SLICES * kSoTurnSums) {
        const int s = threadIdx.x / kSoTurnSums, k = threadIdx.x - s * kSoTurnSums;
        double acc = 0.0;
        for (int64_t t = s; t < tiles; t += SLICES) acc += src[t * kSoTurnSums + k];
        part[threadIdx.x] = acc;
    }
    __syncthreads();
    if (threadIdx.x < kSoTurnSums) {
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < SLICES; ++s) acc += part[s * kSoTurnSums + threadIdx.x];
        sums[(int64_t)blockIdx.x * kSoTurnSums + threadIdx.x] = acc;
    }
}

// ---- a ring of Drifts, Quadrupoles, Dipoles, Sextupoles, RFCavities and Multipoles tracked drift-kick-drift, TURN AFTER TURN (chx_dkd_turns) --
// dkd_chain_kernel with the item loop inside the turn loop of so_turns_kernel. What the second-order ring does not have: every
// drift-kick-drift element leaves the reference energy as the round trip f(E) = sqrt(sqrt(E^2 - m^2)^2 + m^2) of what it received
// (dkd_energy_round_trip), and an element's constants depend on the energy in front of it. f is a composition of monotone,
// correctly rounded operations, so E, f(E), f(f(E)), ... is monotone and ends in a fixed point — but not quickly for every E:
// beside a power of two it can move one ulp per element for thousands of elements. So no turn is ASSUMED to repeat the one before
// it. The constants of turn t are those of turn t - 1 exactly when both turns start with the same energy bits (then every later
// turn does too), and that is what the kernels test:
//   dkd_turns_energy_kernel     one lane walks the turns of the call from energy_in: start[t] = the energy in front of turn t,
//                               block_of_turn[t] = the block of constants turn t reads. A turn whose start energy has the bits of
//                               the turn before shares its block, and so do all turns behind it; any other turn opens a block.
//                               Blocks are opened one per turn from the first turn on, so block k belongs to turn k of the call.
//                               block_of_turn[turns] = the number of blocks; energy_out = the energy behind the last turn.
//   dkd_turns_constants_kernel  a workgroup per (block, item); those of blocks that were not opened return at once. The others
//                               walk from their block's start energy to the energy in front of their item and leave the item's
//                               constants (dkd_item_constants, the chain's own). One workgroup more adds up the path length.
//   dkd_turns_kernel<MODE, BEND, SEXT, RF, MP>, dkd_turns_kernel_f64<BEND, SEXT, RF, MP>   a particle per lane; per turn the block's address (a scalar load),
//                               the chain's item loop (dkd_items); the loss test, the freezing of a lost row in the LDS tile,
//                               the record and the probe rows are turns_frame's.
//   so_turns_reduce_kernel      as it is.
template <typename T>
__device__ __forceinline__ bool dkd_same_bits(T a, T b) {
    if constexpr (sizeof(T) == 4) return __float_as_uint(a) == __float_as_uint(b);
    else return __double_as_longlong(a) == __double_as_longlong(b);
}

// the reference energy behind `count` drift-kick-drift items that received Ee
template <typename T>
__device__ __forceinline__ T dkd_energy_behind(T Ee, T m, int count) {
    for (int k = 0; k < count; ++k) {
        const T En = dkd_energy_round_trip<T>(Ee, m);
        if (dkd_same_bits<T>(En, Ee)) break;                  // a fixed point: every later round trip returns it again
        Ee = En;
    }
    return Ee;
}

template <typename T>
__global__ void dkd_turns_energy_kernel(int E, int turns, const T* energy_in, T* energy_out, double mc2, T* __restrict__ start,
                                        int32_t* __restrict__ block_of_turn) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const T m = (T)mc2;
    T Et = *energy_in;                                        // (energy_out may be energy_in: read before anything is written)
    int block = 0, t = 0;
    for (; t < turns; ++t) {
        if (t > 0 && dkd_same_bits<T>(Et, start[t - 1])) break;                  // this turn repeats the last one, and so does every later one
        start[t] = Et;
        block_of_turn[t] = block++;
        Et = dkd_energy_behind<T>(Et, m, E);
    }
    for (; t < turns; ++t) {
        start[t] = Et;
        block_of_turn[t] = block - 1;
    }
    block_of_turn[turns] = block;
    *energy_out = Et;
}

template <typename T>
__global__ void dkd_turns_constants_kernel(DkdChainArgs args, int E, int turns, const T* __restrict__ start,
                                           const int32_t* __restrict__ block_of_turn, double mc2, double nq, double* __restrict__ cst,
                                           const T* s_in, T* s_out) {
    if ((int)blockIdx.x == turns * E) {                       // one workgroup more: the path length after ONE turn
        dkd_chain_path_length<T>(args, E, s_in, s_out);
        return;
    }
    const int block = blockIdx.x / E, e = blockIdx.x - block * E;
    if (block >= block_of_turn[turns] || threadIdx.x != 0) return;
    const int kind = args.meta[e] & 15, fringe = (args.meta[e] >> 4) & 3, steps = args.meta[e] >> 6;
    const T Ee = dkd_energy_behind<T>(start[block], (T)mc2, e);                  // (block k is turn k's: see above)
    dkd_item_constants<T>(kind, fringe, steps, (const T*)args.params[e], Ee, mc2, nq, cst + ((int64_t)block * E + e) * kDkdCstStride);
}

// the drift-kick-drift ring (as built: float64 beams, MODE is not read): a particle per lane; a turn is dkd_items over the block of
// constants of that turn (its address: a scalar load), which leaves 1 in the seventh column as every drift-kick-drift kernel does.
// MODE, BEND, SEXT, RF, MP as in dkd_items
template <int MODE, bool BEND, bool SEXT, bool RF, bool MP, typename T>
struct DkdRing {
    const double* __restrict__ cst;
    const int32_t* __restrict__ block_of_turn;
    int E;
    double mc2;
    T v[6], v6;                        // (six coordinates and the seventh column, kept apart as in dkd_items)
    __device__ __forceinline__ void load(const T* lds, const int (&p)[1], const bool (&on)[1]) {
        v6 = on[0] ? lds[p[0] * 7 + 6] : (T)1;
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] = on[0] ? lds[p[0] * 7 + j] : (T)0;
    }
    __device__ __forceinline__ T get(int, int j) const { return j < 6 ? v[j] : v6; }
    __device__ __forceinline__ void turn(int k) {
        dkd_items<MODE, BEND, SEXT, RF, MP, false, T>(cst + (int64_t)block_of_turn[k] * E * kDkdCstStride, E, mc2, v, v6);
    }
};

// (cst and block_of_turn are kernel arguments of their own, __restrict__: see so_turns_kernel — the stores of the records must not
// be taken for stores into the constants, or these stop coming through scalar loads)
// float32 beams: the frame's text and the item loop written out. On turns_frame with dkd_items every instantiation kept its waves
// per SIMD, but the "storage" ring ran 1.7 to 2.4 % slower at 1e3 and 1e5 particles and the "mixed" and "double" rings 0.8 to 1.4 %
// (profiles/turn_frame.md). A change to the rules of turns_frame or a new kind in dkd_items is made here too.
template <int MODE, bool BEND, bool SEXT, bool RF, bool MP>
__global__ __launch_bounds__(CHX_BLOCK) void dkd_turns_kernel(const double* __restrict__ cst, const int32_t* __restrict__ block_of_turn,
                                                              double mc2, SoTurnsArgs<float> a) {
    constexpr int TP = CHX_BLOCK;
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    __shared__ double red[4 * kSoTurnSums];
    const int64_t n0 = (int64_t)blockIdx.x * TP;
    const int np = (int)((a.N - n0 < TP) ? (a.N - n0) : TP);
    tile_load<float, TP>(a.x_in + n0 * 7, lds, np * 7, a.in_vec_ok != 0, true);
    __syncthreads();
    const int p = threadIdx.x;
    const bool on = p < np;
    float v[6], v6 = on ? lds[p * 7 + 6] : 1.0f;
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = on ? lds[p * 7 + j] : 0.0f;
    int lost = on ? a.lost_turn[n0 + p] : -1;                  // (a lane past the end of the beam: never alive)
    float ax = __builtin_inff(), ay = __builtin_inff();
    if (a.aperture) { ax = a.aperture[0]; ay = a.aperture[1]; }
    int64_t next_record = a.next_record;
    int rec = 0;
    const int end_turn = a.first_turn + a.num_turns;
    for (int t = a.first_turn; t < end_turn; ++t) {
        if (__any(lost == 0)) {
            const double* __restrict__ turn_cst = cst + (int64_t)block_of_turn[t - a.first_turn] * a.E * kDkdCstStride;
            for (int e = 0; e < a.E; ++e) {
                const double* __restrict__ c = turn_cst + (int64_t)e * kDkdCstStride;
                const int32_t* w = reinterpret_cast<const int32_t*>(c + kDkdMeta);
                const int kind = w[0], steps = w[1];
                if (kind == CHX_DKD_DRIFT) dkd_chain_step<MODE, CHX_DKD_DRIFT>(c, mc2, steps, v);
                else if (SEXT && kind == CHX_DKD_SEXTUPOLE) dkd_chain_step<MODE, CHX_DKD_SEXTUPOLE>(c, mc2, steps, v);
                else if (RF && kind == CHX_DKD_RFCAVITY) dkd_chain_step<MODE, CHX_DKD_RFCAVITY>(c, mc2, steps, v);
                else if (MP && kind == CHX_DKD_MULTIPOLE) dkd_chain_step<MODE, CHX_DKD_MULTIPOLE>(c, mc2, steps, v);
                else if (!BEND || kind == CHX_DKD_QUADRUPOLE) dkd_chain_step<MODE, CHX_DKD_QUADRUPOLE>(c, mc2, steps, v);
                else dkd_chain_step<MODE, CHX_DKD_DIPOLE>(c, mc2, steps, v);
            }
            v6 = 1.0f;                                         // (the drift-kick-drift kernels write 1 into the seventh column)
            if (so_turn_outside<float>(v, ax, ay) && lost == 0) {
                lost = t;
#pragma unroll
                for (int j = 0; j < 6; ++j) lds[p * 7 + j] = v[j];                                  // frozen here
                lds[p * 7 + 6] = v6;
            }
        }
        if (t == next_record) {
            double w[1], xd[1][6];
            const bool live[1] = {lost == 0};
            const int64_t n = n0 + p;
            w[0] = 1.0;
            if (on && a.charges) w[0] = (double)a.charges[n];
            if (on && a.survival) w[0] = w[0] * (double)a.survival[n];
#pragma unroll
            for (int j = 0; j < 6; ++j) xd[0][j] = (double)v[j];
            if (n < a.K) {
                float* dst = a.probe + ((int64_t)rec * a.K + n) * 7;
#pragma unroll
                for (int j = 0; j < 6; ++j) dst[j] = live[0] ? v[j] : lds[p * 7 + j];
                dst[6] = live[0] ? v6 : lds[p * 7 + 6];
            }
            so_turn_record<1>(w, xd, live, red, a.partials + ((int64_t)rec * gridDim.x + blockIdx.x) * kSoTurnSums);
            next_record += a.record_every;
            ++rec;
        }
    }
    if (lost == 0) {
#pragma unroll
        for (int j = 0; j < 6; ++j) lds[p * 7 + j] = v[j];
        lds[p * 7 + 6] = v6;
    }
    if (on) a.lost_turn[n0 + p] = lost;
    __syncthreads();
    tile_store<float, TP>(a.x_out + n0 * 7, lds, np * 7, a.out_vec_ok != 0, true);
}

// float64 beams: turns_frame with the DkdRing policy
template <bool BEND, bool SEXT, bool RF, bool MP>
__global__ __launch_bounds__(CHX_BLOCK) void dkd_turns_kernel_f64(const double* __restrict__ cst, const int32_t* __restrict__ block_of_turn,
                                                                  double mc2, SoTurnsArgs<double> a) {
    DkdRing<0, BEND, SEXT, RF, MP, double> ring{cst, block_of_turn, a.E, mc2};
    turns_frame<double, 1>(ring, a);
}

}  // namespace

// A run of elements tracked with their second-order maps (element.py:195-228) on ONE beam. float32: the particles stay in
// registers for the whole run (so_chain_kernel, two launches; x_tmp holds the folded coefficients). Otherwise E launches of
// chx_apply_second_order, rows ping-ponging between x_out and x_tmp so that the last element writes x_out; the path length like
// chx_dkd_chain (lengths[E]: device pointers to the elements' length scalars). Same results as E separate calls, bit for bit.
extern "C" int chx_second_order_chain(const void* const* T_maps, const void* const* lengths, int64_t E, const void* x_in, int64_t N,
                                      int dtype, void* x_out, void* x_tmp, const void* s_in, void* s_out, void* stream) {
    return chx_second_order_chain_mixed(T_maps, nullptr, lengths, E, x_in, N, dtype, x_out, x_tmp, s_in, s_out, stream);
}

// The same run with first-order maps in between: linear[e] != 0 marks T_maps[e] as a [7][7] map (a merged run of linear elements
// that stands between second-order elements, applied like chx_apply_affine7) — a lattice whose drifts are tracked linearly and
// whose magnets to second order is still ONE pass over the beam.
extern "C" int chx_second_order_chain_mixed(const void* const* T_maps, const int32_t* linear, const void* const* lengths, int64_t E,
                                            const void* x_in, int64_t N, int dtype, void* x_out, void* x_tmp, const void* s_in,
                                            void* s_out, void* stream) {
    if (!T_maps || E < 1 || E > 65535 || !x_in || !x_out || (E > 1 && !x_tmp) || N < 1) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if ((s_in == nullptr) != (s_out == nullptr) || (s_out && !lengths)) return CHX_ERR_INVALID_ARG;
    if (x_out == x_in || x_tmp == x_in || x_tmp == x_out) return CHX_ERR_INVALID_ARG;
    for (int64_t e = 0; e < E; ++e)
        if (!T_maps[e]) return CHX_ERR_INVALID_ARG;
    // a scratch of 256 coefficients per element inside x_tmp: the particles stay in registers for the whole run (so_chain_kernel,
    // so_chain_kernel_f64) — two launches per 224 elements instead of E passes over HBM, the same values
    static const bool fused_off = [] { const char* v = getenv("CHX_SO_CHAIN_FUSED"); return v && v[0] == '0'; }();
    // (a longer run takes several such pairs, the later ones in place on x_out: a workgroup holds its whole tile in registers
    // before it writes)
    const int64_t per_pass = std::min<int64_t>(kSoChainMax, N * 7 / kSoCoefStride);
    const bool fuse = !fused_off && E >= 2 && per_pass >= 2;
    if (fuse) {
        hipStream_t s = (hipStream_t)stream;
        const int per_tile = dtype == CHX_F32 ? 2 * CHX_BLOCK : CHX_BLOCK;
        const int64_t tiles = (N + per_tile - 1) / per_tile;
        if (tiles > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
        for (int64_t done = 0; done < E; done += per_pass) {
            const int n = (int)std::min<int64_t>(per_pass, E - done);
            SoChainPtrs maps;
            for (int e = 0; e < kSoChainMax; ++e) {
                maps.T[e] = e < n ? T_maps[done + e] : nullptr;
                maps.length[e] = e < n && lengths ? lengths[done + e] : nullptr;
                maps.linear[e] = (e < n && linear && linear[done + e]) ? 1 : 0;
                if (s_out && e < n && !maps.length[e]) return CHX_ERR_INVALID_ARG;
            }
            const void* src = done == 0 ? x_in : x_out;
            const void* s_from = done == 0 ? s_in : s_out;
            const unsigned blocks = (unsigned)(n + (s_out ? 1 : 0));
            if (dtype == CHX_F32) {
                hipLaunchKernelGGL(so_chain_coeff_kernel<float>, dim3(blocks), dim3(CHX_BLOCK), 0, s, maps, n, (float*)x_tmp,
                                   (const float*)s_from, (float*)s_out);
                CHX_CHECK_LAUNCH();
                hipLaunchKernelGGL(so_chain_kernel, dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s, (const float*)src, (const float*)x_tmp, n,
                                   (float*)x_out, N, (int)chx_aligned16(src), (int)chx_aligned16(x_out));
            } else {
                hipLaunchKernelGGL(so_chain_coeff_kernel<double>, dim3(blocks), dim3(CHX_BLOCK), 0, s, maps, n, (double*)x_tmp,
                                   (const double*)s_from, (double*)s_out);
                CHX_CHECK_LAUNCH();
                hipLaunchKernelGGL(so_chain_kernel_f64, dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s, (const double*)src,
                                   (const double*)x_tmp, n, (double*)x_out, N, (int)chx_aligned16(src), (int)chx_aligned16(x_out));
            }
            CHX_CHECK_LAUNCH();
        }
    } else {
        const void* src = x_in;
        for (int64_t e = 0; e < E; ++e) {
            void* dst = ((E - 1 - e) & 1) ? x_tmp : x_out;
            const int st = (linear && linear[e]) ? chx_apply_affine7(src, T_maps[e], dst, 1, 1, 1, N, dtype, stream)
                                                 : chx_apply_second_order(src, T_maps[e], dst, 1, 1, 1, N, dtype, stream);
            if (st != CHX_OK) return st;
            src = dst;
        }
    }
    for (int64_t done = 0; s_out && !fuse && done < E; done += kDkdSChunk) {      // (the fused form has s from its first launch)
        DkdLengthPtrs a;
        const int n = (int)((E - done < kDkdSChunk) ? (E - done) : kDkdSChunk);
        for (int e = 0; e < kDkdSChunk; ++e) a.p[e] = e < n ? lengths[done + e] : nullptr;
        for (int e = 0; e < n; ++e)
            if (!a.p[e]) return CHX_ERR_INVALID_ARG;
        const void* from = done == 0 ? s_in : s_out;
        if (dtype == CHX_F32)
            hipLaunchKernelGGL(dkd_path_length_kernel<float>, dim3(1), dim3(1), 0, (hipStream_t)stream, a, n, (const float*)from, (float*)s_out);
        else
            hipLaunchKernelGGL(dkd_path_length_kernel<double>, dim3(1), dim3(1), 0, (hipStream_t)stream, a, n, (const double*)from,
                               (double*)s_out);
        CHX_CHECK_LAUNCH();
    }
    return CHX_OK;
}

// ---- the host side of the two ring entry points (chx_second_order_turns, chx_dkd_turns): what both check and launch -------------
namespace {
// the arguments the two entry points share, and what turns_call_ok derives from them
struct TurnsCall {
    const void *x_in, *charges, *survival, *aperture;
    void* x_out;
    int32_t* lost_turn;
    double* sums;
    void* probe;
    int64_t N, K, first_turn, num_turns, record_every;
    int64_t rec0, records;             // records in front of this chunk, records of this chunk
};

// the turn and record ranges. lost_turn holds turn numbers as int32, and the kernels count to first_turn + num_turns in int: the
// last turn stays below INT_MAX. Fills rec0 and records.
bool turns_call_ok(TurnsCall& c) {
    if (c.first_turn < 1 || c.num_turns < 1 || c.record_every < 1 || c.K < 0 || c.K > c.N) return false;
    if (c.first_turn >= 0x7fffffffLL || c.num_turns >= 0x7fffffffLL || c.first_turn + c.num_turns - 1 >= 0x7fffffffLL ||
        c.record_every > 0x7fffffffLL)
        return false;
    c.rec0 = (c.first_turn - 1) / c.record_every;
    c.records = (c.first_turn + c.num_turns - 1) / c.record_every - c.rec0;             // (at most num_turns: a grid size)
    return !(c.records > 0 && (!c.sums || (c.K > 0 && !c.probe)));
}

// aliasing: no output may share an address with another output or with an input, except outs[i] == ins[i] for i < same_ok
// (null pointers are absent arguments)
bool turns_no_alias(std::initializer_list<const void*> outs, std::initializer_list<const void*> ins, size_t same_ok) {
    for (size_t i = 0; i < outs.size(); ++i) {
        const void* o = outs.begin()[i];
        if (!o) continue;
        for (size_t j = i + 1; j < outs.size(); ++j)
            if (o == outs.begin()[j]) return false;
        for (size_t j = 0; j < ins.size(); ++j)
            if (o == ins.begin()[j] && !(i == j && i < same_ok)) return false;
    }
    return true;
}

template <typename T>
SoTurnsArgs<T> turns_args(const TurnsCall& c, int E, void* partials) {
    SoTurnsArgs<T> a;
    a.x_in = (const T*)c.x_in;
    a.x_out = (T*)c.x_out;
    a.charges = (const T*)c.charges;
    a.survival = (const T*)c.survival;
    a.aperture = (const T*)c.aperture;
    a.lost_turn = c.lost_turn;
    a.partials = (double*)partials;
    a.probe = c.K > 0 && c.records > 0 ? (T*)c.probe + c.rec0 * c.K * 7 : nullptr;
    a.N = c.N;
    a.K = c.K;
    a.E = E;
    a.first_turn = (int)c.first_turn;
    a.num_turns = (int)c.num_turns;
    a.next_record = (c.rec0 + 1) * c.record_every;
    a.record_every = c.record_every;
    a.in_vec_ok = (int)chx_aligned16(c.x_in);
    a.out_vec_ok = (int)chx_aligned16(c.x_out);
    return a;
}

// sums[record][14] of this chunk's records from partials[record][tiles][14]
int turns_reduce(const TurnsCall& c, const double* partials, int64_t tiles, hipStream_t s) {
    if (c.records > 0) {
        hipLaunchKernelGGL(so_turns_reduce_kernel, dim3((unsigned)c.records), dim3(CHX_BLOCK), 0, s, partials, tiles,
                           c.sums + c.rec0 * kSoTurnSums);
        CHX_CHECK_LAUNCH();
    }
    return CHX_OK;
}

// A run of second-order elements as a RING: turns [first_turn, first_turn + num_turns) of it in one particle launch (so_turns_kernel,
// so_turns_kernel_f64), with the loss flags, the record sums and the probe rows of the recorded turns (see turns_frame).
int64_t so_turns_tiles(int64_t N, int dtype) {
    const int per_tile = dtype == CHX_F32 ? 2 * CHX_BLOCK : CHX_BLOCK;
    return (N + per_tile - 1) / per_tile;
}
size_t so_turns_coef_bytes(int64_t E, int dtype) { return (size_t)E * kSoCoefStride * (dtype == CHX_F32 ? 4 : 8); }
template <typename T>
int so_turns_launch(const SoChainPtrs& maps, int E, const TurnsCall& c, const void* s_in, void* s_out, void* workspace, int64_t tiles,
                    size_t coef_bytes, hipStream_t s) {
    T* coef = (T*)workspace;
    hipLaunchKernelGGL(so_chain_coeff_kernel<T>, dim3((unsigned)(E + (s_out ? 1 : 0))), dim3(CHX_BLOCK), 0, s, maps, E, coef, (const T*)s_in,
                       (T*)s_out);
    CHX_CHECK_LAUNCH();
    const SoTurnsArgs<T> a = turns_args<T>(c, E, (char*)workspace + coef_bytes);
    if constexpr (sizeof(T) == 4) hipLaunchKernelGGL(so_turns_kernel, dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s, (const float*)coef, a);
    else hipLaunchKernelGGL(so_turns_kernel_f64, dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s, (const double*)coef, a);
    CHX_CHECK_LAUNCH();
    return turns_reduce(c, a.partials, tiles, s);
}
}  // namespace

extern "C" size_t chx_second_order_turns_workspace_bytes(int64_t E, int64_t N, int64_t records_in_chunk, int dtype) {
    if (E < 1 || N < 1 || records_in_chunk < 0 || (dtype != CHX_F32 && dtype != CHX_F64)) return 0;
    return so_turns_coef_bytes(E, dtype) + (size_t)records_in_chunk * (size_t)so_turns_tiles(N, dtype) * kSoTurnSums * sizeof(double);
}

extern "C" int chx_second_order_turns(const void* const* T_maps, const int32_t* linear, const void* const* lengths, int64_t E,
                                      const void* x_in, const void* charges, const void* survival, int64_t N, int dtype,
                                      int64_t first_turn, int64_t num_turns, int64_t record_every, const void* aperture, int64_t K,
                                      void* x_out, int32_t* lost_turn, double* sums, void* probe, const void* s_in, void* s_out,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!T_maps || E < 1 || E > kSoChainMax || !x_in || !x_out || !lost_turn || !workspace || N < 1) return CHX_ERR_INVALID_ARG;
    TurnsCall c{x_in, charges, survival, aperture, x_out, lost_turn, sums, probe, N, K, first_turn, num_turns, record_every, 0, 0};
    if (!turns_call_ok(c)) return CHX_ERR_INVALID_ARG;
    if ((s_in == nullptr) != (s_out == nullptr) || (s_out && !lengths)) return CHX_ERR_INVALID_ARG;
    if (workspace_bytes < chx_second_order_turns_workspace_bytes(E, N, c.records, dtype) || !chx_aligned16(workspace)) return CHX_ERR_INVALID_ARG;
    // aliasing: the first chunk reads a beam it must not write (x_out != x_in), later chunks run in place on x_out; nothing else
    // may share an address
    if (first_turn == 1 && x_in == x_out) return CHX_ERR_INVALID_ARG;
    if (!turns_no_alias({x_out, lost_turn, sums, probe, workspace, s_out}, {x_in, charges, survival, aperture, s_in}, 1)) return CHX_ERR_INVALID_ARG;
    const int64_t tiles = so_turns_tiles(N, dtype);
    if (tiles > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
    SoChainPtrs maps;
    for (int e = 0; e < kSoChainMax; ++e) {
        maps.T[e] = e < E ? T_maps[e] : nullptr;
        maps.length[e] = e < E && lengths ? lengths[e] : nullptr;
        maps.linear[e] = (e < E && linear && linear[e]) ? 1 : 0;
        if (e < E && (!maps.T[e] || (s_out && !maps.length[e]))) return CHX_ERR_INVALID_ARG;
    }
    const size_t coef_bytes = so_turns_coef_bytes(E, dtype);
    if (dtype == CHX_F32) return so_turns_launch<float>(maps, (int)E, c, s_in, s_out, workspace, tiles, coef_bytes, (hipStream_t)stream);
    return so_turns_launch<double>(maps, (int)E, c, s_in, s_out, workspace, tiles, coef_bytes, (hipStream_t)stream);
}

// A ring of Drifts, Quadrupoles, Dipoles, Sextupoles, RFCavities and Multipoles tracked drift-kick-drift: turns [first_turn, first_turn + num_turns) in one particle
// launch (dkd_turns_kernel, dkd_turns_kernel_f64; see the kernels for the energy walk in front of it). The workspace, every part
// 16-byte aligned: start[turns] (dtype) | block_of_turn[turns + 1] (int32) | constants[turns][E][kDkdCstStride] (double) |
// partials[records][tiles][14] (double). The host cannot know how many blocks of constants the device will open: room for one per turn.
namespace {
struct DkdTurnsLayout {
    size_t blocks, cst, partials, total;                      // byte offsets of the parts behind start[], and the size
};
DkdTurnsLayout dkd_turns_layout(int64_t E, int64_t N, int64_t turns, int64_t records, int dtype) {
    DkdTurnsLayout l;
    l.blocks = round_up16((size_t)turns * (dtype == CHX_F32 ? 4 : 8));
    l.cst = l.blocks + round_up16((size_t)(turns + 1) * sizeof(int32_t));
    l.partials = l.cst + (size_t)turns * (size_t)E * kDkdCstStride * sizeof(double);
    l.total = l.partials + (size_t)records * (size_t)((N + CHX_BLOCK - 1) / CHX_BLOCK) * kSoTurnSums * sizeof(double);
    return l;
}
template <typename T>
int dkd_turns_launch(const DkdChainArgs& items, int E, const DkdKinds& has, int mode, const TurnsCall& c, const void* energy_in,
                     void* energy_out, double mass_eV, double n_charges, const void* s_in, void* s_out, void* workspace,
                     const DkdTurnsLayout& l, int64_t tiles, hipStream_t s) {
    const int num_turns = (int)c.num_turns;
    T* start = (T*)workspace;
    int32_t* block_of_turn = (int32_t*)((char*)workspace + l.blocks);
    double* cst = (double*)((char*)workspace + l.cst);
    hipLaunchKernelGGL(dkd_turns_energy_kernel<T>, dim3(1), dim3(1), 0, s, E, num_turns, (const T*)energy_in, (T*)energy_out, mass_eV,
                       start, block_of_turn);
    CHX_CHECK_LAUNCH();
    hipLaunchKernelGGL(dkd_turns_constants_kernel<T>, dim3((unsigned)((int64_t)num_turns * E + (s_out ? 1 : 0))), dim3(64), 0, s, items, E,
                       num_turns, (const T*)start, (const int32_t*)block_of_turn, mass_eV, n_charges, cst, (const T*)s_in, (T*)s_out);
    CHX_CHECK_LAUNCH();
    const SoTurnsArgs<T> a = turns_args<T>(c, E, (char*)workspace + l.partials);
    const dim3 grid((unsigned)tiles), wg(CHX_BLOCK);
    if constexpr (sizeof(T) == 8) {
        dkd_variant(has, [&](auto B, auto S, auto R, auto M) {
            hipLaunchKernelGGL((dkd_turns_kernel_f64<B.value, S.value, R.value, M.value>), grid, wg, 0, s, (const double*)cst,
                               (const int32_t*)block_of_turn, mass_eV, a);
        });
    } else {
        dkd_mode_variant(mode, [&](auto MODE) {
            dkd_variant(has, [&](auto B, auto S, auto R, auto M) {
                hipLaunchKernelGGL((dkd_turns_kernel<MODE.value, B.value, S.value, R.value, M.value>), grid, wg, 0, s, (const double*)cst,
                                   (const int32_t*)block_of_turn, mass_eV, a);
            });
        });
    }
    CHX_CHECK_LAUNCH();
    return turns_reduce(c, a.partials, tiles, s);
}
}  // namespace

extern "C" size_t chx_dkd_turns_workspace_bytes(int64_t E, int64_t N, int64_t turns_in_chunk, int64_t records_in_chunk, int dtype) {
    if (E < 1 || E > kDkdChainMax || N < 1 || turns_in_chunk < 1 || turns_in_chunk >= 0x7fffffffLL || records_in_chunk < 0 ||
        (dtype != CHX_F32 && dtype != CHX_F64))
        return 0;
    return dkd_turns_layout(E, N, turns_in_chunk, records_in_chunk, dtype).total;
}

extern "C" int chx_dkd_turns(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at,
                             int storage_precision, int64_t E, const void* x_in, const void* energy_in, void* energy_out,
                             double mass_eV, double n_charges, const void* charges, const void* survival, int64_t N, int dtype,
                             int64_t first_turn, int64_t num_turns, int64_t record_every, const void* aperture, int64_t K,
                             void* x_out, int32_t* lost_turn, double* sums, void* probe, const void* s_in, void* s_out,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!kinds || !params || !num_steps || !fringe_at || E < 1 || E > kDkdChainMax || !x_in || !energy_in || !energy_out || !x_out ||
        !lost_turn || !workspace || N < 1)
        return CHX_ERR_INVALID_ARG;
    if (storage_precision < 0 || storage_precision > 2) return CHX_ERR_INVALID_ARG;
    TurnsCall c{x_in, charges, survival, aperture, x_out, lost_turn, sums, probe, N, K, first_turn, num_turns, record_every, 0, 0};
    if (!turns_call_ok(c)) return CHX_ERR_INVALID_ARG;
    if ((s_in == nullptr) != (s_out == nullptr)) return CHX_ERR_INVALID_ARG;
    DkdKinds has;
    if (!dkd_items_ok(kinds, params, num_steps, fringe_at, E, &has)) return CHX_ERR_INVALID_ARG;
    const int64_t tiles = (N + CHX_BLOCK - 1) / CHX_BLOCK;
    if (tiles > 0x7fffffffLL || num_turns * E >= 0x7fffffffLL) return CHX_ERR_INVALID_ARG;             // (grid sizes)
    const DkdTurnsLayout l = dkd_turns_layout(E, N, num_turns, c.records, dtype);
    if (workspace_bytes < l.total || !chx_aligned16(workspace)) return CHX_ERR_INVALID_ARG;
    // aliasing: the first chunk reads a beam it must not write (x_out != x_in), later chunks run in place on x_out; energy_out may
    // be energy_in (the chunks of a call hand the energy on through one device scalar); nothing else may share an address
    if (first_turn == 1 && x_in == x_out) return CHX_ERR_INVALID_ARG;
    if (!turns_no_alias({x_out, energy_out, lost_turn, sums, probe, workspace, s_out}, {x_in, energy_in, charges, survival, aperture, s_in}, 2))
        return CHX_ERR_INVALID_ARG;
    const DkdChainArgs items = dkd_chain_args(kinds, params, nullptr, num_steps, fringe_at, 0, (int)E);
    if (dtype == CHX_F32)
        return dkd_turns_launch<float>(items, (int)E, has, storage_precision, c, energy_in, energy_out, mass_eV, n_charges, s_in, s_out, workspace,
                                       l, tiles, (hipStream_t)stream);
    return dkd_turns_launch<double>(items, (int)E, has, 0, c, energy_in, energy_out, mass_eV, n_charges, s_in, s_out, workspace, l, tiles,
                                    (hipStream_t)stream);
}

// The one-turn map of such a ring with its Jacobian, and the closed orbit (include/chx.h). Two launches: the constants of ONE turn
// (dkd_chain_prepare_kernel: the walk of the reference energy a first turn of chx_dkd_turns makes), then dkd_ring_jacobian_kernel.
extern "C" size_t chx_dkd_ring_jacobian_workspace_bytes(int64_t E) {
    if (E < 1 || E > kDkdChainMax) return 0;
    return dkd_ring_layout(E).total;
}

extern "C" int chx_dkd_ring_jacobian(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at,
                                     int64_t E, const void* energy_in, double mass_eV, double n_charges, int dtype, const double* start,
                                     int64_t B, int mode, int64_t num_iterations, int record_along, double* orbit, double* image,
                                     double* matrix, double* residual, double* dispersion, double* orbit_along, double* matrix_along,
                                     void* s_along, void* workspace, size_t workspace_bytes, void* stream) {
    static_assert(kRingCstStride == kDkdCstStride && kRingMeta == kDkdMeta, "dkd_ring_jacobian_kernel reads the chain's blocks");
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!kinds || !params || !num_steps || !fringe_at || E < 1 || E > kDkdChainMax || !energy_in || !start || B < 1 || !orbit || !image ||
        !matrix || !residual || !dispersion || !workspace)
        return CHX_ERR_INVALID_ARG;
    if (mode < 0 || mode > 2 || (mode != 0 && (num_iterations < 1 || num_iterations >= 0x7fffffffLL))) return CHX_ERR_INVALID_ARG;
    if (record_along != 0 && record_along != 1) return CHX_ERR_INVALID_ARG;
    if (record_along && (!orbit_along || !matrix_along || !s_along)) return CHX_ERR_INVALID_ARG;
    if (!dkd_items_ok(kinds, params, num_steps, fringe_at, E)) return CHX_ERR_INVALID_ARG;
    const int64_t groups = chx_optics::workgroups(B);
    if (groups > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
    if (workspace_bytes < dkd_ring_layout(E).total || !chx_aligned16(workspace)) return CHX_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const double* cst;
    const int st = dkd_ring_prepare(kinds, params, num_steps, fringe_at, E, dtype, energy_in, mass_eV, n_charges, workspace, s, cst);
    if (st != CHX_OK) return st;
    const RingJacobianOut o{orbit, image, matrix, residual, dispersion, record_along ? orbit_along : nullptr,
                            record_along ? matrix_along : nullptr, record_along ? s_along : nullptr};
    const int passes = mode == 0 ? 1 : (int)num_iterations + 1;
    hipLaunchKernelGGL(dkd_ring_jacobian_kernel, dim3((unsigned)groups), dim3(chx_optics::kLanes), 0, s, (const double*)cst, (int)E, mass_eV, start,
                       B, mode, passes, dtype == CHX_F32 ? 1 : 0, o);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

// The synchrotron-radiation integrals on the closed orbits a chx_dkd_ring_jacobian call found (include/chx.h). Two launches: the
// constants of one turn as above, then dkd_ring_radiation_kernel.
namespace {
// [p, p + n) and [q, q + k) share a byte (null pointers are absent arguments)
bool bytes_overlap(const void* p, size_t n, const void* q, size_t k) {
    if (!p || !q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + k && b < a + n;
}
}  // namespace

extern "C" size_t chx_dkd_ring_radiation_workspace_bytes(int64_t E) { return chx_dkd_ring_jacobian_workspace_bytes(E); }

extern "C" int chx_dkd_ring_radiation(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at,
                                      int64_t E, const void* energy_in, double mass_eV, double n_charges, int dtype, const double* orbit,
                                      const double* beta0, const double* alpha0, const double* eta0, int64_t B, double* integrals,
                                      double* along, void* workspace, size_t workspace_bytes, void* stream) {
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!kinds || !params || !num_steps || !fringe_at || E < 1 || E > kDkdChainMax || !energy_in || !orbit || !beta0 || !alpha0 || !eta0 ||
        B < 1 || !integrals || !workspace)
        return CHX_ERR_INVALID_ARG;
    if (!dkd_items_ok(kinds, params, num_steps, fringe_at, E)) return CHX_ERR_INVALID_ARG;
    const int64_t groups = chx_optics::workgroups(B);
    if (groups > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
    if (workspace_bytes < dkd_ring_layout(E).total || !chx_aligned16(workspace)) return CHX_ERR_INVALID_ARG;
    // aliasing: nothing that is written may share a byte with anything else
    const size_t row = (size_t)B * sizeof(double);
    const std::pair<const void*, size_t> written[] = {{integrals, row * chx_radiation::kIntegrals},
                                                      {along, row * (size_t)E * chx_radiation::kIntegrals},
                                                      {workspace, workspace_bytes}};
    const std::pair<const void*, size_t> read[] = {{orbit, row * 6}, {beta0, row * 2}, {alpha0, row * 2}, {eta0, row * 4}};
    for (size_t i = 0; i < 3; ++i) {
        for (size_t j = i + 1; j < 3; ++j)
            if (bytes_overlap(written[i].first, written[i].second, written[j].first, written[j].second)) return CHX_ERR_INVALID_ARG;
        for (const auto& r : read)
            if (bytes_overlap(written[i].first, written[i].second, r.first, r.second)) return CHX_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const double* cst;
    const int st = dkd_ring_prepare(kinds, params, num_steps, fringe_at, E, dtype, energy_in, mass_eV, n_charges, workspace, s, cst);
    if (st != CHX_OK) return st;
    const RingRadiationIn in{orbit, beta0, alpha0, eta0};
    hipLaunchKernelGGL(dkd_ring_radiation_kernel, dim3((unsigned)groups), dim3(chx_optics::kLanes), 0, s, (const double*)cst, (int)E, mass_eV, in, B,
                       integrals, along);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

// The derivative of chx_dkd_ring_jacobian's results with respect to K knobs (include/chx.h). Four launches: the constants of one
// turn as above, a fill of the tangents' block with zeros, dkd_ring_sensitivity_prepare_kernel for the (knob, item) pairs a knob
// touches (in pieces of kSensPairs pairs: they travel as kernel arguments), then dkd_ring_sensitivity_kernel.
namespace {
constexpr int kSensPairs = 128;
struct SensPairs {
    const void* params[kSensPairs];        // the item's parameters
    int32_t knob[kSensPairs];
    int32_t meta[kSensPairs];              // item | kind << 8 | fringe_at << 12 | (bit k: the knob moves parameter k) << 14
};

// (a workaround: with a hipMemsetAsync node in its place one replay of a captured graph read stale words where the zeros belong;
// the cause was not found — the node may not have been ordered before its readers —, with a kernel launch it did not happen)
__global__ void dkd_ring_sensitivity_zero_kernel(double* __restrict__ dcst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dcst[i] = 0.0;
}

// the tangent of an item's constants along its knob: dkd_constants<Dual> (what dkd_bwd_kernel evaluates) seeded in the knob's
// parameters, for the energy dkd_chain_prepare_kernel gives the item (a ring has no linear runs: every item in front of it makes
// the round trip)
template <typename T>
__global__ __launch_bounds__(64) void dkd_ring_sensitivity_prepare_kernel(SensPairs p, int count, int E, const T* __restrict__ energy_in, double mc2, double nq,
                                                    double* __restrict__ dcst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int item = p.meta[i] & 255, kind = (p.meta[i] >> 8) & 15, fringe = (p.meta[i] >> 12) & 3, mask = p.meta[i] >> 14;
    const T m = (T)mc2;
    T Ee = *energy_in;
    for (int k = 0; k < item; ++k) {
        const T En = dkd_energy_round_trip<T>(Ee, m);
        if (En == Ee) break;
        Ee = En;
    }
    const int P = dkd_num_params(kind);
    const T* pe = (const T*)p.params[i];
    Dual pd[CHX_MAX_PARAMS], cd[C_N + 1];
#pragma unroll
    for (int k = 0; k < CHX_MAX_PARAMS; ++k) pd[k] = mk(k < P ? (double)pe[k] : 0.0, ((mask >> k) & 1) ? 1.0 : 0.0);
#pragma unroll
    for (int k = 0; k <= C_N; ++k) cd[k] = mk(0.0, 0.0);
    dkd_constants<Dual>(kind, pd, mk((double)Ee, 0.0), mc2, nq, fringe, cd);
    double* out = dcst + ((int64_t)p.knob[i] * E + item) * kSensStride;
#pragma unroll
    for (int k = 0; k <= C_N; ++k) out[k] = cd[k].d;
}
}  // namespace

extern "C" size_t chx_dkd_ring_sensitivity_workspace_bytes(int64_t E, int64_t K) {
    if (E < 1 || E > kDkdChainMax || K < 0 || K > (1 << 20)) return 0;
    return dkd_ring_layout(E).total + (size_t)K * (size_t)E * kSensStride * sizeof(double);
}

extern "C" int chx_dkd_ring_sensitivity(const int32_t* kinds, const void* const* params, const int32_t* num_steps, const int32_t* fringe_at,
                                        int64_t E, const void* energy_in, double mass_eV, double n_charges, int dtype, const double* orbit,
                                        int64_t B, int mode, const int32_t* knob_of, const int32_t* item_of, const int32_t* slot_of,
                                        int64_t num_components, int64_t K, int record_along, double* d_orbit, double* d_image,
                                        double* d_matrix, double* d_dispersion, double* d_orbit_along, double* d_matrix_along, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (!kinds || !params || !num_steps || !fringe_at || E < 1 || E > kDkdChainMax || !energy_in || !orbit || B < 1 || K < 0 || K > (1 << 20) ||
        num_components < 0 || num_components > K * E * CHX_MAX_PARAMS || (num_components > 0 && (!knob_of || !item_of || !slot_of)))
        return CHX_ERR_INVALID_ARG;
    if (mode < 0 || mode > 2 || (record_along != 0 && record_along != 1)) return CHX_ERR_INVALID_ARG;
    if (K > 0 && (!d_orbit || !d_image || !d_matrix || !d_dispersion || !workspace || (record_along && (!d_orbit_along || !d_matrix_along)))) return CHX_ERR_INVALID_ARG;
    if (!dkd_items_ok(kinds, params, num_steps, fringe_at, E)) return CHX_ERR_INVALID_ARG;
    // the components by (knob, item): one pair each, with the set of parameters the knob moves (a component named twice is refused)
    std::vector<std::pair<int64_t, int32_t>> comps((size_t)num_components);
    for (int64_t c = 0; c < num_components; ++c) {
        if (knob_of[c] < 0 || knob_of[c] >= K || item_of[c] < 0 || item_of[c] >= E || slot_of[c] < 0 ||
            slot_of[c] >= dkd_num_params(kinds[item_of[c]]))
            return CHX_ERR_INVALID_ARG;
        comps[(size_t)c] = {(int64_t)knob_of[c] * E + item_of[c], slot_of[c]};
    }
    std::sort(comps.begin(), comps.end());
    for (size_t c = 1; c < comps.size(); ++c)
        if (comps[c] == comps[c - 1]) return CHX_ERR_INVALID_ARG;
    if (K == 0) return CHX_OK;
    const int64_t groups = chx_optics::pair_workgroups(B, K);
    if (groups > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
    if (workspace_bytes < chx_dkd_ring_sensitivity_workspace_bytes(E, K) || !chx_aligned16(workspace)) return CHX_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const double* cst;
    const int st = dkd_ring_prepare(kinds, params, num_steps, fringe_at, E, dtype, energy_in, mass_eV, n_charges, workspace, s, cst);
    if (st != CHX_OK) return st;
    double* dcst = (double*)((char*)workspace + dkd_ring_layout(E).total);          // the tangents' block stands behind the turn's
    const int64_t tangents = K * E * kSensStride;
    hipLaunchKernelGGL(dkd_ring_sensitivity_zero_kernel, dim3((unsigned)((tangents + 255) / 256)), dim3(256), 0, s, dcst, tangents);
    CHX_CHECK_LAUNCH();
    SensPairs pairs;
    int count = 0;
    auto flush = [&]() -> int {
        if (count == 0) return CHX_OK;
        for (int i = count; i < kSensPairs; ++i) {
            pairs.params[i] = nullptr;
            pairs.knob[i] = pairs.meta[i] = 0;
        }
        if (dtype == CHX_F32)
            hipLaunchKernelGGL(dkd_ring_sensitivity_prepare_kernel<float>, dim3((kSensPairs + 63) / 64), dim3(64), 0, s, pairs, count, (int)E,
                               (const float*)energy_in, mass_eV, n_charges, dcst);
        else
            hipLaunchKernelGGL(dkd_ring_sensitivity_prepare_kernel<double>, dim3((kSensPairs + 63) / 64), dim3(64), 0, s, pairs, count, (int)E,
                               (const double*)energy_in, mass_eV, n_charges, dcst);
        CHX_CHECK_LAUNCH();
        count = 0;
        return CHX_OK;
    };
    for (size_t c = 0; c < comps.size(); ++c) {
        const bool same = c > 0 && comps[c].first == comps[c - 1].first;
        if (!same) {
            if (count == kSensPairs) {
                const int rc = flush();
                if (rc != CHX_OK) return rc;
            }
            const int item = (int)(comps[c].first % E);
            pairs.params[count] = params[item];
            pairs.knob[count] = (int32_t)(comps[c].first / E);
            pairs.meta[count] = item | (kinds[item] << 8) | (fringe_at[item] << 12);
            ++count;
        }
        pairs.meta[count - 1] |= (1 << comps[c].second) << 14;
    }
    const int rc = flush();
    if (rc != CHX_OK) return rc;
    const RingSensitivityOut o{d_orbit, d_image, d_matrix, d_dispersion, record_along ? d_orbit_along : nullptr, record_along ? d_matrix_along : nullptr};
    hipLaunchKernelGGL(dkd_ring_sensitivity_kernel, dim3((unsigned)groups), dim3(chx_optics::kLanes), 0, s, (const double*)cst, (const double*)dcst,
                       (int)E, mass_eV, orbit, B, K, mode, o);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

namespace {
template <typename T, int KIND>
int launch_dkd_bwd(const void* x_in, const void* params, const void* energy, const void* dY, double mc2, double nq,
                   int num_steps, int fringe, int P, int64_t B, int64_t Bx, int64_t Bp, int64_t Be, int64_t N, void* dx,
                   double* partials, hipStream_t s) {
    const int64_t tiles = ((N + CHX_BLOCK - 1) / CHX_BLOCK) * B;
    if (tiles > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
    hipLaunchKernelGGL((dkd_bwd_kernel<T, KIND>), dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s, (const T*)x_in,
                       (const T*)params, (const T*)energy, (const T*)dY, mc2, nq, num_steps, fringe, P, B, Bx, Bp, Be, N,
                       (T*)dx, partials);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

template <typename T>
int dispatch_dkd_bwd(int kind, const void* x_in, const void* params, const void* energy, const void* dY, double mc2,
                     double nq, int num_steps, int fringe, int64_t B, int64_t Bx, int64_t Bp, int64_t Be, int64_t N,
                     void* dx, double* partials, hipStream_t s) {
    const int P = dkd_num_params(kind);
    switch (kind) {
        case CHX_DKD_DRIFT:
            return launch_dkd_bwd<T, CHX_DKD_DRIFT>(x_in, params, energy, dY, mc2, nq, num_steps, fringe, P, B, Bx, Bp,
                                                    Be, N, dx, partials, s);
        case CHX_DKD_QUADRUPOLE:
            return launch_dkd_bwd<T, CHX_DKD_QUADRUPOLE>(x_in, params, energy, dY, mc2, nq, num_steps, fringe, P, B, Bx,
                                                         Bp, Be, N, dx, partials, s);
        case CHX_DKD_DIPOLE:
            return launch_dkd_bwd<T, CHX_DKD_DIPOLE>(x_in, params, energy, dY, mc2, nq, num_steps, fringe, P, B, Bx, Bp,
                                                     Be, N, dx, partials, s);
        case CHX_DKD_TDC:
            return launch_dkd_bwd<T, CHX_DKD_TDC>(x_in, params, energy, dY, mc2, nq, num_steps, fringe, P, B, Bx, Bp, Be,
                                                  N, dx, partials, s);
        case CHX_DKD_SEXTUPOLE:
            return launch_dkd_bwd<T, CHX_DKD_SEXTUPOLE>(x_in, params, energy, dY, mc2, nq, num_steps, fringe, P, B, Bx,
                                                        Bp, Be, N, dx, partials, s);
        case CHX_DKD_RFCAVITY:
            return launch_dkd_bwd<T, CHX_DKD_RFCAVITY>(x_in, params, energy, dY, mc2, nq, num_steps, fringe, P, B, Bx,
                                                       Bp, Be, N, dx, partials, s);
        case CHX_DKD_MULTIPOLE:
            return launch_dkd_bwd<T, CHX_DKD_MULTIPOLE>(x_in, params, energy, dY, mc2, nq, num_steps, fringe, P, B, Bx,
                                                        Bp, Be, N, dx, partials, s);
    }
    return CHX_ERR_INVALID_ARG;
}
}  // namespace

extern "C" int64_t chx_dkd_bwd_partials_count(int kind, int64_t B, int64_t N) {
    const int P = dkd_num_params(kind);
    if (P < 0 || B < 0 || N < 0) return 0;
    return B * ((N + CHX_BLOCK - 1) / CHX_BLOCK) * (P + 1);
}

extern "C" int chx_dkd_track_bwd(int kind, const void* x_in, const void* params, const void* energy, const void* dY,
                                 double mass_eV, double n_charges, int32_t num_steps, int32_t fringe_at, int64_t B,
                                 int64_t Bx, int64_t Bp, int64_t Be, int64_t N, int dtype, void* dx, double* partials,
                                 void* stream) {
    if (dkd_num_params(kind) < 0) return CHX_ERR_INVALID_ARG;
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (B < 0 || N < 0) return CHX_ERR_INVALID_ARG;
    if (B == 0 || N == 0) return CHX_OK;
    if (!x_in || !params || !energy || !dY || (!dx && !partials)) return CHX_ERR_INVALID_ARG;
    if (!chx_bcast_ok(Bx, B) || !chx_bcast_ok(Bp, B) || !chx_bcast_ok(Be, B)) return CHX_ERR_INVALID_ARG;
    if ((kind == CHX_DKD_QUADRUPOLE || kind == CHX_DKD_SEXTUPOLE || kind == CHX_DKD_MULTIPOLE) && num_steps < 1) return CHX_ERR_INVALID_ARG;
    if ((kind == CHX_DKD_SEXTUPOLE || kind == CHX_DKD_MULTIPOLE) && num_steps >= (1 << 25)) return CHX_ERR_INVALID_ARG;        // (the chain's and the ring's cap)
    if (fringe_at < 0 || fringe_at > 3) return CHX_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    return dtype == CHX_F32 ? dispatch_dkd_bwd<float>(kind, x_in, params, energy, dY, mass_eV, n_charges, num_steps,
                                                      fringe_at, B, Bx, Bp, Be, N, dx, partials, s)
                            : dispatch_dkd_bwd<double>(kind, x_in, params, energy, dY, mass_eV, n_charges, num_steps,
                                                       fringe_at, B, Bx, Bp, Be, N, dx, partials, s);
}

// ---------------------------------------------------------------------------------------------
// second-order tracking: x_out_i = sum_jk T_ijk x_j x_k (element.py:207-217)
// ---------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ float nl_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double nl_fma(double a, double b, double c) { return fma(a, b, c); }

// The quadratic form is symmetric in (j,k): the 343 coefficients of a batch row are folded once per
// workgroup into U[i][j<=k] = T_ijk + T_ikj (196 doubles in LDS, read wave-uniformly), so a particle costs
// 28 products + 196 FMAs instead of 343 + 49.
template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void second_order_kernel(const T* __restrict__ x_in, const T* __restrict__ Tt,
                                                                 T* __restrict__ x_out, int64_t B, int64_t Bx,
                                                                 int64_t BT, int64_t N, int in_vec_ok,
                                                                 int out_vec_ok) {
    constexpr int TP = CHX_BLOCK;
    __shared__ __attribute__((aligned(16))) T lds[TP * 7];
    __shared__ T U[7 * 28];  // arithmetic in the storage dtype, like the reference's einsum

    const chx_tile<TP> tc = chx_tile_coords<TP>(N);
    const int64_t b = tc.b, n0 = tc.n0;
    const int np = tc.np();
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const bool in_vec = CHX_TILE_VEC_OK(T, in_vec_ok, in_row, N), out_vec = CHX_TILE_VEC_OK(T, out_vec_ok, b, N);

    if (threadIdx.x < 7 * 28) {
        const int i = threadIdx.x / 28;
        int r = threadIdx.x - i * 28, j = 0;
        while (r >= 7 - j) { r -= 7 - j; ++j; }
        const int k = j + r;
        const T* Tb = Tt + ((BT == 1) ? 0 : b) * 343 + i * 49;
        U[threadIdx.x] = (j == k) ? Tb[j * 7 + k] : Tb[j * 7 + k] + Tb[k * 7 + j];
    }
    tile_load<T, TP>(x_in + (in_row * N + n0) * 7, lds, np * 7, in_vec, !(Bx == 1 && B > 1));
    __syncthreads();

    const int p = threadIdx.x;
    if (p < np) {
        T x[7], q[28], y[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) x[j] = lds[p * 7 + j];
        {
            int c = 0;
#pragma unroll
            for (int j = 0; j < 7; ++j)
#pragma unroll
                for (int k = j; k < 7; ++k) q[c++] = x[j] * x[k];
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            T acc = U[i * 28] * q[0];
#pragma unroll
            for (int c = 1; c < 28; ++c) acc = nl_fma(U[i * 28 + c], q[c], acc);
            y[i] = acc;
        }
#pragma unroll
        for (int j = 0; j < 7; ++j) lds[p * 7 + j] = y[j];
    }
    __syncthreads();
    tile_store<T, TP>(x_out + (b * N + n0) * 7, lds, np * 7, out_vec, true);
}


// float32: TWO particles per lane in packed arithmetic (v_pk_mul_f32 / v_pk_fma_f32 on {particle p, particle p + 256}): every
// coefficient fetched from LDS serves two particles and every instruction two multiply-adds; per-lane IEEE fma on both halves,
// the same products in the same order as the one-particle kernel above.
// Round 4 (profiles/r04_second_order.md; kernel trace at 1e6 particles, the linear apply = 9.1 us): the round-3 form of this
// kernel took 17.9 us — 6 of them arithmetic, 1.8 the coefficient fill in FRONT of the tile loads (its two dependent global
// loads stalled every workgroup before it had requested a single row), ~2.6 the lower occupancy (74 VGPRs: the 28 products of
// both particles were kept in registers) and a third barrier. Now: the rows are requested first and the coefficients folded
// while they fly; the products x_j x_k are formed where they are used (same rounding: a product, then an fma), which brings the
// kernel to the apply kernel's 8 waves per SIMD; groups of four coefficients that are all zero are skipped (a drift's tensor has
// 15 non-zero entries of 343, a quadrupole's 27: track_methods.py:80-296) — wave-uniform jumps over a ds_read_b128, four packed
// products and four packed FMAs; a lane overwrites the rows it has read itself, so two barriers suffice. (Wave-private staging
// without any workgroup barrier was measured slower, 19.4 us: as for the linear apply at this size.)
__global__ __launch_bounds__(CHX_BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8)))
void second_order_pk_kernel(const float* __restrict__ x_in, const float* __restrict__ Tt, float* __restrict__ x_out, int64_t B,
                            int64_t Bx, int64_t BT, int64_t N, int in_vec_ok, int out_vec_ok) {
    constexpr int TP = 2 * CHX_BLOCK;
    __shared__ __attribute__((aligned(16))) float lds[TP * 7];
    __shared__ __attribute__((aligned(16))) float U[7 * 28];   // rows of 28 = seven 16-byte groups: read as ds_read_b128
    const chx_tile<TP> tc = chx_tile_coords<TP>(N);
    const int64_t b = tc.b, n0 = tc.n0;
    const int np = tc.np();
    const int64_t in_row = (Bx == 1) ? 0 : b;
    const bool in_vec = CHX_TILE_VEC_OK(float, in_vec_ok, in_row, N), out_vec = CHX_TILE_VEC_OK(float, out_vec_ok, b, N);
    tile_load<float, TP>(x_in + (in_row * N + n0) * 7, lds, np * 7, in_vec, !(Bx == 1 && B > 1));
    if (threadIdx.x < 7 * 28) {
        // U[i][(j,k)], j <= k: T_ijk + T_ikj folded (element.py:207-217 sums over all j, k)
        const int i = threadIdx.x / 28;
        int r = threadIdx.x - i * 28, j = 0;
        while (r >= 7 - j) { r -= 7 - j; ++j; }
        const int k = j + r;
        const float* Tb = Tt + ((BT == 1) ? 0 : b) * 343 + i * 49;
        U[threadIdx.x] = (j == k) ? Tb[j * 7 + k] : Tb[j * 7 + k] + Tb[k * 7 + j];
    }
    __syncthreads();
    unsigned long long groups;
    {
        const int lane = threadIdx.x & 63;
        bool nz = false;
        if (lane < 49) {
            const chx_v4f u = *reinterpret_cast<const chx_v4f*>(&U[4 * lane]);
            nz = u[0] != 0.0f || u[1] != 0.0f || u[2] != 0.0f || u[3] != 0.0f;
        }
        groups = __ballot(nz);
    }
    const int p0 = threadIdx.x, p1 = threadIdx.x + CHX_BLOCK;
    const bool on0 = p0 < np, on1 = p1 < np;
    chx_v2f x[7], y[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) x[j] = chx_v2f{on0 ? lds[p0 * 7 + j] : 0.0f, on1 ? lds[p1 * 7 + j] : 0.0f};
    // The products that are skipped are exact zeros for finite coordinates; a non-finite coordinate makes EVERY output NaN in the
    // dense sum (0 * inf, 0 * nan in each row): restored explicitly. (An overflow of x_j x_k at finite coordinates of ~1e19 is not.)
    bool bad0 = false, bad1 = false;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        bad0 = bad0 || !isfinite(x[j].x);
        bad1 = bad1 || !isfinite(x[j].y);
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        chx_v2f acc = chx_v2f{0.0f, 0.0f};
#pragma unroll
        for (int m = 0; m < 7; ++m) {
            if (!((groups >> (i * 7 + m)) & 1ull)) continue;           // wave-uniform
            const chx_v4f u = *reinterpret_cast<const chx_v4f*>(&U[i * 28 + 4 * m]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                constexpr int kJ[28] = {0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 6};
                constexpr int kK[28] = {0, 1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6, 2, 3, 4, 5, 6, 3, 4, 5, 6, 4, 5, 6, 5, 6, 6};
                const int c = 4 * m + e;
                const chx_v2f uu = {u[e], u[e]};
                const chx_v2f q = x[kJ[c]] * x[kK[c]];
                acc = __builtin_elementwise_fma(uu, q, acc);
            }
        }
        y[i] = chx_v2f{bad0 ? __builtin_nanf("") : acc.x, bad1 ? __builtin_nanf("") : acc.y};
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        if (on0) lds[p0 * 7 + j] = y[j].x;
        if (on1) lds[p1 * 7 + j] = y[j].y;
    }
    __syncthreads();
    tile_store<float, TP>(x_out + (b * N + n0) * 7, lds, np * 7, out_vec, true);
}

// Backward of second_order_kernel (arithmetic in fp64). With h_c = sum_i dY_i U_ic (28 values per particle)
//   dx_m = sum_{k >= m} h_(m,k) x_k + sum_{j <= m} h_(j,m) x_j
// and dU_ic = sum_n dY_i x_j x_k: 196 lanes each own one (i, c) and walk the tile's particles in LDS; a workgroup
// strides over the tiles of its batch row and writes one 196-vector of partial sums (the caller adds them up and
// unfolds dT_ijk = dT_ikj = dU_i(jk)).
constexpr int kSoBwdBlocks = 256;

template <typename T>
__global__ __launch_bounds__(CHX_BLOCK) void second_order_bwd_kernel(const T* __restrict__ x_in, const T* __restrict__ Tt,
                                                                     const T* __restrict__ dY, T* __restrict__ dx,
                                                                     double* __restrict__ dU_partials, int64_t B,
                                                                     int64_t Bx, int64_t BT, int64_t N) {
    constexpr int TP = CHX_BLOCK;
    __shared__ double xs[TP * 7], gs[TP * 7];
    __shared__ double U[7 * 28];
    const int64_t b = blockIdx.y;
    const int64_t in_row = (Bx == 1) ? 0 : b;
    int ui = 0, uj = 0, uk = 0;
    if (threadIdx.x < 7 * 28) {
        ui = threadIdx.x / 28;
        int r = threadIdx.x - ui * 28;
        while (r >= 7 - uj) { r -= 7 - uj; ++uj; }
        uk = uj + r;
        const T* Tb = Tt + ((BT == 1) ? 0 : b) * 343 + ui * 49;
        U[threadIdx.x] = (uj == uk) ? (double)Tb[uj * 7 + uk] : (double)Tb[uj * 7 + uk] + (double)Tb[uk * 7 + uj];
    }
    double dU = 0.0;
    const int64_t tiles = (N + TP - 1) / TP;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t n0 = t * TP;
        const int np = (int)((N - n0 < TP) ? (N - n0) : TP);
        __syncthreads();
        for (int e = threadIdx.x; e < np * 7; e += TP) {
            xs[e] = (double)x_in[(in_row * N + n0) * 7 + e];
            gs[e] = (double)dY[(b * N + n0) * 7 + e];
        }
        __syncthreads();
        const int p = threadIdx.x;
        if (dx && p < np) {
            double x[7], g[7], h[28];
#pragma unroll
            for (int j = 0; j < 7; ++j) { x[j] = xs[p * 7 + j]; g[j] = gs[p * 7 + j]; }
#pragma unroll
            for (int c = 0; c < 28; ++c) {
                double acc = 0.0;
#pragma unroll
                for (int i = 0; i < 7; ++i) acc = fma(g[i], U[i * 28 + c], acc);
                h[c] = acc;
            }
            double d[7] = {0, 0, 0, 0, 0, 0, 0};
            {
                int c = 0;
#pragma unroll
                for (int j = 0; j < 7; ++j)
#pragma unroll
                    for (int k = j; k < 7; ++k) {
                        d[j] = fma(h[c], x[k], d[j]);
                        d[k] = fma(h[c], x[j], d[k]);
                        ++c;
                    }
            }
#pragma unroll
            for (int j = 0; j < 7; ++j) dx[(b * N + n0 + p) * 7 + j] = (T)d[j];
        }
        if (dU_partials && threadIdx.x < 7 * 28) {
            for (int q = 0; q < np; ++q) dU = fma(gs[q * 7 + ui], xs[q * 7 + uj] * xs[q * 7 + uk], dU);
        }
    }
    if (dU_partials && threadIdx.x < 7 * 28) dU_partials[(b * gridDim.x + blockIdx.x) * 196 + threadIdx.x] = dU;
}

}  // namespace

extern "C" int chx_apply_second_order(const void* x_in, const void* T, void* x_out, int64_t B, int64_t Bx,
                                      int64_t BT, int64_t N, int dtype, void* stream) {
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (B < 0 || N < 0) return CHX_ERR_INVALID_ARG;
    if (B == 0 || N == 0) return CHX_OK;
    if (!x_in || !T || !x_out) return CHX_ERR_INVALID_ARG;
    if (!chx_bcast_ok(Bx, B) || !chx_bcast_ok(BT, B)) return CHX_ERR_INVALID_ARG;
    const int64_t tiles = ((N + CHX_BLOCK - 1) / CHX_BLOCK) * B;
    if (tiles > 0x7fffffffLL) return CHX_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == CHX_F32) {
        const int64_t tiles2 = ((N + 2 * CHX_BLOCK - 1) / (2 * CHX_BLOCK)) * B;
        hipLaunchKernelGGL(second_order_pk_kernel, dim3((unsigned)tiles2), dim3(CHX_BLOCK), 0, s, (const float*)x_in, (const float*)T,
                           (float*)x_out, B, Bx, BT, N, (int)chx_aligned16(x_in), (int)chx_aligned16(x_out));
    } else
        hipLaunchKernelGGL(second_order_kernel<double>, dim3((unsigned)tiles), dim3(CHX_BLOCK), 0, s,
                           (const double*)x_in, (const double*)T, (double*)x_out, B, Bx, BT, N,
                           (int)chx_aligned16(x_in), (int)chx_aligned16(x_out));
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}

extern "C" int64_t chx_second_order_bwd_partials_count(int64_t B) { return B * kSoBwdBlocks * 196; }

extern "C" int chx_apply_second_order_bwd(const void* x_in, const void* T, const void* dY, void* dx, double* dU_partials,
                                          int64_t B, int64_t Bx, int64_t BT, int64_t N, int dtype, void* stream) {
    if (dtype != CHX_F32 && dtype != CHX_F64) return CHX_ERR_DTYPE;
    if (B < 0 || N < 0 || B > 65535) return CHX_ERR_INVALID_ARG;
    if (B == 0 || N == 0) return CHX_OK;
    if (!x_in || !T || !dY || (!dx && !dU_partials)) return CHX_ERR_INVALID_ARG;
    if (!chx_bcast_ok(Bx, B) || !chx_bcast_ok(BT, B)) return CHX_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(kSoBwdBlocks, (unsigned)B);
    if (dtype == CHX_F32)
        hipLaunchKernelGGL(second_order_bwd_kernel<float>, grid, dim3(CHX_BLOCK), 0, s, (const float*)x_in, (const float*)T,
                           (const float*)dY, (float*)dx, dU_partials, B, Bx, BT, N);
    else
        hipLaunchKernelGGL(second_order_bwd_kernel<double>, grid, dim3(CHX_BLOCK), 0, s, (const double*)x_in,
                           (const double*)T, (const double*)dY, (double*)dx, dU_partials, B, Bx, BT, N);
    CHX_CHECK_LAUNCH();
    return CHX_OK;
}
