// radiation_check.hip — the host-callable parts of csrc/chx_radiation_dev.h (chx_dkd_ring_radiation, Segment.radiation_integrals)
// against closed-form sector-bend values in long double, without a GPU, under the address and undefined-behaviour sanitizers:
//   hipcc --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all
//         -I cheetah_amd/csrc -o radiation_check tests/host/radiation_check.hip
// Prints one "<part>: ok" line per part and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "chx_radiation_dev.h"

using namespace chx_radiation;
typedef long double ld;

static int failures = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            std::printf("FAILED: ");      \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            ++failures;                   \
        }                                 \
    } while (0)

static void part(const char* name, int before) {
    if (failures == before) std::printf("%s: ok\n", name);
}

// the 4 x 6 block of a sector bend of radius rho through the angle phi in the x plane (a drift of rho phi in y), rel_beta = 1:
// x, px, y, py rows, columns x, px, y, py, tau, delta
static void sector_block(double rho, double phi, double* A) {
    for (int i = 0; i < 24; ++i) A[i] = 0.0;
    const double c = std::cos(phi), s = std::sin(phi);
    A[0 * 6 + 0] = c;        A[0 * 6 + 1] = rho * s;  A[0 * 6 + 5] = rho * (1.0 - c);
    A[1 * 6 + 0] = -s / rho; A[1 * 6 + 1] = c;        A[1 * 6 + 5] = s;
    A[2 * 6 + 2] = 1.0;      A[2 * 6 + 3] = rho * phi;
    A[3 * 6 + 3] = 1.0;
}

// the same point in closed form, long double, by the textbook expressions (gamma eta^2 + 2 alpha eta eta' + beta eta'^2: not the
// header's form of H)
struct Ref {
    ld eta, etap, beta, alpha, H;
};
static Ref sector_ref(ld rho, ld phi, ld beta0, ld alpha0, ld eta0, ld etap0) {
    const ld C = cosl(phi), S = rho * sinl(phi), Cp = -sinl(phi) / rho, Sp = cosl(phi), gamma0 = (1 + alpha0 * alpha0) / beta0;
    Ref r;
    r.eta = C * eta0 + S * etap0 + rho * (1 - cosl(phi));
    r.etap = Cp * eta0 + Sp * etap0 + sinl(phi);
    r.beta = C * C * beta0 - 2 * C * S * alpha0 + S * S * gamma0;
    r.alpha = -C * Cp * beta0 + (C * Sp + S * Cp) * alpha0 - S * Sp * gamma0;
    const ld gamma = (1 + r.alpha * r.alpha) / r.beta;
    r.H = gamma * r.eta * r.eta + 2 * r.alpha * r.eta * r.etap + r.beta * r.etap * r.etap;
    return r;
}

static bool close_to(double got, ld want, ld rel, ld scale = 0) {
    const ld s = scale > 0 ? scale : fabsl(want);
    return fabsl((ld)got - want) <= rel * s;
}

int main() {
    int before = failures;
    // ---- the Gauss-Legendre table: ascending nodes in (0, 1), symmetric, weights sum to 1, monomials exact up to degree 15
    {
        ld wsum = 0;
        for (int j = 0; j < kNodes; ++j) {
            wsum += gl8_weight(j);
            EXPECT(gl8_node(j) > 0.0 && gl8_node(j) < 1.0, "node %d outside (0, 1)", j);
            if (j > 0) EXPECT(gl8_node(j) > gl8_node(j - 1), "nodes not ascending at %d", j);
            EXPECT(std::fabs(gl8_node(j) + gl8_node(kNodes - 1 - j) - 1.0) <= 2.3e-16, "nodes %d not symmetric", j);
            EXPECT(gl8_weight(j) == gl8_weight(kNodes - 1 - j), "weights %d not symmetric", j);
        }
        EXPECT(fabsl(wsum - 1) <= 2.3e-16L, "weights sum to 1 %+.3Le", wsum - 1);
        for (int k = 0; k <= 15; ++k) {
            ld q = 0;
            for (int j = 0; j < kNodes; ++j) q += (ld)gl8_weight(j) * powl((ld)gl8_node(j), k);
            EXPECT(fabsl(q * (k + 1) - 1) <= 1e-15L, "degree %d: %.3Le", k, q * (k + 1) - 1);
        }
        ld q16 = 0;                        // degree 16 is the first the rule misses, by (8!)^4 / (17 (16!)^2) = 3.5e-10
        for (int j = 0; j < kNodes; ++j) q16 += (ld)gl8_weight(j) * powl((ld)gl8_node(j), 16);
        EXPECT(fabsl(q16 - 1.0L / 17) > 1e-12L && fabsl(q16 - 1.0L / 17) < 1e-9L, "degree 16: %.3Le", q16 - 1.0L / 17);
    }
    part("gauss-legendre table", before);

    before = failures;
    // ---- a lane's terms and the order of the group's sum
    {
        const double col[4] = {1.5, -2.5, 3.5, -4.5}, eta0[4] = {0.1, 0.2, 0.3, 0.4}, beta0[2] = {2.0, 3.0}, alpha0[2] = {0.5, -0.25};
        double t[kTerms];
        for (int m = 6; m < 8; ++m) {
            lane_terms(m, col, eta0, beta0, alpha0, t);
            for (int k = 0; k < kTerms; ++k) EXPECT(t[k] == 0.0, "lane %d term %d is not zero", m, k);
        }
        lane_terms(4, col, eta0, beta0, alpha0, t);
        for (int k = 0; k < kTerms; ++k) EXPECT(t[k] == 0.0, "lane 4 term %d is not zero", k);
        lane_terms(5, col, eta0, beta0, alpha0, t);
        for (int k = 0; k < kTerms; ++k) EXPECT(t[k] == (k < 4 ? col[k] : 0.0), "lane 5 term %d", k);
        lane_terms(1, col, eta0, beta0, alpha0, t);
        EXPECT(t[0] == 0.2 * 1.5 && t[4] == -(0.5 * 1.5) && t[5] == -(0.5 * -2.5) && t[6] == 1.5 && t[7] == -2.5 && t[8] == 0.0 && t[11] == 0.0,
               "lane 1 terms");
        lane_terms(2, col, eta0, beta0, alpha0, t);
        EXPECT(t[2] == 0.3 * 3.5 && t[8] == 3.0 * 3.5 && t[9] == 3.0 * -4.5 && t[10] == 0.0 && t[4] == 0.0, "lane 2 terms");
        const double v[8] = {1e16, 1.0, -1e16, 1.0, 3.0, 4.0, 5.0, 6.0};
        EXPECT(group_sum(v) == ((1e16 + 1.0) + (-1e16 + 1.0)) + ((3.0 + 4.0) + (5.0 + 6.0)), "group_sum order");
    }
    part("lane terms", before);

    before = failures;
    // ---- eta, beta, alpha and H at points of a sector bend from arbitrary start values, against the closed forms
    {
        const double rho = 0.95492965855137201, beta0[2] = {1.7, 2.9}, alpha0[2] = {-0.6, 0.8}, eta0[4] = {0.31, -0.07, 0.0, 0.0};
        for (int k = 0; k <= 10; ++k) {
            const double phi = 0.5235987755982988 * k / 10.0;
            double A[24];
            sector_block(rho, phi, A);
            Node n;
            node_from_block(A, eta0, beta0, alpha0, 1.0, n);
            const Ref r = sector_ref(rho, phi, beta0[0], alpha0[0], eta0[0], eta0[1]);
            EXPECT(close_to(n.eta[0], r.eta, 4e-16L, 1) && close_to(n.eta[1], r.etap, 4e-16L, 1), "eta at phi %g", phi);
            EXPECT(close_to(n.beta[0], r.beta, 1e-15L) && close_to(n.alpha[0], r.alpha, 2e-15L, 1), "beta, alpha at phi %g", phi);
            EXPECT(close_to(n.H[0], r.H, 4e-15L), "H at phi %g: %.17g against %.17Lg", phi, n.H[0], r.H);
            // y: a drift of rho phi, no dispersion: H_y is an exact zero
            const ld L = (ld)rho * phi, g0 = (1 + (ld)alpha0[1] * alpha0[1]) / beta0[1];
            EXPECT(close_to(n.beta[1], beta0[1] - 2 * L * alpha0[1] + L * L * g0, 1e-15L) && close_to(n.alpha[1], alpha0[1] - L * g0, 2e-15L, 1),
                   "beta_y, alpha_y at phi %g", phi);
            EXPECT(n.eta[2] == 0.0 && n.eta[3] == 0.0 && n.H[1] == 0.0, "y dispersion at phi %g", phi);
            // the factor p0c / E0 scales eta and eta', H with its square
            Node s;
            node_from_block(A, eta0, beta0, alpha0, 0.5, s);
            EXPECT(s.eta[0] == 0.5 * (n.eta[0]) && close_to(s.H[0], 0.25L * n.H[0], 4e-16L) && s.beta[0] == n.beta[0], "rel_beta at phi %g", phi);
        }
        // a plane without a periodic solution is NaN in its own beta, alpha and H only
        double A[24];
        sector_block(rho, 0.3, A);
        const double bad[2] = {beta0[0], NAN}, bad_a[2] = {alpha0[0], NAN};
        Node n, ok;
        node_from_block(A, eta0, bad, bad_a, 1.0, n);
        node_from_block(A, eta0, beta0, alpha0, 1.0, ok);
        EXPECT(n.H[1] != n.H[1] && n.beta[1] != n.beta[1], "NaN start values in y do not reach H_y");
        EXPECT(n.H[0] == ok.H[0] && n.beta[0] == ok.beta[0] && n.eta[0] == ok.eta[0] && n.eta[2] == 0.0, "NaN start values in y leak into x");
    }
    part("point inside a sector bend", before);

    before = failures;
    // ---- a Dipole's contribution: the matched cell of a ring of one sector bend (beta = rho, alpha = 0, eta = rho, H = rho at every
    // point), the edge terms, the tilt, the zeros; and an unmatched bend against a fine composite Simpson sum of the closed forms
    {
        const double rho = 1.25, h = 1.0 / rho, theta = 0.5235987755982988, L = rho * theta;
        const double beta0[2] = {rho, 3.0}, alpha0[2] = {0.0, 0.0}, eta0[4] = {rho, 0.0, 0.0, 0.0};
        BendSums b = bend_sums_zero();
        for (int j = 0; j < kNodes; ++j) {
            double A[24];
            sector_block(rho, gl8_node(j) * theta, A);
            Node n;
            node_from_block(A, eta0, beta0, alpha0, 1.0, n);
            bend_sums_add(b, gl8_weight(j), 1.0, 0.0, n);
        }
        double out[kIntegrals];
        bend_contribution(L, h, 1.0, 0.0, 0.0, 0.0, rho, rho, b, out);
        EXPECT(close_to(out[0], (ld)L, 2e-15L) && out[1] == L * (h * h) && out[2] == L * (h * h * h), "I1, I2, I3 of the matched bend");
        EXPECT(close_to(out[3], (ld)L * h * h, 2e-15L) && close_to(out[5], (ld)L * h * h, 2e-15L) && out[4] == 0.0 && out[6] == 0.0,
               "I4, I5 of the matched bend: %.17g %.17g %g %g", out[3], out[5], out[4], out[6]);
        // rectangular faces e1 = e2 = theta / 2 take h^2 eta tan e off I4 each
        const double ch = h * std::tan(0.5 * theta);
        double rect[kIntegrals];
        bend_contribution(L, h, 1.0, 0.0, ch, ch, rho, rho, b, rect);
        EXPECT(close_to(rect[3], (ld)L * h * h - 2 * (ld)h * ch * rho, 4e-15L, (ld)L * h * h) && rect[0] == out[0] && rect[5] == out[5], "edge terms");
        double one[kIntegrals];
        bend_contribution(L, h, 1.0, 0.0, ch, 0.0, rho, 7.0, b, one);                    // a face whose fringe is off takes nothing
        EXPECT(close_to(one[3], (ld)L * h * h - (ld)h * ch * rho, 4e-15L, (ld)L * h * h), "one edge");
        // the sign of h: I1 and I4 are odd in it with eta as it is, I3 and I5 even
        double neg[kIntegrals];
        bend_contribution(L, -h, 1.0, 0.0, 0.0, 0.0, rho, rho, b, neg);
        EXPECT(neg[0] == -out[0] && neg[1] == out[1] && neg[2] == out[2] && neg[3] == -out[3] && neg[5] == out[5], "the sign of h");
        // a vertical bend: the same sums with the planes swapped land in I4y, I5y; I4x is an exact zero
        BendSums v = bend_sums_zero();
        v.s1 = b.s1; v.s4y = b.s4x; v.s5y = b.s5x;
        double vert[kIntegrals];
        bend_contribution(L, h, 0.0, 1.0, ch, ch, rho, rho, v, vert);
        EXPECT(vert[4] == rect[3] && vert[6] == rect[5] && vert[3] == 0.0 && vert[5] == 0.0 && vert[0] == rect[0], "vertical bend");
        double zero[kIntegrals];
        bend_contribution(0.0, NAN, 1.0, 0.0, NAN, NAN, NAN, NAN, b, zero);
        for (int k = 0; k < kIntegrals; ++k) EXPECT(zero[k] == 0.0, "L = 0, entry %d", k);
        bend_contribution(L, 0.0, 1.0, 0.0, 0.0, 0.0, rho, rho, b, zero);
        for (int k = 0; k < kIntegrals; ++k) EXPECT(zero[k] == 0.0, "h = 0, entry %d", k);

        // unmatched: sum_j w_j H(s_j) and sum_j w_j eta(s_j) against composite Simpson with 2000 intervals of the closed forms
        const double ub[2] = {1.7, 2.9}, ua[2] = {-0.6, 0.8}, ue[4] = {0.31, -0.07, 0.0, 0.0};
        BendSums u = bend_sums_zero();
        for (int j = 0; j < kNodes; ++j) {
            double A[24];
            sector_block(rho, gl8_node(j) * theta, A);
            Node n;
            node_from_block(A, ue, ub, ua, 1.0, n);
            bend_sums_add(u, gl8_weight(j), 1.0, 0.0, n);
        }
        const int N = 2000;
        ld sh = 0, se = 0;
        for (int k = 0; k <= N; ++k) {
            const Ref r = sector_ref(rho, (ld)theta * k / N, ub[0], ua[0], ue[0], ue[1]);
            const ld w = (k == 0 || k == N) ? 1 : (k % 2 ? 4 : 2);
            sh += w * r.H;
            se += w * r.eta;
        }
        sh /= 3 * (ld)N;
        se /= 3 * (ld)N;
        EXPECT(close_to(u.s5x, sh, 1e-13L) && close_to(u.s4x, se, 1e-13L) && u.s1 == u.s4x, "quadrature of an unmatched bend: %.3Le %.3Le",
               (u.s5x - sh) / sh, (u.s4x - se) / se);
    }
    part("bend contribution", before);

    if (failures) std::printf("%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
