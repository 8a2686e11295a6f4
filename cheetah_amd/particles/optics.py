"""Linear optics of a ring from its one-turn matrix: what `Segment.one_turn_map`, `Segment.closed_orbit` and `Segment.ring_optics`
return, and the algebra between them.

`twiss_from_matrix`, `propagate_twiss` and `eigen_tunes` are plain float64 torch on whatever device their inputs are on (no
kernel, no synchronisation): they also run on CPU tensors. The matrices come from `chx_dkd_ring_jacobian` (include/chx.h), which
carries a phase-space point and its six tangents through a ring of drift-kick-drift elements in one launch.

Coordinates: (x, px, y, py, tau, delta). A one-turn matrix M is symplectic with S = diag(J2, J2, -J2) (tau and delta form a pair
of the opposite sign), which is why the off-momentum quantities below read column 5 and row 4.

beta, alpha and the phase advance are the UNCOUPLED (projected) functions of the two diagonal 2 x 2 blocks. In a ring with
coupling (tilted quadrupoles, skew multipoles, an orbit off the axis of a sextupole) they are not the functions of the normal
modes; `RingOptics.coupling` — the largest absolute entry of the two off-diagonal 2 x 2 blocks of M_4 — says when to distrust
them. The tunes are eigen-tunes of the full 4 x 4 block and stay right with coupling.

Gradients with respect to settings: `Segment.ring_sensitivity` returns the raw tangents (`RingSensitivity`), and with `wrt=...` the
results of `one_turn_map`, `closed_orbit`, `ring_optics` and `chromaticity` carry an autograd graph to the named settings — one
node (`RingValues`) whose forward keeps the tangents of `chx_dkd_ring_sensitivity` and whose backward contracts them with the
cotangents; the algebra below differentiates by itself from there.

Out of scope here: vectorised lattice settings, second derivatives of the optics, gradients with respect to the energy, Edwards-Teng
or other coupled parametrisations, the synchrotron tune of a 6-D search (`matrix` is returned: take its eigenvalues), second-order
and linear rings."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

__all__ = ["OneTurnMap", "ClosedOrbit", "RingOptics", "RingSensitivity", "RadiationIntegrals", "twiss_from_matrix", "propagate_twiss",
           "eigen_tunes"]

_TWO_PI = 2.0 * math.pi


def _block(M: torch.Tensor, plane: int) -> torch.Tensor:
    return M[..., 2 * plane:2 * plane + 2, 2 * plane:2 * plane + 2]


def twiss_from_matrix(M: torch.Tensor):
    """(beta, alpha, mu) of a periodic 2 x 2 block M (..., 2, 2): cos mu = tr / 2, beta = M12 / sin mu, alpha = (M11 - M22) / (2 sin mu)
    with the sign of sin mu taken from M12, so beta > 0 and mu lies in (0, 2 pi): a fractional tune above one half comes back above
    one half. NaN where |tr| >= 2 (no periodic solution)."""
    M = M.to(torch.float64)
    m11, m12, m22 = M[..., 0, 0], M[..., 0, 1], M[..., 1, 1]
    cos_mu = 0.5 * (m11 + m22)
    # sin^2 = 1 - cos^2 loses digits beside cos = +-1; det M = 1 gives the same number as -(M12 M21) - ((M11 - M22) / 2)^2
    half = 0.5 * (m11 - m22)
    sin2 = -(m12 * M[..., 1, 0]) - half * half
    stable = (cos_mu.abs() < 1.0) & (sin2 > 0)
    nan = torch.full_like(cos_mu, float("nan"))
    sin_mu = torch.where(stable, torch.sqrt(torch.where(stable, sin2, torch.ones_like(sin2))) * torch.sign(m12), nan)
    beta = m12 / sin_mu
    alpha = half / sin_mu
    mu = torch.remainder(torch.atan2(sin_mu, cos_mu), _TWO_PI)
    return beta, alpha, mu


def propagate_twiss(A: torch.Tensor, beta0: torch.Tensor, alpha0: torch.Tensor):
    """(beta, alpha, phase) behind a 2 x 2 transfer block A (..., 2, 2) for the functions beta0, alpha0 in front of it:
    beta = ((A11 beta0 - A12 alpha0)^2 + A12^2) / beta0, alpha = -((A11 beta0 - A12 alpha0)(A21 beta0 - A22 alpha0) + A12 A22) / beta0,
    phase = atan2(A12, A11 beta0 - A12 alpha0) in [0, 2 pi)."""
    A = A.to(torch.float64)
    a11, a12, a21, a22 = A[..., 0, 0], A[..., 0, 1], A[..., 1, 0], A[..., 1, 1]
    u = a11 * beta0 - a12 * alpha0
    w = a21 * beta0 - a22 * alpha0
    beta = (u * u + a12 * a12) / beta0
    alpha = -(u * w + a12 * a22) / beta0
    phase = torch.remainder(torch.atan2(a12, u), _TWO_PI)
    return beta, alpha, phase


def eigen_tunes(M4: torch.Tensor):
    """(tunes, stable) of a symplectic 4 x 4 one-turn block (..., 4, 4), both (..., 2): the eigenvalues come in pairs exp(+-i mu), and
    u = 2 cos mu solves u^2 - a u + (b - 2) = 0 with a = tr M and b = (a^2 - tr M^2) / 2 — closed form, no eigen-solver. The two roots
    go to x and y by the nearer trace of a diagonal block; the fractional tune lies in [0, 1) with the sign of sin mu from M12 (M34).
    NaN and stable = False where a root is complex or |u| > 2."""
    M4 = M4.to(torch.float64)
    a = M4.diagonal(dim1=-2, dim2=-1).sum(-1)
    tr2 = (M4 * M4.transpose(-1, -2)).sum((-2, -1))
    b = 0.5 * (a * a - tr2)
    # the roots of u^2 - a u + (b - 2): discriminant a^2 - 4 b + 8 = 2 tr M^2 - a^2 + 8
    disc = a * a - 4.0 * (b - 2.0)
    real = disc >= 0
    root = torch.sqrt(torch.where(real, disc, torch.zeros_like(disc)))
    u_hi, u_lo = 0.5 * (a + root), 0.5 * (a - root)
    tx = M4[..., 0, 0] + M4[..., 1, 1]
    ty = M4[..., 2, 2] + M4[..., 3, 3]
    x_high = tx >= ty                                           # the larger root to the plane with the larger block trace
    u = torch.stack([torch.where(x_high, u_hi, u_lo), torch.where(x_high, u_lo, u_hi)], dim=-1)
    sign = torch.sign(torch.stack([M4[..., 0, 1], M4[..., 2, 3]], dim=-1))
    stable = real.unsqueeze(-1) & (u.abs() <= 2.0)
    cos_mu = torch.where(stable, 0.5 * u, torch.zeros_like(u))
    mu = torch.acos(cos_mu)                                     # in [0, pi]
    mu = torch.where(sign < 0, _TWO_PI - mu, mu)
    tunes = torch.remainder(mu / _TWO_PI, 1.0)
    return torch.where(stable, tunes, torch.full_like(tunes, float("nan"))), stable


def _along(matrix_along: torch.Tensor, beta0: torch.Tensor, alpha0: torch.Tensor):
    """beta, alpha and the accumulated phase (B, E + 1, 2) from the cumulative matrices (B, E + 1, 6, 6) and the start values (B, 2)."""
    betas, alphas, phases = [], [], []
    for plane in range(2):
        A = _block(matrix_along, plane)                                        # (B, E + 1, 2, 2)
        b0, a0 = beta0[:, None, plane], alpha0[:, None, plane]
        beta, alpha, phi = propagate_twiss(A, b0, a0)
        # item by item: each increment in [0, 2 pi) (an item advances the phase by less than a turn) — so the accumulated phase is
        # phi_k plus 2 pi for every item at which phi fell. Counted in integers: no sum of rounded increments, and the same bits
        # for a seed whatever the batch it stands in. (A fall of rounding size — a thin kick between the two rotations of a tilt —
        # is no advance of a whole turn.)
        wraps = torch.cumsum(((phi[:, 1:] - phi[:, :-1]) < -1e-9).to(torch.int64), dim=1)
        total = phi + _TWO_PI * torch.cat([torch.zeros_like(wraps[:, :1]), wraps], dim=1).to(torch.float64)       # (NaN stays NaN)
        betas.append(beta)
        alphas.append(alpha)
        phases.append(total)
    return torch.stack(betas, -1), torch.stack(alphas, -1), torch.stack(phases, -1)


@dataclass
class OneTurnMap:
    """`Segment.one_turn_map`: `start` (B, 7) the seeds, `end` (B, 7) their images after one turn, `matrix` (B, 6, 6) with
    matrix[b, i, m] = d end_i / d start_m, all float64. With `along`: `orbit_along` (B, E + 1, 7), `matrix_along` (B, E + 1, 6, 6) —
    index 0 the start (the identity), index k behind item k of the ring, the cumulative map — and `s` (E + 1,) in the settings' dtype."""
    start: torch.Tensor
    end: torch.Tensor
    matrix: torch.Tensor
    orbit_along: Optional[torch.Tensor] = None
    matrix_along: Optional[torch.Tensor] = None
    s: Optional[torch.Tensor] = None


@dataclass
class ClosedOrbit:
    """`Segment.closed_orbit`: `orbit` (B, 7) the closed orbit at the start of the ring, `residual` (B,) = max |one turn of it - it| over
    the closed coordinates (x, px, y, py; with `longitudinal` all six), `matrix` (B, 6, 6) the one-turn matrix on it, `dispersion`
    (B, 4) = (I - M_4)^-1 M[:4, 5], d(x, px, y, py) / d delta of the 4-D closed orbit. float64. A seed whose search failed (beyond the
    dynamic aperture, a singular Newton system) is NaN in its own rows."""
    orbit: torch.Tensor
    residual: torch.Tensor
    matrix: torch.Tensor
    dispersion: torch.Tensor


@dataclass
class RingOptics(ClosedOrbit):
    """`Segment.ring_optics`: the `ClosedOrbit` fields and
    tunes (B, 2)          the fractional eigen-tunes of the 4 x 4 block in [0, 1) (`eigen_tunes`), NaN where unstable
    stable (B, 2)         bool
    coupling (B,)         the largest absolute entry of the two off-diagonal 2 x 2 blocks of M_4
    beta, alpha, phase_advance   (B, E + 1, 2) with `along` — index 0 the start, index k behind item k — else the start values (B, 2)
                          (phase_advance: zeros). The UNCOUPLED (projected) functions of the diagonal blocks: `coupling` tells
                          when to distrust them. phase_advance[:, -1] / 2 pi is the full tune with its integer part.
    dispersion_along (B, E + 1, 4)   eta_k = A_k[:4, :4] eta_0 + A_k[:4, 5] (None without `along`)
    orbit_along (B, E + 1, 7)        the closed orbit behind every item (None without `along`)
    slip (B,)             M[4, 5] + M[4, :4] . eta_0: d tau / d delta per turn on the dispersive orbit
    s (E + 1,)            the path length behind every item, in the settings' dtype (None without `along`)"""
    tunes: torch.Tensor = None
    stable: torch.Tensor = None
    coupling: torch.Tensor = None
    beta: torch.Tensor = None
    alpha: torch.Tensor = None
    phase_advance: torch.Tensor = None
    slip: torch.Tensor = None
    dispersion_along: Optional[torch.Tensor] = None
    orbit_along: Optional[torch.Tensor] = None
    s: Optional[torch.Tensor] = None


def ring_optics_from(closed: ClosedOrbit, orbit_along=None, matrix_along=None, s=None) -> RingOptics:
    """The optics of a closed orbit and (optionally) the cumulative matrices along the ring: torch algebra only."""
    M = closed.matrix
    M4 = M[:, :4, :4]
    tunes, stable_eig = eigen_tunes(M4)
    coupling = torch.maximum(M4[:, :2, 2:].abs().amax((-2, -1)), M4[:, 2:, :2].abs().amax((-2, -1)))
    b0, a0 = [], []
    for plane in range(2):
        beta, alpha, _ = twiss_from_matrix(_block(M, plane))
        b0.append(beta)
        a0.append(alpha)
    beta0, alpha0 = torch.stack(b0, -1), torch.stack(a0, -1)
    stable = stable_eig
    eta0 = closed.dispersion
    slip = M[:, 4, 5] + (M[:, 4, :4] * eta0).sum(-1)
    if matrix_along is None:
        return RingOptics(closed.orbit, closed.residual, M, eta0, tunes=tunes, stable=stable, coupling=coupling, beta=beta0, alpha=alpha0,
                          phase_advance=torch.zeros_like(beta0), slip=slip)
    beta, alpha, phase = _along(matrix_along, beta0, alpha0)
    eta = (matrix_along[:, :, :4, :4] @ eta0[:, None, :, None]).squeeze(-1) + matrix_along[:, :, :4, 5]
    return RingOptics(closed.orbit, closed.residual, M, eta0, tunes=tunes, stable=stable, coupling=coupling, beta=beta, alpha=alpha,
                      phase_advance=phase, slip=slip, dispersion_along=eta, orbit_along=orbit_along, s=s)


_ELECTRON_RADIUS = 2.8179403205e-15       # r_e, m (CODATA 2022; csrc/chx_sr.hip)
_ELECTRON_MASS_EV = 510998.95069          # m_e c^2, eV
_HBAR_C = 1.973269804593025e-7            # hbar c, eV m
_SPEED_OF_LIGHT = 299792458.0


@dataclass
class RadiationIntegrals:
    """`Segment.radiation_integrals`: the synchrotron-radiation integrals of a ring on its 4-D closed orbit and what follows from
    them, float64, B seeds, E items, planes u = x, y (the definitions: the method's docstring, include/chx.h).
    I1, I2, I3 (B,)       I4, I5 (B, 2)
    integrals_along (B, E, 7)   every item's contribution in the order (I1, I2, I3, I4x, I4y, I5x, I5y), exact zeros for items
                          that are no Dipoles (None without `along`); the totals are the sums over the items in their order
    closed                the `RingOptics` (without `along`) the integrals were evaluated on
    energy_loss (B,)      U0 = (2/3) r_c mc^2 beta0^3 gamma0^4 I2, eV per turn
    partition (B, 3)      (J_x, J_y, J_E) = (1 - I4x / I2, 1 - I4y / I2, 2 + (I4x + I4y) / I2)
    damping_turns (B, 3)  2 E0 / (J U0)
    damping_time (B, 3)   damping_turns C / (beta0 c), s
    emittance (B, 2)      eps_u = C_q gamma0^2 I5u / (J_u I2), geometric, m rad; C_q = 55 / (32 sqrt 3) lambda_c. The vertical
                          opening-angle limit is not included: eps_y = 0 in a flat ring
    energy_spread (B,)    sigma_delta = sqrt(C_q gamma0^2 I3 / (J_E I2))
    circumference         C, the sum of the items' lengths (0-d)
    A seed whose search failed is NaN in its own rows; a plane without a periodic solution is NaN in its I5 and emittance."""
    I1: torch.Tensor
    I2: torch.Tensor
    I3: torch.Tensor
    I4: torch.Tensor
    I5: torch.Tensor
    integrals_along: Optional[torch.Tensor]
    closed: "RingOptics"
    energy_loss: torch.Tensor
    partition: torch.Tensor
    damping_turns: torch.Tensor
    damping_time: torch.Tensor
    emittance: torch.Tensor
    energy_spread: torch.Tensor
    circumference: torch.Tensor


def radiation_constants(mass_eV: float, num_charges: float):
    """(r_c, C_q) of a species: r_c = Z^2 r_e m_e / m in m and C_q = 55 / (32 sqrt 3) hbar c / mc^2 in m, as `SynchrotronRadiationKick`
    takes them."""
    r_c = num_charges * num_charges * _ELECTRON_RADIUS * _ELECTRON_MASS_EV / mass_eV
    return r_c, 55.0 / (32.0 * math.sqrt(3.0)) * _HBAR_C / mass_eV


def radiation_integrals_from(closed: "RingOptics", integrals: torch.Tensor, integrals_along, energy: torch.Tensor, mass_eV: float,
                             num_charges: float, circumference: torch.Tensor) -> RadiationIntegrals:
    """The `RadiationIntegrals` of the kernel's sums (B, 7): a handful of float64 torch operations, no synchronisation."""
    I1, I2, I3, I4, I5 = integrals[:, 0], integrals[:, 1], integrals[:, 2], integrals[:, 3:5], integrals[:, 5:7]
    E0 = energy.to(torch.float64)
    r_c, c_q = radiation_constants(mass_eV, num_charges)
    gamma2 = (E0 / mass_eV) ** 2
    beta_rel = torch.sqrt(1.0 - 1.0 / gamma2)
    loss = (2.0 / 3.0) * r_c * mass_eV * beta_rel ** 3 * gamma2 * gamma2 * I2
    ratio = I4 / I2[:, None]
    partition = torch.cat([1.0 - ratio, 2.0 + ratio.sum(-1, keepdim=True)], dim=-1)
    turns = 2.0 * E0 / (partition * loss[:, None])
    C = circumference.to(torch.float64)
    emittance = c_q * gamma2 * I5 / (partition[:, :2] * I2[:, None])
    spread = torch.sqrt(c_q * gamma2 * I3 / (partition[:, 2] * I2))
    return RadiationIntegrals(I1, I2, I3, I4, I5, integrals_along, closed, loss, partition, turns, turns * (C / (beta_rel * _SPEED_OF_LIGHT)),
                              emittance, spread, C)


@dataclass
class RingSensitivity:
    """`Segment.ring_sensitivity`: the derivatives of a closed orbit and its optics with respect to K knobs — the tensors of `wrt` in
    their order, a 0-d setting one knob, an (n,) setting (a misalignment) n knobs in a row; a tensor shared by many elements is ONE
    knob. Total derivatives: the closed orbit moves with the knob. float64.
    closed                the `ClosedOrbit` the derivatives were taken on
    d_orbit (B, K, 6)                 d orbit / d knob at the start of the ring (0 on the held coordinates tau, delta of a 4-D orbit)
    d_matrix (B, K, 6, 6)             d one-turn matrix / d knob
    d_dispersion (B, K, 4)            d dispersion / d knob
    d_orbit_along (B, K, E + 1, 6)    d orbit / d knob behind every item, index 0 the start (None without `along`): with order-0
                                      Multipole correctors as knobs, d_orbit_along[..., 0] is the orbit response matrix
    d_matrix_along (B, K, E + 1, 6, 6)   d cumulative matrix / d knob (None without `along`)
    d_tunes (B, K, 2)                 d eigen-tunes / d knob (`eigen_tunes`)
    d_beta (B, K, E + 1, 2)           d beta / d knob behind every item (`twiss_from_matrix`, `propagate_twiss`); without `along`
                                      (B, K, 2), the start values
    A seed whose search failed is NaN in its own rows. (Through `wrt=`, the gradient of a loss is NaN only if a failed seed's results
    enter it with a cotangent that is not zero.)"""
    closed: ClosedOrbit
    d_orbit: torch.Tensor
    d_matrix: torch.Tensor
    d_dispersion: torch.Tensor
    d_orbit_along: Optional[torch.Tensor]
    d_matrix_along: Optional[torch.Tensor]
    d_tunes: torch.Tensor
    d_beta: torch.Tensor


def _start_beta(M: torch.Tensor):
    """beta and alpha at the start from the diagonal blocks of M (..., 6, 6): two tensors (..., 2)."""
    ba = [twiss_from_matrix(_block(M, plane))[:2] for plane in range(2)]
    return torch.stack([b for b, _ in ba], -1), torch.stack([a for _, a in ba], -1)


def ring_sensitivity_from(closed: ClosedOrbit, sens: dict, matrix_along=None) -> RingSensitivity:
    """The `RingSensitivity` of the raw tangents of `chx_dkd_ring_sensitivity`: d_tunes and d_beta by forward-mode differentiation
    (`torch.func.jvp`) of the algebra above, every (seed, knob) a row of one batch. torch only."""
    M, dM = closed.matrix, sens["d_matrix"]
    B, K = dM.shape[:2]
    rows = M[:, None].expand(B, K, 6, 6).contiguous().view(B * K, 6, 6)     # (a copy: forward mode takes no overlapping primal)
    d_rows = dM.reshape(B * K, 6, 6)

    def tangent(f, primals, tangents):
        """The tangent of f, NaN where its value is (a seed that failed is NaN in its own rows, like the value)."""
        value, t = torch.func.jvp(f, primals, tangents)
        return torch.where(torch.isnan(value), value, t)

    if K == 0:
        d_tunes = dM.new_zeros((B, 0, 2))
        d_beta = dM.new_zeros((B, 0, 2) if matrix_along is None else (B, 0, matrix_along.shape[1], 2))
    else:
        d_tunes = tangent(lambda m: eigen_tunes(m[:, :4, :4])[0], (rows,), (d_rows,)).reshape(B, K, 2)
        if matrix_along is None:
            d_beta = tangent(lambda m: _start_beta(m)[0], (rows,), (d_rows,)).reshape(B, K, 2)
        else:
            E1 = matrix_along.shape[1]
            along = matrix_along[:, None].expand(B, K, E1, 6, 6).contiguous().view(B * K, E1, 6, 6)
            d_along = sens["d_matrix_along"].reshape(B * K, E1, 6, 6)
            d_beta = tangent(lambda m, a: _along(a, *_start_beta(m))[0], (rows, along), (d_rows, d_along)).reshape(B, K, E1, 2)
    return RingSensitivity(closed, sens["d_orbit"], dM, sens["d_dispersion"], sens.get("d_orbit_along"), sens.get("d_matrix_along"),
                           d_tunes, d_beta)


class RingValues(torch.autograd.Function):
    """The results of `chx_dkd_ring_jacobian` as functions of the settings in `wrt`: forward hands out the kernel's tensors as they are
    (the bits of a call without `wrt`) and keeps the tangents of `chx_dkd_ring_sensitivity`; backward contracts the cotangents with
    them (einsum, no kernel of this library) and hands every setting the entries of its knobs."""

    NAMES = (("orbit", "d_orbit", "bi,bki->k"), ("image", "d_image", "bi,bki->k"), ("matrix", "d_matrix", "bij,bkij->k"),
             ("dispersion", "d_dispersion", "bi,bki->k"), ("orbit_along", "d_orbit_along", "bei,bkei->k"),
             ("matrix_along", "d_matrix_along", "beij,bkeij->k"))

    @staticmethod
    def forward(ctx, out: dict, sens: dict, knobs, *wrt):
        ctx.set_materialize_grads(False)
        names = [n for n in RingValues.NAMES if n[0] in out and n[1] in sens]
        ctx.tangents = [(sens[d], rule) for _, d, rule in names]
        ctx.knobs = knobs                                     # per tensor of wrt: (first knob, count, 0-d?)
        ctx.like = [(t.dtype, t.shape) for t in wrt]
        return tuple(out[v] for v, _, _ in names)

    @staticmethod
    def backward(ctx, *grads):
        total = None
        for g, (tangent, rule) in zip(grads, ctx.tangents):
            if g is None:
                continue
            # a seed that failed has NaN tangents: it counts where its cotangent is not zero and nowhere else (a loss that never
            # touches a lost seed keeps finite gradients)
            lost = torch.isnan(tangent)
            part = torch.einsum(rule, g, torch.where(lost, torch.zeros_like(tangent), tangent))
            touched = torch.einsum(rule, (g != 0).to(tangent.dtype), lost.to(tangent.dtype)) > 0
            part = torch.where(touched, torch.full_like(part, float("nan")), part)
            total = part if total is None else total + part
        if total is None:
            return (None, None, None) + (None,) * len(ctx.like)
        per = [total[first].to(dtype) if scalar else total[first:first + count].to(dtype).reshape(shape)
               for (first, count, scalar), (dtype, shape) in zip(ctx.knobs, ctx.like)]
        return (None, None, None) + tuple(per)


def attach_gradients(out: dict, sens: dict, knobs, wrt, n_closed: int) -> dict:
    """`out` (the dict of `chx_dkd_ring_jacobian`'s tensors) with an autograd graph to the settings `wrt`: the same bits, `residual`
    recomputed from image and orbit so that it carries gradients too."""
    names = [v for v, d, _ in RingValues.NAMES if v in out and d in sens]
    res = dict(out)
    res.update(zip(names, RingValues.apply(out, sens, knobs, *wrt)))
    r = (res["image"] - res["orbit"])[:, :n_closed].abs().amax(-1)          # closing_error of the kernel, with a graph
    res["residual"] = out["residual"] + (r - r.detach())
    return res
