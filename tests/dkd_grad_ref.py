"""A gradient reference for the drift-kick-drift backward pass (chx_dkd_track_bwd) that shares no code with the kernel, and the
table of cases that tests/test_dkd_grad_ref_host.py (no GPU) and tests/test_gpu_dkd_grad_edges.py run. No GPU needed.

The loss is sum(W * x_out) over the six coordinates. Its gradient with respect to every element parameter, the reference energy
and the incoming particles:

  Drift, Quadrupole, Dipole, TDC   central differences D(h) of the float64 CPU oracle's forward pass (oracle.dkd_track) with one
                                   Richardson step: ref = (4 D(h/2) - D(h)) / 3, its own uncertainty u = |D(h/2) - D(h)|. For the
                                   particles one coordinate of ALL particles is moved at once (particles do not interact), so 6
                                   coordinates x 4 evaluations give the whole dx.
  Sextupole, RFCavity              the oracle does not know these kinds: float64 torch autograd on the CPU through the restated maps
                                   of tests/test_dkd_sextupole_host.py and tests/test_rfcavity_host.py (polynomials and sines without
                                   removable singularities; u = 0). The sextupole's tilt enters that map through numpy, so its
                                   derivative is the Richardson difference of the restated map.

Unlike the reference's autograd (NaN at k1 == 0: a complex square root at 0) the differences see the limit, which is the definition
of the gradient there.

Acceptance of a kernel gradient `got` (tests/test_gpu_dkd_grad_edges.py): |got - ref| <= 2e-7 |ref| + 4 u + floor; the host test
caps u <= 5e-8 |ref| + floor for every case, so the reference cannot hide a failure. With S = sum |W * x_out|:
  floor of a parameter    1e-9 S / scale, scale = max(|value|, UNIT of the parameter)   (UNIT: the table below. A value below its
                          UNIT, k1 = 1e-12 for one, keeps the UNIT: its own magnitude would make the floor useless)
  floor of the energy     1e-9 S / E
  floor of dx[n, j]       1e-9 (S / N) / SIG[j]: a particle's share of S over the beam size of the coordinate (the particle on the
                          axis has neither a magnitude nor a loss term of its own)
Steps: h = HREL * scale for a parameter (HREL below, chosen on the CPU so that the cap holds), H_ENERGY * (E - mc2), H_X * SIG[j]."""
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

M_E = 510998.95069
M_P = 938272089.4300001
SIG = np.array([3e-4, 5e-5, 3e-4, 5e-5, 2e-5, 1e-3])      # the beams' sizes, as tests/golden/nonlinear_grad.npz's

DRIFT, QUAD, DIPOLE, TDC, SEXT, RF = 0, 1, 2, 3, 5, 6    # _ops.DKD_KIND
KIND_NAME = {DRIFT: "drift", QUAD: "quadrupole", DIPOLE: "dipole", TDC: "tdc", SEXT: "sextupole", RF: "rfcavity"}
PNAMES = {
    DRIFT: ("length",),
    QUAD: ("length", "k1", "tilt", "mx", "my"),
    DIPOLE: ("length", "angle", "e1", "e2", "tilt", "fint", "fint_exit", "gap", "gap_exit"),
    TDC: ("length", "voltage", "phase", "frequency", "tilt", "mx", "my"),
    SEXT: ("length", "k2", "tilt", "mx", "my"),
    RF: ("length", "voltage", "phase", "frequency"),
}
# the unit scale of a parameter: what stands in for its magnitude where that is zero (or below it)
UNIT = {
    DRIFT: (0.1,),
    QUAD: (0.1, 1.0, 0.1, 1e-3, 1e-3),
    DIPOLE: (0.1, 0.1, 0.1, 0.1, 0.1, 0.5, 0.5, 0.05, 0.05),
    TDC: (0.1, 1e6, 0.1, 1e9, 0.1, 1e-3, 1e-3),
    SEXT: (0.1, 1.0, 0.1, 1e-3, 1e-3),
    RF: (0.1, 1e6, 0.1, 1e9),
}
# the relative step of the central differences, per parameter: small where the third derivative is large (a tilt, a phase), large
# where the oracle's rounding (1e-15 on a dipole's outgoing px: its angles are differences of numbers near pi / 2) sets the error
HREL = {
    DRIFT: (1e-3,),
    QUAD: (3e-5, 1e-4, 3e-5, 1e-3, 1e-3),
    DIPOLE: (3e-4, 2e-3, 5e-3, 1e-3, 2e-3, 3e-2, 3e-2, 3e-2, 3e-2),
    TDC: (3e-3, 3e-4, 1e-5, 1e-3, 1e-3, 2e-2, 2e-2),
    SEXT: (1e-4,) * 5,          # (the tilt alone: the other gradients of the Sextupole and the RFCavity are autograd's)
}
# ... of the reference energy, relative to the kinetic energy. Its gradient is tiny and the outgoing delta = (E - E_ref) / p0c carries
# 3e-16 of rounding, so the step is large — less so where the energy matters more (a cavity's 1 / p0c kick, a focusing strength)
H_ENERGY = {DRIFT: 1e-3, QUAD: 1e-4, DIPOLE: 1e-3, TDC: 5e-5}
# ... of the particles' coordinates, relative to the beam size (delta: the chromatic terms have the larger third derivative)
H_X = np.array([3e-2, 3e-2, 3e-2, 3e-2, 3e-2, 2e-3])
REGULAR = {
    DRIFT: ((0.8,), 1, 3),
    QUAD: ((0.3, 4.2, 0.3, 1e-3, -2e-3), 5, 3),
    DIPOLE: ((0.5, 0.2, 0.08, 0.05, 0.1, 0.5, 0.4, 0.05, 0.04), 1, 3),
    TDC: ((1.0, 1e7, 0.2, 1e9, 0.05, 2e-4, -1e-4), 1, 3),
    SEXT: ((0.2, 30.0, 0.2, 1e-3, -5e-4), 3, 3),
    RF: ((0.4, 2e6, 0.1, 480e6), 1, 3),
}


@dataclass(frozen=True)
class Case:
    name: str
    kind: int
    params: tuple
    num_steps: int = 1
    fringe_at: int = 3
    energy: float = 1e8
    mc2: float = M_E
    nq: float = -1.0
    N: int = 300                  # one full tile of 256 particles plus 44
    seed: int = 1
    h_energy: float = 0.0         # the energy's relative step where it is not H_ENERGY's
    hrel: tuple = ()              # ((parameter name, relative step), ...) where it is not HREL's
    steep_px: float = 0.0         # particles 3..8 get this px (the large-angle dipole: both branches of x2 in one beam)

    @property
    def P(self):
        return len(self.params)

    def scale(self, k):
        return max(abs(self.params[k]), UNIT[self.kind][k])

    def step(self, k):
        return dict(self.hrel).get(PNAMES[self.kind][k], HREL[self.kind][k]) * self.scale(k)

    def energy_step(self):
        return (self.h_energy or H_ENERGY[self.kind]) * (self.energy - self.mc2)


def _regular(name, kind, **kw):
    params, steps, fringe = REGULAR[kind]
    return Case(name, kind, params, num_steps=steps, fringe_at=fringe, **kw)


def _with(kind, **changes):
    p = list(REGULAR[kind][0])
    for key, v in changes.items():
        p[PNAMES[kind].index(key)] = v
    return tuple(p)


_Q0 = (0.3, 0.0, 0.0, 0.0, 0.0)
_LARGE = (1.0, 2.0, 0.1, 0.05, 0.0, 0.5, 0.5, 0.02, 0.02)
BRANCH_CASES = (
    # ---- Quadrupole, k1 near zero: the val(w) == 0 branch of quad_coefficients and its neighbourhood
    Case("quad_k1_0_n1", QUAD, _Q0, num_steps=1),
    Case("quad_k1_0_n3", QUAD, _Q0, num_steps=3),
    Case("quad_k1_0_tilt_misaligned", QUAD, (0.3, 0.0, 0.3, 1e-3, -2e-3), num_steps=2),
    Case("quad_k1_+1e-12", QUAD, (0.3, 1e-12, 0.0, 0.0, 0.0)),
    Case("quad_k1_-1e-12", QUAD, (0.3, -1e-12, 0.0, 0.0, 0.0)),
    Case("quad_k1_+1e-6", QUAD, (0.3, 1e-6, 0.0, 0.0, 0.0)),
    Case("quad_k1_-1e-6", QUAD, (0.3, -1e-6, 0.0, 0.0, 0.0)),
    # ---- protons of 62 MeV kinetic energy: beta0 = 0.35, pz = delta / beta0, and low_energy_z_correction changes its branch at
    # |pz| = 1.6e-3 — inside a beam with sigma_delta = 1e-3
    Case("quad_protons_low_energy", QUAD, (0.3, 2.0, 0.1, 0.0, 0.0), num_steps=2, energy=1e9, mc2=M_P, nq=1.0, h_energy=5e-5),
    # ---- Dipole, angle near zero (g = 0: sinc, cosc and sqrta2minusbdiva at their limits)
    Case("dipole_angle_0", DIPOLE, _with(DIPOLE, angle=0.0)),
    Case("dipole_angle_1e-9", DIPOLE, _with(DIPOLE, angle=1e-9)),
    # ---- Dipole, large angle: |angle + phi1| >= pi / 2 for all particles but 3..8, whose px = -+0.5 keeps them below
    Case("dipole_angle_+2", DIPOLE, _LARGE, steep_px=-0.5, hrel=(("angle", 3e-5),)),
    Case("dipole_angle_-2", DIPOLE, (1.0, -2.0) + _LARGE[2:], steep_px=0.5, hrel=(("angle", 3e-5),)),
    # ---- Dipole fringes
    Case("dipole_fringe_neither", DIPOLE, REGULAR[DIPOLE][0], fringe_at=0),
    Case("dipole_fringe_entrance", DIPOLE, REGULAR[DIPOLE][0], fringe_at=1),
    Case("dipole_fringe_exit", DIPOLE, REGULAR[DIPOLE][0], fringe_at=2),
    Case("dipole_fringe_both", DIPOLE, REGULAR[DIPOLE][0], fringe_at=3),
    Case("dipole_gap_0_fint_0", DIPOLE, _with(DIPOLE, fint=0.0, fint_exit=0.0, gap=0.0, gap_exit=0.0)),
    Case("dipole_gap_0", DIPOLE, _with(DIPOLE, gap=0.0, gap_exit=0.0)),
    Case("dipole_fint_0", DIPOLE, _with(DIPOLE, fint=0.0, fint_exit=0.0)),
    # ---- Drift
    Case("drift_length_0", DRIFT, (0.0,)),
    # ---- TDC
    Case("tdc_voltage_0", TDC, _with(TDC, voltage=0.0)),
    Case("tdc_voltage_0_upright", TDC, (1.0, 0.0, 0.2, 1e9, 0.0, 0.0, 0.0)),
    Case("tdc_phase_0", TDC, _with(TDC, phase=0.0)),
    Case("tdc_phase_0_upright", TDC, (1.0, 1e7, 0.0, 1e9, 0.0, 0.0, 0.0)),
    # ---- Sextupole
    Case("sextupole_k2_0_n1", SEXT, _with(SEXT, k2=0.0), num_steps=1),
    Case("sextupole_k2_0_n4", SEXT, _with(SEXT, k2=0.0), num_steps=4),
    # ---- RFCavity
    Case("rfcavity_voltage_0", RF, _with(RF, voltage=0.0)),
    Case("rfcavity_length_0", RF, _with(RF, length=0.0)),
    Case("rfcavity_phase_0", RF, _with(RF, phase=0.0)),
    Case("rfcavity_phase_0.25", RF, _with(RF, phase=0.25)),
    Case("rfcavity_phase_0.5", RF, _with(RF, phase=0.5)),
)
TILE_SIZES = (1, 64, 255, 256, 257, 513)
TILE_CASES = tuple(_regular(f"{KIND_NAME[k]}_N{n}", k, N=n, seed=2) for k in (DRIFT, QUAD, DIPOLE, TDC, SEXT, RF) for n in TILE_SIZES)
CASES = {c.name: c for c in BRANCH_CASES + TILE_CASES}
assert len(CASES) == len(BRANCH_CASES) + len(TILE_CASES)


def beam(case):
    """(x (N, 7), W (N, 7)) float64. From three particles on: particle 0 on the axis, particle 1 with delta = 0, particle 2
    with px = py = 0."""
    rng = np.random.default_rng(case.seed)
    x = np.ones((case.N, 7))
    x[:, :6] = rng.standard_normal((case.N, 6)) * SIG
    W = rng.standard_normal((case.N, 7))
    if case.N >= 3:
        x[0, :6] = 0.0
        x[1, 5] = 0.0
        x[2, 1] = x[2, 3] = 0.0
    if case.steep_px:
        x[3:9, 1] = case.steep_px
    return x, W


def _oracle():
    from oracle import chx_oracle

    chx_oracle.build()
    return chx_oracle


def _restated(case, x, p, E):
    """(x_out, ref_energy) of the restated torch maps; x, E and the entries of p are float64 tensors (tilt: a float)."""
    if case.kind == SEXT:
        from tests.test_dkd_sextupole_host import restated_map

        return restated_map(x, E, torch.tensor(case.mc2, dtype=torch.float64), p[0], p[1], p[2], p[3], p[4], case.num_steps)
    from tests.test_rfcavity_host import restated_map

    return restated_map(x, E, torch.tensor(case.mc2, dtype=torch.float64), case.nq, p[0], p[1], p[2], p[3])


def forward(case, x, params, energy):
    """x_out (N, 7) float64 of the independent forward pass: the oracle (kinds 0 - 3) or the restated map."""
    if case.kind in (SEXT, RF):
        t = lambda v: torch.tensor(float(v), dtype=torch.float64)  # noqa: E731
        p = [t(v) for v in params]
        if case.kind == SEXT:
            p[2] = float(params[2])
        with torch.no_grad():
            return _restated(case, torch.from_numpy(np.ascontiguousarray(x)), p, t(energy))[0].numpy()
    out, _ = _oracle().dkd_track(case.kind, x[None], np.asarray(params, dtype=np.float64)[None], np.float64(energy), case.mc2, case.nq,
                                 case.num_steps, case.fringe_at)
    return out[0]


def _richardson(f, h):
    """(ref, D(h / 2) - D(h)) of the derivative of the array-valued f at 0: central differences at h and h / 2, one Richardson step."""
    d1 = (f(h) - f(-h)) / (2.0 * h)
    d2 = (f(0.5 * h) - f(-0.5 * h)) / h
    return (4.0 * d2 - d1) / 3.0, d2 - d1


@dataclass
class Reference:
    out: np.ndarray       # x_out (N, 7)
    S: float              # sum |W x_out| over the six coordinates
    dp: np.ndarray        # (P,)
    u_p: np.ndarray
    de: float
    u_e: float
    dx: np.ndarray        # (N, 6)
    u_x: np.ndarray
    floor_p: np.ndarray
    floor_e: float
    floor_x: np.ndarray   # (6,)


def reference_for(case, x, W):
    """The gradients of sum(W * x_out) for this case's element on the beam x, with their uncertainties and floors."""
    params = np.asarray(case.params, dtype=np.float64)
    W6 = W[:, :6]
    out = forward(case, x, params, case.energy)
    S = float(np.abs(W6 * out[:, :6]).sum())
    P = case.P
    dp, u_p, dx, u_x = np.zeros(P), np.zeros(P), np.zeros((case.N, 6)), np.zeros((case.N, 6))

    def loss_terms(xx, pp, ee):      # per particle, differences are taken before anything is summed
        return (W6 * forward(case, xx, pp, ee)[:, :6]).sum(axis=1)

    def fd_param(k):
        def f(h):
            pp = params.copy()
            pp[k] += h
            return loss_terms(x, pp, case.energy)

        ref, diff = _richardson(f, case.step(k))
        return float(ref.sum()), abs(float(diff.sum()))

    if case.kind in (SEXT, RF):
        xt = torch.from_numpy(x.copy()).requires_grad_(True)
        pt = [torch.tensor(float(v), dtype=torch.float64, requires_grad=True) for v in params]
        et = torch.tensor(float(case.energy), dtype=torch.float64, requires_grad=True)
        pin = list(pt)
        if case.kind == SEXT:
            pin[2] = float(params[2])
        got = _restated(case, xt, pin, et)[0]
        (got[:, :6] * torch.from_numpy(W6)).sum().backward()
        for k in range(P):
            if case.kind == SEXT and k == 2:
                dp[k], u_p[k] = fd_param(k)
            else:
                dp[k] = 0.0 if pt[k].grad is None else float(pt[k].grad)
        de, u_e = (0.0 if et.grad is None else float(et.grad)), 0.0
        dx = xt.grad.numpy()[:, :6].copy()
    else:
        for k in range(P):
            dp[k], u_p[k] = fd_param(k)
        r, diff = _richardson(lambda h: loss_terms(x, params, case.energy + h), case.energy_step())
        de, u_e = float(r.sum()), abs(float(diff.sum()))
        for j in range(6):
            def f(h, j=j):
                xx = x.copy()
                xx[:, j] += h
                return loss_terms(xx, params, case.energy)

            dx[:, j], diff = _richardson(f, H_X[j] * SIG[j])
            u_x[:, j] = np.abs(diff)
    floor_p = np.array([1e-9 * S / case.scale(k) for k in range(P)])
    return Reference(out, S, dp, u_p, de, u_e, dx, u_x, floor_p, 1e-9 * S / case.energy, 1e-9 * (S / case.N) / SIG)


@functools.lru_cache(maxsize=None)
def reference(name):
    """`reference_for` the case `name` on its own beam, computed once per process and shared. Treat it as read-only."""
    case = CASES[name]
    x, W = beam(case)
    return reference_for(case, x, W)


def low_energy_evaluation(case, x):
    """(evaluation, threshold) of low_energy_z_correction (bmadx.py:184-216) per particle: the series is used below the threshold."""
    p0c = math.sqrt(case.energy ** 2 - case.mc2 ** 2)
    en = case.energy + x[:, 5] * p0c
    pz = (np.sqrt(en ** 2 - case.mc2 ** 2) - p0c) / p0c
    beta0 = p0c / case.energy
    return case.mc2 * (beta0 * pz) ** 2, 3e-7 * case.energy


def dipole_branch_angle(case, x):
    """angle + phi1 per particle at the entrance of the dipole body (dipole.py:246-336; after tilt and entrance fringe)."""
    L, angle, e1, _, tilt = case.params[:5]
    s, c = math.sin(tilt), math.cos(tilt)
    X, px, py = x[:, 0] * c + x[:, 2] * s, x[:, 1] * c + x[:, 3] * s, -x[:, 1] * s + x[:, 3] * c
    if case.fringe_at & 1:
        px = px + X * (angle / L) * math.tan(e1)
    p0c = math.sqrt(case.energy ** 2 - case.mc2 ** 2)
    en = case.energy + x[:, 5] * p0c
    pz = (np.sqrt(en ** 2 - case.mc2 ** 2) - p0c) / p0c
    return angle + np.arcsin(px / np.sqrt((1 + pz) ** 2 - py ** 2))       # (py's fringe kick is of second order here)
