"""Segment.one_turn_map, closed_orbit, ring_optics and chromaticity on the GPU (chx_dkd_ring_jacobian).

 1. matrix against six backward passes through `track` (the per-element Jacobians multiplied in the other order): 1e-9 max(1, |M|).
 2. matrix against Richardson-extrapolated central differences of float64 `Segment.track` (no code shared with the dual numbers):
    1e-8 max(1, |M|), the reference's own error estimate below a tenth of that.
 3. symplecticity of the one-turn and of every cumulative matrix against the six-backward-pass matrix's.
 4. the per-item records against the one-turn results, bit for bit.
 5. the closed orbit of one corrector against `track` and against theta beta cot(pi Q) / 2.
 6. off-momentum orbits against the dispersion; slip and dispersion against the hand computation of tests/test_gpu_rfcavity.py.
 7. tunes and chromaticity against `track_turns` + `TurnByTurn.tunes`.
 8. rotation of the element list, periodicity.
 9. a Drift / Quadrupole ring against the product of the linear maps (chx_build).
10. B at the edges of the layout — a seed is 8 lanes, a workgroup is one wave of 8 seeds: 1, 7, 8, 9 (a workgroup's edge), 65, 257 (more
    workgroups, a ragged last one); E = 1, 2, 192, 193; a linear element; a float32 ring.
11. NaN isolation, an unstable plane, a 6-D search without RF, determinism, graph capture.

The rings are the 48-item ring of tests/test_gpu_rfcavity.py (`small_ring`) and variations of it; B <= 257."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_dkd_sextupole import S as SYMPLECTIC_S  # (the matrix diag(J2, J2, -J2) only)
from tests.test_gpu_track_turns import same_bits  # (helper only)

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
DKD = {"tracking_method": "drift_kick_drift"}
CELLS, ENERGY, M_E = 6, 1e8, 510998.95069
TWO_PI = 2 * math.pi


def _kw(dt=F64):
    return {"dtype": dt, "device": "cuda"}


def T(v, dt=F64):
    return torch.tensor(v, **_kw(dt))


def electron(dt=F64):
    import cheetah_amd as ca

    return ca.Species("electron", **_kw(dt))


def make_ring(kf=3.0, kd=-3.0, voltage=None, sextupoles=False, multipoles=False, corrector=None, dt=F64, kd_last=None, widen=False,
              bends=True):
    """The ring of tests/test_gpu_rfcavity.py::small_ring — six cells [QF, D, B, D, QD, D, B, D] of 2.6 m with sector bends of 30
    degrees, 48 items —, with the first Drift an RFCavity on harmonic 400 when `voltage` is given, the Drift behind every QF a
    Sextupole and the Drift behind every QD a tilted, shifted order-3 Multipole on request, and a zero-length order-0 Multipole of
    knl = -corrector in front of everything (one item more). `widen`: a float64 ring of the float32 ring's setting values.
    `bends=False`: Drifts of the bends' length in their place (a periodic channel: one "turn" is one pass)."""
    import cheetah_amd as ca

    kw = _kw(F64 if widen else dt)
    t = (lambda v: T(v, F32).to(F64)) if widen else (lambda v: T(v, dt))  # noqa: E731
    els = []
    if corrector is not None:
        els.append(ca.Multipole(t(0.0), order=0, knl=t(-corrector), name="corrector", **DKD, **kw))
    for c in range(CELLS):
        for j, kind in enumerate("qdbdQdbd"):
            name = f"c{c}_{j}"
            if kind == "d" and c == 0 and j == 1 and voltage is not None:
                f = ca.RFCavity.harmonic_frequency(CELLS * 2.6, 400, T(ENERGY)).to(dt)
                els.append(ca.RFCavity(t(0.3), voltage=t(voltage), phase=t(0.0), frequency=f, name="rf", **kw))
            elif kind == "d" and j == 1 and sextupoles:
                els.append(ca.Sextupole(t(0.3), k2=t(20.0 if c % 2 == 0 else -30.0), num_steps=2, name=name, **DKD, **kw))
            elif kind == "d" and j == 5 and multipoles:
                els.append(ca.Multipole(t(0.3), order=3, knl=t(400.0), ksl=t(-150.0), tilt=t(0.2), misalignment=t([3e-4, -2e-4]), num_steps=2,
                                        name=name, **DKD, **kw))
            elif kind == "d":
                els.append(ca.Drift(t(0.3), name=name, **DKD, **kw))
            elif kind == "b" and not bends:
                els.append(ca.Drift(t(0.5), name=name, **DKD, **kw))
            elif kind == "b":
                els.append(ca.Dipole(t(0.5), angle=t(2 * math.pi / (2 * CELLS)), name=name, **DKD, **kw))
            else:
                k1 = kf if kind == "q" else (kd_last if (kd_last is not None and c == CELLS - 1) else kd)
                els.append(ca.Quadrupole(t(0.2), k1=t(k1), num_steps=1, name=name, **DKD, **kw))
    return ca.Segment(els)


def single_element(name):
    import cheetah_amd as ca

    kw = _kw()
    return ca.Segment([{
        "drift": lambda: ca.Drift(T(0.7), **DKD, **kw),
        "quadrupole": lambda: ca.Quadrupole(T(0.3), k1=T(4.2), tilt=T(0.3), misalignment=T([1e-3, -2e-3]), num_steps=3, **DKD, **kw),
        "dipole": lambda: ca.Dipole(T(0.5), angle=T(0.4), dipole_e1=T(0.1), dipole_e2=T(-0.05), tilt=T(0.2), fringe_integral=T(0.5),
                                    gap=T(0.03), **DKD, **kw),
        "sextupole": lambda: ca.Sextupole(T(0.2), k2=T(100.0), tilt=T(0.3), misalignment=T([1e-3, -5e-4]), num_steps=3, **DKD, **kw),
        "rfcavity": lambda: ca.RFCavity(T(0.3), voltage=T(1e6), phase=T(0.13), frequency=T(480e6), **kw),
        "multipole": lambda: ca.Multipole(T(0.2), order=3, knl=T(500.0), ksl=T(-200.0), tilt=T(0.3), misalignment=T([1e-3, -5e-4]), num_steps=2,
                                          **DKD, **kw),
    }[name]()])


RINGS = {
    "rf": lambda: make_ring(voltage=5e4),
    "sext_mp": lambda: make_ring(sextupoles=True, multipoles=True),
    "sext_mp_straight": lambda: make_ring(sextupoles=True, multipoles=True, bends=False),
    "bend": lambda: make_ring(),
    **{k: functools.partial(single_element, k) for k in ("drift", "quadrupole", "dipole", "sextupole", "rfcavity", "multipole")},
}
MATRIX_CASES = ["rf", "sext_mp", "sext_mp_straight", "drift", "quadrupole", "dipole", "sextupole", "rfcavity", "multipole"]


def seeds():
    """The origin and four drawn points of 5e-3 scale in x and y (the beam of the symplecticity tests), (5, 6) float64 on the device."""
    g = torch.Generator().manual_seed(21)
    x = torch.randn(4, 6, generator=g, dtype=F64) * torch.tensor([5e-3, 2e-5, 5e-3, 2e-5, 1e-4, 2e-3], dtype=F64)
    return torch.cat([torch.zeros(1, 6, dtype=F64), x]).cuda()


def rows7(x6):
    return torch.cat([x6, torch.ones_like(x6[:, :1])], dim=1)


def beam_of(x6):
    import cheetah_amd as ca

    return ca.ParticleBeam(rows7(x6), T(ENERGY), species=electron())


@functools.lru_cache(maxsize=None)
def ring(name):
    return RINGS[name]()


@functools.lru_cache(maxsize=None)
def six_pass_jacobian(name):
    """(5, 6, 6) numpy: the Jacobian of one turn at `seeds()` from six backward passes through `track`. Computed once, read-only."""
    rows = []
    for i in range(6):
        p = rows7(seeds()).requires_grad_(True)
        import cheetah_amd as ca

        out = ring(name).track(ca.ParticleBeam(p, T(ENERGY), species=electron()))
        out.particles[:, i].sum().backward()
        rows.append(p.grad[:, :6].cpu().numpy())
    J = np.stack(rows, axis=1)
    J.setflags(write=False)
    return J


@functools.lru_cache(maxsize=None)
def one_turn(name, along=False):
    return ring(name).one_turn_map(seeds(), T(ENERGY), along=along)


def symplectic_residual(M):
    return max(np.abs(m.T @ SYMPLECTIC_S @ m - SYMPLECTIC_S).max() for m in M.reshape(-1, 6, 6))


# ---- 1. six backward passes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MATRIX_CASES)
def test_matrix_matches_six_backward_passes(name):
    got = one_turn(name)
    M, J = got.matrix.cpu().numpy(), six_pass_jacobian(name)
    assert M.shape == (5, 6, 6) and got.matrix.dtype == F64 and got.end.shape == (5, 7) and (got.end[:, 6] == 1).all()
    want = ring(name).track(beam_of(seeds())).particles
    assert np.abs((got.end - want).cpu().numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))   # (the value path is `track`'s)
    assert same_bits(got.start[:, :6], seeds())
    for b in range(5):
        bound = 1e-9 * max(1.0, np.abs(J[b]).max())
        err = np.abs(M[b] - J[b]).max()
        print(name, "seed", b, "max |M|", np.abs(J[b]).max(), "error / bound", err / bound)
        assert err <= bound, (name, b, err / bound)


# ---- 2. differences -----------------------------------------------------------------------------------------------------------------------
#: the steps of tests/dkd_grad_ref.py (H_X * SIG: a few per cent of a beam size per coordinate, 2e-3 of it for delta) ...
DIFF_STEPS = np.array([3e-2, 3e-2, 3e-2, 3e-2, 3e-2, 2e-3]) * np.array([3e-4, 5e-5, 3e-4, 5e-5, 2e-5, 1e-3])
#: ... and a quarter of them where octupoles and sextupoles give the plain difference a large third derivative (a kick of
#: knl = 500 m^-3: h^2 knl / 8 = 5e-9 at h = 9e-6, half the bound). Measured per column on an MI355X, estimate / bound:
#:   the RF ring        full steps 0.01 .. 0.06, half steps up to 0.23, quarter steps up to 0.37: ROUNDING — every Dipole leaves
#:                      1e-15 in px (its angles are differences of numbers near pi / 2: tests/dkd_grad_ref.py says the same of the
#:                      oracle), twelve of them at beta of 5 m over a step of 1.5e-6 are 0.05 of the bound;
#:   the ring with Sextupoles and Multipoles AND bends   x and y columns 0.39 and 1.36 at full steps (truncation), 0.02 and 0.09 at a
#:                      quarter; px, py and delta columns 0.06 .. 0.27 at full steps and never below 0.08 at any: no step keeps both
#:                      errors under the cap, so the DIFFERENCE test takes that ring without its bends (Drifts of their length: no
#:                      such rounding; a tenth of the steps: 0.18 at a quarter), and the six-backward-pass test takes both.
DIFF_SCALE = {"sext_mp_straight": 0.1, "sextupole": 0.25, "multipole": 0.25}
DIFF_CASES = [c for c in MATRIX_CASES if c != "sext_mp"]


def difference_jacobian(r, x0, scale=1.0):
    """(ref, estimate), both (B, 6, 6): central differences of float64 `Segment.track` at h and h / 2 with one Richardson step,
    `tests/dkd_grad_ref.py::_richardson` — every displaced copy of every seed in ONE beam."""
    B = x0.shape[0]
    rows, index = [], {}
    for j in range(6):
        for f in (1.0, -1.0, 0.5, -0.5):
            x = x0.clone()
            x[:, j] += f * scale * DIFF_STEPS[j]
            index[(j, f)] = len(rows)
            rows.append(x)
    out = r.track(beam_of(torch.cat(rows))).particles[:, :6].cpu().numpy().reshape(len(rows), B, 6)
    ref, est = np.zeros((B, 6, 6)), np.zeros((B, 6, 6))
    for j in range(6):
        h = scale * DIFF_STEPS[j]
        d1 = (out[index[(j, 1.0)]] - out[index[(j, -1.0)]]) / (2.0 * h)
        d2 = (out[index[(j, 0.5)]] - out[index[(j, -0.5)]]) / h
        ref[:, :, j] = (4.0 * d2 - d1) / 3.0
        est[:, :, j] = d2 - d1
    return ref, est


@pytest.mark.parametrize("name", DIFF_CASES)
def test_matrix_matches_differences_of_track(name):
    M = one_turn(name).matrix.cpu().numpy()
    ref, est = difference_jacobian(ring(name), seeds(), DIFF_SCALE.get(name, 1.0))
    for b in range(5):
        bound = 1e-8 * max(1.0, np.abs(ref[b]).max())
        u, err = np.abs(est[b]).max(), np.abs(M[b] - ref[b]).max()
        print(name, "seed", b, "max |M|", np.abs(ref[b]).max(), "reference's estimate / bound", u / bound, "error / bound", err / bound)
        assert u <= 0.1 * bound, (name, b, u / bound)            # the reference cannot hide a failure
        assert err <= bound, (name, b, err / bound)


# ---- 3. symplecticity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rf", "sext_mp"])
def test_one_turn_and_cumulative_matrices_are_symplectic(name):
    got = one_turn(name, along=True)
    r_ref = symplectic_residual(six_pass_jacobian(name)[1:])
    r_turn = symplectic_residual(got.matrix[1:].cpu().numpy())
    r_along = symplectic_residual(got.matrix_along[1:].cpu().numpy())
    print(name, "residual: six backward passes", r_ref, "one turn", r_turn, "cumulative (largest)", r_along)
    assert r_ref < 1e-9
    assert r_turn <= max(10 * r_ref, 1e-12)
    assert r_along <= max(10 * r_ref, 1e-12)


# ---- 4. along ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rf", "sext_mp", "drift"])
def test_records_along_the_ring_end_in_the_one_turn_results(name):
    got, plain = one_turn(name, along=True), one_turn(name)
    E = len(ring(name).elements)
    assert got.matrix_along.shape == (5, E + 1, 6, 6) and got.orbit_along.shape == (5, E + 1, 7) and got.s.shape == (E + 1,)
    assert same_bits(got.matrix_along[:, E], got.matrix) and same_bits(got.orbit_along[:, E], got.end)
    assert same_bits(got.matrix, plain.matrix) and same_bits(got.end, plain.end)
    assert same_bits(got.matrix_along[:, 0], torch.eye(6, **_kw()).expand(5, 6, 6).contiguous())
    assert same_bits(got.orbit_along[:, 0], got.start)
    out = ring(name).track(beam_of(seeds()))
    assert got.s.dtype == F64 and float(got.s[0]) == 0.0 and same_bits(got.s[-1], out.s)
    # behind item k: `track` of the first k items
    import cheetah_amd as ca

    k = min(17, E)
    part = ca.Segment([e.clone() for e in ring(name).elements[:k]]).track(beam_of(seeds()))
    assert np.abs((got.orbit_along[:, k] - part.particles).cpu().numpy()).max() <= 1e-12 * float(part.particles.abs().max())
    assert same_bits(got.s[k], part.s)


# ---- 5. corrector ---------------------------------------------------------------------------------------------------------------------------
THETA = 1e-4


@pytest.mark.parametrize("bends", [False, True])
def test_closed_orbit_of_one_corrector(bends):
    """Measured on an MI355X (the figures are printed): without bends — Drifts and Quadrupoles, whose departure from the linear
    map at delta = 0 is the exact drifts' px^2 / 2 = 5e-9 — x at the corrector equals theta beta cot(pi Q) / 2 within 1e-6. WITH the
    sector bends of the ring (rho = 0.955 m) the same comparison is off by 1.6e-4 of x: a sector bend's exact map departs from its
    linear part at the relative order x / rho, and x / rho = 1.8e-4 here. There the formula is held to max |x| / rho over the ring
    (2.1e-4). Measured without / with bends: closing error of `track` on the orbit and `residual`, both 2.6e-6 / 0.047 of the
    1e-10 max |orbit| bound; the formula 2.4e-8 / 1.6e-4; the orbit from a guess 1e-3 away differs by 1.4e-19 / 6.3e-16 m."""
    kicked, bare = make_ring(corrector=THETA, bends=bends), make_ring(corrector=0.0, bends=bends)
    co = kicked.closed_orbit(T(ENERGY))
    assert co.orbit.shape == (1, 7) and co.residual.shape == (1,) and co.matrix.shape == (1, 6, 6) and co.dispersion.shape == (1, 4)
    orbit = co.orbit[0, :6].cpu().numpy()
    assert abs(orbit[0]) > 1e-5                                                             # zero is not a solution
    assert orbit[4] == 0.0 and orbit[5] == 0.0 and float(co.orbit[0, 6]) == 1.0            # tau and delta are held
    back = kicked.track(beam_of(co.orbit[:, :6])).particles[0, :6].cpu().numpy()
    bound = 1e-10 * np.abs(orbit).max()
    closing = np.abs(back[:4] - orbit[:4]).max()
    print("corrector, bends", bends, ": orbit", orbit, "closing error of track / bound", closing / bound, "residual / bound", float(co.residual) / bound)
    assert closing <= bound
    assert float(co.residual) <= bound
    opt = bare.ring_optics(T(ENERGY))
    beta, Q = float(opt.beta[0, 0, 0]), float(opt.phase_advance[0, -1, 0]) / TWO_PI
    want = THETA * beta / (2.0 * math.tan(math.pi * Q))
    x_max = float(kicked.ring_optics(T(ENERGY)).orbit_along[0, :, 0].abs().max())
    formula_bound = x_max / (0.5 / (TWO_PI / 12)) if bends else 1e-6
    print("corrector, bends", bends, ": beta", beta, "Q", Q, "x", orbit[0], "theta beta cot(pi Q) / 2", want, "relative difference",
          abs(orbit[0] - want) / abs(want), "bound", formula_bound)
    assert abs(orbit[0] - want) <= formula_bound * abs(want)
    guess = co.orbit[:, :6].clone()
    guess[0, :4] += torch.tensor([1e-3, -1e-3 / 5, -1e-3, 1e-3 / 5], **_kw())               # 1e-3 away (px, py: over beta of a few metres)
    far = kicked.closed_orbit(T(ENERGY), guess=guess)
    print("corrector: from a guess 1e-3 away, difference", float((far.orbit - co.orbit).abs().max()))
    assert float((far.orbit - co.orbit).abs().max()) <= bound
    assert float(far.residual) <= bound


# ---- 6. off-momentum ------------------------------------------------------------------------------------------------------------------------
def test_off_momentum_orbits_follow_the_dispersion():
    r = ring("bend")
    d = 1e-3
    co = r.closed_orbit(T(ENERGY), delta=T([-d, 0.0, d]))
    assert co.orbit.shape == (3, 7) and same_bits(co.orbit[:, 5], T([-d, 0.0, d]))
    orbit, eta = co.orbit[:, :4].cpu().numpy(), co.dispersion.cpu().numpy()
    assert float(co.residual.max()) <= 1e-10 * np.abs(orbit).max()
    assert np.abs(orbit[1]).max() <= 1e-13                                                   # the axis is the orbit of delta = 0
    symmetric = (orbit[2] - orbit[0]) / (2 * d)
    one_sided = (orbit[2] - orbit[1]) / d
    scale = np.abs(eta[1]).max()
    print("dispersion", eta[1], "symmetric difference off by", np.abs(symmetric - eta[1]).max() / scale, "one-sided by",
          np.abs(one_sided - eta[1]).max() / scale)
    assert scale > 0.1                                                                       # (metres: the bends do disperse)
    assert np.abs(symmetric - eta[1]).max() <= 1e-5 * scale
    assert np.abs(one_sided - eta[1]).max() <= 1e-1 * scale                                  # (first order in delta: a sanity check only)
    # slip and dispersion: the hand computation of tests/test_gpu_rfcavity.py from the same matrix
    opt = r.ring_optics(T(ENERGY), delta=T([-d, 0.0, d]))
    for b in range(3):
        J = opt.matrix[b].cpu().numpy()
        eta_hand = np.linalg.solve(np.eye(4) - J[:4, :4], J[:4, 5])
        slip_hand = J[4, 5] + J[4, :4] @ eta_hand
        assert np.abs(opt.dispersion[b].cpu().numpy() - eta_hand).max() <= 1e-12 * np.abs(eta_hand).max()
        assert abs(float(opt.slip[b]) - slip_hand) <= 1e-12 * abs(slip_hand)
        assert np.abs(opt.dispersion_along[b, 0].cpu().numpy() - eta_hand).max() <= 1e-12 * np.abs(eta_hand).max()
        assert np.abs(opt.dispersion_along[b, -1].cpu().numpy() - eta_hand).max() <= 1e-9 * np.abs(eta_hand).max()    # periodic
    assert float(opt.slip[1]) > 0                                                            # above transition (the RF test's a0 > 0)


# ---- 7. tunes against tracking --------------------------------------------------------------------------------------------------------------
#: a working point with both fractional tunes in (0.05, 0.45): about (2.28, 0.27) from the linear matrices of the cell
KF, KD = 5.0, -3.25


def test_tunes_and_chromaticity_match_tracking():
    import cheetah_amd as ca

    r = make_ring(kf=KF, kd=KD)
    d = 1e-3
    delta = T([-d, 0.0, d])
    opt = r.ring_optics(T(ENERGY), delta=delta)
    assert opt.stable.all() and opt.tunes.shape == (3, 2)
    tunes = opt.tunes.cpu().numpy()
    assert ((tunes > 0.05) & (tunes < 0.45)).all(), tunes
    start = opt.orbit.clone()
    start[:, 0] += 1e-6
    start[:, 2] += 1e-6
    tbt = r.track_turns(ca.ParticleBeam(start, T(ENERGY), species=electron()), 1024, record_first=3, fused=True)
    assert not tbt.lost_turn.any()
    tracked = tbt.tunes(planes=("x", "y")).tune.cpu().numpy().reshape(3, 2)
    print("tunes from the matrix", tunes.tolist(), "from 1024 turns", tracked.tolist(), "largest difference", np.abs(tunes - tracked).max())
    assert np.abs(tunes - tracked).max() <= 1e-7
    full = (opt.phase_advance[:, -1] / TWO_PI).cpu().numpy()
    assert np.abs((full % 1.0) - tunes).max() <= 1e-9 and (full[:, 0] > 2).all() and (full[:, 1] < 1).all()      # the integer parts
    xi = r.chromaticity(T(ENERGY), h=d)
    assert xi.shape == (2,) and xi.dtype == F64
    xi_tracked = (tracked[2] - tracked[0]) / (2 * d)
    print("chromaticity", xi.tolist(), "from tracking", xi_tracked.tolist())
    assert np.abs(xi.cpu().numpy() - xi_tracked).max() <= 1e-4
    assert (xi < 0).all()                                                                     # the natural chromaticity


# ---- 8. rotation --------------------------------------------------------------------------------------------------------------------------
def test_rotating_the_element_list_moves_the_start():
    import cheetah_amd as ca

    r = ring("bend")
    opt = r.ring_optics(T(ENERGY))
    E = len(r.elements)
    assert opt.beta.shape == (1, E + 1, 2) and opt.alpha.shape == (1, E + 1, 2) and opt.phase_advance.shape == (1, E + 1, 2)
    rel = lambda a, b: float(((a - b).abs() / b.abs().clamp_min(1.0)).max())  # noqa: E731
    assert rel(opt.beta[:, E], opt.beta[:, 0]) <= 1e-9 and rel(opt.alpha[:, E], opt.alpha[:, 0]) <= 1e-9          # periodicity
    for k in (1, 17):
        rot = ca.Segment([e.clone() for e in r.elements[k:] + r.elements[:k]]).ring_optics(T(ENERGY))
        print("start at item", k, "beta", rot.beta[0, 0].tolist(), opt.beta[0, k].tolist(), "tunes", rot.tunes.tolist(), opt.tunes.tolist())
        assert rel(rot.beta[:, 0], opt.beta[:, k]) <= 1e-9
        assert rel(rot.alpha[:, 0], opt.alpha[:, k]) <= 1e-9
        assert float((rot.tunes - opt.tunes).abs().max()) <= 1e-12
        assert float((rot.s[-1] - opt.s[-1]).abs()) <= 1e-12 * float(opt.s[-1])


# ---- 9. linear ----------------------------------------------------------------------------------------------------------------------------
def test_drift_quadrupole_ring_matches_the_linear_maps():
    import cheetah_amd as ca

    kw = _kw()
    spec = [("q", 0.2, 2.0), ("d", 0.7, 0.0), ("q", 0.3, -1.8), ("d", 1.1, 0.0), ("q", 0.25, 1.1), ("d", 0.4, 0.0)]

    def build(method):
        return [ca.Quadrupole(T(L), k1=T(k), tracking_method=method, **kw) if kind == "q" else ca.Drift(T(L), tracking_method=method, **kw)
                for kind, L, k in spec]

    M = ca.Segment(build("drift_kick_drift")).one_turn_map(torch.zeros(1, 6, **kw), T(ENERGY)).matrix[0].cpu().numpy()
    R = np.eye(7)
    for el in build("linear"):
        R = el.first_order_transfer_map(T(ENERGY), electron())[..., :, :].reshape(7, 7).cpu().numpy() @ R
    err = np.abs(M[:4, :4] - R[:4, :4]).max() / np.abs(R[:4, :4]).max()
    print("linear check: max |M|", np.abs(R[:4, :4]).max(), "relative difference", err)
    assert err <= 1e-12


# ---- 10. shapes and edges -----------------------------------------------------------------------------------------------------------------
def many_seeds(B):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, 6, generator=g, dtype=F64) * torch.tensor([1e-3, 2e-5, 1e-3, 2e-5, 1e-4, 1e-3], dtype=F64)
    return x.cuda()


FIELDS = ("orbit", "residual", "matrix", "dispersion", "tunes", "beta", "alpha", "phase_advance", "slip", "dispersion_along", "orbit_along")


@pytest.mark.parametrize("B", [1, 7, 8, 9, 65, 257])
def test_every_seed_equals_its_single_seed_result(B):
    r = ring("sext_mp")
    guess = many_seeds(257)[:B]
    opt = r.ring_optics(T(ENERGY), guess=guess, delta=guess[:, 5].clone(), num_iterations=4)
    assert opt.orbit.shape == (B, 7) and opt.matrix.shape == (B, 6, 6) and torch.isfinite(opt.matrix).all()
    for b in sorted({0, B // 2, B - 1}):
        one = r.ring_optics(T(ENERGY), guess=guess[b], delta=guess[b, 5].clone(), num_iterations=4)
        for f in FIELDS:
            assert same_bits(getattr(opt, f)[b:b + 1], getattr(one, f)), (B, b, f)
    mp = r.one_turn_map(guess, T(ENERGY))
    assert same_bits(mp.matrix[B - 1:], r.one_turn_map(guess[B - 1], T(ENERGY)).matrix)


@pytest.mark.parametrize("E", [1, 2, 192])
def test_item_counts(E):
    import cheetah_amd as ca

    kw = _kw()
    els = [ca.Quadrupole(T(0.05), k1=T(1.5 if k % 4 == 0 else -1.5), num_steps=1, name=f"e{k}", **DKD, **kw) if k % 2 == 0
           else ca.Drift(T(0.1), name=f"e{k}", **DKD, **kw) for k in range(E)]
    seg = ca.Segment(els)
    x = many_seeds(9)
    got = seg.one_turn_map(x, T(ENERGY), along=True)
    assert got.matrix_along.shape == (9, E + 1, 6, 6) and same_bits(got.matrix_along[:, E], got.matrix)
    want = seg.track(beam_of(x))
    assert np.abs((got.end - want.particles).cpu().numpy()).max() <= 1e-12 * float(want.particles.abs().max())
    assert same_bits(got.s[-1], want.s)
    r = symplectic_residual(got.matrix.cpu().numpy())
    print("E", E, "symplectic residual", r)
    assert r <= 1e-12 * max(1.0, float(got.matrix.abs().max()) ** 2)


def test_lattices_that_do_not_qualify_are_refused_with_the_reason():
    import cheetah_amd as ca

    kw = _kw()
    long_ring = ca.Segment([ca.Drift(T(0.1), name=f"d{k}", **DKD, **kw) for k in range(193)])
    for call in (lambda s: s.one_turn_map(torch.zeros(1, 6, **kw), T(ENERGY)), lambda s: s.closed_orbit(T(ENERGY)),
                 lambda s: s.ring_optics(T(ENERGY)), lambda s: s.chromaticity(T(ENERGY))):
        with pytest.raises(ValueError, match="193 drift-kick-drift elements, the fused kernel takes 1 to 192"):
            call(long_ring)
    linear = ca.Segment([ca.Drift(T(0.3), **kw)] + [e.clone() for e in ring("bend").elements[1:]])
    reason = linear._turn_items_dkd(linear._plan(), torch.empty(0, 7, **kw))
    assert isinstance(reason, str) and "run of linear elements" in reason
    with pytest.raises(ValueError) as info:
        linear.ring_optics(T(ENERGY))
    assert reason in str(info.value)
    with pytest.raises(ValueError, match="requires grad"):
        ring("bend").one_turn_map(torch.zeros(1, 6, **kw).requires_grad_(True), T(ENERGY))
    trainable = ca.Segment([e.clone() for e in ring("bend").elements])
    trainable.elements[0].k1 = torch.nn.Parameter(T(3.0))
    with pytest.raises(ValueError, match="requires grad"):
        trainable.ring_optics(T(ENERGY))


def test_float32_ring_gives_float64_results():
    """The float64 ring is built from the float32 ring's setting VALUES, the energy and the mass among them. The reference energy is
    a fixed point of the float32 round trip sqrt(sqrt(E^2 - m^2)^2 + m^2) every element applies: the float32 ring then keeps the
    energy from item to item as the float64 ring does to 1e-16 (an energy that moves by a float32 ulp per item, 6e-8 of itself,
    moves the matrix by as much: a property of float32 settings, not of this kernel)."""
    import cheetah_amd as ca

    sp32 = electron(F32)
    m32 = np.float32(sp32.mass_eV_float)
    e32 = np.float32(ENERGY)
    for _ in range(64):
        p = np.sqrt(e32 * e32 - m32 * m32, dtype=np.float32)
        nxt = np.sqrt(p * p + m32 * m32, dtype=np.float32)
        if nxt == e32:
            break
        e32 = nxt
    else:
        raise AssertionError("no fixed point of the float32 round trip")
    r32 = make_ring(sextupoles=True, dt=F32)
    r64 = make_ring(sextupoles=True, widen=True)
    assert r64.elements[0].k1.dtype == F64 and all(float(a.length) == float(b.length) for a, b in zip(r64.elements, r32.elements))
    assert float(r64.elements[2].angle) == float(r32.elements[2].angle) and float(r64.elements[1].k2) == float(r32.elements[1].k2)
    sp64 = ca.Species("custom", num_elementary_charges=T(-1.0), mass_eV=T(float(m32)), **_kw())
    x = seeds()
    got = r32.one_turn_map(x, T(float(e32), F32), species=sp32, along=True)
    want = r64.one_turn_map(x, T(float(e32)), species=sp64, along=True)
    assert got.matrix.dtype == F64 and got.end.dtype == F64 and got.matrix_along.dtype == F64 and got.s.dtype == F32
    M, W = got.matrix.cpu().numpy(), want.matrix.cpu().numpy()
    for b in range(5):
        bound = 1e-9 * max(1.0, np.abs(W[b]).max())
        print("float32 ring, seed", b, "difference / bound", np.abs(M[b] - W[b]).max() / bound)
        assert np.abs(M[b] - W[b]).max() <= bound
    assert same_bits(got.s[-1], r32.track(ca.ParticleBeam(rows7(x).to(F32), T(float(e32), F32), species=sp32)).s)


# ---- 11. isolation and determinism --------------------------------------------------------------------------------------------------------
def test_a_lost_seed_is_nan_in_its_own_rows_only():
    r = ring("sext_mp")
    x = many_seeds(12)
    clean = r.ring_optics(T(ENERGY), guess=x, delta=x[:, 5].clone(), num_iterations=4)
    bad = x.clone()
    bad[5, 1] = 1.5                                              # px > 1 + delta: the first drift's square root is negative
    opt = r.ring_optics(T(ENERGY), guess=bad, delta=x[:, 5].clone(), num_iterations=4)
    keep = torch.arange(12, device="cuda") != 5
    for f in FIELDS:
        a, b = getattr(opt, f), getattr(clean, f)
        assert same_bits(a[keep], b[keep]), f
        # (the seventh column is 1; the records along the ring are what the last pass met: finite up to the item of the loss)
        assert torch.isnan(a[5][:6] if f == "orbit" else (a[5][-1, :4] if f == "orbit_along" else a[5])).all(), f
    assert not opt.stable[5].any() and same_bits(opt.stable[keep], clean.stable[keep])
    mp = r.one_turn_map(bad, T(ENERGY))
    assert torch.isnan(mp.end[5, :6]).all() and torch.isnan(mp.matrix[5]).all() and torch.isfinite(mp.matrix[keep]).all()


def test_an_unstable_plane_is_flagged_alone():
    # the last QD strengthened until the vertical trace leaves [-2, 2]
    for kd_last in (-3.0, -8.0):
        opt = make_ring(kd_last=kd_last).ring_optics(T(ENERGY))
        M = opt.matrix[0].cpu().numpy()
        tr = (M[0, 0] + M[1, 1], M[2, 2] + M[3, 3])
        print("last QD k1", kd_last, "traces", tr, "stable", opt.stable.tolist(), "tunes", opt.tunes.tolist())
        if kd_last == -3.0:
            assert opt.stable.all() and torch.isfinite(opt.beta).all()
            continue
        assert abs(tr[1]) > 2 and abs(tr[0]) < 2
        assert opt.stable.tolist() == [[True, False]]
        assert torch.isfinite(opt.beta[..., 0]).all() and torch.isnan(opt.beta[..., 1]).all() and torch.isnan(opt.alpha[..., 1]).all()
        assert torch.isfinite(opt.tunes[0, 0]) and torch.isnan(opt.tunes[0, 1])
        assert float(opt.residual) <= 1e-12                      # the axis is still the closed orbit


def test_six_dimensional_search():
    # without RF nothing closes tau: M - I is singular on (tau, delta) — a non-finite or large residual, and nothing raised
    x = torch.zeros(1, 6, **_kw())
    x[0, 5] = 1e-3
    no_rf = ring("bend").closed_orbit(T(ENERGY), guess=x, longitudinal=True)
    res = float(no_rf.residual)
    print("6-D search without RF: residual", res)
    assert not (res <= 1e-9)
    # with RF on the harmonic: the axis, and from a start inside the bucket the search returns to it
    rf = ring("rf")
    x = torch.zeros(1, 6, **_kw())
    x[0, 4], x[0, 0] = 1e-3, 1e-4
    co = rf.closed_orbit(T(ENERGY), guess=x, longitudinal=True)
    print("6-D search with RF: orbit", co.orbit[0].tolist(), "residual", float(co.residual))
    assert float(co.residual) <= 1e-12 and float(co.orbit[0, :6].abs().max()) <= 1e-10


def test_two_calls_give_the_same_bits_and_a_graph_replays():
    import cheetah_amd as ca

    r = make_ring(sextupoles=True)
    x = many_seeds(65)
    a = r.ring_optics(T(ENERGY), guess=x, delta=x[:, 5].clone())
    b = r.ring_optics(T(ENERGY), guess=x, delta=x[:, 5].clone())
    for f in FIELDS + ("s", "coupling"):
        assert same_bits(getattr(a, f), getattr(b, f)), f
    assert same_bits(a.stable, b.stable)
    # captured once, replayed after an in-place edit of a setting
    energy, delta = T(ENERGY), x[:, 5].clone()
    step = ca.graph.capture(lambda: r.ring_optics(energy, guess=x, delta=delta))
    first = step()
    for f in FIELDS:
        assert same_bits(getattr(first, f), getattr(a, f)), f
    r.elements[0].k1.copy_(T(3.1))
    replayed = step()
    fresh = r.ring_optics(T(ENERGY), guess=x, delta=x[:, 5].clone())
    assert not same_bits(fresh.matrix, a.matrix)
    for f in FIELDS:
        assert same_bits(getattr(replayed, f), getattr(fresh, f)), f
