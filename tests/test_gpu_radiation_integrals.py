"""Segment.radiation_integrals on the GPU (chx_dkd_ring_radiation).

 1. on the axis against closed-form linear matrices (thick quadrupole, drift, sector bend, thin edge; periodic beta, alpha, eta;
    16-point Gauss-Legendre inside each bend) in numpy float64, for the sector ring and the ring of rectangular bends. Bound: 16 x
    the difference between that reference and its evaluation in numpy.longdouble, floor 1e-13 of the integral's scale (I4 on the
    scale of I2: it cancels).
 2. inside one bend, off the axis, against composite Simpson sums S128 and S64 of `ring_optics(along=True)` on the ring with that
    bend in 128 pieces. Bound: |S128 - S64| + 1e-12 relative (15 x Simpson's own Richardson estimate), which must itself stay
    below 1e-8 relative.
 3. split invariance: every Dipole in 3 pieces gives the same totals to 1e-12 relative, on and off the axis.
 4. the vertical ring (every element tilted by pi / 2) swaps x and y to 1e-12 relative; the flat ring's I4y, I5y, eps_y are exact zeros.
 5. the energy loss against one turn of `with_radiation_kicks(1, quantum_excitation=False)` through `track`, within 10 U0 / E0.
 6. constants: U0 = 88.46 keV for electrons at 1 GeV on rho = 1 m, C_q = 3.8319e-13 m, J_x + J_y + J_E = 4.
 7. slip: on the axis closed.slip beta0^2 + C / gamma0^2 = I1 to 1e-10 relative; sign and powers of beta0 from a ring of Drifts.
 8. B in {1, 7, 8, 9, 65}: every seed equals its single-seed result bit for bit.
 9. E = 1 and E = 192.
10. two calls and a graph replay give the same bits; a lost seed is NaN in its own rows only; a float32 ring.
11. refusals, each with its reason.

The ring is the 48-item ring of tests/test_gpu_ring_optics.py::make_ring (six cells [QF, D, B, D, QD, D, B, D] of 2.6 m, sector
bends of 30 degrees), built again here. Measured errors are printed before they are asserted."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
DKD = {"tracking_method": "drift_kick_drift"}
CELLS, ENERGY, M_E = 6, 1e8, 510998.95069
ANGLE = 2 * math.pi / (2 * CELLS)
NAMES = ("I1", "I2", "I3", "I4x", "I4y", "I5x", "I5y")
FIELDS = ("I1", "I2", "I3", "I4", "I5", "energy_loss", "partition", "damping_turns", "damping_time", "emittance", "energy_spread")


def _kw(dt=F64):
    return {"dtype": dt, "device": "cuda"}


def T(v, dt=F64):
    return torch.tensor(v, **_kw(dt))


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int64 if t.dtype == F64 else np.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def beta_rel(energy=ENERGY):
    return math.sqrt(1.0 - (M_E / energy) ** 2)


def lattice(kf=3.0, kd=-3.0, rect=False):
    """The ring as plain numbers: ("q", L, k1), ("d", L), ("b", L, angle, e1, e2)."""
    e = ANGLE / 2 if rect else 0.0
    cell = [("q", 0.2, kf), ("d", 0.3), ("b", 0.5, ANGLE, e, e), ("d", 0.3), ("q", 0.2, kd), ("d", 0.3), ("b", 0.5, ANGLE, e, e), ("d", 0.3)]
    return cell * CELLS


def make_ring(sextupoles=False, corrector=None, rect=False, vertical=False, dt=F64, widen=False, pieces=1, split=None):
    """The ring of tests/test_gpu_ring_optics.py::make_ring — 48 items —, with the Drift behind every QF a Sextupole and a zero-length
    order-0 Multipole of knl = -corrector in front of everything on request; `rect`: e1 = e2 = angle / 2; `vertical`: every element
    tilted by pi / 2 (a Quadrupole's tilt makes it -k1: its k1 is flipped back); `widen`: a float64 ring of the float32 ring's
    setting values; `pieces`: every Dipole as that many `_arc_pieces`; `split` = (name, n): that one Dipole as n pieces."""
    import cheetah_amd as ca

    kw = _kw(F64 if widen else dt)
    t = (lambda v: T(v, F32).to(F64)) if widen else (lambda v: T(v, dt))  # noqa: E731
    tilt = {"tilt": t(math.pi / 2)} if vertical else {}
    els = []
    if corrector is not None:
        els.append(ca.Multipole(t(0.0), order=0, knl=t(-corrector), name="corrector", **DKD, **kw))
    for c in range(CELLS):
        for j, item in enumerate(lattice(rect=rect)[:8]):
            name = f"c{c}_{j}"
            if item[0] == "d" and j == 1 and sextupoles:
                els.append(ca.Sextupole(t(0.3), k2=t(20.0 if c % 2 == 0 else -30.0), num_steps=2, name=name, **tilt, **DKD, **kw))
            elif item[0] == "d":
                els.append(ca.Drift(t(item[1]), name=name, **DKD, **kw))
            elif item[0] == "b":
                bend = ca.Dipole(t(item[1]), angle=t(item[2]), dipole_e1=t(item[3]), dipole_e2=t(item[4]), name=name, **tilt, **DKD, **kw)
                n = pieces if split is None else (split[1] if split[0] == name else 1)
                els += bend._arc_pieces(n, "p") if n > 1 else [bend]
            else:
                els.append(ca.Quadrupole(t(item[1]), k1=t(-item[2] if vertical else item[2]), num_steps=1, name=name, **tilt, **DKD, **kw))
    return ca.Segment(els)


def totals(rad):
    """(B, 7) float64 numpy in the order of NAMES."""
    return torch.cat([rad.I1[:, None], rad.I2[:, None], rad.I3[:, None], rad.I4, rad.I5], dim=1).cpu().numpy()


def relative(a, b):
    """|a - b| / |b| entry by entry, 0 where both are exact zeros."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((a == 0) & (b == 0), 0.0, np.abs(a - b) / np.abs(b))


OFF_AXIS = {"sextupoles": True, "corrector": 1e-4}
OFF_DELTA = 1e-3


# ---- 1. on the axis against closed-form linear matrices --------------------------------------------------------------------------------
def reference_integrals(items, ft):
    """(I1, I2, I3, I4x, I5x) of the flat ring `items` from 3 x 3 matrices on (x, x', dp / p) in the float type `ft`: the exact
    linearisation of the maps on the axis. eta is d x / d (dp / p): what the kernel's beta0 d x / d delta is."""
    f = lambda v: ft(v)  # noqa: E731
    one, zero = f(1), f(0)
    mat = lambda rows: np.array(rows, dtype=ft)  # noqa: E731

    def drift(L):
        return mat([[one, L, zero], [zero, one, zero], [zero, zero, one]])

    def quad(L, k):
        r = np.sqrt(abs(k))
        if k > 0:
            c, s = np.cos(r * L), np.sin(r * L)
            return mat([[c, s / r, zero], [-r * s, c, zero], [zero, zero, one]])
        c, s = np.cosh(r * L), np.sinh(r * L)
        return mat([[c, s / r, zero], [r * s, c, zero], [zero, zero, one]])

    def sector(L, h):
        c, s = np.cos(h * L), np.sin(h * L)
        return mat([[c, s / h, (one - c) / h], [-h * s, c, s], [zero, zero, one]])

    def edge(h, e):
        return mat([[one, zero, zero], [h * np.tan(e), one, zero], [zero, zero, one]])

    def element(item):
        if item[0] == "d":
            return drift(f(item[1]))
        if item[0] == "q":
            return quad(f(item[1]), f(item[2]))
        L, h = f(item[1]), f(item[2]) / f(item[1])
        return edge(h, f(item[4])) @ sector(L, h) @ edge(h, f(item[3]))

    M = np.eye(3, dtype=ft)
    for item in items:
        M = element(item) @ M
    half = (M[0, 0] - M[1, 1]) / 2
    sin_mu = np.sign(M[0, 1]) * np.sqrt(-(M[0, 1] * M[1, 0]) - half * half)
    beta0, alpha0 = M[0, 1] / sin_mu, half / sin_mu
    a, b, c, d = one - M[0, 0], -M[0, 1], -M[1, 0], one - M[1, 1]
    det = a * d - b * c
    eta0 = np.array([(d * M[0, 2] - b * M[1, 2]) / det, (a * M[1, 2] - c * M[0, 2]) / det], dtype=ft)
    x16, w16 = np.polynomial.legendre.leggauss(16)
    nodes, weights = ((x16 + 1) / 2).astype(ft), (w16 / 2).astype(ft)

    def eta_at(A):
        return A[:2, :2] @ eta0 + A[:2, 2]

    I = np.zeros(5, dtype=ft)
    A = np.eye(3, dtype=ft)
    for item in items:
        if item[0] == "b":
            L, h, e1, e2 = f(item[1]), f(item[2]) / f(item[1]), f(item[3]), f(item[4])
            eta_in = eta_at(A)[0]
            Ae = edge(h, e1) @ A
            s_eta, s_H = zero, zero
            for node, w in zip(nodes, weights):
                As = sector(node * L, h) @ Ae
                eta = eta_at(As)
                u, v = As[0, 0] * beta0 - As[0, 1] * alpha0, As[1, 0] * beta0 - As[1, 1] * alpha0
                beta, alpha = (u * u + As[0, 1] ** 2) / beta0, -(u * v + As[0, 1] * As[1, 1]) / beta0
                s_eta = s_eta + w * eta[0]
                s_H = s_H + w * (eta[0] ** 2 + (beta * eta[1] + alpha * eta[0]) ** 2) / beta
            eta_out = eta_at(element(item) @ A)[0]
            I += np.array([L * h * s_eta, L * h * h, L * abs(h) ** 3, L * h ** 3 * s_eta - h * (h * np.tan(e1) * eta_in + h * np.tan(e2) * eta_out),
                           L * abs(h) ** 3 * s_H], dtype=ft)
        A = element(item) @ A
    return I


@pytest.mark.parametrize("rect", [False, True], ids=["sector", "rectangular"])
def test_on_axis_against_closed_form_matrices(rect):
    rad = make_ring(rect=rect).radiation_integrals(T(ENERGY), along=True)
    got = totals(rad)[0]
    ref = reference_integrals(lattice(rect=rect), np.float64)
    ref_ld = reference_integrals(lattice(rect=rect), np.longdouble)
    scale = np.abs(ref.copy())
    scale[3] = scale[1]                                           # I4 on the scale of I2
    bound = np.maximum(16 * np.abs(ref.astype(np.longdouble) - ref_ld).astype(np.float64), 1e-13 * scale)
    mine = got[[0, 1, 2, 3, 5]]
    for k, name in enumerate(("I1", "I2", "I3", "I4x", "I5x")):
        print(f"{'rectangular' if rect else 'sector'} {name}: kernel {mine[k]:.15g} reference {ref[k]:.15g} error {abs(mine[k] - ref[k]):.3e} "
              f"({abs(mine[k] - ref[k]) / scale[k]:.3e} of the scale) bound {bound[k]:.3e}")
    print("J_x", float(rad.partition[0, 0]), "U0 [eV]", float(rad.energy_loss), "eps_x", float(rad.emittance[0, 0]), "sigma_delta",
          float(rad.energy_spread))
    assert (np.abs(mine - ref) <= bound).all()
    assert got[4] == 0.0 and got[6] == 0.0 and float(rad.emittance[0, 1]) == 0.0       # a flat ring: exact zeros
    assert abs(float(rad.partition[0, 0]) - (1.023 if rect else 0.165)) < 5e-4
    # the records along the ring: zeros off the Dipoles, the totals their sums in the items' order
    along = rad.integrals_along[0].cpu().numpy()
    bends = np.array([item[0] == "b" for item in lattice()])
    assert along.shape == (48, 7) and (along[~bends] == 0).all() and (along[bends, 1] > 0).all()
    run = np.zeros(7)
    for row in along:
        run = run + row
    assert np.array_equal(run, got)
    assert same_bits(rad.I5, make_ring(rect=rect).radiation_integrals(T(ENERGY)).I5)     # the same with and without `along`


# ---- 2. inside one bend, off the axis, against the ring optics of the finely split ring -------------------------------------------------
@pytest.mark.parametrize("name", ["c0_2", "c0_6"], ids=["behind_qf", "behind_qd"])
def test_one_bend_off_axis_against_simpson_sums_of_ring_optics(name):
    ring = make_ring(**OFF_AXIS)
    index = [e.name for e in ring.elements].index(name)
    rad = ring.radiation_integrals(T(ENERGY), delta=OFF_DELTA, along=True)
    got = rad.integrals_along[0, index].cpu().numpy()
    fine = make_ring(**OFF_AXIS, split=(name, 128))
    assert len(fine.elements) == len(ring.elements) + 127
    opt = fine.ring_optics(T(ENERGY), delta=OFF_DELTA, along=True)
    assert float(opt.residual) < 1e-12 and float(rad.closed.residual) < 1e-12 and float(rad.closed.orbit[0, 0].abs()) > 1e-5
    rows = slice(index, index + 129)                              # behind the item in front of the bend ... behind the last piece
    eta = beta_rel() * opt.dispersion_along[0, rows]              # (129, 4)
    beta, alpha = opt.beta[0, rows], opt.alpha[0, rows]           # (129, 2)
    L, h = 0.5, ANGLE / 0.5
    H = [(eta[:, 2 * u] ** 2 + (beta[:, u] * eta[:, 2 * u + 1] + alpha[:, u] * eta[:, 2 * u]) ** 2) / beta[:, u] for u in range(2)]
    zero = torch.zeros_like(eta[:, 0])
    # a sector bend in a flat ring: cos t = 1, sin t = 0, no edge terms
    integrands = torch.stack([h * eta[:, 0], zero + h * h, zero + abs(h) ** 3, h ** 3 * eta[:, 0], zero, abs(h) ** 3 * H[0], abs(h) ** 3 * H[1]], dim=1)

    def simpson(f):
        n = f.shape[0] - 1
        w = torch.ones(n + 1, **_kw())
        w[1:-1:2], w[2:-1:2] = 4.0, 2.0
        return ((w[:, None] * f).sum(0) * (L / (3.0 * n))).cpu().numpy()

    s128, s64 = simpson(integrands), simpson(integrands[::2])
    bound = np.abs(s128 - s64) + 1e-12 * np.abs(s128)
    for k, n in enumerate(NAMES):
        print(f"{name} {n}: kernel {got[k]:.15g} S128 {s128[k]:.15g} |kernel - S128| {abs(got[k] - s128[k]):.3e} bound {bound[k]:.3e} "
              f"(relative {bound[k] / abs(s128[k]) if s128[k] else 0.0:.3e})")
    live = s128 != 0                                              # (I4y, I5y: exact zeros on both sides in a flat ring)
    assert live[[0, 1, 2, 3, 5]].all()
    assert (bound[live] < 1e-8 * np.abs(s128[live])).all()       # else the comparison proves nothing
    assert (np.abs(got - s128) <= bound).all()


# ---- 3. split invariance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off_axis", [False, True], ids=["on_axis", "off_axis"])
def test_split_invariance(off_axis):
    kw, delta = (OFF_AXIS, OFF_DELTA) if off_axis else ({}, None)
    whole = make_ring(**kw).radiation_integrals(T(ENERGY), delta=delta)
    split_ring = make_ring(**kw, pieces=3)
    assert len(split_ring.elements) == 72 + (1 if off_axis else 0)
    split = split_ring.radiation_integrals(T(ENERGY), delta=delta)
    rel = relative(totals(split)[0], totals(whole)[0])
    print("split in 3, relative differences", dict(zip(NAMES, rel)))
    assert (rel <= 1e-12).all()
    for f in ("energy_loss", "partition", "emittance", "energy_spread", "damping_time"):
        assert (relative(getattr(split, f).cpu().numpy(), getattr(whole, f).cpu().numpy()) <= 1e-11).all(), f


# ---- 4. the vertical ring ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rect", [False, True], ids=["sector", "rectangular"])
def test_vertical_ring_swaps_the_planes(rect):
    flat = make_ring(rect=rect).radiation_integrals(T(ENERGY))
    vert = make_ring(rect=rect, vertical=True).radiation_integrals(T(ENERGY))
    f, v = totals(flat)[0], totals(vert)[0]
    assert f[4] == 0.0 and f[6] == 0.0 and float(flat.emittance[0, 1]) == 0.0
    rel = relative(v[[0, 1, 2, 4, 6]], f[[0, 1, 2, 3, 5]])
    print("vertical ring against the flat ring", rel, "its I4x, I5x", v[3], v[5])
    assert (rel <= 1e-12).all()
    assert abs(v[3]) <= 1e-12 * f[1] and abs(v[5]) <= 1e-12 * f[5]                     # (cos(pi / 2) is 6e-17, not 0)
    assert (relative(vert.partition[0, [1, 0, 2]].cpu().numpy(), flat.partition[0].cpu().numpy()) <= 1e-12).all()
    assert relative(float(vert.emittance[0, 1]), float(flat.emittance[0, 0])) <= 1e-12


# ---- 5. the energy loss against the merged kick -----------------------------------------------------------------------------------------
def test_energy_loss_against_one_turn_of_radiation_kicks():
    import cheetah_amd as ca

    ring = make_ring()
    rad = ring.radiation_integrals(T(ENERGY))
    particle = torch.zeros(1, 7, **_kw())
    particle[0, 6] = 1.0
    out = ring.with_radiation_kicks(1, quantum_excitation=False).track(ca.ParticleBeam(particle, T(ENERGY), species=ca.Species("electron", **_kw())))
    p0c = math.sqrt(ENERGY ** 2 - M_E ** 2)
    lost = -float(out.particles[0, 5]) * p0c
    u0 = float(rad.energy_loss)
    print("U0 from the integrals", u0, "eV, from one tracked turn", lost, "eV, relative difference", abs(lost - u0) / u0, "allowed", 10 * u0 / ENERGY)
    assert 8.0 < u0 < 10.0
    assert abs(lost - u0) <= 10 * u0 / ENERGY * u0


# ---- 6. constants -----------------------------------------------------------------------------------------------------------------------
def test_constants():
    import cheetah_amd as ca
    from cheetah_amd.particles.optics import radiation_constants

    # twelve bends of rho = 1 m; the faces defocus vertically, so the orbit is found although y has no periodic solution
    kw = _kw()
    ring = ca.Segment([ca.Dipole(T(ANGLE), angle=T(ANGLE), dipole_e1=T(-0.1), dipole_e2=T(-0.1), name=f"b{i}", **DKD, **kw) for i in range(12)])
    rad = ring.radiation_integrals(T(1e9))
    print("rho = 1 m at 1 GeV: I2", float(rad.I2), "U0", float(rad.energy_loss), "eV")
    assert abs(float(rad.I2) - 2 * math.pi) <= 1e-14 * 2 * math.pi and abs(float(rad.energy_loss) - 88.46e3) < 5.0
    assert abs(radiation_constants(M_E, -1.0)[1] - 3.8319e-13) < 0.5e-17
    for r in (make_ring(), make_ring(rect=True), make_ring(**OFF_AXIS)):
        J = r.radiation_integrals(T(ENERGY), delta=OFF_DELTA).partition[0]
        print("partition", J.tolist(), "sum - 4", float(J.sum()) - 4.0)
        assert abs(float(J.sum()) - 4.0) <= 4e-15


# ---- 7. slip ----------------------------------------------------------------------------------------------------------------------------
def test_slip_and_the_first_integral():
    import cheetah_amd as ca

    gamma2, b2 = (ENERGY / M_E) ** 2, beta_rel() ** 2
    # a ring of Drifts (I1 = 0: there is no Dipole) fixes the sign and the powers: d tau / d delta = -C / (beta0^2 gamma0^2)
    drifts = ca.Segment([ca.Drift(T(0.65), **DKD, **_kw()) for _ in range(4)])
    m45 = float(drifts.one_turn_map(torch.zeros(1, 6, **_kw()), T(ENERGY)).matrix[0, 4, 5])
    print("Drifts: M[4, 5]", m45, "-C / (beta0^2 gamma0^2)", -2.6 / (b2 * gamma2))
    assert abs(m45 * b2 * gamma2 + 2.6) <= 1e-10 * 2.6
    for rect in (False, True):
        rad = make_ring(rect=rect).radiation_integrals(T(ENERGY))
        C = float(rad.circumference)
        want = float(rad.closed.slip) * b2 + C / gamma2
        print("rectangular" if rect else "sector", "I1", float(rad.I1), "slip beta0^2 + C / gamma0^2", want, "relative", abs(float(rad.I1) - want) / want)
        assert abs(C - CELLS * 2.6) <= 1e-14 * C
        assert abs(float(rad.I1) - want) <= 1e-10 * abs(want)


# ---- 8. batch size ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def single_seed_results():
    ring = make_ring(**OFF_AXIS)
    deltas = torch.linspace(-2e-3, 2e-3, 65, **_kw())
    return ring, deltas, [ring.radiation_integrals(T(ENERGY), delta=deltas[b:b + 1].clone(), along=True) for b in range(65)]


@pytest.mark.parametrize("B", [1, 7, 8, 9, 65])
def test_every_seed_equals_its_single_seed_result(B):
    ring, deltas, singles = single_seed_results()
    rad = ring.radiation_integrals(T(ENERGY), delta=deltas[:B].clone(), along=True)
    assert rad.I1.shape == (B,) and rad.I4.shape == (B, 2) and rad.integrals_along.shape == (B, 49, 7) and rad.damping_time.shape == (B, 3)
    assert torch.isfinite(rad.integrals_along).all() and float(rad.closed.residual.max()) < 1e-11
    for b in range(B):
        for f in FIELDS + ("integrals_along",):
            assert same_bits(getattr(rad, f)[b:b + 1], getattr(singles[b], f)), (b, f)
    if B == 65:
        spread = totals(rad)
        print("I5x over delta = -2e-3 ... 2e-3:", spread[0, 5], spread[32, 5], spread[64, 5])
        assert spread[0, 5] != spread[64, 5]


# ---- 9. item count ----------------------------------------------------------------------------------------------------------------------
def test_one_item_and_192_items():
    import cheetah_amd as ca

    L, angle = 0.5, ANGLE
    one = ca.Segment([ca.Dipole(T(L), angle=T(angle), dipole_e1=T(-0.2), dipole_e2=T(-0.2), **DKD, **_kw())])
    rad = one.radiation_integrals(T(ENERGY), along=True)
    h = angle / L
    assert float(rad.I2) == L * (h * h) and float(rad.I3) == L * (abs(h) * (h * h)) and rad.integrals_along.shape == (1, 1, 7)
    assert math.isnan(float(rad.I5[0, 1])) and math.isnan(float(rad.emittance[0, 1]))          # y has no periodic solution
    assert math.isfinite(float(rad.I5[0, 0])) and math.isfinite(float(rad.I1)) and torch.isfinite(rad.I4).all()
    whole = make_ring().radiation_integrals(T(ENERGY))
    ring = make_ring(pieces=13)
    assert len(ring.elements) == 192
    rad = ring.radiation_integrals(T(ENERGY), along=True)
    rel = relative(totals(rad)[0], totals(whole)[0])
    print("192 items, relative differences", dict(zip(NAMES, rel)))
    assert rad.integrals_along.shape == (1, 192, 7) and (rel <= 1e-12).all()
    with pytest.raises(ValueError, match="193 drift-kick-drift elements"):
        ca.Segment(list(ring.elements) + [ca.Drift(T(0.0), **DKD, **_kw())]).radiation_integrals(T(ENERGY))


# ---- 10. reproducibility and failure ----------------------------------------------------------------------------------------------------
def test_two_calls_and_a_graph_replay_give_the_same_bits():
    import cheetah_amd as ca

    ring, deltas, _ = single_seed_results()
    energy, delta = T(ENERGY), deltas.clone()
    a = ring.radiation_integrals(energy, delta=delta, along=True)
    b = ring.radiation_integrals(energy, delta=delta, along=True)
    for f in FIELDS + ("integrals_along", "circumference"):
        assert same_bits(getattr(a, f), getattr(b, f)), f
    step = ca.graph.capture(lambda: ring.radiation_integrals(energy, delta=delta, along=True))
    first = step()
    for f in FIELDS + ("integrals_along", "circumference"):
        assert same_bits(getattr(first, f), getattr(a, f)), f
    delta.mul_(0.5)                                               # replayed after an in-place edit of an input
    replayed = step()
    fresh = ring.radiation_integrals(energy, delta=delta.clone(), along=True)
    assert not same_bits(fresh.I5, a.I5)
    for f in FIELDS + ("integrals_along",):
        assert same_bits(getattr(replayed, f), getattr(fresh, f)), f


def test_a_lost_seed_is_nan_in_its_own_rows_only():
    ring, deltas, _ = single_seed_results()
    delta = deltas[:12].clone()
    guess = torch.zeros(12, 6, **_kw())
    clean = ring.radiation_integrals(T(ENERGY), delta=delta, guess=guess, num_iterations=4, along=True)
    bad = guess.clone()
    bad[5, 1] = 1.5                                               # px > 1 + delta: the first drift's square root is negative
    rad = ring.radiation_integrals(T(ENERGY), delta=delta, guess=bad, num_iterations=4, along=True)
    keep = torch.arange(12, device="cuda") != 5
    for f in FIELDS + ("integrals_along",):
        a, b = getattr(rad, f), getattr(clean, f)
        assert same_bits(a[keep], b[keep]), f
        assert torch.isnan(a[5]).all(), f
    assert torch.isfinite(clean.integrals_along).all()


def test_float32_ring_gives_float64_results():
    """As tests/test_gpu_ring_optics.py::test_float32_ring_gives_float64_results: the float64 ring holds the float32 ring's setting
    values, the energy a fixed point of the float32 round trip every element applies, so both rings keep the same energy from item to
    item; its bound, 1e-9 relative (I4 on the scale of I2), is kept."""
    import cheetah_amd as ca

    sp32 = ca.Species("electron", **_kw(F32))
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
    sp64 = ca.Species("custom", num_elementary_charges=T(-1.0), mass_eV=T(float(m32)), **_kw())
    got = make_ring(sextupoles=True, dt=F32).radiation_integrals(T(float(e32), F32), species=sp32, delta=OFF_DELTA, along=True)
    want = make_ring(sextupoles=True, widen=True).radiation_integrals(T(float(e32)), species=sp64, delta=OFF_DELTA, along=True)
    for f in FIELDS + ("integrals_along", "circumference"):
        assert getattr(got, f).dtype == F64, f
    g, w = totals(got)[0], totals(want)[0]
    scale = np.abs(w)
    scale[3] = scale[1]
    print("float32 ring against the widened ring", np.abs(g - w) / np.where(scale > 0, scale, 1.0))
    assert (np.abs(g - w) <= 1e-9 * scale).all()
    assert same_bits(got.circumference, want.circumference)
    assert relative(float(got.energy_loss), float(want.energy_loss)) <= 1e-9


# ---- 11. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_with_their_reasons():
    import cheetah_amd as ca

    ring = make_ring()
    els = [e.clone() for e in ring.elements]
    els[1] = ca.Drift(T(0.3), **_kw())                             # a linear Drift
    with pytest.raises(ValueError, match="radiation_integrals: a run of linear elements stands in the ring"):
        ca.Segment(els).radiation_integrals(T(ENERGY))
    trainable = ca.Segment([e.clone() for e in ring.elements])
    trainable.elements[2].angle = torch.nn.Parameter(T(ANGLE))
    with pytest.raises(ValueError, match="radiation_integrals: a setting of the lattice requires grad"):
        trainable.radiation_integrals(T(ENERGY))
    with pytest.raises(ValueError, match="radiation_integrals has no autograd: an input requires grad"):
        ring.radiation_integrals(T(ENERGY).requires_grad_(True))
    # `along` records for a ring `track_turns` does not fuse: float32 elements of two arithmetic classes
    mixed = make_ring(dt=F32)
    mixed.elements[0].dkd_precision = "storage"
    with pytest.raises(ValueError, match="radiation_integrals: .*more than one arithmetic class"):
        mixed.radiation_integrals(T(ENERGY, F32), along=True)
