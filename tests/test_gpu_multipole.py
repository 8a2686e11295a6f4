"""The Multipole on the GPU (CHX_DKD_MULTIPOLE): Bmad's exact drifts around `num_steps` thin kicks of one order m = 0 .. 3,
d px - i d py = -(knl + i ksl) / n (x + i y)^m / m!.

1. golden     the float64 kernel against tests/golden/dkd_multipole.npz (the map composed from the reference's bmadx functions):
              1e-12 of each column's largest magnitude, the Sextupole's bound. The generator's spread between two orderings of the
              same arithmetic is 4e-18; a wrong formula shows at 1e-3 and above (the kicks move px, py by their whole size).
2. relations  in float64, 1e-12 of each column's largest magnitude: no strength = a Drift; order 2 = the Sextupole; a thin order-0
              element = px - knl, py + ksl; a tilt = the strengths rotated, knl + i ksl -> (knl + i ksl) e^{-i (m + 1) theta}
              (what rotates by e^{+i (m + 1) theta} is knl - i ksl: the kick is d px - i d py, and p' = p e^{-i theta}).
3. convergence  order 1 against the drift-kick-drift Quadrupole: second order in 1 / n, a factor of 3.5 to 4.5 per doubling.
4. gradients  `backward()` against autograd through this project's drift-kick-drift `Drift`s and a torch kick: 1e-9 of each
              gradient's largest magnitude. The composition takes the entrance and the exit transformation's tilt and shift as
              separate leaves; where a gradient is the sum of two such terms that cancel (the tilt and the shift of an element
              without strength, the shift of an order-0 kick: analytically zero), the bound is 1e-9 of the TERMS' magnitude — a
              bound relative to a sum that is zero up to rounding would ask for nothing or for everything.
5. symplectic  the Sextupole test's J^T S J - S for order 3 with both strengths, tilt and shift.
6. float32    "mixed" and "storage" within 4 x the Sextupole's per-column error on the same beam, steps and mode: order 2 with the
              Sextupole's strength, order 3 at the strength of equal rms kick; "double" = the float64 result rounded.
7. batch      `knl` of shape (3,) on one beam = three scalar tracks, bit for bit.
8. fast paths  `Segment.track` (one chx_dkd_chain_mixed call) and `track_turns(fused=True)` (chx_dkd_turns) against the element-by-
              element loops, bit for bit, in every arithmetic mode; no host synchronisation.
9. physics    the amplitude detuning of a thin octupole in a FODO cell: d nu / d J = knl beta^2 / (16 pi) within 2 %.

Measured on an MI355X: golden 5.2e-14 (delta's round trip through the energy; the other columns 1e-16); relations 2.1e-16, 1.9e-16,
5.9e-14 and 1.0e-15; ratios per doubling 3.90 to 4.10; gradients 2.1e-13; J^T S J - S 2.2e-16 and 4.4e-16 (the Quadrupole: 6.7e-16,
1.1e-15); float32 at most 2.3 x the Sextupole's error; d nu / d J = 401.10 against 403.25, with knl = 0 3.4e-5 of that.

Every test fails without the feature: `ca.Multipole` does not exist. N from {1, 255, 257, 700} (a tile is 256 rows), num_steps from
{1, 3}."""
import cmath
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_dkd_sextupole import (MODE_IDS, MODES, T, _kw, as_float64, column_error, make_beam, outputs, sextupole,  # (helpers only)
                                          symplectic_residual, turn_beam)
from tests.test_gpu_track_turns import same_bits  # (helper only)
from tests.test_gpu_track_turns_dkd import check_records, run_loop, same_bits_nan_for_nan  # (helpers only; TURNS = 37, N = 700)
from tests.test_gpu_track_turns_no_sync import sync_warnings  # (helper only)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dkd_multipole.npz")
F64, F32 = torch.float64, torch.float32
DKD = {"tracking_method": "drift_kick_drift"}
TURNS = 37


def multipole(dt, length, order, knl, ksl, tilt=0.0, mis=(0.0, 0.0), n=1, **extra):
    import cheetah_amd as ca

    return ca.Multipole(T(length, dt), order, knl=T(knl, dt), ksl=T(ksl, dt), tilt=T(tilt, dt), misalignment=T(list(mis), dt), num_steps=n,
                        **extra, **_kw(dt))


# ---- 1. golden ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


GOLDEN_NAMES = ["order0_thin_upright_n1", "order1_thin_tilted_n1", "order2_thin_misaligned_n1", "order3_thin_tilted_misaligned_n1",
                "order0_tilted_n3", "order1_misaligned_n3", "order2_upright_n1", "order3_tilted_misaligned_n3"]


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_float64_kernel_matches_the_reference_composition(name, n):
    import cheetah_amd as ca

    g = golden()
    assert list(g["names"]) == GOLDEN_NAMES
    length, knl, ksl, tilt, mx, my = g[f"{name}_params"]
    el = multipole(F64, length, int(g[f"{name}_order"]), knl, ksl, tilt, (mx, my), int(g[f"{name}_steps"]))
    mass, charge = g["species"]
    species = ca.Species("custom", num_elementary_charges=T(float(charge)), mass_eV=T(float(mass)), **_kw(F64))
    for tag in g["beams"]:
        beam = ca.ParticleBeam(T(g[f"in_{tag}"][:n]), T(float(g["energy"])), species=species)
        out = el.track(beam)
        want = g[f"{name}_{tag}_out"]
        err = np.abs(out.particles.cpu().numpy() - want[:n])[:, :6].max(axis=0) / np.abs(want)[:, :6].max(axis=0)
        print(name, tag, n, "error per column / the column's largest magnitude", err)
        assert (err <= 1e-12).all(), (name, tag, err)
        assert (out.particles[:, 6] == 1).all()
        assert abs(float(out.energy) - float(g[f"{name}_{tag}_energy_out"])) <= 4 * 2.0 ** -52 * float(g["energy"])
        assert float(out.s) == float(length)


# ---- 2. relations -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_zero_strength_is_a_drift(order):
    import cheetah_amd as ca

    beam = make_beam(F64, 257)
    want = ca.Drift(T(0.3), **DKD, **_kw(F64)).track(beam)
    for n in (1, 3):
        out = multipole(F64, 0.3, order, 0.0, 0.0, n=n).track(beam)
        err = column_error(out.particles, want.particles)
        print("order", order, "knl = ksl = 0, num_steps", n, err)
        assert (err <= 1e-12).all(), err
        assert same_bits(out.energy, want.energy) and same_bits(out.s, want.s)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("sigma", [1e-3, 5e-3], ids=["1mm", "5mm"])
def test_order_two_without_skew_is_the_sextupole(sigma, n):
    beam = make_beam(F64, 700, sigma)
    length, k2, tilt, mis = 0.25, -80.0, -0.4, (1e-3, -5e-4)
    want = sextupole(F64, length, k2, tilt, mis, n).track(beam)
    out = multipole(F64, length, 2, k2 * length, 0.0, tilt, mis, n).track(beam)
    err = column_error(out.particles, want.particles)
    print("order 2 against the Sextupole, sigma", sigma, "num_steps", n, err)
    assert (err <= 1e-12).all(), err
    assert same_bits(out.energy, want.energy) and same_bits(out.s, want.s)


def test_a_thin_dipole_kick_moves_px_by_minus_knl_and_py_by_ksl():
    beam = make_beam(F64, 257)
    knl, ksl = 1e-4, -2e-4
    out = multipole(F64, 0.0, 0, knl, ksl).track(beam)
    want = beam.particles.clone()
    want[:, 1] -= knl
    want[:, 3] += ksl
    err = column_error(out.particles, want)
    print("thin order 0", err)
    assert (err <= 1e-12).all(), err                             # x, y, tau, delta: up to the coordinate round trip
    assert same_bits(out.particles[:, 0], beam.particles[:, 0]) and same_bits(out.particles[:, 2], beam.particles[:, 2])
    assert same_bits(out.s, beam.s)                              # s stays
    # a horizontal corrector of angle theta is order 0 with knl = -theta
    kicked = multipole(F64, 0.0, 0, -3e-5, 0.0).track(beam)
    assert np.abs((kicked.particles[:, 1] - beam.particles[:, 1]).cpu().numpy() - 3e-5).max() <= 1e-12 * 3e-5


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("n,length", [(1, 0.0), (3, 0.2)], ids=["thin", "L0.2-n3"])
def test_a_tilt_rotates_the_strengths(n, length, order):
    beam = make_beam(F64, 700, 5e-3)
    theta, mis = 0.37, (1e-3, -5e-4)
    k = complex(-0.4, 0.5) * 1e-4 * 300.0 ** order               # kicks of some 1e-5 rad on a beam of 5 mm
    tilted = multipole(F64, length, order, k.real, k.imag, theta, mis, n).track(beam)
    r = k * cmath.exp(-1j * (order + 1) * theta)
    rotated = multipole(F64, length, order, r.real, r.imag, 0.0, mis, n).track(beam)
    err = column_error(tilted.particles, rotated.particles)
    drift = multipole(F64, length, order, 0.0, 0.0, 0.0, mis, n).track(beam)
    moved = column_error(drift.particles, rotated.particles)
    print("order", order, "length", length, "tilted against rotated strengths", err, "the kicks move the columns by", moved)
    assert (err <= 1e-12).all(), err
    assert moved[1] > 1e-2 and moved[3] > 1e-2                   # (the kick is there to be rotated)


# ---- 3. convergence ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,k1", [(0.2, 3.0), (0.3, -2.0)])
def test_order_one_converges_to_the_quadrupole_in_second_order(length, k1):
    import cheetah_amd as ca

    beam = make_beam(F64, 700, 1e-3)
    want = ca.Quadrupole(T(length), k1=T(k1), num_steps=1, **DKD, **_kw(F64)).track(beam).particles
    errors = []
    for n in (2, 4, 8, 16):
        got = multipole(F64, length, 1, k1 * length, 0.0, n=n).track(beam).particles
        errors.append(column_error(got, want)[:5])               # x, px, y, py, tau (delta does not change)
    ratios = np.array([errors[i] / errors[i + 1] for i in range(3)])
    print("L", length, "k1", k1, "errors at n = 2, 4, 8, 16:", errors, "ratios per doubling:", ratios)
    assert (ratios >= 3.5).all() and (ratios <= 4.5).all(), ratios


# ---- 4. gradients -----------------------------------------------------------------------------------------------------------------------
def composed(beam, length, order, knl, ksl, tilt_in, tilt_out, mis_in, mis_out, n):
    """offset_set, Drift(h), n x [kick, Drift(2 h; h behind the last kick)], offset_unset — with this project's drift-kick-drift
    Drift elements and torch operations (every Drift converts (tau, delta) <-> (z, pz) on its own). The entrance and the exit
    transformation take their own tilt and shift: the element's gradient is the sum of the two. Differentiable."""
    import cheetah_amd as ca

    def rebuilt(b, x, px, y, py):
        p = torch.stack([x, px, y, py, b.particles[:, 4], b.particles[:, 5], b.particles[:, 6]], dim=1)
        return ca.ParticleBeam(p, b.energy, particle_charges=b.particle_charges, survival_probabilities=b.survival_probabilities, s=b.s,
                               species=b.species)

    def drift(b, L):
        return ca.Drift(L, **DKD, **_kw(F64)).track(b)            # (L may carry a graph)

    s, c = torch.sin(tilt_in), torch.cos(tilt_in)
    x, px, y, py = (beam.particles[:, j] for j in range(4))
    xi, yi = x - mis_in[0], y - mis_in[1]
    b = rebuilt(beam, xi * c + yi * s, px * c + py * s, -xi * s + yi * c, -px * s + py * c)
    h = length / (2 * n)
    bn, an = knl / math.factorial(order) / n, ksl / math.factorial(order) / n
    b = drift(b, h)
    for step in range(n):
        x, px, y, py = (b.particles[:, j] for j in range(4))
        re, im = torch.ones_like(x), torch.zeros_like(x)
        for _ in range(order):
            re, im = re * x - im * y, re * y + im * x
        b = rebuilt(b, x, px - (bn * re - an * im), y, py + (bn * im + an * re))
        b = drift(b, 2 * h if step + 1 < n else h)
    s, c = torch.sin(tilt_out), torch.cos(tilt_out)
    x, px, y, py = (b.particles[:, j] for j in range(4))
    return rebuilt(b, x * c - y * s + mis_out[0], px * c - py * s, x * s + y * c + mis_out[1], px * s + py * c)


#: length, order, knl, ksl, tilt, misalignment, num_steps, rows put on the element's axis
GRAD_CASES = {
    "order3-tilted-misaligned-n3": (0.25, 3, -2e4, 1.5e4, -0.4, (1e-3, -5e-4), 3, ()),
    "order1-n1": (0.2, 1, 0.6, -0.3, 0.3, (2e-4, 1e-4), 1, ()),
    "order3-thin": (0.0, 3, 2e4, -1e4, 0.2, (1e-3, -5e-4), 1, ()),
    "order0-n3": (0.2, 0, 1e-4, -2e-4, 0.3, (1e-3, -5e-4), 3, ()),
    "order2-no-strength": (0.2, 2, 0.0, 0.0, 0.3, (1e-3, -5e-4), 1, ()),
    "order1-no-strength-thin": (0.0, 1, 0.0, 0.0, 0.3, (1e-3, -5e-4), 1, ()),
    "order2-on-axis-rows": (0.2, 2, 20.0, -12.0, 0.3, (0.0, 0.0), 3, (0, 256, 699)),
    "order1-on-axis-rows-thin": (0.0, 1, 0.6, -0.3, 0.0, (0.0, 0.0), 1, (0, 256, 699)),
}


@pytest.mark.parametrize("case", list(GRAD_CASES))
def test_backward_matches_autograd_through_the_composition(case):
    import cheetah_amd as ca

    length, order, knl, ksl, tilt, mis, n, on_axis = GRAD_CASES[case]
    base = make_beam(F64, 700, 1e-3)
    start = base.particles.clone()
    for row in on_axis:
        start[row, 0] = start[row, 2] = 0.0                      # x = y = 0 exactly, in front of a thin or at the first drift's start
    W = torch.randn(700, 7, generator=torch.Generator().manual_seed(9), dtype=F64).cuda()

    def gradients(track, names):
        values = {"particles": start.clone(), "energy": T(1e8), "length": T(length), "knl": T(knl), "ksl": T(ksl), "tilt": T(tilt),
                  "misalignment": T(list(mis)), "tilt_out": T(tilt), "misalignment_out": T(list(mis))}
        leaves = {k: values[k].requires_grad_(True) for k in names}
        beam = ca.ParticleBeam(leaves["particles"], leaves["energy"], s=base.s, species=base.species)
        out = track(beam, leaves)
        loss = (out.particles * W).sum() + 1e-9 * out.energy
        loss.backward()
        return {k: v.grad.cpu().numpy() for k, v in leaves.items()}, float(loss.detach())

    def element(beam, p):
        el = ca.Multipole(p["length"], order, knl=p["knl"], ksl=p["ksl"], tilt=p["tilt"], misalignment=p["misalignment"], num_steps=n, **_kw(F64))
        return el.track(beam)

    names = ["particles", "energy", "length", "knl", "ksl", "tilt", "misalignment"]
    got, loss = gradients(element, names)
    parts, loss_c = gradients(lambda beam, p: composed(beam, p["length"], order, p["knl"], p["ksl"], p["tilt"], p["tilt_out"],
                                                       p["misalignment"], p["misalignment_out"], n), names + ["tilt_out", "misalignment_out"])
    assert abs(loss - loss_c) <= 1e-11 * abs(loss_c)
    want = {k: parts[k] for k in names}
    want["tilt"] = parts["tilt"] + parts["tilt_out"]
    want["misalignment"] = parts["misalignment"] + parts["misalignment_out"]
    terms = {"tilt": np.abs(parts["tilt"]).max(), "misalignment": np.abs(parts["misalignment"]).max()}
    for name in names:
        scale = np.abs(want[name]).max()
        if name in terms and scale <= 1e-6 * terms[name]:
            scale = terms[name]                                  # two terms that cancel: measured against the terms (module docstring)
            print(case, name, "is a sum of cancelling terms of magnitude", scale)
        rel = np.abs(got[name] - want[name]).max() / scale
        print(case, name, "largest gradient", scale, "relative difference", rel)
        assert scale > 0 and rel <= 1e-9, (name, rel)
    for row in on_axis:                                          # the rows on the axis by themselves: no lost derivative at x = y = 0
        scale = np.abs(want["particles"][row]).max()
        rel = np.abs(got["particles"][row] - want["particles"][row]).max() / scale
        print(case, "row", row, "on the axis: relative difference", rel)
        assert scale > 0 and rel <= 1e-9, (row, rel)


# ---- 5. symplecticity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
def test_the_map_is_symplectic(n):
    import cheetah_amd as ca

    x = make_beam(F64, 4, 5e-3, seed=21).particles
    quad = ca.Quadrupole(T(0.2), k1=T(3.0), tilt=T(0.3), misalignment=T([1e-3, -5e-4]), num_steps=n, **DKD, **_kw(F64))
    r_quad = symplectic_residual(quad, x)
    r_oct = symplectic_residual(multipole(F64, 0.2, 3, 2e4, -1e4, 0.3, (1e-3, -5e-4), n), x)
    print("num_steps", n, "residual: Quadrupole", r_quad, "Multipole of order 3", r_oct)
    assert r_quad < 1e-9
    assert r_oct <= max(10 * r_quad, 1e-12)


# ---- 6. float32 ---------------------------------------------------------------------------------------------------------------------------
def equal_rms_octupole_strength(beam64, k2l):
    """knl of an octupole whose kick has the rms size of the sextupole's k2 L on this beam: |k2 L u^2 / 2| against |knl u^3 / 6|."""
    u = torch.complex(beam64.particles[:, 0], beam64.particles[:, 2]).abs()
    return abs(k2l) * float((u ** 4).mean().sqrt() / 2) / float((u ** 6).mean().sqrt() / 6)


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("tilt", [0.0, 0.3], ids=["upright", "tilted"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("precision", ["mixed", "storage"])
def test_float32_modes_stay_within_four_sextupole_errors(precision, n, tilt, order):
    import cheetah_amd as ca

    beam = make_beam(F32, 700, 1e-3)
    beam64 = ca.ParticleBeam(beam.particles.to(F64), beam.energy.to(F64), s=beam.s.to(F64), species=beam.species)     # (one mass for both)
    sext = sextupole(F32, 0.2, 100.0, tilt, (0.0, 0.0), n)
    knl = 20.0 if order == 2 else equal_rms_octupole_strength(beam64, 20.0)
    mult = multipole(F32, 0.2, order, knl, 0.0, tilt, (0.0, 0.0), n)
    errors = {}
    for name, el, cls, extra in (("Sextupole", sext, ca.Sextupole, {}), ("Multipole", mult, ca.Multipole, {"order": order})):
        el.dkd_precision = precision
        want = as_float64(el, cls, **extra).track(beam64).particles
        got = el.track(beam).particles
        assert got.dtype == F32
        errors[name] = np.abs(got.cpu().numpy().astype(np.float64) - want.cpu().numpy())[:, :6].max(axis=0) / \
            np.abs(want.cpu().numpy())[:, :6].max(axis=0)
        print(precision, n, tilt, "order", order, "knl", knl, name, "error per column / the column's largest magnitude", errors[name])
    assert (errors["Multipole"] <= 4 * errors["Sextupole"]).all(), errors


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("mis", [(0.0, 0.0), (1e-3, -5e-4)], ids=["on-axis", "misaligned"])
@pytest.mark.parametrize("n", [1, 3])
def test_double_precision_on_a_float32_beam_is_the_float64_result_rounded(n, mis, order):
    import cheetah_amd as ca

    beam = make_beam(F32, 700, 1e-3)
    beam64 = ca.ParticleBeam(beam.particles.to(F64), beam.energy.to(F64), s=beam.s.to(F64), species=beam.species)     # (one mass for both)
    k = complex(-0.4, 0.5) * 1e-4 * 1000.0 ** order              # kicks of some 1e-5 rad on a beam of 1 mm
    mult = multipole(F32, 0.2, order, k.real, k.imag, 0.3, mis, n)
    mult.dkd_precision = "double"
    want = as_float64(mult, ca.Multipole, order=order).track(beam64).particles.to(F32)
    assert same_bits(mult.track(beam).particles, want)
    if mis != (0.0, 0.0):                                        # a shifted Multipole in "mixed": evaluated in float64 as well
        mult.dkd_precision = "mixed"
        assert same_bits(mult.track(beam).particles, want)


# ---- 7. batch -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("order", [1, 3])
def test_a_vector_of_strengths_is_three_scalar_tracks(order, dt):
    import cheetah_amd as ca

    beam = make_beam(dt, 257, 1e-3)
    strengths = [0.02 * 1000.0 ** order, 0.0, -0.007 * 1000.0 ** order]
    ksl = -5e-3 * 1000.0 ** order
    el = ca.Multipole(T(0.2, dt), order, knl=T(strengths, dt), ksl=T(ksl, dt), tilt=T(0.1, dt), num_steps=3, **_kw(dt))
    out = el.track(beam)
    assert out.particles.shape == (3, 257, 7)
    for i, knl in enumerate(strengths):
        want = multipole(dt, 0.2, order, knl, ksl, 0.1, n=3).track(beam)
        assert same_bits(out.particles[i], want.particles), i
        assert same_bits(out.energy.reshape(-1)[0], want.energy)


# ---- 8. fast paths ------------------------------------------------------------------------------------------------------------------------
def lattice(dt, precision):
    """[Q, D, M (order 3), D, Q, Dipole, M (order 1, skew, thin), RFCavity], drift-kick-drift throughout."""
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: T(v, dt)  # noqa: E731
    els = [ca.Quadrupole(t(0.2), k1=t(2.0), tilt=t(0.01), misalignment=t([2e-5, -1e-5]), num_steps=1, name="qf", **DKD, **kw),
           ca.Drift(t(0.5), name="d1", **DKD, **kw),
           multipole(dt, 0.1, 3, 2e4, -1e4, 0.0, (0.0, 0.0), 3, name="oct"),
           ca.Drift(t(0.4), name="d2", **DKD, **kw),
           ca.Quadrupole(t(0.2), k1=t(-2.0), num_steps=3, name="qd", **DKD, **kw),
           ca.Dipole(t(0.3), angle=t(0.004), dipole_e1=t(0.001), dipole_e2=t(0.002), fringe_integral=t(0.5), gap=t(0.02), fringe_at="both",
                     name="bend", **DKD, **kw),
           multipole(dt, 0.0, 1, 0.0, 0.05, 0.2, (1e-4, -2e-4), 1, name="skew"),
           ca.RFCavity(t(0.3), voltage=t(1e6), phase=t(0.13), frequency=t(480e6), name="rf", **kw)]
    for e in els:
        e.dkd_precision = precision
    return ca.Segment(els)


@pytest.mark.parametrize("n", [255, 700])
@pytest.mark.parametrize("precision,dt", MODES, ids=MODE_IDS)
def test_segment_track_is_one_chain_call_with_the_elements_bits(precision, dt, n, monkeypatch):
    from cheetah_amd import _ops

    seg, beam = lattice(dt, precision), make_beam(dt, n, 1e-3)
    want = beam
    for e in seg.elements:
        want = e.track(want)
    calls, orig = [], _ops.dkd_chain
    monkeypatch.setattr(_ops, "dkd_chain", lambda *a, **k: (calls.append((list(a[0]), a[3] and list(a[3]))), orig(*a, **k))[1])
    for _ in range(2):                                           # the second track: the cached run
        got = seg.track(beam)
        assert same_bits(got.particles, want.particles) and same_bits(got.energy, want.energy) and same_bits(got.s, want.s)
    kinds, orders = [1, 0, 8, 0, 1, 2, 8, 6], [3, 3, 3, 3, 3, 3, 1, 0]        # (the orders of the two Multipoles travel as fringe_at)
    assert calls == [(kinds, orders), (kinds, None)]             # (the cached run hands back its argument arrays)
    assert torch.isfinite(got.particles).all()


def ring(dt, precision, which="six"):
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: T(v, dt)  # noqa: E731
    if which == "one":
        els = [multipole(dt, 0.3, 3, 2e3, -1e3, 0.1, (0.0, 0.0), 3, name="m1")]
    else:                                                        # a FODO cell with a Multipole behind each quadrupole
        els = [ca.Quadrupole(t(0.2), k1=t(2.0), num_steps=1, name="qf", **DKD, **kw), multipole(dt, 0.1, 3, 2e3, -1e3, 0.0, (0.0, 0.0), 3, name="m1"),
               ca.Drift(t(0.5), name="d1", **DKD, **kw), ca.Quadrupole(t(0.2), k1=t(-2.0), num_steps=3, name="qd", **DKD, **kw),
               multipole(dt, 0.0, 1, 0.0, 0.01, 0.2, (1e-4, -2e-4), 1, name="m2"), ca.Drift(t(0.9), name="d2", **DKD, **kw)]
    for e in els:
        e.dkd_precision = precision
    return ca.Segment(els)


@pytest.mark.parametrize("which", ["six", "one"])
@pytest.mark.parametrize("precision,dt", MODES, ids=MODE_IDS)
def test_fused_turns_are_the_general_loops(precision, dt, which, monkeypatch):
    """An aperture of 5 mm on a beam of 3 mm: the large amplitudes are lost, on several turns."""
    import cheetah_amd as ca
    from cheetah_amd import _ops

    r, beam = ring(dt, precision, which), turn_beam(dt, 3e-3)
    aperture = T([5e-3, 5e-3], dt)
    kinds, orig = [], _ops.dkd_turns
    monkeypatch.setattr(_ops, "dkd_turns", lambda *a, **k: (kinds.append(list(a[0][0])), orig(*a, **k))[1])
    general = r.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=3, fused=False)
    assert kinds == []
    fused = r.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=3, fused=True)
    assert kinds == [[1, 8, 0, 1, 8, 0] if which == "six" else [8]]
    lost = general.lost_turn.cpu().numpy()
    print(which, "lost", (lost > 0).sum(), "of 700 on turns", np.unique(lost))
    assert (lost > 0).any() and (lost == 0).any()
    assert np.array_equal(fused.lost_turn.cpu().numpy(), lost)
    assert same_bits_nan_for_nan(fused.outgoing.particles, general.outgoing.particles.cpu().numpy())
    for a, b in ((fused.outgoing.energy, general.outgoing.energy), (fused.outgoing.s, general.outgoing.s),
                 (fused.outgoing.survival_probabilities, general.outgoing.survival_probabilities), (fused.turns, general.turns)):
        assert same_bits(a, b)
    assert same_bits_nan_for_nan(fused.particles, general.particles.cpu().numpy())
    ref = run_loop(r, beam, TURNS)                               # the plain loop over `track`: what the records are restated from
    check_records(fused, ref, lost, 5, 3)
    check_records(general, ref, lost, 5, 3)
    assert same_bits(r.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=3).sums, fused.sums)     # fused=None: fused
    # chunked launches: two turns of the six-item ring (twelve of the single Multipole) per launch
    launches = []
    monkeypatch.setattr(_ops, "dkd_turns", lambda *a, **k: (launches.append(a[12]), orig(*a, **k))[1])
    monkeypatch.setattr(ca.particles.turns, "_MAX_ITEM_STEPS", 12)
    chunked = r.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=3, fused=True)
    assert launches == ([2] * 18 + [1] if which == "six" else [12, 12, 12, 1])
    for a, b in zip(outputs(fused), outputs(chunked)):
        assert same_bits(a, b)


def test_a_ring_without_a_multipole_still_takes_the_fused_ring(monkeypatch):
    import cheetah_amd as ca
    from cheetah_amd import _ops

    r = ring(F32, "mixed")
    plain = ca.Segment([ca.Drift(e.length.clone(), name=e.name, **DKD, **_kw(F32)) if isinstance(e, ca.Multipole) else e.clone()
                        for e in r.elements if not (isinstance(e, ca.Multipole) and float(e.length) == 0.0)])
    calls, orig = [], _ops.dkd_turns
    monkeypatch.setattr(_ops, "dkd_turns", lambda *a, **k: (calls.append((list(a[0][0]), list(a[0][2]))), orig(*a, **k))[1])
    tbt = plain.track_turns(make_beam(F32, 700, 1e-3), 3)
    assert calls == [([1, 0, 0, 1, 0], [1, 1, 1, 3, 1])] and not tbt.lost_turn.any()
    want = make_beam(F32, 700, 1e-3)
    for _ in range(3):
        for e in plain.elements:
            want = e.track(want)
    assert same_bits(tbt.outgoing.particles, want.particles)


def test_fused_turns_with_multipoles_do_not_synchronise(monkeypatch):
    import cheetah_amd as ca
    from cheetah_amd import _ops

    r = ring(F32, "mixed")
    beam = make_beam(F32, 1000, 1e-3)
    aperture = T([2e-3, 2e-3], F32)
    assert len(sync_warnings(lambda: torch.tensor(1.0, device="cuda"), warm=0)) == 1       # the switch sees what it should see
    monkeypatch.setattr(ca.particles.turns, "_MAX_ITEM_STEPS", 24)                       # six items, 4 turns per launch: 3 launches
    launches, orig = [], _ops.dkd_turns
    monkeypatch.setattr(_ops, "dkd_turns", lambda *a, **k: (launches.append(a[12]), orig(*a, **k))[1])
    hits = sync_warnings(lambda: r.track_turns(beam, 10, record_every=3, aperture=aperture, record_first=2, fused=True))
    assert launches[-3:] == [4, 4, 2]                                                    # the fused path, in three chunks
    assert not hits, [(w.filename, w.lineno) for w in hits]


# ---- 9. physics: amplitude detuning -----------------------------------------------------------------------------------------------------
def detuning_ring(knl):
    """A thin octupole at the symmetry point of a FODO cell (alpha = 0 there), 100 MeV electrons, float64."""
    import cheetah_amd as ca

    kw = _kw(F64)
    q = lambda L, k1, name: ca.Quadrupole(T(L), k1=T(k1), num_steps=1, name=name, **DKD, **kw)  # noqa: E731
    return ca.Segment([multipole(F64, 0.0, 3, knl, 0.0, name="oct"), q(0.1, 2.0, "qf1"), ca.Drift(T(0.7), name="d1", **DKD, **kw),
                       q(0.2, -2.0, "qd"), ca.Drift(T(0.7), name="d2", **DKD, **kw), q(0.1, 2.0, "qf2")])


def one_turn_jacobian(r):
    """The 6 x 6 Jacobian of one turn at the origin from six backward passes."""
    import cheetah_amd as ca

    rows = []
    x0 = torch.zeros(1, 7, **_kw(F64))
    x0[0, 6] = 1.0
    for i in range(6):
        p = x0.clone().requires_grad_(True)
        out = r.track(ca.ParticleBeam(p, T(1e8), species=ca.Species("electron", **_kw(F64))))
        out.particles[0, i].backward()
        rows.append(p.grad[0, :6].cpu().numpy())
    return np.stack(rows)


def test_a_thin_octupole_detunes_with_amplitude():
    import cheetah_amd as ca

    knl, turns = 500.0, 512
    J = one_turn_jacobian(detuning_ring(knl))
    M = J[:2, :2]
    mu = math.acos((M[0, 0] + M[1, 1]) / 2)
    if M[0, 1] < 0:
        mu = 2 * math.pi - mu
    beta, alpha, nu0 = M[0, 1] / math.sin(mu), (M[0, 0] - M[1, 1]) / (2 * math.sin(mu)), mu / (2 * math.pi)
    print("beta_x", beta, "alpha_x", alpha, "nu_0", nu0)
    assert abs(beta - 6.367) <= 2e-3 and abs(nu0 - 0.05313) <= 2e-5 and abs(alpha) <= 1e-9
    amplitudes = np.array([0.25e-3, 1e-3, 2e-3, 3e-3, 4e-3])
    x = torch.zeros(5, 7, **_kw(F64))
    x[:, 0], x[:, 6] = torch.from_numpy(amplitudes).cuda(), 1.0
    beam = ca.ParticleBeam(x, T(1e8), species=ca.Species("electron", **_kw(F64)))
    action = amplitudes ** 2 / (2 * beta)
    predicted = knl * beta ** 2 / (16 * math.pi)
    slopes = {}
    for strength in (knl, 0.0):
        tbt = detuning_ring(strength).track_turns(beam, turns, record_first=5, fused=True)
        assert not tbt.lost_turn.any()
        nu = tbt.tunes(planes=("x",)).tune.reshape(5).cpu().numpy()
        slopes[strength] = np.polyfit(action, nu, 1)[0]
        print("knl", strength, "tunes", nu, "slope", slopes[strength], "predicted", predicted * strength / knl)
    assert abs(slopes[knl] - predicted) <= 0.02 * predicted, (slopes[knl], predicted)
    assert abs(slopes[0.0]) <= 1e-3 * predicted, (slopes[0.0], predicted)
