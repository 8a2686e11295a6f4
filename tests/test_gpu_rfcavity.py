"""The RFCavity on the GPU (CHX_DKD_RFCAVITY): half a drift, the energy kick |n_q| V sin(2 pi (phase - f t)), half a drift.

1. golden    the float64 kernel against tests/golden/dkd_rfcavity.npz (the map composed from the reference's bmadx functions with
             the sine taken directly): 1e-12 of each column's largest magnitude, NaN where the stored row is NaN.
2. V = 0     two half Drifts: 1e-14 per column against `Drift(L)`, the energy's bits.
3. backward  `backward()` against torch autograd through the float64 restatement of tests/test_rfcavity_host.py on the CPU:
             particles, energy and the four settings, 1e-9 of each gradient's largest magnitude.
4. symplectic  J^T S J - S as for the Sextupole, against the drift-kick-drift Quadrupole of that test.
5. float32   "mixed" = "double" bit for bit (the kind is evaluated in float64), "double" = the float64 result rounded, "storage"
             against the float64 evaluation within 4 x the error of a drift-kick-drift Quadrupole of the same length.
6. fast paths  `Segment.track` (one chx_dkd_chain_mixed call) and `track_turns(fused=True)` (chx_dkd_turns) against the element-by-
             element loops, bit for bit.
7. physics   the synchrotron tune of a small ring from 1024 tracked turns against the eigen-tune of the one-turn Jacobian; the
             unstable zero crossing; the bucket height.

N from {1, 255, 257, 700} (a tile is 256 rows)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_dkd_sextupole import column_error, sextupole, symplectic_residual  # (helpers only)
from tests.test_gpu_dkd_sextupole import make_beam as sextupole_beam  # (helper only)
from tests.test_gpu_track_turns import bits, same_bits  # (helpers only)
from tests.test_gpu_track_turns_dkd import drifting_energy, reference_sums, run_loop, same_bits_nan_for_nan  # (helpers only)
from tests.test_rfcavity_host import restated_map  # (helper only: the map in float64 torch)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dkd_rfcavity.npz")
F64, F32 = torch.float64, torch.float32
DKD = {"tracking_method": "drift_kick_drift"}
C_LIGHT = 299792458.0
M_E = 510998.95069
MODES = [("double", F32), ("storage", F32), ("mixed", F32), ("mixed", F64)]
MODE_IDS = ["f32-double", "f32-storage", "f32-mixed", "f64"]


def _kw(dt):
    return {"dtype": dt, "device": "cuda"}


def T(v, dt=F64):
    return torch.tensor(v, **_kw(dt))


def cavity(dt, length, voltage, phase, frequency, **extra):
    import cheetah_amd as ca

    return ca.RFCavity(T(length, dt), voltage=T(voltage, dt), phase=T(phase, dt), frequency=T(frequency, dt), **extra, **_kw(dt))


def make_beam(dt, n=700, sigma_tau=1e-2, seed=3, energy=1e8):
    """sigma_x = sigma_y = 1 mm, sigma_tau = `sigma_tau`, sigma_delta = 2e-3, electrons; drawn in float64 on the CPU, rounded to dt."""
    import cheetah_amd as ca

    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 7, generator=g, dtype=F64) * torch.tensor([1e-3, 2e-5, 1e-3, 2e-5, sigma_tau, 2e-3, 0.0], dtype=F64)
    x[:, 6] = 1.0
    return ca.ParticleBeam(x.to(**_kw(dt)), T(energy, dt), s=T(0.25, dt), species=ca.Species("electron", **_kw(dt)))


# ---- 1. golden ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


GOLDEN_NAMES = ["electron_phase0_L0", "electron_phase0_L0.3", "electron_phase0.5_L0", "electron_phase0.5_L0.3", "electron_phase0.13_L0",
                "electron_phase0.13_L0.3", "proton_phase0.13_L0", "proton_phase0.13_L0.3", "proton_phase0.5_L0.3"]


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_float64_kernel_matches_the_reference_composition(name, n):
    import cheetah_amd as ca

    g = golden()
    assert sorted(GOLDEN_NAMES) == sorted(str(s) for s in g["names"])
    length, voltage, phase, frequency = g[f"{name}_params"]
    sp = str(g[f"{name}_species"])
    mass, charge = g[f"{sp}_species"]
    energy = float(g[f"{sp}_energy"])
    species = ca.Species("custom", num_elementary_charges=T(float(charge)), mass_eV=T(float(mass)), **_kw(F64))
    el = cavity(F64, length, voltage, phase, frequency)
    for tag in g["beams"]:
        beam = ca.ParticleBeam(T(g[f"{sp}_in_{tag}"][:n]), T(energy), species=species)
        out = el.track(beam)
        got, want = out.particles.cpu().numpy(), g[f"{name}_{tag}_out"]
        assert np.array_equal(np.isnan(got), np.isnan(want[:n])), (name, tag, "NaN in other places")
        if n == 257 and tag == "long" and name in ("electron_phase0.13_L0", "proton_phase0.13_L0.3"):
            assert np.isnan(got[256]).tolist() == [True, False, True, False, True, True, False]      # the row below its rest mass
        live, live_n = ~np.isnan(want).any(axis=1), ~np.isnan(want[:n]).any(axis=1)
        err = np.abs(got[live_n] - want[:n][live_n])[:, :6].max(axis=0) / np.abs(want[live])[:, :6].max(axis=0)
        print(name, tag, n, "error per column / the column's largest magnitude", err)
        assert (err <= 1e-12).all(), (name, tag, err)
        assert (out.particles[:, 6] == 1).all()
        assert abs(float(out.energy) - float(g[f"{name}_{tag}_energy_out"])) <= 4 * 2.0 ** -52 * energy
        assert float(out.s) == float(length)


# ---- 2. zero voltage ------------------------------------------------------------------------------------------------------------------
def test_zero_voltage_is_a_drift():
    import cheetah_amd as ca

    beam = make_beam(F64, 257)
    want = ca.Drift(T(0.3), **DKD, **_kw(F64)).track(beam)
    el = cavity(F64, 0.3, 0.0, 0.13, 480e6)
    assert not el.is_active
    out = el.track(beam)
    err = column_error(out.particles, want.particles)
    print("V = 0:", err)
    assert (err <= 1e-14).all(), err                             # up to rounding: two pieces of the one drift
    assert same_bits(out.energy, want.energy)
    assert same_bits(out.s, want.s)


# ---- 3. backward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [0.0, 0.3])
def test_backward_matches_autograd_through_the_restated_map(length):
    import cheetah_amd as ca

    n = 700
    base = make_beam(F64, n, sigma_tau=0.2)                      # |f t| up to 1: the gradient passes through the reduction
    W = torch.randn(n, 7, generator=torch.Generator().manual_seed(9), dtype=F64)
    values = {"particles": base.particles.cpu(), "energy": torch.tensor(1e8, dtype=F64), "length": torch.tensor(length, dtype=F64),
              "voltage": torch.tensor(1e6, dtype=F64), "phase": torch.tensor(0.13, dtype=F64), "frequency": torch.tensor(480e6, dtype=F64)}

    def gradients(device, track):
        leaves = {k: v.clone().to(device).requires_grad_(True) for k, v in values.items()}
        out, energy = track(leaves)
        loss = (out * W.to(device)).sum() + 1e-9 * energy
        loss.backward()
        return {k: v.grad.cpu().numpy() for k, v in leaves.items()}, float(loss.detach())

    def element(p):
        el = ca.RFCavity(p["length"], voltage=p["voltage"], phase=p["phase"], frequency=p["frequency"], **_kw(F64))
        out = el.track(ca.ParticleBeam(p["particles"], p["energy"], s=base.s, species=base.species))
        return out.particles, out.energy

    def restated(p):
        return restated_map(p["particles"], p["energy"], torch.tensor(M_E, dtype=F64), -1.0, p["length"], p["voltage"], p["phase"], p["frequency"])

    got, loss = gradients("cuda", element)
    want, loss_c = gradients("cpu", restated)
    assert abs(loss - loss_c) <= 1e-11 * abs(loss_c)
    for name in want:
        scale = np.abs(want[name]).max()
        rel = np.abs(got[name] - want[name]).max() / scale
        print("L", length, name, "largest gradient", scale, "relative difference", rel)
        assert scale > 0 and rel <= 1e-9, (name, rel)


# ---- 4. symplecticity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [0.0, 0.3])
def test_the_map_is_symplectic(length):
    import cheetah_amd as ca

    x = sextupole_beam(F64, 4, 5e-3, seed=21).particles.clone()
    x[:, 4] = T([0.0, 0.05, -0.3, 1.1])                          # tau from the crest to more than a period (f tau / c = 1.8)
    quad = ca.Quadrupole(T(0.2), k1=T(3.0), tilt=T(0.3), misalignment=T([1e-3, -5e-4]), num_steps=1, **DKD, **_kw(F64))
    r_quad = symplectic_residual(quad, x)
    r_cav = symplectic_residual(cavity(F64, length, 1e6, 0.13, 480e6), x)
    print("L", length, "residual: Quadrupole", r_quad, "RFCavity", r_cav)
    assert r_quad < 1e-9                                         # (S is the right matrix: with +J2 for (tau, delta) this is 1e-4)
    assert r_cav <= max(10 * r_quad, 1e-12)


# ---- 5. float32 -----------------------------------------------------------------------------------------------------------------------
def widened(el):
    """The cavity with its float32 settings widened to float64 (the same values)."""
    import cheetah_amd as ca

    return ca.RFCavity(el.length.to(F64), voltage=el.voltage.to(F64), phase=el.phase.to(F64), frequency=el.frequency.to(F64), **_kw(F64))


@pytest.mark.parametrize("length", [0.0, 0.3])
def test_mixed_is_double_and_double_is_the_float64_result_rounded(length):
    import cheetah_amd as ca

    beam = make_beam(F32, 700)
    beam64 = ca.ParticleBeam(beam.particles.to(F64), beam.energy.to(F64), s=beam.s.to(F64), species=beam.species)     # (one mass for both)
    el = cavity(F32, length, 1e6, 0.13, 480e6)
    want = widened(el).track(beam64).particles.to(F32)
    el.dkd_precision = "double"
    double = el.track(beam)
    assert double.particles.dtype == F32 and same_bits(double.particles, want)
    el.dkd_precision = "mixed"
    mixed = el.track(beam)
    assert same_bits(mixed.particles, double.particles) and same_bits(mixed.energy, double.energy)


def test_storage_stays_within_four_quadrupole_errors():
    """x, px, y, py see only the two half drifts. tau and delta pass the (tau, delta) <-> (z, pz) conversions like every element,
    and in between the kick rounds E_new = E_old + dE, pc_new and pz once each in float32 — three roundings of 2^-24 of the
    energy on top of the conversions' own. The measured ratios are printed per column."""
    import cheetah_amd as ca

    beam = make_beam(F32, 700)
    beam64 = ca.ParticleBeam(beam.particles.to(F64), beam.energy.to(F64), s=beam.s.to(F64), species=beam.species)
    quad = ca.Quadrupole(T(0.3, F32), k1=T(3.0, F32), num_steps=1, **DKD, **_kw(F32))
    quad64 = ca.Quadrupole(T(0.3), k1=T(3.0), num_steps=1, **DKD, **_kw(F64))
    cav = cavity(F32, 0.3, 1e6, 0.13, 480e6)
    errors = {}
    for name, el, el64 in (("Quadrupole", quad, quad64), ("RFCavity", cav, widened(cav))):
        el.dkd_precision = "storage"
        want = el64.track(beam64).particles
        got = el.track(beam).particles
        assert got.dtype == F32
        errors[name] = column_error(got, want)
        print("storage", name, "error per column / the column's largest magnitude", errors[name])
    print("storage: RFCavity / Quadrupole per column", errors["RFCavity"] / errors["Quadrupole"])
    assert (errors["RFCavity"] <= 4 * errors["Quadrupole"]).all(), errors


# ---- 6. fast paths --------------------------------------------------------------------------------------------------------------------
def lattice(dt, precision):
    """[Quadrupole, Drift, Dipole, RFCavity, Sextupole, Drift], drift-kick-drift throughout."""
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: T(v, dt)  # noqa: E731
    els = [ca.Quadrupole(t(0.2), k1=t(2.0), tilt=t(0.01), misalignment=t([2e-5, -1e-5]), num_steps=1, name="qf", **DKD, **kw),
           ca.Drift(t(0.5), name="d1", **DKD, **kw),
           ca.Dipole(t(0.3), angle=t(0.004), dipole_e1=t(0.001), dipole_e2=t(0.002), fringe_integral=t(0.5), gap=t(0.02), fringe_at="both",
                     name="bend", **DKD, **kw),
           cavity(dt, 0.3, 1e6, 0.13, 480e6, name="rf"),
           sextupole(dt, 0.1, 40.0, 0.0, (0.0, 0.0), 3, name="s1"),
           ca.Drift(t(0.4), name="d2", **DKD, **kw)]
    for e in els:
        e.dkd_precision = precision
    return ca.Segment(els)


@pytest.mark.parametrize("n", [255, 700])
@pytest.mark.parametrize("precision,dt", MODES, ids=MODE_IDS)
def test_segment_track_is_one_chain_call_with_the_elements_bits(precision, dt, n, monkeypatch):
    from cheetah_amd import _ops

    seg, beam = lattice(dt, precision), make_beam(dt, n)
    want = beam
    for e in seg.elements:
        want = e.track(want)
    calls, orig = [], _ops.dkd_chain
    monkeypatch.setattr(_ops, "dkd_chain", lambda *a, **k: (calls.append(list(a[0])), orig(*a, **k))[1])
    for _ in range(2):                                           # the second track: the cached run
        got = seg.track(beam)
        assert same_bits(got.particles, want.particles) and same_bits(got.energy, want.energy) and same_bits(got.s, want.s)
    assert calls == [[1, 0, 2, 6, 5, 0]] * 2
    assert torch.isfinite(got.particles).all()


RING_TURNS = 40
RING_PHASE = 0.0


def ring(dt, precision, thin=False):
    """[RFCavity, Quadrupole, Sextupole, Drift, Quadrupole, Dipole, Drift]: the cavity first, so that the phase at which a row
    meets it on its first turn is known on the host."""
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: T(v, dt)  # noqa: E731
    els = [cavity(dt, 0.0 if thin else 0.3, 1e6, RING_PHASE, 480e6, name="rf"),
           ca.Quadrupole(t(0.2), k1=t(2.0), num_steps=1, name="qf", **DKD, **kw), sextupole(dt, 0.1, 40.0, 0.0, (0.0, 0.0), 3, name="s1"),
           ca.Drift(t(0.5), name="d1", **DKD, **kw), ca.Quadrupole(t(0.2), k1=t(-2.0), num_steps=3, name="qd", **DKD, **kw),
           ca.Dipole(t(0.3), angle=t(0.004), fringe_at="both", name="bend", **DKD, **kw), ca.Drift(t(0.9), name="d2", **DKD, **kw)]
    for e in els:
        e.dkd_precision = precision
    return ca.Segment(els)


def turn_beam(dt, energy=1e8, thin=False):
    """700 rows of 0.2 mm; row 5 starts 8 mm off the axis (the aperture is 5 mm); row 300 has 100 keV of kinetic energy and meets
    the cavity a quarter period behind the zero crossing, where it is decelerated by the full 1 MV: NaN on the first turn."""
    import cheetah_amd as ca

    g = torch.Generator().manual_seed(11)
    x = torch.randn(700, 7, generator=g, dtype=F64) * torch.tensor([2e-4, 1e-5, 2e-4, 1e-5, 1e-3, 1e-3, 0.0], dtype=F64)
    x[:, 6] = 1.0
    x[5, 0] = 8e-3
    p0c = math.sqrt(energy ** 2 - M_E ** 2)
    kinetic = 1e5
    pc = math.sqrt((M_E + kinetic) ** 2 - M_E ** 2)
    beta, beta0 = pc / (M_E + kinetic), p0c / energy
    # tau at the kick = tau_0 + the half drift's slip (L / 2)(1 / beta - 1 / beta0); there phase - f tau / c = -1/4
    x[300, :4] = 0.0
    x[300, 4] = (RING_PHASE + 0.25) * C_LIGHT / 480e6 - (0.0 if thin else 0.15) * (1.0 / beta - 1.0 / beta0)
    x[300, 5] = (M_E + kinetic - energy) / p0c
    gen = torch.Generator().manual_seed(5)
    charges = (torch.rand(700, generator=gen, dtype=F64) + 0.5).to(**_kw(dt)) * 1e-15
    survival = (torch.rand(700, generator=gen, dtype=F64) * 0.5 + 0.5).to(**_kw(dt))
    return ca.ParticleBeam(x.to(**_kw(dt)), T(energy, dt), particle_charges=charges, survival_probabilities=survival, s=T(0.25, dt),
                           species=ca.Species("electron", **_kw(dt)))


def outputs(tbt):
    return [tbt.outgoing.particles, tbt.outgoing.energy, tbt.outgoing.survival_probabilities, tbt.outgoing.s, tbt.lost_turn, tbt.turns,
            tbt.sums, tbt.particles]


def check_fused_against_general(r, beam, dt, monkeypatch, chunk=None):
    """`track_turns(fused=True)` against `fused=False`: particles, energy, path length, survival, lost_turn and probe rows bit for
    bit; the records of both against the float64 restatement from the plain loop over `track` (the bound of
    tests/test_gpu_track_turns_dkd.py). Returns the fused result and lost_turn."""
    import cheetah_amd as ca

    aperture = T([5e-3, 5e-3], dt)
    kwargs = {"record_every": 5, "aperture": aperture, "record_first": 3}
    general = r.track_turns(beam, RING_TURNS, fused=False, **kwargs)
    if chunk is not None:
        monkeypatch.setattr(ca.particles.turns, "_MAX_ITEM_STEPS", chunk)
    fused = r.track_turns(beam, RING_TURNS, fused=True, **kwargs)        # (raises without the feature: "... is not a drift-kick-drift ...")
    lost = general.lost_turn.cpu().numpy()
    print("lost", (lost > 0).sum(), "of 700 on turns", np.unique(lost), "row 5:", lost[5], "row 300:", lost[300])
    assert lost[5] > 0 and lost[300] == 1 and (lost == 0).sum() > 600
    assert np.isnan(general.outgoing.particles[300].cpu().numpy())[[0, 2, 4, 5]].all()          # frozen as the kick and the turn left it
    assert np.array_equal(fused.lost_turn.cpu().numpy(), lost)
    assert same_bits_nan_for_nan(fused.outgoing.particles, general.outgoing.particles.cpu().numpy())
    for a, b in ((fused.outgoing.energy, general.outgoing.energy), (fused.outgoing.s, general.outgoing.s),
                 (fused.outgoing.survival_probabilities, general.outgoing.survival_probabilities), (fused.turns, general.turns)):
        assert same_bits(a, b)
    assert fused.particles.shape == (RING_TURNS // 5, 3, 7)
    assert same_bits_nan_for_nan(fused.particles, general.particles.cpu().numpy())
    ref = run_loop(r, beam, RING_TURNS)                          # the plain loop over `track`: what the records are restated from
    assert same_bits(fused.outgoing.energy, ref["e"][RING_TURNS])
    alive = lost == 0
    assert same_bits(fused.outgoing.particles[torch.from_numpy(alive).cuda()], ref["x"][RING_TURNS][alive])
    for tbt in (fused, general):
        got = tbt.sums.cpu().numpy()
        for k, turn in enumerate(range(5, RING_TURNS + 1, 5)):
            want, bound = reference_sums(ref["x"], ref["w"], lost, turn)
            assert got[k, 0] == want[0], (turn, got[k, 0], want[0])
            assert (np.abs(got[k, 1:] - want[1:]) <= bound[1:]).all(), (turn, got[k], want)
    return fused, ref


@pytest.mark.parametrize("thin", [False, True], ids=["L0.3", "thin"])
@pytest.mark.parametrize("precision,dt", MODES, ids=MODE_IDS)
def test_fused_turns_are_the_general_loops(precision, dt, thin, monkeypatch):
    from cheetah_amd import _ops

    r, beam = ring(dt, precision, thin), turn_beam(dt, thin=thin)
    calls, orig = [], _ops.dkd_turns
    monkeypatch.setattr(_ops, "dkd_turns", lambda *a, **k: (calls.append(a[12]), orig(*a, **k))[1])
    whole, _ = check_fused_against_general(r, beam, dt, monkeypatch)
    assert calls == [RING_TURNS]
    # seven items: two turns per launch
    del calls[:]
    chunked, _ = check_fused_against_general(r, beam, dt, monkeypatch, chunk=14)
    assert calls == [2] * (RING_TURNS // 2)
    for a, b in zip(outputs(whole), outputs(chunked)):
        assert same_bits_nan_for_nan(a, b.cpu().numpy())


@pytest.mark.parametrize("precision,dt", [("mixed", F32), ("mixed", F64)], ids=["f32", "f64"])
def test_fused_turns_follow_a_drifting_reference_energy(precision, dt, monkeypatch):
    energy = drifting_energy(dt)
    assert energy is not None, "no energy found whose round trip goes on drifting on the device"
    r, beam = ring(dt, precision), turn_beam(dt, energy=energy)
    _, ref = check_fused_against_general(r, beam, dt, monkeypatch, chunk=14)
    starts = {bits(e).item() for e in ref["e"][:4]}
    print("turn-start energies of the first four turns:", len(starts), "bit patterns")
    assert len(starts) >= 2                                      # the energy moves from turn to turn: more than one block of constants


def test_a_ring_without_a_cavity_still_takes_the_fused_ring(monkeypatch):
    import cheetah_amd as ca
    from cheetah_amd import _ops

    r = ring(F32, "mixed")
    plain = ca.Segment([ca.Drift(T(0.3, F32), name="d0", **DKD, **_kw(F32))] + [e.clone() for e in r.elements[1:]])
    calls, orig = [], _ops.dkd_turns
    monkeypatch.setattr(_ops, "dkd_turns", lambda *a, **k: (calls.append(a[2]), orig(*a, **k))[1])
    tbt = plain.track_turns(make_beam(F32, 700, 1e-3), 3)
    assert calls == [7] and not tbt.lost_turn.any()


# ---- 7. the synchrotron tune ----------------------------------------------------------------------------------------------------------
CELLS, HARMONIC, Q_TARGET, TUNE_TURNS = 6, 400, 0.04, 1024


def small_ring(phase, voltage):
    """Six FODO cells [QF, D, B, D, QD, D, B, D] of 2.6 m with sector bends of 30 degrees (48 items, 15.6 m); the first Drift is the
    cavity, on harmonic 400. 100 MeV electrons are far above transition (the bends give a momentum compaction of about 0.3):
    phase 0 is the stable zero crossing."""
    import cheetah_amd as ca

    kw = _kw(F64)
    els = []
    for c in range(CELLS):
        for j, kind in enumerate("qdbdQdbd"):
            name = f"c{c}_{j}"
            if kind == "d" and len(els) == 1:
                f = ca.RFCavity.harmonic_frequency(CELLS * 2.6, HARMONIC, T(1e8))
                els.append(ca.RFCavity(T(0.3), voltage=T(voltage), phase=T(phase), frequency=f, name="rf", **kw))
            elif kind == "d":
                els.append(ca.Drift(T(0.3), name=name, **DKD, **kw))
            elif kind == "b":
                els.append(ca.Dipole(T(0.5), angle=T(2 * math.pi / (2 * CELLS)), name=name, **DKD, **kw))
            else:
                els.append(ca.Quadrupole(T(0.2), k1=T(3.0 if kind == "q" else -3.0), num_steps=1, name=name, **DKD, **kw))
    assert len(els) == 48 and sum(isinstance(e, ca.RFCavity) for e in els) == 1
    return ca.Segment(els)


def one_turn_jacobian(r):
    """The 6 x 6 Jacobian of one turn at the origin from six backward passes, as `symplectic_residual` takes it."""
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


def single(tau):
    import cheetah_amd as ca

    x = torch.zeros(1, 7, **_kw(F64))
    x[0, 4], x[0, 6] = tau, 1.0
    return ca.ParticleBeam(x, T(1e8), species=ca.Species("electron", **_kw(F64)))


def standard_map_bucket_height(a, A, k, turns=20000):
    """The largest |delta| of the orbit of delta' = delta - A sin(k tau), tau' = tau + a delta' that starts beside the unstable
    fixed point, at (k tau, delta) = (pi - 1e-4, 0): the height of the bucket of the turn-by-turn map. For a k A -> 0 it is the
    pendulum's 2 sqrt(A / (k a)); one kick per turn makes it higher by a k A / 24 of itself to leading order (0.15 % at Q_s = 0.03,
    1.1 % at 0.08)."""
    tau, delta, top = (math.pi - 1e-4) / k, 0.0, 0.0
    for _ in range(turns):
        delta -= A * math.sin(k * tau)
        tau += a * delta
        top = max(top, abs(delta))
    return top


def test_synchrotron_tune_bucket_and_unstable_phase():
    p0c = math.sqrt(1e16 - M_E ** 2)
    # the ring without voltage: its slip a (tau' = tau + a delta on the dispersive orbit) sets the voltage for Q_s = Q_TARGET
    J0 = one_turn_jacobian(small_ring(0.0, 0.0))
    eta = np.linalg.solve(np.eye(4) - J0[:4, :4], J0[:4, 5])
    a0 = J0[4, 5] + J0[4, :4] @ eta
    f = float(small_ring(0.0, 0.0).rf.frequency)
    k = 2 * math.pi * f / C_LIGHT
    voltage = 2 * p0c * (1 - math.cos(2 * math.pi * Q_TARGET)) / (a0 * k)
    print("V = 0: traces", np.trace(J0[0:2, 0:2]), np.trace(J0[2:4, 2:4]), "dispersion", eta, "slip a", a0, "f", f, "voltage", voltage)
    assert a0 > 0 and 1e3 < voltage < 1e6
    r = small_ring(0.0, voltage)
    J = one_turn_jacobian(r)
    tr_x, tr_y = np.trace(J[0:2, 0:2]), np.trace(J[2:4, 2:4])
    eig = np.linalg.eigvals(J)
    assert np.allclose(np.abs(eig), 1.0, atol=1e-9), np.abs(eig)             # all three planes stable
    tunes = np.abs(np.angle(eig)) / (2 * math.pi)
    Q_s = tunes.min()
    print("one-turn traces x, y:", tr_x, tr_y, "eigen-tunes", np.sort(tunes), "Q_s", Q_s)
    assert abs(tr_x) < 2 and abs(tr_y) < 2
    assert 0.03 <= Q_s <= 0.16
    # 1. the tune of a small oscillation
    phi = 1e-3
    tbt = r.track_turns(single(phi / k), TUNE_TURNS, record_first=1, fused=True)
    assert not tbt.lost_turn.any()
    measured = float(tbt.tunes(planes=("tau",)).tune.reshape(()))
    bound = 2 * Q_s * phi ** 2 / 16 + 10 * TUNE_TURNS ** -3.0      # the pendulum's amplitude shift + the documented resolution
    print("tune from", TUNE_TURNS, "turns:", measured, "difference", measured - Q_s, "bound", bound)
    assert abs(measured - Q_s) <= bound
    # 2. the other zero crossing is unstable: |tau| grows monotonically beyond 100 times its start
    away = small_ring(0.5, voltage).track_turns(single(phi / k), TUNE_TURNS, record_first=1, fused=True)
    tau = np.abs(away.particles[:, 0, 4].cpu().numpy())
    beyond = np.nonzero(tau > 100 * phi / k)[0]
    assert beyond.size > 0, tau.max()
    first = beyond[0]
    print("phase 0.5: |tau| passes 100 times its start on turn", first + 1)
    assert (np.diff(np.concatenate([[phi / k], tau[:first + 1]])) > 0).all()
    # 3. the bucket. To first order in the transverse coordinates a turn is the standard map delta' = delta - A sin(k tau),
    # tau' = tau + a delta' with A = |n_q| V / p0c, whose small-amplitude tune is cos(2 pi Q_s) = 1 - a k A / 2: that gives a from
    # Q_s, V and f. The orbit through (k tau, delta) = (3, 0) lies inside the bucket, at sin(3 / 2) = 0.9975 of its height.
    A = voltage / p0c
    a = 2 * (1 - math.cos(2 * math.pi * Q_s)) / (k * A)
    height = standard_map_bucket_height(a, A, k)
    wide = r.track_turns(single(3.0 / k), TUNE_TURNS, record_first=1, fused=True)
    assert not wide.lost_turn.any()
    delta = np.abs(wide.particles[:, 0, 5].cpu().numpy())
    print("a", a, "bucket height", height, "of the pendulum", 2 * math.sqrt(A / (k * a)), "largest |delta| from k tau = 3:", delta.max(), "=",
          delta.max() / height, "of it")
    assert delta.max() <= height
    assert delta.max() >= 0.9 * height                           # (and it does go round the bucket: a kick of another size would not)
    assert np.abs(wide.particles[:, 0, 4].cpu().numpy()).max() <= math.pi / k
