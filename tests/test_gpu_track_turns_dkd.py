"""Segment.track_turns on a ring of drift-kick-drift elements: the fused turn kernels (chx_dkd_turns) against the loop they
replace, `for _ in range(turns): beam = ring.track(beam)` — particles, reference ENERGY and path length bit for bit, also at an
energy that goes on drifting from element to element — and against a numpy float64 restatement of the records over that loop's
beams.

N = 700 particles: three tiles of 256 rows, the last one partial. Two rings, drift-kick-drift throughout:
  A  Quadrupole (tilted, shifted), Drift, Marker, Quadrupole (three steps), Drift — a FODO cell; the kernels without BEND;
  B  the same with two bends of a few mrad (a Dipole with both fringes, face angles, fint and gap; an RBend) — the BEND kernels.
The sums of a record are float64 sums of N terms taken in another order than numpy's: the bound is the worst case of such a sum,
N * 2^-52 * sum w |x_j| (sum w x_j^2 for the second moments)."""
import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_track_turns import EPS, bits, reference_losses, same_bits  # (helpers only)

pytestmark = pytest.mark.gpu

N = 700
TURNS = 37
#: (dkd_precision, dtype): the three arithmetic modes of a float32 beam, and a float64 beam (which ignores the mode)
MODES = [("double", torch.float32), ("storage", torch.float32), ("mixed", torch.float32), ("mixed", torch.float64)]
MODE_IDS = ["f32-double", "f32-storage", "f32-mixed", "f64"]
DTYPE_MODES = [("mixed", torch.float32), ("mixed", torch.float64)]
DTYPE_IDS = ["f32", "f64"]


def _kw(dt):
    return {"dtype": dt, "device": "cuda"}


def make_ring(dt, ring="A", precision=None, extra=None):
    """`precision` None leaves `dkd_precision` to the class. `extra`: an element put between the first Drift and the Marker."""
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    dkd = {"tracking_method": "drift_kick_drift"}
    els = [ca.Quadrupole(t(0.2), k1=t(2.0), tilt=t(0.01), misalignment=t([2e-5, -1e-5]), num_steps=1, name="qf", **dkd, **kw),
           ca.Drift(t(0.5), name="d1", **dkd, **kw)]
    if extra is not None:
        els.append(extra)
    els += [ca.Marker(name="mark", **kw), ca.Quadrupole(t(0.2), k1=t(-2.0), num_steps=3, name="qd", **dkd, **kw)]
    if ring == "B":
        els += [ca.Dipole(t(0.3), angle=t(0.004), dipole_e1=t(0.001), dipole_e2=t(0.002), fringe_integral=t(0.5), gap=t(0.02),
                          fringe_at="both", name="bend", **dkd, **kw),
                ca.RBend(t(0.3), angle=t(-0.004), rbend_e1=t(0.0005), name="rbend", **dkd, **kw), ca.Drift(t(0.5), name="d2", **dkd, **kw)]
    else:
        els.append(ca.Drift(t(1.1), name="d2", **dkd, **kw))
    if precision is not None:
        for e in els:
            e.dkd_precision = precision
    return ca.Segment(els)


def make_beam(dt, size=2e-4, bad_rows=(), energy=1e8):
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(11)
    beam = ca.ParticleBeam.from_parameters(num_particles=N, sigma_x=t(size), sigma_px=t(size / 20), sigma_y=t(size), sigma_py=t(size / 20),
                                           sigma_p=t(1e-3), energy=t(1e8), **kw)
    x = beam.particles.clone()
    for row in bad_rows:
        x[row, 0] = float("inf")
    gen = torch.Generator().manual_seed(5)                   # the weights of tests/test_gpu_track_turns.py
    charges = (torch.rand(N, generator=gen, dtype=torch.float64) + 0.5).to(**kw) * 1e-15
    survival = (torch.rand(N, generator=gen, dtype=torch.float64) * 0.5 + 0.5).to(**kw)
    return ca.ParticleBeam(x, t(energy), particle_charges=charges, survival_probabilities=survival, s=t(0.25), species=beam.species)


def run_loop(ring, beam, turns=TURNS):
    """The loop `track_turns` replaces: the beams after 0 .. turns turns as one (turns + 1, N, 7) array, the reference energy in
    front of turn 1 and behind every turn, the path length after one turn, the weights."""
    xs, es, s_one = [beam.particles.cpu().numpy()], [beam.energy.cpu().numpy()], None
    w = beam.particle_charges.cpu().numpy().astype(np.float64) * beam.survival_probabilities.cpu().numpy().astype(np.float64)
    s0 = beam.s.cpu().numpy()
    for turn in range(turns):
        beam = ring.track(beam)
        xs.append(beam.particles.cpu().numpy())
        es.append(beam.energy.cpu().numpy())
        if turn == 0:
            s_one = beam.s.cpu().numpy()
    xs, es = np.stack(xs), np.stack(es)
    xs.setflags(write=False)
    es.setflags(write=False)
    return {"x": xs, "e": es, "w": w, "s0": s0, "s_one": s_one}


@functools.lru_cache(maxsize=None)
def loop_reference(dt, ring, precision, size, bad_rows, energy=1e8):
    """Once per case, shared by the tests and never modified."""
    return run_loop(make_ring(dt, ring, precision), make_beam(dt, size, bad_rows, energy))


def reference_sums(xs, w, lost, turn):
    """The 14 sums of the record of `turn` in numpy float64, and the bound of each (see the module docstring)."""
    alive = (lost == 0) | (lost > turn)
    x = xs[turn][alive, :6].astype(np.float64)
    wa = w[alive]
    sums = np.concatenate([[alive.sum(), wa.sum()], (wa[:, None] * x).sum(axis=0), (wa[:, None] * x * x).sum(axis=0)])
    bound = N * EPS * np.concatenate([[0.0, wa.sum()], (wa[:, None] * np.abs(x)).sum(axis=0), (wa[:, None] * x * x).sum(axis=0)])
    return sums, bound


def same_bits_nan_for_nan(a, b):
    """Bit for bit wherever the loop's value `b` is a number, and a NaN exactly where the loop has a NaN. The rows that start with
    an infinite x come out of their first turn as NaNs, and IEEE 754 leaves the sign of a NaN result open: in "mixed" arithmetic
    the two kernels (dkd_chain_kernel, dkd_turns_kernel) were compiled to give tau = 0x7fc00000 and 0xffc00000 there. Everything
    that is a number, in those rows too, is compared by its bits."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def check_records(tbt, ref, lost, record_every, record_first):
    R = TURNS // record_every
    turns = np.arange(1, R + 1) * record_every
    assert tbt.turns.dtype == torch.int64 and np.array_equal(tbt.turns.cpu().numpy(), turns)
    got = tbt.sums.cpu().numpy()
    assert got.shape == (R, 14) and got.dtype == np.float64
    for r, turn in enumerate(turns):
        want, bound = reference_sums(ref["x"], ref["w"], lost, turn)
        print("record", turn, "max |got - want| / bound", np.max(np.abs(got[r, 1:] - want[1:]) / np.maximum(bound[1:], 1e-300)))
        assert got[r, 0] == want[0], (turn, got[r, 0], want[0])
        assert (np.abs(got[r, 1:] - want[1:]) <= bound[1:]).all(), (turn, got[r], want)
    if record_first:
        assert tbt.particles.shape == (R, record_first, 7)
        frozen = np.where(lost[:record_first] > 0, lost[:record_first], TURNS + 1)
        for r, turn in enumerate(turns):
            rows = np.stack([ref["x"][min(turn, frozen[k]), k] for k in range(record_first)])
            assert same_bits_nan_for_nan(tbt.particles[r], rows), turn
    else:
        assert tbt.particles is None


def check_against_loop(tbt, ref, num_turns, beam):
    """Particles, energy and path length of `num_turns` calls of `track`, bit for bit; nobody lost."""
    assert same_bits(tbt.outgoing.particles, ref["x"][num_turns])
    assert tbt.outgoing.energy.shape == () and same_bits(tbt.outgoing.energy, ref["e"][num_turns])
    s0, s_one = ref["s0"], ref["s_one"]
    assert same_bits(tbt.outgoing.s, s0 + s0.dtype.type(num_turns) * (s_one - s0))       # the documented one multiplication
    assert tbt.lost_turn.dtype == torch.int32 and not tbt.lost_turn.any()
    assert same_bits(tbt.outgoing.survival_probabilities, beam.survival_probabilities)
    assert same_bits(tbt.outgoing.particle_charges, beam.particle_charges)


def outputs(tbt):
    return [tbt.outgoing.particles, tbt.outgoing.energy, tbt.outgoing.survival_probabilities, tbt.outgoing.s, tbt.lost_turn, tbt.turns,
            tbt.sums, tbt.particles]


# ---- 1. bit for bit against the loop -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,dt", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("ring_kind", ["A", "B"])
@pytest.mark.parametrize("num_turns", [1, 2, 37])
def test_particles_energy_and_s_are_the_loops_bit_for_bit(precision, dt, ring_kind, num_turns):
    ref = loop_reference(dt, ring_kind, precision, 2e-4, ())
    ring, beam = make_ring(dt, ring_kind, precision), make_beam(dt)
    assert np.isfinite(ref["x"]).all()
    fused = ring.track_turns(beam, num_turns, fused=True)                                # (raises without the fused ring)
    check_against_loop(fused, ref, num_turns, beam)
    check_against_loop(ring.track_turns(beam, num_turns), ref, num_turns, beam)           # fused=None: the same path
    check_against_loop(ring.track_turns(beam, num_turns, fused=False), ref, num_turns, beam)
    assert same_bits(beam.particles, ref["x"][0]) and same_bits(beam.energy, ref["e"][0])  # the incoming beam is left alone


def test_fused_none_takes_the_fused_ring(monkeypatch):
    """fused=None on a qualifying ring runs chx_dkd_turns, not the loop."""
    from cheetah_amd import _ops

    calls, orig = [], _ops.dkd_turns
    monkeypatch.setattr(_ops, "dkd_turns", lambda *a, **k: (calls.append(a[2]), orig(*a, **k))[1])
    make_ring(torch.float32, "B", "mixed").track_turns(make_beam(torch.float32), 3)
    assert calls == [6]                                                                  # one call, six items (the Marker is skipped)


# ---- 2. a drifting reference energy -----------------------------------------------------------------------------------------------------
def round_trip(E, m):
    """What every drift-kick-drift element leaves of the reference energy (bmadx.py:49), restated in torch in E's dtype."""
    p0 = torch.sqrt(E * E - m * m)
    return torch.sqrt(p0 * p0 + m * m)


def turn_start_bits(ring, beam, turns):
    out = [bits(beam.energy).item()]
    for _ in range(turns - 1):
        beam = ring.track(beam)
        out.append(bits(beam.energy).item())
    return out


@functools.lru_cache(maxsize=None)
def drifting_energy(dt):
    """An energy (a Python float, exact in dt) whose turn-start energies in the plain loop over `track` take at least three
    distinct bit patterns within the first 4 turns of ring A, or None. Candidates: the two known from numpy, then 4096 values on
    either side of 2^25 and 2^26 eV (float32: neighbouring floats; float64: seeded uniform draws within 8192 eV). Shortlisted with
    the round trip restated in torch (ring A: four elements per turn), confirmed with the loop."""
    kw = _kw(dt)
    known = [33559016.0, 67095196.0] if dt == torch.float32 else [33553824.816828918, 67102260.188750185]
    parts = [torch.tensor(known, **kw)]
    gen = torch.Generator().manual_seed(3)
    for base in (2.0 ** 25, 2.0 ** 26):
        if dt == torch.float32:
            b = torch.tensor(base, dtype=torch.float32).view(torch.int32)
            parts.append((b + torch.arange(-4096, 4096, dtype=torch.int32)).view(torch.float32).to("cuda"))
        else:
            parts.append((base + (torch.rand(8192, generator=gen, dtype=torch.float64) - 0.5) * 16384.0).to("cuda"))
    cand = torch.cat(parts)
    ring, beam = make_ring(dt, "A", "mixed"), make_beam(dt)
    m = torch.tensor(beam.species.mass_eV_float, **kw)
    e4 = e8 = cand
    for _ in range(4):
        e4 = round_trip(e4, m)
    e8 = e4
    for _ in range(4):
        e8 = round_trip(e8, m)
    short = cand[(cand != e4) & (e4 != e8)].cpu().tolist()
    print("candidates", cand.numel(), "shortlisted", len(short))
    for energy in short[:8] + short[::max(1, len(short) // 24)]:              # (the known ones first, then a spread over the rest)
        starts = turn_start_bits(ring, make_beam(dt, energy=energy), 4)
        if len(set(starts)) >= 3:
            print("drifting energy", repr(energy), "turn-start bits", starts)
            return energy
    return None


@pytest.mark.parametrize("precision,dt", DTYPE_MODES, ids=DTYPE_IDS)
def test_a_drifting_reference_energy_is_followed_turn_by_turn(precision, dt, monkeypatch):
    import cheetah_amd as ca

    energy = drifting_energy(dt)
    assert energy is not None, "no energy found whose round trip goes on drifting on the device"
    ref = loop_reference(dt, "A", precision, 2e-4, (), energy)
    assert len({bits(e).item() for e in ref["e"][:4]}) >= 3                               # (the starts of turns 1 .. 4)
    assert not same_bits(ref["e"][1], ref["e"][2]) and not same_bits(ref["e"][2], ref["e"][3])
    ring, beam = make_ring(dt, "A", precision), make_beam(dt, energy=energy)
    whole = ring.track_turns(beam, TURNS, record_first=3, fused=True)
    check_against_loop(whole, ref, TURNS, beam)
    check_against_loop(ring.track_turns(beam, TURNS, fused=False), ref, TURNS, beam)
    for r in range(TURNS):                                                              # every turn of it, through the probe rows
        assert same_bits(whole.particles[r], ref["x"][r + 1, :3]), r + 1
    # ring A has four items: two turns per launch, so the boundary between turns 2 and 3 falls where the energy still moves
    monkeypatch.setattr(ca.particles.turns, "_MAX_ITEM_STEPS", 8)
    chunked = ring.track_turns(beam, TURNS, record_first=3, fused=True)
    check_against_loop(chunked, ref, TURNS, beam)
    for a, b in zip(outputs(whole), outputs(chunked)):
        assert same_bits(a, b)


# ---- 3. records ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,dt", DTYPE_MODES, ids=DTYPE_IDS)
@pytest.mark.parametrize("record_every", [1, 5])
def test_records_match_the_float64_restatement(precision, dt, record_every):
    ref = loop_reference(dt, "B", precision, 2e-4, ())
    ring, beam = make_ring(dt, "B", precision), make_beam(dt)
    lost = np.zeros(N, np.int32)
    first = ring.track_turns(beam, TURNS, record_every=record_every, record_first=3, fused=True)
    check_records(first, ref, lost, record_every, 3)
    check_records(ring.track_turns(beam, TURNS, record_every=record_every, fused=True), ref, lost, record_every, 0)
    again = ring.track_turns(beam, TURNS, record_every=record_every, record_first=3, fused=True)
    assert same_bits(first.sums, again.sums)                                            # two calls: identical bits
    mean, std = first.mean.cpu().numpy(), first.std.cpu().numpy()
    got = first.sums.cpu().numpy()
    np.testing.assert_allclose(std, np.sqrt(np.maximum(0.0, got[:, 8:] / got[:, 1:2] - mean * mean)), rtol=1e-12, atol=0.0)


# ---- 4. losses -----------------------------------------------------------------------------------------------------------------------------
BIG = 2e-3               # ten times the size of the other tests' beam
BAD_ROWS = (1, 600)      # a row of the first tile and one of the last, partial tile


def loss_aperture(ref, dt):
    """(a_x, a_y) in the beam's dtype from the loop's own excursions: a_x = the 70 % quantile over the finite particles of their
    largest |x| of all turns, a_y the same of |y| — between a quarter and two thirds of the beam is lost, on several turns."""
    finite = np.isfinite(ref["x"]).all(axis=(0, 2))
    reach = np.abs(ref["x"][:, finite]).max(axis=0)
    return torch.tensor([np.quantile(reach[:, 0], 0.7), np.quantile(reach[:, 2], 0.7)], **_kw(dt))


@pytest.mark.parametrize("precision,dt", DTYPE_MODES, ids=DTYPE_IDS)
@pytest.mark.parametrize("ring_kind", ["A", "B"])
def test_losses(precision, dt, ring_kind):
    ref = loop_reference(dt, ring_kind, precision, BIG, BAD_ROWS)
    aperture = loss_aperture(ref, dt)
    lost = reference_losses(ref["x"], aperture.cpu().numpy())
    share = (lost > 0).mean()
    print("aperture", aperture.tolist(), "lost share", share, "turns of loss", np.unique(lost))
    assert (lost > 0).any() and (lost == 0).any() and 0.2 <= share <= 0.7, share         # some, not all (on the loop alone)
    assert len(np.unique(lost)) > 3                                                      # particles leave on several different turns
    assert all(lost[row] == 1 for row in BAD_ROWS)
    ring, beam = make_ring(dt, ring_kind, precision), make_beam(dt, BIG, BAD_ROWS)
    final = np.where(lost > 0, lost, TURNS)
    frozen = ref["x"][final, np.arange(N)]                   # a lost particle: the loop's coordinates at the turn of its loss
    for fused in (True, False):
        tbt = ring.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=3, fused=fused)
        assert np.array_equal(tbt.lost_turn.cpu().numpy(), lost)
        assert same_bits_nan_for_nan(tbt.outgoing.particles, frozen)
        assert np.isnan(frozen[list(BAD_ROWS)]).any() and np.isfinite(frozen[lost == 0]).all()
        assert same_bits(tbt.outgoing.energy, ref["e"][TURNS])
        surv = tbt.outgoing.survival_probabilities.cpu().numpy()
        assert (surv[lost > 0] == 0).all() and same_bits(surv[lost == 0], beam.survival_probabilities.cpu().numpy()[lost == 0])
        assert np.isfinite(tbt.sums.cpu().numpy()).all()     # the non-finite rows are selected out, not multiplied by 0
        check_records(tbt, ref, lost, 5, 3)                  # (row 1 of the probe: frozen at turn 1)


@pytest.mark.parametrize("precision,dt", MODES, ids=MODE_IDS)
def test_probe_rows_of_the_second_tile_and_of_frozen_particles(precision, dt):
    """record_first = 300: probe rows of the second tile (rows 256 - 299), some of the 300 lost and frozen — the fused ring against
    the turn-by-turn path, bit for bit and NaN for NaN, in every arithmetic mode."""
    aperture = loss_aperture(loop_reference(dt, "A", precision, BIG, BAD_ROWS), dt)
    ring, beam = make_ring(dt, "A", precision), make_beam(dt, BIG, BAD_ROWS)
    general = ring.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=300, fused=False)
    fused = ring.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=300, fused=True)
    lost = general.lost_turn.cpu().numpy()
    recorded = general.turns.cpu().numpy()
    assert general.particles.shape == (len(recorded), 300, 7) and len(recorded) == TURNS // 5
    frozen = (lost[:300] > 0) & (lost[:300] <= recorded.max())               # recorded at least once after its loss
    assert frozen.any() and frozen[256:].any()
    assert np.array_equal(fused.lost_turn.cpu().numpy(), lost)
    assert same_bits_nan_for_nan(fused.particles, general.particles.cpu().numpy())


# ---- 5. chunking ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,dt", DTYPE_MODES, ids=DTYPE_IDS)
@pytest.mark.parametrize("record_every", [1, 5])
def test_chunked_launches_give_the_single_launchs_bits(precision, dt, record_every, monkeypatch):
    import cheetah_amd as ca
    from cheetah_amd import _ops

    ref = loop_reference(dt, "A", precision, BIG, BAD_ROWS)
    ring, beam = make_ring(dt, "A", precision), make_beam(dt, BIG, BAD_ROWS)
    aperture = loss_aperture(ref, dt)
    launches, orig = [], _ops.dkd_turns
    monkeypatch.setattr(_ops, "dkd_turns", lambda *a, **k: (launches.append(a[12]), orig(*a, **k))[1])      # (num_turns of the launch)

    def call():
        del launches[:]
        tbt = ring.track_turns(beam, TURNS, record_every=record_every, aperture=aperture, record_first=3, fused=True)
        return tbt, list(launches)

    whole, n_whole = call()
    monkeypatch.setattr(ca.particles.turns, "_MAX_ITEM_STEPS", 4 * 19)                                    # four items: 19 turns per launch
    halves, n_halves = call()
    monkeypatch.setattr(ca.particles.turns, "_MAX_ITEM_STEPS", 8)                                         # two turns per launch
    many, n_many = call()
    monkeypatch.setattr(ca.particles.turns, "_MAX_PARTIAL_BYTES", 1)                                      # and one record per launch
    by_record, n_by_record = call()
    assert n_whole == [37] and n_halves == [19, 18] and n_many == [2] * 18 + [1] and len(n_by_record) >= len(n_many)
    assert (whole.lost_turn > 0).any() and whole.sums.shape[0] == TURNS // record_every
    for other in (halves, many, by_record):
        for a, b in zip(outputs(whole), outputs(other)):
            assert same_bits(a, b)


# ---- 6. staying off the fused path ------------------------------------------------------------------------------------------------------------
def _off_path_rings(dt):
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    dkd = {"tracking_method": "drift_kick_drift"}
    rings = {
        "corrector": (make_ring(dt, "A", extra=ca.HorizontalCorrector(t(0.1), angle=t(1e-5), name="hcor", **kw)), "linear elements"),
        "linear-drift": (make_ring(dt, "B", extra=ca.Drift(t(0.1), name="lin", **kw)), "linear elements"),
        "tdc": (make_ring(dt, "A", extra=ca.TransverseDeflectingCavity(t(0.1), voltage=t(1e4), phase=t(0.0), frequency=t(1e9), name="tdc",
                                                                       **kw)), "TransverseDeflectingCavity 'tdc'"),
        "193-items": (ca.Segment([ca.Drift(t(0.01), **dkd, **kw) for _ in range(193)]), "193 drift-kick-drift elements"),
        "vector-k1": (make_ring(dt, "A", extra=ca.Quadrupole(t(0.1), k1=t([0.1, 0.2]), name="vec", **dkd, **kw)), "Quadrupole 'vec'"),
        "requires-grad": (make_ring(dt, "A", extra=ca.Quadrupole(t(0.1), k1=t(0.1).requires_grad_(True), name="train", **dkd, **kw)),
                          "requires grad"),
    }
    if dt == torch.float32:
        mixed = make_ring(dt, "A")
        mixed.qd.dkd_precision = "double"
        rings["precision-classes"] = (mixed, "arithmetic class")
    return rings


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=DTYPE_IDS)
@pytest.mark.parametrize("case", ["corrector", "linear-drift", "precision-classes", "tdc", "193-items", "vector-k1", "requires-grad"])
def test_rings_that_do_not_qualify_take_the_general_path(dt, case):
    rings = _off_path_rings(dt)
    if case not in rings:
        # (no float64 case of "precision-classes": a float64 beam is one arithmetic class whatever dkd_precision says — checked here)
        mixed = make_ring(dt, "A")
        mixed.qd.dkd_precision = "double"
        beam = make_beam(dt)
        assert same_bits(mixed.track_turns(beam, 3, fused=True).outgoing.particles, mixed.track_turns(beam, 3, fused=False).outgoing.particles)
        return
    ring, reason = rings[case]
    beam = make_beam(dt)
    with pytest.raises(ValueError, match=reason) as err:
        ring.track_turns(beam, 3, fused=True)
    assert "fused=True" in str(err.value) and "drift_kick_drift" in str(err.value)        # the second-order reason stands in front
    auto = ring.track_turns(beam, 3, record_every=2, record_first=2)
    general = ring.track_turns(beam, 3, record_every=2, record_first=2, fused=False)
    for a, b in zip(outputs(auto), outputs(general)):
        assert same_bits(a, b)
    assert torch.isfinite(auto.outgoing.particles).all()


# ---- 7. settings are followed ---------------------------------------------------------------------------------------------------------------
def test_settings_and_dkd_precision_are_read_at_every_call(monkeypatch):
    from cheetah_amd.accelerator.element import Element

    dt, turns = torch.float32, 5
    ring, beam = make_ring(dt, "B"), make_beam(dt)                                       # (`dkd_precision` left to the class)
    seen = []

    def check():
        tbt = ring.track_turns(beam, turns, fused=True)
        check_against_loop(tbt, run_loop(ring, beam, turns), turns, beam)
        assert all(not same_bits(tbt.outgoing.particles, earlier) for earlier in seen)    # each change changed the result
        seen.append(tbt.outgoing.particles)

    check()
    ring.qf.k1.mul_(1.05)                                                                # an in-place edit
    check()
    ring.bend.angle.add_(1e-4)
    check()
    monkeypatch.setattr(Element, "dkd_precision", "double")                              # on the class: moves no epoch
    check()
    monkeypatch.setattr(Element, "dkd_precision", "storage")
    check()
