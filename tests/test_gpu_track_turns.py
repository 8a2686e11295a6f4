"""Segment.track_turns: the fused turn kernel (chx_second_order_turns) and the general path against the loop it replaces,
`for _ in range(turns): beam = ring.track(beam)`, and against a numpy float64 restatement of the records over that loop's beams.

The ring is [Quadrupole, Drift, Sextupole, Drift, Quadrupole(-k1), Drift] with second-order magnets and linear drifts: a FODO cell
with a phase advance of 28.5 degrees in both planes (trace of the one-turn matrix 1.757), so a matched-size beam stays bounded.
N = 1000 particles: 2 tiles in float32 (512 rows each) and 4 in float64 (256 each), the last one partial in both.

Particles, loss turns and probe rows are compared bit for bit. The sums of a record are float64 sums of N terms taken in another
order than numpy's: the bound is the worst case of such a sum, N * 2^-52 * sum w |x_j| (sum w x_j^2 for the second moments)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 1000
TURNS = 37
DTYPES = [torch.float32, torch.float64]
EPS = 2.0 ** -52


def _kw(dt):
    return {"dtype": dt, "device": "cuda"}


def make_ring(dt, kind="second_order"):
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    if kind == "linear":                 # every element linear: the plan is ONE merged run
        return ca.Segment([ca.Quadrupole(t(0.2), k1=t(2.0), **kw), ca.Drift(t(0.5), **kw), ca.Drift(t(0.1), **kw),
                           ca.Drift(t(0.5), **kw), ca.Quadrupole(t(0.2), k1=t(-2.0), **kw), ca.Drift(t(1.1), **kw)])
    first = "drift_kick_drift" if kind == "dkd" else "second_order"
    so = {"tracking_method": "second_order"}
    return ca.Segment([ca.Quadrupole(t(0.2), k1=t(2.0), tracking_method=first, **kw), ca.Drift(t(0.5), **kw),
                       ca.Sextupole(t(0.1), k2=t(40.0), **so, **kw), ca.Drift(t(0.5), **kw),
                       ca.Quadrupole(t(0.2), k1=t(-2.0), **so, **kw), ca.Drift(t(1.1), **kw)])


def make_beam(dt, size=2e-4, bad_row=None):
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(11)
    beam = ca.ParticleBeam.from_parameters(num_particles=N, sigma_x=t(size), sigma_px=t(size / 20), sigma_y=t(size), sigma_py=t(size / 20),
                                           sigma_p=t(1e-3), energy=t(1e8), **kw)
    x = beam.particles.clone()
    if bad_row is not None:
        x[bad_row, 0] = float("inf")
    gen = torch.Generator().manual_seed(5)
    charges = (torch.rand(N, generator=gen, dtype=torch.float64) + 0.5).to(**kw) * 1e-15
    survival = (torch.rand(N, generator=gen, dtype=torch.float64) * 0.5 + 0.5).to(**kw)
    return ca.ParticleBeam(x, beam.energy, particle_charges=charges, survival_probabilities=survival, s=t(0.25), species=beam.species)


@functools.lru_cache(maxsize=None)
def loop_reference(dt, kind, size, bad_row):
    """The loop `track_turns` replaces, once per case: the beams after 0 .. TURNS turns as one (TURNS + 1, N, 7) array, the path
    length after one turn, the weights. Shared by the tests and never modified."""
    ring, beam = make_ring(dt, kind), make_beam(dt, size, bad_row)
    xs, s_one = [beam.particles.cpu().numpy()], None
    w = beam.particle_charges.cpu().numpy().astype(np.float64) * beam.survival_probabilities.cpu().numpy().astype(np.float64)
    s0 = beam.s.cpu().numpy()
    for turn in range(TURNS):
        beam = ring.track(beam)
        xs.append(beam.particles.cpu().numpy())
        if turn == 0:
            s_one = beam.s.cpu().numpy()
    xs = np.stack(xs)
    xs.setflags(write=False)
    return {"x": xs, "w": w, "s0": s0, "s_one": s_one}


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def reference_losses(xs, aperture):
    """lost_turn of the loop: the first turn at whose end the particle is non-finite or outside the aperture (0: never)."""
    bad = ~np.isfinite(xs[1:, :, :6]).all(axis=2)
    if aperture is not None:
        bad |= (np.abs(xs[1:, :, 0]) > aperture[0]) | (np.abs(xs[1:, :, 2]) > aperture[1])
    first = np.argmax(bad, axis=0) + 1
    return np.where(bad.any(axis=0), first, 0).astype(np.int32)


def reference_sums(xs, w, lost, turn):
    """The 14 sums of the record of `turn` in numpy float64, and the bound of each (see the module docstring)."""
    alive = (lost == 0) | (lost > turn)
    x = xs[turn][alive, :6].astype(np.float64)
    wa = w[alive]
    sums = np.concatenate([[alive.sum(), wa.sum()], (wa[:, None] * x).sum(axis=0), (wa[:, None] * x * x).sum(axis=0)])
    bound = N * EPS * np.concatenate([[0.0, wa.sum()], (wa[:, None] * np.abs(x)).sum(axis=0), (wa[:, None] * x * x).sum(axis=0)])
    return sums, bound


def check_records(tbt, ref, lost, record_every, record_first):
    R = TURNS // record_every
    turns = np.arange(1, R + 1) * record_every
    assert tbt.turns.dtype == torch.int64 and np.array_equal(tbt.turns.cpu().numpy(), turns)
    got = tbt.sums.cpu().numpy()
    assert got.shape == (R, 14) and got.dtype == np.float64
    mean, charge, std = tbt.mean.cpu().numpy(), tbt.charge.cpu().numpy(), tbt.std.cpu().numpy()
    for r, turn in enumerate(turns):
        want, bound = reference_sums(ref["x"], ref["w"], lost, turn)
        assert tbt.num_alive[r].item() == want[0], (turn, tbt.num_alive[r].item(), want[0])
        assert abs(charge[r] - want[1]) <= bound[1], (turn, charge[r], want[1])
        assert (np.abs(mean[r] * charge[r] - want[2:8]) <= bound[2:8]).all(), (turn, mean[r] * charge[r], want[2:8])
        assert (np.abs(got[r, 8:] - want[8:]) <= bound[8:]).all(), (turn, got[r, 8:], want[8:])
    # std is the population form over the call's own sums
    np.testing.assert_allclose(std, np.sqrt(np.maximum(0.0, got[:, 8:] / got[:, 1:2] - mean * mean)), rtol=1e-12, atol=0.0)
    if record_first:
        assert tbt.particles.shape == (R, record_first, 7)
        frozen = np.where(lost[:record_first] > 0, lost[:record_first], TURNS + 1)
        for r, turn in enumerate(turns):
            rows = np.stack([ref["x"][min(turn, frozen[k]), k] for k in range(record_first)])
            assert same_bits(tbt.particles[r], rows), turn
    else:
        assert tbt.particles is None


# ---- 1. particles ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["second_order", "linear"])
@pytest.mark.parametrize("num_turns", [1, 2, 37])
def test_particles_are_the_loops_bit_for_bit(dt, kind, num_turns):
    ref = loop_reference(dt, kind, 2e-4, None)
    ring, beam = make_ring(dt, kind), make_beam(dt)
    fused = ring.track_turns(beam, num_turns, fused=True)
    assert same_bits(fused.outgoing.particles, ref["x"][num_turns])
    assert same_bits(ring.track_turns(beam, num_turns).outgoing.particles, ref["x"][num_turns])         # fused=None: the same path
    general = ring.track_turns(beam, num_turns, fused=False)
    assert same_bits(general.outgoing.particles, ref["x"][num_turns])
    for tbt in (fused, general):
        assert tbt.lost_turn.dtype == torch.int32 and not tbt.lost_turn.any()
        assert same_bits(tbt.outgoing.survival_probabilities, beam.survival_probabilities)
        assert same_bits(tbt.outgoing.particle_charges, beam.particle_charges) and same_bits(tbt.outgoing.energy, beam.energy)
        # the documented path length: one multiplication, in the beam's dtype
        s0, s_one = ref["s0"], ref["s_one"]
        assert same_bits(tbt.outgoing.s, s0 + s0.dtype.type(num_turns) * (s_one - s0))
    assert same_bits(beam.particles, ref["x"][0])                                                      # the incoming beam is left alone


# ---- 2. records --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("record_every", [1, 5])
def test_records_match_the_float64_restatement(dt, record_every):
    ref = loop_reference(dt, "second_order", 2e-4, None)
    ring, beam = make_ring(dt), make_beam(dt)
    lost = np.zeros(N, np.int32)
    for fused in (True, False):
        check_records(ring.track_turns(beam, TURNS, record_every=record_every, fused=fused), ref, lost, record_every, 0)
        check_records(ring.track_turns(beam, TURNS, record_every=record_every, record_first=3, fused=fused), ref, lost, record_every, 3)


# ---- 3. losses ---------------------------------------------------------------------------------------------------------------------------
BIG = 2e-3               # the enlarged beam: ten times the matched size
APERTURE = (4e-3, 4e-3)  # two of its standard deviations


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("bad_row", [None, 1])
def test_losses(dt, bad_row):
    ref = loop_reference(dt, "second_order", BIG, bad_row)
    lost = reference_losses(ref["x"], APERTURE)
    share = (lost > 0).mean()
    assert 0.05 <= share <= 0.95, share                      # (on the loop reference alone)
    assert len(np.unique(lost)) > 3                          # particles leave on several different turns
    if bad_row is not None:
        assert lost[bad_row] == 1
    ring, beam = make_ring(dt), make_beam(dt, BIG, bad_row)
    aperture = torch.tensor(APERTURE, **_kw(dt))
    final = np.where(lost > 0, lost, TURNS)
    frozen = ref["x"][final, np.arange(N)]                   # a lost particle: the loop's coordinates at the turn of its loss
    for fused in (True, False):
        tbt = ring.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=3, fused=fused)
        assert np.array_equal(tbt.lost_turn.cpu().numpy(), lost)
        assert same_bits(tbt.outgoing.particles, frozen)
        surv = tbt.outgoing.survival_probabilities.cpu().numpy()
        assert (surv[lost > 0] == 0).all() and same_bits(surv[lost == 0], beam.survival_probabilities.cpu().numpy()[lost == 0])
        assert np.isfinite(tbt.sums.cpu().numpy()).all()     # the non-finite row is selected out, not multiplied by 0
        check_records(tbt, ref, lost, 5, 3)
    # the aperture is read through its address: an in-place edit changes the next call
    aperture.mul_(0.5)
    lost_half = reference_losses(ref["x"], (APERTURE[0] / 2, APERTURE[1] / 2))
    assert (lost_half != lost).any()
    assert np.array_equal(ring.track_turns(beam, TURNS, aperture=aperture, fused=True).lost_turn.cpu().numpy(), lost_half)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_probe_rows_beyond_the_first_256_and_of_frozen_particles(dt):
    """record_first = 600: the probe rows of a float32 lane's second particle (rows 256 - 511 of the first tile), of the second
    tile, and of the float64 kernel's second and third tile, some of them lost and frozen — the fused ring against the turn-by-turn
    path, bit for bit."""
    ring, beam = make_ring(dt), make_beam(dt, BIG)
    aperture = torch.tensor(APERTURE, **_kw(dt))
    general = ring.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=600, fused=False)
    fused = ring.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=600, fused=True)
    lost = general.lost_turn.cpu().numpy()
    recorded = general.turns.cpu().numpy()
    assert general.particles.shape == (len(recorded), 600, 7) and len(recorded) == TURNS // 5
    frozen = (lost[:600] > 0) & (lost[:600] <= recorded.max())               # recorded at least once after its loss
    assert frozen.any() and frozen[256:].any()
    assert np.array_equal(fused.lost_turn.cpu().numpy(), lost)
    assert same_bits(fused.particles, general.particles)


# ---- 4. chunking, 5. determinism ----------------------------------------------------------------------------------------------------------
def outputs(tbt):
    return [tbt.outgoing.particles, tbt.outgoing.survival_probabilities, tbt.outgoing.s, tbt.lost_turn, tbt.turns, tbt.sums, tbt.particles]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("record_every", [1, 5])
def test_chunked_launches_give_the_single_launchs_bits(dt, record_every, monkeypatch):
    import cheetah_amd as ca

    ring, beam = make_ring(dt), make_beam(dt, BIG, 1)
    aperture = torch.tensor(APERTURE, **_kw(dt))
    call = lambda: ring.track_turns(beam, TURNS, record_every=record_every, aperture=aperture, record_first=3, fused=True)  # noqa: E731
    whole = call()
    again = call()                                           # determinism: two calls, identical bits
    monkeypatch.setattr(ca.particles.turns, "_MAX_ITEM_STEPS", 12)                                      # 6 items: 2 turns per launch
    chunked = call()
    monkeypatch.setattr(ca.particles.turns, "_MAX_PARTIAL_BYTES", 1)                                    # and one record per launch
    by_record = call()
    assert (whole.lost_turn > 0).any() and whole.sums.shape[0] == TURNS // record_every
    for other in (again, chunked, by_record):
        for a, b in zip(outputs(whole), outputs(other)):
            assert same_bits(a, b)


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors():
    import cheetah_amd as ca

    dt = torch.float32
    kw = _kw(dt)
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    ring, beam = make_ring(dt), make_beam(dt)
    grad_beam = ca.ParticleBeam(beam.particles.clone().requires_grad_(True), beam.energy, particle_charges=beam.particle_charges,
                                survival_probabilities=beam.survival_probabilities, s=beam.s, species=beam.species)
    with pytest.raises(ValueError, match="requires grad"):
        ring.track_turns(grad_beam, 2)
    with_cavity = ca.Segment(list(ring.elements) + [ca.Cavity(t(1.0), voltage=t(1e6), phase=t(0.0), frequency=t(1.3e9), **kw)])
    with pytest.raises(ValueError, match="fused=True"):
        with_cavity.track_turns(beam, 2, fused=True)
    with pytest.raises(ValueError, match="record_first"):
        ring.track_turns(beam, 2, record_first=N + 1)
    with pytest.raises(ValueError, match="num_turns"):
        ring.track_turns(beam, 0)
    with pytest.raises(ValueError, match="record_every"):
        ring.track_turns(beam, 2, record_every=0)


# ---- 7. the general path ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_a_ring_that_is_not_fusable_takes_the_general_path(dt):
    ref = loop_reference(dt, "dkd", BIG, None)
    lost = reference_losses(ref["x"], APERTURE)
    assert (lost > 0).any()
    ring, beam = make_ring(dt, "dkd"), make_beam(dt, BIG)
    aperture = torch.tensor(APERTURE, **_kw(dt))
    with pytest.raises(ValueError, match="drift_kick_drift"):
        ring.track_turns(beam, TURNS, fused=True)
    tbt = ring.track_turns(beam, TURNS, record_every=5, aperture=aperture, record_first=3)
    assert np.array_equal(tbt.lost_turn.cpu().numpy(), lost)
    final = np.where(lost > 0, lost, TURNS)
    assert same_bits(tbt.outgoing.particles, ref["x"][final, np.arange(N)])
    check_records(tbt, ref, lost, 5, 3)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_a_vectorised_lattice_takes_the_general_path_beam_by_beam(dt):
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    ring = ca.Segment([ca.Quadrupole(t(0.2), k1=t([2.0, 1.9, 2.1]), **kw), ca.Drift(t(1.1), **kw),
                       ca.Quadrupole(t(0.2), k1=t(-2.0), **kw), ca.Drift(t(1.1), **kw)])
    beam = make_beam(dt, BIG)
    with pytest.raises(ValueError, match="fused=True"):
        ring.track_turns(beam, TURNS, fused=True)
    b, xs = beam, [beam.particles.expand(3, N, 7).cpu().numpy()]
    for _ in range(TURNS):
        b = ring.track(b)
        xs.append(b.particles.cpu().numpy())
    xs = np.stack(xs)                                                                                   # (TURNS + 1, 3, N, 7)
    w = beam.particle_charges.cpu().numpy().astype(np.float64) * beam.survival_probabilities.cpu().numpy().astype(np.float64)
    tbt = ring.track_turns(beam, TURNS, record_every=5, aperture=torch.tensor(APERTURE, **kw), record_first=3)
    assert tbt.lost_turn.shape == (3, N) and tbt.sums.shape == (TURNS // 5, 3, 14) and tbt.particles.shape == (TURNS // 5, 3, 3, 7)
    assert tbt.mean.shape == (TURNS // 5, 3, 6) and tbt.num_alive.shape == (TURNS // 5, 3)
    for row in range(3):
        lost = reference_losses(xs[:, row], APERTURE)
        assert (lost > 0).any() and np.array_equal(tbt.lost_turn[row].cpu().numpy(), lost)
        final = np.where(lost > 0, lost, TURNS)
        assert same_bits(tbt.outgoing.particles[row], xs[final, row, np.arange(N)])
        one = ca.TurnByTurn(None, tbt.lost_turn[row], tbt.turns, tbt.sums[:, row].contiguous(), tbt.particles[:, row])
        check_records(one, {"x": xs[:, row], "w": w}, lost, 5, 3)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_weights_the_kernel_cannot_read_keep_a_beam_off_the_fused_path(dt):
    """The kernel reads charges and survival as N values of the particles' dtype. A beam with vectorised charges, (3, N) over
    particles (N, 7), is a vectorised beam and takes the general path with its shapes; weights of another dtype are turned away
    as well."""
    import cheetah_amd as ca

    ref = loop_reference(dt, "second_order", BIG, None)
    lost = reference_losses(ref["x"], APERTURE)
    ring, beam = make_ring(dt), make_beam(dt, BIG)
    aperture = torch.tensor(APERTURE, **_kw(dt))
    factors = torch.tensor([1.0, 2.0, 0.5], **_kw(dt))
    vec = ca.ParticleBeam(beam.particles, beam.energy, particle_charges=beam.particle_charges * factors[:, None],
                          survival_probabilities=beam.survival_probabilities, s=beam.s, species=beam.species)
    assert vec.particle_charges.shape == (3, N)
    with pytest.raises(ValueError, match="particle_charges"):
        ring.track_turns(vec, TURNS, fused=True)
    tbt = ring.track_turns(vec, TURNS, record_every=5, aperture=aperture)
    R = TURNS // 5
    assert tbt.sums.shape == (R, 3, 14) and tbt.mean.shape == (R, 3, 6) and tbt.charge.shape == (R, 3)
    assert np.array_equal(tbt.lost_turn.cpu().numpy(), lost)
    for row in range(3):
        w = vec.particle_charges[row].cpu().numpy().astype(np.float64) * beam.survival_probabilities.cpu().numpy().astype(np.float64)
        one = ca.TurnByTurn(None, tbt.lost_turn, tbt.turns, tbt.sums[:, row].contiguous())
        check_records(one, {"x": ref["x"], "w": w}, lost, 5, 0)
    other = torch.float32 if dt == torch.float64 else torch.float64
    for name in ("particle_charges", "survival_probabilities"):
        weights = {"particle_charges": beam.particle_charges, "survival_probabilities": beam.survival_probabilities}
        weights[name] = weights[name].to(other)
        mixed = ca.ParticleBeam(beam.particles, beam.energy, s=beam.s, species=beam.species, **weights)
        assert getattr(mixed, name).dtype == other
        with pytest.raises(ValueError, match=name):
            ring.track_turns(mixed, 2, fused=True)
