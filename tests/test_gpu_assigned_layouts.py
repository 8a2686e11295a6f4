"""Settings assigned in every tensor layout a control loop may hand over — a fresh tensor, a row or a column of a matrix of actions, a
strided slice, a stride-0 expansion, an element of a vector, a view whose base is edited in place afterwards — tracked on every path
that reads settings through device addresses (the run plans, the stretch table, the drift-kick-drift parameters, a captured graph).

An assignment of a tensor with the same dtype, device and shape as the old one is "soft" (Element.__setattr__): the plans take the new
address on the spot (_FastRun.absorb) instead of re-reading the element. A plan addresses entry i of a (2,) setting as
data_ptr() + i * element_size(), so only contiguous tensors may take that route; the others must take the full re-derivation, which
declines them and leaves the element to its own track.

Every step is checked twice: against the float64 oracle (oracle/chx_oracle.py), built from the element's settings read back as Python
floats — no plan, table or address is involved — and, bit for bit, against a freshly built lattice whose setting is a contiguous copy
of the assigned one. Every step is repeated with the plans' self-check (segment._CHECK_PLANS) on."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# per-column scaled error against the float64 oracle (as benchmarks/fuzz_paths.py:check scales it); float64 measured on the MI355X:
# 2.5e-15 (particles, screen read beam), 2.6e-16 (BPM reading), 5.3e-15 (ParameterBeam / track_moments mu and cov)
TOL64 = 2e-11
# float32 (beam and settings in float32 on the device, the oracle in float64): 4x the largest error measured on the MI355X over this
# file's cases — particles and the screen's read beam 6.06e-7 (the drift-kick-drift quadrupole included), the BPM reading 8.86e-8
TOL32 = {"particles": 4 * 6.1e-7, "reading": 4 * 8.9e-8}

VECTOR_SETTINGS = [("Q1", "misalignment"), ("SOL", "misalignment"), ("BPM1", "misalignment"), ("SCR", "misalignment"),
                   ("SCR", "pixel_size")]
SCALAR_SETTINGS = [("Q1", "k1"), ("Q1", "tilt"), ("SOL", "k"), ("HC", "angle"), ("VC", "angle"), ("CC", "horizontal_angle"),
                   ("CC", "vertical_angle"), ("D1", "angle"), ("DR", "length")]
VECTOR_LAYOUTS = ["fresh", "row", "column", "step2", "expand", "edited_column"]
SCALAR_LAYOUTS = ["fresh", "element", "edited_element"]
CONTIGUOUS = {"fresh", "row", "element", "edited_element"}

NEW_VALUES = {
    ("Q1", "misalignment"): [3e-4, -5e-5], ("SOL", "misalignment"): [-1e-4, 2e-4], ("BPM1", "misalignment"): [2e-5, -4e-5],
    ("SCR", "misalignment"): [5e-5, -3e-5], ("SCR", "pixel_size"): [5e-5, 7e-5],
    ("Q1", "k1"): 7.3, ("Q1", "tilt"): 0.25, ("SOL", "k"): -0.8, ("HC", "angle"): -2e-4, ("VC", "angle"): 1.5e-4,
    ("CC", "horizontal_angle"): 6e-5, ("CC", "vertical_angle"): -9e-5, ("D1", "angle"): 0.08, ("DR", "length"): 0.7,
}

CASES = [(e, n, lay) for e, n in VECTOR_SETTINGS for lay in VECTOR_LAYOUTS] + \
        [(e, n, lay) for e, n in SCALAR_SETTINGS for lay in SCALAR_LAYOUTS]


def _ids(case):
    return f"{case[0]}.{case[1]}-{case[2]}"


def _lattice(ca, dt, cavity=True, aperture=True, dkd=False):
    """Runs of linear magnets (persistent run plans) between an active BPM, an Aperture, a Cavity and an active Screen (the items of a
    stretch table)."""
    kw = {"dtype": dt, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    els = [
        ca.Drift(t(0.2), name="D0", **kw),
        ca.Quadrupole(t(0.15), k1=t(5.0), tilt=t(0.1), misalignment=t([1e-4, -2e-4]), name="Q1",
                      tracking_method="drift_kick_drift" if dkd else "linear", **kw),
        ca.Drift(t(0.3), **kw),
        ca.Solenoid(t(0.2), k=t(1.2), misalignment=t([4e-5, 6e-5]), name="SOL", **kw),
        ca.HorizontalCorrector(t(0.02), angle=t(1e-4), name="HC", **kw),
        ca.VerticalCorrector(t(0.02), angle=t(-1e-4), name="VC", **kw),
        ca.CombinedCorrector(t(0.02), horizontal_angle=t(3e-5), vertical_angle=t(4e-5), name="CC", **kw),
        ca.Dipole(t(0.4), angle=t(0.05), name="D1", **kw),
        ca.Drift(t(0.5), name="DR", **kw),
        ca.BPM(is_active=True, misalignment=t([1e-5, 2e-5]), name="BPM1", **kw),
        ca.Quadrupole(t(0.1), k1=t(-6.0), name="Q2", **kw),
        ca.Drift(t(0.25), **kw),
    ]
    if aperture:
        els.append(ca.Aperture(x_max=t(2e-2), y_max=t(2e-2), is_active=True, name="AP", **kw))
    if cavity:
        els.append(ca.Cavity(t(0.5), voltage=t(8e6), phase=t(20.0), frequency=t(1.3e9), name="CAV", **kw))
    els += [ca.Drift(t(0.3), **kw), ca.Quadrupole(t(0.1), k1=t(2.0), name="Q3", **kw), ca.Drift(t(0.2), **kw),
            ca.Screen(resolution=(40, 32), pixel_size=t([6e-5, 6e-5]), misalignment=t([0.0, 0.0]), is_active=True, name="SCR", **kw)]
    return ca.Segment(els)


def _layout(layout, value, dt):
    """(tensor holding `value` in the given layout, the base tensor a later in-place edit goes to). The entries of a base that are not
    the setting hold other, plausible values: a plan that addresses the wrong entry tracks visibly wrong physics."""
    kw = {"dtype": dt, "device": "cuda"}
    v = torch.tensor(value, **kw)
    junk = -2.5 * v.reshape(-1)[0] + 1e-5
    if layout == "fresh":
        return v, v
    if layout == "row":                          # contiguous, nonzero storage offset
        m = junk.expand(5, 2).clone()
        m[3] = v
        return m[3], m
    if layout in ("column", "edited_column"):    # stride 5
        m = junk.expand(2, 5).clone()
        m[:, 3] = v
        return m[:, 3], m
    if layout == "step2":                        # stride 2
        m = junk.expand(4).clone()
        m[::2] = v
        return m[::2], m
    if layout == "expand":                       # stride 0: both entries are entry 2 of the base
        m = junk.expand(4).clone()
        m[2] = v[0]
        return m[2].expand(2), m
    if layout in ("element", "edited_element"):  # 0-d, nonzero storage offset
        m = junk.expand(6).clone()
        m[4] = v
        return m[4], m
    raise ValueError(layout)


# ---- the float64 oracle -----------------------------------------------------------------------------------------------------------

def _kind_name(ca, e):
    for cls, name in ((ca.Drift, "drift"), (ca.Quadrupole, "quadrupole"), (ca.Dipole, "dipole"), (ca.VerticalCorrector, "vcor"),
                      (ca.HorizontalCorrector, "hcor"), (ca.CombinedCorrector, "ccor"), (ca.Solenoid, "solenoid")):
        if isinstance(e, cls):
            return name
    return None


def _floats(e):
    return [float(v) for v in e._builder_params()]


def _oracle_particles(ca, seg, x0, energy):
    """x0 (N, 7) float64 through the lattice element by element in float64: (outgoing particles, energy, {monitor name: particles
    there})."""
    from oracle import chx_oracle as oracle

    x, E, at = np.ascontiguousarray(x0, dtype=np.float64), float(energy), {}
    for e in seg.elements:
        kind = _kind_name(ca, e)
        if kind is not None and getattr(e, "tracking_method", "linear") == "drift_kick_drift":
            num_steps, fringe = e._dkd_options()
            out, _ = oracle.dkd_track("quadrupole", x[None], _floats(e), E, num_steps=num_steps, fringe_at=fringe)
            x = out[0]
        elif kind is not None:
            x = oracle.apply(x[None], oracle.build_rmatrix(kind, _floats(e), E))[0]
        elif isinstance(e, ca.Cavity):
            p = _floats(e)
            name = "cavity_sw" if e.cavity_type == "standing_wave" else "cavity_tw"
            coeffs, e_out = oracle.cavity_coeffs(p, E)
            x = oracle.cavity_track(x[None], oracle.build_rmatrix(name, p, E), coeffs)[0]
            E = float(e_out[0])
        elif isinstance(e, ca.Aperture):
            assert np.abs(x[:, 0]).max() < float(e.x_max) and np.abs(x[:, 2]).max() < float(e.y_max)   # (nothing is lost)
        elif isinstance(e, (ca.BPM, ca.Screen)):
            at[e.name] = x.copy()
        else:
            assert isinstance(e, ca.Marker) or type(e).__name__ == "Marker", type(e)
    return x, E, at


def _oracle_map(ca, seg, energy):
    from oracle import chx_oracle as oracle

    R = np.eye(7)
    for e in seg.elements:
        kind = _kind_name(ca, e)
        if kind is not None:
            R = oracle.build_rmatrix(kind, _floats(e), float(energy))[0] @ R
    return R


def _column_error(got, want):
    """max over columns of max |got - want| / max |want| of that column."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 7)
    want = np.asarray(want, dtype=np.float64).reshape(-1, 7)
    cols = np.abs(want).max(axis=0) + 1e-300
    return float((np.abs(got - want).max(axis=0) / cols).max())


def _within(err, dt, what, kind="particles"):
    """Every comparison with the oracle goes through here (one place to read the measured errors from)."""
    tol = TOL64 if dt == torch.float64 else TOL32[kind]
    assert err <= tol, f"{what}: {err:.3e} from the float64 oracle (allowed {tol:.1e})"


# ---- the paths ----------------------------------------------------------------------------------------------------------------------

def _particle_beam(ca, dt, n=4000):
    kw = {"dtype": dt, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(3)
    return ca.ParticleBeam.from_parameters(num_particles=n, sigma_x=t(2e-4), sigma_y=t(1.5e-4), sigma_px=t(2e-5), sigma_py=t(3e-5),
                                           mu_x=t(5e-5), sigma_tau=t(1e-5), sigma_p=t(1e-3), energy=t(1.2e8), **kw)


def _fresh_like(ca, seg_factory, elem, name, value):
    fresh = seg_factory()
    setattr(getattr(fresh, elem), name, value.detach().clone().contiguous())
    return fresh


def _check_particles(ca, seg, fresh, beam, dt, what):
    """`seg.track(beam)` against the oracle and against `fresh`: particles, energy, the BPM's reading, the screen's read beam and
    image. Returns the outgoing particles."""
    with torch.no_grad():
        out = seg.track(beam)
        want = fresh.track(beam)
    x, E, at = _oracle_particles(ca, seg, beam.particles.double().cpu().numpy(), float(beam.energy))
    _within(_column_error(out.particles.cpu(), x), dt, f"{what}: particles (per-column scaled)")
    assert float(out.energy) == pytest.approx(E, rel=1e-12 if dt == torch.float64 else 2e-7)
    bpm = seg.BPM1
    mis = np.array([float(v) for v in bpm.misalignment])
    xy = at["BPM1"][:, [0, 2]].mean(axis=0) - mis
    scale = np.abs(at["BPM1"][:, [0, 2]]).max(axis=0)
    _within(float((np.abs(bpm.reading.double().cpu().numpy() - xy) / scale).max()), dt, f"{what}: BPM reading", "reading")
    scr = seg.SCR
    read = at["SCR"].copy()
    read[:, 0] -= float(scr.misalignment[0])
    read[:, 2] -= float(scr.misalignment[1])
    _within(_column_error(scr.get_read_beam().particles.cpu(), read), dt, f"{what}: screen read beam")
    # bit for bit against the fresh lattice
    assert torch.equal(out.particles, want.particles), what
    assert torch.equal(out.energy, want.energy) and torch.equal(out.s, want.s), what
    assert torch.equal(bpm.reading, fresh.BPM1.reading), what
    assert torch.equal(scr.get_read_beam().particles, fresh.SCR.get_read_beam().particles), what
    img, want_img = scr.reading, fresh.SCR.reading
    # (cloud-in-cell deposits with float atomics: the order of the additions may differ between two runs)
    assert torch.equal(img, want_img) or torch.allclose(img, want_img, rtol=1e-5, atol=0), what
    assert float(img.sum()) > 0, what
    return out.particles


def _check_parameters(ca, seg, fresh, beam, dt, what):
    with torch.no_grad():
        out = seg.track(beam)
        want = fresh.track(beam)
    R = _oracle_map(ca, seg, float(beam.energy))
    mu0, cov0 = beam.mu.double().cpu().numpy(), beam.cov.double().cpu().numpy()
    mu, cov = R @ mu0, R @ cov0 @ R.T
    sig = np.sqrt(np.diag(cov))[:6]
    _within(float((np.abs(out.mu.double().cpu().numpy() - mu)[:6] / (sig + np.abs(mu[:6]))).max()), dt, f"{what}: mu")
    _within(float((np.abs(out.cov.double().cpu().numpy() - cov)[:6, :6] / np.outer(sig, sig)).max()), dt, f"{what}: cov")
    assert torch.equal(out.mu, want.mu) and torch.equal(out.cov, want.cov), what
    assert torch.equal(seg.BPM1.reading, fresh.BPM1.reading), what
    assert torch.equal(seg.SCR.reading, fresh.SCR.reading), what


def _check_moments(ca, seg, fresh, beam, dt, what):
    from oracle import chx_oracle as oracle

    with torch.no_grad():
        got = seg.track_moments(beam, exact=True)
        want = fresh.track_moments(beam, exact=True)
    x, _, _ = _oracle_particles(ca, seg, beam.particles.double().cpu().numpy(), float(beam.energy))
    m = oracle.moments(x)
    mu, cov = m["mu"][0], m["cov"][0]
    sig = np.sqrt(np.diag(cov))
    _within(float((np.abs(got.mu.double().cpu().numpy()[:6] - mu) / (sig + np.abs(mu))).max()), dt, f"{what}: mu")
    _within(float((np.abs(got.cov.double().cpu().numpy()[:6, :6] - cov) / np.outer(sig, sig)).max()), dt, f"{what}: cov")
    assert torch.equal(got.mu, want.mu) and torch.equal(got.cov, want.cov), what


def _assign_and_check(ca, seg_factory, beam, dt, elem, name, layout, check):
    from cheetah_amd.accelerator import segment

    seg = seg_factory()
    with torch.no_grad():
        seg.track(beam)                                  # the plans are derived here; the next assignment is absorbed or re-read
    value, base = _layout(layout, NEW_VALUES[(elem, name)], dt)
    reads = {"n": 0}
    real_read = segment._FastRun._read

    def counting_read(self, e, i):
        reads["n"] += 1
        return real_read(self, e, i)

    hard = ca.Element._hard_epoch
    segment._FastRun._read = counting_read
    try:
        setattr(getattr(seg, elem), name, value)
        with torch.no_grad():
            seg.track(beam)
    finally:
        segment._FastRun._read = real_read
    took_soft_path = ca.Element._hard_epoch == hard
    steps = [value]
    if layout.startswith("edited"):
        steps.append("edit")
    for step in steps:
        if step == "edit":
            base.mul_(1.25)                              # every path must follow the edit through the view
        what = f"{elem}.{name} = <{layout}> ({'after the in-place edit' if step == 'edit' else 'assigned'})"
        old = segment._CHECK_PLANS
        problems = []        # (both runs are reported: what the plain track computes and what the plans' self-check says)
        try:
            for checked in (False, True):
                segment._CHECK_PLANS = checked
                fresh = _fresh_like(ca, seg_factory, elem, name, getattr(getattr(seg, elem), name))
                try:
                    check(ca, seg, fresh, beam, dt, what + (" with CHX_CHECK_PLANS" if checked else ""))
                except (AssertionError, RuntimeError) as exc:
                    problems.append(f"{type(exc).__name__}: {str(exc).splitlines()[0]}")
        finally:
            segment._CHECK_PLANS = old
        assert not problems, problems
    if layout in CONTIGUOUS:
        assert reads["n"] == 0, "a contiguous soft assignment was re-read instead of patched"
        assert took_soft_path
    else:
        assert not took_soft_path, "a strided or expanded setting took the soft path"


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_particle_beam_track(case, dt):
    import cheetah_amd as ca

    elem, name, layout = case
    _assign_and_check(ca, lambda: _lattice(ca, dt), _particle_beam(ca, dt), dt, elem, name, layout, _check_particles)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_parameter_beam_track(case):
    import cheetah_amd as ca

    dt = torch.float64
    kw = {"dtype": dt, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    beam = ca.ParameterBeam.from_parameters(sigma_x=t(2e-4), sigma_y=t(1.5e-4), sigma_px=t(2e-5), sigma_py=t(3e-5), mu_x=t(5e-5),
                                            cov_xpx=t(1e-9), sigma_tau=t(1e-5), sigma_p=t(1e-3), energy=t(1.2e8), **kw)
    elem, name, layout = case
    _assign_and_check(ca, lambda: _lattice(ca, dt, cavity=False, aperture=False), beam, dt, elem, name, layout,
                      _check_parameters)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "SCR"], ids=_ids)
def test_track_moments_exact(case):
    import cheetah_amd as ca

    dt = torch.float64
    elem, name, layout = case
    _assign_and_check(ca, lambda: _lattice(ca, dt), _particle_beam(ca, dt), dt, elem, name, layout, _check_moments)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "Q1"], ids=_ids)
def test_drift_kick_drift_quadrupole(case, dt):
    """A quadrupole tracked drift-kick-drift reads the same (tensor, index) pairs as the run plans (Element._dkd_params_stacked)."""
    import cheetah_amd as ca

    elem, name, layout = case
    _assign_and_check(ca, lambda: _lattice(ca, dt, dkd=True), _particle_beam(ca, dt), dt, elem, name, layout, _check_particles)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_captured_step_follows_edits_of_the_base(case):
    """A step captured (cheetah_amd.graph.capture) after the assignment, replayed after in-place edits of the assigned tensor's base."""
    import cheetah_amd as ca
    import cheetah_amd.graph as graph
    from cheetah_amd.accelerator import segment

    dt = torch.float64
    elem, name, layout = case
    beam = _particle_beam(ca, dt, n=2000)
    seg = _lattice(ca, dt)
    with torch.no_grad():
        seg.track(beam)
        value, base = _layout(layout, NEW_VALUES[(elem, name)], dt)
        setattr(getattr(seg, elem), name, value)
        step = graph.capture(lambda: (seg.track(beam).particles, seg.BPM1.reading))
        for k in range(3):
            if k:
                base.mul_(1.25 if k == 1 else 0.8)      # in place: the replay follows
            particles, reading = step()
            x, _, at = _oracle_particles(ca, seg, beam.particles.double().cpu().numpy(), float(beam.energy))
            _within(_column_error(particles.cpu(), x), dt, f"replay {k}: particles")
            fresh = _fresh_like(ca, lambda: _lattice(ca, dt), elem, name, getattr(getattr(seg, elem), name))
            want = fresh.track(beam)
            assert torch.equal(particles, want.particles), k
            scale = np.abs(at["BPM1"][:, [0, 2]]).max(axis=0)
            xy = at["BPM1"][:, [0, 2]].mean(axis=0) - np.array([float(v) for v in seg.BPM1.misalignment])
            _within(float((np.abs(reading.cpu().numpy() - xy) / scale).max()), dt, f"replay {k}: BPM reading", "reading")
            if elem == "BPM1" and layout not in CONTIGUOUS:
                # (a monitor whose misalignment the stretch cannot address reads the beam in the walk, the fresh lattice's inside the
                # stretch: under capture the two reductions may round differently)
                assert torch.allclose(reading, fresh.BPM1.reading, rtol=0, atol=1e-13 * float(scale.max())), k
            else:
                assert torch.equal(reading, fresh.BPM1.reading), k
        # an eager track after the replays, with the plans' self-check on
        old = segment._CHECK_PLANS
        segment._CHECK_PLANS = True
        try:
            assert torch.equal(seg.track(beam).particles, want.particles)
        finally:
            segment._CHECK_PLANS = old


def test_check_plans_raises_on_a_plan_that_addresses_a_strided_setting():
    """CHX_CHECK_PLANS: a run plan that holds a (2,) setting it could not address — here a column view swapped into the buffer
    dictionary behind the element's back, which moves no counter — raises, whatever address the plan holds."""
    import cheetah_amd as ca
    from cheetah_amd.accelerator import segment

    dt = torch.float64
    seg = _lattice(ca, dt)
    beam = _particle_beam(ca, dt, n=1000)
    m = torch.zeros(2, 5, dtype=dt, device="cuda")
    old = segment._CHECK_PLANS
    try:
        with torch.no_grad():
            seg.track(beam)
            view = m[:, 0]
            view.copy_(seg.Q1.misalignment)
            seg.Q1._buffers["misalignment"] = view
            segment._CHECK_PLANS = True
            with pytest.raises(RuntimeError, match="cannot address"):
                seg.track(beam)
    finally:
        segment._CHECK_PLANS = old


@pytest.mark.parametrize("with_stretch", [True, False])
def test_raw_capture_after_an_assignment_then_eager_tracks(with_stretch):
    """A raw capture (no warm-up) right after an assignment, while the plans are stale; then an assignment and an eager track, a replay,
    and an eager track without an assignment: the last one must be the fresh lattice's. (The replay itself may use the capture-time
    tensor: a new tensor needs a new capture, cheetah_amd/graph.py.)"""
    import cheetah_amd as ca

    dt = torch.float64
    kw = {"dtype": dt, "device": "cuda"}
    beam = _particle_beam(ca, dt, n=2000)

    def build():
        return _lattice(ca, dt) if with_stretch else _lattice(ca, dt, cavity=False, aperture=False)

    seg = build()
    with torch.no_grad():
        seg.track(beam)
        first = torch.tensor(3.0, **kw)
        seg.Q1.k1 = first
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g):
                seg.track(beam)
        torch.cuda.current_stream().wait_stream(side)
        second = torch.tensor(-4.0, **kw)
        seg.Q1.k1 = second
        eager = seg.track(beam).particles.clone()
        g.replay()
        after = seg.track(beam).particles
        fresh = build()
        fresh.Q1.k1 = second.clone()
        want = fresh.track(beam).particles
        assert torch.equal(eager, want)
        assert torch.equal(after, want), "an eager track after a replay used the capture-time settings"
