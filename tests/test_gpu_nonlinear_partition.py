"""How `Segment.track` partitions a lattice of non-linear elements into calls of `_ops.dkd_chain` / `_ops.second_order_chain`
(reference: cheetah/accelerator/segment.py:545-574 merges only linear elements; element.py:195-228 tracks the others one by one):
for a table of small lattices, the kinds list of every call in order and the planner rows that took an item, written out; the
particles, energy and s bit for bit those of the same pieces tracked one after the other; and a second track of every case from
the kept run, with the same calls and the same bits.

64 particles per beam: the kernels are not under test here, the host's scanner is. The class lists in the comments of DKD_CASES
are the rows of the same name in tests/test_nonlinear_items_host.py (PARTITIONS): the first call's length here is the count
there — change both tables together."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 64
DKD = {"tracking_method": "drift_kick_drift"}
SO = {"tracking_method": "second_order"}
Q, D, B, S, TDC, LIN = 1, 0, 2, 5, 3, 4              # _ops.DKD_KIND / DKD_LINEAR


def _kw(dt):
    return {"dtype": dt, "device": "cuda"}


def _tools(dt):
    import cheetah_amd as ca

    kw = _kw(dt)
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    return ca, kw, t


def _beam(dt):
    ca, kw, t = _tools(dt)
    torch.manual_seed(5)
    return ca.ParticleBeam.from_parameters(num_particles=N, sigma_x=t(2e-4), sigma_px=t(3e-5), sigma_y=t(1e-4), sigma_py=t(2e-5),
                                           sigma_tau=t(1e-4), sigma_p=t(1e-3), energy=t(6.3e6), **kw)


# Each case: dt -> (pieces, {dtype: kinds lists of the calls}, {planner row: items taken}). A piece of linear elements is one merged
# run (tracked as a Segment of its own in the walk piece by piece), every other piece one element.
def dkd_magnets_only(dt):                                                   # classes [2, 2, 2, 2]
    ca, kw, t = _tools(dt)
    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Drift(t(0.5), **DKD, **kw)],
            [ca.Dipole(t(0.4), angle=t(0.03), **DKD, **kw)], [ca.Sextupole(t(0.1), k2=t(9.0), **DKD, **kw)]], \
        [[Q, D, B, S]], {"drift_kick_drift_run": 1}


def dkd_runs_between(dt):                                                   # classes [2, None, 2, None, 2]
    ca, kw, t = _tools(dt)
    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Drift(t(0.5), **kw), ca.HorizontalCorrector(t(0.1), angle=t(1e-4), **kw)],
            [ca.Quadrupole(t(0.2), k1=t(-3.0), **DKD, **kw)], [ca.Drift(t(0.3), **kw)], [ca.Dipole(t(0.4), angle=t(0.03), **DKD, **kw)]], \
        [[Q, LIN, Q, LIN, B]], {"drift_kick_drift_run": 1}


def dkd_markers(dt):
    """A Marker between two magnets is no item; one at the end of the stretch is skipped by the returned index (`after[]`): it is
    not tracked as a merged run of its own."""
    ca, kw, t = _tools(dt)
    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Marker(name="between")], [ca.Quadrupole(t(0.2), k1=t(-3.0), **DKD, **kw)],
            [ca.Marker(name="at_the_end")], [ca.Quadrupole(t(0.1), k1=t(1.0), **SO, **kw)]], \
        [[Q, Q]], {"drift_kick_drift_run": 1, "merged_run": 0, "second_order_run": 0, "element": 1}


def dkd_leading_run(dt):                                                    # classes [None, 2, None, 2]
    ca, kw, t = _tools(dt)
    return [[ca.Drift(t(0.4), **kw), ca.Quadrupole(t(0.1), k1=t(0.7), **kw)], [ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)],
            [ca.Drift(t(0.3), **kw)], [ca.Quadrupole(t(0.2), k1=t(-3.0), **DKD, **kw)]], \
        [[LIN, Q, LIN, Q]], {"run_ahead_of_nonlinear": 1, "drift_kick_drift_run": 0, "merged_run": 0}


def dkd_two_classes(dt):                                                    # float32: classes [1, 1, 2, None, 2]; float64: [0, 0, 0, None, 0]
    ca, kw, t = _tools(dt)
    pieces = [[ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Drift(t(0.5), **DKD, **kw)], [ca.Quadrupole(t(0.2), k1=t(-3.0), **DKD, **kw)],
              [ca.Drift(t(0.3), **kw)], [ca.Quadrupole(t(0.2), k1=t(2.0), **DKD, **kw)]]
    pieces[0][0].dkd_precision = pieces[1][0].dkd_precision = "storage"
    if dt == torch.float32:
        return pieces, [[Q, D], [Q, LIN, Q]], {"drift_kick_drift_run": 2}
    return pieces, [[Q, D, Q, LIN, Q]], {"drift_kick_drift_run": 1}


def dkd_tdc_in_front_of_magnets(dt):
    """The stock TransverseDeflectingCavity does not say which tensors its parameters are (`_dkd_scalar_refs()` is None), so it is
    no item at all: each is tracked on its own, and the stretch behind them is one call."""
    ca, kw, t = _tools(dt)
    tdc = lambda: ca.TransverseDeflectingCavity(t(0.3), voltage=t(2e4), phase=t(0.1), frequency=t(1e9), **kw)  # noqa: E731
    return [[tdc()], [tdc()], [ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Drift(t(0.3), **kw)]], \
        [[Q, LIN]], {"drift_kick_drift_run": 1, "element": 2}


def dkd_kind_outside_registers(dt):                                         # classes [-1, -1, 2, None]
    """A kind outside `_DKD_IN_REGISTERS` that IS an item (a TransverseDeflectingCavity that names its parameter tensors) takes
    element passes: the fall-back call stops where a stretch can start."""
    ca, kw, t = _tools(dt)

    class NamedTdc(ca.TransverseDeflectingCavity):
        def _dkd_scalar_refs(self):
            length, voltage, phase, frequency, tilt, m = self._settings("length", "voltage", "phase", "frequency", "tilt", "misalignment")
            return [(length, None), (voltage, None), (phase, None), (frequency, None), (tilt, None), (m, 0), (m, 1)]

    tdc = lambda: NamedTdc(t(0.3), voltage=t(2e4), phase=t(0.1), frequency=t(1e9), **kw)  # noqa: E731
    return [[tdc()], [tdc()], [ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Drift(t(0.3), **kw)]], \
        [[TDC, TDC], [Q, LIN]], {"drift_kick_drift_run": 2}


def dkd_run_that_does_not_qualify(dt):
    """A vectorised setting inside a linear run: the stretch ends in front of it (`k = failed`); behind it the beam is vectorised."""
    ca, kw, t = _tools(dt)
    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Drift(t(0.3), **kw)], [ca.Quadrupole(t(0.2), k1=t(-3.0), **DKD, **kw)],
            [ca.Drift(t(0.3), **kw), ca.HorizontalCorrector(t(0.1), angle=t([1e-4, 2e-4]), **kw)], [ca.Quadrupole(t(0.2), k1=t(2.0), **DKD, **kw)]], \
        [[Q, LIN, Q]], {"drift_kick_drift_run": 1, "merged_run": 1, "element": 1}


def dkd_run_in_front_of_a_cavity(dt):
    """The run in front of an active Cavity belongs to the cavity's stretch."""
    ca, kw, t = _tools(dt)
    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Quadrupole(t(0.2), k1=t(-3.0), **DKD, **kw)], [ca.Drift(t(0.3), **kw)],
            [ca.Cavity(t(0.5), voltage=t(1e6), phase=t(10.0), frequency=t(1.3e9), **kw)]], \
        [[Q, Q]], {"drift_kick_drift_run": 1, "lattice_stretch": 1}


def dkd_single_element(dt):                                                 # classes [2]
    ca, kw, t = _tools(dt)
    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Quadrupole(t(0.2), k1=t(1.0), **SO, **kw)],
            [ca.Quadrupole(t(0.2), k1=t(-3.0), **DKD, **kw)]], \
        [], {"drift_kick_drift_run": 0, "second_order_run": 0, "element": 3}


def dkd_overridden_track(dt):
    ca, kw, t = _tools(dt)

    class MyQuad(ca.Quadrupole):
        def track(self, incoming):
            return super().track(incoming)

    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Drift(t(0.5), **DKD, **kw)], [MyQuad(t(0.2), k1=t(-3.0), **DKD, **kw)],
            [ca.Drift(t(0.5), **DKD, **kw)], [ca.Quadrupole(t(0.2), k1=t(2.0), **DKD, **kw)]], \
        [[Q, D], [D, Q]], {"drift_kick_drift_run": 2, "element": 1}


def dkd_vectorised_magnet(dt):
    ca, kw, t = _tools(dt)
    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw)], [ca.Drift(t(0.5), **DKD, **kw)],
            [ca.Quadrupole(t(0.2), k1=t([-3.0, -2.0]), **DKD, **kw)], [ca.Drift(t(0.5), **DKD, **kw)]], \
        [[Q, D]], {"drift_kick_drift_run": 1, "element": 2}                 # (behind it the beam is vectorised: no run)


DKD_CASES = [dkd_magnets_only, dkd_runs_between, dkd_markers, dkd_leading_run, dkd_two_classes, dkd_tdc_in_front_of_magnets, dkd_kind_outside_registers,
             dkd_run_that_does_not_qualify, dkd_run_in_front_of_a_cavity, dkd_single_element, dkd_overridden_track, dkd_vectorised_magnet]


def so_magnets_only(dt):
    ca, kw, t = _tools(dt)
    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **SO, **kw)], [ca.Drift(t(0.5), **SO, **kw)], [ca.Sextupole(t(0.1), k2=t(9.0), **SO, **kw)],
            [ca.Dipole(t(0.4), angle=t(0.03), **SO, **kw)]], [4], {"second_order_run": 1}


def so_runs_between(dt):
    ca, kw, t = _tools(dt)
    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **SO, **kw)], [ca.Drift(t(0.5), **kw), ca.HorizontalCorrector(t(0.1), angle=t(1e-4), **kw)],
            [ca.Sextupole(t(0.1), k2=t(9.0), **SO, **kw)], [ca.Drift(t(0.3), **kw)], [ca.Quadrupole(t(0.2), k1=t(-3.0), **SO, **kw)]], \
        [5], {"second_order_run": 1}


def so_markers(dt):
    """The second-order scan counts a trailing Marker run into the stretch's end as well: nothing else tracks it."""
    ca, kw, t = _tools(dt)
    return [[ca.Quadrupole(t(0.2), k1=t(3.0), **SO, **kw)], [ca.Marker(name="between")], [ca.Quadrupole(t(0.2), k1=t(-3.0), **SO, **kw)],
            [ca.Marker(name="at_the_end")], [ca.Quadrupole(t(0.1), k1=t(1.0), **DKD, **kw)]], \
        [2], {"second_order_run": 1, "merged_run": 0, "drift_kick_drift_run": 0, "element": 1}


def so_leading_run(dt):
    ca, kw, t = _tools(dt)
    return [[ca.Drift(t(0.4), **kw), ca.Quadrupole(t(0.1), k1=t(0.7), **kw)], [ca.Quadrupole(t(0.2), k1=t(3.0), **SO, **kw)],
            [ca.Drift(t(0.3), **kw)], [ca.Quadrupole(t(0.2), k1=t(-3.0), **SO, **kw)]], \
        [4], {"run_ahead_of_nonlinear": 1, "second_order_run": 0, "merged_run": 0}


SO_CASES = [so_magnets_only, so_runs_between, so_markers, so_leading_run]


def _check(case, dt, spy_name, cache_name):
    import cheetah_amd as ca
    from cheetah_amd import _ops
    from cheetah_amd.accelerator import _planner

    pieces, expected, taken = case(dt)
    beam = _beam(dt)
    seg = ca.Segment([e for piece in pieces for e in piece])
    subs = [ca.Segment(piece) if piece[0].is_skippable else piece[0] for piece in pieces]
    assert all(len(piece) == 1 or all(e.is_skippable for e in piece) for piece in pieces)
    ref = beam
    for piece in subs:
        ref = piece.track(ref)
    calls, orig = [], getattr(_ops, spy_name)
    record = (lambda a: list(a[0])) if spy_name == "dkd_chain" else (lambda a: len(a[0]))
    setattr(_ops, spy_name, lambda *a, **k: (calls.append(record(a)), orig(*a, **k))[1])
    try:
        before = dict(_planner.TAKEN)
        first = seg.track(beam)
        delta = {name: _planner.TAKEN[name] - before[name] for name in taken}
        first_calls = list(calls)
        again = seg.track(beam)                               # every stretch from the kept run
    finally:
        setattr(_ops, spy_name, orig)
    assert first_calls == expected, first_calls
    assert delta == taken, delta
    assert calls == expected + expected, calls
    for out in (first, again):
        assert torch.equal(out.particles, ref.particles) and torch.equal(out.energy, ref.energy) and torch.equal(out.s, ref.s)
    assert out.particles.shape == ref.particles.shape
    kept = seg.__dict__.get(cache_name)
    assert (len(kept[1]) if kept is not None else 0) == len(expected), kept


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", DKD_CASES, ids=[c.__name__ for c in DKD_CASES])
def test_drift_kick_drift_partition(case, dt):
    _check(case, dt, "dkd_chain", "_dkd_run_cache")


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", SO_CASES, ids=[c.__name__ for c in SO_CASES])
def test_second_order_partition(case, dt):
    _check(case, dt, "second_order_chain", "_so_run_cache")


def test_an_unknown_precision_ends_the_stretch():
    """The element itself refuses to track with an unknown `dkd_precision`; the stretch in front of it is still one call."""
    import cheetah_amd as ca
    from cheetah_amd import _ops

    ca, kw, t = _tools(torch.float32)
    els = [ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw), ca.Drift(t(0.5), **DKD, **kw), ca.Quadrupole(t(0.2), k1=t(-3.0), **DKD, **kw)]
    els[2].dkd_precision = "half"
    calls, orig = [], _ops.dkd_chain
    _ops.dkd_chain = lambda *a, **k: (calls.append(list(a[0])), orig(*a, **k))[1]
    try:
        with pytest.raises(ValueError, match="dkd_precision must be 'double', 'mixed' or 'storage', got 'half'"):
            ca.Segment(els).track(_beam(torch.float32))
    finally:
        _ops.dkd_chain = orig
    assert calls == [[Q, D]], calls
