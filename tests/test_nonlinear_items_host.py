"""What is an item of a run of non-linear elements, without a GPU: the rule that decides whether an element is a drift-kick-drift
item, asked through `Segment._turn_items_dkd` on CPU tensors (the ring refuses with the rule's reason, so every branch has a text
to compare), and the partition of a list of arithmetic classes into stretches (`accelerator/_nonlinear.py`: `stretch_length`,
`fallback_length` — the scanner of `Segment._dkd_run` as a pure function).

The reason strings were recorded before the rule moved out of `Segment`: they must come out byte for byte."""
import pytest
import torch

F32, F64 = torch.float32, torch.float64
DKD = {"tracking_method": "drift_kick_drift"}
NOT_AN_ITEM = "is not a drift-kick-drift Drift, Quadrupole, Dipole, Sextupole, RFCavity or Multipole"
NOT_SCALARS = "are not all scalars of the beam's dtype on its device (vectorised settings take the general path)"


def t(v, dtype=F64):
    return torch.tensor(v, dtype=dtype)


def ring_of(*middle, dtype=F64):
    """Quadrupole, drift, `middle`, drift: a ring that qualifies when `middle` does."""
    import cheetah_amd as ca

    kw = {"dtype": dtype}
    return ca.Segment([ca.Quadrupole(t(0.2, dtype), k1=t(1.5, dtype), name="qf", **DKD, **kw), ca.Drift(t(0.5, dtype), name="d1", **DKD, **kw),
                       *middle, ca.Drift(t(0.7, dtype), name="d2", **DKD, **kw)])


def rule(seg, dtype=F64, trainable=()):
    return seg._turn_items_dkd(seg._plan(), torch.empty((0, 7), dtype=dtype), trainable)


def quad(name="q", dtype=F64, cls=None, **kw):
    import cheetah_amd as ca

    kw = {**DKD, **kw}
    return (cls or ca.Quadrupole)(t(0.2, dtype), k1=kw.pop("k1", t(-1.5, dtype)), name=name, dtype=dtype, **kw)


def _bad_elements():
    import cheetah_amd as ca

    class TrackQuad(ca.Quadrupole):
        def track(self, incoming):
            return super().track(incoming)

    class DkdQuad(ca.Quadrupole):
        def _track_drift_kick_drift(self, incoming):
            return super()._track_drift_kick_drift(incoming)

    class InternalQuad(ca.Quadrupole):
        def _track_internal(self, incoming):
            return super()._track_internal(incoming)

    half = quad("qh")
    half.dkd_precision = "half"
    return [
        ("second_order", quad("qs", tracking_method="second_order"), f"Quadrupole 'qs' (tracking method 'second_order') {NOT_AN_ITEM}"),
        ("kind_not_in_registers", ca.TransverseDeflectingCavity(t(0.3), voltage=t(1e5), phase=t(0.1), frequency=t(1e9), name="tdc", dtype=F64),
         f"TransverseDeflectingCavity 'tdc' (tracking method 'drift_kick_drift') {NOT_AN_ITEM}"),
        ("overrides_track", quad("qt", cls=TrackQuad), "TrackQuad 'qt' overrides `track`"),
        ("overrides_track_dkd", quad("qd", cls=DkdQuad), "DkdQuad 'qd' overrides `track`"),
        ("overrides_track_internal", quad("qi", cls=InternalQuad), "InternalQuad 'qi' overrides `track`"),
        ("unknown_precision", half, "Quadrupole 'qh' has the unknown dkd_precision 'half'"),
        ("vectorised_setting", quad("qv", k1=t([1.0, 2.0])), f"the settings of Quadrupole 'qv' {NOT_SCALARS}"),
        ("wrong_dtype_setting", quad("q32", dtype=F32), f"the settings of Quadrupole 'q32' {NOT_SCALARS}"),
        ("linear_run", ca.Quadrupole(t(0.2), k1=t(0.3), name="ql", dtype=F64),
         "a run of linear elements stands in the ring (its map depends on the reference energy in front of it, and an energy that drifts "
         "from turn to turn would need a map per turn: left to the general path on purpose)"),
    ]


BAD_IDS = ["second_order", "kind_not_in_registers", "overrides_track", "overrides_track_dkd", "overrides_track_internal", "unknown_precision",
           "vectorised_setting", "wrong_dtype_setting", "linear_run"]


@pytest.mark.parametrize("row", range(len(BAD_IDS)), ids=BAD_IDS)
def test_a_bad_element_is_refused_with_its_reason(row):
    name, element, reason = _bad_elements()[row]
    assert name == BAD_IDS[row]
    assert rule(ring_of(element)) == reason
    # the first bad element speaks: one that qualifies in front of it changes nothing, and the rule reads the element every time
    assert rule(ring_of(quad("ok"), element)) == reason
    assert rule(ring_of(element)) == reason


def test_a_ring_that_qualifies_gives_its_argument_set():
    import cheetah_amd as ca
    from cheetah_amd import _ops

    K = _ops.DKD_KIND
    sext = ca.Sextupole(t(0.1), k2=t(4.0), num_steps=3, name="s", dtype=F64, **DKD)
    bend = ca.Dipole(t(0.4), angle=t(0.05), fringe_at="entrance", name="b", dtype=F64, **DKD)
    seg = ring_of(sext, ca.Marker(name="m"), bend)
    ring = rule(seg)
    assert type(ring).__name__ == "_DkdRing"
    assert ring.kinds == [K["quadrupole"], K["drift"], K["sextupole"], K["dipole"], K["drift"]]      # the Marker is no item
    assert [tuple(p.shape) for p in ring.params] == [(1, n) for n in (5, 1, 5, 9, 1)] and all(p.dtype == F64 for p in ring.params)
    assert ring.num_steps == [e._dkd_options()[0] for e in seg.elements if e.name != "m"] and ring.num_steps[2] == 3
    assert ring.fringe_at == [e._dkd_options()[1] for e in seg.elements if e.name != "m"] and ring.fringe_at[3] == _ops.FRINGE_AT["entrance"]
    assert ring.storage == 0                                # a float64 ring is one class, whatever `dkd_precision` says


@pytest.mark.parametrize("count,reason", [(0, "the ring has 0 drift-kick-drift elements, the fused kernel takes 1 to 192"),
                                          (192, None),
                                          (193, "the ring has 193 drift-kick-drift elements, the fused kernel takes 1 to 192")])
def test_the_ring_takes_1_to_192_elements(count, reason):
    import cheetah_amd as ca

    length = t(0.1)
    seg = ca.Segment([ca.Marker(name="start")] + [ca.Drift(length, name=f"d{k}", dtype=F64, **DKD) for k in range(count)])
    got = rule(seg)
    if reason is None:
        assert len(got.kinds) == count
    else:
        assert got == reason


def test_two_arithmetic_classes_are_one_on_a_float64_ring():
    from cheetah_amd import _ops

    reason = "the elements' `dkd_precision` settings put them into more than one arithmetic class (one launch evaluates one)"
    for dtype, expected in ((F32, reason), (F64, 0)):
        stored = quad("qs", dtype)
        stored.dkd_precision = "storage"
        got = rule(ring_of(stored, dtype=dtype), dtype)
        assert (got if isinstance(got, str) else got.storage) == expected
    # one class that is not the default: the ring carries its code
    seg = ring_of(dtype=F32)
    for e in seg.elements:
        e.dkd_precision = "storage"
    assert rule(seg, F32).storage == _ops.DKD_PRECISION["storage"] == 1
    assert rule(ring_of(dtype=F32), F32).storage == _ops.DKD_PRECISION["mixed"] == 2


def test_a_trainable_setting_is_taken_only_when_named():
    k1 = t(2.0).requires_grad_(True)
    seg = ring_of(quad("qg", k1=k1))
    assert seg.qg.k1 is k1
    # with autograd on, the element's parameter array is not formed at all (the callers ask under no_grad)
    assert rule(seg) == rule(seg, trainable="all") == f"the settings of Quadrupole 'qg' {NOT_SCALARS}"
    with torch.no_grad():
        assert rule(seg) == "a setting of the lattice requires grad"
        assert rule(seg, trainable={id(seg.qf.k1)}) == "a setting of the lattice requires grad"
        for trainable in ({id(k1)}, "all"):
            assert len(rule(seg, trainable=trainable).kinds) == 4


# ---- the partition of a list of arithmetic classes (no device, no lattice) ------------------------------------------------------------
# Per item: None = a merged run of linear elements (goes with any class), c >= 0 = the arithmetic class of an item the chain keeps
# in registers, -1 = a drift-kick-drift item it takes in element passes only. (stretch_length, fallback_length) of each list.
# The rows named after a case are the class lists of that case in tests/test_gpu_nonlinear_partition.py (DKD_CASES there): the count
# here is the length of the first `_ops.dkd_chain` call observed there — change both tables together.
PARTITIONS = [
    ("magnets_only", [2, 2, 2, 2], 4, 0),
    ("runs_between", [2, None, 2, None, 2], 5, 0),                  # the runs ride along (a trailing run too)
    ("leading_run", [None, 2, None, 2], 4, 0),
    ("two_classes_f32", [1, 1, 2, None, 2], 2, 0),                  # the stretch splits at the boundary ...
    ("two_classes_f32 (behind the first call)", [2, None, 2], 3, 0),
    ("two_classes_f64", [0, 0, 0, None, 0], 5, 0),                  # ... and is one stretch on a float64 beam
    ("kind_outside_registers", [-1, -1, 2, None], 0, 2),            # the fall-back stops where a stretch can start
    ("kind_outside_registers (behind the first call)", [2, None], 2, 0),
    ("single_element", [2], 1, 0),                                  # (fewer than two items: no call — the caller's test)
    ("only a run", [None], 0, 0),
    ("nothing", [], 0, 0),
    ("a run between two classes goes with the first", [1, None, 2, 2], 2, 0),
    ("elements of changing classes, no stretch anywhere", [-1, 1, 2, -1], 0, 4),
    ("a class whose successor is another class starts no stretch", [-1, 1, 2, 2], 0, 2),
    ("a lone -1 in front of a stretch", [-1, 2, 2], 0, 0),          # one element: no call, `Element.track` takes it
    ("the fall-back never takes a run", [-1, -1, None, 2], 0, 2),
    ("a run in front of a classless item", [None, -1, -1], 0, 0),
]


@pytest.mark.parametrize("name,classes,stretch,fallback", PARTITIONS, ids=[p[0] for p in PARTITIONS])
def test_partition_of_a_class_list(name, classes, stretch, fallback):
    from cheetah_amd.accelerator import _nonlinear

    assert _nonlinear.stretch_length(classes) == stretch
    if stretch < 2:
        assert _nonlinear.fallback_length(classes) == fallback
