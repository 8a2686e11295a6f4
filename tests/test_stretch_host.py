"""The pure host-side pieces of the stretch call (cheetah_amd/accelerator/_stretch.py), without a device: the expectations are
what `Segment._lead_at`, the extent loop of `Segment._lattice_stretch` and its host-side path-length sum gave before these moved
out of segment.py, written down as literals."""
import copy
import types

import pytest
import torch

import cheetah_amd as ca
from cheetah_amd.accelerator import _stretch


def _drift(name, length=0.5):
    return ca.Drift(length=torch.tensor(length), name=name)


def _cavity(name):
    return ca.Cavity(length=torch.tensor(1.0), voltage=torch.tensor(1e6), phase=torch.tensor(0.0), frequency=torch.tensor(1.3e9), name=name)


@pytest.mark.parametrize("lead_in, acc, energy_shape, expected", [
    ((), (8,), (), (8,)),
    ((8, 1), (8, 4), (), (8, 4)),
    ((), (), (64,), (64,)),
    ((3,), (2, 3), (2, 1), (2, 3)),
    ((4,), (4,), (4,), (4,)),            # equal inputs
    ((2, 3), (2, 3), (), (2, 3)),
    ((5,), None, (), (5,)),              # no vectorised setting in front of the point
])
def test_lead_at(lead_in, acc, energy_shape, expected):
    got = _stretch._lead_at(lead_in, acc, torch.Size(energy_shape))
    assert got == expected and type(got) is tuple


_SCREEN_LATTICE = lambda: [_drift("a"), _cavity("c"), ca.Screen(is_active=True, name="s"), _drift("b"), _cavity("c2")]  # noqa: E731


@pytest.mark.parametrize("elements, with_screens, kinds, expected", [
    (lambda: [_drift("a"), _cavity("c"), _drift("b")], True, ["run", "element", "run"], [(3, 1), (3, 1), (3, 0)]),
    (lambda: [_drift("a"), ca.BPM(is_active=True, name="m"), _drift("b"), _cavity("c")], True,
     ["run", "element", "run", "element"], [(4, 2), (4, 2), (4, 1), (4, 1)]),
    (_SCREEN_LATTICE, True, ["run", "element", "element", "run", "element"], [(5, 3), (5, 3), (5, 2), (5, 1), (5, 1)]),
    (_SCREEN_LATTICE, False, ["run", "element", "element", "run", "element"], [(2, 1), (2, 1), (2, 0), (5, 1), (5, 1)]),
    (lambda: [_drift("a"), ca.SpaceChargeKick(torch.tensor(1.0), name="k"), _drift("b")], True,
     ["run", "element", "run"], [(1, 0), (1, 0), (3, 0)]),
])
def test_extent(elements, with_screens, kinds, expected):
    """(end, items that are no runs) of the stretch from every plan item."""
    plan = ca.Segment(elements())._plan()
    assert [kind for kind, _ in plan] == kinds
    assert [_stretch.extent(plan, i, with_screens) for i in range(len(plan))] == expected


def test_joins_keeps_the_moments_entry_asymmetry():
    """An aperture is walked over by the extent loop, but the ParameterBeam walk does not START a stretch at one."""
    aperture = ca.Aperture(x_max=torch.tensor(1e-3), y_max=torch.tensor(1e-3), is_active=True, name="ap")
    assert _stretch.joins("element", aperture) and not _stretch.joins("element", aperture, apertures=False)
    screen = ca.Screen(is_active=True, name="s")
    assert _stretch.joins("element", screen) and not _stretch.joins("element", screen, screens=False)
    assert _stretch.joins("run", None, screens=False, apertures=False)
    assert not _stretch.joins("element", ca.SpaceChargeKick(torch.tensor(1.0), name="k"))


def test_host_side_path_length():
    """`s` behind [Cavity | run | BPM] for an incoming `s` the launch does not take: the lengths summed on the host's side."""
    seg = ca.Segment([_cavity("c"), _drift("a"), _drift("b", 0.25), ca.BPM(is_active=True, name="m")])
    plan = seg._plan()
    assert [kind for kind, _ in plan] == ["element", "run", "element"]
    lp = types.SimpleNamespace(items=plan, count=len(plan))
    s_out = _stretch._s_out_host(seg, lp, torch.tensor(2.0))
    assert s_out.item() == 3.75 and s_out.item() == 2.0 + seg.length.item()
    lp.count = 1           # (the table ended behind the cavity: only its length)
    assert _stretch._s_out_host(seg, lp, torch.tensor(2.0)).item() == 3.0


def test_cache_entries_also_on_a_copied_segment():
    """One entry per (start, dtype, device, ..., with_screens); a copy travels without derived state and starts its own table."""
    seg = ca.Segment([_drift("a"), _cavity("c"), _drift("b")])
    plan = seg._plan()
    key = (0, torch.float32, torch.device("cpu"), True)
    entry = _stretch._entry(seg, plan, 0, key)
    assert entry == [3, None] and _stretch._entry(seg, plan, 0, key) is entry and seg.__dict__["_lattice_cache"][0] is plan
    assert _stretch._entry(seg, plan, 2, (2,) + key[1:]) is False                                  # (a run alone: no stretch)
    assert _stretch._entry(seg, plan, 0, (0, torch.float64) + key[2:], worth=False) is False       # (the caller's own test)
    clone = copy.deepcopy(seg)
    assert clone.__dict__["_lattice_store"] is None
    assert _stretch._entry(clone, clone._plan(), 0, key) == [3, None] and _stretch._entry(seg, plan, 0, key) is entry
