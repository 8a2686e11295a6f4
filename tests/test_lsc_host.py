"""The LSCKick element without a GPU: exports and C-ABI symbols, workspace queries and rejected arguments, constructor errors,
element basics, LatticeJSON with and without a radius, the structure of Segment.with_lsc_kicks, and the errors of tracking a beam
that cannot be tracked here (before any device work)."""
import re
import subprocess

import pytest
import torch

NEW_SYMBOLS = ("chx_lsc_workspace_bytes", "chx_lsc_kick", "chx_lsc_kick_bwd")


def test_exported_from_the_package_and_the_accelerator_module():
    import cheetah_amd as ca
    import cheetah_amd.accelerator as acc

    assert ca.LSCKick is acc.LSCKick
    assert issubclass(ca.LSCKick, ca.Element)
    assert ca._ops.LSC_MAX_BINS == 4096
    assert callable(ca._ops.lsc_kick) and callable(ca._ops.lsc_scale_rho) and callable(ca.Segment.with_lsc_kicks)


def test_lsc_symbols_exported_and_bound():
    import cheetah_amd._lib as L

    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (chx_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.chx_abi_version() == 9


def test_workspace_and_invalid_arguments_on_the_host():
    import cheetah_amd._lib as L

    lib = L.lib()
    assert lib.chx_lsc_workspace_bytes(1, 10**6, 500) > 0
    assert lib.chx_lsc_workspace_bytes(4, 10**6, 4096) > lib.chx_lsc_workspace_bytes(1, 10**6, 4096)
    assert lib.chx_lsc_workspace_bytes(1, 10**6, 1) == 0
    assert lib.chx_lsc_workspace_bytes(1, 10**6, 4097) == 0
    assert lib.chx_lsc_workspace_bytes(0, 10**6, 200) == 0
    assert lib.chx_lsc_workspace_bytes(1, 0, 200) == 0
    # rejected before any device work: no particles, M out of range, a non-positive mass
    assert lib.chx_lsc_kick(None, None, None, None, None, None, 511e3, 1.0, 1, 1, 1, 1, 1, 1, 1, 10, 8, 0, None, None, None, 0,
                            None) == -1
    assert lib.chx_lsc_kick_bwd(None, None, None, 1, 1, 1, 1, 10, 8, 0, None, None, None, None, None, None, None, 0, None) == -1
    x = torch.zeros(10, 7, dtype=torch.float64)
    q = w = torch.ones(10, dtype=torch.float64)
    e = torch.ones(1, dtype=torch.float64)
    p = [t.data_ptr() for t in (x, q, w, e, e, e)]
    state = torch.zeros(64, dtype=torch.float64)
    for M, mass in ((1, 511e3), (4097, 511e3), (8, 0.0), (8, -1.0)):
        assert lib.chx_lsc_kick(*p, mass, 1.0, 1, 1, 1, 1, 1, 1, 1, 10, M, 1, x.data_ptr(), state.data_ptr(), None, 0, None) == -1
    # the backward pass needs both per-row outputs
    assert lib.chx_lsc_kick_bwd(*p[:3], 1, 1, 1, 1, 10, 8, 1, state.data_ptr(), x.data_ptr(), x.data_ptr(), None, e.data_ptr(), None,
                                None, 0, None) == -1


def _kick(**kw):
    import cheetah_amd as ca

    args = {"effect_length": torch.tensor(0.5), "beam_radius": torch.tensor(2e-4)}
    args.update(kw)
    return ca.LSCKick(**args)


@pytest.mark.parametrize("kw", [
    {"num_bins": 1},
    {"num_bins": 4097},
    {"num_bins": 0},
    {"num_bins": 2.5},
    {"num_bins": True},
    {"effect_length": torch.tensor(-0.1)},
    {"effect_length": torch.tensor([0.1, -1e-3])},
    {"effect_length": torch.tensor(float("nan"))},
    {"effect_length": torch.tensor(float("inf"))},
    {"beam_radius": torch.tensor(0.0)},
    {"beam_radius": torch.tensor(-1e-4)},
    {"beam_radius": torch.tensor([1e-4, 0.0])},
    {"beam_radius": torch.tensor(float("nan"))},
    {"beam_radius": torch.tensor(float("inf"))},
    {"beam_radius": None, "radius_factor": 0.0},
    {"beam_radius": None, "radius_factor": float("nan")},
])
def test_constructor_value_errors(kw):
    with pytest.raises(ValueError):
        _kick(**kw)


def test_element_basics():
    import cheetah_amd as ca

    k = _kick(num_bins=37, name="lsc1")
    assert not k.is_skippable
    assert float(k.length) == 0.0
    assert k.split(torch.tensor(0.1)) == [k]
    assert k.defining_features == ["name", "effect_length", "beam_radius", "radius_factor", "num_bins"]
    assert k.defining_tensors == ["effect_length", "beam_radius"]
    r = repr(k)
    assert r.startswith("LSCKick(name='lsc1', effect_length=tensor(0.5000)") and "num_bins=37" in r and "radius_factor=1.7" in r
    c = k.clone()
    assert type(c) is type(k) and c.name == "lsc1" and c.num_bins == 37 and c.radius_factor == 1.7
    for f in ("effect_length", "beam_radius"):
        assert torch.equal(getattr(c, f), getattr(k, f)) and getattr(c, f) is not getattr(k, f)
    d = ca.LSCKick(torch.tensor(0.5))
    assert d.num_bins == 200 and d.beam_radius is None and d.radius_factor == 1.7
    assert d.defining_tensors == ["effect_length"] and d.clone().beam_radius is None
    with pytest.raises(NotImplementedError):
        d.first_order_transfer_map(torch.tensor(1e8), ca.Species("electron"))
    # batched settings and float arguments
    b = ca.LSCKick([0.1, 0.2, 0.0], torch.tensor([[1e-4], [2e-4]], dtype=torch.float64), dtype=torch.float64)
    assert b.effect_length.shape == (3,) and b.effect_length.dtype == torch.float64 and b.beam_radius.shape == (2, 1)
    p = ca.LSCKick(torch.nn.Parameter(torch.tensor(0.3)), torch.nn.Parameter(torch.tensor(1e-4)))
    assert {n for n, _ in p.named_parameters()} == {"effect_length", "beam_radius"}


@pytest.mark.parametrize("radius", [None, 3e-4])
def test_lattice_json_round_trip(tmp_path, radius):
    import json

    import cheetah_amd as ca

    k = _kick(effect_length=torch.tensor(0.25), beam_radius=None if radius is None else torch.tensor(radius), radius_factor=1.3,
              num_bins=123, name="lsck")
    seg = ca.Segment([ca.Drift(torch.tensor(1.0), name="d1"), k, ca.Drift(torch.tensor(0.5), name="d2")], name="lat")
    path = tmp_path / "lattice.json"
    ca.latticejson.save_cheetah_model(seg, str(path))
    stored = json.loads(path.read_text())["elements"]["lsck"]
    assert stored[0] == "LSCKick" and (stored[1]["beam_radius"] is None) == (radius is None)
    back = ca.latticejson.load_cheetah_model(str(path))
    k2 = back.elements[1]
    assert type(k2) is ca.LSCKick and k2.name == "lsck" and k2.num_bins == 123 and k2.radius_factor == 1.3
    assert torch.allclose(k2.effect_length, k.effect_length)
    if radius is None:
        assert k2.beam_radius is None
    else:
        assert torch.allclose(k2.beam_radius, k.beam_radius)


def test_with_lsc_kicks_structure():
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    inner = ca.Segment([ca.Quadrupole(t(0.3), k1=t(1.0), name="q3"), ca.Marker(name="m3"), ca.Drift(t(0.2), name="d3")],
                       name="inner")
    seg = ca.Segment([ca.Drift(t(1.0), name="d1"), ca.Marker(name="m1"), ca.Quadrupole(t(0.1), k1=t(2.0), name="q1"),
                      ca.Drift(t(0.0), name="empty"), ca.CSRKick(t(0.1), t(0.02), name="csr"),
                      ca.LSCKick(t(0.4), t(1e-4), name="lsc"), ca.SpaceChargeKick(t(0.3), name="sc"), inner,
                      ca.Drift(t(0.7), name="keep"), ca.Drift(t([0.0, 0.6]), name="batched")], name="lat")
    out = seg.with_lsc_kicks(num_bins=77, radius_factor=1.5, except_for=["keep"])
    assert type(out) is ca.Segment and out.name == "lat"
    assert [e.name for e in out.elements] == ["d1", "d1_lsc_kick", "m1", "q1", "q1_lsc_kick", "empty", "csr", "lsc", "sc", "inner",
                                              "keep", "batched", "batched_lsc_kick"]
    assert [e.name for e in out.elements[9].elements] == ["q3", "q3_lsc_kick", "m3", "d3", "d3_lsc_kick"]
    kicks = [e for e in out.elements + out.elements[9].elements if e.name.endswith("_lsc_kick")]
    assert all(type(k) is ca.LSCKick and k.num_bins == 77 and k.radius_factor == 1.5 and k.beam_radius is None for k in kicks)
    # the kick's effect_length IS the element's length: in-place edits and gradients follow
    assert out.elements[1].effect_length is seg.elements[0].length and out.elements[0] is seg.elements[0]
    assert out.elements[4].effect_length is seg.elements[2].length and out.elements[-1].effect_length is seg.elements[-1].length
    assert torch.allclose(out.length, seg.length)
    # an explicit radius goes to every kick
    a = t(2e-4)
    assert all(k.beam_radius is a for k in seg.with_lsc_kicks(beam_radius=a).elements if k.name.endswith("_lsc_kick"))
    # max_step: elements longer than the step are split first, every piece gets its kick
    stepped = seg.with_lsc_kicks(max_step=0.4)
    names = [e.name for e in stepped.elements]
    assert names[:6] == ["d1_split_0", "d1_split_0_lsc_kick", "d1_split_1", "d1_split_1_lsc_kick", "d1_split_2", "d1_split_2_lsc_kick"]
    assert names[6:9] == ["m1", "q1", "q1_lsc_kick"]
    for piece, kick in zip(stepped.elements[0:6:2], stepped.elements[1:6:2]):
        assert kick.effect_length is piece.length and abs(float(piece.length) - 1 / 3) < 1e-15
    assert torch.allclose(stepped.length, seg.length)
    for bad in ({"num_bins": 1}, {"num_bins": 2.0}, {"radius_factor": -1.0}, {"beam_radius": t(0.0)}, {"max_step": 0.0},
                {"max_step": -1.0}, {"max_step": float("nan")}):
        with pytest.raises(ValueError):
            seg.with_lsc_kicks(**bad)


def test_tracking_errors_before_any_device_work():
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    for k in (_kick(), _kick(beam_radius=None)):
        with pytest.raises(RuntimeError, match="GPU only"):
            k.track(beam)
        with pytest.raises(TypeError, match="needs a ParticleBeam"):
            k.track(ca.ParameterBeam.from_parameters())
        with ca.sharding.particle_sharded():
            with pytest.raises(NotImplementedError, match="particle-sharded"):
                k.track(beam)
