"""The Wakefield element without a GPU: constructor errors, repr / clone / defining features, LatticeJSON, split, the C-ABI entry
points exported and bound, and the errors of tracking a beam that cannot be tracked here (before any device work)."""
import re
import subprocess

import pytest
import torch

NEW_SYMBOLS = ("chx_wake_workspace_bytes", "chx_wake_kick", "chx_wake_kick_bwd")


def _wake(**kw):
    import cheetah_amd as ca

    args = {"wake_spacing": torch.tensor(1e-5), "longitudinal_wake": torch.linspace(2e13, 0.0, 64)}
    args.update(kw)
    return ca.Wakefield(**args)


def test_exported_from_the_package_and_the_accelerator_module():
    import cheetah_amd as ca
    import cheetah_amd.accelerator as acc

    assert ca.Wakefield is acc.Wakefield
    assert issubclass(ca.Wakefield, ca.Element)
    assert ca._ops.WAKE_MAX_BINS == 4096


def test_wake_symbols_exported_and_bound():
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
    assert lib.chx_wake_workspace_bytes(1, 10**6, 1000) > 0
    assert lib.chx_wake_workspace_bytes(4, 10**6, 4096) > lib.chx_wake_workspace_bytes(1, 10**6, 4096)
    assert lib.chx_wake_workspace_bytes(1, 10**6, 1) == 0
    assert lib.chx_wake_workspace_bytes(1, 10**6, 4097) == 0
    # rejected before any device work: no particles, no table, M out of range
    assert lib.chx_wake_kick(None, None, None, None, None, 0, None, 0, None, 1, 1, 1, 1, 10, 8, 0, None, None, None, 0, None) == -1
    assert lib.chx_wake_kick_bwd(None, None, None, None, None, 0, None, 0, None, 1, 1, 1, 1, 10, 8, 0, None, None, None, None, None,
                                 None, None, None, 0, None) == -1


@pytest.mark.parametrize("kw", [
    {"num_bins": 1},
    {"num_bins": 4097},
    {"num_bins": 0},
    {"num_bins": 2.5},
    {"num_bins": True},
    {"longitudinal_wake": torch.ones(3, 4)},
    {"longitudinal_wake": torch.tensor(1.0)},
    {"longitudinal_wake": torch.ones(8), "transverse_wake": torch.ones(2, 2)},
    {"longitudinal_wake": None},
    {"longitudinal_wake": torch.zeros(0)},
    {"wake_spacing": torch.tensor(0.0)},
    {"wake_spacing": torch.tensor(-1e-5)},
    {"wake_spacing": torch.tensor(float("nan"))},
    {"wake_spacing": torch.tensor([1e-5, 2e-5])},
    {"wake_spacing": None},
])
def test_constructor_value_errors(kw):
    with pytest.raises(ValueError):
        _wake(**kw)


def test_element_basics():
    w = _wake(factor=torch.tensor(3.0), num_bins=37, name="wake1")
    assert not w.is_skippable
    assert float(w.length) == 0.0
    assert w.split(torch.tensor(0.1)) == [w]
    assert w.transverse_wake.shape == (0,)
    assert w.defining_features == ["name", "wake_spacing", "longitudinal_wake", "transverse_wake", "factor", "num_bins"]
    assert w.defining_tensors == ["wake_spacing", "longitudinal_wake", "transverse_wake", "factor"]
    r = repr(w)
    assert r.startswith("Wakefield(name='wake1', wake_spacing=tensor(1.0000e-05)") and "num_bins=37" in r
    c = w.clone()
    assert type(c) is type(w) and c.name == "wake1" and c.num_bins == 37
    for f in ("wake_spacing", "longitudinal_wake", "transverse_wake", "factor"):
        assert torch.equal(getattr(c, f), getattr(w, f)) and getattr(c, f) is not getattr(w, f)
    # transverse only, default factor
    t = _wake(longitudinal_wake=None, transverse_wake=torch.linspace(0.0, 1e15, 10))
    assert t.longitudinal_wake.shape == (0,) and float(t.factor) == 1.0 and t.num_bins == 200


def test_lattice_json_round_trip_with_one_table_absent(tmp_path):
    import cheetah_amd as ca

    w = _wake(longitudinal_wake=None, transverse_wake=torch.linspace(0.0, 1e15, 10), factor=torch.tensor(2.5), num_bins=123,
              name="trwake")
    seg = ca.Segment([ca.Drift(torch.tensor(1.0), name="d1"), w, ca.Drift(torch.tensor(0.5), name="d2")], name="lat")
    path = tmp_path / "lattice.json"
    ca.latticejson.save_cheetah_model(seg, str(path))
    back = ca.latticejson.load_cheetah_model(str(path))
    w2 = back.elements[1]
    assert type(w2) is ca.Wakefield and w2.name == "trwake" and w2.num_bins == 123
    assert w2.longitudinal_wake.shape == (0,)
    assert torch.allclose(w2.transverse_wake, w.transverse_wake)
    assert float(w2.factor) == 2.5 and torch.allclose(w2.wake_spacing, w.wake_spacing)


def test_tracking_errors_before_any_device_work():
    import cheetah_amd as ca

    w = _wake()
    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    with pytest.raises(RuntimeError, match="GPU only"):
        w.track(beam)
    with pytest.raises(TypeError):
        w.track(ca.ParameterBeam.from_parameters())
    with ca.sharding.particle_sharded():
        with pytest.raises(NotImplementedError, match="particle-sharded"):
            w.track(beam)
