"""The CSRKick element without a GPU: exports and C-ABI symbols, workspace queries and rejected arguments, constructor errors,
element basics, LatticeJSON, the structure of Dipole.split_for_csr and Segment.with_csr_kicks, and the errors of tracking a beam
that cannot be tracked here (before any device work)."""
import re
import subprocess

import pytest
import torch

NEW_SYMBOLS = ("chx_csr_workspace_bytes", "chx_csr_kick", "chx_csr_kick_bwd")


def test_exported_from_the_package_and_the_accelerator_module():
    import cheetah_amd as ca
    import cheetah_amd.accelerator as acc

    assert ca.CSRKick is acc.CSRKick
    assert issubclass(ca.CSRKick, ca.Element)
    assert ca._ops.CSR_MAX_BINS == 4096
    assert callable(ca._ops.csr_kick) and callable(ca.Dipole.split_for_csr) and callable(ca.Segment.with_csr_kicks)


def test_csr_symbols_exported_and_bound():
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
    assert lib.chx_csr_workspace_bytes(1, 10**6, 500) > 0
    assert lib.chx_csr_workspace_bytes(4, 10**6, 4096) > lib.chx_csr_workspace_bytes(1, 10**6, 4096)
    assert lib.chx_csr_workspace_bytes(1, 10**6, 1) == 0
    assert lib.chx_csr_workspace_bytes(1, 10**6, 4097) == 0
    assert lib.chx_csr_workspace_bytes(0, 10**6, 200) == 0
    assert lib.chx_csr_workspace_bytes(1, 0, 200) == 0
    # rejected before any device work: no particles, M out of range, a non-positive mass
    assert lib.chx_csr_kick(None, None, None, None, None, None, 511e3, 1.0, 1, 1, 1, 1, 1, 1, 1, 10, 8, 0, None, None, None, 0,
                            None) == -1
    assert lib.chx_csr_kick_bwd(None, None, None, 1, 1, 1, 1, 10, 8, 0, None, None, None, None, None, None, 0, None) == -1
    x = torch.zeros(10, 7, dtype=torch.float64)
    q = w = torch.ones(10, dtype=torch.float64)
    e = torch.ones(1, dtype=torch.float64)
    p = [t.data_ptr() for t in (x, q, w, e, e, e)]
    state = torch.zeros(64, dtype=torch.float64)
    for M, mass in ((1, 511e3), (4097, 511e3), (8, 0.0), (8, -1.0)):
        assert lib.chx_csr_kick(*p, mass, 1.0, 1, 1, 1, 1, 1, 1, 1, 10, M, 1, x.data_ptr(), state.data_ptr(), None, 0, None) == -1


def _kick(**kw):
    import cheetah_amd as ca

    args = {"effect_length": torch.tensor(0.1), "angle": torch.tensor(0.02)}
    args.update(kw)
    return ca.CSRKick(**args)


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
    {"angle": torch.tensor(float("nan"))},
])
def test_constructor_value_errors(kw):
    with pytest.raises(ValueError):
        _kick(**kw)


def test_element_basics():
    import cheetah_amd as ca

    k = _kick(num_bins=37, name="csr1")
    assert not k.is_skippable
    assert float(k.length) == 0.0
    assert k.split(torch.tensor(0.1)) == [k]
    assert k.defining_features == ["name", "effect_length", "angle", "num_bins"]
    assert k.defining_tensors == ["effect_length", "angle"]
    r = repr(k)
    assert r.startswith("CSRKick(name='csr1', effect_length=tensor(0.1000)") and "num_bins=37" in r
    c = k.clone()
    assert type(c) is type(k) and c.name == "csr1" and c.num_bins == 37
    for f in ("effect_length", "angle"):
        assert torch.equal(getattr(c, f), getattr(k, f)) and getattr(c, f) is not getattr(k, f)
    d = _kick()
    assert d.num_bins == 200
    with pytest.raises(NotImplementedError):
        d.first_order_transfer_map(torch.tensor(1e8), ca.Species("electron"))
    # batched settings and float arguments
    b = ca.CSRKick([0.1, 0.2, 0.0], torch.tensor([[0.01], [-0.02]], dtype=torch.float64), dtype=torch.float64)
    assert b.effect_length.shape == (3,) and b.effect_length.dtype == torch.float64 and b.angle.shape == (2, 1)
    p = ca.CSRKick(torch.nn.Parameter(torch.tensor(0.3)), torch.nn.Parameter(torch.tensor(0.01)))
    assert {n for n, _ in p.named_parameters()} == {"effect_length", "angle"}


def test_lattice_json_round_trip(tmp_path):
    import cheetah_amd as ca

    k = _kick(effect_length=torch.tensor(0.25), angle=torch.tensor(-0.03), num_bins=123, name="csrk")
    seg = ca.Segment([ca.Drift(torch.tensor(1.0), name="d1"), k, ca.Drift(torch.tensor(0.5), name="d2")], name="lat")
    path = tmp_path / "lattice.json"
    ca.latticejson.save_cheetah_model(seg, str(path))
    back = ca.latticejson.load_cheetah_model(str(path))
    k2 = back.elements[1]
    assert type(k2) is ca.CSRKick and k2.name == "csrk" and k2.num_bins == 123
    assert torch.allclose(k2.effect_length, k.effect_length) and torch.allclose(k2.angle, k.angle)


def _bend(cls="Dipole", fringe_at="both", **kw):
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    common = {"k1": t(0.7), "tilt": t(0.1), "gap": t(0.02), "gap_exit": t(0.03), "fringe_integral": t(0.5),
              "fringe_integral_exit": t(0.4), "fringe_at": fringe_at, "fringe_type": "linear_edge", "name": "b"}
    common.update(kw)
    if cls == "RBend":
        return ca.RBend(t(0.6), angle=t(0.12), rbend_e1=t(0.01), rbend_e2=t(-0.02), **common)
    return ca.Dipole(t(0.6), angle=t(0.12), dipole_e1=t(0.05), dipole_e2=t(0.07), **common)


@pytest.mark.parametrize("cls", ["Dipole", "RBend"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_split_for_csr_structure(cls, n):
    import cheetah_amd as ca

    bend = _bend(cls, tracking_method="drift_kick_drift")
    parts = bend.split_for_csr(n, num_bins=300)
    assert len(parts) == 2 * n
    dips, kicks = parts[0::2], parts[1::2]
    assert all(type(d) is ca.Dipole for d in dips) and all(type(k) is ca.CSRKick for k in kicks)
    for i, (d, k) in enumerate(zip(dips, kicks)):
        assert d.name == f"b_csr_{i}" and k.name == f"b_csr_kick_{i}"
        assert torch.allclose(d.length, bend.length / n) and torch.allclose(d.angle, bend.angle / n)
        assert torch.allclose(k.effect_length, bend.length / n) and torch.allclose(k.angle, bend.angle / n)
        assert k.num_bins == 300
        for f in ("k1", "tilt", "gap", "gap_exit"):
            assert torch.equal(getattr(d, f), getattr(bend, f)), f
        assert d.tracking_method == "drift_kick_drift" and d.fringe_type == "linear_edge"
        first, last = i == 0, i == n - 1
        assert torch.equal(d.dipole_e1, bend.dipole_e1 if first else torch.zeros_like(bend.dipole_e1))
        assert torch.equal(d.dipole_e2, bend.dipole_e2 if last else torch.zeros_like(bend.dipole_e2))
        assert float(d.fringe_integral) == (0.5 if first else 0.0)
        assert float(d.fringe_integral_exit) == (0.4 if last else 0.0)
        assert d.fringe_at == ("both" if first and last else "entrance" if first else "exit" if last else "neither")
    total = sum(float(d.angle) for d in dips)
    assert abs(total - float(bend.angle)) < 1e-15
    if cls == "RBend":   # the effective face angles: rbend_e + angle / 2
        assert abs(float(dips[0].dipole_e1) - (0.01 + 0.06)) < 1e-15 and abs(float(dips[-1].dipole_e2) - (-0.02 + 0.06)) < 1e-15


@pytest.mark.parametrize("fringe_at,first,last", [("entrance", "entrance", "neither"), ("exit", "neither", "exit"),
                                                  ("neither", "neither", "neither")])
def test_split_for_csr_keeps_only_the_original_fringes(fringe_at, first, last):
    parts = _bend(fringe_at=fringe_at).split_for_csr(3)
    assert [parts[0].fringe_at, parts[2].fringe_at, parts[4].fringe_at] == [first, "neither", last]


def test_split_for_csr_leaves_straight_bends_and_rejects_bad_arguments():
    import cheetah_amd as ca

    straight = ca.Dipole(torch.tensor(0.5), angle=torch.tensor(0.0))
    assert straight.split_for_csr(4) == [straight]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            _bend().split_for_csr(bad)
    with pytest.raises(ValueError):
        _bend().split_for_csr(2, num_bins=1)


def test_with_csr_kicks_structure():
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    inner = ca.Segment([ca.Dipole(t(0.3), angle=t(-0.05), name="b3"), ca.Drift(t(0.2), name="d3")], name="inner")
    seg = ca.Segment([ca.Drift(t(1.0), name="d1"), _bend(name="b1"), ca.Quadrupole(t(0.1), k1=t(2.0), name="q1"),
                      _bend("RBend", name="b2"), ca.Dipole(t(0.4), angle=t(0.0), name="straight"), inner,
                      _bend(name="keep")], name="lat")
    out = seg.with_csr_kicks(3, num_bins=77, except_for=["keep"])
    assert type(out) is ca.Segment and out.name == "lat"
    names = [e.name for e in out.elements]
    expect = ["d1"] + [f"b1_csr{s}_{i}" for i in range(3) for s in ("", "_kick")] + ["q1"] + \
             [f"b2_csr{s}_{i}" for i in range(3) for s in ("", "_kick")] + ["straight", "inner", "keep"]
    assert names == expect
    assert out.elements[0] is seg.elements[0] and out.elements[-1] is seg.elements[-1]
    assert all(k.num_bins == 77 for k in out.elements if isinstance(k, ca.CSRKick))
    assert [e.name for e in out.elements[-2].elements] == ["b3_csr_0", "b3_csr_kick_0", "b3_csr_1", "b3_csr_kick_1", "b3_csr_2",
                                                          "b3_csr_kick_2", "d3"]
    assert torch.allclose(out.length, seg.length)
    with pytest.raises(ValueError):
        seg.with_csr_kicks(0)


def test_tracking_errors_before_any_device_work():
    import cheetah_amd as ca

    k = _kick()
    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    with pytest.raises(RuntimeError, match="GPU only"):
        k.track(beam)
    with pytest.raises(TypeError):
        k.track(ca.ParameterBeam.from_parameters())
    with ca.sharding.particle_sharded():
        with pytest.raises(NotImplementedError, match="particle-sharded"):
            k.track(beam)
