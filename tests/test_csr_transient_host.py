"""The TransientCSRKick element without a GPU: exports and C-ABI symbols, workspace queries and rejected arguments, constructor
errors, element basics, LatticeJSON, the structure of Dipole.split_for_csr and Segment.with_csr_kicks with `transient=True`, and the
errors of tracking a beam that cannot be tracked here (before any device work)."""
import os
import re
import subprocess

import pytest
import torch

from cheetah_amd import TransientCSRKick

NEW_SYMBOLS = ("chx_csr_transient_workspace_bytes", "chx_csr_transient_kick", "chx_csr_transient_kick_bwd")


def test_exported_from_the_package_and_the_accelerator_module():
    import cheetah_amd as ca
    import cheetah_amd.accelerator as acc

    assert ca.TransientCSRKick is acc.TransientCSRKick is TransientCSRKick
    assert issubclass(TransientCSRKick, ca.Element) and not issubclass(TransientCSRKick, ca.CSRKick)
    assert callable(ca._ops.csr_transient_kick) and callable(ca._ops.csr_transient_x)


def test_symbols_in_the_header_exported_and_bound():
    import cheetah_amd._lib as L

    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (chx_[a-z0-9_]+)", out))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "chx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in exported, name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert "CHX_CSR_TRANSIENT_STATE_DOUBLES" in header
    assert lib.chx_abi_version() == 9


def test_workspace_and_invalid_arguments_on_the_host():
    import cheetah_amd._lib as L

    lib = L.lib()
    ws = lib.chx_csr_transient_workspace_bytes
    assert ws(1, 10**6, 500) > 0
    assert ws(4, 10**6, 4096) > ws(1, 10**6, 4096)
    assert ws(1, 10**6, 500) > lib.chx_csr_workspace_bytes(1, 10**6, 500)      # the partials of d(x)
    assert ws(1, 10**6, 1) == 0
    assert ws(1, 10**6, 4097) == 0
    assert ws(0, 10**6, 200) == 0
    assert ws(1, 0, 200) == 0
    # rejected before any device work: no particles, M out of range, a non-positive mass, a distance of neither 1 nor B rows
    assert lib.chx_csr_transient_kick(None, None, None, None, None, None, None, 511e3, 1.0, 1, 1, 1, 1, 1, 1, 1, 1, 10, 8, 0, None,
                                      None, None, 0, None) == -1
    assert lib.chx_csr_transient_kick_bwd(None, None, None, 1, 1, 1, 1, 10, 8, 0, None, None, None, None, None, None, None, 0,
                                          None) == -1
    x = torch.zeros(10, 7, dtype=torch.float64)
    q = w = torch.ones(10, dtype=torch.float64)
    e = torch.ones(1, dtype=torch.float64)
    p = [t.data_ptr() for t in (x, q, w, e, e, e, e)]
    state = torch.zeros(64, dtype=torch.float64)
    for M, mass, Bd in ((1, 511e3, 1), (4097, 511e3, 1), (8, 0.0, 1), (8, -1.0, 1), (8, 511e3, 2), (8, 511e3, 0)):
        assert lib.chx_csr_transient_kick(*p, mass, 1.0, 1, 1, 1, 1, 1, 1, 1, Bd, 10, M, 1, x.data_ptr(), state.data_ptr(), None, 0,
                                          None) == -1
    # a missing distance pointer, and a missing d_x in the backward call
    p[6] = None
    assert lib.chx_csr_transient_kick(*p, 511e3, 1.0, 1, 1, 1, 1, 1, 1, 1, 1, 10, 8, 1, x.data_ptr(), state.data_ptr(), None, 0,
                                      None) == -1
    a = x.data_ptr()
    assert lib.chx_csr_transient_kick_bwd(a, a, a, 1, 1, 1, 1, 10, 8, 1, state.data_ptr(), a, a, None, state.data_ptr(), None, None, 0,
                                          None) == -1


def _kick(**kw):
    args = {"effect_length": torch.tensor(0.1), "angle": torch.tensor(0.02), "entrance_distance": torch.tensor(0.05)}
    args.update(kw)
    return TransientCSRKick(**args)


@pytest.mark.parametrize("kw", [
    {"entrance_distance": torch.tensor(-0.01)},
    {"entrance_distance": torch.tensor([0.1, -1e-3])},
    {"entrance_distance": torch.tensor(float("nan"))},
    {"entrance_distance": torch.tensor(float("inf"))},
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
    assert k.defining_features == ["name", "effect_length", "angle", "entrance_distance", "num_bins"]
    assert k.defining_tensors == ["effect_length", "angle", "entrance_distance"]
    r = repr(k)
    assert r.startswith("TransientCSRKick(name='csr1', effect_length=tensor(0.1000)") and "num_bins=37" in r
    assert "entrance_distance=tensor(0.0500)" in r
    c = k.clone()
    assert type(c) is type(k) and c.name == "csr1" and c.num_bins == 37
    for f in ("effect_length", "angle", "entrance_distance"):
        assert torch.equal(getattr(c, f), getattr(k, f)) and getattr(c, f) is not getattr(k, f)
    d = _kick()
    assert d.num_bins == 200
    assert float(_kick(entrance_distance=0.0).entrance_distance) == 0.0          # d = 0 is allowed: no kick
    with pytest.raises(NotImplementedError):
        d.first_order_transfer_map(torch.tensor(1e8), ca.Species("electron"))
    # batched settings and float arguments
    b = TransientCSRKick([0.1, 0.2, 0.0], torch.tensor([[0.01], [-0.02]], dtype=torch.float64), [0.05, 0.1, 0.0],
                         dtype=torch.float64)
    assert b.effect_length.shape == (3,) and b.angle.shape == (2, 1)
    assert b.entrance_distance.shape == (3,) and b.entrance_distance.dtype == torch.float64
    p = TransientCSRKick(*(torch.nn.Parameter(torch.tensor(v)) for v in (0.3, 0.01, 0.1)))
    assert {n for n, _ in p.named_parameters()} == {"effect_length", "angle", "entrance_distance"}
    doc = TransientCSRKick.__doc__
    for limit in ("ultra-relativistic", "1-D", "long straight", "exit transient"):
        assert limit in doc, limit
    assert "TransientCSRKick" in ca.CSRKick.__doc__ and "no entrance" not in ca.CSRKick.__doc__


def test_lattice_json_round_trip(tmp_path):
    import cheetah_amd as ca

    k = _kick(effect_length=torch.tensor(0.25), angle=torch.tensor(-0.03), entrance_distance=torch.tensor(0.125), num_bins=123,
              name="csrk")
    seg = ca.Segment([ca.Drift(torch.tensor(1.0), name="d1"), k, ca.Drift(torch.tensor(0.5), name="d2")], name="lat")
    path = tmp_path / "lattice.json"
    ca.latticejson.save_cheetah_model(seg, str(path))
    back = ca.latticejson.load_cheetah_model(str(path))
    k2 = back.elements[1]
    assert type(k2) is TransientCSRKick and k2.name == "csrk" and k2.num_bins == 123
    for f in ("effect_length", "angle", "entrance_distance"):
        assert torch.allclose(getattr(k2, f), getattr(k, f)), f


def _bend(cls="Dipole", **kw):
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    common = {"k1": t(0.7), "tilt": t(0.1), "gap": t(0.02), "gap_exit": t(0.03), "fringe_integral": t(0.5),
              "fringe_integral_exit": t(0.4), "fringe_at": "both", "fringe_type": "linear_edge", "name": "b"}
    common.update(kw)
    if cls == "RBend":
        return ca.RBend(t(0.6), angle=t(0.12), rbend_e1=t(0.01), rbend_e2=t(-0.02), **common)
    return ca.Dipole(t(0.6), angle=t(0.12), dipole_e1=t(0.05), dipole_e2=t(0.07), **common)


@pytest.mark.parametrize("cls", ["Dipole", "RBend"])
@pytest.mark.parametrize("n", [1, 3])
def test_split_for_csr_transient_structure(cls, n):
    import cheetah_amd as ca

    bend = _bend(cls, tracking_method="drift_kick_drift")
    parts = bend.split_for_csr(n, num_bins=300, transient=True)
    steady = bend.split_for_csr(n, num_bins=300)
    assert len(parts) == len(steady) == 2 * n
    dips, kicks = parts[0::2], parts[1::2]
    assert all(type(d) is ca.Dipole for d in dips) and all(type(k) is TransientCSRKick for k in kicks)
    assert all(type(k) is ca.CSRKick for k in steady[1::2])                 # the default is today's
    assert all(type(k) is ca.CSRKick for k in bend.split_for_csr(n, 300, False)[1::2])
    for i, (d, k, d0, k0) in enumerate(zip(dips, kicks, steady[0::2], steady[1::2])):
        assert d.name == d0.name == f"b_csr_{i}" and k.name == k0.name == f"b_csr_kick_{i}"
        assert torch.equal(k.effect_length, k0.effect_length) and torch.equal(k.angle, k0.angle)
        assert torch.allclose(k.effect_length, bend.length / n) and torch.allclose(k.angle, bend.angle / n)
        assert abs(float(k.entrance_distance) - (i + 0.5) * 0.6 / n) < 1e-15
        assert k.entrance_distance.dtype == torch.float64 and k.num_bins == 300
        # the bend's pieces, fringe handling included, are those of the default split
        for f in d0.defining_features:
            a, b = getattr(d, f), getattr(d0, f)
            assert torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b, f
        assert d.tracking_method == "drift_kick_drift"
        first, last = i == 0, i == n - 1
        assert d.fringe_at == ("both" if first and last else "entrance" if first else "exit" if last else "neither")


def test_split_for_csr_transient_leaves_straight_bends_and_rejects_bad_arguments():
    import cheetah_amd as ca

    straight = ca.Dipole(torch.tensor(0.5), angle=torch.tensor(0.0))
    assert straight.split_for_csr(4, transient=True) == [straight]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            _bend().split_for_csr(bad, transient=True)
    with pytest.raises(ValueError):
        _bend().split_for_csr(2, num_bins=1, transient=True)


def test_with_csr_kicks_transient_structure():
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    inner = ca.Segment([ca.Dipole(t(0.3), angle=t(-0.05), name="b3"), ca.Drift(t(0.2), name="d3")], name="inner")
    seg = ca.Segment([ca.Drift(t(1.0), name="d1"), _bend(name="b1"), ca.Quadrupole(t(0.1), k1=t(2.0), name="q1"),
                      _bend("RBend", name="b2"), ca.Dipole(t(0.4), angle=t(0.0), name="straight"), inner,
                      _bend(name="keep")], name="lat")
    out = seg.with_csr_kicks(3, num_bins=77, except_for=["keep"], transient=True)
    assert type(out) is ca.Segment and out.name == "lat"
    names = [e.name for e in out.elements]
    expect = ["d1"] + [f"b1_csr{s}_{i}" for i in range(3) for s in ("", "_kick")] + ["q1"] + \
             [f"b2_csr{s}_{i}" for i in range(3) for s in ("", "_kick")] + ["straight", "inner", "keep"]
    assert names == expect
    assert out.elements[0] is seg.elements[0] and out.elements[-1] is seg.elements[-1]
    kicks = [k for k in out.elements if isinstance(k, TransientCSRKick)]
    assert len(kicks) == 6 and all(k.num_bins == 77 for k in kicks)
    assert not any(isinstance(k, ca.CSRKick) for k in out.elements)
    assert [round(float(k.entrance_distance), 12) for k in kicks] == [0.1, 0.3, 0.5] * 2       # every bend from its own entrance
    nested = out.elements[-2].elements
    assert [e.name for e in nested] == ["b3_csr_0", "b3_csr_kick_0", "b3_csr_1", "b3_csr_kick_1", "b3_csr_2", "b3_csr_kick_2", "d3"]
    assert all(type(k) is TransientCSRKick for k in nested[1:6:2])
    assert [round(float(k.entrance_distance), 12) for k in nested[1:6:2]] == [0.05, 0.15, 0.25]
    assert torch.allclose(out.length, seg.length)
    # the default still yields CSRKick, and the names are the same
    default = seg.with_csr_kicks(3, num_bins=77, except_for=["keep"])
    assert [e.name for e in default.elements] == expect
    assert sum(type(k) is ca.CSRKick for k in default.elements) == 6
    assert not any(isinstance(k, TransientCSRKick) for k in default.elements)
    with pytest.raises(ValueError):
        seg.with_csr_kicks(0, transient=True)


def test_with_lsc_kicks_gives_a_transient_csr_kick_no_lsc_kick():
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    seg = ca.Segment([_bend(name="b1"), ca.Drift(t(1.0), name="d1")]).with_csr_kicks(2, transient=True).with_lsc_kicks()
    assert [e.name for e in seg.elements] == ["b1_csr_0", "b1_csr_0_lsc_kick", "b1_csr_kick_0", "b1_csr_1", "b1_csr_1_lsc_kick",
                                              "b1_csr_kick_1", "d1", "d1_lsc_kick"]


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
