"""The SynchrotronRadiationKick element without a GPU: exports and C-ABI symbols, the workspace query and rejected arguments,
constructor errors, element basics, LatticeJSON, the structure, names and stream numbering of Dipole.split_for_radiation and
Segment.with_radiation_kicks, and the errors of tracking a beam that cannot be tracked here (before any device work). The integer
Philox4x32-10 that the GPU tests compare the kernel's words with is defined here and pinned to the published known answers."""
import copy
import re
import subprocess

import pytest
import torch

NEW_SYMBOLS = ("chx_sr_workspace_bytes", "chx_sr_kick", "chx_sr_kick_bwd", "chx_sr_normals")

M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) on Python integers: (c0, c1, c2, c3), (k0, k1) -> four 32-bit words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


@pytest.mark.parametrize("counter, key, words", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_python_philox_known_answers(counter, key, words):
    assert philox4x32_10(counter, key) == words


def test_exported_from_the_package_and_the_accelerator_module():
    import cheetah_amd as ca
    import cheetah_amd.accelerator as acc

    assert ca.SynchrotronRadiationKick is acc.SynchrotronRadiationKick
    assert issubclass(ca.SynchrotronRadiationKick, ca.Element)
    assert callable(ca._ops.sr_kick) and callable(ca._ops.sr_factors) and callable(ca._ops.sr_normals)
    assert callable(ca.Dipole.split_for_radiation) and callable(ca.Segment.with_radiation_kicks)


def test_sr_symbols_exported_and_bound():
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
    assert lib.chx_sr_workspace_bytes(1, 10**6) > 0
    assert lib.chx_sr_workspace_bytes(4, 10**6) == 4 * lib.chx_sr_workspace_bytes(1, 10**6)
    assert lib.chx_sr_workspace_bytes(1, 257) == 2 * lib.chx_sr_workspace_bytes(1, 256) == 2 * 3 * 8
    assert lib.chx_sr_workspace_bytes(0, 10**6) == 0
    assert lib.chx_sr_workspace_bytes(1, 0) == 0
    assert lib.chx_sr_workspace_bytes(65536, 10) == 0
    assert lib.chx_sr_workspace_bytes(1, 2**32) == 0
    x = torch.zeros(10, 7, dtype=torch.float64)
    e = torch.ones(1, dtype=torch.float64)
    call = torch.zeros(1, dtype=torch.int64)
    d = torch.zeros(3, dtype=torch.float64)
    ws = torch.zeros(64, dtype=torch.uint8)
    p = [t.data_ptr() for t in (x, e, e, e)]
    good = dict(mass=511e3, B=1, N=10, out=x.data_ptr(), call=call.data_ptr())

    def fwd(**kw):
        a = {**good, **kw}
        return lib.chx_sr_kick(*p, a["mass"], 1.0, 1, 0, 0, a["call"], a["B"], 1, 1, 1, 1, a["N"], 1, a["out"], None)

    def bwd(**kw):
        a = {"dx": x.data_ptr(), "dg": d.data_ptr(), **good, **kw}
        return lib.chx_sr_kick_bwd(*p, a["mass"], 1.0, 1, 0, 0, a["call"], a["B"], 1, 1, 1, 1, a["N"], 1, x.data_ptr(), a["dx"],
                                   a["dg"], d.data_ptr(), d.data_ptr(), ws.data_ptr(), 64, None)

    # rejected before any device work: no particles, no rows, a non-positive mass, null outputs, no call index
    for bad in ({"N": 0}, {"B": 0}, {"mass": 0.0}, {"mass": -1.0}, {"out": None}, {"call": None}):
        assert fwd(**bad) == -1, bad
    for bad in ({"N": 0}, {"B": 0}, {"mass": 0.0}, {"dx": None}, {"dg": None}, {"call": None}):
        assert bwd(**bad) == -1, bad
    assert lib.chx_sr_kick(None, None, None, None, 511e3, 1.0, 1, 0, 0, None, 1, 1, 1, 1, 1, 10, 0, None, None) == -1
    words = torch.zeros(10, 4, dtype=torch.int32)
    xi = torch.zeros(10, dtype=torch.float64)
    assert lib.chx_sr_normals(0, 0, 0, 1, 0, words.data_ptr(), xi.data_ptr(), None) == -1
    assert lib.chx_sr_normals(0, 0, 0, 0, 10, words.data_ptr(), xi.data_ptr(), None) == -1
    assert lib.chx_sr_normals(0, 0, 0, 1, 10, None, xi.data_ptr(), None) == -1
    assert lib.chx_sr_normals(0, 0, 0, 1, 10, words.data_ptr(), None, None) == -1


def _kick(**kw):
    import cheetah_amd as ca

    args = {"effect_length": torch.tensor(0.5), "angle": torch.tensor(0.05)}
    args.update(kw)
    return ca.SynchrotronRadiationKick(**args)


@pytest.mark.parametrize("kw", [
    {"effect_length": torch.tensor(-0.1)},
    {"effect_length": torch.tensor([0.1, -1e-3])},
    {"effect_length": torch.tensor(float("nan"))},
    {"effect_length": torch.tensor(float("inf"))},
    {"angle": torch.tensor(float("nan"))},
    {"angle": torch.tensor([0.1, float("inf")])},
    {"seed": -1}, {"seed": 2**32}, {"seed": 1.0}, {"seed": True},
    {"stream": -1}, {"stream": 2**32}, {"stream": 2.5}, {"stream": False},
])
def test_constructor_value_errors(kw):
    with pytest.raises(ValueError):
        _kick(**kw)


def test_element_basics():
    import cheetah_amd as ca

    k = _kick(seed=7, stream=3, name="sr1")
    assert not k.is_skippable
    assert float(k.length) == 0.0
    assert k.split(torch.tensor(0.1)) == [k]
    assert k.defining_features == ["name", "effect_length", "angle", "quantum_excitation", "seed", "stream"]
    assert k.defining_tensors == ["effect_length", "angle"]
    r = repr(k)
    assert r.startswith("SynchrotronRadiationKick(name='sr1', effect_length=tensor(0.5000)") and "seed=7" in r and "stream=3" in r \
        and "quantum_excitation=True" in r
    assert k.call_index == 0
    k.reseed(call_index=5)
    c = k.clone()
    assert type(c) is type(k) and c.name == "sr1" and (c.seed, c.stream, c.quantum_excitation) == (7, 3, True)
    assert c.call_index == 5 and c._call_index is not k._call_index
    d = copy.deepcopy(k)
    assert d.call_index == 5 and d._call_index is not k._call_index and d.seed == 7
    for f in ("effect_length", "angle"):
        assert torch.equal(getattr(c, f), getattr(k, f)) and getattr(c, f) is not getattr(k, f)
    k.reseed(seed=2**32 - 1)
    assert k.call_index == 0 and k.seed == 2**32 - 1 and c.call_index == 5 and c.seed == 7
    for bad in ({"seed": -1}, {"seed": 1.5}, {"call_index": -1}, {"call_index": 2**63}):
        with pytest.raises(ValueError):
            k.reseed(**bad)
    q = ca.SynchrotronRadiationKick(torch.tensor(0.5), torch.tensor(-0.1), quantum_excitation=False)
    assert (q.seed, q.stream, q.quantum_excitation) == (0, 0, False)
    with pytest.raises(NotImplementedError):
        q.first_order_transfer_map(torch.tensor(1e8), ca.Species("electron"))
    # batched settings and float arguments
    b = ca.SynchrotronRadiationKick([0.1, 0.2, 0.0], torch.tensor([[0.01], [0.02]], dtype=torch.float64), dtype=torch.float64)
    assert b.effect_length.shape == (3,) and b.effect_length.dtype == torch.float64 and b.angle.shape == (2, 1)
    p = ca.SynchrotronRadiationKick(torch.nn.Parameter(torch.tensor(0.3)), torch.nn.Parameter(torch.tensor(0.02)))
    assert {n for n, _ in p.named_parameters()} == {"effect_length", "angle"}
    # the call index is not part of a saved state
    assert "_call_index" not in k.state_dict()


def test_lattice_json_round_trip(tmp_path):
    import json

    import cheetah_amd as ca

    k = _kick(effect_length=torch.tensor(0.25), angle=torch.tensor(-0.03), quantum_excitation=False, seed=2**32 - 1, stream=17,
              name="srk")
    k.reseed(call_index=9)
    seg = ca.Segment([ca.Drift(torch.tensor(1.0), name="d1"), k, ca.Drift(torch.tensor(0.5), name="d2")], name="lat")
    path = tmp_path / "lattice.json"
    ca.latticejson.save_cheetah_model(seg, str(path))
    stored = json.loads(path.read_text())["elements"]["srk"]
    assert stored[0] == "SynchrotronRadiationKick"
    assert (stored[1]["seed"], stored[1]["stream"], stored[1]["quantum_excitation"]) == (2**32 - 1, 17, False)
    back = ca.latticejson.load_cheetah_model(str(path))
    k2 = back.elements[1]
    assert type(k2) is ca.SynchrotronRadiationKick and k2.name == "srk"
    assert (k2.seed, k2.stream, k2.quantum_excitation) == (2**32 - 1, 17, False)
    assert torch.allclose(k2.effect_length, k.effect_length) and torch.allclose(k2.angle, k.angle)
    assert k2.call_index == 0


def test_split_for_radiation_structure():
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    bend = ca.Dipole(t(0.6), angle=t(0.09), k1=t(0.2), dipole_e1=t(0.01), dipole_e2=t(0.02), fringe_integral=t(0.5), gap=t(0.03),
                     name="B")
    parts = bend.split_for_radiation(3, quantum_excitation=False, seed=11, first_stream=4)
    assert [p.name for p in parts] == ["B_sr_0", "B_sr_kick_0", "B_sr_1", "B_sr_kick_1", "B_sr_2", "B_sr_kick_2"]
    pieces, kicks = parts[0::2], parts[1::2]
    assert all(type(p) is ca.Dipole for p in pieces) and all(type(k) is ca.SynchrotronRadiationKick for k in kicks)
    assert [k.stream for k in kicks] == [4, 5, 6] and all(k.seed == 11 and not k.quantum_excitation for k in kicks)
    for p, k in zip(pieces, kicks):
        assert k.effect_length is p.length and k.angle is p.angle
        assert abs(float(p.length) - 0.2) < 1e-15 and abs(float(p.angle) - 0.03) < 1e-15 and float(p.k1) == 0.2
    # face handling is split_for_csr's
    for mine, theirs in zip(pieces, bend.split_for_csr(3)[0::2]):
        assert mine.fringe_at == theirs.fringe_at
        for f in ("dipole_e1", "dipole_e2", "fringe_integral", "fringe_integral_exit", "gap", "gap_exit", "tilt"):
            assert torch.equal(getattr(mine, f), getattr(theirs, f)), f
    assert [p.fringe_at for p in pieces] == ["entrance", "neither", "exit"]
    assert float(pieces[0].dipole_e1) == 0.01 and float(pieces[1].dipole_e1) == 0.0 and float(pieces[2].dipole_e2) == 0.02
    # defaults, a zero-angle bend, an RBend, bad arguments
    assert [k.stream for k in bend.split_for_radiation(2)[1::2]] == [0, 1]
    straight = ca.Dipole(t(0.6), angle=t(0.0), name="S")
    assert straight.split_for_radiation(3) == [straight]
    rb = ca.RBend(t(0.4), angle=t(0.08), name="R").split_for_radiation(2)
    assert [type(p) for p in rb] == [ca.Dipole, ca.SynchrotronRadiationKick] * 2
    assert abs(float(rb[0].dipole_e1) - 0.04) < 1e-15 and float(rb[0].dipole_e2) == 0.0 and abs(float(rb[2].dipole_e2) - 0.04) < 1e-15
    for bad in ({"num_kicks": 0}, {"num_kicks": 1.0}, {"num_kicks": 1, "seed": -1}, {"num_kicks": 1, "first_stream": 2**32},
                {"num_kicks": 2, "first_stream": 2**32 - 1}):
        with pytest.raises(ValueError):
            bend.split_for_radiation(**bad)


def test_with_radiation_kicks_structure():
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    inner = ca.Segment([ca.Dipole(t(0.3), angle=t(0.02), name="b3"), ca.Marker(name="m3"), ca.RBend(t(0.2), angle=t(-0.01), name="r3")],
                       name="inner")
    seg = ca.Segment([ca.Drift(t(1.0), name="d1"), ca.Dipole(t(0.5), angle=t(0.05), name="b1"), ca.Dipole(t(0.5), angle=t(0.0), name="b0"),
                      inner, ca.Dipole(t(0.4), angle=t(0.04), name="keep"), ca.Dipole(t(0.5), angle=t([0.0, 0.03]), name="b2")],
                     name="lat")
    out = seg.with_radiation_kicks(num_kicks=2, seed=5, except_for=["keep"])
    assert type(out) is ca.Segment and out.name == "lat"
    assert [e.name for e in out.elements] == ["d1", "b1_sr_0", "b1_sr_kick_0", "b1_sr_1", "b1_sr_kick_1", "b0", "inner", "keep",
                                              "b2_sr_0", "b2_sr_kick_0", "b2_sr_1", "b2_sr_kick_1"]
    nested = out.elements[6]
    assert type(nested) is ca.Segment
    assert [e.name for e in nested.elements] == ["b3_sr_0", "b3_sr_kick_0", "b3_sr_1", "b3_sr_kick_1", "m3", "r3_sr_0", "r3_sr_kick_0",
                                                 "r3_sr_1", "r3_sr_kick_1"]
    assert out.elements[0] is seg.elements[0] and out.elements[5] is seg.elements[2] and out.elements[7] is seg.elements[4]
    flat = out.elements[:6] + nested.elements + out.elements[7:]
    kicks = [e for e in flat if isinstance(e, ca.SynchrotronRadiationKick)]
    # streams count in lattice order through the nested Segment: no two kicks share one
    assert [k.stream for k in kicks] == list(range(8)) and all(k.seed == 5 and k.quantum_excitation for k in kicks)
    assert torch.allclose(out.length, seg.length)
    # defaults: one kick per bend
    one = seg.with_radiation_kicks(quantum_excitation=False)
    names = [e.name for e in one.elements]
    assert names[:3] == ["d1", "b1_sr_0", "b1_sr_kick_0"] and names[-4:] == ["keep_sr_0", "keep_sr_kick_0", "b2_sr_0", "b2_sr_kick_0"]
    assert not one.elements[2].quantum_excitation and one.elements[2].seed == 0
    # behind with_csr_kicks: one radiation kick per CSR piece; and with_lsc_kicks gives the zero-length kick none
    both = ca.Segment([ca.Drift(t(1.0), name="d1"), ca.Dipole(t(0.5), angle=t(0.05), name="b1")], name="c")
    both = both.with_csr_kicks(2).with_radiation_kicks(1)
    assert [e.name for e in both.elements] == ["d1", "b1_csr_0_sr_0", "b1_csr_0_sr_kick_0", "b1_csr_kick_0", "b1_csr_1_sr_0",
                                               "b1_csr_1_sr_kick_0", "b1_csr_kick_1"]
    assert [e.stream for e in both.elements if isinstance(e, ca.SynchrotronRadiationKick)] == [0, 1]
    assert [p.fringe_at for p in both.elements[1::3]] == ["entrance", "exit"]
    lsc = both.with_lsc_kicks()
    assert not any(e.name.endswith("sr_kick_0_lsc_kick") for e in lsc.elements)
    for bad in ({"num_kicks": 0}, {"num_kicks": 2.0}, {"seed": -1}, {"seed": 2**32}):
        with pytest.raises(ValueError):
            seg.with_radiation_kicks(**bad)


def test_tracking_errors_before_any_device_work():
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    for k in (_kick(), _kick(quantum_excitation=False)):
        with pytest.raises(RuntimeError, match="GPU only"):
            k.track(beam)
        with pytest.raises(TypeError, match="needs a ParticleBeam"):
            k.track(ca.ParameterBeam.from_parameters())
        with ca.sharding.particle_sharded():
            with pytest.raises(NotImplementedError, match="particle-sharded"):
                k.track(beam)
        assert k.call_index == 0
