"""The IBSKick element without a GPU: Bane's g(alpha) from the arithmetic-geometric mean against the quadrature of his integral, the
strength K against a hand-computed case, exports and C-ABI symbols, the workspace query and rejected arguments, constructor errors,
element basics, LatticeJSON, the structure, names and stream numbering of Segment.with_ibs_kicks, and the errors of tracking a beam
that cannot be tracked here (before any device work)."""
import copy
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

NEW_SYMBOLS = ("chx_ibs_workspace_bytes", "chx_ibs_kick", "chx_ibs_kick_bwd", "chx_ibs_normals")
F64 = torch.float64
R_E = 2.8179403205e-15          # m
E_CHARGE = 1.602176634e-19      # C
C_LIGHT = 299792458.0           # m / s


def _quadrature_g(alpha: float) -> float:
    """Bane's g(alpha) = (2 sqrt(alpha) / pi) int_0^inf du / sqrt((1 + u^2)(alpha^2 + u^2)); with u = tan(theta) the integral is
    int_0^(pi/2) dtheta / sqrt(alpha^2 cos^2 theta + sin^2 theta): 400 Gauss-Legendre nodes."""
    x, w = np.polynomial.legendre.leggauss(400)
    theta, w = (x + 1.0) * (math.pi / 4), w * (math.pi / 4)
    return 2.0 * math.sqrt(alpha) / math.pi * float(np.sum(w / np.sqrt(alpha**2 * np.cos(theta) ** 2 + np.sin(theta) ** 2)))


def test_g_against_the_quadrature_of_banes_integral():
    import cheetah_amd as ca

    g = lambda a: float(ca._ops.ibs_g(torch.tensor(a, dtype=F64)))  # noqa: E731
    for alpha in (1e-3, 0.01, 0.1, 0.5, 1.0, 2.0, 10.0, 1e3):
        dev = abs(g(alpha) - _quadrature_g(alpha))
        print(f"g({alpha}) = {g(alpha):.15f}, against the quadrature {dev:.2e}")
        assert dev <= 1e-10, alpha
        assert abs(g(alpha) - g(1.0 / alpha)) <= 4 * 2.0 ** -52, alpha       # symmetric: the AGM of (1, a) is a times that of (1, 1/a)
    assert g(1.0) == 1.0
    # vectorised, and differentiable
    a = torch.tensor([0.5, 2.0], dtype=F64, requires_grad=True)
    out = ca._ops.ibs_g(a)
    assert out.shape == (2,) and abs(float((out[0] - out[1]).detach())) <= 4 * 2.0 ** -52
    out.sum().backward()
    assert torch.isfinite(a.grad).all() and float(a.grad[0]) > 0 > float(a.grad[1])


def test_strength_against_the_closed_form_at_a_hand_computed_case():
    """Electrons, gamma = 500, eps = 1 nm and sigma = 100 um in both planes, Lambda = 10, L = 100 m, 1 kA: the line density is
    n = I / (e c) = 2.08e13 / m and V = K e n = sqrt(pi) r_e^2 Lambda L n / (4 gamma^3 sqrt(eps^2 sigma^2)) = 5.9e-9 (g(1) = 1)."""
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=F64)  # noqa: E731
    mass = ca.Species("electron", dtype=F64).mass_eV_float
    n = 1e3 / (E_CHARGE * C_LIGHT)
    assert abs(n / 2.08e13 - 1) < 2e-3
    V = math.sqrt(math.pi) * R_E**2 * 10.0 * 100.0 * n / (4 * 500.0**3 * 1e-9 * 1e-4)
    assert abs(V / 5.9e-9 - 1) < 1e-2
    args = (t(500.0 * mass), mass, 1.0, t(100.0), t(10.0), t(1e-4), t(1e-4), t(1e-9), t(1e-9))
    K = ca._ops.ibs_strength(*args, t(1.0))                                   # h = 1: K itself
    # r_c of the library is r_e m_e / m with its own m_e: the species' mass agrees with it to 1e-9
    assert abs(float(K) * E_CHARGE * n / V - 1) < 1e-8
    # K / h; a row without a grid has the factor 0; an invalid moment gives NaN; L = 0 gives 0
    Kh = ca._ops.ibs_strength(*args, t([2.0, 0.0, 0.5]))
    assert Kh.shape == (3,) and float(Kh[1]) == 0.0 and abs(float(Kh[0]) * 2 / float(K) - 1) < 1e-15 \
        and abs(float(Kh[2]) / 2 / float(K) - 1) < 1e-15
    for i in (4, 5, 6, 7, 8):
        for bad in (0.0, -1e-4, float("nan"), float("inf")):
            a = list(args)
            a[i] = t(bad)
            assert torch.isnan(ca._ops.ibs_strength(*a, t(1.0))), (i, bad)
    a = list(args)
    a[3] = t(0.0)
    assert float(ca._ops.ibs_strength(*a, t(1.0))) == 0.0
    # the scalings: gamma^-3, Z^4 / |Z| at a fixed mass, the aspect ratio through g
    a = list(args)
    a[0] = t(1000.0 * mass)
    assert abs(float(ca._ops.ibs_strength(*a, t(1.0))) * 8 / float(K) - 1) < 1e-14
    a = list(args)
    a[2] = 2.0
    assert abs(float(ca._ops.ibs_strength(*a, t(1.0))) / 8 / float(K) - 1) < 1e-14
    a = list(args)
    a[5], a[7] = t(4e-4), t(1e-9)                                             # sigma_x x 4 at equal emittances: alpha = 4
    assert abs(float(ca._ops.ibs_strength(*a, t(1.0))) / (float(K) * _quadrature_g(4.0) / 2) - 1) < 1e-10


def test_exported_from_the_package_and_the_accelerator_module():
    import cheetah_amd as ca
    import cheetah_amd.accelerator as acc

    assert ca.IBSKick is acc.IBSKick
    assert issubclass(ca.IBSKick, ca.Element)
    for name in ("ibs_kick", "ibs_strength", "ibs_g", "ibs_normals"):
        assert callable(getattr(ca._ops, name)), name
    assert ca._ops.IBS_MAX_BINS == 4096
    assert callable(ca.Segment.with_ibs_kicks)


def test_ibs_symbols_exported_bound_and_declared():
    import cheetah_amd._lib as L

    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (chx_[a-z0-9_]+)", out))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "chx.h")).read()
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
        assert re.search(rf"\b{name}\s*\(", header), name
    assert "#define CHX_IBS_STATE_DOUBLES(M) (CHX_WAKE_STATE_HEADER + 2 * (int64_t)(M))" in header


def test_workspace_and_invalid_arguments_on_the_host():
    import cheetah_amd._lib as L

    lib = L.lib()
    assert lib.chx_ibs_workspace_bytes(1, 10**6, 200) > 0
    assert lib.chx_ibs_workspace_bytes(1, 10**6, 4096) > lib.chx_ibs_workspace_bytes(1, 10**6, 200)
    for B, N, M in ((0, 10, 200), (1, 0, 200), (1, 10, 1), (1, 10, 4097)):
        assert lib.chx_ibs_workspace_bytes(B, N, M) == 0
    x = torch.zeros(10, 7, dtype=F64)
    v = torch.ones(10, dtype=F64)
    e = torch.ones(1, dtype=F64)
    call = torch.zeros(1, dtype=torch.int64)
    state = torch.zeros(8 + 2 * 16, dtype=F64)
    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    good = dict(mass=511e3, B=1, N=10, M=16, out=x.data_ptr(), call=call.data_ptr(), sx=e.data_ptr(), Bsx=1, ws=ws.data_ptr())

    def fwd(**kw):
        a = {**good, **kw}
        return lib.chx_ibs_kick(x.data_ptr(), v.data_ptr(), v.data_ptr(), e.data_ptr(), e.data_ptr(), e.data_ptr(), a["sx"], e.data_ptr(),
                                e.data_ptr(), e.data_ptr(), a["mass"], 1.0, 0, 0, a["call"], a["B"], 1, 1, 1, 1, 1, 1, a["Bsx"], 1, 1, 1,
                                a["N"], a["M"], 1, a["out"], state.data_ptr(), a["ws"], ws.numel(), None)

    def bwd(**kw):
        a = {"dx": x.data_ptr(), "ds": e.data_ptr(), **good, **kw}
        return lib.chx_ibs_kick_bwd(x.data_ptr(), v.data_ptr(), v.data_ptr(), 0, 0, a["call"], a["B"], 1, 1, 1, a["N"], a["M"], 1,
                                    state.data_ptr(), x.data_ptr(), a["dx"], None, a["ds"], a["ws"], ws.numel(), None)

    # rejected before any device work
    for bad in ({"N": 0}, {"B": 0}, {"B": 65536}, {"M": 1}, {"M": 4097}, {"mass": 0.0}, {"mass": -1.0}, {"out": None}, {"call": None},
                {"sx": None}, {"Bsx": 2}):
        assert fwd(**bad) == -1, bad
    assert fwd(ws=None) < 0
    for bad in ({"N": 0}, {"B": 0}, {"M": 1}, {"dx": None}, {"ds": None}, {"call": None}):
        assert bwd(**bad) == -1, bad
    assert bwd(ws=None) < 0
    words = torch.zeros(10, 4, dtype=torch.int32)
    xi = torch.zeros(10, dtype=F64)
    assert lib.chx_ibs_normals(0, 0, 0, 1, 0, words.data_ptr(), xi.data_ptr(), None) == -1
    assert lib.chx_ibs_normals(0, 0, 0, 0, 10, words.data_ptr(), xi.data_ptr(), None) == -1
    assert lib.chx_ibs_normals(0, 0, 0, 65536, 10, words.data_ptr(), xi.data_ptr(), None) == -1
    assert lib.chx_ibs_normals(0, 0, 0, 1, 10, None, xi.data_ptr(), None) == -1
    assert lib.chx_ibs_normals(0, 0, 0, 1, 10, words.data_ptr(), None, None) == -1


def _kick(**kw):
    import cheetah_amd as ca

    args = {"effect_length": torch.tensor(2.0)}
    args.update(kw)
    return ca.IBSKick(**args)


@pytest.mark.parametrize("kw", [
    {"effect_length": torch.tensor(-0.1)},
    {"effect_length": torch.tensor([0.1, -1e-3])},
    {"effect_length": torch.tensor(float("nan"))},
    {"effect_length": torch.tensor(float("inf"))},
    {"coulomb_log": 0.0}, {"coulomb_log": -1.0}, {"coulomb_log": float("nan")}, {"coulomb_log": torch.tensor([10.0, float("inf")])},
    {"coulomb_log": None},
    {"sigma_x": 0.0}, {"sigma_y": -1e-4}, {"emittance_x": float("nan")}, {"emittance_y": torch.tensor([1e-9, 0.0])},
    {"sigma_x": float("inf")},
    {"num_bins": 1}, {"num_bins": 4097}, {"num_bins": 200.0}, {"num_bins": True},
    {"seed": -1}, {"seed": 2**32}, {"seed": 1.0}, {"seed": True},
    {"stream": -1}, {"stream": 2**32}, {"stream": 2.5}, {"stream": False},
])
def test_constructor_value_errors(kw):
    with pytest.raises(ValueError, match="IBSKick"):
        _kick(**kw)


def test_element_basics():
    import cheetah_amd as ca

    k = _kick(seed=7, stream=3, sigma_x=1e-4, emittance_y=torch.tensor(2e-9), name="ibs1")
    assert isinstance(k, ca.accelerator._binned_kick.BinnedKick)
    assert not k.is_skippable
    assert float(k.length) == 0.0
    assert k.split(torch.tensor(0.1)) == [k]
    assert k.defining_features == ["name", "effect_length", "coulomb_log", "sigma_x", "sigma_y", "emittance_x", "emittance_y", "num_bins",
                                   "seed", "stream"]
    assert k.defining_tensors == ["effect_length", "coulomb_log", "sigma_x", "emittance_y"]
    assert ca.IBSKick._plain_features == ("seed", "stream")
    assert k.sigma_y is None and k.emittance_x is None and float(k.coulomb_log) == 10.0 and k.num_bins == 200
    r = repr(k)
    assert r.startswith("IBSKick(name='ibs1', effect_length=tensor(2.)") and "seed=7" in r and "stream=3" in r and "sigma_y=None" in r
    assert k.call_index == 0
    k.reseed(call_index=5)
    c = k.clone()
    assert type(c) is type(k) and c.name == "ibs1" and (c.seed, c.stream, c.num_bins) == (7, 3, 200)
    assert c.call_index == 5 and c._call_index is not k._call_index
    d = copy.deepcopy(k)
    assert d.call_index == 5 and d._call_index is not k._call_index and d.seed == 7
    for f in ("effect_length", "coulomb_log", "sigma_x", "emittance_y"):
        assert torch.equal(getattr(c, f), getattr(k, f)) and getattr(c, f) is not getattr(k, f)
    k.reseed(seed=2**32 - 1)
    assert k.call_index == 0 and k.seed == 2**32 - 1 and c.call_index == 5 and c.seed == 7
    for bad in ({"seed": -1}, {"seed": 1.5}, {"call_index": -1}, {"call_index": 2**63}):
        with pytest.raises(ValueError):
            k.reseed(**bad)
    with pytest.raises(NotImplementedError):
        k.first_order_transfer_map(torch.tensor(1e8), ca.Species("electron"))
    # batched settings and float arguments
    b = ca.IBSKick([0.1, 0.2, 0.0], coulomb_log=torch.tensor([[8.0], [12.0]], dtype=F64), dtype=F64)
    assert b.effect_length.shape == (3,) and b.effect_length.dtype == F64 and b.coulomb_log.shape == (2, 1)
    p = ca.IBSKick(torch.nn.Parameter(torch.tensor(0.3)), sigma_x=torch.nn.Parameter(torch.tensor(1e-4)))
    assert {n for n, _ in p.named_parameters()} == {"effect_length", "sigma_x"}
    # the call index is not part of a saved state
    assert "_call_index" not in k.state_dict()


def test_lattice_json_round_trip(tmp_path):
    import json

    import cheetah_amd as ca

    k = _kick(effect_length=torch.tensor(0.25), coulomb_log=8.5, sigma_x=torch.tensor(1.5e-4), emittance_x=torch.tensor(2e-9),
              num_bins=65, seed=2**32 - 1, stream=17, name="ibsk")
    k.reseed(call_index=9)
    seg = ca.Segment([ca.Drift(torch.tensor(1.0), name="d1"), k, ca.Drift(torch.tensor(0.5), name="d2")], name="lat")
    path = tmp_path / "lattice.json"
    ca.latticejson.save_cheetah_model(seg, str(path))
    stored = json.loads(path.read_text())["elements"]["ibsk"]
    assert stored[0] == "IBSKick"
    assert (stored[1]["seed"], stored[1]["stream"], stored[1]["num_bins"]) == (2**32 - 1, 17, 65)
    assert stored[1]["sigma_y"] is None and stored[1]["emittance_y"] is None
    back = ca.latticejson.load_cheetah_model(str(path))
    k2 = back.elements[1]
    assert type(k2) is ca.IBSKick and k2.name == "ibsk"
    assert (k2.seed, k2.stream, k2.num_bins) == (2**32 - 1, 17, 65)
    for f in ("effect_length", "coulomb_log", "sigma_x", "emittance_x"):
        assert torch.allclose(getattr(k2, f), getattr(k, f)), f
    assert k2.sigma_y is None and k2.emittance_y is None
    assert k2.call_index == 0


def test_with_ibs_kicks_structure():
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=F64)  # noqa: E731
    inner = ca.Segment([ca.Drift(t(0.3), name="d3"), ca.Marker(name="m3"), ca.Quadrupole(t(0.2), k1=t(1.0), name="q3")], name="inner")
    old = ca.IBSKick(t(0.7), stream=99, name="old")
    seg = ca.Segment([ca.Drift(t(1.0), name="d1"), ca.Quadrupole(t(0.2), k1=t(2.0), name="q1"), ca.Drift(t(0.0), name="d0"), inner,
                      ca.Drift(t(0.4), name="keep"), old, ca.LSCKick(t(0.4), name="lsc"), ca.Drift(t([0.0, 0.5]), name="d2")], name="lat")
    out = seg.with_ibs_kicks(coulomb_log=8.0, num_bins=65, seed=5, except_for=["keep"])
    assert type(out) is ca.Segment and out.name == "lat"
    assert [e.name for e in out.elements] == ["d1", "d1_ibs_kick", "q1", "q1_ibs_kick", "d0", "inner", "keep", "old", "lsc", "d2",
                                              "d2_ibs_kick"]
    nested = out.elements[5]
    assert type(nested) is ca.Segment and [e.name for e in nested.elements] == ["d3", "d3_ibs_kick", "m3", "q3", "q3_ibs_kick"]
    assert out.elements[0] is seg.elements[0] and out.elements[6] is seg.elements[4] and out.elements[7] is old
    flat = out.elements[:5] + nested.elements + out.elements[6:]
    kicks = [e for e in flat if isinstance(e, ca.IBSKick) and e is not old]
    # streams count in lattice order through the nested Segment: no two kicks share one
    assert [k.stream for k in kicks] == list(range(5)) and all(k.seed == 5 and k.num_bins == 65 for k in kicks)
    assert all(float(k.coulomb_log) == 8.0 and k.coulomb_log.dtype == F64 for k in kicks)
    assert all(k.sigma_x is None and k.sigma_y is None and k.emittance_x is None and k.emittance_y is None for k in kicks)
    # the effect length IS the element's length tensor
    assert kicks[0].effect_length is seg.elements[0].length and kicks[4].effect_length is seg.elements[7].length
    assert torch.allclose(out.length, seg.length)
    # max_step splits, every piece gets its kick, the streams go on from first_stream
    split = ca.Segment([ca.Drift(t(1.0), name="d1"), ca.Quadrupole(t(0.2), k1=t(2.0), name="q1")], name="s")
    split = split.with_ibs_kicks(max_step=0.4, first_stream=10)
    assert [e.name for e in split.elements] == ["d1_split_0", "d1_split_0_ibs_kick", "d1_split_1", "d1_split_1_ibs_kick", "d1_split_2",
                                                "d1_split_2_ibs_kick", "q1", "q1_ibs_kick"]
    assert [e.stream for e in split.elements[1::2]] == [10, 11, 12, 13] and all(e.seed == 0 for e in split.elements[1::2])
    assert all(k.effect_length is p.length for p, k in zip(split.elements[0::2], split.elements[1::2]))
    assert abs(float(sum(k.effect_length for k in split.elements[1::2])) - 1.2) < 1e-15
    # applied twice: the kicks that are there get none; the other collective kicks' methods give an IBS kick none either
    twice = split.with_ibs_kicks()
    assert sum(isinstance(e, ca.IBSKick) for e in twice.elements) == 8 and not any(e.name.endswith("ibs_kick_ibs_kick") for e in twice.elements)
    assert not any(e.name.endswith("ibs_kick_lsc_kick") for e in split.with_lsc_kicks().elements)
    for bad in ({"num_bins": 1}, {"num_bins": 2.0}, {"seed": -1}, {"seed": 2**32}, {"first_stream": -1}, {"first_stream": 2**32},
                {"coulomb_log": 0.0}, {"coulomb_log": None}, {"max_step": 0.0}, {"max_step": float("inf")}):
        with pytest.raises(ValueError, match="with_ibs_kicks|IBSKick"):
            seg.with_ibs_kicks(**bad)


def test_tracking_errors_before_any_device_work():
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    for k in (_kick(), _kick(sigma_x=1e-4, sigma_y=1e-4, emittance_x=1e-9, emittance_y=1e-9)):
        with pytest.raises(RuntimeError, match="GPU only"):
            k.track(beam)
        with pytest.raises(TypeError, match="needs a ParticleBeam: the intrabeam-scattering kick follows the beam's current profile"):
            k.track(ca.ParameterBeam.from_parameters())
        with ca.sharding.particle_sharded():
            with pytest.raises(NotImplementedError, match="particle-sharded"):
                k.track(beam)
        assert k.call_index == 0
