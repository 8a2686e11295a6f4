"""The LaserModulator element without a GPU: exports and C-ABI symbols, the workspace query and rejected arguments, constructor
errors, element basics, LatticeJSON with and without a pulse envelope, the structure, lengths and amplitudes of
`Undulator.with_laser`, the known answers of `laser_modulation_amplitude` and `Undulator.resonant_wavelength`, and the errors of
tracking a beam that cannot be tracked here (before any device work)."""
import copy
import json
import math
import re
import subprocess

import pytest
import torch

NEW_SYMBOLS = ("chx_laser_workspace_bytes", "chx_laser_kick", "chx_laser_kick_bwd")
F64 = torch.float64
SETTINGS = ["amplitude", "wavelength", "phase", "laser_sigma", "offset_x", "offset_y", "pulse_sigma", "pulse_center"]

# the known-answer case: an electron beam of 135 MeV in a planar undulator of K = 1.385, L_u = 0.5 m, lambda_u = 0.05 m, a laser of
# 1.2 MW peak power and sigma_r = 175 um
E0, K, LU, PERIOD, SIGMA_R, POWER = 135e6, 1.385, 0.5, 0.05, 175e-6, 1.2e6
M_E = 510998.95069                                       # eV
P_0 = 1.602176634e-19 * 299792458.0 / 2.8179403205e-15 * M_E     # (e c / r_e) m_e c^2 / e, W


def t(v):
    return torch.tensor(v, dtype=F64)


def test_exported_from_the_package_and_the_accelerator_module():
    import cheetah_amd as ca
    import cheetah_amd.accelerator as acc

    assert ca.LaserModulator is acc.LaserModulator
    assert issubclass(ca.LaserModulator, ca.Element)
    assert ca.laser_modulation_amplitude is acc.laser_modulation_amplitude
    assert callable(ca._ops.laser_kick) and callable(ca._ops.laser_factors)
    assert callable(ca.Undulator.with_laser) and callable(ca.Undulator.resonant_wavelength)


def test_laser_symbols_exported_and_bound():
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
    assert lib.chx_laser_workspace_bytes(1, 10**6) > 0
    assert lib.chx_laser_workspace_bytes(4, 10**6) == 4 * lib.chx_laser_workspace_bytes(1, 10**6)
    assert lib.chx_laser_workspace_bytes(1, 257) == 2 * lib.chx_laser_workspace_bytes(1, 256) == 2 * 8 * 8
    assert lib.chx_laser_workspace_bytes(0, 10**6) == 0
    assert lib.chx_laser_workspace_bytes(1, 0) == 0
    assert lib.chx_laser_workspace_bytes(65536, 10) == 0
    assert lib.chx_laser_workspace_bytes(1, 2**32) == 0
    x = torch.zeros(10, 7, dtype=F64)
    e = torch.ones(1, dtype=F64)
    d = torch.zeros(8, dtype=F64)
    ws = torch.zeros(64, dtype=torch.uint8)
    good = dict(x=x.data_ptr(), s=[e.data_ptr()] * 9, mass=511e3, B=1, Bx=1, rows=[1] * 9, N=10, dtype=1, out=x.data_ptr(),
                dx=x.data_ptr(), dr=d.data_ptr(), ws=ws.data_ptr(), ws_bytes=64)

    def fwd(**kw):
        a = {**good, **kw}
        return lib.chx_laser_kick(a["x"], *a["s"], a["mass"], a["B"], a["Bx"], *a["rows"], a["N"], a["dtype"], a["out"], None)

    def bwd(**kw):
        a = {**good, **kw}
        return lib.chx_laser_kick_bwd(a["x"], *a["s"], a["mass"], a["B"], a["Bx"], *a["rows"], a["N"], a["dtype"], x.data_ptr(),
                                      a["dx"], a["dr"], a["ws"], a["ws_bytes"], None)

    def without(i):
        s = list(good["s"])
        s[i] = None
        return s

    def rows(i, n):
        r = list(good["rows"])
        r[i] = n
        return r

    # rejected before any device work: no particles, no rows, a non-positive mass, null pointers (every setting but pulse_sigma, the
    # eighth), a setting of neither 1 nor B rows
    bad_both = [{"N": 0}, {"B": 0}, {"mass": 0.0}, {"mass": -1.0}, {"mass": float("nan")}, {"x": None}, {"Bx": 2}]
    bad_both += [{"s": without(i)} for i in range(9) if i != 7] + [{"rows": rows(i, 2)} for i in range(9)]
    for bad in bad_both + [{"out": None}]:
        assert fwd(**bad) == -1, bad
    for bad in bad_both + [{"dx": None}, {"dr": None}]:
        assert bwd(**bad) == -1, bad
    # a dtype that is not a beam's, a misaligned output, a workspace that is missing or too small: their own codes, in that order
    codes = {fwd(dtype=2), bwd(dtype=2), fwd(out=x.data_ptr() + 8), bwd(dx=x.data_ptr() + 8), bwd(ws=None), bwd(ws_bytes=63)}
    assert all(c < -1 for c in codes) and fwd(dtype=2) == bwd(dtype=2) and fwd(out=x.data_ptr() + 8) == bwd(dx=x.data_ptr() + 8)
    assert len({fwd(dtype=2), fwd(out=x.data_ptr() + 8), bwd(ws=None)}) == 3 and bwd(ws=None) == bwd(ws_bytes=63)


def _kick(**kw):
    import cheetah_amd as ca

    args = {"amplitude": t(20e3), "wavelength": t(8e-7), "laser_sigma": t(2e-4)}
    args.update(kw)
    return ca.LaserModulator(**args)


@pytest.mark.parametrize("kw", [
    {"amplitude": t(float("nan"))}, {"amplitude": t([1.0, float("inf")])},
    {"wavelength": t(0.0)}, {"wavelength": t(-8e-7)}, {"wavelength": t(float("nan"))}, {"wavelength": t([8e-7, 0.0])},
    {"laser_sigma": t(0.0)}, {"laser_sigma": t(-1e-4)}, {"laser_sigma": t(float("inf"))},
    {"phase": t(float("nan"))}, {"phase": float("inf")},
    {"offset_x": t(float("nan"))}, {"offset_y": t(float("-inf"))},
    {"pulse_sigma": t(0.0)}, {"pulse_sigma": t(-1e-3)}, {"pulse_sigma": t(float("nan"))}, {"pulse_sigma": t([1e-3, 0.0])},
    {"pulse_center": t(float("nan"))},
    {"wavelength": None}, {"laser_sigma": None}, {"phase": None},
])
def test_constructor_value_errors(kw):
    with pytest.raises(ValueError):
        _kick(**kw)


def test_element_basics():
    import cheetah_amd as ca

    k = _kick(phase=t(0.3), offset_x=t(1e-5), name="lh")
    assert not k.is_skippable
    assert float(k.length) == 0.0
    assert k.split(torch.tensor(0.1)) == [k]
    assert k.defining_features == ["name"] + SETTINGS
    assert k.defining_tensors == [s for s in SETTINGS if s != "pulse_sigma"]
    assert k.pulse_sigma is None and float(k.pulse_center) == 0.0 and float(k.offset_y) == 0.0
    r = repr(k)
    assert r.startswith("LaserModulator(name='lh', amplitude=tensor(20000.") and "pulse_sigma=None" in r
    with pytest.raises(NotImplementedError):
        k.first_order_transfer_map(torch.tensor(1e8), ca.Species("electron"))
    p = _kick(pulse_sigma=t(3e-4), pulse_center=t(-1e-4), amplitude=t(-5e3))
    for e in (k, p):
        c, d = e.clone(), copy.deepcopy(e)
        for other in (c, d):
            assert type(other) is ca.LaserModulator and other.name == e.name
            for s in SETTINGS:
                a, b = getattr(e, s), getattr(other, s)
                assert (a is None and b is None) or (torch.equal(a, b) and a is not b and a.dtype == b.dtype), s
    # batched settings, float arguments, parameters
    b = ca.LaserModulator([1e3, -2e3, 0.0], 8e-7, torch.tensor([[1e-4], [2e-4]], dtype=F64), pulse_sigma=1e-3, dtype=F64)
    assert b.amplitude.shape == (3,) and b.amplitude.dtype == F64 and b.laser_sigma.shape == (2, 1) and b.pulse_sigma.dtype == F64
    assert b.wavelength.shape == () and b.wavelength.dtype == F64
    q = ca.LaserModulator(torch.nn.Parameter(t(1e3)), t(8e-7), t(1e-4), phase=torch.nn.Parameter(t(0.1)))
    assert {n for n, _ in q.named_parameters()} == {"amplitude", "phase"}
    assert set(k.state_dict()) == {"length"} | {s for s in SETTINGS if s != "pulse_sigma"}


@pytest.mark.parametrize("pulse_sigma", [None, 2.5e-4])
def test_lattice_json_round_trip(tmp_path, pulse_sigma):
    import cheetah_amd as ca

    k = _kick(amplitude=t(-12e3), phase=t(0.7), offset_x=t(2e-5), offset_y=t(-3e-5), pulse_center=t(1e-4), name="lhk",
              pulse_sigma=None if pulse_sigma is None else t(pulse_sigma))
    seg = ca.Segment([ca.Drift(t(1.0), name="d1"), k, ca.Drift(t(0.5), name="d2")], name="lat")
    path = tmp_path / "lattice.json"
    ca.latticejson.save_cheetah_model(seg, str(path))
    stored = json.loads(path.read_text())["elements"]["lhk"]
    assert stored[0] == "LaserModulator"
    assert stored[1]["pulse_sigma"] == pulse_sigma and stored[1]["amplitude"] == -12e3 and set(SETTINGS) <= set(stored[1])
    back = ca.latticejson.load_cheetah_model(str(path), dtype=F64)
    k2 = back.elements[1]
    assert type(k2) is ca.LaserModulator and k2.name == "lhk"
    for s in SETTINGS:
        a, b = getattr(k, s), getattr(k2, s)
        assert (a is None and b is None) or (b.dtype == F64 and torch.equal(a, b)), s


def _undulator(**kw):
    import cheetah_amd as ca

    args = {"length": t(LU), "period": t(PERIOD), "ky": t(K), "name": "U", "dtype": F64}
    args.update(kw)
    return ca.Undulator(**args)


def _amplitude_restated(power, k, length, sigma_r, energy, mass=M_E, z=1.0):
    """A = mc^2 sqrt(P_L / P_0) K L_u [JJ] / (gamma0 sigma_r) in float64 with torch's Bessel functions."""
    k = t(k)
    xi = k**2 / (4 + 2 * k**2)
    jj = torch.special.bessel_j0(xi) - torch.special.bessel_j1(xi)
    p0 = P_0 * (mass / M_E) ** 2 / z**2
    return float(mass * math.sqrt(power / p0) * k * length * jj / (energy / mass * sigma_r)), float(jj)


def test_known_answers():
    import cheetah_amd as ca

    assert abs(P_0 / 8.710023e9 - 1) < 1e-6
    A = ca.laser_modulation_amplitude(t(POWER), t(K), t(LU), t(SIGMA_R), t(E0))
    ref, jj = _amplitude_restated(POWER, K, LU, SIGMA_R, E0)
    assert abs(jj / 0.8635996 - 1) < 1e-6
    assert A.dtype == F64 and A.shape == ()
    assert abs(float(A) / ref - 1) < 1e-9
    assert abs(float(A) / 77585.65 - 1) < 1e-6
    # floats, broadcasting, another species (a proton: P_0 larger by (m_p / m_e)^2, gamma0 smaller, mc^2 larger)
    assert abs(float(ca.laser_modulation_amplitude(POWER, K, LU, SIGMA_R, E0).double()) / ref - 1) < 1e-5
    B = ca.laser_modulation_amplitude(t([POWER, 4 * POWER]), t(K), t([[LU], [LU / 3]]), t(SIGMA_R), t(E0))
    assert B.shape == (2, 2)
    assert torch.allclose(B, t([[ref, 2 * ref], [ref / 3, 2 * ref / 3]]), rtol=1e-12)
    proton = ca.Species("proton", dtype=F64)
    ref_p, _ = _amplitude_restated(POWER, K, LU, SIGMA_R, 2e9, mass=float(proton.mass_eV))
    assert abs(float(ca.laser_modulation_amplitude(t(POWER), t(K), t(LU), t(SIGMA_R), t(2e9), species=proton)) / ref_p - 1) < 1e-9
    # differentiable: dA/dP = A / 2P, dA/dE = -A / E, dA/dsigma = -A / sigma, dA/dL = A / L, dA/dK against a central difference
    leaves = [t(v).requires_grad_() for v in (POWER, K, LU, SIGMA_R, E0)]
    A = ca.laser_modulation_amplitude(*leaves)
    gP, gK, gL, gS, gE = torch.autograd.grad(A, leaves)
    a = float(A.detach())
    for got, want in ((gP, a / (2 * POWER)), (gL, a / LU), (gS, -a / SIGMA_R), (gE, -a / E0)):
        assert abs(float(got) / want - 1) < 1e-12
    h = 1e-6
    fd = (_amplitude_restated(POWER, K + h, LU, SIGMA_R, E0)[0] - _amplitude_restated(POWER, K - h, LU, SIGMA_R, E0)[0]) / (2 * h)
    assert abs(float(gK) / fd - 1) < 1e-8
    # the resonant wavelength
    lam = _undulator().resonant_wavelength(t(E0))
    assert lam.dtype == F64 and abs(float(lam) / 7.017329e-7 - 1) < 1e-6
    assert abs(float(lam) / (PERIOD * (1 + K**2 / 2) / (2 * (E0 / M_E) ** 2)) - 1) < 1e-14
    assert abs(float(_undulator(ky=None, kx=t(K)).resonant_wavelength(E0)) / float(lam) - 1) < 1e-14
    assert float(_undulator().resonant_wavelength(t(2e9), species=proton)) > 1e3 * float(lam)


@pytest.mark.parametrize("n", [1, 3])
def test_with_laser_structure(n):
    import cheetah_amd as ca

    und = _undulator()
    seg = und.with_laser(POWER, SIGMA_R, E0, phase=0.4, offset_x=1e-5, offset_y=-2e-5, pulse_sigma=3e-4, pulse_center=1e-4, num_kicks=n)
    assert type(seg) is ca.Segment and seg.name == "U" and len(seg.elements) == 3 * n
    assert [type(e) for e in seg.elements] == [ca.Undulator, ca.LaserModulator, ca.Undulator] * n
    names = [e.name for e in seg.elements]
    assert names[:3] == ["U_laser_0", "U_laser_kick_0", "U_laser_1"] and len(set(names)) == 3 * n
    assert names[-3:] == [f"U_laser_{2 * n - 2}", f"U_laser_kick_{n - 1}", f"U_laser_{2 * n - 1}"]
    pieces = [e for e in seg.elements if isinstance(e, ca.Undulator)]
    kicks = [e for e in seg.elements if isinstance(e, ca.LaserModulator)]
    for p in pieces:
        assert abs(float(p.length) - LU / (2 * n)) < 1e-16 and float(p.ky) == K and float(p.kx) == 0.0 and float(p.period) == PERIOD
        assert p.length.dtype == F64
    assert abs(float(seg.length) - LU) < 1e-15
    ref, _ = _amplitude_restated(POWER, K, LU / n, SIGMA_R, E0)
    lam = float(und.resonant_wavelength(t(E0)))
    for k in kicks:
        assert abs(float(k.amplitude) / ref - 1) < 1e-9 and k.amplitude.dtype == F64
        assert float(k.wavelength) == lam                       # wavelength=None: the resonant one
        assert (float(k.phase), float(k.offset_x), float(k.offset_y), float(k.pulse_sigma), float(k.pulse_center)) == \
            (0.4, 1e-5, -2e-5, 3e-4, 1e-4)
        assert float(k.laser_sigma) == SIGMA_R
    # n kicks of L_u / n add up to the one kick's amplitude
    assert abs(n * float(kicks[0].amplitude) / 77585.65 - 1) < 1e-6


def test_with_laser_arguments():
    und = _undulator()
    seg = und.with_laser(t(POWER), t(SIGMA_R), t(E0), wavelength=8e-7)
    kick = seg.elements[1]
    assert float(kick.wavelength) == 8e-7 and kick.pulse_sigma is None and float(kick.phase) == 0.0
    # K from kx when that is the non-zero one
    assert float(_undulator(ky=None, kx=t(K)).with_laser(POWER, SIGMA_R, E0).elements[1].amplitude) == float(kick.amplitude)
    # both or neither non-zero: not a planar undulator
    for kw in ({"kx": t(0.5)}, {"ky": None}):
        with pytest.raises(ValueError, match="planar"):
            _undulator(**kw).with_laser(POWER, SIGMA_R, E0)
    for bad in (0, -1, 1.0, True):
        with pytest.raises(ValueError):
            und.with_laser(POWER, SIGMA_R, E0, num_kicks=bad)
    with pytest.raises(ValueError):
        und.with_laser(POWER, -SIGMA_R, E0)
    with pytest.raises(ValueError):
        und.with_laser(POWER, SIGMA_R, E0, wavelength=0.0)


def test_tracking_errors_before_any_device_work():
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    for k in (_kick(), _kick(pulse_sigma=t(1e-3))):
        with pytest.raises(RuntimeError, match="GPU only"):
            k.track(beam)
        with pytest.raises(TypeError, match="needs a ParticleBeam"):
            k.track(ca.ParameterBeam.from_parameters())
    # nothing about particle-sharded beams: no particle depends on another, so the kick is the same on every rank
    with ca.sharding.particle_sharded():
        with pytest.raises(RuntimeError, match="GPU only"):
            _kick().track(beam)
