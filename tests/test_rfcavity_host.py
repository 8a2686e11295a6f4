"""Host side of the RFCavity (no GPU): the constructor, the parameter order, the one tracking method, `clone`, the LatticeJSON
round trip, `harmonic_frequency`, the C ABI's argument checks that return before any launch — and the stored vectors of
tests/golden/dkd_rfcavity.npz against a restatement of the map in float64 torch on the CPU."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dkd_rfcavity.npz")
F64 = {"dtype": torch.float64}
C_LIGHT = 299792458.0


def t(v):
    return torch.tensor(v, **F64)


def make(**kw):
    import cheetah_amd as ca

    return ca.RFCavity(t(0.3), voltage=t(1e6), phase=t(0.13), frequency=t(480e6), name="rf", **kw, **F64)


# ---- constructor ---------------------------------------------------------------------------------------------------------------------
def test_constructor_defaults_and_parameter_order():
    import cheetah_amd as ca
    import cheetah_amd.accelerator as acc
    from cheetah_amd import _ops

    assert acc.RFCavity is ca.RFCavity
    assert _ops.DKD_KIND["rfcavity"] == 6 and ca.RFCavity._dkd_kind == 6 and _ops.DKD_NUM_PARAMS[6] == 4
    d = ca.RFCavity(t(0.0), name="thin", **F64)                  # a thin cavity is allowed; every setting defaults to 0
    assert (float(d.length), float(d.voltage), float(d.phase), float(d.frequency)) == (0.0, 0.0, 0.0, 0.0)
    assert d.voltage.dtype == torch.float64 and d.tracking_method == "drift_kick_drift"
    assert not d.is_active and not d.is_skippable
    c = make()
    assert c.is_active and not c.is_skippable
    assert [float(p) for p in c._dkd_params()] == [0.3, 1e6, 0.13, 480e6]
    refs = c._dkd_scalar_refs()
    assert [(r[0] is tn, r[1]) for r, tn in zip(refs, (c.length, c.voltage, c.phase, c.frequency))] == [(True, None)] * 4
    assert c._dkd_options() == (1, 0)                            # num_steps is not read, no fringe
    assert c.defining_features == ["name", "length", "voltage", "phase", "frequency"]
    assert not hasattr(c, "tilt") and not hasattr(c, "misalignment")
    with pytest.raises(ValueError, match="length"):
        ca.RFCavity(t(-0.1), **F64)
    # positional: (length, voltage, phase, frequency, tracking_method, name)
    p = ca.RFCavity(t(0.2), t(2e6), t(0.5), t(1e9), "drift_kick_drift", "pos", None, None, None, torch.float64)
    assert (float(p.length), float(p.voltage), float(p.phase), float(p.frequency), p.name) == (0.2, 2e6, 0.5, 1e9, "pos")
    # a Parameter stays a Parameter
    q = ca.RFCavity(t(0.2), voltage=torch.nn.Parameter(t(1e6)), **F64)
    assert isinstance(q.voltage, torch.nn.Parameter)


def test_only_drift_kick_drift_is_offered():
    import cheetah_amd as ca

    assert ca.RFCavity.supported_tracking_methods == ["drift_kick_drift"]
    c = make()
    for method in ("linear", "second_order", "bmadx"):
        with pytest.warns(ca.PhysicsWarning, match=f"Invalid tracking method '{method}'"):
            c.tracking_method = method
        assert c.tracking_method == "drift_kick_drift"
    with pytest.warns(ca.PhysicsWarning, match="Invalid tracking method 'linear'"):
        assert make(tracking_method="linear").tracking_method == "drift_kick_drift"


def test_clone_split_repr():
    c = make()
    k = c.clone()
    assert k is not c and type(k) is type(c) and k.name == "rf" and k.tracking_method == "drift_kick_drift"
    for name in ("length", "voltage", "phase", "frequency"):
        assert torch.equal(getattr(k, name), getattr(c, name)) and getattr(k, name) is not getattr(c, name), name
    assert c.split(t(0.05)) == [c]                               # one kick: not split, like the TransverseDeflectingCavity
    text = repr(c)
    assert text.startswith("RFCavity(name='rf', length=") and "voltage=" in text and "phase=" in text and "frequency=" in text


def test_lattice_json_round_trip(tmp_path):
    import cheetah_amd as ca

    seg = ca.Segment([ca.Drift(t(0.5), name="d", **F64), make(), ca.RFCavity(t(0.0), voltage=t(-2e5), phase=t(0.5), frequency=t(1.3e9),
                                                                            name="thin", **F64)], name="cell")
    path = tmp_path / "cell.json"
    seg.to_lattice_json(str(path))
    with open(path) as f:
        written = json.load(f)["elements"]
    assert written["rf"][0] == "RFCavity"
    assert written["rf"][1] == {"length": 0.3, "voltage": 1e6, "phase": 0.13, "frequency": 480e6, "metadata": {}}
    back = ca.Segment.from_lattice_json(str(path), **F64)
    assert type(back.rf) is ca.RFCavity and type(back.thin) is ca.RFCavity
    for el in ("rf", "thin"):
        for name in ("length", "voltage", "phase", "frequency"):
            assert torch.equal(getattr(getattr(back, el), name), getattr(getattr(seg, el), name)), (el, name)


def test_harmonic_frequency():
    import cheetah_amd as ca
    from cheetah_amd.particles.species import electron_mass_eV

    C, h, E = 48.0, 77, 1e8
    beta0 = math.sqrt(1.0 - (electron_mass_eV / E) ** 2)
    f = ca.RFCavity.harmonic_frequency(t(C), h, t(E))
    assert isinstance(f, torch.Tensor) and f.dtype == torch.float64
    assert abs(float(f) - h * beta0 * C_LIGHT / C) <= 2e-16 * 4 * float(f)
    proton = ca.Species("proton", **F64)
    beta_p = math.sqrt(1.0 - (float(proton.mass_eV) / 2e9) ** 2)
    fp = ca.RFCavity.harmonic_frequency(t(C), h, t(2e9), species=proton)
    assert abs(float(fp) - h * beta_p * C_LIGHT / C) <= 2e-16 * 4 * float(fp) and float(fp) < float(f)


# ---- C ABI: what returns before a launch ---------------------------------------------------------------------------------------------
def test_c_abi_knows_the_kind():
    import cheetah_amd._lib as L

    lib = L.lib()
    assert lib.chx_abi_version() == 9
    # the exported count keeps the answers of ABI 9 (6 was no kind); the entry points and the partials' count know the four parameters
    assert lib.chx_dkd_num_params(6) == -1 and lib.chx_dkd_num_params(7) == -1 and lib.chx_dkd_num_params(4) == -1
    assert [lib.chx_dkd_num_params(k) for k in (0, 1, 2, 3, 5)] == [1, 5, 9, 7, 5]
    assert lib.chx_dkd_bwd_partials_count(6, 2, 700) == 2 * 3 * 5 and lib.chx_dkd_bwd_partials_count(7, 2, 700) == 0
    ok, invalid = 0, -1
    # an empty beam returns CHX_OK behind the check of the kind and before every other: 6 is known, 7 is not
    for precision in (0, 1, 2):
        assert lib.chx_dkd_track_p(6, None, None, None, 0.511e6, -1.0, 1, 0, 1, 1, 1, 1, 0, 0, precision, None, None, None) == ok
        assert lib.chx_dkd_track_p(7, None, None, None, 0.511e6, -1.0, 1, 0, 1, 1, 1, 1, 0, 0, precision, None, None, None) == invalid
    assert lib.chx_dkd_track_bwd(6, None, None, None, None, 0.511e6, -1.0, 1, 0, 1, 1, 1, 1, 0, 1, None, None, None) == ok
    assert lib.chx_dkd_track_bwd(7, None, None, None, None, 0.511e6, -1.0, 1, 0, 1, 1, 1, 1, 0, 1, None, None, None) == invalid
    # the other argument checks hold for the kind: null pointers, fringe_at outside 0 .. 3 (num_steps is not read: any value)
    assert lib.chx_dkd_track_p(6, None, 0x20000, 0x30000, 0.511e6, -1.0, 1, 0, 1, 1, 1, 1, 700, 0, 0, 0x40000, None, None) == invalid
    assert lib.chx_dkd_track_p(6, 0x10000, 0x20000, 0x30000, 0.511e6, -1.0, 1, 4, 1, 1, 1, 1, 700, 0, 0, 0x40000, None, None) == invalid


def test_ring_entry_point_still_refuses_the_other_kinds_before_any_launch():
    """chx_dkd_turns with a cavity among its items (kind 6) and a kind it does not take: 3 (the TDC), 4 (a linear run), -1, 7.
    (That it TAKES kind 6 cannot be seen without a launch: every refusal has one code. tests/test_gpu_rfcavity.py runs it.)"""
    import cheetah_amd._lib as L

    lib = L.lib()
    E, N = 3, 1000
    i32, vp = ctypes.c_int32 * 193, ctypes.c_void_p * 193
    ws_bytes = lib.chx_dkd_turns_workspace_bytes(E, N, 4, 4, 0)
    pad = lambda v, fill: list(v) + [fill] * (193 - len(v))  # noqa: E731
    for kinds in ((6, 3, 0), (6, 4, 2), (-1, 6, 1), (0, 6, 7), (7, 7, 7)):
        ka, pa, sa, fa = i32(*pad(kinds, 0)), vp(*([0x10000] * 193)), i32(*pad((1, 1, 1), 1)), i32(*pad((0, 0, 0), 0))
        assert lib.chx_dkd_turns(ka, pa, sa, fa, 2, E, 0x20000, 0x21000, 0x22000, 0.511e6, -1.0, None, None, N, 0, 1, 4, 1, None, 2, 0x30000,
                                 0x40000, 0x50000, 0x60000, None, None, 0x70000, ws_bytes, None) == -1, kinds


# ---- the stored vectors against a restatement on the CPU -----------------------------------------------------------------------------
def turn_sincos(u):
    """sin and cos of 2 pi u (u in turns, a float64 tensor) from the reduced phase: r = u - round(u) is exact, the quadrant
    j = round(4 r) is split off exactly, and the sine and cosine of the rest, |y| <= 1/8 turn, are rotated by it — so that
    u = 0, 1/4, 1/2 ... give exact zeros and ones, as sincospi does."""
    r = u - torch.round(u)
    j = torch.round(4 * r)
    y = r - j / 4
    s, c = torch.sin(2 * math.pi * y), torch.cos(2 * math.pi * y)
    q = j.to(torch.int64) % 4
    sin = torch.where(q == 0, s, torch.where(q == 1, c, torch.where(q == 2, -s, -c)))
    cos = torch.where(q == 0, c, torch.where(q == 1, -s, torch.where(q == 2, -c, s)))
    return sin, cos


def restated_map(x, energy, mc2, nq, length, voltage, phase, frequency):
    """The map of include/chx.h (CHX_DKD_RFCAVITY) in float64 torch: (tau, delta) <-> (z, pz) once, half a drift, the kick with
    the reduced phase and the addition theorem, half a drift. Differentiable in every argument."""
    X, px, Y, py, tau, delta = (x[:, j] for j in range(6))
    p0c = torch.sqrt(energy ** 2 - mc2 ** 2)
    en = energy + delta * p0c
    p = torch.sqrt(en ** 2 - mc2 ** 2)
    z, pz = -(p / en) * tau, (p - p0c) / p0c

    def drift(L, X, Y, z, pz):
        P = 1 + pz
        Px, Py = px / P, py / P
        Pxy2 = Px ** 2 + Py ** 2
        Pl = torch.sqrt(1 - Pxy2)
        so = lambda v: v / (torch.sqrt(1 + v) + 1)  # noqa: E731
        dz = L * (so(mc2 ** 2 * (2 * pz + pz ** 2) / ((p0c * P) ** 2 + mc2 ** 2)) + so(-Pxy2) / Pl)
        return X + L * Px / Pl, Y + L * Py / Pl, z + dz

    X, Y, z = drift(length / 2, X, Y, z, pz)
    pc_old = (1 + pz) * p0c
    beta_old = pc_old / torch.sqrt(pc_old ** 2 + mc2 ** 2)
    time = -z / (beta_old * C_LIGHT)
    S0, C0 = turn_sincos(phase)
    sn, cs = turn_sincos(frequency * time)
    E_new = pc_old / beta_old + abs(nq) * voltage * (S0 * cs - C0 * sn)
    pc = torch.sqrt(E_new ** 2 - mc2 ** 2)
    beta = pc / E_new
    pz = (pc - p0c) / p0c
    z = z * beta / beta_old
    X, Y, z = drift(length / 2, X, Y, z, pz)
    pe = (1 + pz) * p0c
    ee = torch.sqrt(pe ** 2 + mc2 ** 2)
    ref = torch.sqrt(p0c ** 2 + mc2 ** 2)
    return torch.stack([X, px, Y, py, -z / (pe / ee), (ee - ref) / p0c, torch.ones_like(X)], dim=1), ref


def golden_cases():
    """(name, tag, x, energy, mc2, nq, params, want, energy_out) of every stored case and beam."""
    g = np.load(GOLDEN)
    for name in g["names"]:
        sp = str(g[f"{name}_species"])
        mc2, nq = g[f"{sp}_species"]
        for tag in g["beams"]:
            yield (str(name), str(tag), torch.from_numpy(g[f"{sp}_in_{tag}"]), float(g[f"{sp}_energy"]), float(mc2), float(nq),
                   g[f"{name}_params"], g[f"{name}_{tag}_out"], float(g[f"{name}_{tag}_energy_out"]))


def column_errors(got, want):
    """max |got - want| per column over the column's largest magnitude, over the rows that are finite in `want`; the NaN pattern
    must be the same."""
    assert (np.isnan(got) == np.isnan(want)).all(), "NaN in other places"
    live = ~np.isnan(want).any(axis=1)
    return np.abs(got[live] - want[live]).max(axis=0) / np.abs(want[live]).max(axis=0)


def test_stored_vectors_cover_the_cases():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 512 * 1024
    params = {str(n): g[f"{n}_params"] for n in g["names"]}
    assert {(str(g[f"{n}_species"]), p[2], p[0]) for n, p in params.items()} >= \
        {("electron", ph, L) for ph in (0.0, 0.5, 0.13) for L in (0.0, 0.3)} | {("proton", 0.13, 0.0), ("proton", 0.13, 0.3)}
    assert list(g["beams"]) == ["short", "long"]
    f = float(g["frequency"])
    for sp in ("electron", "proton"):
        assert g[f"{sp}_in_short"].shape == g[f"{sp}_in_long"].shape == (257, 7)
        turns = np.abs(g[f"{sp}_in_long"][:, 4]) * f / C_LIGHT
        assert (turns > 1).sum() > 50 and turns.max() > 2                      # the reduction is exercised
    # the doomed particle: the last row of the long beam, NaN in x, y, tau, delta where it is decelerated below its rest mass
    lost = {n: np.isnan(g[f"{n}_long_out"]) for n in params}
    assert all(not m[:256].any() for m in lost.values()) and all(not np.isnan(g[f"{n}_short_out"]).any() for n in params)
    hit = [n for n, m in lost.items() if m[256].any()]
    assert "electron_phase0.13_L0" in hit and "proton_phase0.13_L0.3" in hit
    for n in hit:
        assert lost[n][256].tolist() == [True, False, True, False, True, True, False], n


def test_stored_vectors_match_the_restated_map():
    for name, tag, x, energy, mc2, nq, (length, voltage, phase, frequency), want, e_want in golden_cases():
        got, e_out = restated_map(x, t(energy), t(mc2), nq, t(length), t(voltage), t(phase), t(frequency))
        err = column_errors(got.numpy(), want)
        print(name, tag, "max error per column / the column's largest magnitude:", err)
        assert (err <= 1e-12).all(), (name, tag, err)
        assert (got[:, 6] == 1).all()
        assert abs(float(e_out) - e_want) <= 1e-15 * energy


def test_restated_zero_crossings_are_exact():
    """phase = 0 and 0.5 with a particle on the reference orbit (tau = 0): no energy change at all, not 1e-16 of the voltage."""
    x = torch.zeros(1, 7, **F64)
    x[0, 6] = 1.0
    for phase in (0.0, 0.5, 1.0, -0.5):
        out, _ = restated_map(x, t(1e8), t(510998.95069), -1.0, t(0.0), t(1e6), t(phase), t(480e6))
        assert float(out[0, 5]) == 0.0 and float(out[0, 4]) == 0.0, phase
