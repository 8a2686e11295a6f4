"""Host side of the Multipole (no GPU): the constructor, the parameter order, what it refuses, `clone`, `repr`, the LatticeJSON
round trip with `order` and `num_steps`, the C ABI's argument checks that return before any launch — and the stored vectors of
tests/golden/dkd_multipole.npz against a restatement of the map in float64 torch on the CPU."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dkd_multipole.npz")
RFCAVITY_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dkd_rfcavity.npz")
F64 = {"dtype": torch.float64}


def t(v):
    return torch.tensor(v, **F64)


def make(order=3, **kw):
    import cheetah_amd as ca

    return ca.Multipole(t(0.25), order, knl=t(2e4), ksl=t(-1e4), misalignment=t([1e-3, -5e-4]), tilt=t(-0.4), name="oct", **kw, **F64)


# ---- constructor ---------------------------------------------------------------------------------------------------------------------
def test_constructor_defaults_and_parameter_order():
    import cheetah_amd as ca
    import cheetah_amd.accelerator as acc
    from cheetah_amd import _ops

    assert acc.Multipole is ca.Multipole
    assert _ops.DKD_KIND["multipole"] == 8 and ca.Multipole._dkd_kind == 8 and _ops.DKD_NUM_PARAMS[8] == 6
    assert 7 not in _ops.DKD_KIND.values() and _ops.DKD_NUM_PARAMS[7] is None
    d = ca.Multipole(t(0.0), 2, name="thin", **F64)              # a thin element is allowed; the strengths default to 0
    assert (float(d.length), float(d.knl), float(d.ksl), float(d.tilt), d.misalignment.tolist()) == (0.0, 0.0, 0.0, 0.0, [0.0, 0.0])
    assert d.knl.dtype == torch.float64 and d.tracking_method == "drift_kick_drift" and d.order == 2 and d.num_steps == 1
    assert not d.is_active and not d.is_skippable
    assert ca.Multipole(t(0.0), 1, ksl=t(0.1), **F64).is_active and ca.Multipole(t(0.0), 1, knl=t(0.1), **F64).is_active
    m = make(num_steps=3)
    assert m.is_active and not m.is_skippable
    assert [float(p) for p in m._dkd_params()] == [0.25, 2e4, -1e4, -0.4, 1e-3, -5e-4]      # length first, like every kind
    refs = m._dkd_scalar_refs()
    assert [(r[0] is tn, r[1]) for r, tn in zip(refs, (m.length, m.knl, m.ksl, m.tilt, m.misalignment, m.misalignment))] == \
        [(True, None)] * 4 + [(True, 0), (True, 1)]
    assert m._dkd_options() == (3, 3)                            # (num_steps, the order where a Dipole's fringe bits travel)
    assert make(order=0)._dkd_options() == (1, 0)
    assert m.defining_features == ["name", "length", "order", "knl", "ksl", "misalignment", "tilt"]
    assert m.defining_tensors == ["length", "knl", "ksl", "misalignment", "tilt"]
    assert ca.Multipole.supported_tracking_methods == ["drift_kick_drift"]
    with pytest.warns(ca.PhysicsWarning, match="Invalid tracking method 'linear'"):
        m.tracking_method = "linear"
    assert m.tracking_method == "drift_kick_drift"
    # positional: (length, order, knl, ksl, misalignment, tilt, num_steps, tracking_method, name)
    p = ca.Multipole(t(0.2), 1, t(0.6), t(-0.3), t([1e-4, 2e-4]), t(0.1), 2, "drift_kick_drift", "pos", None, None, None, torch.float64)
    assert (float(p.length), p.order, float(p.knl), float(p.ksl), p.misalignment.tolist(), float(p.tilt), p.num_steps, p.name) == \
        (0.2, 1, 0.6, -0.3, [1e-4, 2e-4], 0.1, 2, "pos")
    q = ca.Multipole(t(0.0), 3, knl=torch.nn.Parameter(t(500.0)), **F64)        # a Parameter stays a Parameter
    assert isinstance(q.knl, torch.nn.Parameter)
    assert m.split(t(0.05)) == [m] and m.merge(make(num_steps=3)) is None       # the base behaviour, as the RFCavity


def test_refusals():
    import cheetah_amd as ca

    for order in (-1, 4, 7, True, False, 2.0, "2", None, t(2.0)):
        with pytest.raises(ValueError, match=r"Multipole\.order must be an int of 0 \.\. 3"):
            ca.Multipole(t(0.1), order, **F64)
    m = make()
    with pytest.raises(ValueError, match=r"Multipole\.order"):
        m.order = 4
    assert m.order == 3
    for steps in (0, -1, 1 << 25, True, 1.5, "3", None):
        with pytest.raises(ValueError, match=rf"Multipole\.num_steps must be an int of 1 \.\. {(1 << 25) - 1}"):
            ca.Multipole(t(0.1), 2, num_steps=steps, **F64)
        with pytest.raises(ValueError, match=r"Multipole\.num_steps"):
            m.num_steps = steps
    assert m.num_steps == 1
    m.num_steps = (1 << 25) - 1
    assert m.num_steps == (1 << 25) - 1
    m.num_steps = np.int64(4)                                    # anything with __index__, as for the Sextupole
    assert m.num_steps == 4 and type(m.num_steps) is int
    with pytest.raises(ValueError, match=r"Multipole\.length must not be negative"):
        ca.Multipole(t(-0.1), 2, **F64)


def test_an_edit_of_order_or_num_steps_moves_the_revision():
    m = make()
    before = m.__dict__["_revision"]
    m.order = 1
    assert m.__dict__["_revision"] > before and m._dkd_options() == (1, 1)
    before = m.__dict__["_revision"]
    m.num_steps = 5
    assert m.__dict__["_revision"] > before and m._dkd_options() == (5, 1)


def test_clone_and_repr():
    m = make(order=1, num_steps=3)
    k = m.clone()
    assert k is not m and type(k) is type(m) and k.name == "oct" and k.order == 1 and k.num_steps == 3
    for name in ("length", "knl", "ksl", "misalignment", "tilt"):
        assert torch.equal(getattr(k, name), getattr(m, name)) and getattr(k, name) is not getattr(m, name), name
    text = repr(m)
    assert text.startswith("Multipole(name='oct', length=") and ", order=1, knl=" in text and "ksl=" in text and text.endswith(", num_steps=3)")
    assert "num_steps" not in repr(make())                       # the default is not written, as for the Sextupole


def test_lattice_json_round_trip(tmp_path):
    import cheetah_amd as ca

    seg = ca.Segment([ca.Drift(t(0.5), name="d", **F64), make(num_steps=3),
                      ca.Multipole(t(0.0), 0, knl=t(-1e-4), name="hcor", **F64),
                      ca.Multipole(t(0.0), 1, ksl=t(0.02), name="skew", **F64)], name="cell")
    path = tmp_path / "cell.json"
    seg.to_lattice_json(str(path))
    with open(path) as f:
        written = json.load(f)["elements"]
    assert written["oct"][0] == "Multipole"
    assert written["oct"][1] == {"length": 0.25, "order": 3, "knl": 2e4, "ksl": -1e4, "misalignment": [1e-3, -5e-4], "tilt": -0.4,
                                 "num_steps": 3, "metadata": {}}
    assert written["hcor"][1] == {"length": 0.0, "order": 0, "knl": -1e-4, "ksl": 0.0, "misalignment": [0.0, 0.0], "tilt": 0.0,
                                  "metadata": {}}          # num_steps = 1 is not written
    back = ca.Segment.from_lattice_json(str(path), **F64)
    for el in ("oct", "hcor", "skew"):
        a, b = getattr(back, el), getattr(seg, el)
        assert type(a) is ca.Multipole and a.order == b.order and type(a.order) is int and a.num_steps == b.num_steps
        for name in ("length", "knl", "ksl", "misalignment", "tilt"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (el, name)


def test_the_ring_refusal_names_the_kind():
    """The text `track_turns(fused=True)` raises for a ring it does not take lists the Multipole (the check itself runs on the GPU)."""
    import cheetah_amd as ca
    from cheetah_amd.accelerator import segment

    ring = ca.Segment([make(), ca.Drift(t(1.0), tracking_method="drift_kick_drift", **F64),
                       ca.Quadrupole(t(0.2), k1=t(1.0), tracking_method="second_order", name="q", **F64)])
    reason = ring._turn_items_dkd(ring._plan(), torch.empty((0, 7), **F64))
    assert reason == "Quadrupole 'q' (tracking method 'second_order') is not a drift-kick-drift Drift, Quadrupole, Dipole, Sextupole, " \
                     "RFCavity or Multipole"
    ring.elements[2] = ca.Drift(t(0.5), tracking_method="drift_kick_drift", **F64)
    assert ring._turn_items_dkd(ring._plan(), torch.empty((0, 7), **F64)).kinds == [8, 0, 0]       # the Multipole itself is taken
    assert segment._DKD_IN_REGISTERS == (0, 1, 2, 5, 6, 8)


# ---- C ABI: what returns before a launch ---------------------------------------------------------------------------------------------
def test_c_abi_knows_the_kind():
    import cheetah_amd._lib as L

    lib = L.lib()
    assert lib.chx_abi_version() == 9
    # the exported count keeps the answers of ABI 9 (8 was no kind); the entry points and the partials' count know the six parameters
    assert lib.chx_dkd_num_params(8) == -1 and lib.chx_dkd_num_params(7) == -1 and lib.chx_dkd_num_params(9) == -1
    assert [lib.chx_dkd_num_params(k) for k in (0, 1, 2, 3, 5)] == [1, 5, 9, 7, 5]
    assert lib.chx_dkd_bwd_partials_count(8, 2, 700) == 2 * 3 * 7              # 6 parameters + the energy, per tile
    assert lib.chx_dkd_bwd_partials_count(8, 1, 256) == 7 and lib.chx_dkd_bwd_partials_count(8, 1, 257) == 14
    assert lib.chx_dkd_bwd_partials_count(7, 2, 700) == 0 and lib.chx_dkd_bwd_partials_count(9, 2, 700) == 0
    ok, invalid = 0, -1
    # an empty beam returns CHX_OK behind the check of the kind and before every other: 8 is known, 7 and 9 are not
    for precision in (0, 1, 2):
        for order in (0, 1, 2, 3):
            assert lib.chx_dkd_track_p(8, None, None, None, 0.511e6, -1.0, 1, order, 1, 1, 1, 1, 0, 0, precision, None, None, None) == ok
        for kind in (7, 9):
            assert lib.chx_dkd_track_p(kind, None, None, None, 0.511e6, -1.0, 1, 0, 1, 1, 1, 1, 0, 0, precision, None, None, None) == invalid
    assert lib.chx_dkd_track_bwd(8, None, None, None, None, 0.511e6, -1.0, 1, 3, 1, 1, 1, 1, 0, 1, None, None, None) == ok
    for kind in (7, 9):
        assert lib.chx_dkd_track_bwd(kind, None, None, None, None, 0.511e6, -1.0, 1, 0, 1, 1, 1, 1, 0, 1, None, None, None) == invalid
    # the other argument checks hold for the kind: null pointers, an order outside 0 .. 3, num_steps outside 1 .. 2^25 - 1
    for dtype in (0, 1):
        for precision in (0, 1, 2):
            call = lambda steps, order, x=0x10000: lib.chx_dkd_track_p(  # noqa: E731
                8, x, 0x20000, 0x30000, 0.511e6, -1.0, steps, order, 1, 1, 1, 1, 700, dtype, precision, 0x40000, None, None)
            assert call(1, 0, None) == invalid
            assert call(1, 4) == invalid and call(1, -1) == invalid
            assert call(0, 3) == invalid and call(1 << 25, 3) == invalid
        bwd = lambda steps, order: lib.chx_dkd_track_bwd(  # noqa: E731
            8, 0x10000, 0x20000, 0x30000, 0x50000, 0.511e6, -1.0, steps, order, 1, 1, 1, 1, 700, dtype, 0x40000, None, None)
        assert bwd(1, 4) == invalid and bwd(0, 3) == invalid and bwd(1 << 25, 3) == invalid


def test_ring_entry_point_still_refuses_the_other_kinds_before_any_launch():
    """chx_dkd_turns with a Multipole among its items (kind 8) and a kind it does not take: 3 (the TDC), 9, 7, 4 (a linear run), -1.
    (That it TAKES kind 8 cannot be seen without a launch: every refusal has one code. tests/test_gpu_multipole.py runs it.)"""
    import cheetah_amd._lib as L

    lib = L.lib()
    E, N = 3, 1000
    i32, vp = ctypes.c_int32 * 193, ctypes.c_void_p * 193
    ws_bytes = lib.chx_dkd_turns_workspace_bytes(E, N, 4, 4, 0)
    pad = lambda v, fill: list(v) + [fill] * (193 - len(v))  # noqa: E731

    def call(kinds, steps=(1, 1, 1), orders=(0, 0, 0)):
        ka, pa, sa, fa = i32(*pad(kinds, 0)), vp(*([0x10000] * 193)), i32(*pad(steps, 1)), i32(*pad(orders, 0))
        return lib.chx_dkd_turns(ka, pa, sa, fa, 2, E, 0x20000, 0x21000, 0x22000, 0.511e6, -1.0, None, None, N, 0, 1, 4, 1, None, 2, 0x30000,
                                 0x40000, 0x50000, 0x60000, None, None, 0x70000, ws_bytes, None)

    for kinds in ((8, 3, 0), (8, 9, 8), (8, 7, 1), (8, 4, 2), (-1, 8, 1)):
        assert call(kinds) == -1, kinds
    # an order outside 0 .. 3 and a step count outside 1 .. 2^25 - 1 on a Multipole of an otherwise valid ring
    assert call((8, 0, 1), orders=(4, 0, 0)) == -1 and call((8, 0, 1), orders=(-1, 0, 0)) == -1
    assert call((8, 0, 1), steps=(0, 1, 1)) == -1 and call((8, 0, 1), steps=(1 << 25, 1, 1)) == -1


# ---- the stored vectors against a restatement on the CPU -----------------------------------------------------------------------------
def restated_map(x, energy, mc2, length, order, knl, ksl, tilt, mx, my, n):
    """The map of include/chx.h (CHX_DKD_MULTIPOLE) in float64 torch: (tau, delta) <-> (z, pz) once, the shift and the rotation, a
    drift of L / 2n, n x (kick, drift of L / n; L / 2n behind the last kick), the rotation and the shift back. The power of x + i y by
    `order` complex multiplications from 1. Differentiable in every tensor argument."""
    X, px, Y, py, tau, delta = (x[:, j] for j in range(6))
    p0c = torch.sqrt(energy ** 2 - mc2 ** 2)
    en = energy + delta * p0c
    p = torch.sqrt(en ** 2 - mc2 ** 2)
    z, pz = -(p / en) * tau, (p - p0c) / p0c
    s, c = torch.sin(tilt), torch.cos(tilt)
    xi, yi = X - mx, Y - my
    X, Y, px, py = xi * c + yi * s, -xi * s + yi * c, px * c + py * s, -px * s + py * c

    def drift(L, X, Y, z):
        P = 1 + pz
        Px, Py = px / P, py / P
        Pxy2 = Px ** 2 + Py ** 2
        Pl = torch.sqrt(1 - Pxy2)
        so = lambda v: v / (torch.sqrt(1 + v) + 1)  # noqa: E731
        dz = L * (so(mc2 ** 2 * (2 * pz + pz ** 2) / ((p0c * P) ** 2 + mc2 ** 2)) + so(-Pxy2) / Pl)
        return X + L * Px / Pl, Y + L * Py / Pl, z + dz

    h = length / (2 * n)
    bn, an = knl / math.factorial(order) / n, ksl / math.factorial(order) / n
    X, Y, z = drift(h, X, Y, z)
    for step in range(n):
        re, im = torch.ones_like(X), torch.zeros_like(X)
        for _ in range(order):
            re, im = re * X - im * Y, re * Y + im * X
        px, py = px - (bn * re - an * im), py + (bn * im + an * re)
        X, Y, z = drift(2 * h if step + 1 < n else h, X, Y, z)
    X, Y, px, py = X * c - Y * s + mx, X * s + Y * c + my, px * c - py * s, px * s + py * c
    pe = (1 + pz) * p0c
    ee = torch.sqrt(pe ** 2 + mc2 ** 2)
    ref = torch.sqrt(p0c ** 2 + mc2 ** 2)
    return torch.stack([X, px, Y, py, -z / (pe / ee), (ee - ref) / p0c, torch.ones_like(X)], dim=1), ref


def golden_cases():
    """(name, tag, x, energy, mc2, params, order, steps, want, energy_out) of every stored case and beam."""
    g = np.load(GOLDEN)
    mc2, _ = g["species"]
    for name in g["names"]:
        for tag in g["beams"]:
            yield (str(name), str(tag), torch.from_numpy(g[f"in_{tag}"]), float(g["energy"]), float(mc2), g[f"{name}_params"],
                   int(g[f"{name}_order"]), int(g[f"{name}_steps"]), g[f"{name}_{tag}_out"], float(g[f"{name}_{tag}_energy_out"]))


def test_stored_vectors_cover_the_cases():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) <= os.path.getsize(RFCAVITY_GOLDEN)
    sext = np.load(os.path.join(os.path.dirname(GOLDEN), "dkd_sextupole.npz"))
    assert list(g["beams"]) == ["1mm", "5mm"]
    for tag in g["beams"]:
        assert g[f"in_{tag}"].shape == (257, 7) and np.array_equal(g[f"in_{tag}"], sext[f"in_{tag}"])        # the sextupole generator's beams
    cases = {str(n): (g[f"{n}_params"], int(g[f"{n}_order"]), int(g[f"{n}_steps"])) for n in g["names"]}
    assert all(p[1] != 0 and p[2] != 0 for p, _, _ in cases.values())                    # both strengths, everywhere
    for order in range(4):
        mine = [(p, n) for p, m, n in cases.values() if m == order]
        assert any(p[0] == 0 for p, _ in mine) and any(p[0] > 0 for p, _ in mine), order   # a thin and a thick case per order
    assert {n for _, _, n in cases.values()} == {1, 3}
    shapes = {(p[3] != 0, bool(p[4] != 0 or p[5] != 0)) for p, _, _ in cases.values()}
    assert shapes == {(False, False), (True, False), (False, True), (True, True)}       # upright, tilted, misaligned, both
    for n in cases:
        for tag in g["beams"]:
            assert g[f"{n}_{tag}_out"].shape == (257, 7) and np.isfinite(g[f"{n}_{tag}_out"]).all()


def test_stored_vectors_match_the_restated_map():
    worst = 0.0
    for name, tag, x, energy, mc2, (length, knl, ksl, tilt, mx, my), order, n, want, e_want in golden_cases():
        got, e_out = restated_map(x, t(energy), t(mc2), t(length), order, t(knl), t(ksl), t(tilt), t(mx), t(my), n)
        err = (np.abs(got.numpy() - want).max(axis=0) / np.abs(want).max(axis=0))
        print(name, tag, "max error per column / the column's largest magnitude:", err)
        worst = max(worst, err.max())
        assert (err <= 1e-12).all(), (name, tag, err)
        assert (got[:, 6] == 1).all()
        assert abs(float(e_out) - e_want) <= 1e-15 * energy
    print("largest:", worst)


def test_restated_thin_dipole_kick_and_the_derivative_at_the_origin():
    """What the Horner form is for: a thin order-0 element moves px by -knl and py by +ksl, and the derivative of a thin
    order-m kick with respect to the strengths and the coordinates is right at x = y = 0 and at knl = ksl = 0."""
    x = torch.zeros(1, 7, **F64)
    x[0, 6] = 1.0
    z = t(0.0)
    out, _ = restated_map(x, t(1e8), t(510998.95069), z, 0, t(1e-4), t(-2e-4), z, z, z, 1)
    assert out[0, :4].tolist() == [0.0, -1e-4, 0.0, -2e-4]
    for order, want in ((1, (-0.6, -0.3, -0.3, 0.6)), (2, (0.0,) * 4), (3, (0.0,) * 4)):
        p = x.clone().requires_grad_(True)
        out, _ = restated_map(p, t(1e8), t(510998.95069), z, order, t(0.6), t(-0.3), z, z, z, 1)
        gx, = torch.autograd.grad(out[0, 1], p, retain_graph=True)
        gy, = torch.autograd.grad(out[0, 3], p)
        assert (float(gx[0, 0]), float(gx[0, 2]), float(gy[0, 0]), float(gy[0, 2])) == want, order      # d px / d (x, y), d py / d (x, y)
    knl = t(0.0).requires_grad_(True)
    p = x.clone()
    p[0, 0], p[0, 2] = 2e-3, -1e-3
    out, _ = restated_map(p, t(1e8), t(510998.95069), z, 3, knl, t(0.0), z, z, z, 1)
    g, = torch.autograd.grad(out[0, 1], knl)
    assert abs(float(g) + (2e-3 ** 3 - 3 * 2e-3 * 1e-3 ** 2) / 6) <= 1e-24
