"""The CSRDriftKick element without a GPU: exports and C-ABI symbols, workspace queries and rejected arguments, constructor errors,
element basics, LatticeJSON, the errors of tracking a beam that cannot be tracked here (before any device work), the structure of
Segment.with_csr_kicks with `drift_kicks`, the float64 restatement of the kick's table (`_b_table`, which the GPU tests use as their
reference) against 50-digit arithmetic, and the convergence of the node sums to the continuous formula."""
import math
import os
import re
import subprocess

import pytest
import torch

from cheetah_amd import CSRDriftKick

NEW_SYMBOLS = ("chx_csr_drift_workspace_bytes", "chx_csr_drift_kick", "chx_csr_drift_kick_bwd")
F64 = torch.float64


# ---- the float64 restatement of the table: the kernels' arithmetic, operation for operation ------------------------------------------
def _newton(psi, c, xh):
    """One Newton step for the root of psi^3 (psi + 4 xh) / (psi + xh) = c, over a common denominator."""
    a = psi + xh
    n = psi * psi * psi * (psi + 4.0 * xh) - c * a
    w = psi * (psi + 2.0 * xh)
    return psi - n * a / (3.0 * w * w)


def _root(c, xh):
    """psi(c) for c > 0 (any shape): 12 Newton steps from the power of two at or above the upper end c^(1/3) of its bracket
    (c = m 2^e with m < 1: 2^ceil(e / 3)) without a graph, and one more with it, so that autograd gives the root's implicit
    derivative."""
    with torch.no_grad():
        _, e = torch.frexp(c)
        psi = torch.ldexp(torch.ones_like(c), torch.ceil(e.to(F64) / 3).to(torch.int32))
        for _ in range(12):
            psi = _newton(psi, c, xh)
    return _newton(psi, c, xh)


class _Log1p(torch.autograd.Function):
    """log1p(x) for x > -1/2 as the kernels form it, from IEEE operations and the exact frexp (a library log1p differs by an ulp
    from one platform to the next, and the table's second differences magnify that): 1 + x = m 2^e with m in [sqrt(1/2),
    sqrt(2)), log m = 2 s (1 + z / 3 + ... + z^11 / 23), s = (m - 1) / (m + 1), z = s^2, ln 2 in two parts, and the rounding of
    1 + x put back to first order."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        u = 1.0 + x
        m, e = torch.frexp(u)
        small = m < 0.70710678118654757
        m = torch.where(small, 2.0 * m, m)
        e = e.to(F64) - small.to(F64)
        s = (m - 1.0) / (m + 1.0)
        z = s * s
        p = torch.full_like(z, 1.0 / 23.0)
        for n in range(10, -1, -1):
            p = 1.0 / (2 * n + 1) + z * p
        return e * 6.93147180369123816490e-01 + (2.0 * s * p + (e * 1.90821492927058770002e-10 + (x - (u - 1.0)) / u))

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g / (1.0 + x)


def _G_closed(psi, xh):
    return (0.5 * psi * psi + xh * xh * psi / (psi + xh)) - xh * xh * _Log1p.apply(psi / xh)


def _G(psi, xh, series=True):
    """G(psi; xh) = psi^2 / 2 + xh^2 psi / (psi + xh) - xh^2 log1p(psi / xh); below psi / xh = 1/4 (with `series`) the series
    xh^2 sum_(n=3)^(32) (-1)^(n+1) (1 - 1/n) r^n in Horner's form."""
    if float(xh) == 0.0:
        return 0.5 * psi * psi
    if not series:
        return _G_closed(psi, xh)
    r = psi / xh
    acc = torch.full_like(r, -(1.0 - 1.0 / 32.0))
    for n in range(31, 2, -1):
        c = 1.0 - 1.0 / n
        acc = (c if n & 1 else -c) + r * acc
    return torch.where(r < 0.25, xh * xh * (r * r * r * acc), _G_closed(psi, xh))


def _y_max(xh, phi, kappa):
    return phi * phi * phi * (phi + 4.0 * xh) / (kappa * (phi + xh))


def _t_table(M, xh, phi, kappa, series=True):
    """t_i = G(psi_i), i = 0 ... M, psi_i = min(psi(i h), phi): phi itself for i > p = floor(y) (held fixed); t_0 = 0."""
    p = int(min(math.floor(float(_y_max(xh, phi, kappa))), M))
    i = torch.arange(1, M + 1, dtype=F64)
    psi = _root(i * kappa, xh)
    psi = torch.where(psi > phi, phi, psi)
    psi = torch.where(i > p, phi, psi)
    return torch.cat([torch.zeros(1, dtype=F64), _G(psi, xh, series)]), p


def _b_table(M, xh, phi, kappa):
    """b_j, j < M, for 0-d float64 xh >= 0, phi > 0, kappa > 0 (differentiable in all three, the lags p and p + 1 held fixed):
    b_0 = -g_0, b_j = g_(j-1) - g_j, g_j = t_(j+1) - t_j, then -beta (1 - f, f) at the lags (p, p + 1), beta = kappa / (3 (phi + 2
    xh)), f = y - p."""
    t, p = _t_table(M, xh, phi, kappa)
    g = t[1:] - t[:-1]
    b = torch.cat([(t[:1] - t[:1]) - g[:1], g[:-1] - g[1:]])
    beta = kappa / (3.0 * (phi + 2.0 * xh))
    y = _y_max(xh, phi, kappa)
    j = torch.arange(M)
    e = lambda n: (j == n).to(F64)  # noqa: E731     (zero for a lag beyond the grid)
    return b - beta * (1.0 - (y - p)) * e(p) - beta * (y - p) * e(p + 1)


# ---- exports and the C ABI ---------------------------------------------------------------------------------------------------------
def test_exported_from_the_package_and_the_accelerator_module():
    import cheetah_amd as ca
    import cheetah_amd.accelerator as acc

    assert ca.CSRDriftKick is acc.CSRDriftKick is CSRDriftKick
    assert issubclass(CSRDriftKick, ca.Element) and not issubclass(CSRDriftKick, (ca.CSRKick, ca.TransientCSRKick))
    assert callable(ca._ops.csr_drift_kick) and callable(ca._ops.csr_drift_factors)


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
    assert "CHX_CSR_DRIFT_STATE_DOUBLES" in header
    assert lib.chx_abi_version() == 9


def test_workspace_and_invalid_arguments_on_the_host():
    import cheetah_amd._lib as L

    lib = L.lib()
    ws = lib.chx_csr_drift_workspace_bytes
    assert ws(1, 10**6, 500) > 0
    assert ws(4, 10**6, 4096) > ws(1, 10**6, 4096)
    assert ws(1, 10**6, 500) > lib.chx_csr_workspace_bytes(1, 10**6, 500)      # the partials of the shape numbers' cotangents
    assert ws(1, 10**6, 1) == 0
    assert ws(1, 10**6, 4097) == 0
    assert ws(0, 10**6, 200) == 0
    assert ws(1, 0, 200) == 0
    # rejected before any device work: no particles, M out of range, a non-positive mass, a distance of neither 1 nor B rows
    assert lib.chx_csr_drift_kick(None, None, None, None, None, None, None, None, 511e3, 1.0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 10, 8, 0,
                                  None, None, None, 0, None) == -1
    assert lib.chx_csr_drift_kick_bwd(None, None, None, 1, 1, 1, 1, 10, 8, 0, None, None, None, None, None, None, None, None, None, 0,
                                      None) == -1
    x = torch.zeros(10, 7, dtype=F64)
    q = w = torch.ones(10, dtype=F64)
    e = torch.ones(1, dtype=F64)
    p = [t.data_ptr() for t in (x, q, w, e, e, e, e, e)]
    state = torch.zeros(64, dtype=F64)
    for M, mass, Bd in ((1, 511e3, 1), (4097, 511e3, 1), (8, 0.0, 1), (8, -1.0, 1), (8, 511e3, 2), (8, 511e3, 0)):
        assert lib.chx_csr_drift_kick(*p, mass, 1.0, 1, 1, 1, 1, 1, 1, 1, 1, Bd, 10, M, 1, x.data_ptr(), state.data_ptr(), None, 0,
                                      None) == -1
    # a missing bend_length pointer, and a missing d_kappa in the backward call
    p[5] = None
    assert lib.chx_csr_drift_kick(*p, 511e3, 1.0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 10, 8, 1, x.data_ptr(), state.data_ptr(), None, 0,
                                  None) == -1
    a, s = x.data_ptr(), state.data_ptr()
    assert lib.chx_csr_drift_kick_bwd(a, a, a, 1, 1, 1, 1, 10, 8, 1, s, a, a, None, s, s, s, None, None, 0, None) == -1


# ---- the element -------------------------------------------------------------------------------------------------------------------
def _kick(**kw):
    args = {"effect_length": torch.tensor(0.1), "bend_length": torch.tensor(0.4), "bend_angle": torch.tensor(0.02),
            "exit_distance": torch.tensor(0.05)}
    args.update(kw)
    return CSRDriftKick(**args)


@pytest.mark.parametrize("kw", [
    {"exit_distance": torch.tensor(-0.01)},
    {"exit_distance": torch.tensor([0.1, -1e-3])},
    {"exit_distance": torch.tensor(float("nan"))},
    {"exit_distance": torch.tensor(float("inf"))},
    {"bend_length": torch.tensor(-0.4)},
    {"bend_length": torch.tensor([0.4, float("inf")])},
    {"bend_length": torch.tensor(float("nan"))},
    {"num_bins": 1},
    {"num_bins": 4097},
    {"num_bins": 0},
    {"num_bins": 2.5},
    {"num_bins": True},
    {"effect_length": torch.tensor(-0.1)},
    {"effect_length": torch.tensor([0.1, -1e-3])},
    {"effect_length": torch.tensor(float("nan"))},
    {"effect_length": torch.tensor(float("inf"))},
    {"bend_angle": torch.tensor(float("nan"))},
    {"bend_angle": torch.tensor(float("inf"))},
])
def test_constructor_value_errors(kw):
    with pytest.raises(ValueError):
        _kick(**kw)


def test_element_basics():
    import cheetah_amd as ca

    k = _kick(num_bins=37, name="csrd1")
    assert not k.is_skippable
    assert float(k.length) == 0.0
    assert k.split(torch.tensor(0.1)) == [k]
    settings = ["effect_length", "bend_length", "bend_angle", "exit_distance"]
    assert k.defining_features == ["name", *settings, "num_bins"]
    assert k.defining_tensors == settings
    r = repr(k)
    assert r.startswith("CSRDriftKick(name='csrd1', effect_length=tensor(0.1000)") and "num_bins=37" in r
    assert "exit_distance=tensor(0.0500)" in r and "bend_length=tensor(0.4000)" in r
    c = k.clone()
    assert type(c) is type(k) and c.name == "csrd1" and c.num_bins == 37
    for f in settings:
        assert torch.equal(getattr(c, f), getattr(k, f)) and getattr(c, f) is not getattr(k, f)
    assert _kick().num_bins == 200
    assert float(_kick(exit_distance=0.0).exit_distance) == 0.0                 # x = 0 is allowed: the bend's exit face
    for zero in ("effect_length", "bend_length", "bend_angle"):                 # allowed: no kick
        assert float(getattr(_kick(**{zero: torch.tensor(0.0)}), zero)) == 0.0
    with pytest.raises(NotImplementedError):
        k.first_order_transfer_map(torch.tensor(1e8), ca.Species("electron"))
    # batched settings and float arguments
    b = CSRDriftKick([0.1, 0.2, 0.0], 0.4, torch.tensor([[0.01], [-0.02]], dtype=F64), [0.05, 0.1, 0.0], dtype=F64)
    assert b.effect_length.shape == (3,) and b.bend_angle.shape == (2, 1) and b.bend_length.shape == ()
    assert b.exit_distance.shape == (3,) and b.exit_distance.dtype == F64
    p = CSRDriftKick(*(torch.nn.Parameter(torch.tensor(v)) for v in (0.3, 0.4, 0.01, 0.1)))
    assert {n for n, _ in p.named_parameters()} == set(settings)
    doc = CSRDriftKick.__doc__
    for limit in ("ultra-relativistic", "1-D", "this one bend only", "straight in front of the bend is ignored"):
        assert limit in doc, limit
    assert "CSRDriftKick" in ca.CSRKick.__doc__ and "CSRDriftKick" in ca.TransientCSRKick.__doc__


def test_lattice_json_round_trip(tmp_path):
    import cheetah_amd as ca

    k = _kick(effect_length=torch.tensor(0.25), bend_length=torch.tensor(0.5), bend_angle=torch.tensor(-0.03),
              exit_distance=torch.tensor(0.125), num_bins=123, name="csrd")
    seg = ca.Segment([ca.Drift(torch.tensor(1.0), name="d1"), k, ca.Drift(torch.tensor(0.5), name="d2")], name="lat")
    path = tmp_path / "lattice.json"
    ca.latticejson.save_cheetah_model(seg, str(path))
    back = ca.latticejson.load_cheetah_model(str(path))
    k2 = back.elements[1]
    assert type(k2) is CSRDriftKick and k2.name == "csrd" and k2.num_bins == 123
    for f in ("effect_length", "bend_length", "bend_angle", "exit_distance"):
        assert torch.allclose(getattr(k2, f), getattr(k, f)), f


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


def test_factors_restated_for_the_chain_rule():
    import cheetah_amd as ca

    t = lambda *v: torch.tensor(v, dtype=F64)  # noqa: E731
    e, L, Lb, th, d, h = t(1e8, 1e8, 1e8, 1e8), t(0.2, 0.0, 0.2, 0.2), t(0.5, 0.5, 0.0, 0.5), t(-0.04, -0.04, -0.04, 0.0), \
        t(0.3, 0.3, 0.3, 0.3), t(1e-6, 1e-6, 1e-6, 1e-6)
    leaves = [v.clone().requires_grad_() for v in (e, L, Lb, th, d)]
    scale, xh, phi, kappa = ca._ops.csr_drift_factors(leaves[0], 510998.95, 1.0, *leaves[1:], h)
    p0c = math.sqrt(1e8 ** 2 - 510998.95 ** 2)
    assert abs(float(scale[0].detach()) - 0.2 / p0c) < 1e-12 * 0.2 / p0c
    assert float(xh[0].detach()) == 0.3 * 0.04 / 0.5 and float(phi[0].detach()) == 0.04 and float(kappa[0].detach()) == 24 * 1e-6 * 0.04 / 0.5
    for f in (scale, xh, phi, kappa):
        assert torch.equal(f[1:], torch.zeros(3, dtype=F64))                    # no kick where L, L_b or theta is 0
    (scale.sum() + xh.sum() + phi.sum() + kappa.sum()).backward()
    for v in leaves:
        assert torch.isfinite(v.grad).all() and torch.equal(v.grad[1:], torch.zeros(3, dtype=F64))
    assert float(leaves[3].grad[0]) < 0                                          # through |theta|
    # a row without a grid
    none = ca._ops.csr_drift_factors(e[:1], 510998.95, 1.0, L[:1], Lb[:1], th[:1], d[:1], t(0.0))
    assert all(float(f) == 0.0 for f in none)


# ---- Segment.with_csr_kicks(..., drift_kicks=n) ---------------------------------------------------------------------------------------
def _t(v):
    return torch.tensor(v, dtype=F64)


def _lattice():
    import cheetah_amd as ca

    inner = ca.Segment([ca.Drift(_t(0.6), name="d3"), ca.Marker(name="m2")], name="inner")
    return ca.Segment([ca.Drift(_t(1.0), name="d0"), ca.Dipole(_t(0.5), angle=_t(0.05), name="b1"), ca.Drift(_t(2.0), name="d1"),
                       ca.Quadrupole(_t(0.2), k1=_t(1.5), name="q1"), ca.Marker(name="m1"), inner,
                       ca.Dipole(_t(0.4), angle=_t(-0.04), name="b2"), ca.Drift(_t(1.0), name="d4")], name="lat")


def _flat(seg):
    import cheetah_amd as ca

    return [x for e in seg.elements for x in (_flat(e) if isinstance(e, ca.Segment) else [e])]


def test_with_csr_kicks_drift_structure():
    import cheetah_amd as ca

    seg = _lattice()
    out = seg.with_csr_kicks(2, num_bins=77, transient=True, drift_kicks=3)
    assert type(out) is ca.Segment and out.name == "lat"
    bend = lambda b: [f"{b}_csr{s}_{i}" for i in range(2) for s in ("", "_kick")]  # noqa: E731
    drift = lambda d: [f"{d}_csr_drift{s}_{i}" for i in range(3) for s in ("", "_kick")]  # noqa: E731
    assert [e.name for e in out.elements] == ["d0"] + bend("b1") + drift("d1") + ["q1", "q1_csr_drift_kick", "m1", "inner"] + \
        bend("b2") + drift("d4")
    nested = out.elements[14]
    assert type(nested) is ca.Segment and [e.name for e in nested.elements] == drift("d3") + ["m2"]
    assert out.elements[0] is seg.elements[0]                                   # nothing in front of the first bend
    kicks = [k for k in _flat(out) if isinstance(k, CSRDriftKick)]
    assert len(kicks) == 10 and all(k.num_bins == 77 and k.exit_distance.dtype == F64 for k in kicks)
    third = 2.0 / 3
    expect = [third / 2, 1.5 * third, 2.5 * third, 2.1, 2.2 + 0.1, 2.2 + 0.3, 2.2 + 0.5, 1 / 6, 0.5, 5 / 6]
    assert [float(k.exit_distance) for k in kicks] == pytest.approx(expect, abs=1e-14)
    assert [float(k.effect_length) for k in kicks] == pytest.approx([third] * 3 + [0.2] + [0.2] * 3 + [1 / 3] * 3, abs=1e-14)
    b1, b2 = seg.elements[1], seg.elements[6]
    for k in kicks[:7]:                                                         # the bend's own tensors: edits and gradients follow
        assert k.bend_length is b1.length and k.bend_angle is b1.angle
    for k in kicks[7:]:
        assert k.bend_length is b2.length and k.bend_angle is b2.angle
    assert kicks[3].effect_length is seg.elements[3].length
    pieces = [e for e in _flat(out) if isinstance(e, ca.Drift) and "_csr_drift_" in e.name]
    assert len(pieces) == 9 and all(type(p) is ca.Drift for p in pieces)
    assert torch.allclose(out.length, seg.length, rtol=0, atol=1e-14)


def test_with_csr_kicks_drift_default_except_for_and_max_distance():
    import cheetah_amd as ca

    seg = _lattice()
    names = lambda s: [e.name for e in _flat(s)]  # noqa: E731
    # the default is today's: no drift kicks, the elements behind the bends untouched
    default = seg.with_csr_kicks(2, num_bins=77, transient=True)
    assert names(default) == names(seg.with_csr_kicks(2, 77, None, True, 0, None))
    assert not any(isinstance(e, CSRDriftKick) for e in _flat(default))
    assert default.elements[5] is seg.elements[2] and default.elements[-1] is seg.elements[-1]
    assert names(default) == ["d0", "b1_csr_0", "b1_csr_kick_0", "b1_csr_1", "b1_csr_kick_1", "d1", "q1", "m1", "d3", "m2", "b2_csr_0",
                              "b2_csr_kick_0", "b2_csr_1", "b2_csr_kick_1", "d4"]
    # a bend in `except_for` ends the run without kicks and starts none
    kept = seg.with_csr_kicks(2, transient=True, drift_kicks=1, except_for=["b2"])
    assert names(kept)[-2:] == ["b2", "d4"] and kept.elements[-1] is seg.elements[-1]
    assert sum(isinstance(e, CSRDriftKick) for e in _flat(kept)) == 3
    # an element that starts beyond max_distance ends the run: d1 starts at 0, q1 at 2.0, d3 at 2.2
    for limit, n in ((2.1, 3), (1.9, 2), (0.0, 2), (5.0, 5)):
        cut = seg.with_csr_kicks(1, drift_kicks=2, max_distance=limit, except_for=["b2"])
        assert sum(isinstance(e, CSRDriftKick) for e in _flat(cut)) == n, limit
    # compared on the largest batch entry
    batched = ca.Segment([ca.Dipole(_t(0.5), angle=_t(0.05), name="b"), ca.Drift(_t([0.5, 1.5]), name="d1"),
                          ca.Drift(_t(1.0), name="d2")])
    assert sum(isinstance(e, CSRDriftKick) for e in batched.with_csr_kicks(1, drift_kicks=1, max_distance=1.0).elements) == 1
    assert sum(isinstance(e, CSRDriftKick) for e in batched.with_csr_kicks(1, drift_kicks=1, max_distance=1.5).elements) == 2
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            seg.with_csr_kicks(2, drift_kicks=bad)
    with pytest.raises(ValueError):
        seg.with_csr_kicks(2, drift_kicks=1, max_distance=-1.0)


def test_with_lsc_kicks_gives_a_csr_drift_kick_no_lsc_kick():
    import cheetah_amd as ca

    seg = ca.Segment([ca.Dipole(_t(0.5), angle=_t(0.05), name="b1"), ca.Drift(_t(1.0), name="d1")])
    seg = seg.with_csr_kicks(1, transient=True, drift_kicks=1).with_lsc_kicks()
    assert [e.name for e in seg.elements] == ["b1_csr_0", "b1_csr_0_lsc_kick", "b1_csr_kick_0", "d1_csr_drift_0",
                                              "d1_csr_drift_0_lsc_kick", "d1_csr_drift_kick_0"]


# ---- the table against 50-digit arithmetic --------------------------------------------------------------------------------------------
TABLE_M = 4096
KAPPAS = (1e-8, 1e-5, 1e-2)
XHATS = (0.0, 1e-4, 1e-2, 1.0, 100.0)


def _exact_differences(kappa, xh, psi64):
    """G(psi_(j+1)) - G(psi_j), j < TABLE_M, at 50 digits: every root polished from its float64 value by Newton steps (the error
    squares with each step: four of them carry 1e-15 far below 1e-50)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    kap, x = mp.mpf(kappa), mp.mpf(xh)
    t = [mp.mpf(0)]
    for i, p0 in enumerate(psi64, start=1):
        c, psi = kap * i, mp.mpf(p0)
        for _ in range(4):
            a = psi + x
            q = psi * (psi + 2 * x) / a
            psi -= (psi ** 3 * (psi + 4 * x) / a - c) / (3 * q * q)
        t.append(psi * psi / 2 + ((x * x * psi / (psi + x) - x * x * mp.log1p(psi / x)) if xh else 0))
    return [t[i + 1] - t[i] for i in range(TABLE_M)]


@pytest.mark.parametrize("xh", XHATS)
@pytest.mark.parametrize("kappa", KAPPAS)
def test_table_differences_against_50_digit_arithmetic(kappa, xh):
    """Every g_j = G(psi_(j+1)) - G(psi_j), j <= 4095, of the float64 restatement within 1e-11 of the largest one. The bound is about
    twice the largest deviation of this scheme measured over these ranges (4.6e-12: the differencing near j = 4000 of entries that
    carry the rounding of a root each). The closed form of G alone must miss the bound at xh = 100, where psi / xh is below 1e-3:
    that is what the series is for."""
    k, x = torch.tensor(kappa, dtype=F64), torch.tensor(xh, dtype=F64)
    i = torch.arange(1, TABLE_M + 1, dtype=F64)
    psi = _root(i * k, x)
    exact = _exact_differences(kappa, xh, psi.tolist())
    largest = max(abs(float(v)) for v in exact)
    worst = {}
    for series in (True, False):
        t = torch.cat([torch.zeros(1, dtype=F64), _G(psi, x, series)])
        g = (t[1:] - t[:-1]).tolist()
        worst[series] = max(abs(float(a - b)) for a, b in zip(g, exact)) / largest
    print(f"kappa {kappa:g}, xh {xh:g}: series switch {worst[True]:.2e}, closed form alone {worst[False]:.2e} of the largest entry")
    assert psi.isfinite().all()
    assert worst[True] <= 1e-11
    if xh == 100.0:
        assert worst[False] > 1e-11


# ---- convergence of the node sums to the continuous formula -----------------------------------------------------------------------
def _node_sums(M, sigma, R, phi, xh):
    """(tau_k, S_k) of a Gaussian line density of unit charge sampled on M nodes over +-5 sigma: D_k = h lambda(tau_k)."""
    tau = torch.linspace(-5 * sigma, 5 * sigma, M, dtype=F64)
    h = float(tau[1] - tau[0])
    D = h * torch.exp(-0.5 * (tau / sigma) ** 2) / (sigma * math.sqrt(2 * math.pi))
    b = _b_table(M, torch.tensor(xh, dtype=F64), torch.tensor(phi, dtype=F64), torch.tensor(24 * h / R, dtype=F64))
    n = torch.arange(M)
    lag = n[None, :] - n[:, None]
    T = torch.where(lag >= 0, b[lag.clamp(min=0)], torch.zeros((), dtype=F64))
    return tau, (T @ D) / (2 * h * h)


def _continuous(tau, sigma, R, phi, xh, n=40001):
    """(4 / R) { int_0^phi lambda'(tau + u(psi)) (du / dpsi) / (psi + 2 xh) dpsi - lambda(tau + u(phi)) / (phi + 2 xh) } by Simpson's
    rule in psi, where the integrand is smooth: du / dpsi = (R / 8) psi^2 (psi + 2 xh)^2 / (psi + xh)^2."""
    lam = lambda s: torch.exp(-0.5 * (s / sigma) ** 2) / (sigma * math.sqrt(2 * math.pi))  # noqa: E731
    psi = torch.linspace(0, phi, n, dtype=F64)[1:]
    u = (R / 24) * psi ** 3 * (psi + 4 * xh) / (psi + xh)
    wgt = (R / 8) * psi ** 2 * (psi + 2 * xh) / (psi + xh) ** 2
    simpson = torch.ones(n, dtype=F64)
    simpson[1:-1:2], simpson[2:-1:2] = 4.0, 2.0
    simpson = (simpson * (phi / (n - 1)) / 3)[1:]                                 # the integrand is 0 at psi = 0
    s = tau[:, None] + u[None, :]
    integral = ((-s / sigma ** 2) * lam(s) * (wgt * simpson)[None, :]).sum(dim=1)
    return (4 / R) * (integral - lam(tau + float(u[-1])) / (phi + 2 * xh))


@pytest.mark.parametrize("ratio", [0.0, 1.0, 20.0])
def test_node_sums_converge_to_the_continuous_formula(ratio):
    """A Gaussian density sampled on the nodes, xh = ratio phi, y = u(phi) / h = 0.3 M: the largest deviation of S_k from the
    quadrature of the continuous formula, relative to the largest |S_k|. Measured with this restatement:
        xh / phi =  0:  M = 200  1.186e-03, M = 400  3.872e-04
        xh / phi =  1:  M = 200  4.864e-05, M = 400  1.257e-05
        xh / phi = 20:  M = 200  2.486e-06, M = 400  6.382e-07
    The scheme is second order in h (a piecewise linear density, every interval integrated exactly), so halving h must divide the
    deviation by 3 or more, and the M = 400 deviation is bounded by twice its measured value."""
    measured_400 = {0.0: 3.872e-04, 1.0: 1.257e-05, 20.0: 6.382e-07}[ratio]
    sigma, R = 1e-4, 8.0
    u_max = 3.0 * sigma                                                          # 0.3 of the grid's 10 sigma
    phi = (24 * u_max * (1 + ratio) / (R * (1 + 4 * ratio))) ** (1 / 3)
    err = {}
    for M in (200, 400):
        tau, S = _node_sums(M, sigma, R, phi, ratio * phi)
        exact = _continuous(tau, sigma, R, phi, ratio * phi)
        err[M] = float((S - exact).abs().max() / exact.abs().max())
    print(f"xh / phi = {ratio:g}: M = 200 {err[200]:.3e}, M = 400 {err[400]:.3e}, ratio {err[200] / err[400]:.2f}")
    assert err[400] <= 2 * measured_400
    assert err[200] / err[400] >= 3
