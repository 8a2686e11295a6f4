"""Segment.ring_sensitivity and the `wrt` argument without a GPU: chx_dkd_ring_sensitivity is exported and bound, its invalid
arguments are refused before any launch, the Python argument errors come before the device is asked for, the public names are
there, and csrc/chx_dual2.h with the (seed, knob) parts of csrc/chx_optics_dev.h pass tests/host/dual2_check.hip — a stand-alone
program built for the host with the address and undefined-behaviour sanitizers (nothing is loaded into Python)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
DKD = {"tracking_method": "drift_kick_drift"}


def test_symbol_exported_and_bound():
    import cheetah_amd._lib as L
    import cheetah_amd._ops  # noqa: F401  (adds the signatures)

    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (chx_[a-z0-9_]+)", out))
    for name in ("chx_dkd_ring_sensitivity", "chx_dkd_ring_sensitivity_workspace_bytes"):
        assert name in exported and name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype is L.SIGNATURES[name][0]
    assert lib.chx_abi_version() == 9                                   # an additive export
    header = open(os.path.join(ROOT, "include", "chx.h")).read()
    assert "int chx_dkd_ring_sensitivity(" in header and "size_t chx_dkd_ring_sensitivity_workspace_bytes(" in header
    # 56 doubles per item and the energies behind them (padded to 16 bytes), 17 doubles per knob and item
    assert lib.chx_dkd_ring_sensitivity_workspace_bytes(3, 5) == lib.chx_dkd_ring_jacobian_workspace_bytes(3) + 5 * 3 * 17 * 8
    assert lib.chx_dkd_ring_sensitivity_workspace_bytes(0, 1) == 0 and lib.chx_dkd_ring_sensitivity_workspace_bytes(193, 1) == 0
    assert lib.chx_dkd_ring_sensitivity_workspace_bytes(3, -1) == 0


def test_public_names():
    import cheetah_amd as ca
    from cheetah_amd.particles import optics
    import inspect

    assert ca.RingSensitivity is optics.RingSensitivity and callable(ca.Segment.ring_sensitivity)
    assert list(inspect.signature(ca.Segment.ring_sensitivity).parameters) == ["self", "energy", "wrt", "species", "delta", "guess", "longitudinal",
                                                                                 "num_iterations", "along"]
    for name in ("one_turn_map", "closed_orbit", "ring_optics", "chromaticity"):
        assert inspect.signature(getattr(ca.Segment, name)).parameters["wrt"].default is None
    fields = [f.name for f in optics.RingSensitivity.__dataclass_fields__.values()]
    for name in ("closed", "d_orbit", "d_matrix", "d_orbit_along", "d_matrix_along", "d_tunes", "d_beta"):
        assert name in fields
    assert callable(ca._ops.dkd_ring_sensitivity)


def _call(lib, **change):
    """chx_dkd_ring_sensitivity for a ring of two Drifts and one Quadrupole with every argument valid — the pointers address host
    memory, which no launch may come to read — but those in `change`."""
    E, B, K = 3, 2, 2
    kinds = (ctypes.c_int32 * E)(0, 1, 0)                               # CHX_DKD_DRIFT, CHX_DKD_QUADRUPOLE
    par = [(ctypes.c_double * 5)(0.5, 1.0, 0.0, 0.0, 0.0) for _ in range(E)]
    params = (ctypes.c_void_p * E)(*[ctypes.addressof(p) for p in par])
    steps, fringe = (ctypes.c_int32 * E)(1, 1, 1), (ctypes.c_int32 * E)(3, 3, 3)
    energy = ctypes.c_double(1e8)
    buf = lambda n: (ctypes.c_double * n)()  # noqa: E731
    a = {"kinds": kinds, "params": params, "num_steps": steps, "fringe_at": fringe, "E": E, "energy_in": ctypes.addressof(energy),
         "mass_eV": 510998.95, "n_charges": -1.0, "dtype": 1, "orbit": buf(B * 6), "B": B, "mode": 1,
         "knob_of": (ctypes.c_int32 * 3)(0, 1, 1), "item_of": (ctypes.c_int32 * 3)(1, 0, 2), "slot_of": (ctypes.c_int32 * 3)(1, 0, 0),
         "num_components": 3, "K": K, "record_along": 1, "d_orbit": buf(B * K * 6), "d_image": buf(B * K * 6), "d_matrix": buf(B * K * 36),
         "d_dispersion": buf(B * K * 4), "d_orbit_along": buf(B * K * (E + 1) * 6), "d_matrix_along": buf(B * K * (E + 1) * 36),
         "workspace": None, "workspace_bytes": 0, "stream": None}
    ws = ctypes.create_string_buffer(lib.chx_dkd_ring_sensitivity_workspace_bytes(E, K) + 16)
    a["workspace"] = (ctypes.addressof(ws) + 15) // 16 * 16
    a["workspace_bytes"] = lib.chx_dkd_ring_sensitivity_workspace_bytes(E, K)
    a.update(change)
    return lib.chx_dkd_ring_sensitivity(*a.values()), a


def test_invalid_arguments_are_refused_before_any_launch():
    import cheetah_amd._lib as L
    import cheetah_amd._ops as ops

    lib = L.lib()
    INVALID, DTYPE = -1, -2
    f64 = ops.dtype_code(F64)
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    cases = {
        "kinds": None, "params": None, "num_steps": None, "fringe_at": None, "energy_in": None, "orbit": None, "knob_of": None, "item_of": None,
        "slot_of": None, "d_orbit": None, "d_image": None, "d_matrix": None, "d_dispersion": None, "d_orbit_along": None, "d_matrix_along": None,
        "workspace": None,
    }
    for name, value in cases.items():
        assert _call(lib, dtype=f64, **{name: value})[0] == INVALID, name
    for change in ({"K": -1}, {"B": 0}, {"E": 0}, {"E": 193}, {"mode": 3}, {"mode": -1}, {"record_along": 2}, {"num_components": -1},
                   {"knob_of": i32(0, 2, 1)}, {"knob_of": i32(0, -1, 1)}, {"item_of": i32(1, 3, 2)}, {"item_of": i32(-1, 0, 2)},
                   {"slot_of": i32(5, 0, 0)},            # a Quadrupole has five parameters
                   {"slot_of": i32(1, 1, 0)},            # a Drift has one
                   {"slot_of": i32(1, -1, 0)},
                   {"knob_of": i32(1, 1, 1), "item_of": i32(0, 0, 2), "slot_of": i32(0, 0, 0)},      # a component named twice
                   {"kinds": i32(0, 7, 0)}, {"num_steps": i32(1, 0, 1)}, {"fringe_at": i32(3, 4, 3)}, {"workspace_bytes": 16}):
        assert _call(lib, dtype=f64, **change)[0] == INVALID, change
    _, a = _call(lib, dtype=f64, K=-1)
    assert _call(lib, dtype=f64, workspace=a["workspace"] + 8)[0] == INVALID          # not 16-byte aligned
    assert _call(lib, dtype=7)[0] == DTYPE
    # K = 0 is a valid call that launches nothing
    assert _call(lib, dtype=f64, K=0, num_components=0)[0] == 0


def _cpu_ring(**grad):
    import cheetah_amd as ca

    kw = {"dtype": F64}
    k1 = torch.tensor(3.0, **kw, requires_grad=grad.get("k1", False))
    k2 = torch.tensor(-3.0, **kw, requires_grad=grad.get("k2", False))
    els = [ca.Quadrupole(torch.tensor(0.2, **kw), k1=k1, **DKD, **kw), ca.Drift(torch.tensor(1.0, **kw), **DKD, **kw),
           ca.Quadrupole(torch.tensor(0.2, **kw), k1=k2, **DKD, **kw), ca.Drift(torch.tensor(1.0, **kw), **DKD, **kw)]
    return ca.Segment(els), k1, k2


def test_python_argument_errors_come_before_the_device_check():
    energy = torch.tensor(1e8, dtype=F64)
    seg, k1, k2 = _cpu_ring()
    stranger = torch.tensor(3.0, dtype=F64)                               # the value of k1, another tensor
    calls = (lambda w: seg.ring_optics(energy, wrt=w), lambda w: seg.closed_orbit(energy, wrt=w), lambda w: seg.chromaticity(energy, wrt=w),
             lambda w: seg.one_turn_map(torch.zeros(1, 6, dtype=F64), energy, wrt=w), lambda w: seg.ring_sensitivity(energy, w))
    for call in calls:
        with pytest.raises(ValueError, match=r"wrt\[1\] is not a setting"):
            call([k1, stranger])
        with pytest.raises(ValueError, match=r"wrt\[1\] is the tensor of wrt\[0\] again"):
            call([k1, k1])
        with pytest.raises(ValueError, match="'all'"):
            call("every")
    with pytest.raises(ValueError, match="wrt must be"):
        seg.ring_sensitivity(energy, None)
    seg, k1, k2 = _cpu_ring(k1=True, k2=True)
    for call in calls[:4]:
        with pytest.raises(ValueError, match="requires grad"):
            call(None)                                                    # as before
        with pytest.raises(ValueError, match="requires grad"):
            call([k1])                                                    # k2 requires grad and is not named
    with pytest.raises(ValueError, match="requires grad"):
        seg.ring_sensitivity(energy, [k2])
    # with every trainable setting named, the next refusal is the device's: there is no CPU fallback
    for w in ([k1, k2], "all"):
        with pytest.raises(RuntimeError, match="GPU only"):
            seg.ring_optics(energy, wrt=w)


def test_knobs_are_found_by_identity():
    import cheetah_amd as ca

    kw = {"dtype": F64}
    shared, mis = torch.tensor(3.0, **kw), torch.tensor([1e-3, -1e-3], **kw)
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    els = [ca.Quadrupole(t(0.2), k1=shared, **DKD, **kw), ca.Drift(t(1.0), **DKD, **kw), ca.Marker(**kw),
           ca.Sextupole(t(0.1), k2=t(5.0), misalignment=mis, **DKD, **kw), ca.Quadrupole(t(0.2), k1=shared, **DKD, **kw)]
    seg = ca.Segment(els)
    wrt, layout, components, K = seg._ring_knobs("test", seg._plan(), [mis, shared, els[1].length])
    assert K == 4 and layout == [(0, 2, False), (2, 1, True), (3, 1, True)]
    # (knob, item, slot): the Marker is no item; k1 is slot 1 of a Quadrupole, the misalignment slots 3 and 4 of a Sextupole
    assert sorted(components) == [(0, 2, 3), (1, 2, 4), (2, 0, 1), (2, 3, 1), (3, 1, 0)]
    shared.requires_grad_(True)
    wrt, layout, components, K = seg._ring_knobs("test", seg._plan(), "all")
    assert len(wrt) == 1 and wrt[0] is shared and K == 1 and sorted(components) == [(0, 0, 1), (0, 3, 1)]


def test_backward_contracts_the_tangents():
    """`RingValues` on CPU tensors: the gradient of a sum of its outputs is the einsum of the cotangents with the tangents, a
    two-entry setting gets both of its knobs."""
    from cheetah_amd.particles.optics import attach_gradients

    g = torch.Generator().manual_seed(1)
    B, K, E1 = 3, 3, 4
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    out = {"orbit": r(B, 6), "image": r(B, 6), "matrix": r(B, 6, 6), "residual": r(B).abs(), "dispersion": r(B, 4), "orbit_along": r(B, E1, 6),
           "matrix_along": r(B, E1, 6, 6)}
    sens = {"d_orbit": r(B, K, 6), "d_image": r(B, K, 6), "d_matrix": r(B, K, 6, 6), "d_dispersion": r(B, K, 4), "d_orbit_along": r(B, K, E1, 6),
            "d_matrix_along": r(B, K, E1, 6, 6)}
    a, b = torch.tensor(1.0, dtype=F64, requires_grad=True), torch.tensor([0.0, 0.0], dtype=torch.float32, requires_grad=True)
    res = attach_gradients(dict(out), sens, [(0, 1, True), (1, 2, False)], [a, b], 4)
    for name in ("orbit", "image", "matrix", "dispersion", "orbit_along", "matrix_along"):
        assert torch.equal(res[name].detach(), out[name]) and res[name].requires_grad
    assert torch.equal(res["residual"].detach(), out["residual"]) and res["residual"].requires_grad
    w = {name: r(*out[name].shape) for name in ("orbit", "matrix", "dispersion", "matrix_along")}
    sum((w[n] * res[n]).sum() for n in w).backward()
    want = sum(torch.einsum("b...,bk...->k", w[n], sens["d_" + n]) for n in w)
    assert a.grad.shape == () and b.grad.shape == (2,) and b.grad.dtype == torch.float32
    assert abs(float(a.grad) - float(want[0])) <= 1e-13 * float(want.abs().max())
    assert torch.allclose(b.grad.double(), want[1:], rtol=1e-6)


def test_a_lost_seed_poisons_a_gradient_only_through_a_cotangent():
    from cheetah_amd.particles.optics import attach_gradients

    g = torch.Generator().manual_seed(2)
    B, K = 4, 2
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731
    out = {"orbit": r(B, 6), "image": r(B, 6), "matrix": r(B, 6, 6), "residual": r(B).abs(), "dispersion": r(B, 4)}
    sens = {"d_orbit": r(B, K, 6), "d_image": r(B, K, 6), "d_matrix": r(B, K, 6, 6), "d_dispersion": r(B, K, 4)}
    for t in list(out.values()) + list(sens.values()):
        t[2] = float("nan")                                               # seed 2 failed
    a, b = (torch.tensor(1.0, dtype=F64, requires_grad=True) for _ in range(2))
    res = attach_gradients(dict(out), sens, [(0, 1, True), (1, 1, True)], [a, b], 4)
    live = torch.tensor([0, 1, 3])
    res["matrix"][live].sum().backward(retain_graph=True)
    want = sens["d_matrix"][live].sum((0, 2, 3))
    assert torch.isfinite(a.grad) and torch.allclose(torch.stack([a.grad, b.grad]), want, rtol=1e-13)
    a.grad = b.grad = None
    res["matrix"].nansum().backward()                                     # (nansum hands seed 2 a cotangent of zero as well)
    assert torch.isfinite(a.grad)
    a.grad = b.grad = None
    res2 = attach_gradients(dict(out), sens, [(0, 1, True), (1, 1, True)], [a, b], 4)
    res2["orbit"].sum().backward()
    assert torch.isnan(a.grad) and torch.isnan(b.grad)                    # the lost seed entered the loss


def test_wrt_is_read_once():
    energy = torch.tensor(1e8, dtype=F64)
    seg, k1, k2 = _cpu_ring()
    stranger = torch.tensor(3.0, dtype=F64)
    with pytest.raises(ValueError, match=r"wrt\[1\] is not a setting"):
        seg.ring_optics(energy, wrt=(t for t in (k1, stranger)))          # a generator is validated like a list
    with pytest.raises(ValueError, match="wrt must be"):
        seg.ring_optics(energy, wrt=3)
    with pytest.raises(RuntimeError, match="GPU only"):
        seg.ring_optics(energy, wrt=(t for t in (k1, k2)))


def test_dual2_and_lane_maps_on_the_host_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "dual2_check"
    subprocess.run([hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cheetah_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "dual2_check.hip")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    for part in ("unary functions", "operators, atan2, cst, val, tan_of", "composition", "named closed forms", "lane maps", "orbit sensitivity system"):
        assert f"{part}: ok" in run.stdout
