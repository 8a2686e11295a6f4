"""Segment.radiation_integrals without a GPU: chx_dkd_ring_radiation is exported and bound, its invalid arguments are refused before
any launch, the Python refusals come before the device is asked for, the public names are there, and csrc/chx_radiation_dev.h passes
tests/host/radiation_check.hip — a stand-alone program built for the host with the address and undefined-behaviour sanitizers
(nothing is loaded into Python)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
DKD = {"tracking_method": "drift_kick_drift"}


def test_symbols_exported_and_bound():
    import cheetah_amd._lib as L
    import cheetah_amd._ops  # noqa: F401  (adds the signatures)

    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (chx_[a-z0-9_]+)", out))
    for name in ("chx_dkd_ring_radiation", "chx_dkd_ring_radiation_workspace_bytes"):
        assert name in exported and name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype is L.SIGNATURES[name][0]
    assert lib.chx_abi_version() == 9                                   # an additive export
    header = open(os.path.join(ROOT, "include", "chx.h")).read()
    assert "int chx_dkd_ring_radiation(" in header and "size_t chx_dkd_ring_radiation_workspace_bytes(" in header
    for text in ("integrals[B][7] = (I1, I2, I3, I4x, I4y, I5x, I5y)", "8-point Gauss-Legendre", "theta^16 / 16!"):
        assert text in header
    assert "chx_dkd_ring_radiation" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the constants of one turn: what chx_dkd_ring_jacobian takes
    assert lib.chx_dkd_ring_radiation_workspace_bytes(3) == lib.chx_dkd_ring_jacobian_workspace_bytes(3) > 0
    assert lib.chx_dkd_ring_radiation_workspace_bytes(192) > 0
    assert lib.chx_dkd_ring_radiation_workspace_bytes(0) == 0 and lib.chx_dkd_ring_radiation_workspace_bytes(193) == 0
    assert lib.chx_dkd_ring_radiation_workspace_bytes(-1) == 0


def test_public_names():
    import cheetah_amd as ca
    from cheetah_amd.particles import optics

    assert ca.RadiationIntegrals is optics.RadiationIntegrals and callable(ca.Segment.radiation_integrals)
    sig = inspect.signature(ca.Segment.radiation_integrals)
    assert list(sig.parameters) == ["self", "energy", "species", "delta", "guess", "num_iterations", "along"]
    assert sig.parameters["num_iterations"].default == 10 and sig.parameters["along"].default is False
    fields = [f.name for f in optics.RadiationIntegrals.__dataclass_fields__.values()]
    assert fields == ["I1", "I2", "I3", "I4", "I5", "integrals_along", "closed", "energy_loss", "partition", "damping_turns", "damping_time",
                      "emittance", "energy_spread", "circumference"]
    assert callable(ca._ops.dkd_ring_radiation)
    doc = ca.Segment.radiation_integrals.__doc__
    for text in ("Gauss-Legendre", "theta^16 / 16!", "1e-10 at theta = pi / 2", "closed.slip beta0^2 + C / gamma0^2"):
        assert text in doc


def test_derived_quantities_on_cpu_tensors():
    """`radiation_integrals_from` is plain torch: electrons at 1 GeV on one bending radius of 1 m (I2 = 2 pi, I3 = 2 pi, I4 = 0)."""
    import math

    from cheetah_amd.particles.optics import radiation_constants, radiation_integrals_from

    r_c, c_q = radiation_constants(510998.95069, -1.0)
    assert abs(c_q - 3.8319e-13) < 0.5e-17 and abs(r_c - 2.8179403205e-15) < 1e-27
    two_pi = 2 * math.pi
    integrals = torch.tensor([[two_pi, two_pi, two_pi, 0.0, 0.0, two_pi, 0.0]], dtype=F64)
    rad = radiation_integrals_from(None, integrals, None, torch.tensor(1e9, dtype=F64), 510998.95069, -1.0, torch.tensor(two_pi, dtype=F64))
    assert abs(float(rad.energy_loss) - 88.46e3) < 5.0                   # 88.46 keV to 4 digits
    assert torch.equal(rad.partition, torch.tensor([[1.0, 1.0, 2.0]], dtype=F64))
    gamma = 1e9 / 510998.95069
    assert abs(float(rad.emittance[0, 0]) / (c_q * gamma ** 2) - 1) < 1e-14 and float(rad.emittance[0, 1]) == 0.0
    assert abs(float(rad.energy_spread) / math.sqrt(c_q * gamma ** 2 / 2) - 1) < 1e-14
    turns = 2e9 / float(rad.energy_loss)
    assert torch.allclose(rad.damping_turns, torch.tensor([[turns, turns, turns / 2]], dtype=F64), rtol=1e-14)
    beta = math.sqrt(1 - 1 / gamma ** 2)
    assert torch.allclose(rad.damping_time, rad.damping_turns * two_pi / (beta * 299792458.0), rtol=1e-14)


def _call(lib, **change):
    """chx_dkd_ring_radiation for a ring of a Drift, a Dipole and a Drift with every argument valid — the pointers address host
    memory, which no launch may come to read — but those in `change`."""
    E, B = 3, 2
    kinds = (ctypes.c_int32 * E)(0, 2, 0)                               # CHX_DKD_DRIFT, CHX_DKD_DIPOLE
    par = [(ctypes.c_double * 9)(0.5, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0) for _ in range(E)]
    params = (ctypes.c_void_p * E)(*[ctypes.addressof(p) for p in par])
    steps, fringe = (ctypes.c_int32 * E)(1, 1, 1), (ctypes.c_int32 * E)(3, 3, 3)
    energy = ctypes.c_double(1e8)
    buf = lambda n: (ctypes.c_double * n)()  # noqa: E731
    a = {"kinds": kinds, "params": params, "num_steps": steps, "fringe_at": fringe, "E": E, "energy_in": ctypes.addressof(energy),
         "mass_eV": 510998.95, "n_charges": -1.0, "dtype": 1, "orbit": buf(B * 6), "beta0": buf(B * 2), "alpha0": buf(B * 2), "eta0": buf(B * 4),
         "B": B, "integrals": buf(B * 7), "along": buf(B * E * 7), "workspace": None, "workspace_bytes": 0, "stream": None}
    ws = ctypes.create_string_buffer(lib.chx_dkd_ring_radiation_workspace_bytes(E) + 16)
    a["workspace"] = (ctypes.addressof(ws) + 15) // 16 * 16
    a["workspace_bytes"] = lib.chx_dkd_ring_radiation_workspace_bytes(E)
    same = change.pop("same", {})                                      # {argument: the argument whose buffer it gets (+ bytes)}
    a.update(change)
    for name, (other, skip) in same.items():
        target = a[other]
        a[name] = (target if isinstance(target, int) else ctypes.addressof(target)) + skip
    return lib.chx_dkd_ring_radiation(*a.values()), a, (par, energy, ws)


def test_invalid_arguments_are_refused_before_any_launch():
    import cheetah_amd._lib as L
    import cheetah_amd._ops as ops

    lib = L.lib()
    INVALID, DTYPE = -1, -2
    f64 = ops.dtype_code(F64)
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    assert lib.chx_dkd_ring_radiation.argtypes is not None
    for name in ("kinds", "params", "num_steps", "fringe_at", "energy_in", "orbit", "beta0", "alpha0", "eta0", "integrals", "workspace"):
        assert _call(lib, dtype=f64, **{name: None})[0] == INVALID, name
    for change in ({"B": 0}, {"B": -3}, {"E": 0}, {"E": 193}, {"kinds": i32(0, 7, 0)}, {"kinds": i32(0, 3, 0)},     # (3: a TDC is no ring item)
                   {"num_steps": i32(1, 0, 1)}, {"fringe_at": i32(3, 4, 3)}, {"workspace_bytes": 16}):
        assert _call(lib, dtype=f64, **change)[0] == INVALID, change
    assert _call(lib, dtype=f64, same={"workspace": ("workspace", 8)})[0] == INVALID          # not 16-byte aligned
    # aliased buffers, all inside one call's own arguments: an output on an input, on another output, overlapping by its last
    # double, on the workspace; an input inside the workspace
    for same in ({"integrals": ("orbit", 0)}, {"along": ("eta0", 0)}, {"along": ("integrals", 0)}, {"integrals": ("along", 8 * (2 * 3 * 7 - 1))},
                 {"beta0": ("integrals", 8 * 13)}, {"alpha0": ("along", 8 * 41)}, {"integrals": ("workspace", 0)}, {"orbit": ("workspace", 64)},
                 {"along": ("orbit", 8 * 11)}):
        assert _call(lib, dtype=f64, same=same)[0] == INVALID, same
    assert _call(lib, dtype=7)[0] == DTYPE


def _cpu_ring(grad=False, linear=False):
    import cheetah_amd as ca

    kw = {"dtype": F64}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    angle = torch.tensor(0.3, **kw, requires_grad=grad)
    els = [ca.Quadrupole(t(0.2), k1=t(3.0), **DKD, **kw), ca.Drift(t(1.0), **DKD, **kw), ca.Dipole(t(0.5), angle=angle, **DKD, **kw),
           ca.Quadrupole(t(0.2), k1=t(-3.0), **DKD, **kw), ca.Drift(t(1.0), **({} if linear else DKD), **kw)]
    return ca.Segment(els)


def test_python_refusals_come_before_the_device_check():
    energy = torch.tensor(1e8, dtype=F64)
    with pytest.raises(ValueError, match="radiation_integrals: .*requires grad"):
        _cpu_ring(grad=True).radiation_integrals(energy)
    with pytest.raises(ValueError, match="radiation_integrals has no autograd"):
        _cpu_ring().radiation_integrals(torch.tensor(1e8, dtype=F64, requires_grad=True))
    with pytest.raises(ValueError, match="radiation_integrals has no autograd"):
        _cpu_ring().radiation_integrals(energy, delta=torch.tensor([1e-3], dtype=F64, requires_grad=True))
    with pytest.raises(ValueError, match="radiation_integrals: .*linear elements"):
        _cpu_ring(linear=True).radiation_integrals(energy, along=True)
    with pytest.raises(ValueError, match="num_iterations"):
        _cpu_ring().radiation_integrals(energy, num_iterations=0)
    with pytest.raises(TypeError):
        _cpu_ring().radiation_integrals(energy, longitudinal=True)      # the integrals are defined on the 4-D optics
    # a ring that qualifies: the next refusal is the device's, there is no CPU fallback
    with pytest.raises(RuntimeError, match="GPU only"):
        _cpu_ring().radiation_integrals(energy)


def test_node_algebra_on_the_host_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "radiation_check"
    subprocess.run([hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cheetah_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "radiation_check.hip")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    for part in ("gauss-legendre table", "lane terms", "point inside a sector bend", "bend contribution"):
        assert f"{part}: ok" in run.stdout
