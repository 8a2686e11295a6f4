"""Quiet-start beams and the seeded density modulation without a GPU: exports and C-ABI symbols, rejected arguments of
`chx_quiet_sequence` and the density entry points, the workspace query, known values of the Halton restatement that the GPU tests
compare the kernel with, and the ValueErrors of `quiet_start` / `sequence_offset` and of `with_density_modulation`, all raised
before any device work."""
import ctypes
import inspect
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.quiet_ref import halton, modulate_tau, modulation_residual, radical_inverse

NEW_SYMBOLS = ("chx_quiet_sequence", "chx_density_workspace_bytes", "chx_density_modulate", "chx_density_modulate_bwd")
F64 = torch.float64


def test_exported_from_the_ops_module_and_the_beam():
    import cheetah_amd as ca

    assert callable(ca._ops.quiet_sequence) and callable(ca._ops.density_modulate) and callable(ca._ops.density_factors)
    assert callable(ca.ParticleBeam.with_density_modulation)
    for factory in (ca.ParticleBeam.from_distribution, ca.ParticleBeam.from_parameters, ca.ParticleBeam.from_twiss):
        p = inspect.signature(factory).parameters
        assert p["quiet_start"].default is False and p["sequence_offset"].default == 0


def test_new_symbols_exported_and_bound():
    import cheetah_amd._lib as L

    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (chx_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.chx_abi_version() == 9


def test_quiet_sequence_rejects_invalid_arguments_on_the_host():
    import cheetah_amd._lib as L

    lib = L.lib()
    out = torch.zeros(16, 8, dtype=F64)
    good = dict(bases=(5, 7, 11, 13, 2, 3), D=None, N=16, offset=0, normal=1, dtype=1, out=out.data_ptr())

    def call(**kw):
        a = {**good, **kw}
        b = a["bases"]
        arr = None if b is None else ctypes.cast((ctypes.c_int * len(b))(*b), ctypes.c_void_p)
        D = a["D"] if a["D"] is not None else len(b)
        return lib.chx_quiet_sequence(arr, D, a["N"], a["offset"], a["normal"], a["dtype"], a["out"], None)

    bad = [{"N": 0}, {"N": -5}, {"bases": (), "D": 0}, {"bases": (2, 3, 5, 7, 11, 13, 17, 19, 2), "D": 9}, {"offset": -1},
           {"offset": 2**40}, {"offset": 2**40 - 16}, {"offset": 2**40 - 1, "N": 1}, {"N": 2**40}, {"offset": 2**62, "N": 2**62},
           {"bases": None, "D": 6}, {"out": None}, {"bases": (2, 4)}, {"bases": (2, 23)}, {"bases": (2, 1)}, {"bases": (3, 3)},
           {"bases": (0,)}, {"bases": (-2,)}]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(dtype=2) == -2 and call(dtype=-1) == -2


def test_density_workspace_and_invalid_arguments_on_the_host():
    import cheetah_amd._lib as L

    lib = L.lib()
    ws1 = lib.chx_density_workspace_bytes(1, 10**6)
    assert ws1 > 0
    assert lib.chx_density_workspace_bytes(4, 10**6) == 4 * ws1
    assert lib.chx_density_workspace_bytes(1, 257) == 2 * lib.chx_density_workspace_bytes(1, 256) == 2 * 24 * 8
    for B, N in [(0, 10**6), (1, 0), (65536, 10), (1, 2**32), (-1, 10)]:
        assert lib.chx_density_workspace_bytes(B, N) == 0, (B, N)
    x = torch.zeros(10, 7, dtype=F64)
    s = torch.full((2,), 0.1, dtype=F64)
    d = torch.zeros(24, dtype=F64)
    ws = torch.zeros(24 * 8, dtype=torch.uint8)
    good = dict(x=x.data_ptr(), s=[s.data_ptr()] * 3, K=2, B=1, Bx=1, rows=[1] * 3, N=10, dtype=1, out=x.data_ptr(), dx=x.data_ptr(),
                dr=d.data_ptr(), ws=ws.data_ptr(), ws_bytes=24 * 8)

    def fwd(**kw):
        a = {**good, **kw}
        return lib.chx_density_modulate(a["x"], *a["s"], a["K"], a["B"], a["Bx"], *a["rows"], a["N"], a["dtype"], a["out"], None)

    def bwd(**kw):
        a = {**good, **kw}
        return lib.chx_density_modulate_bwd(a["x"], *a["s"], a["K"], a["B"], a["Bx"], *a["rows"], a["N"], a["dtype"], x.data_ptr(),
                                            a["dx"], a["dr"], a["ws"], a["ws_bytes"], None)

    def without(i):
        v = list(good["s"])
        v[i] = None
        return v

    def rows(i, n):
        r = list(good["rows"])
        r[i] = n
        return r

    bad_both = [{"N": 0}, {"B": 0}, {"B": 65536}, {"K": 0}, {"K": 9}, {"x": None}, {"Bx": 2}]
    bad_both += [{"s": without(i)} for i in range(3)] + [{"rows": rows(i, 2)} for i in range(3)]
    for bad in bad_both + [{"out": None}]:
        assert fwd(**bad) == -1, bad
    for bad in bad_both + [{"dx": None}, {"dr": None}]:
        assert bwd(**bad) == -1, bad
    # a dtype that is not a beam's, a misaligned output, a workspace that is missing or too small: their own codes
    assert fwd(dtype=2) == bwd(dtype=2) == -2
    assert fwd(out=x.data_ptr() + 8) == bwd(dx=x.data_ptr() + 8) == -3
    assert bwd(ws=None) == bwd(ws_bytes=24 * 8 - 1) == -5


def test_the_halton_restatement_gives_the_known_values():
    h = halton(3, (2, 3))
    assert h[:, 0].tolist() == [0.5, 0.25, 0.75]
    assert h[:, 1].tolist() == [1 / 3, 2 / 3, 1 / 9]
    assert radical_inverse(np.array([5, 6, 7, 8], dtype=np.uint64), 2).tolist() == [0.625, 0.375, 0.875, 0.0625]
    assert radical_inverse(np.array([2**39], dtype=np.uint64), 2)[0] == 2.0**-40
    assert radical_inverse(np.array([19, 20], dtype=np.uint64), 19).tolist() == [1 / 361, 20 / 361]
    top = halton(16, (2, 3, 5, 7, 11, 13, 17, 19), offset=2**40 - 17)               # the last indices of the range
    assert top.shape == (16, 8) and ((top > 0) & (top < 1)).all()
    assert np.array_equal(halton(10, (2, 3), offset=7), halton(17, (2, 3))[7:])


def test_the_modulation_restatement_solves_its_equation():
    """Sum |A| = 0.95 in three modes over a few hundred wavelengths: the residual of the defining equation is rounding, the map is
    monotone, and a zero amplitude is the identity."""
    g = torch.Generator().manual_seed(0)
    tau = torch.randn(20_000, generator=g, dtype=F64) * 1e-4
    A, lam, phi = (torch.tensor(v, dtype=F64) for v in ([0.5, -0.3, 0.15], [5e-6, 1.43e-5, 2.2e-6], [0.7, -2.0, 3.0]))
    out = modulate_tau(tau, A, lam, phi)
    assert float(modulation_residual(out, tau, A, lam, phi).max()) < 1e-12
    order = torch.argsort(tau)
    assert bool((torch.diff(out[order]) >= 0).all())
    assert torch.equal(modulate_tau(tau, torch.zeros(3, dtype=F64), lam, phi), tau)


@pytest.mark.parametrize("kw", [
    {"sequence_offset": -1}, {"sequence_offset": 1.0}, {"sequence_offset": 0.5}, {"sequence_offset": True},
    {"sequence_offset": 2**40}, {"sequence_offset": 2**40 - 1000}, {"sequence_offset": torch.tensor(3.0)},
])
def test_sequence_offset_value_errors_come_before_any_device_work(kw):
    import cheetah_amd as ca

    cov = torch.eye(6, dtype=F64) * 1e-8
    with pytest.raises(ValueError):
        ca.ParticleBeam.from_distribution(torch.zeros(6, dtype=F64), cov, 1000, dtype=F64, quiet_start=True, **kw)
    with pytest.raises(ValueError):
        ca.ParticleBeam.from_parameters(num_particles=1000, dtype=F64, quiet_start=True, **kw)
    with pytest.raises(ValueError):
        ca.ParticleBeam.from_twiss(num_particles=1000, beta_x=torch.tensor(1.0, dtype=F64), beta_y=torch.tensor(1.0, dtype=F64),
                                   dtype=F64, quiet_start=True, **kw)


def test_quiet_sequence_value_errors_and_the_device_error():
    import cheetah_amd as ca

    q = ca._ops.quiet_sequence
    for args, kw in [((0, (2, 3)), {}), ((10, ()), {}), ((10, (2, 3, 5, 7, 11, 13, 17, 19, 23)), {}), ((10, (2, 4)), {}),
                     ((10, (2, 2)), {}), ((10, (2, 3)), {"offset": -1}), ((10, (2, 3)), {"offset": 2**40 - 10}),
                     ((10.0, (2, 3)), {})]:
        with pytest.raises(ValueError):
            q(*args, **kw)
    with pytest.raises(TypeError):
        q(10, (2, 3), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU only"):      # there is no CPU generator to fall back to
        q(10, (2, 3), device="cpu")


def _cpu_beam():
    import cheetah_amd as ca

    torch.manual_seed(0)
    return ca.ParticleBeam.from_parameters(num_particles=100, dtype=F64)


@pytest.mark.parametrize("kw", [
    {"amplitudes": 1.0}, {"amplitudes": [0.5, 0.5]}, {"amplitudes": [0.6, -0.6]}, {"amplitudes": -1.2},
    {"amplitudes": 0.4, "wavelengths": [1e-6, 2e-6, 3e-6]},                       # one value stands for all three modes: 1.2
    {"amplitudes": torch.tensor([[0.1, 0.1], [0.5, 0.5]], dtype=F64)},
    {"wavelengths": 0.0}, {"wavelengths": -1e-6}, {"wavelengths": [1e-6, 0.0], "amplitudes": [0.1, 0.1]},
    {"amplitudes": float("nan")}, {"amplitudes": float("inf")}, {"wavelengths": float("inf")}, {"wavelengths": float("nan")},
    {"phases": float("nan")}, {"phases": [0.0, float("inf")]},
    {"wavelengths": [1e-6] * 9, "amplitudes": [0.01] * 9}, {"wavelengths": [1e-6] * 9},
    {"wavelengths": [1e-6, 2e-6], "amplitudes": [0.1, 0.1, 0.1]}, {"wavelengths": [1e-6, 2e-6], "phases": [0.0, 0.1, 0.2]},
    {"wavelengths": []}, {"amplitudes": None}, {"wavelengths": None},
])
def test_density_modulation_value_errors_come_before_any_device_work(kw):
    args = {"wavelengths": [1e-6, 2e-6], "amplitudes": 0.1, "phases": 0.0, **kw}
    with pytest.raises(ValueError):
        _cpu_beam().with_density_modulation(**args)


def test_density_modulation_needs_the_device():
    with pytest.raises(RuntimeError, match="GPU only"):
        _cpu_beam().with_density_modulation(1e-6, 0.1)
