"""ParticleBeam.bunching_factor without a GPU: the C-ABI entry points are exported and bound, the workspace query works on the
host, and argument errors are raised before any device work (before the "GPU only" error of a CPU beam)."""
import math
import re
import subprocess

import pytest
import torch

NEW_SYMBOLS = ("chx_bunching_workspace_bytes", "chx_bunching", "chx_bunching_bwd")


def _header_constant(name: str) -> int:
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "chx.h")).read()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


def test_bunching_symbols_exported_and_bound():
    import cheetah_amd._lib as L

    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (chx_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.chx_abi_version() == 9


def test_python_constants_are_the_headers():
    import cheetah_amd as ca

    assert ca._ops.BUNCHING_K_MAX == _header_constant("CHX_BUNCHING_K_MAX")
    assert ca._ops.BUNCHING_CHUNK == _header_constant("CHX_BUNCHING_CHUNK")
    assert ca._ops.BUNCHING_K_TILE == _header_constant("CHX_BUNCHING_K_TILE")
    assert callable(ca.ParticleBeam.bunching_factor)


def test_bunching_workspace_on_the_host():
    import cheetah_amd._lib as L

    lib = L.lib()
    k_max = _header_constant("CHX_BUNCHING_K_MAX")
    chunk = _header_constant("CHX_BUNCHING_CHUNK")
    assert lib.chx_bunching_workspace_bytes(1, 10**6, 1024) >= -(-10**6 // chunk) * 1024 * 16
    assert lib.chx_bunching_workspace_bytes(16, 10**5, 256) >= 16 * lib.chx_bunching_workspace_bytes(1, 10**5, 256) - 16 * 512
    assert lib.chx_bunching_workspace_bytes(1, 1, 1) > 0
    assert lib.chx_bunching_workspace_bytes(1, 10**6, k_max) > 0
    assert lib.chx_bunching_workspace_bytes(1, 10**6, 0) == 0
    assert lib.chx_bunching_workspace_bytes(1, 10**6, k_max + 1) == 0
    assert lib.chx_bunching_workspace_bytes(0, 10**6, 8) == 0
    assert lib.chx_bunching_workspace_bytes(1, 0, 8) == 0
    # the largest call: no overflow of size_t
    assert lib.chx_bunching_workspace_bytes(65535, 2**31 - 1, k_max) >= 65535 * (2**31 // chunk) * k_max * 16


def test_invalid_arguments_are_refused_before_any_device_work():
    import ctypes

    import cheetah_amd._lib as L

    lib = L.lib()
    buf = (ctypes.c_double * 64)()                 # host memory standing in for pointers that must never be dereferenced
    p = ctypes.addressof(buf)

    def fwd(x=p, nu=p, B=1, Bx=1, Bw=1, Bq=1, Bnu=1, N=4, K=2):
        return lib.chx_bunching(x, None, None, nu, B, Bx, Bw, Bq, Bnu, N, K, 1, p, p, p, 1 << 20, None)

    def bwd(x=p, nu=p, B=1, Bx=1, Bw=1, Bq=1, Bnu=1, N=4, K=2):
        return lib.chx_bunching_bwd(x, None, None, nu, B, Bx, Bw, Bq, Bnu, N, K, 1, p, p, p, None, None, None, 0, None)

    k_max = _header_constant("CHX_BUNCHING_K_MAX")
    for call in (fwd, bwd):
        assert call(x=None) == -1
        assert call(nu=None) == -1
        assert call(K=0) == -1
        assert call(K=k_max + 1) == -1
        assert call(N=0) == -1
        assert call(B=0) == -1
        assert call(B=3, Bx=2) == -1
        assert call(B=3, Bnu=2) == -1
    assert lib.chx_bunching(None, None, None, None, 1, 1, 1, 1, 1, 10, 4, 0, None, None, None, 0, None) == -1
    assert lib.chx_bunching_bwd(None, None, None, None, 1, 1, 1, 1, 1, 10, 4, 0, None, None, None, None, None, None, 0, None) == -1
    # w / q given with an improper row count
    assert lib.chx_bunching(p, p, None, p, 3, 1, 2, 1, 1, 4, 2, 1, p, p, p, 1 << 20, None) == -1
    assert lib.chx_bunching_bwd(p, None, p, p, 3, 1, 1, 2, 1, 4, 2, 1, p, p, p, None, None, None, 0, None) == -1


@pytest.mark.parametrize("args,kwargs", [
    ((), {}),
    ((1e-6,), {"wavenumbers": 1e6}),
    (([],), {}),
    ((), {"wavenumbers": torch.zeros(3, 0)}),
    ((float("nan"),), {}),
    ((float("inf"),), {}),
    (([1e-6, float("nan")],), {}),
    ((), {"wavenumbers": float("inf")}),
    ((), {"wavenumbers": torch.tensor([1.0, float("nan")])}),
    ((0.0,), {}),
    ((-1e-6,), {}),
    ((torch.tensor([1e-6, 0.0]),), {}),
    (([[1e-6, 2e-6], [1e-6, -2e-6]],), {}),
])
def test_argument_errors_come_before_the_gpu_check(args, kwargs):
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    with pytest.raises(ValueError):
        beam.bunching_factor(*args, **kwargs)


def test_too_many_wavelengths_are_an_argument_error():
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    with pytest.raises(ValueError, match="at most"):
        beam.bunching_factor(torch.full((ca._ops.BUNCHING_K_MAX + 1,), 1e-6))


def test_cpu_beam_is_refused_and_sharded_beam_is_not_implemented():
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    with pytest.raises(RuntimeError, match="GPU only"):
        beam.bunching_factor(1e-6)
    with pytest.raises(RuntimeError, match="GPU only"):
        beam.bunching_factor(wavenumbers=[1e5, 2e5])
    with ca.sharding.particle_sharded():
        with pytest.raises(NotImplementedError, match="particle-sharded"):
            beam.bunching_factor(1e-6)
        with pytest.raises(ValueError):                      # ... and the argument errors still come first
            beam.bunching_factor()


def test_host_values_become_float64_frequencies_without_a_float32_detour():
    from cheetah_amd.particles.bunching import spatial_frequencies

    cpu = torch.device("cpu")
    lam = 1.234567890123e-6
    assert spatial_frequencies(lam, None, cpu).tolist() == [1.0 / lam]
    assert spatial_frequencies([lam, 3e-7], None, cpu).tolist() == [1.0 / lam, 1.0 / 3e-7]
    assert spatial_frequencies(torch.tensor([lam], dtype=torch.float64), None, cpu).tolist() == [1.0 / lam]
    nu = spatial_frequencies(None, [[1e6, 2e6], [3e6, 4e6]], cpu)
    assert nu.dtype == torch.float64 and nu.shape == (2, 2)
    assert nu.tolist() == [[1e6 / (2 * math.pi), 2e6 / (2 * math.pi)], [3e6 / (2 * math.pi), 4e6 / (2 * math.pi)]]
