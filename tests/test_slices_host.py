"""ParticleBeam.slice_statistics without a GPU: the C-ABI entry points are exported and bound, the workspace query works on the
host, and argument errors are raised before any device work (before the "GPU only" error of a CPU beam)."""
import re
import subprocess

import pytest
import torch

NEW_SYMBOLS = ("chx_slice_moments_workspace_bytes", "chx_slice_moments", "chx_slice_moments_bwd")


def test_slice_symbols_exported_and_bound():
    import cheetah_amd._lib as L

    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (chx_[a-z0-9_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in L.SIGNATURES, name
        assert getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert lib.chx_abi_version() == 9


def test_slice_workspace_and_invalid_arguments_on_the_host():
    import cheetah_amd._lib as L

    lib = L.lib()
    assert lib.chx_slice_moments_workspace_bytes(1, 10**6, 100) > 0
    assert lib.chx_slice_moments_workspace_bytes(16, 10**5, 256) >= lib.chx_slice_moments_workspace_bytes(1, 10**5, 256)
    assert lib.chx_slice_moments_workspace_bytes(1, 10**6, 0) == 0
    assert lib.chx_slice_moments_workspace_bytes(1, 10**6, 4097) == 0
    # rejected before any device work: no particles / edges, S out of range, improper broadcast
    assert lib.chx_slice_moments(None, None, None, None, 1, 1, 1, 1, 1, 10, 4, 0, None, None, None, 0, None) == -1
    assert lib.chx_slice_moments_bwd(None, None, None, None, 1, 1, 1, 1, 1, 10, 4, 0, None, None, None, None, None, None, None, 0,
                                     None) == -1


def test_slice_statistics_exists_and_is_exported():
    import cheetah_amd as ca

    assert callable(ca.ParticleBeam.slice_statistics)
    assert ca.BeamSlices is ca.particles.BeamSlices
    assert ca._ops.SLICES_MAX == 2048


@pytest.mark.parametrize("kwargs", [
    {"num_slices": 0},
    {"num_slices": -3},
    {"num_slices": 2.5},
    {"edges": torch.tensor([0.0])},
    {"edges": torch.zeros(3, 1)},
    {"edges": torch.tensor([0.0, 1.0, 2.0]), "tau_range": (0.0, 1.0)},
    {"num_slices": 5000},
])
def test_argument_errors_come_before_the_gpu_check(kwargs):
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    with pytest.raises(ValueError):
        beam.slice_statistics(**kwargs)


def test_cpu_beam_is_refused_and_sharded_beam_is_not_implemented():
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=100)
    with pytest.raises(RuntimeError, match="GPU only"):
        beam.slice_statistics()
    with ca.sharding.particle_sharded():
        with pytest.raises(NotImplementedError, match="particle-sharded"):
            beam.slice_statistics()
