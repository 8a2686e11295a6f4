"""The bunching factor of a ParticleBeam (`ParticleBeam.bunching_factor`): b(k) = sum a exp(-i k tau) / sum a at chosen
wavelengths, from one `chx_bunching` call."""
from __future__ import annotations

import math
import numbers

import torch

from .. import _ops
from ..sharding import _ACTIVE_GROUP as _SHARDING_STACK


def _on_host(v) -> bool:
    return not (isinstance(v, torch.Tensor) and v.is_cuda)


def spatial_frequencies(wavelengths, wavenumbers, device) -> torch.Tensor:
    """nu = 1 / lambda = k / (2 pi) (…, K) float64 on `device`, with the argument errors of `bunching_factor` raised before any
    device work. Host-side values (floats, sequences, CPU tensors) are checked; device tensors are used as given (a check
    would synchronise)."""
    if (wavelengths is None) == (wavenumbers is None):
        raise ValueError("bunching_factor takes exactly one of `wavelengths` and `wavenumbers`")
    given, name = (wavelengths, "wavelengths") if wavenumbers is None else (wavenumbers, "wavenumbers")
    scalar = isinstance(given, numbers.Real) and not isinstance(given, bool)
    host = _on_host(given)
    # (a Python number or sequence straight to float64: torch's default dtype would round it to float32 first)
    v = (given if isinstance(given, torch.Tensor) else torch.as_tensor(given, dtype=torch.float64)).detach().to(torch.float64)
    if v.dim() == 0:
        v = v.reshape(1)
    if v.shape[-1] == 0:
        raise ValueError(f"{name} must hold at least one value, got shape {tuple(v.shape)}")
    if host and not bool(torch.isfinite(v).all()):
        raise ValueError(f"{name} must be finite")
    if host and wavenumbers is None and not bool((v > 0).all()):
        raise ValueError("wavelengths must be > 0")
    K = v.shape[-1]
    if K > _ops.BUNCHING_K_MAX:
        raise ValueError(f"at most {_ops.BUNCHING_K_MAX} wavelengths per call are supported, got {K}")
    nu = 1.0 / v if wavenumbers is None else v / (2.0 * math.pi)
    if device.type != "cuda" or nu.is_cuda:
        return nu
    if scalar:                               # a fill on the device, not a host-to-device copy
        return torch.full((1,), float(nu[0]), dtype=torch.float64, device=device)
    return nu.to(device, non_blocking=True)


def bunching_factor(beam, wavelengths=None, wavenumbers=None) -> torch.Tensor:
    p, w, q = beam.particles, beam.survival_probabilities, beam.particle_charges
    nu = spatial_frequencies(wavelengths, wavenumbers, p.device)
    if _SHARDING_STACK:
        raise NotImplementedError("bunching_factor of a particle-sharded beam (inside sharding.particle_sharded) is not implemented: "
                                  "summing F and Q over the ranks is not supported yet; gather the particles on one rank first")
    _ops.require_device(p)
    F, Q = _ops.bunching(p, w, q, nu)
    return F / Q.unsqueeze(-1)
