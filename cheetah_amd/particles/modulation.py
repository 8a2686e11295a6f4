"""The seeded density modulation of a ParticleBeam (`ParticleBeam.with_density_modulation`): the longitudinal density times
1 + sum_m A_m cos(2 pi tau / lambda_m + phi_m), from one `chx_density_modulate` call."""
from __future__ import annotations

import numbers

import torch

from .. import _ops


def _on_host(v) -> bool:
    return not (isinstance(v, torch.Tensor) and v.is_cuda)


def _setting(given, name: str) -> torch.Tensor:
    """A setting in float64, 0-dimensional or (…, K), with the argument errors raised before any device work. Host-side values
    (floats, sequences, CPU tensors) are checked; device tensors are used as given (a check would synchronise)."""
    if isinstance(given, bool) or given is None:
        raise ValueError(f"{name} must be numbers or tensors, got {given!r}")
    # (a Python number or sequence straight to float64: torch's default dtype would round it to float32 first)
    v = (given if isinstance(given, torch.Tensor) else torch.as_tensor(given, dtype=torch.float64)).to(torch.float64)
    if v.dim() and v.shape[-1] == 0:
        raise ValueError(f"{name} must hold at least one value, got shape {tuple(v.shape)}")
    if _on_host(given):
        d = v.detach()
        if not bool(torch.isfinite(d).all()):
            raise ValueError(f"{name} must be finite")
        if name == "wavelengths" and not bool((d > 0).all()):
            raise ValueError("wavelengths must be > 0")
    return v


def modulation_settings(wavelengths, amplitudes, phases, device) -> tuple[torch.Tensor, ...]:
    """(amplitudes, wavelengths, phases), each float64 (…, K) on `device` with one K: a single value stands for all K modes. Raises
    `with_density_modulation`'s ValueErrors."""
    given = {"amplitudes": amplitudes, "wavelengths": wavelengths, "phases": phases}
    vals = {name: _setting(v, name) for name, v in given.items()}
    lengths = {v.shape[-1] for v in vals.values() if v.dim()}
    if len(lengths) > 1:
        raise ValueError("wavelengths, amplitudes and phases must hold one value per mode, got lengths "
                         f"{[tuple(v.shape[-1:]) for v in vals.values()]}")
    K = lengths.pop() if lengths else 1
    if K > _ops.DENSITY_MAX_MODES:
        raise ValueError(f"at most {_ops.DENSITY_MAX_MODES} modes per call are supported, got {K}")
    a = vals["amplitudes"]
    if _on_host(amplitudes):
        total = a.detach().abs().sum(dim=-1) if a.dim() else a.detach().abs() * K
        if not bool((total < 1).all()):
            raise ValueError("the amplitudes must satisfy sum |A_m| < 1: beyond that the density would be negative somewhere and the "
                             "map tau' -> tau is not monotone")
    out = []
    for name, v in vals.items():
        scalar = isinstance(given[name], numbers.Real)
        if device.type == "cuda" and not v.is_cuda:
            # (a single number: a fill on the device, not a host-to-device copy)
            v = torch.full((K,), float(v), dtype=torch.float64, device=device) if scalar else v.to(device, non_blocking=True)
        out.append(v.expand(K) if v.dim() == 0 else v)
    return tuple(out)


def with_density_modulation(beam, wavelengths, amplitudes, phases=0.0):
    p = beam.particles
    a, w, ph = modulation_settings(wavelengths, amplitudes, phases, p.device)
    out = _ops.density_modulate(p, a, w, ph)
    return type(beam)(out, beam.energy, particle_charges=beam.particle_charges, survival_probabilities=beam.survival_probabilities,
                      s=beam.s, species=beam.species)
