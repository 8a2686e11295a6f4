"""The laser energy modulation of `cheetah_amd._ops` (LaserModulator): a laser resonant with an undulator's radiation modulates the
energy at the optical wavelength, following the laser's transverse profile and pulse envelope, in one particle pass,
`chx_laser_kick`. Deterministic, no host synchronisation, capturable in a device graph; the autograd node's backward is
`chx_laser_kick_bwd`, which gives the particles' gradient and the per-row cotangents of the eight row factors; `laser_factors`
restates those factors in float64 torch for the chain rule to the eight settings and the energy.

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import math

import torch

from . import _lib
from ._ops import MAX_GRID_ROWS, aligned, bshapes, check, dtype_code, flat_bcast, numel, ptr, require_device, stream_ptr, workspace
from ._ops_grid1d import _rows

__all__ = ["laser_kick", "laser_factors"]

_TWO_PI = 2 * math.pi


def laser_factors(energy, mass_eV: float, amplitude, wavelength, phase, laser_sigma, offset_x, offset_y, pulse_sigma,
                  pulse_center) -> tuple[torch.Tensor, ...]:
    """(a, nu, phi_t, g, x0, y0, h, tau0) = (A / (P0 mc^2), 1 / lambda, phi / (2 pi), 1 / (4 sigma_r^2), x0, y0, 1 / (4 sigma_t^2),
    tau0) in float64, P0 = beta0 gamma0 of the reference energy as `Beam.p0c` forms it and h = 0 for `pulse_sigma=None`: the row
    factors the kernels form on the device, restated here for the chain rule of the backward pass."""
    f64 = lambda t: t.to(torch.float64)  # noqa: E731
    gamma = f64(energy) / mass_eV
    beta = torch.where(gamma.abs() > 0, (1 - gamma.square().reciprocal()).clamp_min(0).sqrt(), torch.ones_like(gamma))
    a = f64(amplitude) / (beta * gamma * mass_eV)
    g = 1 / (4 * f64(laser_sigma).square())
    h = torch.zeros((), dtype=torch.float64, device=g.device) if pulse_sigma is None else 1 / (4 * f64(pulse_sigma).square())
    return a, 1 / f64(wavelength), f64(phase) / _TWO_PI, g, f64(offset_x), f64(offset_y), h, f64(pulse_center)


def _row(t, batch_shape, B: int, dtype):
    """A setting as the kernels read it: a single value of the beam's dtype as it is (no view object per call; an in-place edit
    reaches the kernel), anything else as `_rows` flattens it."""
    if t.dim() == 0 and t.dtype == dtype:
        return t
    return _rows(t, batch_shape, B, dtype)


def _head(x, rows, mass_eV, B):
    return (ptr(x), *map(ptr, rows), mass_eV, B, x.shape[0], *(1 if t is None or t.dim() == 0 else t.shape[0] for t in rows),
            x.shape[1], dtype_code(x.dtype))


def _laser_raw(x, rows, mass_eV, B):
    out = torch.empty((B, x.shape[1], 7), dtype=x.dtype, device=x.device)
    check(_lib.lib().chx_laser_kick(*_head(x, rows, mass_eV, B), ptr(out), stream_ptr()), "chx_laser_kick")
    return out


class LaserKick(torch.autograd.Function):
    """out (B, N, 7) = chx_laser_kick(x, energy and the eight settings as rows); backward = chx_laser_kick_bwd: gradients of the
    particles and, through the per-row cotangents of (a, nu, phi_t, g, x0, y0, h, tau0), of the energy and the settings. `rows`:
    energy, amplitude, wavelength, phase, laser_sigma, offset_x, offset_y, pulse_sigma (or None), pulse_center."""

    @staticmethod
    def forward(ctx, mass_eV, B, x, *rows):
        out = _laser_raw(x, rows, mass_eV, B)
        ctx.save_for_backward(x, *rows)
        ctx.args = (mass_eV, B)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, *rows = ctx.saved_tensors
        mass_eV, B = ctx.args
        N = x.shape[1]
        need = ctx.needs_input_grad[2:]
        dX = torch.empty((B, N, 7), dtype=x.dtype, device=x.device)
        d_rows = torch.empty((B, 8), dtype=torch.float64, device=x.device)
        lib = _lib.lib()
        ws_bytes = lib.chx_laser_workspace_bytes(B, N)
        ws = workspace(ws_bytes, x.device)
        check(lib.chx_laser_kick_bwd(*_head(x, rows, mass_eV, B), ptr(aligned(d_out.to(x.dtype))), ptr(dX), ptr(d_rows), ptr(ws),
                                     ws_bytes, stream_ptr()), "chx_laser_kick_bwd")
        if need[0] and x.shape[0] == 1 and B > 1:
            dX = dX.sum(dim=0, keepdim=True)
        settings = [None] * len(rows)
        wanted = [i for i in range(len(rows)) if need[1 + i]]
        if wanted:
            with torch.enable_grad():
                leaves = [None if t is None else t.detach().requires_grad_(need[1 + i]) for i, t in enumerate(rows)]
                factors = laser_factors(leaves[0], mass_eV, *leaves[1:])
                outs = [(o.expand(B), d_rows[:, k]) for k, o in enumerate(factors) if o.requires_grad]
                grads = torch.autograd.grad([o for o, _ in outs], [leaves[i] for i in wanted], [d for _, d in outs])
            for i, g in zip(wanted, grads):
                settings[i] = g.to(x.dtype)
        return None, None, (dX if need[0] else None), *settings


def laser_kick(particles: torch.Tensor, energy: torch.Tensor, mass_eV: float, amplitude: torch.Tensor, wavelength: torch.Tensor,
               phase: torch.Tensor, laser_sigma: torch.Tensor, offset_x: torch.Tensor, offset_y: torch.Tensor,
               pulse_sigma: torch.Tensor | None, pulse_center: torch.Tensor) -> torch.Tensor:
    """The energy modulation delta' = delta + a exp(-g ((x - x0)^2 + (y - y0)^2) - h (tau - tau0)^2) sin(2 pi (tau / lambda) + phi)
    on a beam of any batch shape (broadcast of the particles', the energy's and the eight settings' batch shapes) -> particles
    (*batch, N, 7); the row factors are `laser_factors`'. `pulse_sigma=None`: no envelope. Differentiable with respect to the
    particles, the energy and all eight settings."""
    settings = (energy, amplitude, wavelength, phase, laser_sigma, offset_x, offset_y, pulse_sigma, pulse_center)
    require_device(particles, *settings)
    batch_shape = bshapes(particles.shape[:-2], *(t.shape for t in settings if t is not None))
    B = numel(batch_shape)
    if B > MAX_GRID_ROWS:
        raise ValueError(f"LaserModulator: at most {MAX_GRID_ROWS} batch rows per kick, got {B}")
    N = particles.shape[-2]
    x = aligned(flat_bcast(particles, batch_shape, 2)[0])
    rows = tuple(None if t is None else _row(t, batch_shape, B, particles.dtype) for t in settings)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, *rows)):
        out = LaserKick.apply(float(mass_eV), B, x, *rows)
    else:
        out = _laser_raw(x, rows, float(mass_eV), B)
    return out.reshape(*batch_shape, N, 7)
