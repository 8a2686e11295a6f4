"""The seeded density modulation of `cheetah_amd._ops` (`ParticleBeam.with_density_modulation`): every particle's tau moves to the
root tau' of tau' + sum_m A_m / (2 pi nu_m) sin(2 pi (tau' nu_m + phi_t,m)) = tau, which multiplies the longitudinal density by
1 + sum_m A_m cos(2 pi tau / lambda_m + phi_m), in one particle pass, `chx_density_modulate`. Deterministic, no host synchronisation,
capturable in a device graph; the autograd node's backward is `chx_density_modulate_bwd`, which gives the particles' gradient and the
per-row cotangents of (A_m, nu_m, phi_t,m); `density_factors` restates those factors in float64 torch for the chain rule to the
amplitudes, wavelengths and phases.

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import math

import torch

from . import _lib
from ._ops import MAX_GRID_ROWS, aligned, bshapes, check, dtype_code, flat_bcast, numel, ptr, require_device, stream_ptr, workspace

__all__ = ["density_modulate", "density_factors", "DENSITY_MAX_MODES"]

#: CHX_DENSITY_MAX_MODES: modes per call
DENSITY_MAX_MODES = 8
_TWO_PI = 2 * math.pi


def density_factors(amplitudes, wavelengths, phases) -> tuple[torch.Tensor, ...]:
    """(A, nu, phi_t) = (A, 1 / lambda, phi / (2 pi)) in float64: the row factors the kernels form on the device, restated here
    for the chain rule of the backward pass."""
    f64 = lambda t: t.to(torch.float64)  # noqa: E731
    return f64(amplitudes), 1 / f64(wavelengths), f64(phases) / _TWO_PI


def _head(x, rows, B, K):
    return (ptr(x), *map(ptr, rows), K, B, x.shape[0], *(t.shape[0] for t in rows), x.shape[1], dtype_code(x.dtype))


def _modulate_raw(x, rows, B, K):
    out = torch.empty((B, x.shape[1], 7), dtype=x.dtype, device=x.device)
    check(_lib.lib().chx_density_modulate(*_head(x, rows, B, K), ptr(out), stream_ptr()), "chx_density_modulate")
    return out


class DensityModulate(torch.autograd.Function):
    """out (B, N, 7) = chx_density_modulate(x, amplitudes, wavelengths, phases as rows (1 or B, K) float64); backward =
    chx_density_modulate_bwd: gradients of the particles and, through the per-row cotangents of (A_m, nu_m, phi_t,m), of the three
    settings."""

    @staticmethod
    def forward(ctx, B, K, x, *rows):
        out = _modulate_raw(x, rows, B, K)
        ctx.save_for_backward(x, *rows)
        ctx.args = (B, K)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, *rows = ctx.saved_tensors
        B, K = ctx.args
        N = x.shape[1]
        need = ctx.needs_input_grad[2:]
        dX = torch.empty((B, N, 7), dtype=x.dtype, device=x.device)
        d_rows = torch.empty((B, 3, DENSITY_MAX_MODES), dtype=torch.float64, device=x.device)
        lib = _lib.lib()
        ws_bytes = lib.chx_density_workspace_bytes(B, N)
        ws = workspace(ws_bytes, x.device)
        check(lib.chx_density_modulate_bwd(*_head(x, rows, B, K), ptr(aligned(d_out.to(x.dtype))), ptr(dX), ptr(d_rows), ptr(ws),
                                           ws_bytes, stream_ptr()), "chx_density_modulate_bwd")
        if need[0] and x.shape[0] == 1 and B > 1:
            dX = dX.sum(dim=0, keepdim=True)
        settings = [None] * len(rows)
        wanted = [i for i in range(len(rows)) if need[1 + i]]
        if wanted:
            with torch.enable_grad():
                leaves = [t.detach().requires_grad_(need[1 + i]) for i, t in enumerate(rows)]
                factors = density_factors(*leaves)
                outs = [(o.expand(B, K), d_rows[:, k, :K]) for k, o in enumerate(factors) if o.requires_grad]
                grads = torch.autograd.grad([o for o, _ in outs], [leaves[i] for i in wanted], [d for _, d in outs])
            for i, g in zip(wanted, grads):
                settings[i] = g
        return None, None, (dX if need[0] else None), *settings


def density_modulate(particles: torch.Tensor, amplitudes: torch.Tensor, wavelengths: torch.Tensor,
                     phases: torch.Tensor) -> torch.Tensor:
    """tau -> tau' with tau' + sum_m A_m lambda_m / (2 pi) sin(2 pi tau' / lambda_m + phi_m) = tau on a beam of any batch shape
    -> particles (*batch, N, 7). The settings are float64 device tensors (…, K), K <= 8 modes, whose leading dimensions broadcast
    against the particles' batch shape. Every column but tau keeps its bits; a row with sum |A_m| >= 1 gets NaN in tau'.
    Differentiable with respect to the particles and the three settings."""
    settings = (amplitudes, wavelengths, phases)
    require_device(particles, *settings)
    K = amplitudes.shape[-1]
    if any(t.dim() < 1 or t.shape[-1] != K or t.dtype != torch.float64 for t in settings):
        raise ValueError("density_modulate: amplitudes, wavelengths and phases must be float64 tensors (…, K) with one K, got shapes "
                         f"{[tuple(t.shape) for t in settings]} and dtypes {[t.dtype for t in settings]}")
    if not 1 <= K <= DENSITY_MAX_MODES:
        raise ValueError(f"between 1 and {DENSITY_MAX_MODES} modes are supported, got {K}")
    batch_shape = bshapes(particles.shape[:-2], *(t.shape[:-1] for t in settings))
    B = numel(batch_shape)
    if B > MAX_GRID_ROWS:
        raise ValueError(f"with_density_modulation: at most {MAX_GRID_ROWS} batch rows per call, got {B}")
    N = particles.shape[-2]
    x = aligned(flat_bcast(particles, batch_shape, 2)[0])
    rows = tuple(flat_bcast(t, batch_shape, 1)[0].contiguous() for t in settings)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, *rows)):
        out = DensityModulate.apply(B, K, x, *rows)
    else:
        out = _modulate_raw(x, rows, B, K)
    return out.reshape(*batch_shape, N, 7)
