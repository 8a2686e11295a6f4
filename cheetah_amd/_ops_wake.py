"""Short-range wakefield kick of `cheetah_amd._ops` (the Wakefield element): deposit of the surviving particles' charge (and dipole
moment) on M nodes in tau, causal convolution with the sampled wake, gather and kick — one `chx_wake_kick` call (four launches,
deterministic, no host synchronisation) and its autograd node, whose backward is `chx_wake_kick_bwd`.

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import torch

from . import _lib
from ._ops import MAX_GRID_ROWS, aligned, bshapes, check, dtype_code, flat_bcast, numel, ptr, require_device, stream_ptr, workspace

__all__ = ["WAKE_MAX_BINS", "WakeKick", "wake_kick", "wake_scale", "_wake_kick_raw", "_wake_kick_bwd_raw"]

#: CHX_WAKE_MAX_BINS of include/chx.h: the deposit's per-workgroup LDS histograms hold 3 channels of M 64-bit nodes
WAKE_MAX_BINS = 4096
#: doubles per batch row of the state the forward pass leaves for the backward pass (CHX_WAKE_STATE_DOUBLES)
_STATE_HEADER = 8


def _table(t):
    return (None, 0) if t is None else (t, t.numel())


def _wake_kick_raw(x, q, w, scale, wl, wt, h, B: int, N: int, M: int):
    """chx_wake_kick on flat inputs x (Bx, N, 7), q (Bq, N), w (Bw, N) in the beam dtype, scale (B,), wl, wt (L,) or None, h (1,)
    float64 -> (out (B, N, 7), state (B, 8 + 6 M) float64)."""
    lib = _lib.lib()
    ws_bytes = lib.chx_wake_workspace_bytes(B, N, M)
    ws = workspace(ws_bytes, x.device)
    out = torch.empty((B, N, 7), dtype=x.dtype, device=x.device)
    state = torch.empty((B, _STATE_HEADER + 6 * M), dtype=torch.float64, device=x.device)
    (wl, Ll), (wt, Lt) = _table(wl), _table(wt)
    check(lib.chx_wake_kick(ptr(x), ptr(q), ptr(w), ptr(scale), ptr(wl), Ll, ptr(wt), Lt, ptr(h), B, x.shape[0], q.shape[0],
                            w.shape[0], N, M, dtype_code(x.dtype), ptr(out), ptr(state), ptr(ws), ws_bytes, stream_ptr()),
          "chx_wake_kick")
    return out, state


def _wake_kick_bwd_raw(x, q, w, scale, wl, wt, h, state, d_out, B: int, N: int, M: int, need_c: bool, need_wl: bool, need_wt: bool):
    """chx_wake_kick_bwd: (dX (B, N, 7), dC (B, N) | None, d_scale (B,), d_wl | None, d_wt | None); rows of broadcast inputs not
    summed, the tables' gradients summed over the rows."""
    kw = {"dtype": x.dtype, "device": x.device}
    f64 = {"dtype": torch.float64, "device": x.device}
    dX = torch.empty((B, N, 7), **kw)
    dC = torch.empty((B, N), **kw) if need_c else None
    d_scale = torch.empty((B,), **f64)
    d_wl = torch.empty((wl.numel(),), **f64) if need_wl and wl is not None else None
    d_wt = torch.empty((wt.numel(),), **f64) if need_wt and wt is not None else None
    lib = _lib.lib()
    ws_bytes = lib.chx_wake_workspace_bytes(B, N, M)
    ws = workspace(ws_bytes, x.device)
    (wl, Ll), (wt, Lt) = _table(wl), _table(wt)
    check(lib.chx_wake_kick_bwd(ptr(x), ptr(q), ptr(w), ptr(scale), ptr(wl), Ll, ptr(wt), Lt, ptr(h), B, x.shape[0], q.shape[0],
                                w.shape[0], N, M, dtype_code(x.dtype), ptr(state), ptr(d_out), ptr(dX), ptr(dC), ptr(d_scale),
                                ptr(d_wl), ptr(d_wt), ptr(ws), ws_bytes, stream_ptr()), "chx_wake_kick_bwd")
    return dX, dC, d_scale, d_wl, d_wt


class WakeKick(torch.autograd.Function):
    """out (B, N, 7) = chx_wake_kick(x, q, w, scale, wl, wt); backward = chx_wake_kick_bwd: gradients of the particles, the charges
    and survival probabilities (through c = |q| w), the per-row scale factor |Z| / p0c and both tables. The node grid (tau
    range) and the wake spacing h are constants."""

    @staticmethod
    def forward(ctx, x, q, w, scale, wl, wt, h, B, M):
        out, state = _wake_kick_raw(x, q, w, scale, wl, wt, h, B, x.shape[1], M)
        ctx.save_for_backward(x, q, w, scale, wl, wt, h, state)
        ctx.B, ctx.M = B, M
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, q, w, scale, wl, wt, h, state = ctx.saved_tensors
        B, M, N = ctx.B, ctx.M, x.shape[1]
        need = ctx.needs_input_grad
        need_c = need[1] or need[2]
        dX, dC, d_scale, d_wl, d_wt = _wake_kick_bwd_raw(x, q, w, scale, wl, wt, h, state, d_out.contiguous().to(x.dtype), B, N, M,
                                                         need_c, need[4], need[5])
        dq = dw = None
        if need[1]:
            dq = dC * w * torch.sign(q)
            if q.shape[0] == 1 and B > 1:
                dq = dq.sum(dim=0, keepdim=True)
        if need[2]:
            dw = dC * q.abs()
            if w.shape[0] == 1 and B > 1:
                dw = dw.sum(dim=0, keepdim=True)
        if need[0] and x.shape[0] == 1 and B > 1:
            dX = dX.sum(dim=0, keepdim=True)
        return (dX if need[0] else None), dq, dw, (d_scale if need[3] else None), d_wl, d_wt, None, None, None


def wake_scale(energy: torch.Tensor, mass_eV: float, abs_charge_number: float, factor: torch.Tensor) -> torch.Tensor:
    """factor |Z| / p0c in float64 (p0c = beta gamma m c^2 of the reference energy, as `Beam.p0c`), broadcast of the two shapes."""
    e = energy.to(torch.float64)
    gamma = e / mass_eV
    beta = torch.where(gamma.abs() > 0, (1 - gamma.square().reciprocal()).clamp_min(0).sqrt(), torch.ones_like(gamma))
    return factor.to(torch.float64) * abs_charge_number / (beta * gamma * mass_eV)


def wake_kick(particles: torch.Tensor, charges: torch.Tensor, survival: torch.Tensor, energy: torch.Tensor, mass_eV: float,
              abs_charge_number: float, factor: torch.Tensor, longitudinal_wake, transverse_wake, wake_spacing: torch.Tensor,
              num_bins: int) -> torch.Tensor:
    """The wake kick of a beam of any batch shape (broadcast of the particles', charges', survival probabilities', energy's and
    factor's batch shapes) -> particles (*batch, N, 7). `longitudinal_wake` / `transverse_wake`: 1-D tables (V/C, V/(C m)) or
    None; `wake_spacing`: 0-d tensor h (metres between table entries). Differentiable with respect to the particles, charges,
    survival probabilities, energy, factor and both tables."""
    require_device(particles, charges, survival, energy, factor, wake_spacing, longitudinal_wake, transverse_wake)
    dt = particles.dtype
    N = particles.shape[-2]
    batch_shape = bshapes(particles.shape[:-2], charges.shape[:-1], survival.shape[:-1], energy.shape, factor.shape)
    B = numel(batch_shape)
    if B > MAX_GRID_ROWS:
        raise ValueError(f"Wakefield: at most {MAX_GRID_ROWS} batch rows per kick, got {B}")
    x, _ = flat_bcast(particles, batch_shape, 2)
    q, _ = flat_bcast(charges.to(dt), batch_shape, 1)
    w, _ = flat_bcast(survival.to(dt), batch_shape, 1)
    x, q, w = aligned(x), q.contiguous(), w.contiguous()
    scale = wake_scale(energy, mass_eV, abs_charge_number, factor).expand(batch_shape).reshape(B).contiguous()
    wl = None if longitudinal_wake is None else longitudinal_wake.to(torch.float64).contiguous()
    wt = None if transverse_wake is None else transverse_wake.to(torch.float64).contiguous()
    h = wake_spacing.detach().to(torch.float64).reshape(1)
    grads = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, q, w, scale, wl, wt))
    if grads:
        out = WakeKick.apply(x, q, w, scale, wl, wt, h, B, num_bins)
    else:
        out, _ = _wake_kick_raw(x, q, w, scale, wl, wt, h, B, N, num_bins)
    return out.reshape(*batch_shape, N, 7)
