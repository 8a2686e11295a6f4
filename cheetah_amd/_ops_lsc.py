"""Longitudinal space-charge kick of `cheetah_amd._ops` (the LSCKick element): deposit of the surviving particles' charge on M nodes
in tau, the two-sided Toeplitz sum with the exactly integrated on-axis field of a charged disc, gather and kick to delta — one
`chx_lsc_kick` call (four launches, the scale and rho formed on the device, deterministic, no host synchronisation) and its autograd
node, whose backward is `chx_lsc_kick_bwd`.

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import torch

from . import _lib
from ._ops import MAX_GRID_ROWS, aligned, bshapes, check, dtype_code, flat_bcast, numel, ptr, require_device, stream_ptr, workspace
from ._ops_csr import _rows

__all__ = ["LSC_MAX_BINS", "LSCKickFunction", "lsc_kick", "lsc_scale_rho", "_lsc_kick_raw", "_lsc_kick_bwd_raw"]

#: CHX_WAKE_MAX_BINS of include/chx.h: the grid and deposit are the wake's
LSC_MAX_BINS = 4096
#: k_e = 1 / (4 pi eps0), V m / C (chx_lsc.hip)
_K_E = 8.9875517923e9


def _state_doubles(M: int) -> int:
    """Doubles per batch row of the state the forward pass leaves for the backward pass: header, M node sums, rho, a free slot, M
    deposits (CHX_LSC_STATE_DOUBLES)."""
    return 8 + 2 + 2 * M


def _lsc_kick_raw(x, q, w, e, L, a, mass_eV: float, abs_z: float, B: int, N: int, M: int):
    """chx_lsc_kick on flat inputs x (Bx, N, 7), q (Bq, N), w (Bw, N), energy e, length L, radius a ((1,) or (B,)), all in the beam
    dtype -> (out (B, N, 7), state (B, 10 + 2 M) float64)."""
    lib = _lib.lib()
    ws_bytes = lib.chx_lsc_workspace_bytes(B, N, M)
    ws = workspace(ws_bytes, x.device)
    out = torch.empty((B, N, 7), dtype=x.dtype, device=x.device)
    state = torch.empty((B, _state_doubles(M)), dtype=torch.float64, device=x.device)
    check(lib.chx_lsc_kick(ptr(x), ptr(q), ptr(w), ptr(e), ptr(L), ptr(a), mass_eV, abs_z, B, x.shape[0], q.shape[0], w.shape[0],
                           e.shape[0], L.shape[0], a.shape[0], N, M, dtype_code(x.dtype), ptr(out), ptr(state), ptr(ws), ws_bytes,
                           stream_ptr()), "chx_lsc_kick")
    return out, state


def _lsc_kick_bwd_raw(x, q, w, state, d_out, B: int, N: int, M: int, need_c: bool):
    """chx_lsc_kick_bwd: (dX (B, N, 7), dC (B, N) | None, d_scale (B,), d_rho (B,) float64); rows of broadcast inputs not summed."""
    kw = {"dtype": x.dtype, "device": x.device}
    dX = torch.empty((B, N, 7), **kw)
    dC = torch.empty((B, N), **kw) if need_c else None
    d_scale = torch.empty((B,), dtype=torch.float64, device=x.device)
    d_rho = torch.empty((B,), dtype=torch.float64, device=x.device)
    lib = _lib.lib()
    ws_bytes = lib.chx_lsc_workspace_bytes(B, N, M)
    ws = workspace(ws_bytes, x.device)
    check(lib.chx_lsc_kick_bwd(ptr(x), ptr(q), ptr(w), B, x.shape[0], q.shape[0], w.shape[0], N, M, dtype_code(x.dtype), ptr(state),
                               ptr(d_out), ptr(dX), ptr(dC), ptr(d_scale), ptr(d_rho), ptr(ws), ws_bytes, stream_ptr()),
          "chx_lsc_kick_bwd")
    return dX, dC, d_scale, d_rho


def lsc_scale_rho(energy: torch.Tensor, mass_eV: float, abs_charge_number: float, length: torch.Tensor, radius: torch.Tensor,
                  h: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(S, rho) = (|Z| 2 k_e L / (gamma^2 h^2 p0c), a / (gamma h)) in float64 (p0c as `Beam.p0c`), broadcast of the four shapes: the
    factors the kernels form on the device, restated here for the chain rule of the backward pass. `h` is the node spacing of the
    forward's state header, a constant; a row without a grid (h = 0) has S = 0 and a constant rho."""
    e = energy.to(torch.float64)
    gamma = e / mass_eV
    beta = torch.where(gamma.abs() > 0, (1 - gamma.square().reciprocal()).clamp_min(0).sqrt(), torch.ones_like(gamma))
    grid = h > 0
    hs = torch.where(grid, h, torch.ones_like(h))
    S = abs_charge_number * 2 * _K_E * length.to(torch.float64) / (gamma.square() * hs.square() * (beta * gamma * mass_eV))
    rho = radius.to(torch.float64) / (gamma * hs)
    return torch.where(grid, S, torch.zeros_like(S)), torch.where(grid, rho, torch.ones_like(rho))


class LSCKickFunction(torch.autograd.Function):
    """out (B, N, 7) = chx_lsc_kick(x, q, w, energy, L, a); backward = chx_lsc_kick_bwd: gradients of the particles, the charges and
    survival probabilities (through c = |q| w), and of energy, L and the radius through the per-row d(S) and d(rho). The node grid
    (tau range) is a constant."""

    @staticmethod
    def forward(ctx, x, q, w, e, L, a, mass_eV, abs_z, B, M):
        out, state = _lsc_kick_raw(x, q, w, e, L, a, mass_eV, abs_z, B, x.shape[1], M)
        ctx.save_for_backward(x, q, w, e, L, a, state)
        ctx.B, ctx.M, ctx.mass_eV, ctx.abs_z = B, M, mass_eV, abs_z
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, q, w, e, L, a, state = ctx.saved_tensors
        B, M, N = ctx.B, ctx.M, x.shape[1]
        need = ctx.needs_input_grad
        dX, dC, d_scale, d_rho = _lsc_kick_bwd_raw(x, q, w, state, d_out.contiguous().to(x.dtype), B, N, M, need[1] or need[2])
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
        settings = [None, None, None]
        wanted = [i for i in range(3) if need[3 + i]]
        if wanted:
            with torch.enable_grad():
                leaves = [t.detach().requires_grad_(need[3 + i]) for i, t in enumerate((e, L, a))]
                S, rho = lsc_scale_rho(leaves[0], ctx.mass_eV, ctx.abs_z, leaves[1], leaves[2], state[:, 2])
                # S does not see the radius and rho does not see L: only what carries a graph goes into the chain rule
                outs = [(o.expand(B), d) for o, d in ((S, d_scale), (rho, d_rho)) if o.requires_grad]
                grads = torch.autograd.grad([o for o, _ in outs], [leaves[i] for i in wanted], [d for _, d in outs])
            for i, g in zip(wanted, grads):
                settings[i] = g.to(x.dtype)
        return (dX if need[0] else None), dq, dw, *settings, None, None, None, None


def lsc_kick(particles: torch.Tensor, charges: torch.Tensor, survival: torch.Tensor, energy: torch.Tensor, mass_eV: float,
             abs_charge_number: float, length: torch.Tensor, radius: torch.Tensor, num_bins: int) -> torch.Tensor:
    """The longitudinal space-charge kick of a straight section of length `length` on a beam of disc radius `radius` and of any batch
    shape (broadcast of the particles', charges', survival probabilities', energy's, length's and radius' batch shapes) ->
    particles (*batch, N, 7). Differentiable with respect to the particles, charges, survival probabilities, energy, length and
    radius."""
    require_device(particles, charges, survival, energy, length, radius)
    dt = particles.dtype
    N = particles.shape[-2]
    batch_shape = bshapes(particles.shape[:-2], charges.shape[:-1], survival.shape[:-1], energy.shape, length.shape, radius.shape)
    B = numel(batch_shape)
    if B > MAX_GRID_ROWS:
        raise ValueError(f"LSCKick: at most {MAX_GRID_ROWS} batch rows per kick, got {B}")
    x, _ = flat_bcast(particles, batch_shape, 2)
    q, _ = flat_bcast(charges.to(dt), batch_shape, 1)
    w, _ = flat_bcast(survival.to(dt), batch_shape, 1)
    x, q, w = aligned(x), q.contiguous(), w.contiguous()
    e, L, a = (_rows(t, batch_shape, B, dt) for t in (energy, length, radius))
    grads = torch.is_grad_enabled() and any(t.requires_grad for t in (x, q, w, e, L, a))
    if grads:
        out = LSCKickFunction.apply(x, q, w, e, L, a, float(mass_eV), float(abs_charge_number), B, num_bins)
    else:
        out, _ = _lsc_kick_raw(x, q, w, e, L, a, float(mass_eV), float(abs_charge_number), B, N, num_bins)
    return out.reshape(*batch_shape, N, 7)
