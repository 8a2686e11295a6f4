"""Steady-state coherent synchrotron radiation kick of `cheetah_amd._ops` (the CSRKick element): deposit of the surviving particles'
charge on M nodes in tau, the anti-causal Toeplitz sum with the exactly integrated (z - z')^(-1/3) kernel, gather and kick to delta
— one `chx_csr_kick` call (four launches, the scale formed on the device, deterministic, no host synchronisation) and its autograd
node, whose backward is `chx_csr_kick_bwd`.

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import torch

from . import _lib
from ._ops import MAX_GRID_ROWS, aligned, bshapes, check, dtype_code, flat_bcast, numel, ptr, require_device, stream_ptr, workspace

__all__ = ["CSR_MAX_BINS", "CSRKickFunction", "csr_kick", "csr_scale", "_csr_kick_raw", "_csr_kick_bwd_raw"]

#: CHX_WAKE_MAX_BINS of include/chx.h: the grid and deposit are the wake's
CSR_MAX_BINS = 4096
#: doubles per batch row of the state the forward pass leaves for the backward pass: header + M (CHX_CSR_STATE_DOUBLES)
_STATE_HEADER = 8


def _rows(t: torch.Tensor, batch_shape, B: int, dtype):
    """A setting as flat rows of the beam's dtype: (1,) view of a single value (an in-place edit reaches the kernel) or (B,)."""
    t = t.to(dtype)
    if t.numel() == 1:
        return t.reshape(1)
    return t.expand(batch_shape).reshape(B).contiguous()


def _csr_kick_raw(x, q, w, e, L, a, mass_eV: float, abs_z: float, B: int, N: int, M: int):
    """chx_csr_kick on flat inputs x (Bx, N, 7), q (Bq, N), w (Bw, N), energy e, length L, angle a ((1,) or (B,)), all in the beam
    dtype -> (out (B, N, 7), state (B, 8 + M) float64)."""
    lib = _lib.lib()
    ws_bytes = lib.chx_csr_workspace_bytes(B, N, M)
    ws = workspace(ws_bytes, x.device)
    out = torch.empty((B, N, 7), dtype=x.dtype, device=x.device)
    state = torch.empty((B, _STATE_HEADER + M), dtype=torch.float64, device=x.device)
    check(lib.chx_csr_kick(ptr(x), ptr(q), ptr(w), ptr(e), ptr(L), ptr(a), mass_eV, abs_z, B, x.shape[0], q.shape[0], w.shape[0],
                           e.shape[0], L.shape[0], a.shape[0], N, M, dtype_code(x.dtype), ptr(out), ptr(state), ptr(ws), ws_bytes,
                           stream_ptr()), "chx_csr_kick")
    return out, state


def _csr_kick_bwd_raw(x, q, w, state, d_out, B: int, N: int, M: int, need_c: bool):
    """chx_csr_kick_bwd: (dX (B, N, 7), dC (B, N) | None, d_scale (B,) float64); rows of broadcast inputs not summed."""
    kw = {"dtype": x.dtype, "device": x.device}
    dX = torch.empty((B, N, 7), **kw)
    dC = torch.empty((B, N), **kw) if need_c else None
    d_scale = torch.empty((B,), dtype=torch.float64, device=x.device)
    lib = _lib.lib()
    ws_bytes = lib.chx_csr_workspace_bytes(B, N, M)
    ws = workspace(ws_bytes, x.device)
    check(lib.chx_csr_kick_bwd(ptr(x), ptr(q), ptr(w), B, x.shape[0], q.shape[0], w.shape[0], N, M, dtype_code(x.dtype), ptr(state),
                               ptr(d_out), ptr(dX), ptr(dC), ptr(d_scale), ptr(ws), ws_bytes, stream_ptr()), "chx_csr_kick_bwd")
    return dX, dC, d_scale


def _safe_pow(v: torch.Tensor, p: float) -> torch.Tensor:
    """v^p for v > 0, 0 at v = 0 with a zero gradient there (the kick is 0 at L = 0 or theta = 0), NaN for v < 0."""
    pos = v > 0
    r = torch.where(pos, v, torch.ones_like(v)).pow(p)
    return torch.where(pos, r, torch.where(v == 0, torch.zeros_like(v), torch.full_like(v, float("nan"))))


def csr_scale(energy: torch.Tensor, mass_eV: float, abs_charge_number: float, length: torch.Tensor,
              angle: torch.Tensor) -> torch.Tensor:
    """|Z| L^(1/3) |theta|^(2/3) / p0c in float64 (p0c as `Beam.p0c`), broadcast of the three shapes: the factor the kernels form on
    the device, restated here for the chain rule of the backward pass."""
    e = energy.to(torch.float64)
    gamma = e / mass_eV
    beta = torch.where(gamma.abs() > 0, (1 - gamma.square().reciprocal()).clamp_min(0).sqrt(), torch.ones_like(gamma))
    return abs_charge_number * _safe_pow(length.to(torch.float64), 1 / 3) * _safe_pow(angle.to(torch.float64).abs(), 2 / 3) / (
        beta * gamma * mass_eV)


class CSRKickFunction(torch.autograd.Function):
    """out (B, N, 7) = chx_csr_kick(x, q, w, energy, L, theta); backward = chx_csr_kick_bwd: gradients of the particles, the
    charges and survival probabilities (through c = |q| w), and of energy, L and theta through the per-row d(scale). The node
    grid (tau range) is a constant."""

    @staticmethod
    def forward(ctx, x, q, w, e, L, a, mass_eV, abs_z, B, M):
        out, state = _csr_kick_raw(x, q, w, e, L, a, mass_eV, abs_z, B, x.shape[1], M)
        ctx.save_for_backward(x, q, w, e, L, a, state)
        ctx.B, ctx.M, ctx.mass_eV, ctx.abs_z = B, M, mass_eV, abs_z
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, q, w, e, L, a, state = ctx.saved_tensors
        B, M, N = ctx.B, ctx.M, x.shape[1]
        need = ctx.needs_input_grad
        dX, dC, d_scale = _csr_kick_bwd_raw(x, q, w, state, d_out.contiguous().to(x.dtype), B, N, M, need[1] or need[2])
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
                s = csr_scale(leaves[0], ctx.mass_eV, ctx.abs_z, leaves[1], leaves[2]).expand(B)
                grads = torch.autograd.grad(s, [leaves[i] for i in wanted], d_scale)
            for i, g in zip(wanted, grads):
                settings[i] = g.to(x.dtype)
        return (dX if need[0] else None), dq, dw, *settings, None, None, None, None


def csr_kick(particles: torch.Tensor, charges: torch.Tensor, survival: torch.Tensor, energy: torch.Tensor, mass_eV: float,
             abs_charge_number: float, length: torch.Tensor, angle: torch.Tensor, num_bins: int) -> torch.Tensor:
    """The steady-state CSR kick of an arc of length `length` and bend angle `angle` on a beam of any batch shape (broadcast of the
    particles', charges', survival probabilities', energy's, length's and angle's batch shapes) -> particles (*batch, N, 7).
    Differentiable with respect to the particles, charges, survival probabilities, energy, length and angle."""
    require_device(particles, charges, survival, energy, length, angle)
    dt = particles.dtype
    N = particles.shape[-2]
    batch_shape = bshapes(particles.shape[:-2], charges.shape[:-1], survival.shape[:-1], energy.shape, length.shape, angle.shape)
    B = numel(batch_shape)
    if B > MAX_GRID_ROWS:
        raise ValueError(f"CSRKick: at most {MAX_GRID_ROWS} batch rows per kick, got {B}")
    x, _ = flat_bcast(particles, batch_shape, 2)
    q, _ = flat_bcast(charges.to(dt), batch_shape, 1)
    w, _ = flat_bcast(survival.to(dt), batch_shape, 1)
    x, q, w = aligned(x), q.contiguous(), w.contiguous()
    e, L, a = (_rows(t, batch_shape, B, dt) for t in (energy, length, angle))
    grads = torch.is_grad_enabled() and any(t.requires_grad for t in (x, q, w, e, L, a))
    if grads:
        out = CSRKickFunction.apply(x, q, w, e, L, a, float(mass_eV), float(abs_charge_number), B, num_bins)
    else:
        out, _ = _csr_kick_raw(x, q, w, e, L, a, float(mass_eV), float(abs_charge_number), B, N, num_bins)
    return out.reshape(*batch_shape, N, 7)
