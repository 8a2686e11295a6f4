"""The incoherent synchrotron-radiation kick of `cheetah_amd._ops` (SynchrotronRadiationKick): the classical energy loss and the
quantum excitation of a bend's arc in one particle pass, `chx_sr_kick`, with the normal deviates drawn inside the kernel from
Philox4x32-10 (key = (seed, stream), counter = (particle, batch row, call index)). Deterministic, no host synchronisation,
capturable in a device graph; the autograd node's backward is `chx_sr_kick_bwd`, which draws the deviates again from a clone of the
call index the forward pass used, so no (B, N) noise tensor is kept.

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import math

import torch

from . import _lib
from ._ops import MAX_GRID_ROWS, aligned, bshapes, check, dtype_code, flat_bcast, numel, ptr, require_device, stream_ptr, workspace
from ._ops_grid1d import _rows

__all__ = ["sr_kick", "sr_factors", "sr_normals"]

#: r_e (m), m_e c^2 (eV), hbar c (eV m) and 55 / (24 sqrt 3), as csrc/chx_sr.hip
_R_E = 2.8179403205e-15
_M_E = 510998.95069
_HBAR_C = 1.973269804593025e-7
_QUANTUM = 55 / (24 * math.sqrt(3))


def sr_factors(energy: torch.Tensor, mass_eV: float, abs_z: float, length: torch.Tensor,
               angle: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(gamma0, a, b) = (E0 / mc^2, (2/3) r_c theta^2 / L, 55 / (24 sqrt 3) r_c lambda_c |theta|^3 / L^2) in float64, r_c = Z^2 r_e
    m_e / m and lambda_c = hbar c / mc^2; a and b are broadcasts of the length's and the angle's shapes, 0 with zero gradients where
    L = 0 or theta = 0 and NaN for L < 0: the factors the kernels form on the device, restated here for the chain rule of the
    backward pass."""
    gamma = energy.to(torch.float64) / mass_eV
    L, th = length.to(torch.float64), angle.to(torch.float64)
    rc, lc = abs_z * abs_z * _R_E * _M_E / mass_eV, _HBAR_C / mass_eV
    kicks = (L != 0) & (th != 0)
    Ls = torch.where(kicks, L, torch.ones_like(L))
    Ls = torch.where(Ls > 0, Ls, torch.full_like(Ls, float("nan")))
    a = (2 / 3) * rc * th.square() / Ls
    b = _QUANTUM * rc * lc * (th.abs() * th.square()) / Ls.square()
    return gamma, torch.where(kicks, a, torch.zeros_like(a)), torch.where(kicks, b, torch.zeros_like(b))


def _head(x, rows, mass_eV, abs_z, excite, seed, stream, call_index, B):
    e, L, th = rows
    return (ptr(x), ptr(e), ptr(L), ptr(th), mass_eV, abs_z, int(excite), seed, stream, ptr(call_index), B, x.shape[0], e.shape[0],
            L.shape[0], th.shape[0], x.shape[1], dtype_code(x.dtype))


def _sr_raw(x, rows, mass_eV, abs_z, excite, seed, stream, call_index, B):
    out = torch.empty((B, x.shape[1], 7), dtype=x.dtype, device=x.device)
    check(_lib.lib().chx_sr_kick(*_head(x, rows, mass_eV, abs_z, excite, seed, stream, call_index, B), ptr(out), stream_ptr()),
          "chx_sr_kick")
    return out


class SRKick(torch.autograd.Function):
    """out (B, N, 7) = chx_sr_kick(x, energy, length, angle; seed, stream, call index); backward = chx_sr_kick_bwd: gradients of the
    particles and, through the per-row cotangents of (gamma0, a, b), of the three settings. The deviates are constants."""

    @staticmethod
    def forward(ctx, mass_eV, abs_z, excite, seed, stream, call_index, B, x, *rows):
        out = _sr_raw(x, rows, mass_eV, abs_z, excite, seed, stream, call_index, B)
        # the value this call used: the element advances its own buffer in place right after the kick
        ctx.save_for_backward(x, call_index.clone(), *rows)
        ctx.args = (mass_eV, abs_z, excite, seed, stream, B)
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, call_index, *rows = ctx.saved_tensors
        mass_eV, abs_z, excite, seed, stream, B = ctx.args
        N = x.shape[1]
        need = ctx.needs_input_grad[7:]
        dX = torch.empty((B, N, 7), dtype=x.dtype, device=x.device)
        d_rows = [torch.empty((B,), dtype=torch.float64, device=x.device) for _ in range(3)]
        lib = _lib.lib()
        ws_bytes = lib.chx_sr_workspace_bytes(B, N)
        ws = workspace(ws_bytes, x.device)
        check(lib.chx_sr_kick_bwd(*_head(x, rows, mass_eV, abs_z, excite, seed, stream, call_index, B),
                                  ptr(aligned(d_out.to(x.dtype))), ptr(dX), *map(ptr, d_rows), ptr(ws), ws_bytes, stream_ptr()),
              "chx_sr_kick_bwd")
        if need[0] and x.shape[0] == 1 and B > 1:
            dX = dX.sum(dim=0, keepdim=True)
        settings = [None, None, None]
        wanted = [i for i in range(3) if need[1 + i]]
        if wanted:
            with torch.enable_grad():
                leaves = [t.detach().requires_grad_(need[1 + i]) for i, t in enumerate(rows)]
                factors = sr_factors(leaves[0], mass_eV, abs_z, leaves[1], leaves[2])
                outs = [(o.expand(B), d) for o, d in zip(factors, d_rows) if o.requires_grad]
                grads = torch.autograd.grad([o for o, _ in outs], [leaves[i] for i in wanted], [d for _, d in outs])
            for i, g in zip(wanted, grads):
                settings[i] = g.to(x.dtype)
        return None, None, None, None, None, None, None, (dX if need[0] else None), *settings


def sr_kick(particles: torch.Tensor, energy: torch.Tensor, mass_eV: float, abs_charge_number: float, length: torch.Tensor,
            angle: torch.Tensor, quantum_excitation: bool, seed: int, stream: int, call_index: torch.Tensor) -> torch.Tensor:
    """The incoherent synchrotron-radiation kick of an arc of length `length` and bend angle `angle` on a beam of any batch shape
    (broadcast of the particles', energy's, length's and angle's batch shapes) -> particles (*batch, N, 7). `seed`, `stream`: the
    32-bit halves of the generator's key; `call_index`: a one-element int64 device tensor, the upper half of its counter, which the
    kernel reads and the caller advances. Differentiable with respect to the particles, energy, length and angle."""
    require_device(particles, energy, length, angle, call_index)
    if call_index.dtype != torch.int64 or call_index.numel() != 1:
        raise TypeError("sr_kick: call_index must be a one-element int64 tensor")
    batch_shape = bshapes(particles.shape[:-2], energy.shape, length.shape, angle.shape)
    B = numel(batch_shape)
    if B > MAX_GRID_ROWS:
        raise ValueError(f"SynchrotronRadiationKick: at most {MAX_GRID_ROWS} batch rows per kick, got {B}")
    N = particles.shape[-2]
    x = aligned(flat_bcast(particles, batch_shape, 2)[0])
    rows = tuple(_rows(t, batch_shape, B, particles.dtype) for t in (energy, length, angle))
    args = (float(mass_eV), float(abs_charge_number), bool(quantum_excitation), int(seed), int(stream), call_index, B)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x, *rows)):
        out = SRKick.apply(*args, x, *rows)
    else:
        out = _sr_raw(x, rows, *args)
    return out.reshape(*batch_shape, N, 7)


def sr_normals(seed: int, stream: int, call: int, B: int, N: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """The kick's draw for call index `call`: (words (B, N, 4) as int64 values 0 ... 2^32 - 1, xi (B, N) float64) — the raw
    Philox4x32-10 output and the standard normal deviate of every (batch row, particle)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("cheetah_amd draws on the GPU only (HIP kernels, no CPU fallback)")
    words = torch.empty((B, N, 4), dtype=torch.int32, device=device)
    xi = torch.empty((B, N), dtype=torch.float64, device=device)
    check(_lib.lib().chx_sr_normals(int(seed), int(stream), int(call), B, N, ptr(words), ptr(xi), stream_ptr()), "chx_sr_normals")
    return words.to(torch.int64) & 0xFFFFFFFF, xi
