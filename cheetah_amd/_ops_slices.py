"""Slice statistics of `cheetah_amd._ops` (ParticleBeam.slice_statistics): the chx_moments statistics and the charge of the
particles in every interval of tau, for a beam of any batch shape, in one call of `chx_slice_moments` (a stable counting sort by
slice, fixed-size pieces reduced in fp64, merged in order: deterministic, no host synchronisation) and its autograd node, whose
backward is `chx_slice_moments_bwd` (one pass over the particles).

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import torch

from . import _lib
from ._ops import MAX_GRID_ROWS, MOM_NOUT, bshapes, check, dtype_code, flat_bcast, numel, ptr, require_device, stream_ptr, workspace

__all__ = ["SLICES_MAX", "SliceMoments", "slice_moments", "default_tau_range", "_slice_moments_raw", "_slice_moments_bwd_raw"]

#: CHX_SLICES_MAX of include/chx.h: the edges and the ranking pass's per-wave slice counters live in LDS
SLICES_MAX = 2048


def _rows(t, b0, b1):
    return t if t is None or t.shape[0] == 1 else t[b0:b1]


def _slice_moments_raw(x, w, q, e, B: int, N: int, S: int):
    """chx_slice_moments on flat inputs x (Bx, N, 7), w (Bw, N), q (Bq, N), e (Be, S + 1) -> (moments (B, S, 29), charge (B, S))
    float64. More rows than one launch takes (the batch index is a grid dimension): row slices, one call each."""
    if B > MAX_GRID_ROWS:
        outs = [_slice_moments_raw(_rows(x, b0, min(B, b0 + MAX_GRID_ROWS)), _rows(w, b0, min(B, b0 + MAX_GRID_ROWS)),
                                   _rows(q, b0, min(B, b0 + MAX_GRID_ROWS)), _rows(e, b0, min(B, b0 + MAX_GRID_ROWS)),
                                   min(B, b0 + MAX_GRID_ROWS) - b0, N, S)
                for b0 in range(0, B, MAX_GRID_ROWS)]
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    lib = _lib.lib()
    ws_bytes = lib.chx_slice_moments_workspace_bytes(B, N, S)
    ws = workspace(ws_bytes, x.device)
    out = torch.empty((B, S, MOM_NOUT), dtype=torch.float64, device=x.device)
    charge = torch.empty((B, S), dtype=torch.float64, device=x.device)
    check(lib.chx_slice_moments(ptr(x), ptr(w), ptr(q), ptr(e), B, x.shape[0], 1 if w is None else w.shape[0],
                                1 if q is None else q.shape[0], e.shape[0], N, S, dtype_code(x.dtype), ptr(out), ptr(charge), ptr(ws),
                                ws_bytes, stream_ptr()), "chx_slice_moments")
    return out, charge


def _slice_moments_bwd_raw(x, w, q, e, out, d_out, d_charge, B: int, N: int, S: int, need_x: bool, need_w: bool, need_q: bool):
    """chx_slice_moments_bwd: (dX (B, N, 7) | None, dW (B, N) | None, dQ (B, N) | None), rows of broadcast inputs not summed."""
    kw = {"dtype": x.dtype, "device": x.device}
    dX = torch.empty((B, N, 7), **kw) if need_x else None
    dW = torch.empty((B, N), **kw) if need_w else None
    dQ = torch.empty((B, N), **kw) if need_q else None
    lib = _lib.lib()
    for b0 in range(0, B, MAX_GRID_ROWS):
        b1 = min(B, b0 + MAX_GRID_ROWS)
        rows = b1 - b0
        xs, ws_, qs, es = _rows(x, b0, b1), _rows(w, b0, b1), _rows(q, b0, b1), _rows(e, b0, b1)
        ws_bytes = lib.chx_slice_moments_workspace_bytes(rows, N, S)
        ws = workspace(ws_bytes, x.device)
        check(lib.chx_slice_moments_bwd(ptr(xs), ptr(ws_), ptr(qs), ptr(es), rows, xs.shape[0], 1 if ws_ is None else ws_.shape[0],
                                        1 if qs is None else qs.shape[0], es.shape[0], N, S, dtype_code(x.dtype), ptr(out[b0:b1]),
                                        ptr(None if d_out is None else d_out[b0:b1]),
                                        ptr(None if d_charge is None else d_charge[b0:b1]),
                                        ptr(None if dX is None else dX[b0:b1]), ptr(None if dW is None else dW[b0:b1]),
                                        ptr(None if dQ is None else dQ[b0:b1]), ptr(ws), ws_bytes, stream_ptr()),
              "chx_slice_moments_bwd")
    return dX, dW, dQ


class SliceMoments(torch.autograd.Function):
    """(moments (B, S, 29), charge (B, S)) = chx_slice_moments(x, w, q, edges); backward = chx_slice_moments_bwd: gradients of
    the particles, the survival probabilities and the charges in one pass. The edges are constants (detached)."""

    @staticmethod
    def forward(ctx, x, w, q, e, B, S):
        out, charge = _slice_moments_raw(x, w, q, e, B, x.shape[1], S)
        ctx.save_for_backward(x, w, q, e, out)
        ctx.B, ctx.S = B, S
        return out, charge

    @staticmethod
    def backward(ctx, d_out, d_charge):
        x, w, q, e, out = ctx.saved_tensors
        B, S, N = ctx.B, ctx.S, x.shape[1]
        need_x = ctx.needs_input_grad[0]
        need_w = w is not None and ctx.needs_input_grad[1]
        need_q = q is not None and ctx.needs_input_grad[2]
        d_out = None if d_out is None else d_out.contiguous().to(torch.float64)
        d_charge = None if d_charge is None else d_charge.contiguous().to(torch.float64)
        if d_out is None and d_charge is None:
            return None, None, None, None, None, None
        dX, dW, dQ = _slice_moments_bwd_raw(x, w, q, e, out, d_out, d_charge, B, N, S, need_x, need_w, need_q)
        if need_x and x.shape[0] == 1 and B > 1:
            dX = dX.sum(dim=0, keepdim=True)
        if need_w and w.shape[0] == 1 and B > 1:
            dW = dW.sum(dim=0, keepdim=True)
        if need_q and q.shape[0] == 1 and B > 1:
            dQ = dQ.sum(dim=0, keepdim=True)
        return dX, dW, dQ, None, None, None


def default_tau_range(particles: torch.Tensor, survival: torch.Tensor):
    """(min tau, max tau) per batch row over the particles with survival probability > 0 (NaN tau left out): masked reductions
    on the device, no host synchronisation."""
    tau = particles[..., 4]
    alive = (survival > 0) & ~torch.isnan(tau)
    inf = float("inf")
    return torch.where(alive, tau, inf).amin(dim=-1), torch.where(alive, tau, -inf).amax(dim=-1)


def slice_moments(particles: torch.Tensor, survival: torch.Tensor, charges: torch.Tensor, edges: torch.Tensor):
    """Per slice of tau (edges (…, S + 1), increasing, broadcast against the beam's batch shape): (moments (…, S, 29) float64 in
    the chx_moments layout, charge (…, S) float64 = sum of charge x survival probability). Differentiable with respect to the
    particles, the survival probabilities and the charges."""
    require_device(particles, survival, charges, edges)
    dt = particles.dtype
    N, S = particles.shape[-2], edges.shape[-1] - 1
    batch_shape = bshapes(particles.shape[:-2], survival.shape[:-1], charges.shape[:-1], edges.shape[:-1])
    B = numel(batch_shape)
    x, _ = flat_bcast(particles, batch_shape, 2)
    w, _ = flat_bcast(survival.to(dt), batch_shape, 1)
    q, _ = flat_bcast(charges.to(dt), batch_shape, 1)
    e, _ = flat_bcast(edges.detach().to(dt), batch_shape, 1)
    x, w, q, e = x.contiguous(), w.contiguous(), q.contiguous(), e.contiguous()
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or q.requires_grad):
        out, charge = SliceMoments.apply(x, w, q, e, B, S)
    else:
        out, charge = _slice_moments_raw(x, w, q, e, B, N, S)
    return out.reshape(*batch_shape, S, MOM_NOUT), charge.reshape(*batch_shape, S)
