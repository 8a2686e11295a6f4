"""The bunching factor of `cheetah_amd._ops` (ParticleBeam.bunching_factor): F(nu) = sum a exp(-2 pi i nu tau) and Q = sum a
(a = charge x survival probability) for a beam of any batch shape, in one call of `chx_bunching` (a direct sum over
particle x frequency pairs in fixed-size chunks merged in order: deterministic, no host synchronisation) and its autograd node,
whose backward is `chx_bunching_bwd` (every particle sums over the frequencies).

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import torch

from . import _lib
from ._ops import MAX_GRID_ROWS, bshapes, check, dtype_code, flat_bcast, numel, ptr, require_device, stream_ptr, workspace

__all__ = ["BUNCHING_K_MAX", "BUNCHING_CHUNK", "BUNCHING_K_TILE", "Bunching", "bunching", "_bunching_raw", "_bunching_bwd_raw"]

#: CHX_BUNCHING_K_MAX of include/chx.h: the most frequencies one call takes
BUNCHING_K_MAX = 65536
#: CHX_BUNCHING_CHUNK: particles per workgroup, the granule of the ordered merge
BUNCHING_CHUNK = 2048
#: CHX_BUNCHING_K_TILE: frequencies per workgroup
BUNCHING_K_TILE = 256


def _rows(t, b0, b1):
    return t if t is None or t.shape[0] == 1 else t[b0:b1]


def _bunching_raw(x, w, q, nu, B: int, N: int, K: int):
    """chx_bunching on flat inputs x (Bx, N, 7), w (Bw, N), q (Bq, N), nu (Bnu, K) float64 -> (F (B, K, 2), Q (B,)) float64.
    More rows than one launch takes (the batch index is a grid dimension): row slices, one call each."""
    if B > MAX_GRID_ROWS:
        outs = [_bunching_raw(_rows(x, b0, min(B, b0 + MAX_GRID_ROWS)), _rows(w, b0, min(B, b0 + MAX_GRID_ROWS)),
                              _rows(q, b0, min(B, b0 + MAX_GRID_ROWS)), _rows(nu, b0, min(B, b0 + MAX_GRID_ROWS)),
                              min(B, b0 + MAX_GRID_ROWS) - b0, N, K)
                for b0 in range(0, B, MAX_GRID_ROWS)]
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    lib = _lib.lib()
    ws_bytes = lib.chx_bunching_workspace_bytes(B, N, K)
    ws = workspace(ws_bytes, x.device)
    F = torch.empty((B, K, 2), dtype=torch.float64, device=x.device)
    Q = torch.empty((B,), dtype=torch.float64, device=x.device)
    check(lib.chx_bunching(ptr(x), ptr(w), ptr(q), ptr(nu), B, x.shape[0], 1 if w is None else w.shape[0],
                           1 if q is None else q.shape[0], nu.shape[0], N, K, dtype_code(x.dtype), ptr(F), ptr(Q), ptr(ws), ws_bytes,
                           stream_ptr()), "chx_bunching")
    return F, Q


def _bunching_bwd_raw(x, w, q, nu, dF, dQ, B: int, N: int, K: int, need_tau: bool, need_w: bool, need_q: bool):
    """chx_bunching_bwd: (dTau (B, N) | None, dW (B, N) | None, dQpart (B, N) | None), rows of broadcast inputs not summed."""
    kw = {"dtype": x.dtype, "device": x.device}
    dTau = torch.empty((B, N), **kw) if need_tau else None
    dW = torch.empty((B, N), **kw) if need_w else None
    dQp = torch.empty((B, N), **kw) if need_q else None
    lib = _lib.lib()
    for b0 in range(0, B, MAX_GRID_ROWS):
        b1 = min(B, b0 + MAX_GRID_ROWS)
        xs, ws_, qs, ns = _rows(x, b0, b1), _rows(w, b0, b1), _rows(q, b0, b1), _rows(nu, b0, b1)
        check(lib.chx_bunching_bwd(ptr(xs), ptr(ws_), ptr(qs), ptr(ns), b1 - b0, xs.shape[0], 1 if ws_ is None else ws_.shape[0],
                                   1 if qs is None else qs.shape[0], ns.shape[0], N, K, dtype_code(x.dtype),
                                   ptr(None if dF is None else dF[b0:b1]), ptr(None if dQ is None else dQ[b0:b1]),
                                   ptr(None if dTau is None else dTau[b0:b1]), ptr(None if dW is None else dW[b0:b1]),
                                   ptr(None if dQp is None else dQp[b0:b1]), None, 0, stream_ptr()), "chx_bunching_bwd")
    return dTau, dW, dQp


class Bunching(torch.autograd.Function):
    """(F (B, K, 2), Q (B,)) = chx_bunching(x, w, q, nu); backward = chx_bunching_bwd: gradients of tau (column 4 of the
    particles; the other columns get exact zeros), the survival probabilities and the charges in one pass. The frequencies are
    constants (detached)."""

    @staticmethod
    def forward(ctx, x, w, q, nu, B, K):
        F, Q = _bunching_raw(x, w, q, nu, B, x.shape[1], K)
        ctx.save_for_backward(x, w, q, nu)
        ctx.B, ctx.K = B, K
        return F, Q

    @staticmethod
    def backward(ctx, dF, dQ):
        x, w, q, nu = ctx.saved_tensors
        B, K, N = ctx.B, ctx.K, x.shape[1]
        need_x = ctx.needs_input_grad[0]
        need_w = w is not None and ctx.needs_input_grad[1]
        need_q = q is not None and ctx.needs_input_grad[2]
        dF = None if dF is None else dF.contiguous().to(torch.float64)
        dQ = None if dQ is None else dQ.contiguous().to(torch.float64)
        if dF is None and dQ is None:
            return None, None, None, None, None, None
        dTau, dW, dQp = _bunching_bwd_raw(x, w, q, nu, dF, dQ, B, N, K, need_x, need_w, need_q)
        dX = None
        if need_x:
            if x.shape[0] == 1 and B > 1:
                dTau = dTau.sum(dim=0, keepdim=True)
            dX = torch.zeros_like(x)
            dX[..., 4] = dTau
        if need_w and w.shape[0] == 1 and B > 1:
            dW = dW.sum(dim=0, keepdim=True)
        if need_q and q.shape[0] == 1 and B > 1:
            dQp = dQp.sum(dim=0, keepdim=True)
        return dX, dW, dQp, None, None, None


def bunching(particles: torch.Tensor, survival: torch.Tensor, charges: torch.Tensor, nu: torch.Tensor):
    """F(nu) = sum a exp(-2 pi i nu tau) (complex128, (…, K)) and Q = sum a (float64, (…)) with a = charge x survival
    probability, for the frequencies nu (…, K) in turns per metre (float64, broadcast against the beam's batch shape, never
    differentiated). Differentiable with respect to the particles (column 4), the survival probabilities and the charges."""
    require_device(particles, survival, charges, nu)
    dt = particles.dtype
    N, K = particles.shape[-2], nu.shape[-1]
    batch_shape = bshapes(particles.shape[:-2], survival.shape[:-1], charges.shape[:-1], nu.shape[:-1])
    B = numel(batch_shape)
    x, _ = flat_bcast(particles, batch_shape, 2)
    w, _ = flat_bcast(survival.to(dt), batch_shape, 1)
    q, _ = flat_bcast(charges.to(dt), batch_shape, 1)
    f, _ = flat_bcast(nu.detach().to(torch.float64), batch_shape, 1)
    x, w, q, f = x.contiguous(), w.contiguous(), q.contiguous(), f.contiguous()
    if torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or q.requires_grad):
        F, Q = Bunching.apply(x, w, q, f, B, K)
    else:
        F, Q = _bunching_raw(x, w, q, f, B, N, K)
    return torch.view_as_complex(F).reshape(*batch_shape, K), Q.reshape(tuple(batch_shape))
