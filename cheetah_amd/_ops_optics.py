"""The one-turn map of a ring of drift-kick-drift elements, its 6 x 6 Jacobian and the closed orbit (Segment.one_turn_map,
closed_orbit, ring_optics) in one call of `chx_dkd_ring_jacobian`: a lane per (seed, tangent direction) carries the point and one
tangent through all items in registers, the Newton steps of the closed orbit run inside the kernel. Two launches, no workspace
beyond the items' constants, no host synchronisation, deterministic. The definition: include/chx.h, DESIGN.md.

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import c_i64, c_int, c_void_p
from ._ops import check, dtype_code, ptr, require_device, stream_ptr, workspace

__all__ = ["RING_MAX_ITEMS", "RING_MODES", "dkd_ring_jacobian"]

#: the most items one ring may have (kDkdChainMax of csrc/chx_nonlinear.hip, the limit of chx_dkd_turns)
RING_MAX_ITEMS = 192
#: `mode` of chx_dkd_ring_jacobian
RING_MODES = {"map": 0, "closed_4d": 1, "closed_6d": 2}

_lib.SIGNATURES["chx_dkd_ring_jacobian_workspace_bytes"] = (ctypes.c_size_t, [c_i64])
_lib.SIGNATURES["chx_dkd_ring_jacobian"] = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, ctypes.c_double, ctypes.c_double,
                                                    c_int, c_void_p, c_i64, c_int, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p])
if _lib._lib is not None:                       # the library was loaded before this module: bind the symbols now
    for _name in ("chx_dkd_ring_jacobian_workspace_bytes", "chx_dkd_ring_jacobian"):
        _fn = getattr(_lib._lib, _name)
        _fn.restype, _fn.argtypes = _lib.SIGNATURES[_name]


def dkd_ring_jacobian(arrays, E: int, energy: torch.Tensor, mass_eV: float, n_charges: float, start: torch.Tensor, mode: int,
                      num_iterations: int, along: bool):
    """chx_dkd_ring_jacobian for the host arrays of `dkd_turn_arrays` (E items), the reference energy (0-d, the settings' dtype, on
    the device) and start (B, 6) float64: a dict of float64 tensors orbit (B, 6), image (B, 6), matrix (B, 6, 6), residual (B,),
    dispersion (B, 4) and, with `along`, orbit_along (B, E + 1, 6), matrix_along (B, E + 1, 6, 6) and s_along (E + 1,) in the
    energy's dtype. Launches only."""
    if start.dim() != 2 or start.shape[1] != 6 or start.dtype != torch.float64:
        raise ValueError(f"the seeds must be a float64 tensor of the shape (B, 6), got {start.dtype} {tuple(start.shape)}")
    require_device(start, energy)
    start = start.contiguous()
    B, dev = int(start.shape[0]), start.device
    f64 = {"dtype": torch.float64, "device": dev}
    out = {"orbit": torch.empty((B, 6), **f64), "image": torch.empty((B, 6), **f64), "matrix": torch.empty((B, 6, 6), **f64),
           "residual": torch.empty((B,), **f64), "dispersion": torch.empty((B, 4), **f64)}
    if along:
        out["orbit_along"] = torch.empty((B, E + 1, 6), **f64)
        out["matrix_along"] = torch.empty((B, E + 1, 6, 6), **f64)
        out["s_along"] = torch.empty((E + 1,), dtype=energy.dtype, device=dev)
    lib = _lib.lib()
    ws = workspace(lib.chx_dkd_ring_jacobian_workspace_bytes(E), dev)
    check(lib.chx_dkd_ring_jacobian(arrays[0], arrays[1], arrays[2], arrays[3], E, ptr(energy), mass_eV, n_charges, dtype_code(energy.dtype),
                                    ptr(start), B, int(mode), int(num_iterations), int(bool(along)), ptr(out["orbit"]), ptr(out["image"]),
                                    ptr(out["matrix"]), ptr(out["residual"]), ptr(out["dispersion"]), ptr(out.get("orbit_along")),
                                    ptr(out.get("matrix_along")), ptr(out.get("s_along")), ptr(ws), ws.numel(), stream_ptr()),
          "chx_dkd_ring_jacobian")
    return out
