"""The one-turn map of a ring of drift-kick-drift elements, its 6 x 6 Jacobian and the closed orbit (Segment.one_turn_map,
closed_orbit, ring_optics) in one call of `chx_dkd_ring_jacobian`: a lane per (seed, tangent direction) carries the point and one
tangent through all items in registers, the Newton steps of the closed orbit run inside the kernel. Two launches, no workspace
beyond the items' constants, no host synchronisation, deterministic. `chx_dkd_ring_sensitivity` gives the derivatives of those
results with respect to knobs on the ring's settings (Segment.ring_sensitivity, the `wrt` argument): a group of lanes per (seed,
knob) carries second-order dual numbers through the same maps. The definitions: include/chx.h, DESIGN.md.

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import c_i64, c_int, c_void_p
from ._ops import check, dtype_code, ptr, require_device, stream_ptr, workspace

__all__ = ["RING_MAX_ITEMS", "RING_MODES", "dkd_ring_jacobian", "dkd_ring_sensitivity", "dkd_ring_radiation"]

#: the most items one ring may have (kDkdChainMax of csrc/chx_nonlinear.hip, the limit of chx_dkd_turns)
RING_MAX_ITEMS = 192
#: `mode` of chx_dkd_ring_jacobian
RING_MODES = {"map": 0, "closed_4d": 1, "closed_6d": 2}

_lib.SIGNATURES["chx_dkd_ring_jacobian_workspace_bytes"] = (ctypes.c_size_t, [c_i64])
_lib.SIGNATURES["chx_dkd_ring_jacobian"] = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, ctypes.c_double, ctypes.c_double,
                                                    c_int, c_void_p, c_i64, c_int, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p])
_lib.SIGNATURES["chx_dkd_ring_sensitivity_workspace_bytes"] = (ctypes.c_size_t, [c_i64, c_i64])
_lib.SIGNATURES["chx_dkd_ring_sensitivity"] = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, ctypes.c_double, ctypes.c_double,
                                                       c_int, c_void_p, c_i64, c_int, c_void_p, c_void_p, c_void_p, c_i64, c_i64, c_int, c_void_p,
                                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_size_t, c_void_p])
_lib.SIGNATURES["chx_dkd_ring_radiation_workspace_bytes"] = (ctypes.c_size_t, [c_i64])
_lib.SIGNATURES["chx_dkd_ring_radiation"] = (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, ctypes.c_double, ctypes.c_double,
                                                     c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_i64, c_void_p, c_void_p, c_void_p,
                                                     ctypes.c_size_t, c_void_p])
if _lib._lib is not None:                       # the library was loaded before this module: bind the symbols now
    for _name in ("chx_dkd_ring_jacobian_workspace_bytes", "chx_dkd_ring_jacobian", "chx_dkd_ring_sensitivity_workspace_bytes",
                  "chx_dkd_ring_sensitivity", "chx_dkd_ring_radiation_workspace_bytes", "chx_dkd_ring_radiation"):
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


def dkd_ring_sensitivity(arrays, E: int, energy: torch.Tensor, mass_eV: float, n_charges: float, orbit: torch.Tensor, mode: int, components,
                         K: int, along: bool):
    """chx_dkd_ring_sensitivity for the host arrays of `dkd_turn_arrays` (E items), the converged orbits (B, 6) float64 of a
    `dkd_ring_jacobian` call of the same mode and K knobs given by `components`, a sequence of (knob, item, slot): a dict of float64
    tensors d_orbit (B, K, 6), d_image (B, K, 6), d_matrix (B, K, 6, 6), d_dispersion (B, K, 4) and, with `along`, d_orbit_along (B, K, E + 1, 6) and
    d_matrix_along (B, K, E + 1, 6, 6). Launches only."""
    if orbit.dim() != 2 or orbit.shape[1] != 6 or orbit.dtype != torch.float64:
        raise ValueError(f"the orbits must be a float64 tensor of the shape (B, 6), got {orbit.dtype} {tuple(orbit.shape)}")
    require_device(orbit, energy)
    orbit = orbit.contiguous()
    B, K, dev = int(orbit.shape[0]), int(K), orbit.device
    f64 = {"dtype": torch.float64, "device": dev}
    out = {"d_orbit": torch.empty((B, K, 6), **f64), "d_image": torch.empty((B, K, 6), **f64), "d_matrix": torch.empty((B, K, 6, 6), **f64),
           "d_dispersion": torch.empty((B, K, 4), **f64)}
    if along:
        out["d_orbit_along"] = torch.empty((B, K, E + 1, 6), **f64)
        out["d_matrix_along"] = torch.empty((B, K, E + 1, 6, 6), **f64)
    components = list(components)
    i32 = ctypes.c_int32 * max(len(components), 1)
    knob_of, item_of, slot_of = (i32(*[int(c[j]) for c in components]) for j in range(3))
    lib = _lib.lib()
    ws = workspace(lib.chx_dkd_ring_sensitivity_workspace_bytes(E, K), dev)
    check(lib.chx_dkd_ring_sensitivity(arrays[0], arrays[1], arrays[2], arrays[3], E, ptr(energy), mass_eV, n_charges, dtype_code(energy.dtype),
                                       ptr(orbit), B, int(mode), knob_of, item_of, slot_of, len(components), K, int(bool(along)),
                                       ptr(out["d_orbit"]), ptr(out["d_image"]), ptr(out["d_matrix"]), ptr(out["d_dispersion"]), ptr(out.get("d_orbit_along")),
                                       ptr(out.get("d_matrix_along")), ptr(ws), ws.numel(), stream_ptr()), "chx_dkd_ring_sensitivity")
    return out


def dkd_ring_radiation(arrays, E: int, energy: torch.Tensor, mass_eV: float, n_charges: float, orbit: torch.Tensor, beta0: torch.Tensor,
                       alpha0: torch.Tensor, eta0: torch.Tensor, along: bool):
    """chx_dkd_ring_radiation for the host arrays of `dkd_turn_arrays` (E items), the converged 4-D orbits (B, 6) float64 of a
    `dkd_ring_jacobian` call and the start values beta0 (B, 2), alpha0 (B, 2), eta0 (B, 4) of its one-turn matrix: a dict of float64
    tensors integrals (B, 7) = (I1, I2, I3, I4x, I4y, I5x, I5y) and, with `along`, integrals_along (B, E, 7). Launches only."""
    B = int(orbit.shape[0]) if orbit.dim() == 2 else -1
    for name, t, width in (("orbits", orbit, 6), ("beta0", beta0, 2), ("alpha0", alpha0, 2), ("eta0", eta0, 4)):
        if t.dim() != 2 or t.shape[0] != B or t.shape[1] != width or t.dtype != torch.float64:
            raise ValueError(f"the {name} must be a float64 tensor of the shape (B, {width}), got {t.dtype} {tuple(t.shape)}")
    require_device(orbit, energy, beta0, alpha0, eta0)
    orbit, beta0, alpha0, eta0 = orbit.contiguous(), beta0.contiguous(), alpha0.contiguous(), eta0.contiguous()
    dev = orbit.device
    out = {"integrals": torch.empty((B, 7), dtype=torch.float64, device=dev)}
    if along:
        out["integrals_along"] = torch.empty((B, E, 7), dtype=torch.float64, device=dev)
    lib = _lib.lib()
    ws = workspace(lib.chx_dkd_ring_radiation_workspace_bytes(E), dev)
    check(lib.chx_dkd_ring_radiation(arrays[0], arrays[1], arrays[2], arrays[3], E, ptr(energy), mass_eV, n_charges, dtype_code(energy.dtype),
                                     ptr(orbit), ptr(beta0), ptr(alpha0), ptr(eta0), B, ptr(out["integrals"]), ptr(out.get("integrals_along")),
                                     ptr(ws), ws.numel(), stream_ptr()), "chx_dkd_ring_radiation")
    return out
