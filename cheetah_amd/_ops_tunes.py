"""The tunes of `cheetah_amd._ops` (TurnByTurn.tunes): for every recorded row and plane the interpolated peak of the Hann-windowed
spectrum of T consecutive records and the amplitude of that line, in one call of `chx_tunes` (one workgroup per row: a float32
transform in LDS finds the peak's grid point, float64 sums in a fixed order and safeguarded Newton steps find the peak;
deterministic, no workspace, no host synchronisation, capturable in a device graph). The definition: include/chx.h, DESIGN.md.

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import torch

from . import _lib
from ._lib import c_i64, c_int, c_void_p
from ._ops import check, dtype_code, ptr, require_device, stream_ptr

__all__ = ["TUNES_T_MIN", "TUNES_T_MAX", "TUNES_PLANES", "tunes"]

#: CHX_TUNES_T_MIN, CHX_TUNES_T_MAX of include/chx.h: the window lengths one call takes
TUNES_T_MIN = 8
TUNES_T_MAX = 4096
#: plane name -> bit of `columns` (and column 2 * bit of a particle row)
TUNES_PLANES = {"x": 0, "y": 1, "tau": 2}

_lib.SIGNATURES["chx_tunes"] = (c_int, [c_void_p, c_void_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_void_p, c_void_p, c_void_p])
if _lib._lib is not None:                       # the library was loaded before this module: bind the symbol now
    _fn = getattr(_lib._lib, "chx_tunes")
    _fn.restype, _fn.argtypes = _lib.SIGNATURES["chx_tunes"]


def tunes(probe: torch.Tensor, lost, first_record: int, num_records: int, last_turn: int, columns: int):
    """chx_tunes on probe (R, S, 7) (float32 or float64, contiguous) and lost (S,) int32 or None: (tune, amplitude), both (S, C)
    float64 with C the bits set in `columns` (bit 0: x, bit 1: y, bit 2: tau), in that order. The window is the records
    first_record .. first_record + num_records - 1; `last_turn` is the turn number of its last record (the loss rule)."""
    if probe.dim() != 3 or probe.shape[-1] != 7:
        raise ValueError(f"the records must have the shape (R, S, 7), got {tuple(probe.shape)}")
    require_device(probe, lost)
    R, S = int(probe.shape[0]), int(probe.shape[1])
    C = bin(int(columns) & 7).count("1")
    code = dtype_code(probe.dtype)
    probe = probe.contiguous()
    if lost is not None:
        if lost.shape != (S,):
            raise ValueError(f"lost must have the shape ({S},), got {tuple(lost.shape)}")
        lost = lost.to(torch.int32).contiguous()
    nu = torch.empty((S, C), dtype=torch.float64, device=probe.device)
    amp = torch.empty((S, C), dtype=torch.float64, device=probe.device)
    check(_lib.lib().chx_tunes(ptr(probe), ptr(lost), R, S, int(first_record), int(num_records), int(last_turn), int(columns), code,
                               ptr(nu), ptr(amp), stream_ptr()), "chx_tunes")
    return nu, amp
