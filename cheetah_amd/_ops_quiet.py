"""The quiet-start deviates of `cheetah_amd._ops`: the Halton sequence in up to eight prime bases, as uniforms in (0, 1) or as
standard-normal deviates, in one launch, `chx_quiet_sequence`. Bit-defined (integer digits, one IEEE division), bitwise reproducible,
no host synchronisation, capturable in a device graph.

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import ctypes
import numbers

import torch

from . import _lib
from ._ops import check, check_current_device, dtype_code, ptr, stream_ptr

__all__ = ["quiet_sequence", "check_sequence_range", "QUIET_MAX_DIMS", "QUIET_PRIMES", "QUIET_INDEX_END"]

#: CHX_QUIET_MAX_DIMS: columns per call
QUIET_MAX_DIMS = 8
#: the bases the kernel holds as compile-time constants
QUIET_PRIMES = (2, 3, 5, 7, 11, 13, 17, 19)
#: indices stay below 2^40: the digit sums of the radical inverse stay below 2^53
QUIET_INDEX_END = 1 << 40


def check_sequence_range(n, offset) -> None:
    """ValueError unless rows 0 .. n - 1 at `offset` (indices offset + 1 .. offset + n) lie in the sequence's range."""
    for name, v in (("the number of rows", n), ("the sequence offset", offset)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    if n < 1:
        raise ValueError(f"the number of rows must be >= 1, got {n}")
    if offset < 0:
        raise ValueError(f"the sequence offset must be >= 0, got {offset}")
    if offset + n >= QUIET_INDEX_END:
        raise ValueError(f"the sequence offset {offset} with {n} rows passes the end of the sequence's range, 2^40")


def quiet_sequence(n: int, bases, offset: int = 0, normal: bool = True, dtype: torch.dtype = torch.float32,
                   device="cuda") -> torch.Tensor:
    """(n, len(bases)) of `dtype` on `device`: row r is the Halton point of index offset + 1 + r, column d its radical inverse in
    the base bases[d] (distinct primes up to 19, at most eight), u in (0, 1) — or, with `normal`, the standard-normal deviate
    -+ sqrt(2) erfcinv(2 min(u, 1 - u)) of that u, formed in float64 and rounded once to `dtype`. Rows [a, b) of one call equal a call
    with `offset + a`: ranks of a sharded beam pass offset = rank * n. A constant: nothing to differentiate."""
    check_sequence_range(n, offset)
    bases = tuple(bases)
    if not 1 <= len(bases) <= QUIET_MAX_DIMS:
        raise ValueError(f"between 1 and {QUIET_MAX_DIMS} bases are supported, got {len(bases)}")
    if any(b not in QUIET_PRIMES for b in bases) or len(set(bases)) != len(bases):
        raise ValueError(f"the bases must be distinct primes out of {QUIET_PRIMES}, got {bases}")
    code = dtype_code(dtype)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("cheetah_amd generates quiet-start deviates on the GPU only (a HIP kernel, no CPU fallback): pass a ROCm "
                           "device, e.g. device='cuda'.")
    check_current_device(device)
    out = torch.empty((n, len(bases)), dtype=dtype, device=device)
    c_bases = (ctypes.c_int * len(bases))(*bases)
    check(_lib.lib().chx_quiet_sequence(ctypes.cast(c_bases, ctypes.c_void_p), len(bases), n, offset, int(bool(normal)), code, ptr(out),
                                        stream_ptr()), "chx_quiet_sequence")
    return out
