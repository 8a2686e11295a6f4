#!/usr/bin/env python3
"""Time the quiet-start deviates (chx_quiet_sequence) on the GPU at 1e6 rows x 6 columns, float32 and float64: the kernel alone
(normal deviates and uniforms), a torch composition of the same sequence on the GPU (the digits peeled off integer tensors, one
float64 division, `torch.special.ndtri`) as the yardstick, `torch.randn` of the same shape (what a drawn beam costs), and the
factories `from_parameters(quiet_start=True)` / `from_parameters()` end to end (whitening, Cholesky and colouring included). Times
are the mean over back-to-back calls between two events (launch-bound work included). One JSON line per case."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("QUIET_REPS", "50"))
BASES = (5, 7, 11, 13, 2, 3)
N = 1_000_000


def timed(fn, reps=REPS):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def torch_halton(n, bases, offset, dtype, normal=True):
    """The same sequence composed of torch operations: int64 tensors on the GPU, a fixed number of digit steps per base (enough for
    the largest index, so nothing is read back), one float64 division, ndtri."""
    idx = torch.arange(offset + 1, offset + 1 + n, dtype=torch.int64, device="cuda")
    cols = []
    for b in bases:
        i, r, p = idx.clone(), torch.zeros_like(idx), torch.ones_like(idx)
        digits = 1
        while b**digits <= offset + n:
            digits += 1
        for _ in range(digits):
            on = i > 0
            q = i // b
            r = torch.where(on, r * b + (i - q * b), r)
            p = torch.where(on, p * b, p)
            i = q
        cols.append(r.double() / p.double())
    u = torch.stack(cols, dim=1)
    return (torch.special.ndtri(u) if normal else u).to(dtype)


def case(dtype):
    kw = {"dtype": dtype, "device": "cuda"}
    quiet = lambda normal=True: ca._ops.quiet_sequence(N, BASES, normal=normal, **kw)  # noqa: E731
    with torch.no_grad():
        kernel_us = timed(quiet)
        uniform_us = timed(lambda: quiet(False))
        torch_us = timed(lambda: torch_halton(N, BASES, 0, dtype), reps=max(REPS // 5, 5))
        randn_us = timed(lambda: torch.randn(N, 6, **kw))
        beam_quiet_us = timed(lambda: ca.ParticleBeam.from_parameters(num_particles=N, quiet_start=True, **kw), reps=max(REPS // 5, 5))
        beam_randn_us = timed(lambda: ca.ParticleBeam.from_parameters(num_particles=N, **kw), reps=max(REPS // 5, 5))
        u_equal = bool(torch.equal(quiet(False), torch_halton(N, BASES, 0, dtype, normal=False)))
        z_diff = float((quiet().double() - torch_halton(N, BASES, 0, torch.float64)).abs().max())
        lam = [8e-6 / 5, 8e-6 / 20, 8e-6 / 50]                      # the factories' default sigma_tau is 8e-6
        b_quiet = ca.ParticleBeam.from_parameters(num_particles=N, quiet_start=True, **kw).bunching_factor(lam).abs().tolist()
        torch.manual_seed(0)
        b_randn = ca.ParticleBeam.from_parameters(num_particles=N, **kw).bunching_factor(lam).abs().tolist()
    print(json.dumps({"case": "quiet_sequence", "rows": N, "columns": len(BASES), "dtype": str(dtype),
                      "normal_us": round(kernel_us, 1), "uniform_us": round(uniform_us, 1), "torch_composition_us": round(torch_us, 1),
                      "randn_us": round(randn_us, 1), "speedup_vs_torch": round(torch_us / kernel_us, 1),
                      "beam_quiet_us": round(beam_quiet_us, 1), "beam_randn_us": round(beam_randn_us, 1),
                      "uniforms_bit_equal_to_torch": u_equal, "max_abs_normal_difference_to_torch": z_diff,
                      "bunching_quiet": [float(f"{v:.3e}") for v in b_quiet],
                      "bunching_randn": [float(f"{v:.3e}") for v in b_randn]}), flush=True)


def main():
    for dtype in (torch.float32, torch.float64):
        case(dtype)


if __name__ == "__main__":
    main()
