#!/usr/bin/env python3
"""Time ParticleBeam.slice_statistics (chx_slice_moments and its backward) on the GPU: forward and forward + backward at 1e6
float32 particles for S = 50, 100, 256 slices, and a vectorised beam of 16 x 1e5 particles; `_ops.moments` on the same beam is
the yardstick. Times are the mean over back-to-back calls between two events (launch-bound work included). Run under
`rocprofv3 --kernel-trace --stats` for the kernel durations. One JSON line per case."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402
from cheetah_amd import _ops  # noqa: E402

REPS = int(os.environ.get("SLICES_REPS", "100"))


def timed(fn, reps=REPS):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def case(name, beam, S):
    x, w, q = beam.particles, beam.survival_probabilities, beam.particle_charges
    with torch.no_grad():
        edges = beam.slice_statistics(num_slices=S).edges.contiguous()
        moments_us = timed(lambda: _ops.moments(x, w))
        kernel_us = timed(lambda: _ops.slice_moments(x, w, q, edges))
        api_us = timed(lambda: beam.slice_statistics(num_slices=S))
    xg = x.detach().clone().requires_grad_()

    def fwd_bwd():
        xg.grad = None
        m, c = _ops.slice_moments(xg, w, q, edges)
        (m[..., 8:].nan_to_num().sum() + m[..., 2:8].nan_to_num().sum() + c.sum()).backward()

    fb_us = timed(fwd_bwd, reps=max(REPS // 2, 10))
    print(json.dumps({"case": name, "particles": list(x.shape[:-1]), "slices": S, "dtype": str(x.dtype),
                      "slice_moments_fwd_us": round(kernel_us, 1), "slice_statistics_api_us": round(api_us, 1),
                      "slice_moments_fwd_bwd_us": round(fb_us, 1), "moments_us": round(moments_us, 1),
                      "fwd_over_moments": round(kernel_us / moments_us, 2)}), flush=True)


def main():
    kw = {"dtype": torch.float32, "device": "cuda"}
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, **kw)
    for S in (50, 100, 256):
        case("1e6", beam, S)
    vec = ca.ParticleBeam(torch.randn(16, 100_000, 7, **kw) * 1e-5, energy=torch.tensor(1e8, **kw))
    vec.particles[..., 6] = 1.0
    case("16x1e5", vec, 100)


if __name__ == "__main__":
    main()
