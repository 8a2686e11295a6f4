#!/usr/bin/env python3
"""Time the TransientCSRKick (chx_csr_transient_kick and its backward) next to the CSRKick on the same beam in the same process: 1e6
float32 particles, M = 500 and 4096 nodes, at a slippage length of x = M / 8 nodes (the table ends at lag 4x + 2: the sums stop
there) and at x = 2 M (the steady-state table, CSRKick's sums term for term); forward and forward + backward. Times are the mean over
back-to-back calls between two events (launch-bound work included). Run under `rocprofv3 --kernel-trace --stats` for the kernel
durations; `CSRT_CASES=500:0.125` restricts the run to one (M, x / M) pair, so that a trace holds one table length per kernel name.
One JSON line per case."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("CSR_REPS", "100"))
CASES = [(int(m), float(r)) for m, r in (c.split(":") for c in os.environ.get(
    "CSRT_CASES", "500:0.125,500:2,4096:0.125,4096:2").split(","))]


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


def fwd_and_bwd(elem, beam):
    with torch.no_grad():
        fwd_us = timed(lambda: elem.track(beam))
    xg = beam.particles.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(xg, beam.energy, particle_charges=beam.particle_charges, survival_probabilities=beam.survival_probabilities)

    def fwd_bwd():
        xg.grad = None
        elem.track(gb).particles[:, 5].square().sum().backward()

    return fwd_us, timed(fwd_bwd, reps=max(REPS // 2, 10))


def case(beam, M, x_over_M):
    kw = {"dtype": beam.particles.dtype, "device": beam.particles.device}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    L, theta = 0.2, 0.02
    tau = beam.particles[:, 4].double()
    h = float(tau.max() - tau.min()) / (M - 1)
    d = (24 * (L / theta) ** 2 * x_over_M * M * h) ** (1 / 3)        # x = d^3 theta^2 / (24 L^2 h)
    steady = ca.CSRKick(t(L), t(theta), num_bins=M, **kw)
    transient = ca.TransientCSRKick(t(L), t(theta), t(d), num_bins=M, **kw)
    with torch.no_grad():
        a, b = steady.track(beam).particles, transient.track(beam).particles
        same = bool(torch.equal(a, b))
    s_fwd, s_fb = fwd_and_bwd(steady, beam)
    t_fwd, t_fb = fwd_and_bwd(transient, beam)
    print(json.dumps({"case": "single_kick", "particles": beam.particles.shape[0], "bins": M, "x_nodes": round(x_over_M * M, 2),
                      "dtype": str(beam.particles.dtype), "transient_fwd_us": round(t_fwd, 1), "transient_fwd_bwd_us": round(t_fb, 1),
                      "csr_fwd_us": round(s_fwd, 1), "csr_fwd_bwd_us": round(s_fb, 1), "fwd_ratio": round(t_fwd / s_fwd, 3),
                      "fwd_bwd_ratio": round(t_fb / s_fb, 3), "equals_csr_kick_bitwise": same}), flush=True)


def main():
    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, sigma_x=t(2e-4), sigma_y=t(1e-4), sigma_tau=t(1e-4),
                                           sigma_p=t(1e-3), total_charge=t(1e-9), **kw)
    for M, x_over_M in CASES:
        case(beam, M, x_over_M)


if __name__ == "__main__":
    main()
