#!/usr/bin/env python3
"""Time the CSRDriftKick (chx_csr_drift_kick and its backward) next to the TransientCSRKick and the CSRKick on the same beam in the
same process: 1e6 float32 particles, M = 500 and 4096 nodes, a bend of radius 8 m whose radiation spans y = M / 8 nodes (the table
ends at lag y + 2: the sums stop there) and y = 2 M (every lag of the grid), at xh / phi = 1 (both branches of G) and 50 (the
series); forward and forward + backward. The transient kick runs at the same number of non-zero lags (4x = y). Times are the mean
over back-to-back calls between two events (launch-bound work included). Run under `rocprofv3 --kernel-trace --stats` for the
kernel durations; `CSRD_CASES=500:0.125:1` restricts the run to one (M, y / M, xh / phi) triple, so that a trace holds one table
length per kernel name. One JSON line per case."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("CSR_REPS", "100"))
CASES = [(int(m), float(r), float(x)) for m, r, x in (c.split(":") for c in os.environ.get(
    "CSRD_CASES", "500:0.125:1,500:2:1,500:2:50,4096:0.125:1,4096:2:1,4096:2:50").split(","))]
RADIUS = 8.0


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


def case(beam, M, y_over_M, ratio):
    kw = {"dtype": beam.particles.dtype, "device": beam.particles.device}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    L = 0.2
    tau = beam.particles[:, 4].double()
    h = float(tau.max() - tau.min()) / (M - 1)
    y = y_over_M * M
    phi = (24 * y * h * (1 + ratio) / (RADIUS * (1 + 4 * ratio))) ** (1 / 3)       # y = phi^3 (phi + 4 xh) / (kappa (phi + xh))
    d = (24 * RADIUS ** 2 * (y / 4) * h) ** (1 / 3)                                # the transient's 4x = y
    drift = ca.CSRDriftKick(t(L), t(RADIUS * phi), t(phi), t(ratio * phi * RADIUS), num_bins=M, **kw)
    transient = ca.TransientCSRKick(t(L), t(L / RADIUS), t(d), num_bins=M, **kw)
    steady = ca.CSRKick(t(L), t(L / RADIUS), num_bins=M, **kw)
    d_fwd, d_fb = fwd_and_bwd(drift, beam)
    t_fwd, t_fb = fwd_and_bwd(transient, beam)
    s_fwd, s_fb = fwd_and_bwd(steady, beam)
    print(json.dumps({"case": "single_kick", "particles": beam.particles.shape[0], "bins": M, "y_nodes": round(y, 2),
                      "xh_over_phi": ratio, "dtype": str(beam.particles.dtype), "drift_fwd_us": round(d_fwd, 1),
                      "drift_fwd_bwd_us": round(d_fb, 1), "transient_fwd_us": round(t_fwd, 1), "transient_fwd_bwd_us": round(t_fb, 1),
                      "csr_fwd_us": round(s_fwd, 1), "csr_fwd_bwd_us": round(s_fb, 1),
                      "fwd_minus_transient_us": round(d_fwd - t_fwd, 1)}), flush=True)


def main():
    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, sigma_x=t(2e-4), sigma_y=t(1e-4), sigma_tau=t(1e-4),
                                           sigma_p=t(1e-3), total_charge=t(1e-9), **kw)
    for M, y_over_M, ratio in CASES:
        case(beam, M, y_over_M, ratio)


if __name__ == "__main__":
    main()
