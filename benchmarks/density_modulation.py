#!/usr/bin/env python3
"""Time `ParticleBeam.with_density_modulation` (chx_density_modulate and its backward) on the GPU at 1e6 particles, float32 and
float64, one and three modes: forward, forward + backward, a torch composition of the same map in float64 (an unrolled Newton
iteration of eight steps without a safeguard, the phase reduced in turns: what a user would write) as the yardstick, and the
project's own apply kernel (`Drift.track`) on the same beam, which moves the same 56 (112) bytes per particle: the launch floor of a
particle pass. Times are the mean over back-to-back calls between two events (launch-bound work included). One JSON line per case."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("DENSITY_REPS", "50"))
SIGMA_TAU = 1e-4
NEWTON_STEPS = 8


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


def torch_modulation(x, A, lam, phi):
    """The same map composed of torch operations: plain Newton from tau' = tau, unrolled, in float64."""
    nu, phit = 1 / lam, phi / (2 * math.pi)
    c = A / (2 * math.pi * nu)
    tau = x[:, 4].double()
    t = tau
    for _ in range(NEWTON_STEPS):
        w = t[:, None] * nu + phit
        f = w - torch.round(w)
        g = t + (c * torch.sin(2 * math.pi * f)).sum(-1) - tau
        D = 1 + (A * torch.cos(2 * math.pi * f)).sum(-1)
        t = t - g / D
    out = x.clone()
    out[:, 4] = t.to(x.dtype)
    return out


def case(dtype, modes, report=True):
    kw = {"dtype": dtype, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    d64 = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")  # noqa: E731
    beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, sigma_tau=t(SIGMA_TAU), quiet_start=True, **kw)
    x = beam.particles
    lam = d64([SIGMA_TAU / 20, SIGMA_TAU / 7, SIGMA_TAU / 45][:modes])
    A = d64([0.02, 0.05, 0.03][:modes])
    phi = d64([0.7, -2.0, 3.0][:modes])
    drift = ca.Drift(t(0.5), **kw)
    with torch.no_grad():
        fwd_us = timed(lambda: beam.with_density_modulation(lam, A, phi))
        apply_us = timed(lambda: drift.track(beam))
        torch_us = timed(lambda: torch_modulation(x, A, lam, phi), reps=max(REPS // 5, 5))
        out = beam.with_density_modulation(lam, A, phi)
        agree = float(((out.particles[:, 4].double() - torch_modulation(x, A, lam, phi)[:, 4].double()).abs() / lam.min()).max())
        b = out.bunching_factor(lam)
        b_err = float((b - A / 2 * torch.exp(1j * phi)).abs().max())
    xg = x.detach().clone().requires_grad_()
    Ag = A.clone().requires_grad_()
    gb = ca.ParticleBeam(xg, beam.energy, particle_charges=beam.particle_charges, survival_probabilities=beam.survival_probabilities)

    def fwd_bwd():
        xg.grad = Ag.grad = None
        gb.with_density_modulation(lam, Ag, phi).particles[:, 4].square().sum().backward()

    def torch_fwd_bwd():
        xg.grad = Ag.grad = None
        torch_modulation(xg, Ag, lam, phi)[:, 4].square().sum().backward()

    fb_us = timed(fwd_bwd, reps=max(REPS // 2, 10))
    torch_fb_us = timed(torch_fwd_bwd, reps=max(REPS // 5, 5))
    if not report:
        return
    print(json.dumps({"case": "density_modulation", "particles": x.shape[0], "dtype": str(dtype), "modes": modes,
                      "fwd_us": round(fwd_us, 1), "fwd_bwd_us": round(fb_us, 1), "apply_kernel_us": round(apply_us, 1),
                      "fwd_over_apply": round(fwd_us / apply_us, 2), "torch_composition_us": round(torch_us, 1),
                      "torch_composition_fwd_bwd_us": round(torch_fb_us, 1), "speedup_vs_torch": round(torch_us / fwd_us, 2),
                      "speedup_fwd_bwd_vs_torch": round(torch_fb_us / fb_us, 2),
                      "max_difference_to_torch_in_wavelengths": agree, "max_bunching_error": b_err}), flush=True)


def main():
    case(torch.float32, 1, report=False)      # discarded: the first case of a process pays for what the later ones find in place
    for dtype in (torch.float32, torch.float64):
        for modes in (1, 3):
            case(dtype, modes)


if __name__ == "__main__":
    main()
