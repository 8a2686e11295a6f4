#!/usr/bin/env python3
"""Time the SynchrotronRadiationKick (chx_sr_kick and its backward) on the GPU at 1e6 particles, float32 and float64, with and
without quantum excitation: forward, forward + backward, a plain torch composition of the same formulas in the beam's dtype
(`torch.randn` for the deviates) as the yardstick a user would otherwise write, and the project's own apply kernel (`Drift.track`)
on the same beam, which moves the same 56 (112) bytes per particle. Times are the mean over back-to-back calls between two events
(launch-bound work included). Run under `rocprofv3 --kernel-trace --stats` for the kernel durations. One JSON line per case."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("SR_REPS", "100"))


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


def torch_sr(x, gamma0, P0, a, b, excite):
    """The same kick composed of torch operations in the beam's dtype."""
    g = gamma0 + x[:, 5] * P0
    pi = torch.sqrt(g * g - 1)
    g1 = g - a * P0**2 * pi * g
    if excite:
        g1 = g1 - torch.sqrt(b * P0**3 * g**7 / pi**3) * torch.randn_like(g)
    ratio = torch.sqrt(g1 * g1 - 1) / pi
    out = x.clone()
    out[:, 1] *= ratio
    out[:, 3] *= ratio
    out[:, 5] += (g1 - g) / P0
    return out


def case(dtype, excite):
    kw = {"dtype": dtype, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, sigma_x=t(2e-4), sigma_y=t(1e-4), sigma_tau=t(1e-4),
                                           sigma_p=t(1e-3), energy=t(5e9), **kw)
    x = beam.particles
    L, theta = 0.5, 0.05
    kick = ca.SynchrotronRadiationKick(t(L), t(theta), quantum_excitation=excite, **kw)
    drift = ca.Drift(t(L), **kw)
    species = beam.species
    gamma0, a, b = (float(v) for v in ca._ops.sr_factors(beam.energy, species.mass_eV_float, 1.0, t(L), t(theta)))
    P0 = float(beam.p0c) / species.mass_eV_float
    with torch.no_grad():
        fwd_us = timed(lambda: kick.track(beam))
        apply_us = timed(lambda: drift.track(beam))
        torch_us = timed(lambda: torch_sr(x, gamma0, P0, a, b, excite))
        out = kick.track(beam).particles
        mean_loss_eV = -float((out[:, 5] - x[:, 5]).double().mean()) * float(beam.p0c)
        rms_eV = float((out[:, 5] - x[:, 5]).double().std()) * float(beam.p0c)
    xg = x.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(xg, beam.energy, particle_charges=beam.particle_charges, survival_probabilities=beam.survival_probabilities)

    def fwd_bwd():
        xg.grad = None
        kick.track(gb).particles[:, 5].square().sum().backward()

    def torch_fwd_bwd():
        xg.grad = None
        torch_sr(xg, gamma0, P0, a, b, excite)[:, 5].square().sum().backward()

    fb_us = timed(fwd_bwd, reps=max(REPS // 2, 10))
    torch_fb_us = timed(torch_fwd_bwd, reps=max(REPS // 2, 10))
    print(json.dumps({"case": "single_kick", "particles": x.shape[0], "dtype": str(dtype), "quantum_excitation": excite,
                      "sr_fwd_us": round(fwd_us, 1), "sr_fwd_bwd_us": round(fb_us, 1), "apply_kernel_us": round(apply_us, 1),
                      "fwd_over_apply": round(fwd_us / apply_us, 2), "torch_composition_us": round(torch_us, 1),
                      "torch_composition_fwd_bwd_us": round(torch_fb_us, 1), "speedup_vs_torch": round(torch_us / fwd_us, 2),
                      "mean_loss_eV": round(mean_loss_eV, 1), "rms_eV": round(rms_eV, 1)}), flush=True)


def main():
    for dtype in (torch.float32, torch.float64):
        for excite in (True, False):
            case(dtype, excite)


if __name__ == "__main__":
    main()
