#!/usr/bin/env python3
"""Time the LaserModulator (chx_laser_kick and its backward) on the GPU at 1e6 particles, float32 and float64, with and without a
pulse envelope: forward, forward + backward, a plain torch composition of the same formulas in float64 (the phase reduced in
turns, as a user who wants 10^4 turns right would have to write it) as the yardstick, and the project's own apply kernel
(`Drift.track`) on the same beam, which moves the same 56 (112) bytes per particle: the launch floor of a `track`. Times are the
mean over back-to-back calls between two events (launch-bound work included). Run under `rocprofv3 --kernel-trace --stats` for the
kernel durations. One JSON line per case."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("LASER_REPS", "100"))


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


def torch_laser(x, a, nu, phit, g, x0, y0, h, t0):
    """The same kick composed of torch operations, the phase and the envelope in float64, the result in the beam's dtype."""
    u, v, tau = x[:, 0].double() - x0, x[:, 2].double() - y0, x[:, 4].double()
    t = tau * nu + phit
    f = t - torch.round(t)
    w = tau - t0
    kick = a * torch.exp(-g * (u * u + v * v) - h * (w * w)) * torch.sin(2 * math.pi * f)
    out = x.clone()
    out[:, 5] += kick.to(x.dtype)
    return out


def case(dtype, envelope):
    kw = {"dtype": dtype, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, sigma_x=t(2e-4), sigma_y=t(1e-4), sigma_tau=t(3e-4),
                                           sigma_p=t(1e-5), energy=t(135e6), **kw)
    x = beam.particles
    settings = dict(amplitude=t(50e3), wavelength=t(8e-7), laser_sigma=t(1.75e-4), phase=t(0.3), offset_x=t(2e-5), offset_y=t(-1e-5),
                    pulse_sigma=t(2e-4) if envelope else None, pulse_center=t(1e-5))
    kick = ca.LaserModulator(**settings, **kw)
    drift = ca.Drift(t(0.5), **kw)
    factors = [float(v) for v in ca._ops.laser_factors(beam.energy, beam.species.mass_eV_float, settings["amplitude"],
                                                       settings["wavelength"], settings["phase"], settings["laser_sigma"],
                                                       settings["offset_x"], settings["offset_y"], settings["pulse_sigma"],
                                                       settings["pulse_center"])]
    with torch.no_grad():
        fwd_us = timed(lambda: kick.track(beam))
        apply_us = timed(lambda: drift.track(beam))
        torch_us = timed(lambda: torch_laser(x, *factors))
        out = kick.track(beam).particles
        rms_eV = float((out[:, 5] - x[:, 5]).double().std()) * float(beam.p0c)
        agree = float((out[:, 5].double() - torch_laser(x, *factors)[:, 5].double()).abs().max())
    xg = x.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(xg, beam.energy, particle_charges=beam.particle_charges, survival_probabilities=beam.survival_probabilities)

    def fwd_bwd():
        xg.grad = None
        kick.track(gb).particles[:, 5].square().sum().backward()

    def torch_fwd_bwd():
        xg.grad = None
        torch_laser(xg, *factors)[:, 5].square().sum().backward()

    fb_us = timed(fwd_bwd, reps=max(REPS // 2, 10))
    torch_fb_us = timed(torch_fwd_bwd, reps=max(REPS // 2, 10))
    print(json.dumps({"case": "single_kick", "particles": x.shape[0], "dtype": str(dtype), "envelope": envelope,
                      "laser_fwd_us": round(fwd_us, 1), "laser_fwd_bwd_us": round(fb_us, 1), "apply_kernel_us": round(apply_us, 1),
                      "fwd_over_apply": round(fwd_us / apply_us, 2), "torch_composition_us": round(torch_us, 1),
                      "torch_composition_fwd_bwd_us": round(torch_fb_us, 1), "speedup_vs_torch": round(torch_us / fwd_us, 2),
                      "rms_kick_eV": round(rms_eV, 1), "max_abs_difference_to_torch": agree}), flush=True)


def main():
    for dtype in (torch.float32, torch.float64):
        for envelope in (False, True):
            case(dtype, envelope)


if __name__ == "__main__":
    main()
