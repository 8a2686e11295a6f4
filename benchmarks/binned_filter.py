#!/usr/bin/env python3
"""Time the low-pass filter of the binned-beam kicks (`cutoff_wavelength`) on the GPU: LSCKick and CSRKick at 1e6 float32 particles and
M = 500 and M = 4096 nodes, without a cutoff and with cutoffs of about s = 2 and s = 20 node spacings, forward and forward + backward.
Times are the mean over back-to-back calls between two events (launch-bound work included), the three settings of a case taken in
alternating rounds; the stage's own cost is the difference to the unfiltered kick. Run under `rocprofv3 --kernel-trace --stats` for
the kernel durations (grid_filter_kernel against the kicks' node passes lsc_toeplitz_kernel / csr_toeplitz_kernel). Then the point of
the filter: the rms difference between the LSC kicks at M = 512 and M = 4096, with and without a cutoff of 8 node spacings of the
M = 512 grid. One JSON line per case."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("FILTER_REPS", "100"))
ROUNDS = int(os.environ.get("FILTER_ROUNDS", "3"))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def alternating(fns, reps):
    """The best of ROUNDS rounds for every function, the functions taking turns within a round (microseconds per call)."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    best = {name: math.inf for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            best[name] = min(best[name], timed(fn, reps))
    return best


def make(kind, M, cutoff, kw):
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    c = {} if cutoff is None else {"cutoff_wavelength": t(cutoff)}
    if kind == "lsc":
        return ca.LSCKick(t(2.0), t(2.5e-4), num_bins=M, **c, **kw)
    return ca.CSRKick(t(0.2), t(0.02), num_bins=M, **c, **kw)


def timing_case(kind, beam, M, h):
    kw = {"dtype": beam.particles.dtype, "device": beam.particles.device}
    elems = {"off": make(kind, M, None, kw), "s2": make(kind, M, 2 * math.pi * 2.0 * h, kw), "s20": make(kind, M, 2 * math.pi * 20.0 * h, kw)}
    with torch.no_grad():
        fwd = alternating({name: (lambda e=e: e.track(beam)) for name, e in elems.items()}, REPS)
    xg = beam.particles.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(xg, beam.energy, particle_charges=beam.particle_charges, survival_probabilities=beam.survival_probabilities)

    def fwd_bwd(elem):
        xg.grad = None
        elem.track(gb).particles[:, 5].square().sum().backward()

    both = alternating({name: (lambda e=e: fwd_bwd(e)) for name, e in elems.items()}, max(REPS // 2, 10))
    row = {"case": "timing", "kick": kind, "particles": beam.particles.shape[0], "bins": M, "dtype": str(beam.particles.dtype)}
    for name in elems:
        row[f"fwd_{name}_us"] = round(fwd[name], 1)
        row[f"fwd_bwd_{name}_us"] = round(both[name], 1)
    for name in ("s2", "s20"):
        row[f"fwd_{name}_minus_off_us"] = round(fwd[name] - fwd["off"], 1)
        row[f"fwd_bwd_{name}_minus_off_us"] = round(both[name] - both["off"], 1)
    print(json.dumps(row), flush=True)


def convergence_case(beam, h512):
    kw = {"dtype": beam.particles.dtype, "device": beam.particles.device}
    row = {"case": "convergence", "kick": "lsc", "particles": beam.particles.shape[0], "dtype": str(beam.particles.dtype),
           "cutoff_in_spacings_of_512": 8}
    with torch.no_grad():
        for name, cutoff in (("unfiltered", None), ("filtered", 8 * h512)):
            kicks = [(make("lsc", M, cutoff, kw).track(beam).particles[:, 5] - beam.particles[:, 5]).double() for M in (512, 4096)]
            row[f"rms_kick_4096_{name}"] = float(kicks[1].square().mean().sqrt())
            row[f"rms_difference_512_4096_{name}"] = float((kicks[1] - kicks[0]).square().mean().sqrt())
    row["ratio"] = row["rms_difference_512_4096_filtered"] / row["rms_difference_512_4096_unfiltered"]
    print(json.dumps(row), flush=True)


def main():
    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, sigma_x=t(2e-4), sigma_y=t(1e-4), sigma_tau=t(1e-4),
                                           sigma_p=t(1e-3), total_charge=t(1e-9), **kw)
    tau = beam.particles[:, 4].double()
    extent = float(tau.max() - tau.min())
    for kind in ("lsc", "csr"):
        for M in (500, 4096):
            timing_case(kind, beam, M, extent / (M - 1))
    convergence_case(beam, extent / 511)
    # the same particles as a float64 beam: the difference that is left is not float32 rounding
    beam64 = ca.ParticleBeam(beam.particles.double(), beam.energy.double(), particle_charges=beam.particle_charges.double(),
                             survival_probabilities=beam.survival_probabilities.double())
    convergence_case(beam64, extent / 511)


if __name__ == "__main__":
    main()
