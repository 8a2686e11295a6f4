#!/usr/bin/env python3
"""Time the IBSKick (chx_ibs_kick and its backward) on the GPU at 1e6 particles, M = 500 and M = 4096 nodes, float32 and float64
beams: forward with explicit moments and with the four moments taken from the beam (the beam's moments launch on top), forward +
backward, the LSCKick and the SynchrotronRadiationKick on the same beam, and a plain torch composition of the same steps (amin /
amax, scatter_add_, gather, randn_like) as the yardstick. Times are the mean over back-to-back calls between two events (launch-bound
work included). Run under `rocprofv3 --kernel-trace --stats` for the kernel durations. One JSON line per case."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("IBS_REPS", "100"))


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


def torch_ibs(x, q, w, K, M):
    """The same kick composed of torch operations in the beam's dtype: the yardstick a user would otherwise write. `K`: the
    strength, so that the node variance is K D_k / h."""
    tau = x[:, 4]
    alive = (w > 0) & torch.isfinite(tau)
    inf = float("inf")
    lo = torch.where(alive, tau, inf).amin()
    hi = torch.where(alive, tau, -inf).amax()
    h = (hi - lo) / (M - 1)
    u = ((tau - lo) / h).clamp(0, M - 1)
    k = u.floor().clamp(max=M - 2).long()
    f = u - k
    c = torch.where(alive, q.abs() * w, 0.0)
    dep = torch.zeros(M, dtype=x.dtype, device=x.device)
    dep.scatter_add_(0, k, (1 - f) * c).scatter_add_(0, k + 1, f * c)
    node = K / h * dep
    out = x.clone()
    out[:, 5] += torch.sqrt((1 - f) * node[k] + f * node[k + 1]) * torch.randn_like(tau)
    return out


def single_kick(beam, M):
    x, q, w = beam.particles, beam.particle_charges, beam.survival_probabilities
    kw = {"dtype": x.dtype, "device": x.device}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    L = 10.0
    with torch.no_grad():
        moments = {n: getattr(beam, n).clone() for n in ("sigma_x", "sigma_y", "emittance_x", "emittance_y")}
    ibs = ca.IBSKick(t(L), **moments, num_bins=M, **kw)
    ibs_auto = ca.IBSKick(t(L), num_bins=M, **kw)
    lsc = ca.LSCKick(t(L), t(2e-4), num_bins=M, **kw)
    sr = ca.SynchrotronRadiationKick(t(0.5), t(0.05), **kw)
    species = beam.species
    with torch.no_grad():
        K = float(ca._ops.ibs_strength(beam.energy, species.mass_eV_float, 1.0, t(L), ibs.coulomb_log, *moments.values(),
                                       torch.ones((), dtype=torch.float64, device=x.device)))
        fwd_us = timed(lambda: ibs.track(beam))
        auto_us = timed(lambda: ibs_auto.track(beam))
        lsc_us = timed(lambda: lsc.track(beam))
        sr_us = timed(lambda: sr.track(beam))
        torch_us = timed(lambda: torch_ibs(x, q, w, K, M))
        # the composition draws other deviates: compare the variances the two add
        got = (ibs.track(beam).particles[:, 5] - x[:, 5]).double().var()
        ref = (torch_ibs(x, q, w, K, M)[:, 5] - x[:, 5]).double().var()
    xg = x.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(xg, beam.energy, particle_charges=q, survival_probabilities=w)

    def fwd_bwd(elem):
        xg.grad = None
        elem.track(gb).particles[:, 5].square().sum().backward()

    fb_us = timed(lambda: fwd_bwd(ibs), reps=max(REPS // 2, 10))
    lsc_fb_us = timed(lambda: fwd_bwd(lsc), reps=max(REPS // 2, 10))
    print(json.dumps({"case": "single_kick", "particles": x.shape[0], "bins": M, "dtype": str(x.dtype),
                      "ibs_fwd_us": round(fwd_us, 1), "ibs_fwd_moments_from_beam_us": round(auto_us, 1),
                      "ibs_fwd_bwd_us": round(fb_us, 1), "lsc_fwd_us": round(lsc_us, 1), "lsc_fwd_bwd_us": round(lsc_fb_us, 1),
                      "sr_fwd_us": round(sr_us, 1), "torch_composition_us": round(torch_us, 1),
                      "speedup_vs_torch": round(torch_us / fwd_us, 2), "ratio_to_lsc_fwd": round(fwd_us / lsc_us, 2),
                      "ratio_to_lsc_fwd_bwd": round(fb_us / lsc_fb_us, 2), "added_variance": float(got),
                      "added_variance_torch": float(ref)}), flush=True)


def main():
    for dtype in (torch.float32, torch.float64):
        kw = {"dtype": dtype, "device": "cuda"}
        t = lambda v: torch.tensor(v, **kw)  # noqa: E731
        torch.manual_seed(0)
        beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, sigma_x=t(1e-4), sigma_y=t(1e-4), sigma_px=t(1e-5),
                                               sigma_py=t(1e-5), sigma_tau=t(3e-5), sigma_p=t(1e-4), energy=t(2.555e8),
                                               total_charge=t(2.5e-10), **kw)
        for M in (500, 4096):
            single_kick(beam, M)


if __name__ == "__main__":
    main()
