#!/usr/bin/env python3
"""Time the LSCKick (chx_lsc_kick and its backward) on the GPU at 1e6 float32 particles and M = 500 and M = 4096 nodes: forward with
an explicit radius and with the radius taken from the beam (`beam_radius=None`: the beam's moments launch on top), forward +
backward, a plain torch composition of the same steps (amin / amax, scatter_add_, conv1d with the two-sided c^ table, gather) as the
yardstick, and the CSRKick on the same beam and M. Times are the mean over back-to-back calls between two events (launch-bound work
included). Run under `rocprofv3 --kernel-trace --stats` for the kernel durations. One JSON line per case."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("LSC_REPS", "100"))
K_E = 8.9875517923e9


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


def torch_lsc(x, q, w, factor, a_over_gamma, M):
    """The same kick composed of torch operations in the beam's dtype: the yardstick a user would otherwise write. `factor` =
    |Z| 2 k_e L / (gamma^2 p0c), so that S = factor / h^2."""
    dt = x.dtype
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
    dep = torch.zeros(M, dtype=dt, device=x.device)
    dep.scatter_add_(0, k, (1 - f) * c).scatter_add_(0, k + 1, f * c)
    rho = a_over_gamma / h
    j = torch.arange(-1, M + 1, dtype=dt, device=x.device)
    p = j / (j.abs() + torch.sqrt(j * j + rho * rho)) + torch.asinh(j / rho)
    ch = -0.5 * (p[2:] - 2 * p[1:-1] + p[:-2])
    full = torch.cat([-ch[1:].flip(0), ch])
    # V_k = sum_m full[(m - k) + M - 1] D_m: conv1d is a correlation, so the table goes in as it is over the padded deposit
    V = F.conv1d(F.pad(dep.view(1, 1, M), (M - 1, M - 1)), full.view(1, 1, 2 * M - 1)).view(M)
    node = factor / (h * h) * V
    out = x.clone()
    out[:, 5] += (1 - f) * node[k] + f * node[k + 1]
    return out


def single_kick(beam, M):
    x, q, w = beam.particles, beam.particle_charges, beam.survival_probabilities
    kw = {"dtype": x.dtype, "device": x.device}
    L = 2.0
    with torch.no_grad():
        a = float(0.85 * (beam.sigma_x + beam.sigma_y))
    gamma = float(beam.relativistic_gamma)
    lsc = ca.LSCKick(torch.tensor(L, **kw), torch.tensor(a, **kw), num_bins=M, **kw)
    lsc_auto = ca.LSCKick(torch.tensor(L, **kw), num_bins=M, **kw)
    csr = ca.CSRKick(torch.tensor(0.2, **kw), torch.tensor(0.02, **kw), num_bins=M, **kw)
    factor = 2 * K_E * L / (gamma ** 2 * float(beam.p0c))
    with torch.no_grad():
        fwd_us = timed(lambda: lsc.track(beam))
        auto_us = timed(lambda: lsc_auto.track(beam))
        csr_us = timed(lambda: csr.track(beam))
        torch_us = timed(lambda: torch_lsc(x, q, w, factor, a / gamma, M))
        ref = torch_lsc(x, q, w, factor, a / gamma, M)
        got = lsc.track(beam).particles
        agree = float(((got - ref).abs().max() / (ref - x).abs().max()).item())
    xg = x.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(xg, beam.energy, particle_charges=q, survival_probabilities=w)

    def fwd_bwd(elem):
        xg.grad = None
        elem.track(gb).particles[:, 5].square().sum().backward()

    fb_us = timed(lambda: fwd_bwd(lsc), reps=max(REPS // 2, 10))
    csr_fb_us = timed(lambda: fwd_bwd(csr), reps=max(REPS // 2, 10))
    print(json.dumps({"case": "single_kick", "particles": x.shape[0], "bins": M, "dtype": str(x.dtype),
                      "lsc_fwd_us": round(fwd_us, 1), "lsc_fwd_radius_from_beam_us": round(auto_us, 1),
                      "lsc_fwd_bwd_us": round(fb_us, 1), "csr_fwd_us": round(csr_us, 1), "csr_fwd_bwd_us": round(csr_fb_us, 1),
                      "torch_composition_us": round(torch_us, 1), "speedup_vs_torch": round(torch_us / fwd_us, 2),
                      "ratio_to_csr_fwd": round(fwd_us / csr_us, 2), "ratio_to_csr_fwd_bwd": round(fb_us / csr_fb_us, 2),
                      "max_rel_diff_vs_torch": agree}), flush=True)


def main():
    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, sigma_x=t(2e-4), sigma_y=t(1e-4), sigma_tau=t(1e-4),
                                           sigma_p=t(1e-3), total_charge=t(1e-9), **kw)
    for M in (500, 4096):
        single_kick(beam, M)


if __name__ == "__main__":
    main()
