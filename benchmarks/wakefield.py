#!/usr/bin/env python3
"""Time the Wakefield kick (chx_wake_kick and its backward) on the GPU at 1e6 float32 particles and M = 1000 nodes, longitudinal
table only and both tables: forward, forward + backward, and a plain torch composition of the same steps (amin / amax,
scatter_add_, conv1d, gather) as the yardstick. Times are the mean over back-to-back calls between two events (launch-bound work
included). Run under `rocprofv3 --kernel-trace --stats` for the kernel durations. One JSON line per case."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("WAKE_REPS", "100"))


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


def torch_wake(x, q, w, scale, wl, wt, h, M):
    """The same kick composed of torch operations in the beam's dtype (float64 conv1d has no fast kernel here): the yardstick a
    user would otherwise write."""
    dt = x.dtype
    tau = x[:, 4]
    alive = (w > 0) & torch.isfinite(tau)
    inf = float("inf")
    lo = torch.where(alive, tau, inf).amin()
    hi = torch.where(alive, tau, -inf).amax()
    D = (hi - lo) / (M - 1)
    u = ((tau - lo) / D).clamp(0, M - 1)
    k = u.floor().clamp(max=M - 2).long()
    f = u - k
    c = torch.where(alive, q.abs() * w, 0.0)
    n = torch.arange(M, dtype=dt, device=x.device)

    def sample(T):
        p = n * D / h
        j = p.floor().clamp(0, T.numel() - 2).long()
        t = p - j
        Wn = torch.where(p <= T.numel() - 1, (1 - t) * T[j] + t * T[j + 1], 0.0)
        return Wn * torch.where(n == 0, 0.5, 1.0)

    chans = [c] if wt is None else [c, c * x[:, 0], c * x[:, 2]]
    dep = torch.zeros(len(chans), M, dtype=dt, device=x.device)
    for i, v in enumerate(chans):
        dep[i].scatter_add_(0, k, (1 - f) * v).scatter_add_(0, k + 1, f * v)
    kern = [sample(wl)] if wt is None else [sample(wl), sample(wt), sample(wt)]
    kern = torch.stack(kern).flip(-1).unsqueeze(1)                              # (C, 1, M) causal kernels
    grid = F.conv1d(F.pad(dep.unsqueeze(0), (M - 1, 0)), kern, groups=len(chans))[0]
    grid[0] = -grid[0]
    kick = (1 - f) * grid[:, k] + f * grid[:, k + 1]
    out = x.clone()
    out[:, 5] += scale * kick[0]
    if wt is not None:
        out[:, 1] += scale * kick[1]
        out[:, 3] += scale * kick[2]
    return out


def case(name, beam, wake):
    x, q, w = beam.particles, beam.particle_charges, beam.survival_probabilities
    wl = wake.longitudinal_wake
    wt = wake.transverse_wake if wake.transverse_wake.numel() else None
    h = wake.wake_spacing
    scale = float(wake.factor) / float(beam.p0c)
    with torch.no_grad():
        fwd_us = timed(lambda: wake.track(beam))
        torch_us = timed(lambda: torch_wake(x, q, w, scale, wl, wt, h, wake.num_bins))
        ref = torch_wake(x, q, w, scale, wl, wt, h, wake.num_bins)
        got = wake.track(beam).particles
        agree = float(((got - ref).abs().max() / (ref - x).abs().max()).item())
    xg = x.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(xg, beam.energy, particle_charges=q, survival_probabilities=w)

    def fwd_bwd():
        xg.grad = None
        out = wake.track(gb).particles
        (out[:, 5].sum() + out[:, 1].sum()).backward()

    fb_us = timed(fwd_bwd, reps=max(REPS // 2, 10))
    print(json.dumps({"case": name, "particles": x.shape[0], "bins": wake.num_bins, "dtype": str(x.dtype),
                      "wake_fwd_us": round(fwd_us, 1), "wake_fwd_bwd_us": round(fb_us, 1), "torch_composition_us": round(torch_us, 1),
                      "speedup_vs_torch": round(torch_us / fwd_us, 2), "max_rel_diff_vs_torch": agree}), flush=True)


def main():
    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, sigma_x=t(2e-4), sigma_y=t(1e-4), sigma_tau=t(2e-5),
                                           total_charge=t(1e-9), **kw)
    s = torch.linspace(0, 1, 400, **kw)
    wl, wt = 3e13 * torch.exp(-3 * s), 5e15 * s * torch.exp(-2 * s)
    h = t(5e-7)
    case("longitudinal", beam, ca.Wakefield(h, longitudinal_wake=wl, num_bins=1000, **kw))
    case("both", beam, ca.Wakefield(h, longitudinal_wake=wl, transverse_wake=wt, num_bins=1000, **kw))


if __name__ == "__main__":
    main()
