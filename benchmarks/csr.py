#!/usr/bin/env python3
"""Time the CSRKick (chx_csr_kick and its backward) on the GPU at 1e6 float32 particles and M = 500 nodes: forward, forward +
backward, and a plain torch composition of the same steps (amin / amax, scatter_add_, conv1d with the b table, gather) as the
yardstick; then `Segment.track` through a four-dipole chicane split into 10 pieces with CSR kicks per bend, against the same
chicane without kicks. Times are the mean over back-to-back calls between two events (launch-bound work included). Run under
`rocprofv3 --kernel-trace --stats` for the kernel durations. One JSON line per case."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

REPS = int(os.environ.get("CSR_REPS", "100"))
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


def torch_csr(x, q, w, scale, M):
    """The same kick composed of torch operations in the beam's dtype: the yardstick a user would otherwise write. `scale` =
    |Z| L^(1/3) |theta|^(2/3) / p0c."""
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
    j = torch.arange(M, dtype=dt, device=x.device)
    a = (j + 1).pow(2 / 3) - j.pow(2 / 3)
    b = torch.cat([-torch.ones(1, dtype=dt, device=x.device), a[:-1] - a[1:]])
    # S_k = sum_j b_j D_(k+j): conv1d is a correlation, so the anti-causal sum takes b as it is over the right-padded deposit
    S = F.conv1d(F.pad(dep.view(1, 1, M), (0, M - 1)), b.view(1, 1, M)).view(M)
    node = (9 ** (1 / 3) * K_E) * h.pow(-4 / 3) * S
    out = x.clone()
    out[:, 5] += scale * ((1 - f) * node[k] + f * node[k + 1])
    return out


def single_kick(beam):
    x, q, w = beam.particles, beam.particle_charges, beam.survival_probabilities
    kw = {"dtype": x.dtype, "device": x.device}
    L, theta, M = 0.2, 0.02, 500
    csr = ca.CSRKick(torch.tensor(L, **kw), torch.tensor(theta, **kw), num_bins=M, **kw)
    scale = L ** (1 / 3) * theta ** (2 / 3) / float(beam.p0c)
    with torch.no_grad():
        fwd_us = timed(lambda: csr.track(beam))
        torch_us = timed(lambda: torch_csr(x, q, w, scale, M))
        ref = torch_csr(x, q, w, scale, M)
        got = csr.track(beam).particles
        agree = float(((got - ref).abs().max() / (ref - x).abs().max()).item())
    xg = x.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(xg, beam.energy, particle_charges=q, survival_probabilities=w)

    def fwd_bwd():
        xg.grad = None
        csr.track(gb).particles[:, 5].square().sum().backward()

    fb_us = timed(fwd_bwd, reps=max(REPS // 2, 10))
    print(json.dumps({"case": "single_kick", "particles": x.shape[0], "bins": M, "dtype": str(x.dtype),
                      "csr_fwd_us": round(fwd_us, 1), "csr_fwd_bwd_us": round(fb_us, 1), "torch_composition_us": round(torch_us, 1),
                      "speedup_vs_torch": round(torch_us / fwd_us, 2), "max_rel_diff_vs_torch": agree}), flush=True)


def chicane(beam, kicks_per_bend=10):
    kw = {"dtype": beam.particles.dtype, "device": beam.particles.device}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    theta, Lb = 0.05, 0.5
    seg = ca.Segment([ca.Dipole(t(Lb), angle=t(theta), dipole_e2=t(theta), **kw), ca.Drift(t(2.0), **kw),
                      ca.Dipole(t(Lb), angle=t(-theta), dipole_e1=t(-theta), **kw), ca.Drift(t(0.5), **kw),
                      ca.Dipole(t(Lb), angle=t(-theta), dipole_e2=t(-theta), **kw), ca.Drift(t(2.0), **kw),
                      ca.Dipole(t(Lb), angle=t(theta), dipole_e1=t(theta), **kw)])
    split = seg.with_csr_kicks(kicks_per_bend, num_bins=500)
    with torch.no_grad():
        plain_us = timed(lambda: seg.track(beam), reps=max(REPS // 4, 10))
        csr_us = timed(lambda: split.track(beam), reps=max(REPS // 4, 10))
        out = split.track(beam)
    print(json.dumps({"case": "chicane", "particles": beam.particles.shape[0], "bins": 500, "dtype": str(beam.particles.dtype),
                      "bends": 4, "kicks": 4 * kicks_per_bend, "track_us": round(csr_us, 1), "track_without_csr_us": round(plain_us, 1),
                      "per_kick_us": round((csr_us - plain_us) / (4 * kicks_per_bend), 1),
                      "sigma_p_out": float(out.sigma_p)}), flush=True)


def main():
    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=1_000_000, sigma_x=t(2e-4), sigma_y=t(1e-4), sigma_tau=t(1e-4),
                                           sigma_p=t(1e-3), total_charge=t(1e-9), **kw)
    single_kick(beam)
    chicane(beam)


if __name__ == "__main__":
    main()
