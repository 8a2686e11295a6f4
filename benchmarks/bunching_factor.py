#!/usr/bin/env python3
"""Time ParticleBeam.bunching_factor (chx_bunching and its backward) on the GPU: 1e6 particles with K = 64 and K = 1024
wavelengths, float32 and float64 beams, forward and forward + backward, beside a chunked torch composition of the same
arithmetic on the same GPU in the same process (an outer product of tau and nu in float64, the fraction of the phase, sin and cos
in the beam's precision, a float64 weighted sum; row chunks of CHUNK_ROWS particles so that the phase matrix fits in memory).
Times are the mean over back-to-back calls between two device events. The arithmetic issue floor is the instruction mix of the
forward kernel's inner loop (counted in its ISA, per particle x wavelength pair and wave) at the issue rates of the MI355X: a
32-bit VALU instruction 2 cycles per wave, an instruction with a float64 operand 4. One JSON line per case."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402
from cheetah_amd import _ops  # noqa: E402

REPS = int(os.environ.get("BUNCHING_REPS", "20"))
TORCH_REPS = int(os.environ.get("BUNCHING_TORCH_REPS", "3"))
N = int(os.environ.get("BUNCHING_PARTICLES", "1000000"))
CHUNK_ROWS = 16384
SIMDS, CLOCK_HZ = 256 * 4, 2.4e9
#: (32-bit VALU, float64 VALU) instructions per pair and wave in bunching_partial_kernel's loop over four wavelengths per lane
MIX = {torch.float32: (26.5, 8.0), torch.float64: (20.5, 32.0)}


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def torch_chunk(tau, a, nu, dtype):
    t = tau.double()[:, None] * nu[None, :]
    f = (t - torch.round(t)).to(dtype)
    ang = (2.0 * math.pi) * f
    return a @ torch.cos(ang).double(), -(a @ torch.sin(ang).double())


def torch_forward(tau, a, nu, dtype):
    re = torch.zeros_like(nu)
    im = torch.zeros_like(nu)
    for n0 in range(0, tau.shape[0], CHUNK_ROWS):
        r, i = torch_chunk(tau[n0:n0 + CHUNK_ROWS], a[n0:n0 + CHUNK_ROWS], nu, dtype)
        re += r
        im += i
    return re, im, a.sum()


def torch_forward_backward(tau, w, q, nu, g, dtype):
    """The gradient of sum(g_re F_re + g_im F_im) chunk by chunk (the loss is linear in F, so every chunk backpropagates alone)."""
    tau.grad = w.grad = None
    for n0 in range(0, tau.shape[0], CHUNK_ROWS):
        sl = slice(n0, n0 + CHUNK_ROWS)
        r, i = torch_chunk(tau[sl], (w[sl] * q[sl]).double(), nu, dtype)
        ((r * g[:, 0]).sum() + (i * g[:, 1]).sum()).backward()


def case(dtype, K):
    kw = {"dtype": dtype, "device": "cuda"}
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=N, sigma_tau=torch.tensor(1e-4, **kw), **kw)
    x, w, q = beam.particles, beam.survival_probabilities, beam.particle_charges
    lam = torch.logspace(-6, -4, K, dtype=torch.float64, device="cuda")
    nu = 1.0 / lam
    g = torch.randn(K, 2, dtype=torch.float64, device="cuda")
    with torch.no_grad():
        fwd_us = timed(lambda: _ops.bunching(x, w, q, nu), REPS)
        api_us = timed(lambda: beam.bunching_factor(lam), REPS)
        tau, a = x[:, 4].contiguous(), (w * q).double()
        torch_fwd_us = timed(lambda: torch_forward(tau, a, nu, dtype), TORCH_REPS)
        # the two agree (the same arithmetic up to the evaluator and the order of the sums)
        F, Q = _ops.bunching(x, w, q, nu)
        re, im, Qt = torch_forward(tau, a, nu, dtype)
        diff = (torch.view_as_real(F / Q) - torch.stack([re, im], -1) / Qt).abs().max().item()
    xg, wg = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()

    def fwd_bwd():
        xg.grad = wg.grad = None
        F, _ = _ops.bunching(xg, wg, q, nu)
        (torch.view_as_real(F) * g).sum().backward()

    fb_us = timed(fwd_bwd, max(REPS // 2, 5))
    tg, wt = tau.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    torch_fb_us = timed(lambda: torch_forward_backward(tg, wt, q, nu, g, dtype), TORCH_REPS)
    b32, b64 = MIX[dtype]
    floor_us = N * K / 64 * (2 * b32 + 4 * b64) / (SIMDS * CLOCK_HZ) * 1e6
    print(json.dumps({"particles": N, "wavelengths": K, "dtype": str(dtype), "bunching_fwd_us": round(fwd_us, 1),
                      "bunching_factor_api_us": round(api_us, 1), "bunching_fwd_bwd_us": round(fb_us, 1),
                      "torch_fwd_us": round(torch_fwd_us, 1), "torch_fwd_bwd_us": round(torch_fb_us, 1),
                      "torch_over_kernel_fwd": round(torch_fwd_us / fwd_us, 1),
                      "torch_over_kernel_fwd_bwd": round(torch_fb_us / fb_us, 1),
                      "fwd_issue_floor_us": round(floor_us, 1), "fwd_share_of_issue_floor": round(floor_us / fwd_us, 3),
                      "gpairs_per_s_fwd": round(N * K / fwd_us * 1e-3, 1), "max_abs_diff_b": diff}), flush=True)


def main():
    for dtype in (torch.float32, torch.float64):
        for K in (64, 1024):
            case(dtype, K)


if __name__ == "__main__":
    main()
