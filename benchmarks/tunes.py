#!/usr/bin/env python3
"""TurnByTurn.tunes on the records of the drift-kick-drift sextupole ring of benchmarks/track_turns_dkd_sextupole.py: 10^4
particles, all of them recorded, windows of T = 1024 and T = 4096 turns, x and y, float32 and float64 beams.

    python benchmarks/tunes.py [--particles 10000] [--windows 1024,4096] [--dtypes f32,f64] [--calls 50] [--torch-calls 5]

Per case the time of one call between two device events around back-to-back calls, after two warm-up calls:
  tunes     TurnByTurn.tunes(("x", "y")): one chx_tunes launch
  torch     the same definition composed of torch operations on the same GPU: the windowed, mean-removed rows zero-padded into one
            float64 torch.fft.rfft of 2 P points, argmax, the bracket rule and eight safeguarded Newton steps on every row at once
            (direct sums over the (rows, T) phases), the amplitude at the root
and the largest difference between the two results. One JSON line per case."""
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402
from benchmarks.track_turns_dkd_sextupole import ring_for  # noqa: E402

TWO_PI = 2 * math.pi


def sums(v, n, nu):
    """F, G, H (complex) of the rows v (M, T) at nu (M,): the phase reduced in turns."""
    t = nu[:, None] * n
    t = t - torch.floor(t)
    c, s = torch.cos(TWO_PI * t), torch.sin(TWO_PI * t)
    vn = v * n
    vnn = vn * n
    return (torch.complex((v * c).sum(1), -(v * s).sum(1)), torch.complex((vn * c).sum(1), -(vn * s).sum(1)),
            torch.complex((vnn * c).sum(1), -(vnn * s).sum(1)))


def torch_tunes(particles, lost, first, T, last_turn, steps=8):
    """(tune, amplitude), both (K, 2): x and y of particles (R, K, 7)."""
    K = particles.shape[1]
    u = particles[first:first + T, :, 0:3:2].to(torch.float64).permute(1, 2, 0).reshape(2 * K, T)
    n = torch.arange(T, dtype=torch.float64, device=u.device)
    w = torch.sin(math.pi * (n + 0.5) / T) ** 2
    sw = w.sum()
    v = w * (u - ((w * u).sum(1) / sw)[:, None])
    P = 2 * 2 ** math.ceil(math.log2(T))
    A = torch.fft.rfft(v, n=2 * P, dim=1).abs() ** 2            # (M, P + 1)
    ks = A.argmax(1)
    step = 1.0 / (2 * P)
    lo, hi = (ks - 1).clamp(0, P) * step, (ks + 1).clamp(0, P) * step
    slope = lambda F, G: F.real * G.imag - F.imag * G.real  # noqa: E731
    refine = (ks > 0) & (ks < P) & (slope(*sums(v, n, lo)[:2]) > 0) & (slope(*sums(v, n, hi)[:2]) < 0)
    x = ks * step
    for _ in range(steps):
        F, G, H = sums(v, n, x)
        g = slope(F, G)
        dg = TWO_PI * (G.abs() ** 2 - F.real * H.real - F.imag * H.imag)
        lo, hi = torch.where(g > 0, x, lo), torch.where(g > 0, hi, x)
        xn = x - g / dg
        ok = (dg < 0) & (xn >= lo) & (xn <= hi)
        x = torch.where(g == 0, x, torch.where(ok, xn, (lo + hi) / 2))
    nu = torch.where(refine, x, ks * step)
    amp = 2 * sums(v, n, nu)[0].abs() / sw
    dead = ((lost > 0) & (lost <= last_turn)).repeat_interleave(2) | ~torch.isfinite(u).all(1)
    nan = torch.full_like(nu, float("nan"))
    return torch.where(dead, nan, nu).reshape(K, 2), torch.where(dead, nan, amp).reshape(K, 2)


def event_time(fn, calls):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / calls


def main():
    opt = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    particles = int(float(opt("--particles", "10000")))
    windows = [int(v) for v in opt("--windows", "1024,4096").split(",")]
    dtypes = opt("--dtypes", "f32,f64").split(",")
    calls, torch_calls = int(opt("--calls", "50")), int(opt("--torch-calls", "5"))
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    for name in dtypes:
        dt = torch.float64 if name == "f64" else torch.float32
        ring = ring_for(dt, "mixed")
        torch.manual_seed(0)
        beam = ca.ParticleBeam.from_parameters(num_particles=particles, dtype=dt, device="cuda")
        tbt = ring.track_turns(beam, max(windows), record_first=particles)
        for T in windows:
            got = tbt.tunes(("x", "y"), 0, T)
            want = torch_tunes(tbt.particles, tbt.lost_turn, 0, T, T)
            live = ~torch.isnan(want[0])
            row = {"beam": name, "particles": particles, "T": T, "lost": int((tbt.lost_turn > 0).sum()),
                   "tunes_ms": round(event_time(lambda: tbt.tunes(("x", "y"), 0, T), calls), 4),
                   "torch_ms": round(event_time(lambda: torch_tunes(tbt.particles, tbt.lost_turn, 0, T, T), torch_calls), 3),
                   "same_nan": bool(torch.equal(torch.isnan(got.tune), ~live)),
                   "max_tune_difference": float((got.tune - want[0])[live].abs().max()),
                   "max_relative_amplitude_difference": float(((got.amplitude - want[1]) / want[1])[live].abs().max())}
            row["torch_over_tunes"] = round(row["torch_ms"] / row["tunes_ms"], 1)
            print(json.dumps(row), flush=True)
        del tbt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
