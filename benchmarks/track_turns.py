#!/usr/bin/env python3
"""Segment.track_turns on the README's 100-element second-order FODO taken as a ring: 1000 turns at 1e3, 1e5 and 1e6 particles,
float32 and float64, every turn recorded (record_every=1).

    python benchmarks/track_turns.py [turns] [--sizes 1e3,1e5,1e6]

Per case, wall time of one call (best of three, after a warm-up call; synchronised before and after):
  fused     track_turns(fused=True): the turn kernel, chunked launches, records from the kernel
  general   track_turns(fused=False): the loop over Segment.track with the records as float64 torch operations
  loop      for _ in range(turns): beam = ring.track(beam) — no records at all (what a user could write before; also runs on a
            checkout without track_turns, where it is the only case)
and the fused call's WALL time per item step (turns x 100 items) — no kernel trace: at 1e6 particles the turn kernel dominates the
call (the two other launches of a chunk take microseconds), below that the figure is an upper bound on the kernel's duration per
step. One JSON line per case."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402


def ring_for(dt):
    kw = {"dtype": dt, "device": "cuda"}
    tt = lambda v: torch.tensor(v, **kw)  # noqa: E731
    so = {"tracking_method": "second_order"}
    els = []
    for _ in range(25):
        els += [ca.Quadrupole(tt(0.2), k1=tt(4.2), **so, **kw), ca.Drift(tt(0.8), **so, **kw),
                ca.Quadrupole(tt(0.2), k1=tt(-4.2), **so, **kw), ca.Drift(tt(0.8), **so, **kw)]
    return ca.Segment(els)


def best_of(fn, repeat=3):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    turns = int(args[0]) if args else 1000
    sizes = [1e3, 1e5, 1e6]
    if "--sizes" in sys.argv:
        sizes = [float(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(",")]
    has_turns = hasattr(ca.Segment, "track_turns")
    for dt in (torch.float32, torch.float64):
        ring = ring_for(dt)
        for n in sizes:
            n = int(n)
            torch.manual_seed(0)
            beam = ca.ParticleBeam.from_parameters(num_particles=n, dtype=dt, device="cuda")

            def loop():
                b = beam
                with torch.no_grad():
                    for _ in range(turns):
                        b = ring.track(b)
                return b

            row = {"dtype": str(dt).replace("torch.", ""), "particles": n, "turns": turns, "items": 100,
                   "loop_ms": round(best_of(loop) * 1e3, 3)}
            if has_turns:
                row["fused_ms"] = round(best_of(lambda: ring.track_turns(beam, turns, fused=True)) * 1e3, 3)
                row["general_ms"] = round(best_of(lambda: ring.track_turns(beam, turns, fused=False), repeat=2) * 1e3, 3)
                row["fused_ns_per_item_step"] = round(row["fused_ms"] * 1e6 / (turns * 100), 2)
                row["fused_over_loop"] = round(row["loop_ms"] / row["fused_ms"], 2)
                row["fused_over_general"] = round(row["general_ms"] / row["fused_ms"], 2)
                tbt = ring.track_turns(beam, turns, fused=True)
                row["lost"] = int((tbt.lost_turn > 0).sum())
                row["same_bits_as_loop"] = bool(torch.equal(tbt.outgoing.particles, loop().particles)) if row["lost"] == 0 else None
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
