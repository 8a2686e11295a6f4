#!/usr/bin/env python3
"""Segment.track_turns on the drift-kick-drift FODO ring of benchmarks/track_turns_dkd.py with a Sextupole of several steps behind
each quadrupole: 25 x [Quadrupole 0.2 m k1 = 4.2, Sextupole 0.1 m k2 = 10 (num_steps = 3), Drift 0.7 m, Quadrupole k1 = -4.2,
Sextupole k2 = -10, Drift 0.7 m] = 150 items, every element `tracking_method="drift_kick_drift"`; 1000 turns at 1e3, 1e5 and 1e6
particles, every turn recorded; float32 beams in "mixed", "double" and "storage" arithmetic, and float64.

    python benchmarks/track_turns_dkd_sextupole.py [turns] [--sizes 1e3,1e5,1e6] [--repeat 3] [--modes mixed,double,storage,f64]

Per case, wall time of one call (synchronised before and after; one warm-up call of each, then the variants timed in turn for
`repeat` rounds, the best of each kept):
  fused     track_turns(fused=True): chx_dkd_turns, the turn loop in the kernel
  loop      for _ in range(turns): beam = ring.track(beam) — one chx_dkd_chain_mixed call per turn, no records
and whether the two leave the same bits. One JSON line per case."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402
from benchmarks.track_turns_dkd import timed  # noqa: E402

CELLS = 25
ITEMS = 6 * CELLS


def ring_for(dt, precision, num_steps=3):
    kw = {"dtype": dt, "device": "cuda"}
    tt = lambda v: torch.tensor(v, **kw)  # noqa: E731
    dkd = {"tracking_method": "drift_kick_drift"}
    els = []
    for _ in range(CELLS):
        els += [ca.Quadrupole(tt(0.2), k1=tt(4.2), **dkd, **kw), ca.Sextupole(tt(0.1), k2=tt(10.0), num_steps=num_steps, **dkd, **kw),
                ca.Drift(tt(0.7), **dkd, **kw),
                ca.Quadrupole(tt(0.2), k1=tt(-4.2), **dkd, **kw), ca.Sextupole(tt(0.1), k2=tt(-10.0), num_steps=num_steps, **dkd, **kw),
                ca.Drift(tt(0.7), **dkd, **kw)]
    for e in els:
        e.dkd_precision = precision
    return ca.Segment(els)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    turns = int(args[0]) if args else 1000
    sizes = [int(float(v)) for v in opt("--sizes", "1e3,1e5,1e6").split(",")]
    repeat = int(opt("--repeat", "3"))
    modes = opt("--modes", "mixed,double,storage,f64").split(",")
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    for mode in modes:
        dt = torch.float64 if mode == "f64" else torch.float32
        ring = ring_for(dt, "mixed" if mode == "f64" else mode)
        for n in sizes:
            torch.manual_seed(0)
            beam = ca.ParticleBeam.from_parameters(num_particles=n, dtype=dt, device="cuda")

            def loop():
                b = beam
                with torch.no_grad():
                    for _ in range(turns):
                        b = ring.track(b)
                return b

            variants = {"fused": lambda: ring.track_turns(beam, turns, fused=True), "loop": loop}
            best = {}
            for fn in variants.values():                           # warm-up: code objects, allocator, the segment's caches
                fn()
            torch.cuda.synchronize()
            for _ in range(repeat):
                for name, fn in variants.items():
                    best[name] = min(best.get(name, float("inf")), timed(fn))
            row = {"mode": mode, "particles": n, "turns": turns, "items": ITEMS}
            for name in variants:
                row[f"{name}_ms"] = round(best[name] * 1e3, 3)
            row["fused_ns_per_item_step"] = round(row["fused_ms"] * 1e6 / (turns * ITEMS), 2)
            row["loop_over_fused"] = round(row["loop_ms"] / row["fused_ms"], 2)
            tbt, want = ring.track_turns(beam, turns, fused=True), loop()
            row["lost"] = int((tbt.lost_turn > 0).sum())
            row["same_bits_as_loop"] = bool(torch.equal(tbt.outgoing.particles, want.particles) and
                                            torch.equal(tbt.outgoing.energy, want.energy)) if row["lost"] == 0 else None
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
