#!/usr/bin/env python3
"""Segment.track_turns on the sextupole ring with an RFCavity of benchmarks/track_turns_dkd_rfcavity.py with a thin octupole
(`Multipole(0, order 3, knl = 50 m^-3)`, alternating in sign) behind each Sextupole: 23 cells, 185 items with the octupoles (the
fused ring takes 192), 139 without; every element `tracking_method="drift_kick_drift"`; 1000 turns at 1e3, 1e5 and 1e6
particles, every turn recorded; float32 beams in "mixed", "double" and "storage" arithmetic, and float64.

    python benchmarks/track_turns_dkd_multipole.py [turns] [--sizes 1e3,1e5,1e6] [--repeat 3] [--modes mixed,double,storage,f64]
                                                   [--variants fused,fused_plain,loop]

Per case, wall time of one call (synchronised before and after; one warm-up call of each, then the variants timed in turn for
`repeat` rounds, the best of each kept):
  fused        track_turns(fused=True) on the ring with the octupoles: chx_dkd_turns, the kernel with every kind compiled in
  fused_plain  the same on the ring without them: the kernel a ring with a cavity ran before the Multipole existed
               (`--variants fused_plain` is what a build of the parent commit can run)
  loop         for _ in range(turns): beam = ring.track(beam) on the ring with the octupoles — one chx_dkd_chain_mixed call per turn
and whether the fused call leaves the loop's bits, and the same bits when called twice. One JSON line per case."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402
from benchmarks.track_turns_dkd import timed  # noqa: E402

CELLS = 23
ITEMS = 8 * CELLS + 1
PLAIN_ITEMS = 6 * CELLS + 1


def ring_for(dt, precision, octupoles=True):
    kw = {"dtype": dt, "device": "cuda"}
    tt = lambda v: torch.tensor(v, **kw)  # noqa: E731
    dkd = {"tracking_method": "drift_kick_drift"}
    els = []
    for cell in range(CELLS):
        last = cell == CELLS - 1
        for k1, k2, k3l in ((4.2, 10.0, 50.0), (-4.2, -10.0, -50.0)):
            els.append(ca.Quadrupole(tt(0.2), k1=tt(k1), **dkd, **kw))
            els.append(ca.Sextupole(tt(0.1), k2=tt(k2), num_steps=3, **dkd, **kw))
            if octupoles:
                els.append(ca.Multipole(tt(0.0), 3, knl=tt(k3l), **kw))
            if last and k1 < 0:
                els.append(ca.Drift(tt(0.4), **dkd, **kw))
                els.append(ca.RFCavity(tt(0.3), voltage=tt(1e5), phase=tt(0.0), frequency=tt(480e6), **kw))
            else:
                els.append(ca.Drift(tt(0.7), **dkd, **kw))
    for e in els:
        e.dkd_precision = precision
    assert len(els) == (ITEMS if octupoles else PLAIN_ITEMS)
    return ca.Segment(els)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    turns = int(args[0]) if args else 1000
    sizes = [int(float(v)) for v in opt("--sizes", "1e3,1e5,1e6").split(",")]
    repeat = int(opt("--repeat", "3"))
    modes = opt("--modes", "mixed,double,storage,f64").split(",")
    chosen = opt("--variants", "fused,fused_plain,loop").split(",")
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    for mode in modes:
        dt = torch.float64 if mode == "f64" else torch.float32
        precision = "mixed" if mode == "f64" else mode
        ring, plain = ring_for(dt, precision), ring_for(dt, precision, octupoles=False)
        for n in sizes:
            torch.manual_seed(0)
            beam = ca.ParticleBeam.from_parameters(num_particles=n, dtype=dt, device="cuda")

            def loop():
                b = beam
                with torch.no_grad():
                    for _ in range(turns):
                        b = ring.track(b)
                return b

            variants = {"fused": lambda: ring.track_turns(beam, turns, fused=True),
                        "fused_plain": lambda: plain.track_turns(beam, turns, fused=True), "loop": loop}
            variants = {k: v for k, v in variants.items() if k in chosen}
            best = {}
            for fn in variants.values():                           # warm-up: code objects, allocator, the segment's caches
                fn()
            torch.cuda.synchronize()
            for _ in range(repeat):
                for name, fn in variants.items():
                    best[name] = min(best.get(name, float("inf")), timed(fn))
            row = {"mode": mode, "particles": n, "turns": turns, "items": ITEMS, "plain_items": PLAIN_ITEMS}
            for name in variants:
                row[f"{name}_ms"] = round(best[name] * 1e3, 3)
            if "fused" in variants:
                row["fused_ns_per_item_step"] = round(row["fused_ms"] * 1e6 / (turns * ITEMS), 2)
            if "fused_plain" in variants:
                row["plain_ns_per_item_step"] = round(row["fused_plain_ms"] * 1e6 / (turns * PLAIN_ITEMS), 2)
            if "fused" in variants and "loop" in variants:
                row["loop_over_fused"] = round(row["loop_ms"] / row["fused_ms"], 2)
                tbt, again, want = ring.track_turns(beam, turns, fused=True), ring.track_turns(beam, turns, fused=True), loop()
                row["lost"] = int((tbt.lost_turn > 0).sum())
                row["same_bits_as_loop"] = bool(torch.equal(tbt.outgoing.particles, want.particles) and
                                                torch.equal(tbt.outgoing.energy, want.energy)) if row["lost"] == 0 else None
                row["same_bits_twice"] = bool(torch.equal(tbt.outgoing.particles.view(torch.uint8), again.outgoing.particles.view(torch.uint8))
                                              and torch.equal(tbt.sums.view(torch.uint8), again.sums.view(torch.uint8))
                                              and torch.equal(tbt.lost_turn, again.lost_turn))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
