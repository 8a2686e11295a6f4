#!/usr/bin/env python3
"""Segment.ring_sensitivity and ring_optics(wrt=...) (chx_dkd_ring_sensitivity) against what a user did before they existed —
central differences, two `ring_optics` calls per knob with the setting edited in place — on the 48-item and the 185-item ring of
benchmarks/ring_optics.py (float64 settings, 100 MeV electrons).

    python benchmarks/ring_sensitivity.py [--repeat 5]

The knobs of a ring: every Quadrupole k1 and Sextupole k2 in the order of the lattice, then the Quadrupoles' lengths (to reach 16
on the ring with twelve strengths). K = 2, K = 16 and K = all strengths. Per ring and K, wall time of one call (synchronised
before and after; one warm-up call, then `repeat` timed calls, the best and the median kept):
  ring_sensitivity   one call: closed orbit, every tangent behind every item, d_tunes and d_beta
  optics_backward    ring_optics(wrt=knobs) followed by tunes.sum().backward()
  differences        the BASELINE: 2 K calls of ring_optics without `wrt` and the K differences of the tunes
and the largest difference between d_tunes and the baseline's. One JSON line per ring and K."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402
from benchmarks.ring_optics import ENERGY, F64, rf_ring, tt  # noqa: E402
from benchmarks.track_turns_dkd_multipole import ring_for  # noqa: E402


def knobs_of(ring):
    """(the knobs, each tensor once; the number of strengths among them, which come first)"""
    owners = [e for e in ring.elements if isinstance(e, (ca.Quadrupole, ca.Sextupole))]
    strengths = [(e.k1 if isinstance(e, ca.Quadrupole) else e.k2) for e in owners]
    unique = []
    for t in strengths + [e.length for e in owners if isinstance(e, ca.Quadrupole)]:
        if t.dim() == 0 and not any(t is u for u in unique):
            unique.append(t)
    return unique, len({id(t) for t in strengths})


def measure(fn, repeat):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return {"best_ms": round(min(times) * 1e3, 3), "median_ms": round(statistics.median(times) * 1e3, 3)}


def differences(ring, energy, knobs, h=1e-5):
    out = []
    for t in knobs:
        keep = t.clone()
        t.copy_(keep + h)
        plus = ring.ring_optics(energy).tunes
        t.copy_(keep - h)
        minus = ring.ring_optics(energy).tunes
        t.copy_(keep)
        out.append((plus - minus) / (2 * h))
    return torch.stack(out, 1)                                        # (B, K, 2)


def main():
    opt = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    repeat = int(opt("--repeat", "5"))
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    for name, ring in (("rf_ring_48", rf_ring()), ("multipole_ring_185", ring_for(F64, "mixed"))):
        energy = tt(ENERGY)
        every, n_strengths = knobs_of(ring)
        for K in sorted({2, 16, n_strengths}):
            knobs = every[:K]
            if len(knobs) < K:
                continue
            row = {"ring": name, "items": len(ring.elements), "K": K, "repeat": repeat}
            row["ring_sensitivity"] = measure(lambda: ring.ring_sensitivity(energy, knobs), repeat)
            for t in knobs:
                t.requires_grad_(True)

            def optics_backward():
                for t in knobs:
                    t.grad = None
                ring.ring_optics(energy, wrt=knobs).tunes.sum().backward()

            row["optics_backward"] = measure(optics_backward, repeat)
            for t in knobs:
                t.requires_grad_(False)
            row["differences"] = measure(lambda: differences(ring, energy, knobs), max(2, repeat // 2))
            d = ring.ring_sensitivity(energy, knobs, along=False).d_tunes
            worst = float((d - differences(ring, energy, knobs)).abs().max())
            row["d_tunes_difference"] = worst if worst == worst else None      # (None: the ring has no stable eigen-tunes, NaN)
            row["speedup_ring_sensitivity"] = round(row["differences"]["best_ms"] / row["ring_sensitivity"]["best_ms"], 1)
            row["speedup_optics_backward"] = round(row["differences"]["best_ms"] / row["optics_backward"]["best_ms"], 1)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
