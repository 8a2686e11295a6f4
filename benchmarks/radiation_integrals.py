#!/usr/bin/env python3
"""Segment.radiation_integrals (chx_dkd_ring_radiation) against what it contains and against what a user could do before it
existed, on the 48-item and the 185-item ring of benchmarks/ring_optics.py (float64 settings, 100 MeV electrons).

    python benchmarks/radiation_integrals.py [--repeat 7] [--batches 1,4096]

Per ring and B (delta spread over +-1e-3), wall time of one call (synchronised before and after; one warm-up call, then `repeat`
timed calls, the best and the median kept):
  radiation_integrals   the call
  ring_optics           ring_optics(along=False) on the same ring: what the call contains, so the difference is the new kernel
                        with its start values and derived quantities
  split_simpson         the BASELINE, on the 48-item ring only (the 185-item ring has no Dipole: its integrals are zeros, the call
                        walks its items once): the ring with every one of its 12 bends in 12 pieces (180 items, the most the ring
                        kernels' 192 leave room for), ring_optics(along=True), and composite Simpson sums of the integrands in torch
and the largest relative difference between the call's I1, I4x, I5x and the baseline's. One JSON line per ring and B."""
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402
from benchmarks.ring_optics import ENERGY, F64, KW, rf_ring, tt  # noqa: E402
from benchmarks.track_turns_dkd_multipole import ring_for  # noqa: E402

PIECES = 12


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


def split_ring(ring):
    """(the ring with every Dipole in PIECES pieces, the index of each bend's first piece, (L, h) of the bends)"""
    els, first = [], []
    for e in ring.elements:
        if isinstance(e, ca.Dipole):
            first.append(len(els))
            els += e._arc_pieces(PIECES, "p")
        else:
            els.append(e)
    bends = [e for e in ring.elements if isinstance(e, ca.Dipole)]
    L = torch.stack([e.length for e in bends]).to(F64)
    h = torch.stack([e.angle for e in bends]).to(F64) / L
    return ca.Segment(els), torch.tensor(first, device="cuda"), L, h


def split_simpson(fine, first, L, h, energy, delta):
    """(I1, I4x, I5x) (B,) of a flat ring of sector bends from the optics behind every piece."""
    opt = fine.ring_optics(energy, delta=delta, along=True)
    rows = first[:, None] + torch.arange(PIECES + 1, device="cuda")[None]             # (bends, PIECES + 1)
    rel = math.sqrt(1.0 - (510998.95069 / ENERGY) ** 2)
    eta, etap = rel * opt.dispersion_along[:, rows, 0], rel * opt.dispersion_along[:, rows, 1]
    beta, alpha = opt.beta[:, rows, 0], opt.alpha[:, rows, 0]
    H = (eta ** 2 + (beta * etap + alpha * eta) ** 2) / beta
    w = torch.ones(PIECES + 1, **KW)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    simpson = lambda f: (f * w).sum(-1) * (L / (3.0 * PIECES))  # noqa: E731
    return torch.stack([(simpson(eta) * h).sum(-1), (simpson(eta) * h ** 3).sum(-1), (simpson(H) * h.abs() ** 3).sum(-1)], dim=-1)


def main():
    opt = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    repeat = int(opt("--repeat", "7"))
    batches = [int(b) for b in opt("--batches", "1,4096").split(",")]
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    for name, ring in (("rf_ring_48", rf_ring()), ("multipole_ring_185", ring_for(F64, "mixed"))):
        energy = tt(ENERGY)
        has_bends = any(isinstance(e, ca.Dipole) for e in ring.elements)
        if has_bends:
            fine, first, L, h = split_ring(ring)
        for B in batches:
            delta = torch.linspace(-1e-3, 1e-3, B, **KW) if B > 1 else torch.zeros(1, **KW)
            row = {"ring": name, "items": len(ring.elements), "B": B, "repeat": repeat}
            row["radiation_integrals"] = measure(lambda: ring.radiation_integrals(energy, delta=delta), repeat)
            row["ring_optics"] = measure(lambda: ring.ring_optics(energy, delta=delta, along=False), repeat)
            row["new_kernel_and_algebra_ms"] = round(row["radiation_integrals"]["best_ms"] - row["ring_optics"]["best_ms"], 3)
            if has_bends:
                row["split_items"] = len(fine.elements)
                row["split_simpson"] = measure(lambda: split_simpson(fine, first, L, h, energy, delta), max(2, repeat // 2))
                rad = ring.radiation_integrals(energy, delta=delta)
                mine = torch.stack([rad.I1, rad.I4[:, 0], rad.I5[:, 0]], dim=-1)
                theirs = split_simpson(fine, first, L, h, energy, delta)
                row["largest_relative_difference"] = float(((mine - theirs) / mine).abs().max())
                row["speedup"] = round(row["split_simpson"]["best_ms"] / row["radiation_integrals"]["best_ms"], 2)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
