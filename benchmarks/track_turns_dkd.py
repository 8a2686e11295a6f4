#!/usr/bin/env python3
"""Segment.track_turns on the README's 100-element drift-kick-drift FODO taken as a ring: 1000 turns at 1e3, 1e5 and 1e6
particles, every turn recorded (record_every=1); float32 beams in the arithmetic modes "mixed", "double" and "storage", and float64.

    python benchmarks/track_turns_dkd.py [turns] [--sizes 1e3,1e5,1e6] [--repeat 3] [--modes mixed,double,storage,f64]

Per case, wall time of one call (synchronised before and after; after one warm-up call of each, the three are timed in turn,
`repeat` rounds, and the best of each is kept — the three alternate, so a disturbance from outside hits them alike):
  fused     track_turns(fused=True): the energy walk, the constants, the turn kernel (chx_dkd_turns), records from the kernel
  general   track_turns(fused=False): the loop over Segment.track with the same records as float64 torch operations
  loop      for _ in range(turns): beam = ring.track(beam) — no records at all
and the fused call's WALL time per item step (turns x 100 items): at 1e6 particles the turn kernel dominates the call, below that
the figure is an upper bound on the kernel's duration per step.

The cases run at 1e8 eV, a fixed point of the reference energy's round trip: one block of constants serves every turn. One more
case per dtype (float32 "mixed", float64) runs at an energy that goes on DRIFTING, found on the device: among 4096 values on
either side of 2^25 and 2^26 eV the one whose round trip (restated in torch) moves longest; `energy_blocks` is the number of
distinct turn-start energies of the loop, i.e. the blocks of constants the fused call computes (the stationary cases: 1 or 2).
One JSON line per case."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402

ITEMS = 100


def ring_for(dt, precision):
    kw = {"dtype": dt, "device": "cuda"}
    tt = lambda v: torch.tensor(v, **kw)  # noqa: E731
    dkd = {"tracking_method": "drift_kick_drift"}
    els = []
    for _ in range(ITEMS // 4):
        els += [ca.Quadrupole(tt(0.2), k1=tt(4.2), **dkd, **kw), ca.Drift(tt(0.8), **dkd, **kw),
                ca.Quadrupole(tt(0.2), k1=tt(-4.2), **dkd, **kw), ca.Drift(tt(0.8), **dkd, **kw)]
    for e in els:
        e.dkd_precision = precision
    return ca.Segment(els)


def longest_drifting_energy(dt, mass_eV, limit=4000):
    """(energy, round trips it moves for, capped at `limit`) over the candidates of the module docstring."""
    gen = torch.Generator().manual_seed(3)
    parts = []
    for base in (2.0 ** 25, 2.0 ** 26):
        if dt == torch.float32:
            b = torch.tensor(base, dtype=torch.float32).view(torch.int32)
            parts.append((b + torch.arange(-4096, 4096, dtype=torch.int32)).view(torch.float32))
        else:
            parts.append(base + (torch.rand(8192, generator=gen, dtype=torch.float64) - 0.5) * 16384.0)
    cand = torch.cat(parts).to("cuda")
    m = torch.tensor(mass_eV, dtype=dt, device="cuda")
    e, moves = cand.clone(), torch.zeros(cand.shape, dtype=torch.int32, device="cuda")
    for _ in range(limit):
        p0 = torch.sqrt(e * e - m * m)
        nxt = torch.sqrt(p0 * p0 + m * m)
        moves += (nxt != e).to(torch.int32)
        e = nxt
    best = int(torch.argmax(moves))
    return float(cand[best]), int(moves[best])


def timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    opt = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    turns = int(args[0]) if args else 1000
    sizes = [int(float(v)) for v in opt("--sizes", "1e3,1e5,1e6").split(",")]
    repeat = int(opt("--repeat", "3"))
    modes = opt("--modes", "mixed,double,storage,f64").split(",")
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    cases = [(m, 1e8) for m in modes]
    for m in modes:
        if m in ("mixed", "f64"):
            cases.append((m, None))                                # the drifting energy, found below
    for mode, energy in cases:
        dt = torch.float64 if mode == "f64" else torch.float32
        ring = ring_for(dt, "mixed" if mode == "f64" else mode)
        for n in sizes:
            torch.manual_seed(0)
            beam = ca.ParticleBeam.from_parameters(num_particles=n, dtype=dt, device="cuda")
            row = {"mode": mode, "particles": n, "turns": turns, "items": ITEMS}
            if energy is None:
                found, moves = longest_drifting_energy(dt, beam.species.mass_eV_float)
                row["round_trips_moving"] = moves
            beam = ca.ParticleBeam(beam.particles, torch.tensor(found if energy is None else energy, dtype=dt, device="cuda"),
                                   particle_charges=beam.particle_charges, survival_probabilities=beam.survival_probabilities, s=beam.s,
                                   species=beam.species)
            row["energy_eV"] = float(beam.energy)

            def loop(keep=None):
                b = beam
                with torch.no_grad():
                    for _ in range(turns):
                        if keep is not None:
                            keep.append(b.energy)
                        b = ring.track(b)
                return b

            variants = {"fused": lambda: ring.track_turns(beam, turns, fused=True),
                        "general": lambda: ring.track_turns(beam, turns, fused=False), "loop": loop}
            best = {}
            for name, fn in variants.items():                      # warm-up: code objects, allocator, the segment's caches
                fn()
            torch.cuda.synchronize()
            for _ in range(repeat):
                for name, fn in variants.items():
                    best[name] = min(best.get(name, float("inf")), timed(fn))
            for name in variants:
                row[f"{name}_ms"] = round(best[name] * 1e3, 3)
            row["fused_ns_per_item_step"] = round(row["fused_ms"] * 1e6 / (turns * ITEMS), 2)
            row["general_over_fused"] = round(row["general_ms"] / row["fused_ms"], 2)
            row["loop_over_fused"] = round(row["loop_ms"] / row["fused_ms"], 2)
            starts = []
            want = loop(starts)
            row["energy_blocks"] = int(torch.unique(torch.stack(starts)).numel())
            tbt = ring.track_turns(beam, turns, fused=True)
            row["lost"] = int((tbt.lost_turn > 0).sum())
            row["same_bits_as_loop"] = bool(torch.equal(tbt.outgoing.particles, want.particles) and
                                            torch.equal(tbt.outgoing.energy, want.energy)) if row["lost"] == 0 else None
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
