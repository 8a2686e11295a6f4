#!/usr/bin/env python3
"""Segment.one_turn_map, ring_optics and closed_orbit (chx_dkd_ring_jacobian) against what a user did before they existed, on the
48-item ring with an RFCavity of tests/test_gpu_rfcavity.py and on the 185-item ring of benchmarks/track_turns_dkd_multipole.py
(float64 settings, 100 MeV electrons).

    python benchmarks/ring_optics.py [--repeat 5] [--scan 1,64,4096] [--baseline-newton 4]

Per ring, wall time of one call (synchronised before and after; one warm-up call of each, then `repeat` timed calls, the best and
the median kept):
  one_turn_map       the map and its Jacobian at the origin, one call
  ring_optics        closed orbit (10 Newton steps) + optics behind every item, one call
  closed_orbit_B     the 4-D closed orbits of B values of delta in one call, B from --scan
  six_passes         the BASELINE: the 6 x 6 one-turn Jacobian from six backward passes through `track` (one_turn_jacobian of
                     tests/test_gpu_rfcavity.py), one seed
  newton_baseline    the BASELINE closed orbit of ONE delta: `--baseline-newton` Newton steps in numpy, each a six-backward-pass
                     Jacobian and a host solve (a scan of B values of delta costs B times this: not run, the ratio is arithmetic)
One JSON line per ring."""
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402
from benchmarks.track_turns_dkd_multipole import ring_for  # noqa: E402

F64 = torch.float64
KW = {"dtype": F64, "device": "cuda"}
ENERGY = 1e8


def tt(v):
    return torch.tensor(v, **KW)


def rf_ring():
    """tests/test_gpu_rfcavity.py::small_ring(0.0, 5e4): six cells [QF, D, B, D, QD, D, B, D], the first Drift the cavity."""
    dkd = {"tracking_method": "drift_kick_drift"}
    els = []
    for c in range(6):
        for kind in "qdbdQdbd":
            if kind == "d" and len(els) == 1:
                f = ca.RFCavity.harmonic_frequency(6 * 2.6, 400, tt(ENERGY))
                els.append(ca.RFCavity(tt(0.3), voltage=tt(5e4), phase=tt(0.0), frequency=f, **KW))
            elif kind == "d":
                els.append(ca.Drift(tt(0.3), **dkd, **KW))
            elif kind == "b":
                els.append(ca.Dipole(tt(0.5), angle=tt(2 * math.pi / 12), **dkd, **KW))
            else:
                els.append(ca.Quadrupole(tt(0.2), k1=tt(3.0 if kind == "q" else -3.0), num_steps=1, **dkd, **KW))
    return ca.Segment(els)


def six_passes(ring, x6):
    """(image, Jacobian) of one turn at the single point x6 (6,) numpy, from six backward passes."""
    rows, out = [], None
    x0 = torch.zeros(1, 7, **KW)
    x0[0, :6] = torch.as_tensor(x6, **KW)
    x0[0, 6] = 1.0
    for i in range(6):
        p = x0.clone().requires_grad_(True)
        out = ring.track(ca.ParticleBeam(p, tt(ENERGY), species=ca.Species("electron", **KW)))
        out.particles[0, i].backward()
        rows.append(p.grad[0, :6].cpu().numpy())
    return out.particles[0, :6].detach().cpu().numpy(), np.stack(rows)


def newton_baseline(ring, delta, steps):
    x = np.zeros(6)
    x[5] = delta
    for _ in range(steps):
        f, J = six_passes(ring, x)
        x[:4] += np.linalg.solve(J[:4, :4] - np.eye(4), -(f[:4] - x[:4]))
    return x


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


def main():
    opt = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default  # noqa: E731
    repeat = int(opt("--repeat", "5"))
    scan = [int(v) for v in opt("--scan", "1,64,4096").split(",")]
    newton = int(opt("--baseline-newton", "4"))
    assert torch.cuda.is_available(), "this benchmark measures on the GPU"
    for name, ring in (("rf_ring_48", rf_ring()), ("multipole_ring_185", ring_for(F64, "mixed"))):
        energy, origin = tt(ENERGY), torch.zeros(1, 6, **KW)
        row = {"ring": name, "items": len(ring.elements), "repeat": repeat}
        row["one_turn_map"] = measure(lambda: ring.one_turn_map(origin, energy), repeat)
        row["ring_optics"] = measure(lambda: ring.ring_optics(energy), repeat)
        for B in scan:
            delta = torch.linspace(-1e-3, 1e-3, B, **KW) if B > 1 else tt([1e-3])
            row[f"closed_orbit_{B}"] = measure(lambda: ring.closed_orbit(energy, delta=delta), repeat)
        row["six_passes"] = measure(lambda: six_passes(ring, np.zeros(6)), max(2, repeat // 2))
        row["newton_baseline"] = dict(measure(lambda: newton_baseline(ring, 1e-3, newton), 2), newton_steps=newton)
        # the two ways agree (the check of the tests, repeated here on the benchmark's rings)
        _, J = six_passes(ring, np.zeros(6))
        M = ring.one_turn_map(origin, energy).matrix[0].cpu().numpy()
        row["matrix_difference"] = float(np.abs(M - J).max() / max(1.0, np.abs(J).max()))
        co = ring.closed_orbit(energy, delta=tt([1e-3]))
        row["orbit_difference"] = float(np.abs(co.orbit[0, :6].cpu().numpy() - newton_baseline(ring, 1e-3, newton)).max())
        row["one_turn_map_speedup"] = round(row["six_passes"]["best_ms"] / row["one_turn_map"]["best_ms"], 1)
        row["closed_orbit_speedup"] = round(row["newton_baseline"]["best_ms"] / row["closed_orbit_1"]["best_ms"], 1) if 1 in scan else None
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
