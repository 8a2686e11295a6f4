#!/usr/bin/env python3
"""Every output tensor of a fixed, seeded list of calls through the runs of non-linear elements (`accelerator/_nonlinear.py`) and the
ring paths (`accelerator/_ring.py`) of `Segment`, written to ONE file: run it at two commits and compare the files byte for byte
(`cmp`). A refactor of those paths must leave the file as it is.

    python benchmarks/segment_modules_bits.py OUT_FILE

The calls: `track` (twice: found, then from the kept run) over the lattices of tests/test_gpu_nonlinear_partition.py in both dtypes;
`track_turns` fused second-order, fused drift-kick-drift and general, with records, probe rows and an aperture; `one_turn_map`,
`closed_orbit`, `ring_optics`, `chromaticity`, `ring_sensitivity` and `radiation_integrals` with `along`, with `wrt` (values and the
gradients of a backward pass) and with batches of `delta`. Small shapes: 64 to 500 particles, rings of 24 items. Per tensor a line
`name|dtype|shape` and its bytes; the last line of the output is the count and the file's SHA-256 as JSON."""
import dataclasses
import hashlib
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402
from tests.test_gpu_nonlinear_partition import DKD_CASES, SO_CASES, _beam  # noqa: E402

DKD = {"tracking_method": "drift_kick_drift"}
SO = {"tracking_method": "second_order"}
BEAM_FIELDS = ("particles", "energy", "s", "particle_charges", "survival_probabilities")


def flatten(name, obj, out):
    if obj is None:
        return
    if isinstance(obj, torch.Tensor):
        out.append((name, obj.detach()))
    elif isinstance(obj, ca.ParticleBeam):
        for f in BEAM_FIELDS:
            flatten(f"{name}.{f}", getattr(obj, f), out)
    elif dataclasses.is_dataclass(obj):
        for f in dataclasses.fields(obj):
            flatten(f"{name}.{f.name}", getattr(obj, f.name), out)
    elif hasattr(obj, "__slots__"):
        for f in obj.__slots__:
            flatten(f"{name}.{f}", getattr(obj, f), out)
    elif isinstance(obj, dict):
        for k in sorted(obj):
            flatten(f"{name}.{k}", obj[k], out)
    elif isinstance(obj, (tuple, list)):
        for k, v in enumerate(obj):
            flatten(f"{name}.{k}", v, out)
    else:
        out.append((name, torch.as_tensor(obj)))


def track_cases(out):
    for cases in (DKD_CASES, SO_CASES):
        for case in cases:
            for dt in (torch.float32, torch.float64):
                pieces = case(dt)[0]
                seg = ca.Segment([e for piece in pieces for e in piece])
                beam = _beam(dt)
                for k in range(2):
                    flatten(f"track.{case.__name__}.{dt}.{k}", seg.track(beam), out)


def dkd_ring(dt, precision="mixed", cavity=True):
    """Three cells [QF, D, B, D, QD, D, B, D] with a sextupole, a corrector Multipole and (first Drift) an RFCavity: 24 items."""
    kw = {"dtype": dt, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    els = []
    for c in range(3):
        for kind in "qdbdQsbm":
            if kind == "d" and len(els) == 1 and cavity:
                els.append(ca.RFCavity(t(0.3), voltage=t(5e4), phase=t(0.0), frequency=ca.RFCavity.harmonic_frequency(3 * 2.5, 200, t(1e8)), **kw))
            elif kind == "d":
                els.append(ca.Drift(t(0.3), **DKD, **kw))
            elif kind == "b":
                els.append(ca.Dipole(t(0.5), angle=t(2 * math.pi / 6), dipole_e1=t(0.02), **DKD, **kw))
            elif kind == "s":
                els.append(ca.Sextupole(t(0.3), k2=t(4.0 + c), num_steps=2, **DKD, **kw))
            elif kind == "m":
                els.append(ca.Multipole(t(0.3), 0, knl=t(1e-5 * (c + 1)), **kw))
            else:
                els.append(ca.Quadrupole(t(0.2), k1=t(2.2 if kind == "q" else -2.2), misalignment=t([1e-5 * c, 0.0]), **DKD, **kw))
    for e in els:
        e.dkd_precision = precision
    return ca.Segment(els)


def so_ring(dt):
    kw = {"dtype": dt, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    els = []
    for c in range(3):
        els += [ca.Quadrupole(t(0.2), k1=t(2.2), **SO, **kw), ca.Drift(t(0.3), **kw), ca.HorizontalCorrector(t(0.1), angle=t(1e-5), **kw),
                ca.Dipole(t(0.5), angle=t(0.2), **SO, **kw), ca.Marker(name=f"m{c}"), ca.Quadrupole(t(0.2), k1=t(-2.2), **SO, **kw),
                ca.Drift(t(0.3), **SO, **kw), ca.Sextupole(t(0.1), k2=t(3.0), **SO, **kw)]
    return ca.Segment(els)


def turn_cases(out):
    for dt in (torch.float32, torch.float64):
        kw = {"dtype": dt, "device": "cuda"}
        t = lambda v: torch.tensor(v, **kw)  # noqa: E731
        torch.manual_seed(11)
        beam = ca.ParticleBeam.from_parameters(num_particles=500, sigma_x=t(2e-4), sigma_px=t(3e-5), sigma_y=t(2e-4), sigma_py=t(3e-5),
                                               sigma_tau=t(1e-4), sigma_p=t(1e-3), energy=t(1e8), **kw)
        aperture = t([4e-4, 5e-4])
        linear_inside = dkd_ring(dt, cavity=False)
        linear_inside.elements[3] = ca.Drift(t(0.3), **kw)              # a linear run in the ring: the general path
        rings = [("second_order", so_ring(dt), None), ("dkd", dkd_ring(dt), None), ("dkd_general", dkd_ring(dt), False),
                 ("dkd_linear_inside", linear_inside, None)]
        if dt == torch.float32:
            rings.append(("dkd_storage", dkd_ring(dt, "storage"), True))
        for name, ring, fused in rings:
            for args in ({"record_every": 1}, {"record_every": 3, "record_first": 5, "aperture": aperture}):
                flatten(f"turns.{name}.{dt}.{len(args)}", ring.track_turns(beam, 7, fused=fused, **args), out)


def optics_cases(out):
    for dt in (torch.float32, torch.float64):
        dev = {"dtype": torch.float64, "device": "cuda"}
        energy = torch.tensor(1e8, dtype=dt, device="cuda")
        start = torch.tensor([[0.0] * 6, [1e-4, 0, 0, 0, 0, 0], [0, 2e-5, 1e-4, 0, 0, 1e-3], [1e-4, 1e-5, -1e-4, 2e-5, 1e-4, -1e-3],
                              [0, 0, 0, 0, 1e-3, 0]], **dev)
        deltas = torch.tensor([-1e-3, 0.0, 2e-3], **dev)
        for cavity in (False, True):
            ring = dkd_ring(dt, cavity=cavity)
            quads = [e for e in ring.elements if isinstance(e, ca.Quadrupole)]
            sext = [e for e in ring.elements if isinstance(e, ca.Sextupole)]
            knobs = [quads[0].k1, sext[1].k2, quads[1].misalignment, ring.elements[7].knl]
            tag = f"optics.{dt}.cavity{int(cavity)}"
            for along in (False, True):
                flatten(f"{tag}.one_turn_map.{along}", ring.one_turn_map(start, energy, along=along), out)
                flatten(f"{tag}.ring_optics.{along}", ring.ring_optics(energy, delta=deltas, along=along), out)
                flatten(f"{tag}.ring_sensitivity.{along}", ring.ring_sensitivity(energy, knobs, delta=deltas, along=along), out)
                flatten(f"{tag}.radiation_integrals.{along}", ring.radiation_integrals(energy, delta=deltas, along=along), out)
            flatten(f"{tag}.closed_orbit", ring.closed_orbit(energy, delta=deltas), out)
            flatten(f"{tag}.closed_orbit.guess", ring.closed_orbit(energy, guess=start, num_iterations=4), out)
            flatten(f"{tag}.closed_orbit.6d", ring.closed_orbit(energy, delta=1e-4, longitudinal=cavity), out)
            flatten(f"{tag}.chromaticity", ring.chromaticity(energy), out)
            flatten(f"{tag}.ring_sensitivity.all_without_grad", ring.ring_sensitivity(energy, "all"), out)
            # with wrt: the values, and the gradients of one backward pass through each
            for k in knobs:
                k.requires_grad_(True)
            calls = {"one_turn_map": lambda w: ring.one_turn_map(start, energy, along=True, wrt=w),
                     "closed_orbit": lambda w: ring.closed_orbit(energy, delta=deltas, wrt=w),
                     "ring_optics": lambda w: ring.ring_optics(energy, delta=deltas, wrt=w),
                     "chromaticity": lambda w: ring.chromaticity(energy, wrt=w)}
            for name, call in calls.items():
                for w in ((knobs, "all", knobs[1:3]) if name == "ring_optics" else (knobs,)):
                    partial = w is not knobs and w != "all"
                    if partial:                     # (a setting that requires grad and is not named is refused)
                        knobs[0].requires_grad_(False), knobs[3].requires_grad_(False)
                    res = call(w)
                    flatten(f"{tag}.{name}.wrt{len(w)}", res, out)
                    live = []
                    flatten_live(res, live)
                    loss = sum(v.nan_to_num().sum() for v in live if v.requires_grad)
                    flatten(f"{tag}.{name}.wrt{len(w)}.grad", torch.autograd.grad(loss, [k for k in knobs if k.requires_grad]), out)
                    if partial:
                        knobs[0].requires_grad_(True), knobs[3].requires_grad_(True)
            for k in knobs:
                k.requires_grad_(False)


def flatten_live(obj, out):
    """The tensors of a result WITH their graph (flatten detaches)."""
    if isinstance(obj, torch.Tensor):
        out.append(obj)
    elif dataclasses.is_dataclass(obj):
        for f in dataclasses.fields(obj):
            flatten_live(getattr(obj, f.name), out)
    elif isinstance(obj, (tuple, list)):
        for v in obj:
            flatten_live(v, out)


def main():
    assert torch.cuda.is_available(), "the calls run on the GPU"
    path = sys.argv[1]
    out = []
    with torch.no_grad():
        track_cases(out)
    turn_cases(out)
    optics_cases(out)
    torch.cuda.synchronize()
    digest = hashlib.sha256()
    with open(path, "wb") as f:
        for name, v in out:
            v = v.cpu().contiguous()
            blob = f"{name}|{v.dtype}|{tuple(v.shape)}\n".encode() + v.numpy().tobytes() + b"\n"
            f.write(blob)
            digest.update(blob)
    print(json.dumps({"tensors": len(out), "bytes": os.path.getsize(path), "sha256": digest.hexdigest()}))


if __name__ == "__main__":
    main()
