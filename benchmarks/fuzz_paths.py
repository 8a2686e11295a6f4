#!/usr/bin/env python3
"""Differential fuzz of `Segment.track`'s fast paths: drawn flat lattices (linear elements with scalar or (B,) settings, upright and
rotated quadrupoles, dipoles, correctors, solenoids, active cavities, active monitors, apertures and screens, second-order and
drift-kick-drift elements) tracked by `Segment.track` — one-call stretches, merged runs, chains in registers — against the same
elements tracked ONE BY ONE through their own `track` (the path the reference-generated goldens pin). Compared: outgoing particles,
survival probabilities, energy, path length, every monitor's reading, every screen's reading.

usage: python benchmarks/fuzz_paths.py [n_cases] [first_seed]        prints one line per failing case and a summary; exit code 1 on a failure
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cheetah_amd as ca  # noqa: E402


def draw_lattice(rng, fk, B):
    """(elements for Segment.track, a second, independent copy for the walk): B = 0: scalar settings, else some settings are (B,)."""
    t = lambda v: torch.tensor(v, **fk)  # noqa: E731

    def setting(lo, hi, vector_ok=True):
        if B and vector_ok and rng.random() < 0.35:
            return rng.uniform(lo, hi, size=B).tolist()
        return float(rng.uniform(lo, hi))

    specs = []
    n = int(rng.integers(2, 14))
    nonlinear = rng.random() < 0.25 and not B
    with_cavity = rng.random() < 0.3
    for _ in range(n):
        r = rng.random()
        if r < 0.3:
            specs.append(("Drift", {"length": float(rng.uniform(0.05, 1.0))}))
        elif r < 0.55:
            kw = {"length": float(rng.uniform(0.05, 0.4)), "k1": setting(-12.0, 12.0)}
            if rng.random() < 0.3:
                kw["tilt"] = setting(-0.3, 0.3)
            if rng.random() < 0.3:
                kw["misalignment"] = [float(rng.normal() * 1e-4), float(rng.normal() * 1e-4)]
            if nonlinear and rng.random() < 0.5:
                kw["tracking_method"] = str(rng.choice(["second_order", "drift_kick_drift"]))
            specs.append(("Quadrupole", kw))
        elif r < 0.63:
            specs.append(("HorizontalCorrector", {"length": float(rng.uniform(0.02, 0.1)), "angle": setting(-2e-4, 2e-4)}))
        elif r < 0.7:
            specs.append(("VerticalCorrector", {"length": float(rng.uniform(0.02, 0.1)), "angle": setting(-2e-4, 2e-4)}))
        elif r < 0.76:
            kw = {"length": float(rng.uniform(0.2, 0.8)), "angle": float(rng.uniform(-0.2, 0.2))}
            if rng.random() < 0.5:
                kw.update(dipole_e1=float(rng.uniform(-0.1, 0.1)), dipole_e2=float(rng.uniform(-0.1, 0.1)))
            if rng.random() < 0.3:
                kw["tilt"] = float(rng.uniform(-0.2, 0.2))
            specs.append(("Dipole", kw))
        elif r < 0.8:
            specs.append(("Solenoid", {"length": float(rng.uniform(0.1, 0.4)), "k": float(rng.uniform(-2.0, 2.0))}))
        elif r < 0.86:
            specs.append(("BPM", {"is_active": bool(rng.random() < 0.8)}))
        elif r < 0.9:
            specs.append(("Aperture", {"x_max": float(rng.uniform(2e-4, 2e-3)), "y_max": float(rng.uniform(2e-4, 2e-3)),
                                       "shape": str(rng.choice(["rectangular", "elliptical"])), "is_active": bool(rng.random() < 0.8)}))
        elif r < 0.95 and with_cavity:
            specs.append(("Cavity", {"length": float(rng.uniform(0.3, 1.0)), "voltage": setting(1e6, 2e7), "phase": setting(-60.0, 60.0),
                                     "frequency": 1.3e9, "cavity_type": str(rng.choice(["standing_wave", "traveling_wave"]))}))
        else:
            specs.append(("Marker", {}))
    if rng.random() < (0.6 if not B else 0.3):
        specs.insert(int(rng.integers(1, len(specs) + 1)),
                     ("Screen", {"resolution": [int(rng.integers(16, 80)), int(rng.integers(16, 80))], "pixel_size": [6e-5, 5e-5],
                                 "method": str(rng.choice(["cloud-in-cell", "histogram"])) if not B else "cloud-in-cell", "is_active": True,
                                 "misalignment": [float(rng.normal() * 5e-5), 0.0] if rng.random() < 0.3 else [0.0, 0.0]}))

    def build():
        out = []
        for kind, kw in specs:
            args = {}
            for k, v in kw.items():
                args[k] = t(v) if isinstance(v, (float, list)) and k not in ("resolution",) else v
            cls = getattr(ca, kind)
            out.append(cls(**args, **fk) if kind != "Drift" else cls(args["length"], **fk))
        return out

    return specs, build(), build()


def compare(a, b, tol, what, fails, scale=None):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    if a.shape != b.shape:
        fails.append(f"{what}: shapes {tuple(a.shape)} vs {tuple(b.shape)}")
        return
    a64, b64 = a.double(), b.double()
    both_nan = torch.isnan(a64) & torch.isnan(b64)
    finite = b64[~torch.isnan(b64)]
    ref = (finite.abs().amax() if finite.numel() else torch.tensor(0.0, device=b64.device)) if scale is None else scale
    ref = torch.as_tensor(ref).to(dtype=torch.float64, device=b64.device)      # (+ 1e-300 below must not underflow)
    if bool((torch.isnan(a64) != torch.isnan(b64)).any()):
        fails.append(f"{what}: NaNs in different places")
        return
    err = ((a64 - b64).abs().masked_fill(both_nan | (a64 == b64), 0.0) / (ref + 1e-300)).amax() if a.numel() else torch.tensor(0.0)
    if not bool(err <= tol):
        fails.append(f"{what}: {float(err):.3e} of the largest entry (allowed {tol:.1e})")


def one_case(seed):
    rng = np.random.default_rng(seed)
    dt = torch.float64 if rng.random() < 0.5 else torch.float32
    fk = {"dtype": dt, "device": "cuda"}
    B = int(rng.choice([0, 0, 3, 17]))
    specs, els_a, els_b = draw_lattice(rng, fk, B)
    n = int(rng.choice([37, 1000, 4097, 30000]))
    if n == 37 and any(k == "Aperture" and kw["is_active"] for k, kw in specs):
        n = 1000          # (one or two survivors of 37: statistics that divide by ~0 are noise on either path)
    torch.manual_seed(seed)
    t = lambda v: torch.tensor(v, **fk)  # noqa: E731
    beam = ca.ParticleBeam.from_parameters(num_particles=n, sigma_x=t(3e-4), sigma_y=t(2e-4), sigma_px=t(3e-5), sigma_py=t(2e-5),
                                           mu_x=t(float(rng.normal() * 1e-4)), energy=t(float(rng.uniform(2e7, 3e8))), **fk)
    if rng.random() < 0.4:
        beam.survival_probabilities = (0.2 + 0.8 * torch.rand(n, **fk))
    if rng.random() < 0.25 and n <= 4097:
        # a vectorised beam: (Bb, N, 7) particles (the lattice's (B,) settings broadcast against it), sometimes its own energies
        Bb = B if B else 2
        shift = torch.linspace(-1e-4, 1e-4, Bb, **fk).reshape(Bb, 1, 1) * torch.tensor([1.0, 0, 0.5, 0, 0, 0, 0], **fk)
        energy = beam.energy * torch.linspace(0.9, 1.1, Bb, **fk) if rng.random() < 0.4 else beam.energy
        beam = ca.ParticleBeam(beam.particles.unsqueeze(0) + shift, energy, particle_charges=beam.particle_charges,
                               survival_probabilities=beam.survival_probabilities, **fk)
    fails = []
    nested = list(els_a)
    if rng.random() < 0.3 and len(nested) >= 3:
        # (nested Segments, one or two levels: Segment.track sees through plain nested Segments; the walk goes over the flat list)
        for _ in range(int(rng.integers(1, 3))):
            if len(nested) < 2:
                break
            lo = int(rng.integers(0, len(nested) - 1))
            hi = int(rng.integers(lo + 1, len(nested) + 1))
            nested[lo:hi] = [ca.Segment(nested[lo:hi])]
    seg = ca.Segment(nested)
    mode = rng.random()
    if mode < 0.2 and not B:
        gradients(rng, seg, els_a, els_b, beam, dt, fails)
        return specs, dt, B, n, fails
    if mode < 0.35 and not any(kw.get("tracking_method") for _, kw in specs):      # (non-linear methods refuse a ParameterBeam, as the reference's do)
        moments_beam(seg, els_a, els_b, beam, dt, fails)
        return specs, dt, B, n, fails
    if mode < 0.45:
        observables(seg, els_b, beam, dt, fails)
        return specs, dt, B, n, fails
    if mode < 0.55 and not B and beam.particles.dim() == 2:
        record_property(rng, els_a, els_b, beam, dt, fk, fails)
        return specs, dt, B, n, fails
    if mode < 0.62:
        replayed(rng, seg, els_a, els_b, beam, dt, fails)
        return specs, dt, B, n, fails
    # (the layouts of assigned tensors come from a generator of their own: the draws above stay what they were for every seed)
    layouts = np.random.default_rng([seed, 0x1A7])
    for round_ in range(int(rng.integers(1, 4))):
        if round_:
            mutate(rng, els_a, els_b, fk, layouts)
        check(seg, els_a, els_b, beam, dt, fails, f"track {round_}: ")
        if fails:
            break
    return specs, dt, B, n, fails


def gradients(rng, seg, els_a, els_b, beam, dt, fails):
    """Scalar settings as Parameters on both copies: a loss on the outgoing particles, on a beam property and (when there is one) on
    the screen's image — the gradients of the two ways of tracking."""
    pa, pb = [], []
    for ea, eb in zip(els_a, els_b):
        for name in ("k1", "angle", "voltage", "phase"):
            if isinstance(ea, ca.Dipole) or not hasattr(ea, name) or getattr(ea, name).dim() != 0:
                continue
            if rng.random() < 0.6:
                va = torch.nn.Parameter(getattr(ea, name).detach().clone())
                vb = torch.nn.Parameter(va.detach().clone())
                setattr(ea, name, va)
                setattr(eb, name, vb)
                pa.append(va)
                pb.append(vb)
    if not pa:
        return
    n = beam.particles.shape[-2]
    W = torch.linspace(-1.0, 1.0, n * 7, dtype=dt, device="cuda").reshape(n, 7).cos()
    which = rng.random()
    screens = [(ea, eb) for ea, eb in zip(els_a, els_b) if isinstance(ea, ca.Screen)]

    def loss_of(out, scr):
        if which < 0.4:
            return (out.particles * W).sum() / n
        if which < 0.8 or not screens:
            return (out.sigma_x + 0.5 * out.sigma_y + out.mu_x).sum()
        return (scr.reading * scr.reading).sum() * 1e20 if scr.method == "cloud-in-cell" else scr.get_read_beam().sigma_x.sum()

    la = loss_of(seg.track(beam), screens[0][0] if screens else None)
    ref = beam
    for e in els_b:
        ref = e.track(ref)
    lb = loss_of(ref, screens[0][1] if screens else None)
    if la.requires_grad != lb.requires_grad:
        fails.append(f"loss requires_grad {la.requires_grad} vs {lb.requires_grad}")
        return
    if not lb.requires_grad:                 # (every Parameter sits behind the screen the loss reads)
        return
    la.backward()
    lb.backward()
    rel = 1e-8 if dt == torch.float64 else 2e-3
    eps = (1e-13 if dt == torch.float64 else 1e-5) * abs(float(lb.detach()))      # rounding of a gradient that is zero analytically
    compare(la.detach(), lb.detach(), 1e-10 if dt == torch.float64 else 1e-4, "loss", fails)
    gmax = max(float(p.grad.abs()) if p.grad is not None else 0.0 for p in pb) + 1e-300
    for k, (va, vb) in enumerate(zip(pa, pb)):
        ga = va.grad if va.grad is not None else torch.zeros_like(va)
        gb = vb.grad if vb.grad is not None else torch.zeros_like(vb)
        if float(ga) != float(ga) and float(gb) != float(gb):          # (no particle survives an aperture: NaN both ways)
            continue
        if not abs(float(ga) - float(gb)) <= rel * max(abs(float(gb)), 1e-3 * gmax) + eps / max(abs(float(vb.detach())), 1e-3):
            fails.append(f"gradient {k}: {float(ga):.6e} vs {float(gb):.6e} (loss kind {which:.2f})")


def moments_beam(seg, els_a, els_b, beam, dt, fails):
    """The same lattice on a ParameterBeam: Segment.track against the elements one by one; with scalar settings also the gradients of
    a loss on the outgoing moments with respect to settings made Parameters."""
    pb = beam.as_parameter_beam()
    pa, pbs = [], []
    scalar = all(getattr(e, n).dim() == 0 for e in els_a for n in ("k1", "angle", "voltage", "phase") if hasattr(e, n) and not isinstance(e, ca.Dipole))
    if scalar and pb.mu.dim() == 1:
        for ea, eb in zip(els_a, els_b):
            for name in ("k1", "angle"):
                if isinstance(ea, ca.Dipole) or not hasattr(ea, name) or getattr(ea, name).dim() != 0:
                    continue
                va = torch.nn.Parameter(getattr(ea, name).detach().clone())
                vb = torch.nn.Parameter(va.detach().clone())
                setattr(ea, name, va)
                setattr(eb, name, vb)
                pa.append(va)
                pbs.append(vb)
    out = seg.track(pb)
    ref = pb
    for e in els_b:
        ref = e.track(ref)
    if pa and out.mu.requires_grad and ref.mu.requires_grad:
        W = torch.linspace(0.3, 1.7, 49, dtype=dt, device="cuda").reshape(7, 7)
        la = (out.cov * W).sum() * 1e6 + out.mu[:6].sum() * 1e2
        lb = (ref.cov * W).sum() * 1e6 + ref.mu[:6].sum() * 1e2
        la.backward()
        lb.backward()
        gmax = max(float(v.grad.abs()) if v.grad is not None else 0.0 for v in pbs) + 1e-300
        rel = 1e-8 if dt == torch.float64 else 5e-3
        for k, (va, vb) in enumerate(zip(pa, pbs)):
            ga = float(va.grad) if va.grad is not None else 0.0
            gb = float(vb.grad) if vb.grad is not None else 0.0
            if not abs(ga - gb) <= rel * max(abs(gb), 1e-3 * gmax):
                fails.append(f"ParameterBeam gradient {k}: {ga:.6e} vs {gb:.6e}")
        out, ref = out.detach() if hasattr(out, "detach") else out, ref
    tol = 1e-10 if dt == torch.float64 else 1e-4
    compare(out.mu, ref.mu, tol, "mu", fails)
    compare(out.cov, ref.cov, tol, "cov", fails)
    compare(out.energy, ref.energy, 1e-12 if dt == torch.float64 else 2e-7, "energy", fails)
    for ea, eb in zip(els_a, els_b):
        if isinstance(ea, ca.BPM) and ea.is_active:
            compare(ea.reading, eb.reading, tol, "BPM reading", fails, scale=torch.tensor(3e-4))
        if isinstance(ea, ca.Screen):
            compare(ea.reading, eb.reading, 1e-8 if dt == torch.float64 else 1e-3, "screen reading", fails)


def record_property(rng, els_a, els_b, beam, dt, fk, fails):
    """[run of linear elements | active Screen]: the differentiable stretch (RunScreenTrack) and a property of its record as one
    node on the run's settings (RunMomentEntry) against the walk — value and gradients of a drawn beam property of the read beam."""
    linear = (ca.Drift, ca.Quadrupole, ca.HorizontalCorrector, ca.VerticalCorrector, ca.Dipole, ca.Solenoid)
    keep = [k for k, e in enumerate(els_a) if isinstance(e, linear) and getattr(e, "tracking_method", "linear") == "linear"]
    if not keep:
        return
    run_a, run_b = [els_a[k] for k in keep], [els_b[k] for k in keep]
    pa, pb = [], []
    for ea, eb in zip(run_a, run_b):
        for name in ("k1", "angle", "tilt", "length"):
            if not hasattr(ea, name) or getattr(ea, name).dim() != 0 or (name == "length" and not isinstance(ea, ca.Drift)):
                continue
            if rng.random() < 0.4:
                va = torch.nn.Parameter(getattr(ea, name).detach().clone())
                vb = torch.nn.Parameter(va.detach().clone())
                setattr(ea, name, va)
                setattr(eb, name, vb)
                pa.append(va)
                pb.append(vb)
    if not pa:
        return
    mis = [float(rng.normal() * 5e-5), 0.0] if rng.random() < 0.3 else [0.0, 0.0]
    sa = ca.Screen(resolution=(32, 32), pixel_size=torch.tensor([1e-4, 1e-4], **fk), is_active=True, misalignment=torch.tensor(mis, **fk), **fk)
    sb = ca.Screen(resolution=(32, 32), pixel_size=torch.tensor([1e-4, 1e-4], **fk), is_active=True, misalignment=torch.tensor(mis, **fk), **fk)
    seg = ca.Segment(run_a + [sa])
    prop = str(rng.choice(["sigma_x", "sigma_y", "sigma_px", "mu_x", "mu_y", "sigma_tau", "sigma_p", "mu_px"]))
    for step in range(int(rng.integers(1, 3))):          # (a second step: plans and memoised moments are reused)
        for v in pa + pb:
            v.grad = None
        seg.track(beam)
        la = getattr(sa.get_read_beam(), prop)
        ref = beam
        for e in run_b + [sb]:
            ref = e.track(ref)
        lb = getattr(sb.get_read_beam(), prop)
        if la.requires_grad != lb.requires_grad:
            fails.append(f"{prop}: requires_grad {la.requires_grad} vs {lb.requires_grad}")
            return
        compare(la.detach(), lb.detach(), 1e-10 if dt == torch.float64 else 5e-5, prop, fails, scale=lb.detach().abs() + 1e-7)
        if not lb.requires_grad:
            return
        la.backward()
        lb.backward()
        rel = 1e-7 if dt == torch.float64 else 5e-3
        gmax = max(float(v.grad.abs()) if v.grad is not None else 0.0 for v in pb) + 1e-300
        for k, (va, vb) in enumerate(zip(pa, pb)):
            ga = float(va.grad) if va.grad is not None else 0.0
            gb = float(vb.grad) if vb.grad is not None else 0.0
            if ga != ga and gb != gb:
                continue
            if not abs(ga - gb) <= rel * max(abs(gb), 1e-3 * gmax) + (1e-13 if dt == torch.float64 else 1e-5) * max(abs(float(lb.detach())), 1e-5) / max(abs(float(vb.detach())), 1e-3):
                fails.append(f"d {prop} / d setting {k}: {ga:.6e} vs {gb:.6e} (step {step})")


def replayed(rng, seg, els_a, els_b, beam, dt, fails):
    """The step (track + every monitor's and screen's reading) captured once into a device graph (cheetah_amd.graph.capture) and
    replayed after the settings were edited IN PLACE: the replay against the walk with the edited settings."""
    import cheetah_amd.graph as graph

    def step():
        out = seg.track(beam)
        reads = [e.reading for e in els_a if (isinstance(e, ca.BPM) and e.is_active) or (isinstance(e, ca.Screen) and (e.method == "cloud-in-cell" or beam.particles.dim() == 2))]
        return out.particles, out.survival_probabilities, out.energy, reads

    with torch.no_grad():
        try:
            captured = graph.capture(step)
        except NotImplementedError:
            return                            # ('histogram' under a vectorised beam: refused like the reference's)
        for _ in range(2):
            for ea, eb in zip(els_a, els_b):          # in place, the same on both copies
                if isinstance(ea, ca.Quadrupole) and rng.random() < 0.7:
                    f = float(rng.uniform(0.6, 1.4))
                    ea.k1.mul_(f)
                    eb.k1.mul_(f)
                elif isinstance(ea, (ca.HorizontalCorrector, ca.VerticalCorrector)) and rng.random() < 0.7:
                    ea.angle.mul_(-0.5)
                    eb.angle.mul_(-0.5)
            particles, survival, energy, reads = captured()
            ref = beam
            for e in els_b:
                ref = e.track(ref)
            tol = 2e-11 if dt == torch.float64 else 1e-4
            cols = ref.particles.double().abs().reshape(-1, 7).amax(dim=0) + 1e-300
            if particles.shape != ref.particles.shape:
                fails.append(f"replay: particle shapes {tuple(particles.shape)} vs {tuple(ref.particles.shape)}")
                return
            d = (particles.double() - ref.particles.double()).abs().reshape(-1, 7).amax(dim=0) / cols
            if not bool((d <= tol).all()):
                fails.append(f"replay: particles per-column error {[f'{float(v):.2e}' for v in d]}")
            flips = int(((survival - ref.survival_probabilities).abs() > tol).sum()) if survival.shape == ref.survival_probabilities.shape else 99
            if flips > (3 if dt == torch.float32 else 0):
                fails.append(f"replay: survival differs in {flips} entries")
            compare(energy, ref.energy, 1e-12 if dt == torch.float64 else 2e-7, "replay: energy", fails)
            if flips:
                return
            want = [e.reading for e in els_b if (isinstance(e, ca.BPM) and e.is_active) or (isinstance(e, ca.Screen) and (e.method == "cloud-in-cell" or beam.particles.dim() == 2))]
            for ra, rb in zip(reads, want):
                if dt == torch.float32 and ra.dim() >= 2:
                    differing = int(((ra.double() - rb.double()).abs() > 2e-4 * rb.double().abs().amax()).sum())
                    if differing > 8:
                        fails.append(f"replay: screen reading differs in {differing} pixels")
                else:
                    compare(ra, rb, 1e-9 if dt == torch.float64 else 3e-5, "replay: reading", fails,
                            scale=torch.tensor(3e-4) if ra.shape[-1] == 2 and ra.dim() <= 2 else None)
            if fails:
                return


def observables(seg, els_b, beam, dt, fails):
    """`Segment.track_moments` (the last run fused with the moment reduction; exact and with the moments transported algebraically)
    against the moments of the beam the walk tracks."""
    ref = beam
    for e in els_b:
        ref = e.track(ref)
    want = ref.as_parameter_beam()
    sig = want.cov.diagonal(dim1=-2, dim2=-1)[..., :6].abs().sqrt()
    for exact in (True, False):
        got = seg.track_moments(beam, exact=exact)
        tol = (1e-9 if dt == torch.float64 else 2e-4) * (1 if exact else 50)
        if got.mu.shape != want.mu.shape or got.cov.shape != want.cov.shape:
            fails.append(f"track_moments(exact={exact}): shapes {tuple(got.mu.shape)} {tuple(got.cov.shape)} vs {tuple(want.mu.shape)} {tuple(want.cov.shape)}")
            continue
        if bool((torch.isnan(got.mu[..., :6]) != torch.isnan(want.mu[..., :6])).any()) \
                or bool((torch.isnan(got.cov[..., :6, :6]) != torch.isnan(want.cov[..., :6, :6])).any()):
            fails.append(f"track_moments(exact={exact}): NaNs in different places")
            continue
        dmu = torch.nan_to_num((got.mu[..., :6] - want.mu[..., :6]).abs() / (sig + want.mu[..., :6].abs() + 1e-300), nan=0.0).amax()
        scale = sig.unsqueeze(-1) * sig.unsqueeze(-2) + 1e-300
        dcov = torch.nan_to_num((got.cov[..., :6, :6] - want.cov[..., :6, :6]).abs() / scale, nan=0.0).amax()
        if not bool(dmu <= tol) or not bool(dcov <= tol):
            fails.append(f"track_moments(exact={exact}): mu {float(dmu):.2e} cov {float(dcov):.2e} (allowed {tol:.1e})")
    compare(got.energy, want.energy, 1e-12 if dt == torch.float64 else 2e-7, "track_moments energy", fails)


def in_layout(lrng, value):
    """`value` (a 0-d or (2,) setting) in a drawn layout, as a control loop hands it over: itself, an element or a row of a larger
    tensor (an offset), a column of a (2, K) matrix (stride K), every second entry of a (4,) tensor (stride 2), a 0-d tensor expanded
    to (2,) (stride 0). Returns (the tensor to assign, its base). The other entries of the base hold other values."""
    r = lrng.random()
    junk = float(lrng.normal()) * 3e-3
    if value.dim() == 0:
        if r < 0.4:
            return value, value
        base = torch.full((5,), junk, dtype=value.dtype, device=value.device)
        base[3] = value
        return base[3], base
    if value.shape != (2,) or r < 0.2:
        return value, value
    if r < 0.4:
        base = torch.full((4, 2), junk, dtype=value.dtype, device=value.device)
        base[2] = value
        return base[2], base
    if r < 0.6:
        base = torch.full((2, 3), junk, dtype=value.dtype, device=value.device)
        base[:, 1] = value
        return base[:, 1], base
    if r < 0.8:
        base = torch.full((4,), junk, dtype=value.dtype, device=value.device)
        base[::2] = value
        return base[::2], base
    base = torch.full((3,), junk, dtype=value.dtype, device=value.device)
    base[1] = value[0]
    return base[1].expand(2), base


def assign(lrng, ea, eb, name, value):
    """`value` assigned to setting `name` of `ea` in a drawn layout (sometimes with its base edited in place afterwards), a contiguous
    copy of the same values to `eb`."""
    view, base = in_layout(lrng, value)
    setattr(ea, name, view)
    if base is not view and lrng.random() < 0.3:
        with torch.no_grad():
            base.mul_(float(lrng.uniform(0.5, 1.5)))     # (the walk's copy gets the values the view shows afterwards)
    setattr(eb, name, view.detach().clone().contiguous())


def mutate(rng, els_a, els_b, fk, layouts=None):
    """Between two tracks of the same Segment: settings edited in place, assigned as new tensors, diagnostics switched — the same on
    both copies (the plans `Segment.track` keeps must follow). With `layouts` (a generator of its own, so that `rng` draws what it
    always drew): the tensors assigned to `ea` come in drawn layouts (`in_layout`), and Quadrupoles and Solenoids get new
    misalignments."""
    lrng = layouts
    for ea, eb in zip(els_a, els_b):
        r = rng.random()
        if isinstance(ea, ca.Quadrupole) and r < 0.5:
            f = float(rng.uniform(0.5, 1.5))
            if rng.random() < 0.5:
                with torch.no_grad():
                    ea.k1.mul_(f)
                    eb.k1.mul_(f)
            elif lrng is not None:
                assign(lrng, ea, eb, "k1", ea.k1 * f)
            else:
                ea.k1 = ea.k1 * f
                eb.k1 = eb.k1 * f
        elif isinstance(ea, (ca.HorizontalCorrector, ca.VerticalCorrector)) and r < 0.5:
            v = torch.tensor(float(rng.uniform(-2e-4, 2e-4)), **fk)
            if ea.angle.dim() == 0:
                if lrng is not None:
                    assign(lrng, ea, eb, "angle", v)
                else:
                    ea.angle = v
                    eb.angle = v.clone()
        elif isinstance(ea, ca.BPM) and r < 0.3:
            ea.is_active = eb.is_active = not ea.is_active
        elif isinstance(ea, ca.Cavity) and r < 0.4:
            with torch.no_grad():
                ea.phase.add_(5.0)
                eb.phase.add_(5.0)
        elif isinstance(ea, ca.Drift) and r < 0.1:
            f = float(rng.uniform(0.8, 1.2))
            if lrng is not None:
                assign(lrng, ea, eb, "length", ea.length * f)
            else:
                ea.length = ea.length * f
                eb.length = eb.length * f
        if lrng is not None and isinstance(ea, (ca.Quadrupole, ca.Solenoid)) and ea.misalignment.shape == (2,) \
                and lrng.random() < 0.4:
            assign(lrng, ea, eb, "misalignment", torch.tensor(lrng.normal(size=2) * 1e-4, **fk))


def reading_or_refusal(screen):
    try:
        return screen.reading
    except NotImplementedError as exc:
        return exc


def check(seg, els_a, els_b, beam, dt, fails, tag):
    n0 = len(fails)
    out = seg.track(beam)
    ref = beam
    for e in els_b:
        ref = e.track(ref)
    tol = 2e-11 if dt == torch.float64 else 1e-4        # (float32: a composed map of a dozen strong elements against their maps one by one)
    cols = out.particles.double().abs().reshape(-1, 7).amax(dim=0)
    if out.particles.shape != ref.particles.shape:
        fails.append(f"particles: shapes {tuple(out.particles.shape)} vs {tuple(ref.particles.shape)}")
    else:
        d = (out.particles.double() - ref.particles.double()).abs().reshape(-1, 7).amax(dim=0) / (cols + 1e-300)
        if not bool((d <= tol).all()):
            fails.append(f"particles: per-column error {[f'{float(v):.2e}' for v in d]} (allowed {tol:.1e})")
    # (a float32 row within rounding of an aperture's edge survives on one path and not on the other — a composed map against the
    # elements' maps one by one: a few flips are rounding, and what is read behind them differs by those particles' weights)
    flips = 0
    sa, sb = out.survival_probabilities, ref.survival_probabilities
    if sa.shape == sb.shape and dt == torch.float32:
        flips = int(((sa - sb).abs() > tol).sum())
        if flips > 3:
            fails.append(f"survival: {flips} entries differ")
    else:
        compare(sa, sb, tol, "survival", fails, scale=torch.tensor(1.0))
    compare(out.energy, ref.energy, 1e-12 if dt == torch.float64 else 2e-7, "energy", fails)
    compare(out.s, ref.s, 1e-12 if dt == torch.float64 else 1e-6, "s", fails)
    for ea, eb in zip(els_a, els_b):
        if flips:
            break
        if isinstance(ea, ca.BPM) and ea.is_active:
            compare(ea.reading, eb.reading, tol, "BPM reading", fails, scale=torch.tensor(3e-4))
        if isinstance(ea, ca.Screen):
            ra, rb = reading_or_refusal(ea), reading_or_refusal(eb)
            if isinstance(ra, Exception) or isinstance(rb, Exception):      # (screen.py:292-294: 'histogram' refuses vectorised beams)
                if type(ra) is not type(rb):
                    fails.append(f"screen reading: {type(ra).__name__} vs {type(rb).__name__}")
                continue
            if dt == torch.float32:
                # a float32 row that lands within rounding of a bin edge ('histogram') or of the screen's outer edge (either method:
                # out-of-bounds particles contribute nothing) falls on the other side of it on one of the two paths (a composed map
                # against the elements' maps one by one): a few pixels may differ by one particle's charge
                differing = int(((ra.double() - rb.double()).abs() > 2e-4 * rb.double().abs().amax()).sum())
                if differing > 8 or abs(float(ra.double().sum() - rb.double().sum())) > 1e-5 * abs(float(rb.double().sum())):
                    fails.append(f"screen reading ({ea.method}): {differing} pixels differ")
            else:
                compare(ra, rb, 1e-9 if dt == torch.float64 else 2e-4, "screen reading", fails)
    fails[n0:] = [tag + f for f in fails[n0:]]


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    bad = 0
    from cheetah_amd.accelerator import _planner

    for seed in range(first, first + n_cases):
        try:
            specs, dt, B, n, fails = one_case(seed)
        except Exception as exc:  # noqa: BLE001
            specs, dt, B, n, fails = None, None, None, None, [f"raised {type(exc).__name__}: {str(exc)[:300]}"]
        if fails:
            bad += 1
            print(f"seed {seed} dtype {dt} B {B} N {n}: " + "; ".join(fails))
            if specs is not None:
                print("   lattice: " + " ".join(k + (("[" + v.get("tracking_method", "") + "]") if v.get("tracking_method") else "") for k, v in specs))
    print(f"{n_cases - bad} of {n_cases} cases agree; paths taken: { {k: v for k, v in _planner.TAKEN.items() if v} }")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
