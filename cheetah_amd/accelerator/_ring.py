"""The lattice taken as a ring: `Segment.track_turns` (the fused turn kernels `chx_second_order_turns` / `chx_dkd_turns` and the
general loop over `track`) and the linear optics of a ring of drift-kick-drift elements — `one_turn_map`, `closed_orbit`,
`ring_optics`, `radiation_integrals`, `chromaticity`, `ring_sensitivity` (`chx_dkd_ring_jacobian`, `chx_dkd_ring_sensitivity`,
`chx_dkd_ring_radiation`). The public methods of `Segment` carry the user documentation and forward here; every function takes the
segment as its first argument.

What a ring item is comes from `accelerator/_nonlinear.py` (`dkd_item`, `second_order_items`): the ring asks the rule `Segment.track`
asks, and adds its own conditions (the whole plan, one arithmetic class, the kinds the kernels keep in registers)."""
from __future__ import annotations

import collections
import math

import torch

from .. import _ops
from ..particles import optics as _optics
from ..particles import turns as _turns
from ..particles.particle_beam import ParticleBeam
from ..particles.species import Species
# (the segment MODULE: `Segment.track` is read from it at call time)
from . import _nonlinear, segment

#: what `turn_items` hands `track_turns_fused` for a ring of drift-kick-drift elements (chx_dkd_turns): per element the
#: kind, the (1, P) parameter tensor, num_steps and fringe_at; `storage` = the ring's one arithmetic mode
_DkdRing = collections.namedtuple("_DkdRing", "kinds params num_steps fringe_at storage")
#: the electrons `one_turn_map`, `closed_orbit` and `ring_optics` take for `species=None`, by (dtype, device)
_DEFAULT_SPECIES = {}


def _overrides_track(seg) -> bool:
    return type(seg).track is not segment.Segment.track or type(seg)._track_internal is not segment.Segment._track_internal


# ---- multi-turn tracking --------------------------------------------------------------------------------------------------------------------
def turn_items(seg, incoming: ParticleBeam):
    """(maps, lengths, linear) when the WHOLE lattice is one stretch the fused turn kernel takes — second-order elements and
    merged linear runs as in `_nonlinear.second_order_run`, or a single merged linear run —, a `_DkdRing` when it is a ring of
    drift-kick-drift elements instead (`turn_items_dkd`), else the reason (a str) why neither."""
    x, energy = incoming.particles, incoming.energy
    reason = _nonlinear.plain_beam(x, energy, incoming.s, True, False)
    if reason is not None:
        return reason
    # the kernel reads the weights as N values of the particles' dtype through their addresses: nothing else may reach it (a
    # beam with vectorised charges, (B, N) under particles (N, 7), is a vectorised beam: the general path)
    for name, wt in (("particle_charges", incoming.particle_charges), ("survival_probabilities", incoming.survival_probabilities)):
        if wt.shape != x.shape[:1] or wt.dtype != x.dtype or wt.device != x.device:
            return f"the beam's {name} are not one (N,) tensor of the particles' dtype on their device"
    if _overrides_track(seg):
        return "the segment overrides `track`"
    plan = seg._plan()
    if not plan:
        return "the lattice holds nothing to track"
    # (the caller runs under no_grad, so the `grad` flag is False here and `second_order_items` skips its own requires_grad
    # tests: trainable settings are turned away by the sweep over `tensors` below)
    maps, lengths, linear, tensors, j, _ = _nonlinear.second_order_items(seg, plan, 0, x, energy, incoming.species, torch.is_grad_enabled())
    if j < len(plan):
        kind, item = plan[j]
        what = "a run of linear elements that does not qualify (vectorised or trainable settings, or the run in front of a cavity)" \
            if kind == "run" else \
            f"{type(item).__name__} '{item.name}' (tracking method '{item._tracking_method}')"
        reason = f"the lattice is not one stretch of second-order and linear items: {what} ends it"
    elif not 1 <= len(maps) <= 224:
        reason = f"the lattice has {len(maps)} items, the fused kernel takes 1 to 224"
    elif any(t.requires_grad for t in tensors):
        reason = "a setting of the lattice requires grad"
    else:
        return maps, lengths, linear
    ring = turn_items_dkd(seg, plan, x)
    if isinstance(ring, str):
        return f"{reason}; nor is it a ring of drift-kick-drift elements: {ring}"
    return ring


def turn_items_dkd(seg, plan, x: torch.Tensor, trainable=()):
    """A `_DkdRing` when the WHOLE plan is a ring `chx_dkd_turns` takes — drift-kick-drift Drifts, Quadrupoles, Dipoles, Sextupoles,
    RFCavities and Multipoles as `_nonlinear.dkd_run` keeps them in registers (`_nonlinear.dkd_item`), all of one arithmetic class, 1 to
    192 of them, Markers in between skipped — else the reason (a str) why not. Nothing is kept between calls: settings and
    `dkd_precision` are read here every time. `trainable`: the ids of the settings that may require grad (the `wrt` of the ring
    optics; `track_turns` has none), or "all"."""
    kinds, params, steps, fringes, codes, tensors = [], [], [], [], [], []
    dtype, device = x.dtype, x.device
    for kind, e in plan:
        if kind == "run":
            if _nonlinear.identity_run(e):
                continue                                   # Markers between two magnets: nothing to apply, s + 0
            return "a run of linear elements stands in the ring (its map depends on the reference energy in front of it, and an " \
                   "energy that drifts from turn to turn would need a map per turn: left to the general path on purpose)"
        a = _nonlinear.dkd_item(e, dtype, device, True)
        if isinstance(a, str):
            return a
        k, p, n, f, code, refs = a
        kinds.append(k)
        params.append(p)
        steps.append(n)
        fringes.append(f)
        codes.append(code)
        tensors += refs
    if not 1 <= len(kinds) <= 192:
        return f"the ring has {len(kinds)} drift-kick-drift elements, the fused kernel takes 1 to 192"
    classes = _nonlinear.arithmetic_classes(codes, dtype)
    if len(set(classes)) > 1:
        return "the elements' `dkd_precision` settings put them into more than one arithmetic class (one launch evaluates one)"
    if trainable != "all" and any(t.requires_grad and id(t) not in trainable for t in tensors):
        return "a setting of the lattice requires grad"
    return _DkdRing(kinds, params, steps, fringes, classes[0])


def track_turns(seg, incoming: ParticleBeam, num_turns: int, record_every: int, aperture, record_first: int, fused):
    if not isinstance(incoming, ParticleBeam):
        raise TypeError(f"track_turns takes a ParticleBeam, got {type(incoming)}")
    num_turns, record_every, record_first = int(num_turns), int(record_every), int(record_first)
    if num_turns < 1 or record_every < 1:
        raise ValueError("num_turns and record_every must be at least 1")
    x = incoming.particles
    if record_first < 0 or record_first > x.shape[-2]:
        raise ValueError(f"record_first = {record_first} is not within 0 .. {x.shape[-2]} (the number of particles)")
    sp = incoming.species
    if any(t.requires_grad for t in (x, incoming.energy, incoming.s, incoming.particle_charges, incoming.survival_probabilities,
                                     sp.mass_eV, sp.num_elementary_charges)) or (aperture is not None and aperture.requires_grad):
        raise ValueError("track_turns has no autograd: an input requires grad")
    if aperture is not None and (aperture.shape != (2,) or aperture.dtype != x.dtype or aperture.device != x.device):
        raise ValueError("aperture must be a tensor (a_x, a_y) of the beam's dtype on its device")
    with torch.no_grad():
        items = "fused=False" if fused is False else turn_items(seg, incoming)
        if isinstance(items, str):
            if fused:
                raise ValueError(f"track_turns(fused=True): {items}")
            return track_turns_general(seg, incoming, num_turns, record_every, aperture, record_first)
        return track_turns_fused(incoming, items, num_turns, record_every, aperture, record_first)


def track_turns_fused(incoming, items, num_turns, record_every, aperture, record_first):
    dkd = isinstance(items, _DkdRing)
    x = _ops.aligned(incoming.particles)
    N, E, dev = x.shape[0], len(items[0]), x.device
    _ops.check_current_device(dev)
    charges, survival = _ops.aligned(incoming.particle_charges), _ops.aligned(incoming.survival_probabilities)
    if aperture is not None and not aperture.is_contiguous():
        raise ValueError("aperture must be contiguous (it is read through its address)")
    R = num_turns // record_every
    if dkd:
        ws_bytes = lambda records, turns=1: _ops.dkd_turns_workspace_bytes(E, N, turns, records, x.dtype)  # noqa: E731
    else:
        ws_bytes = lambda records, turns=1: _ops.second_order_turns_workspace_bytes(E, N, records, x.dtype)  # noqa: E731
    per_record = ws_bytes(1) - ws_bytes(0)
    chunks = _turns.plan_chunks(num_turns, E, record_every, per_record, _turns._MAX_ITEM_STEPS, _turns._MAX_PARTIAL_BYTES)
    # the coefficient block (a drift-kick-drift ring: a block of constants per turn of a launch, the worst case of a drifting
    # reference energy) and the partials: an allocation of its own, sized for the longest launch and the one that records most
    ws = _ops.workspace(ws_bytes(max(_turns.chunk_records(f, n, record_every) for f, n in chunks), max(n for _, n in chunks)), dev)
    out = torch.empty_like(x)
    lost = torch.zeros(N, dtype=torch.int32, device=dev)
    sums = torch.empty((R, _turns.NUM_SUMS), dtype=torch.float64, device=dev)
    probe = torch.empty((R, record_first, 7), dtype=x.dtype, device=dev) if record_first else None
    s_one = torch.empty_like(incoming.s)
    energy = incoming.energy
    if dkd:
        # the reference energy travels from launch to launch through one device scalar: behind the call the energy behind
        # the last turn
        sp = incoming.species
        arrays = _ops.dkd_turn_arrays(items.kinds, items.params, items.num_steps, items.fringe_at)
        energy = torch.empty_like(incoming.energy)
        for first, n in chunks:
            _ops.dkd_turns(arrays, items.storage, E, x if first == 1 else out, out, incoming.energy if first == 1 else energy, energy,
                           sp.mass_eV_float, sp.num_elementary_charges_float, charges, survival, first, n, record_every, aperture,
                           lost, sums, probe, ws, incoming.s if first == 1 else None, s_one if first == 1 else None)
    else:
        maps, lengths, linear = items
        ptrs = _ops.second_order_turn_ptrs(maps, lengths, linear)
        for first, n in chunks:
            _ops.second_order_turns(ptrs, E, x if first == 1 else out, out, charges, survival, first, n, record_every, aperture, lost,
                                    sums, probe, ws, incoming.s if first == 1 else None, s_one if first == 1 else None)
    s_out = incoming.s + num_turns * (s_one - incoming.s)
    beam = ParticleBeam(out, energy, particle_charges=incoming.particle_charges,
                        survival_probabilities=incoming.survival_probabilities * (lost == 0), s=s_out, species=incoming.species)
    return _turns.TurnByTurn(beam, lost, _turns.recorded_turns(num_turns, record_every, dev), sums, probe, record_every=record_every)


def track_turns_general(seg, incoming, num_turns, record_every, aperture, record_first):
    x = incoming.particles
    dev = x.device
    w = incoming.particle_charges.to(torch.float64) * incoming.survival_probabilities.to(torch.float64)
    lost = torch.zeros(x.shape[:-1], dtype=torch.int32, device=dev)     # (batch dimensions of a vectorised beam in front)
    beam, sums, probe, s_one = incoming, [], [], None
    for t in range(1, num_turns + 1):
        before = beam.particles
        beam = seg.track(beam)
        if t == 1:
            s_one = beam.s
        alive_before = lost == 0
        xt = torch.where(alive_before.unsqueeze(-1), beam.particles, before)     # a lost particle stands where it was lost
        lost = torch.where(alive_before & _turns.is_lost(xt, aperture), torch.full_like(lost, t), lost)
        # (survival 0 from the turn of the loss on: a collective kick of the lattice no longer counts the particle's charge)
        beam = ParticleBeam(xt, beam.energy, particle_charges=beam.particle_charges,
                            survival_probabilities=beam.survival_probabilities * (lost == 0), s=beam.s, species=beam.species)
        if t % record_every == 0:
            sums.append(_turns.record_sums(xt, lost == 0, w))
            if record_first:
                probe.append(xt[..., :record_first, :].clone())
    beam = ParticleBeam(beam.particles, beam.energy, particle_charges=beam.particle_charges,
                        survival_probabilities=beam.survival_probabilities, s=incoming.s + num_turns * (s_one - incoming.s),
                        species=beam.species)
    lead = tuple(beam.particles.shape[:-2])
    sums = torch.stack(sums) if sums else torch.empty((0, *lead, _turns.NUM_SUMS), dtype=torch.float64, device=dev)
    if record_first:
        probe = torch.stack(probe) if probe else torch.empty((0, *lead, record_first, 7), dtype=x.dtype, device=dev)
    return _turns.TurnByTurn(beam, lost, _turns.recorded_turns(num_turns, record_every, dev), sums, probe if record_first else None,
                             record_every=record_every)


# ---- linear optics of a ring ----------------------------------------------------------------------------------------------------------------
def ring_knobs(what: str, plan, wrt):
    """The knobs of `wrt` — a sequence of tensors, each by identity a setting `_dkd_scalar_refs()` lists for an element of the
    ring, or "all": every such setting that requires grad — as (tensors, per tensor (first knob, count, 0-d?), components
    [(knob, item, slot)], K). A 0-d setting is one knob, an (n,) setting n knobs; a tensor many elements share is one knob
    with a component per element."""
    refs = []                                              # (item, slot, tensor, index) in the ring's order
    item = 0
    for kind, e in plan:
        if kind == "run":
            continue                                       # (Markers: `turn_items_dkd` has refused every other run)
        for slot, (t, index) in enumerate(e._dkd_scalar_refs()):
            refs.append((item, slot, t, index))
        item += 1
    if isinstance(wrt, str):
        if wrt != "all":
            raise ValueError(f"{what}: wrt must be a sequence of tensors or 'all', got {wrt!r}")
        seen, wrt = set(), []
        for _, _, t, _ in refs:
            if t.requires_grad and id(t) not in seen:
                seen.add(id(t))
                wrt.append(t)
    wrt = list(wrt)
    first, layout, components = {}, [], []
    K = 0
    for pos, t in enumerate(wrt):
        if not isinstance(t, torch.Tensor) or not any(r[2] is t for r in refs):
            raise ValueError(f"{what}: wrt[{pos}] is not a setting of a drift-kick-drift element of this ring (settings are found by "
                             "identity: pass the tensor the element holds)")
        if id(t) in first:
            raise ValueError(f"{what}: wrt[{pos}] is the tensor of wrt[{[id(u) for u in wrt].index(id(t))}] again")
        first[id(t)] = K
        layout.append((K, max(t.numel(), 1), t.dim() == 0))
        K += max(t.numel(), 1)
    for item, slot, t, index in refs:
        if id(t) in first:
            components.append((first[id(t)] + (0 if index is None else int(index)), item, slot))
    return wrt, layout, components, K


def _ring_inputs(seg, what: str, energy, species, start: torch.Tensor, wrt):
    """(energy as a 0-d tensor, species, wrt as a list / "all" / None) of a ring call, checked: what `ring_jacobian` refuses before it
    looks at the lattice."""
    if not isinstance(energy, torch.Tensor):
        lengths = [e.length for e in seg._leaves() if isinstance(getattr(e, "length", None), torch.Tensor)]
        energy = torch.as_tensor(float(energy), dtype=lengths[0].dtype if lengths else torch.float64, device=start.device)
    if energy.dim() != 0 or not energy.is_floating_point():
        raise ValueError(f"{what}: the energy must be one scalar")
    if species is None:
        # one electron per dtype and device, kept: its tensors are made (and read back once) outside any graph capture
        key = (energy.dtype, energy.device)
        species = _DEFAULT_SPECIES.get(key)
        if species is None:
            species = _DEFAULT_SPECIES[key] = Species("electron", dtype=energy.dtype, device=energy.device)
            species.mass_eV_float
    if any(t.requires_grad for t in (start, energy, species.mass_eV, species.num_elementary_charges)):
        raise ValueError(f"{what} has no autograd: an input requires grad")
    if _overrides_track(seg):
        raise ValueError(f"{what}: the segment overrides `track`")
    if wrt is not None and not isinstance(wrt, str):
        try:
            wrt = list(wrt)                               # once: a generator is read here and nowhere else
        except TypeError:
            raise ValueError(f"{what}: wrt must be a sequence of tensors or 'all', got {type(wrt).__name__}") from None
    return energy, species, wrt


def ring_jacobian(seg, what: str, energy, species, start: torch.Tensor, mode: int, num_iterations: int, along: bool, wrt=None,
                  raw: bool = False, ring_call=None):
    """`_ops.dkd_ring_jacobian` for this lattice taken as a ring: the conditions of `turn_items_dkd` (whose reason a lattice
    that does not qualify is refused with), the energy as a 0-d tensor of the settings' dtype on the seeds' device.
    With `wrt` (`ring_knobs`) also `_ops.dkd_ring_sensitivity` on the orbits found: the same dict with an autograd graph to
    those settings (`particles.optics.attach_gradients`) or, with `raw`, the pair (values, tangents) as the kernels left them.
    `ring_call`: a dict that receives what a further kernel call on the same ring needs (`radiation_integrals`)."""
    energy, species, wrt = _ring_inputs(seg, what, energy, species, start, wrt)
    with torch.no_grad():
        plan = seg._plan()
        trainable = () if wrt is None else ("all" if isinstance(wrt, str) else {id(t) for t in wrt})
        ring = turn_items_dkd(seg, plan, torch.empty((0, 7), dtype=energy.dtype, device=energy.device), trainable) if plan else \
            "the lattice holds nothing to track"
        if isinstance(ring, str):
            raise ValueError(f"{what}: {ring}")
        if wrt is not None:
            wrt, layout, components, K = ring_knobs(what, plan, wrt)
        arrays = _ops.dkd_turn_arrays(ring.kinds, ring.params, ring.num_steps, ring.fringe_at)
        out = _ops.dkd_ring_jacobian(arrays, len(ring.kinds), energy, species.mass_eV_float, species.num_elementary_charges_float,
                                     start, mode, num_iterations, along)
        if ring_call is not None:
            ring_call.update(arrays=arrays, ring=ring, energy=energy, species=species)
        if wrt is None or (K == 0 and not raw):
            return out
        sens = _ops.dkd_ring_sensitivity(arrays, len(ring.kinds), energy, species.mass_eV_float, species.num_elementary_charges_float,
                                         out["orbit"], mode, components, K, along)
    if raw:
        return out, sens
    return _optics.attach_gradients(out, sens, layout, wrt, 6 if mode == 2 else 4)


def seeds(start: torch.Tensor) -> torch.Tensor:
    """(B, 6) float64 from (B, 6), (B, 7) or one such row."""
    if start.dim() == 1:
        start = start.unsqueeze(0)
    if start.dim() != 2 or start.shape[1] not in (6, 7):
        raise ValueError(f"the seeds must have the shape (B, 6) or (B, 7) or be one such row, got {tuple(start.shape)}")
    return start[:, :6].to(torch.float64).contiguous()


def rows7(x6: torch.Tensor) -> torch.Tensor:
    return torch.cat([x6, torch.ones_like(x6[..., :1])], dim=-1)


def closed_from(out: dict):
    """The `ClosedOrbit` of a `ring_jacobian` result."""
    return _optics.ClosedOrbit(rows7(out["orbit"]), out["residual"], out["matrix"], out["dispersion"])


def find_closed_orbit(seg, what, energy, species, delta, guess, longitudinal, num_iterations, along, wrt=None, raw=False, ring_call=None):
    """`ring_jacobian` in its closed-orbit modes (4-D, or 6-D with `longitudinal`) from the seeds `guess` (default: the axis) with
    `delta` written into their sixth coordinate: one orbit per value."""
    num_iterations = int(num_iterations)
    if num_iterations < 1:
        raise ValueError(f"{what}: num_iterations must be at least 1")
    if guess is not None:
        x = seeds(guess).clone()
    else:
        dev = delta.device if isinstance(delta, torch.Tensor) else (energy.device if isinstance(energy, torch.Tensor) else "cuda")
        n = delta.numel() if isinstance(delta, torch.Tensor) else 1
        x = torch.zeros((n, 6), dtype=torch.float64, device=dev)
    if delta is not None:
        d = delta.to(torch.float64).reshape(-1) if isinstance(delta, torch.Tensor) else torch.full((1,), float(delta), dtype=torch.float64, device=x.device)
        if d.requires_grad:
            raise ValueError(f"{what} has no autograd: an input requires grad")
        if d.shape[0] != x.shape[0]:
            if x.shape[0] != 1 and d.shape[0] != 1:
                raise ValueError(f"{what}: {d.shape[0]} values of delta for {x.shape[0]} guesses")
            x = x.expand(max(d.shape[0], x.shape[0]), 6).clone()
        x[:, 5] = d
    return ring_jacobian(seg, what, energy, species, x, 2 if longitudinal else 1, num_iterations, along, wrt, raw, ring_call)


def one_turn_map(seg, start, energy, species, along, wrt):
    out = ring_jacobian(seg, "one_turn_map", energy, species, seeds(start), 0, 1, along, wrt)
    if not along:
        return _optics.OneTurnMap(rows7(out["orbit"]), rows7(out["image"]), out["matrix"])
    return _optics.OneTurnMap(rows7(out["orbit"]), rows7(out["image"]), out["matrix"], rows7(out["orbit_along"]), out["matrix_along"],
                              out["s_along"])


def closed_orbit(seg, energy, species, delta, guess, longitudinal, num_iterations, wrt):
    return closed_from(find_closed_orbit(seg, "closed_orbit", energy, species, delta, guess, longitudinal, num_iterations, False, wrt))


def ring_optics(seg, energy, species, delta, guess, longitudinal, num_iterations, along, wrt):
    out = find_closed_orbit(seg, "ring_optics", energy, species, delta, guess, longitudinal, num_iterations, along, wrt)
    if not along:
        return _optics.ring_optics_from(closed_from(out))
    return _optics.ring_optics_from(closed_from(out), rows7(out["orbit_along"]), out["matrix_along"], out["s_along"])


def radiation_integrals(seg, energy, species, delta, guess, num_iterations, along):
    call = {}
    out = find_closed_orbit(seg, "radiation_integrals", energy, species, delta, guess, False, num_iterations, False, ring_call=call)
    closed = _optics.ring_optics_from(closed_from(out))
    ring, species = call["ring"], call["species"]
    with torch.no_grad():
        rad = _ops.dkd_ring_radiation(call["arrays"], len(ring.kinds), call["energy"], species.mass_eV_float,
                                      species.num_elementary_charges_float, out["orbit"], closed.beta, closed.alpha, out["dispersion"],
                                      bool(along))
        circumference = torch.cat([p[0, :1] for p in ring.params]).to(torch.float64).sum()
    return _optics.radiation_integrals_from(closed, rad["integrals"], rad.get("integrals_along"), call["energy"], species.mass_eV_float,
                                            species.num_elementary_charges_float, circumference)


def chromaticity(seg, energy, species, h, wrt) -> torch.Tensor:
    h = float(h)
    if not h > 0:
        raise ValueError("chromaticity: h must be positive")
    dev = energy.device if isinstance(energy, torch.Tensor) else "cuda"
    opt = seg.ring_optics(energy, species, delta=torch.tensor([-h, 0.0, h], dtype=torch.float64, device=dev), wrt=wrt)
    q = opt.phase_advance[:, -1, :] / (2.0 * math.pi)
    return (q[2] - q[0]) / (2.0 * h)


def ring_sensitivity(seg, energy, wrt, species, delta, guess, longitudinal, num_iterations, along):
    if wrt is None:
        raise ValueError("ring_sensitivity: wrt must be a sequence of settings or 'all'")
    out, sens = find_closed_orbit(seg, "ring_sensitivity", energy, species, delta, guess, longitudinal, num_iterations, along, wrt, True)
    return _optics.ring_sensitivity_from(closed_from(out), sens, out.get("matrix_along"))
