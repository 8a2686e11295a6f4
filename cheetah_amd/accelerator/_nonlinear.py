"""Runs of non-linear elements inside `Segment.track`: consecutive second-order or drift-kick-drift elements, and the merged runs of
linear elements between them, go to the device in ONE call with the particles in registers (`chx_second_order_chain_mixed`,
`chx_dkd_chain_mixed`). Same numbers, bit for bit, as the elements tracked one after the other (reference:
cheetah/accelerator/element.py:195-228, cheetah/accelerator/segment.py:545-574).

`second_order_run` and `dkd_run` are the two drivers (`Segment._second_order_run` / `_dkd_run` forward to them): (outgoing beam,
index behind the stretch), or None when fewer than two items qualify and the walk goes on item by item. The rules both share — and
share with the ring (`accelerator/_ring.py`) — are written once, above the drivers: which element tracks with the stock methods,
which is a drift-kick-drift item, its arithmetic class, how a linear run rides along, the partition of a list of classes into
stretches, the kept run and the outgoing beam.

`_ops.dkd_chain`, `_ops.second_order_chain`, `_ops.CAPTURING` and `Element._epoch` are read through the module / class object at
call time: a stand-in assigned there is honoured."""
from __future__ import annotations

import torch

from .. import _ops
from ..particles.particle_beam import ParticleBeam
from ._plans import _IDENTITY
from .element import Element

#: drift-kick-drift kinds chx_dkd_chain carries through a run in registers
_DKD_IN_REGISTERS = (_ops.DKD_KIND["drift"], _ops.DKD_KIND["quadrupole"], _ops.DKD_KIND["dipole"], _ops.DKD_KIND["sextupole"],
                     _ops.DKD_KIND["rfcavity"], _ops.DKD_KIND["multipole"])


# ---- the rules --------------------------------------------------------------------------------------------------------------------------
def stock(e, method: str) -> bool:
    """Does the element's class track with the stock methods: `Element.track`, the stock `_track_<method>` and `_track_internal`?"""
    cls = type(e)
    if cls.track is not Element.track or cls._track_internal is not Element._track_internal:
        return False
    return getattr(cls, method) is getattr(Element, method)


def plain_beam(x, energy, s, energy_like_x: bool, no_graph: bool):
    """None when (x, energy, s) are one plain beam a fused kernel takes — (N, 7) particles on the device, a scalar energy, a scalar
    path length of the particles' dtype on their device — else the reason. `energy_like_x`: the energy must have the particles' dtype
    and device as well (the drift-kick-drift kernels read it; the second-order run only hands it on). `no_graph`: with autograd on,
    none of the three may require grad (`track_turns` has refused such inputs before it asks)."""
    if x.dim() != 2 or not x.is_cuda:
        return "the beam is not one plain (N, 7) beam on the device"
    if energy.dim() != 0 or s.dim() != 0 or s.dtype != x.dtype or s.device != x.device or (energy_like_x and energy.dtype != x.dtype):
        return "the beam's energy and path length are not scalars of the particles' dtype on their device"
    if energy_like_x and energy.device != x.device:
        return "the beam's energy is not on the particles' device"
    if no_graph and torch.is_grad_enabled() and (x.requires_grad or energy.requires_grad or s.requires_grad):
        return "the beam carries a graph"
    return None


def identity_run(run) -> bool:
    """A run of pass-through elements only (Markers, inactive BPMs / Screens between two non-linear elements): nothing to
    apply, zero length."""
    return all(e._chx_kind == _IDENTITY and e._static_skippable and not e._parameters for e in run.elements)


def run_rides(plan, j: int):
    """What a scan over plan items does with the run plan[j]: True = it rides in the stretch as an item (`run_item`), False = it is
    skipped (Markers between two magnets: nothing to apply, s + 0), None = the scan ends in front of it — the run in front of an
    active Cavity belongs to the cavity's stretch (chx_lattice_track)."""
    if j + 1 < len(plan) and plan[j + 1][0] == "element" and plan[j + 1][1]._is_cavity:
        return None
    return not identity_run(plan[j][1])


def run_item(seg, run, x, energy, species):
    """A merged run of linear elements as an item of a stretch: (map, length, setting tensors), or None when the run does not qualify
    (vectorised or trainable settings). The map is the run's composed (7, 7) map for `energy`, the energy in front of the run
    (chx_run_map: one launch now, none while the stretch stands), in a tensor of its own — the plan's state is shared with every other
    way this run can be tracked; the length is 0 + (l_0 + l_1 + ...), the run's length as the walk adds it."""
    zero = seg.__dict__.get("_zero_s")
    if zero is None or zero.dtype != x.dtype or zero.device != x.device:
        zero = seg.__dict__["_zero_s"] = torch.zeros((), dtype=x.dtype, device=x.device)
    got = seg._run_map_fast(run, x, energy, species, zero)
    if got is None or got[1].dim() != 0 or got[1].dtype != x.dtype or got[1].device != x.device:
        return None
    return got[0].clone(), got[1], run.fast.tensors


def dkd_item(e, dtype, device, in_registers: bool):
    """Is the element a drift-kick-drift item? Its argument set (kind, (1, P) parameter tensor, num_steps, fringe_at, precision code,
    setting tensors) or the reason (a str) why not: another tracking method or no kind (`in_registers`, the ring's condition: a kind
    outside `_DKD_IN_REGISTERS`), an overridden `track`, an unknown `dkd_precision`, settings that are not all scalars of `dtype` on
    `device`. Settings and `dkd_precision` are read here every time."""
    kind, precision = e._dkd_kind, e.dkd_precision
    if e._tracking_method != "drift_kick_drift" or (kind not in _DKD_IN_REGISTERS if in_registers else kind is None):
        return f"{type(e).__name__} '{e.name}' (tracking method '{e._tracking_method}') is not a drift-kick-drift Drift, Quadrupole, Dipole, Sextupole, RFCavity or Multipole"
    if not stock(e, "_track_drift_kick_drift"):
        return f"{type(e).__name__} '{e.name}' overrides `track`"
    if precision not in _ops.DKD_PRECISION:
        return f"{type(e).__name__} '{e.name}' has the unknown dkd_precision {precision!r}"
    p = e._dkd_params_stacked(dtype, device)
    if p is None:
        return f"the settings of {type(e).__name__} '{e.name}' are not all scalars of the beam's dtype on its device (vectorised settings take the general path)"
    n, f = e._dkd_options()
    return kind, p, n, f, _ops.DKD_PRECISION[precision], [t for t, _ in e._dkd_scalar_refs()]


def arithmetic_classes(codes: list, dtype) -> list:
    """The arithmetic classes of drift-kick-drift items with the precision codes `codes` on a beam of `dtype`: float64 beams are
    evaluated in fp64 whatever `dkd_precision` says (one class, 0), else the codes. One launch evaluates one class. Entries that are
    no code (None: a linear run, -1: an item without a class) stay."""
    return [c if c is None or c < 0 else 0 for c in codes] if dtype == torch.float64 else codes


def stretch_length(classes) -> int:
    """How many items form the in-register stretch that starts at the front of `classes` — per item None (a linear run: goes with any
    class), the arithmetic class (>= 0) or -1 (a drift-kick-drift item the chain takes in element passes only): as far as runs and the
    first item's class reach; 0 when there is no item or the first one has no class. (A stretch of fewer than two items is not worth
    a call: the caller's business.)"""
    first = next((c for c in classes if c is not None), None)
    if first is None or first < 0:
        return 0
    k = 0
    while k < len(classes) and classes[k] in (None, first):
        k += 1
    return k


def fallback_length(classes) -> int:
    """Where no stretch starts: how many consecutive elements (no runs) from the front of `classes` go into one call of element
    passes — up to where a stretch could start (an item with a class whose successor is a run or of the same class); 0 for fewer
    than two."""
    if not classes or classes[0] is None:
        return 0
    k = 1
    while k < len(classes) and classes[k] is not None and not (
            classes[k] >= 0 and k + 1 < len(classes) and classes[k + 1] in (None, classes[k])):
        k += 1
    return k if k >= 2 else 0


def outgoing(incoming: ParticleBeam, particles, energy, s_out, species) -> ParticleBeam:
    """The beam behind a stretch: new coordinates, energy and path length, the weights of the incoming beam."""
    return ParticleBeam(particles, energy, particle_charges=incoming.particle_charges,
                        survival_probabilities=incoming.survival_probabilities, s=s_out, species=species)


# ---- the kept run -------------------------------------------------------------------------------------------------------------------------
# A stretch as it was found last time stands while no attribute of any element was assigned (`Element._epoch`) and no setting was
# edited in place: O(1) + one sweep over the version counters instead of ~2.5-3 us of look-ups per element. What else an entry is
# compared with is data of the entry: `energy` (None: the stretch does not depend on energy and species — drift-kick-drift elements
# without a linear run; else the same energy tensor at the same version and the same species floats) and `dkd`, the elements whose
# `dkd_precision` is compared on every hit (it may be set on the CLASS, which moves no epoch; none in a second-order run).
def kept_runs(seg, name: str, plan) -> dict:
    """{plan index: entry} of `seg.__dict__[name]` = (plan, {...}), started anew for another plan."""
    cache = seg.__dict__.get(name)
    if cache is None or cache[0] is not plan:
        cache = seg.__dict__[name] = (plan, {})
    return cache[1]


def entry_stands(ent: dict, x, energy, species, grad: bool) -> bool:
    return ent["epoch"] == Element._epoch and ent["dtype"] == x.dtype and ent["device"] == x.device \
        and [t._version for t in ent["tensors"]] == ent["versions"] and not _ops.CAPTURING[0] \
        and [e.dkd_precision for e in ent["dkd"]] == ent["precisions"] \
        and not (grad and any(t.requires_grad for t in ent["tensors"])) \
        and (ent["energy"] is None or (ent["energy"] is energy and ent["energy_version"] == energy._version
                                       and ent["mass"] == species.mass_eV_float
                                       and ent["nq"] == species.num_elementary_charges_float))


def make_entry(x, tensors, end: int, energy, species, dkd=(), **call) -> dict:
    """An entry for `entry_stands`: `energy` None or the tensor to compare, `dkd` the elements whose precision is compared, `end` the
    plan index behind the stretch, `call` what the op call of a hit takes."""
    return {"epoch": Element._epoch, "dtype": x.dtype, "device": x.device, "tensors": tensors, "versions": [t._version for t in tensors],
            "end": end, "energy": energy, "energy_version": None if energy is None else energy._version,
            "mass": species.mass_eV_float, "nq": species.num_elementary_charges_float, "dkd": dkd,
            "precisions": [e.dkd_precision for e in dkd], **call}


def stable_energy(ent: dict, energy: torch.Tensor, mass: float, e_out: torch.Tensor) -> torch.Tensor:
    """The reference energy behind a cached drift-kick-drift stretch as the SAME tensor object from track to track while the
    incoming energy is the same tensor at the same version (then the value is the same): what stands downstream and depends
    on the energy — run maps of a later stretch, second-order maps — recognises it by identity and keeps its own products.
    A tensor somebody edited in place since is not handed out again."""
    last = ent.get("e_out")
    if last is not None and ent["e_in"] is energy and ent["e_in_version"] == energy._version and ent["e_mass"] == mass \
            and last._version == ent["e_out_version"]:
        return last
    ent["e_in"], ent["e_in_version"], ent["e_mass"], ent["e_out"], ent["e_out_version"] = energy, energy._version, mass, e_out, \
        e_out._version
    return e_out


# ---- second-order elements ------------------------------------------------------------------------------------------------------------------
def second_order_run(seg, plan, i: int, incoming: ParticleBeam):
    """plan[i] and what follows it as one `chx_second_order_chain_mixed` call — second-order elements and the merged runs of
    linear elements between them (a lattice whose drifts are linear and whose magnets second order): (outgoing beam, index
    behind the stretch), or None when fewer than two items or no second-order element qualify (one plain beam without a
    graph, (7, 7, 7) maps and scalar lengths of the beam's dtype without gradients, the stock `track`; runs with scalar
    settings). Same numbers as the walk item by item."""
    x, energy, s = incoming.particles, incoming.energy, incoming.s
    if plain_beam(x, energy, s, False, True) is not None:
        return None
    grad = torch.is_grad_enabled()
    species = incoming.species
    kept = kept_runs(seg, "_so_run_cache", plan)
    ent = kept.get(i)
    if ent is not None and entry_stands(ent, x, energy, species, grad):
        out, s_out, _ = _ops.second_order_chain(ent["maps"], ent["lengths"], x, s, ent["ptrs"])
        return outgoing(incoming, out, energy, s_out, species), ent["end"]
    maps, lengths, linear, tensors, j, last_so = second_order_items(seg, plan, i, x, energy, species, grad)
    if last_so is None or len(maps) < 2:
        return None
    out, s_out, ptrs = _ops.second_order_chain(maps, lengths, x, s, linear=linear)
    if not _ops.CAPTURING[0] and not any(t.requires_grad for t in tensors) and not energy.requires_grad:
        # (maps of tensors that carry gradients are rebuilt on every track, Element._cached_map: nothing to keep)
        kept[i] = make_entry(x, tensors, j, energy, species, maps=maps, lengths=lengths, ptrs=ptrs)
    return outgoing(incoming, out, energy, s_out, species), j


def second_order_items(seg, plan, i: int, x: torch.Tensor, energy: torch.Tensor, species, grad: bool):
    """The items of the stretch that begins at plan[i], as `chx_second_order_chain_mixed` and `chx_second_order_turns` take
    them: (maps, lengths, linear flags, setting tensors, index behind the stretch, index of the last second-order element or
    None). Second-order elements give their (7, 7, 7) map, a merged run of linear elements its composed (7, 7) map (a copy)
    and its summed length; the stretch ends in front of the first item that does not qualify."""
    maps, lengths, linear, tensors = [], [], [], []
    j, last_so = i, None
    while j < len(plan):
        kind, e = plan[j]
        if kind == "run":
            rides = run_rides(plan, j)
            if rides is None:
                break
            if rides:
                item = run_item(seg, e, x, energy, species)
                if item is None:
                    break
                maps.append(item[0])
                lengths.append(item[1])
                linear.append(1)
                tensors += item[2]
        elif kind == "element":
            if e._tracking_method != "second_order" or e._t_kind is None or not stock(e, "_track_second_order"):
                break
            length = e.length
            if length.dim() != 0 or length.dtype != x.dtype or length.device != x.device or (grad and length.requires_grad):
                break
            T = e.second_order_transfer_map(energy, species)
            if T.dim() != 3 or T.dtype != x.dtype or T.device != x.device or (grad and T.requires_grad):
                break
            maps.append(T if T.is_contiguous() else T.contiguous())
            lengths.append(length)
            linear.append(0)
            tensors += e._feature_key()[1]
            last_so = j
        else:
            break
        j += 1
    return maps, lengths, linear, tensors, j, last_so


# ---- drift-kick-drift elements ----------------------------------------------------------------------------------------------------------------
def dkd_run(seg, plan, i: int, incoming: ParticleBeam):
    """plan[i] and the drift-kick-drift elements behind it as one `chx_dkd_chain_mixed` call: (outgoing beam, index behind
    the run), or None when fewer than two items qualify (one plain beam without a graph; scalar settings of the beam's
    dtype that carry no gradient; the stock `track`) — then `Element.track` takes each of them as before. Drifts,
    Quadrupoles, Dipoles, Sextupoles, RFCavities and Multipoles of one arithmetic mode keep the particles in registers, and the merged
    runs of linear elements between them (a lattice whose drifts are linear and whose magnets drift-kick-drift) ride in the same pass."""
    x, energy, s = incoming.particles, incoming.energy, incoming.s
    if plain_beam(x, energy, s, True, True) is not None:
        return None
    grad = torch.is_grad_enabled()
    species = incoming.species
    kept = kept_runs(seg, "_dkd_run_cache", plan)
    ent = kept.get(i)
    if ent is not None and entry_stands(ent, x, energy, species, grad):
        out, e_out, s_out, _ = _ops.dkd_chain(ent["kinds"], ent["params"], None, None, None, x, energy, s, species.mass_eV_float,
                                              species.num_elementary_charges_float, ent["arrays"])
        return outgoing(incoming, out, stable_energy(ent, energy, species.mass_eV_float, e_out), s_out, species), ent["end"]
    seq, after = dkd_scan(plan, i, x)
    # the arithmetic class of every item: a linear run goes with any (None); items the chain keeps in registers with their
    # `dkd_precision`; anything else has none (-1)
    plain = x.dtype in (torch.float32, torch.float64)
    classes = arithmetic_classes([None if a is None else (a[4] if plain and a[0] in _DKD_IN_REGISTERS else -1) for _, a in seq], x.dtype)
    if all(c is None for c in classes):
        return None
    k = stretch_length(classes)
    while k >= 2:
        # a stretch whose particles stay in registers: seq[:k]
        call = dkd_stretch_call(seg, seq[:k], x, energy, species)
        if isinstance(call, int):
            k = call                                       # the stretch ends in front of the run that does not qualify
            continue
        if not call["dkd"]:
            return None
        return dkd_launch(kept, i, incoming, x, energy, s, species, call, after[k - 1])
    # no such stretch starts here: consecutive drift-kick-drift elements (no runs) in one call, element passes, up to where
    # a stretch could start
    k = fallback_length(classes)
    if k < 2:
        return None
    args = [a for _, a in seq[:k]]
    call = {"kinds": [a[0] for a in args], "params": [a[1] for a in args], "steps": [a[2] for a in args], "fringes": [a[3] for a in args],
            "storage": [a[4] for a in args], "lengths": None, "tensors": [t for a in args for t in a[5]], "dkd": [obj for obj, _ in seq[:k]]}
    return dkd_launch(kept, i, incoming, x, energy, s, species, call, after[k - 1])


def dkd_scan(plan, i: int, x: torch.Tensor):
    """What stands at plan[i:]: (seq, after) with seq = [(element, argument set of `dkd_item`) | (run, None)] as far as drift-kick-drift
    elements that qualify and runs of linear elements reach, and after[k] = the plan index behind item k (and the Markers behind
    it)."""
    seq, after = [], []
    j = i
    while j < len(plan):
        kind, e = plan[j]
        if kind == "run":
            rides = run_rides(plan, j)
            if rides is None:
                break
            if not rides:
                j += 1
                if after:
                    after[-1] = j
                continue
            seq.append((e, None))
        elif kind == "element":
            a = dkd_item(e, x.dtype, x.device, False)
            if isinstance(a, str):
                break                                      # (any reason: the stretch ends here)
            seq.append((e, a))
        else:
            break
        j += 1
        after.append(j)
    return seq, after


def dkd_stretch_call(seg, items, x, energy, species):
    """The arguments of `_ops.dkd_chain` for a stretch `items` (of `dkd_scan`) of one arithmetic class — a dict for `dkd_launch` — or
    the position of the first linear run that does not qualify (`run_item`). Each run's map is built for the reference energy in
    front of it (`_ops.dkd_energy_chain`: every drift-kick-drift element hands on the float round trip of its own)."""
    kinds = [_ops.DKD_LINEAR if a is None else a[0] for _, a in items]
    has_runs = _ops.DKD_LINEAR in kinds
    params, lengths, steps, fringes, storage, tensors = [], [], [], [], [], []
    energies = _ops.dkd_energy_chain(kinds, energy, species.mass_eV_float) if has_runs else None
    for r, (obj, a) in enumerate(items):
        length = None
        if a is None:
            item = run_item(seg, obj, x, energy if r == 0 else energies[r - 1], species)
            if item is None:
                return r
            a, length = (_ops.DKD_LINEAR, item[0], 1, 0, 0, item[2]), item[1]
        params.append(a[1])
        lengths.append(length)
        steps.append(a[2])
        fringes.append(a[3])
        storage.append(a[4])
        tensors += a[5]
    return {"kinds": kinds, "params": params, "steps": steps, "fringes": fringes, "storage": storage,
            "lengths": lengths if has_runs else None, "tensors": tensors, "dkd": [obj for obj, a in items if a is not None]}


def dkd_launch(kept: dict, i: int, incoming, x, energy, s, species, call: dict, end: int):
    """One `_ops.dkd_chain` call for the arguments `call`, kept for the next track unless a device graph records."""
    out, e_out, s_out, arrays = _ops.dkd_chain(call["kinds"], call["params"], call["steps"], call["fringes"], call["storage"], x, energy,
                                               s, species.mass_eV_float, species.num_elementary_charges_float, lengths=call["lengths"])
    if not _ops.CAPTURING[0]:
        # (with linear runs inside — `lengths` — the entry also stands only for the same energy tensor at the same version and the
        # same species: their maps depend on both)
        kept[i] = make_entry(x, call["tensors"], end, energy if call["lengths"] is not None else None, species, call["dkd"],
                             kinds=call["kinds"], params=call["params"], lengths=call["lengths"], arrays=arrays)   # (`arrays` holds addresses: the tensors stay referenced)
    return outgoing(incoming, out, e_out, s_out, species), end
