"""The stretch call of `Segment.track`: plan items [run | active Cavity | BPM | Aperture | active Screen]+ taken as ONE call of the
host step (`chx_lattice_track*` for a ParticleBeam, `chx_parameter_lattice_track*` for a ParameterBeam) — every map, energy and
the path length from one preparation launch, the beam through all items in the other. Same numbers, bit for bit, as the walk item
by item (reference: cheetah/accelerator/segment.py:545-574), which costs two launches and 20-160 us of host time per item.

`track_particles` and `track_parameter` are the two drivers (`Segment._lattice_stretch*` forward to them): (outgoing beam, index
behind the stretch), or None when the stretch declines and the walk goes on item by item. What the two beam types share is written
once, above the drivers."""
from __future__ import annotations

import torch

from .. import _lib, _ops
# (the segment MODULE: `_HOST`, `_TORCH_HOST`, `_CHECK_PLANS` and the class attributes are read from it at call time — tests put
# spies and switches there, and a name imported from it would go past them)
from . import segment
from ..particles.parameter_beam import ParameterBeam
from ..particles.particle_beam import ParticleBeam
from ._plans import _FastRun, _LatticePlan
from .cavity import _narrow_to
from .element import Element
from .screen import Screen


# ---- what both beam types share ------------------------------------------------------------------------------------------------------
def joins(kind, item, screens=True, apertures=True) -> bool:
    """May this plan item be part of a stretch? (`screens` / `apertures` False: such an element ends it.)"""
    return kind == "run" or item._is_cavity or item._is_bpm or (apertures and item._is_aperture) or (screens and item._is_screen)


def extent(plan, i: int, with_screens: bool) -> tuple:
    """(j, special): plan[i:j] is as far as a stretch from plan[i] reaches, `special` of its items are no runs (cavities, active
    BPMs, apertures, screens: what makes a stretch worth one call)."""
    j, special = i, 0
    while j < len(plan) and joins(*plan[j], screens=with_screens):
        special += plan[j][0] != "run"
        j += 1
    return j, special


def _entry(seg, plan, i: int, key: tuple, worth: bool = True):
    """The cache entry of the stretch from plan[i] — False (no stretch) or [end, _LatticePlan or None] — under `key` = (i, dtype,
    device, ..., with_screens), in the table of `plan` (one per partition of the lattice that `Segment._plan` keeps)."""
    cache = seg.__dict__.get("_lattice_cache")
    if cache is None or cache[0] is not plan:
        store = seg.__dict__.get("_lattice_store")
        if store is None:                    # (never asked, or a copy: derived state does not travel)
            store = seg.__dict__["_lattice_store"] = {}
        cache = store.get(id(plan))
        if cache is None or cache[0] is not plan:
            if len(store) >= 8:
                store.clear()
            cache = store[id(plan)] = (plan, {})
        seg.__dict__["_lattice_cache"] = cache
    entry = cache[1].get(key)
    if entry is None:
        j, special = extent(plan, i, key[-1])
        entry = cache[1][key] = False if (j - i < 2 or special == 0 or not worth) else [j, None]
    return entry


def _plan_of(entry, plan, i, ref, e, with_screens, particles: bool):
    """The `_LatticePlan` of a cache entry, made or refreshed for this epoch; None = decline: no stretch, an energy or a stretch the
    table does not take, or an upload while a stream is being captured (not part of a recording: the walk is capturable as it is)."""
    if entry is False or e.dtype != ref.dtype or e.device != ref.device or (e.dim() != 0 and not e.is_contiguous()):
        return None
    lp = entry[1]
    if lp is None or lp.epoch != Element._epoch:
        if torch.cuda.is_current_stream_capturing():
            return None
        if lp is None:
            lp = entry[1] = _LatticePlan(plan[i:entry[0]], ref.dtype, ref.device, allow_vector=True, allow_screens=with_screens)
        else:
            lp.refresh()
    # a histogram screen's bin edges sit in the table as arrays formed from its pixel size: an in-place edit of that tensor moves no
    # epoch — re-derive the stretch (the cloud-in-cell extent is derived on the device and follows by itself). Particles only: the
    # moments' screens get their `gauss_geom` with every call and have no edge arrays
    if particles and lp.edge_keys and any(ps._version != version for _, ps, version in lp.edge_keys):
        if torch.cuda.is_current_stream_capturing():
            return None
        lp.patch = None
        lp.refresh()
    if not lp.ok or (lp.apertures and not particles):        # (an aperture only warns for a ParameterBeam: the walk does that)
        return None
    if segment._CHECK_PLANS:
        lp.verify()
    return lp


def _carries_graph(lp, sp, *beam) -> bool:
    """Does anything the stretch reads carry a graph: the beam's tensors, its energy, the species, a setting in the table? (Asked
    where gradients are enabled.)"""
    return segment._any_requires_grad(*beam, sp.mass_eV, sp.num_elementary_charges, *lp.tensors)


def _on_device(s, ref) -> bool:
    """Is the path length one value the launch can read and write: a scalar of the beam's dtype on its device, no graph?"""
    return s.dim() == 0 and s.dtype == ref.dtype and s.device == ref.device and not s.requires_grad


def _flags(lp, energy_rows: bool) -> int:
    return lp.small_runs | (2 if energy_rows else 0) | (4 if lp.e_out_rows else 0)


def _map_rows(lp, lead: tuple, e, energy_rows: bool):
    """Rows of maps the preparation launch forms for outgoing batch shape `lead` (1: one lattice setting and one energy for every
    beam), None = decline. Settings vectorised over a scan of the lattice and / or a scan of beam energies: row b of the outgoing
    beams = the beam (ONE shared beam, or its own row b) through row b of the settings at energy b."""
    if lp.vshape is None and not energy_rows:
        return 1
    if (lp.vshape is not None and tuple(lp.vshape) != lead) or (energy_rows and tuple(e.shape) != lead):
        return None
    Bm = _ops.numel(lead)
    # (a workgroup per (item, row) prepares a stretch with runs of more than 64 elements: beyond a few hundred rows the walk; a
    # plan's state holds one row from the start)
    if Bm > 1 and ((not lp.small_runs and Bm > segment.Segment._STRETCH_MAX_ROWS) or not lp.ensure_rows(Bm)):
        return None
    return Bm


def _bpm_buffers(lp, ref, B: int, N=None) -> tuple:
    """(n_bpm, readings, ws, ws_bytes) of the stretch's active BPMs; `N` particles: with the workspace of the weighted sums."""
    n_bpm = len(lp.bpms)
    if not n_bpm:
        return 0, None, None, 0
    readings = torch.empty((n_bpm, B, 2), dtype=ref.dtype, device=ref.device)
    ws_bytes = 0 if N is None else _lib.lib().chx_lattice_diag_workspace_bytes(N, B, n_bpm)
    return n_bpm, readings, None if N is None else _ops.workspace(ws_bytes, ref.device), ws_bytes


def _lead_at(lead_in, acc, energy_shape) -> tuple:
    """Batch shape of a beam at a point of a stretch: what it came in with, spread over the vectorised settings in front of
    that point (`acc`) and over the beam energies once a map was applied."""
    # (plain tuples, right-aligned: `torch.broadcast_shapes` costs ~6 us a call, and a lattice has a monitor per cell)
    out = tuple(lead_in)
    for other in (acc, tuple(energy_shape)):
        if not other or other == out:
            continue
        a, b = ((1,) * (len(other) - len(out)) + out, tuple(other)) if len(other) > len(out) else (out, (1,) * (len(out) - len(other)) + tuple(other))
        out = tuple(x if y == 1 else y for x, y in zip(a, b))
    return out


def _narrow(t, here: tuple, lead: tuple, tail: tuple = ()):
    """`t` of batch shape `lead` as the walk has it where the beam has batch shape `here` only: equal rows beyond that."""
    return t if here == lead else _narrow_to(t, (*here, *tail))


def _store_readings(lp, readings, lead: tuple, lead_in: tuple, e, energy_rows: bool) -> None:
    """Every monitor's reading, in the shape the walk's has: the beam AT the monitor is spread over the settings in front of it only
    (and over the energies once a map was applied) — (2,) in front of the scan, (8, 1, 2) behind the first axis of a grid scan."""
    same = lead_in == lead         # (nothing to narrow: the usual case, no shape arithmetic per monitor)
    for k, bpm in enumerate(lp.bpms):
        r = readings[k].reshape(*lead, 2)
        if not same and lp.bpm_acc[k] != lead:
            r = _narrow(r, _lead_at(lead_in, lp.bpm_acc[k], e.shape if (energy_rows and lp.bpm_after[k]) else ()), lead, (2,))
        bpm.__dict__["_buffers"]["reading"] = r


def _narrow_e_out(lp, e_out, e, lead: tuple, energy_rows: bool):
    # (only some axes of a grid scan reach the cavities' voltages and phases)
    return _narrow(e_out, _lead_at(e.shape, lp.e_acc, ()), lead) if (lp.e_out_rows and not energy_rows) else e_out


def _s_out_host(seg, lp, s_in):
    """The path length behind the stretch summed on the host's side, for an `s` the launch does not take (`_on_device`)."""
    s_out = s_in
    for kind, item in lp.items[:lp.count]:
        if kind == "run" or item._is_cavity:           # (monitors, apertures and screens have no length)
            s_out = s_out + (seg._run_length(item) if kind == "run" else item.length)
    return s_out


# ---- a ParticleBeam --------------------------------------------------------------------------------------------------------------------
def track_particles(seg, plan, i: int, incoming: ParticleBeam, allow_screens: bool = True):
    """plan[i] and the items behind it as ONE `chx_lattice_track` call when they form a stretch (at least two items, at least one
    of them no run) of settings the table takes and the beam carries no graph: (outgoing beam, index behind the stretch), else None."""
    p, e, sp, s_in = incoming.particles, incoming.energy, incoming.species, incoming.s
    # one energy: active Screens are items of the stretch too (their record and image come from the same two launches) — for one
    # plain beam and for a vectorised one (B beams under the one lattice setting: every record and image holds B of them). Where the
    # screens' host step does not apply after all, the stretch is taken again with `allow_screens` False and ends at the first screen
    with_screens = allow_screens and segment.Segment._STRETCH_SCREENS and p.dim() >= 2 and e.dim() == 0
    entry = _entry(seg, plan, i, (i, p.dtype, p.device, with_screens), worth=p.is_cuda)
    if p.dim() < 2 or not p.is_cuda or (p.dim() > 2 and not p.is_contiguous()):
        return None                    # (B beams in one ParticleBeam: blockIdx.y of the particle pass)
    energy_rows = e.dim() != 0          # a scan of beam energies: row b of the maps is built for energy b
    lp = _plan_of(entry, plan, i, p, e, with_screens, particles=True)
    if lp is None:
        return None
    # gradients: [run of scalar settings | one active Screen] on a beam without a graph is ONE differentiable node
    # (cheetah_amd._chxtorch RunScreenTrack, `grad_run`); anything else takes the general differentiable path
    grad_run = _grad_run(lp, incoming) if (torch.is_grad_enabled() and _carries_graph(lp, sp, p, e)) else False
    if grad_run is None:
        return None
    x = p if p.is_contiguous() and p.data_ptr() % 16 == 0 else _ops.aligned(p)
    _ops.check_current_device(lp.device)
    if lp.bpms or lp.screens:
        from .. import sharding

        if sharding.active_group() is not None:    # (a particle-sharded beam: the monitors read GLOBAL means, a screen sums its image over the ranks)
            return None
    lead_x = lead = tuple(p.shape[:-2])
    if lp.vshape is not None or energy_rows:
        try:
            lead = tuple(torch.broadcast_shapes(lead_x, lp.vshape if lp.vshape is not None else (), e.shape))
        except RuntimeError:
            return None
        if _ops.numel(lead_x) != 1 and lead_x != lead:
            return None
    Bm = _map_rows(lp, lead, e, energy_rows)
    B = _ops.numel(lead)
    if Bm is None or B < 1 or B > 65535:
        return None
    if lp.expanded:
        seg._refresh_expanded(lp.expanded)
    s_dev = s_in if _on_device(s_in, p) else None
    if lp.screens:
        return _particles_screens(seg, plan, i, incoming, lp, p, e, sp, x, lead, B, Bm, s_dev, grad_run)
    if lp.bpms or lp.apertures or lead:
        got = _particles_diag(lp, p, e, sp, incoming.survival_probabilities, x, lead, lead_x, B, Bm, s_dev, energy_rows)
        if got is None:
            return None
        out, e_out, s_out, w_out = got
    else:
        w_out = incoming.survival_probabilities
        out, e_out, s_out = segment._HOST.lattice_track(lp.capsule, x, x.shape[0], e, s_dev, sp.mass_eV_float,
                                                        sp.num_elementary_charges_float, lp.device.index)
    if s_out is None:
        s_out = _s_out_host(seg, lp, s_in)
    return ParticleBeam(out, e_out, particle_charges=incoming.particle_charges, survival_probabilities=w_out, s=s_out,
                        species=sp), i + lp.count


def _particles_screens(seg, plan, i, incoming, lp, p, e, sp, x, lead, B, Bm, s_dev, grad_run):
    """[run | cavity | monitor | aperture | active Screen]+ on one plain beam: the C++ host step (cheetah_amd._chxtorch) allocates the
    outgoing beam, every screen's record and image and enqueues the two launches."""
    q, w, N = incoming.particle_charges, incoming.survival_probabilities, p.shape[-2]
    if Bm != 1 or s_dev is None or q.shape != (N,) or (w.shape != (N,) and tuple(w.shape) != lead + (N,)) or q.dtype != p.dtype \
            or w.dtype != p.dtype or q.device != p.device or w.device != p.device or not q.is_contiguous() or not w.is_contiguous() \
            or (torch.is_grad_enabled() and (q.requires_grad or w.requires_grad)) or (lead and grad_run) \
            or (lead and any(scr.method != "cloud-in-cell" for scr in lp.screens)):      # (screen.py:292-294: the others refuse vectorised beams)
        # (settings, charges or weights the screens' host step does not take: the stretch without its screens)
        return seg._lattice_stretch(plan, i, incoming, allow_screens=False)
    if grad_run:
        return _run_screen_grad(seg, incoming, lp, x, *grad_run), i + lp.count
    for ap in lp.apertures:
        ap._check_limits()
    n_bpm, readings, ws, ws_bytes = _bpm_buffers(lp, p, B, N)
    w_out = torch.empty(lead + (N,), dtype=p.dtype, device=p.device) if lp.apertures else None
    # (a vectorised beam goes in as (B, N, 7): the beams of a (2, 3, N, 7) array one behind the other)
    out, e_out, s_out, records, images = segment._TORCH_HOST.lattice_track_screens(
        lp.capsule_s, x.reshape(B, N, 7) if lead else x, e, s_dev, q, w, sp.mass_eV_float, sp.num_elementary_charges_float,
        lp.device.index, Screen._EAGER_IMAGE_PARTICLES, w_out, n_bpm, readings, ws, ws_bytes)
    _store_readings(lp, readings, lead, lead, e, False)
    for screen, record, image in zip(lp.screens, records, images):
        if lead and image is not None:
            image = image.reshape(lead + tuple(image.shape[-2:]))
        screen._record_stretch(record, N, sp, image, lead=lead)
    return ParticleBeam(out.reshape(p.shape) if lead else out, e_out, particle_charges=q,
                        survival_probabilities=w if w_out is None else w_out, s=s_out, species=sp), i + lp.count


def _grad_run(lp, incoming: ParticleBeam):
    """(run, its differentiable plan) when the stretch `lp` is [run of scalar settings | one active Screen] and the only
    things that carry a graph are settings of the run (a beam, an energy, a species or a screen geometry with a graph: None)."""
    p, e, sp = incoming.particles, incoming.energy, incoming.species
    if p.requires_grad or e.requires_grad or sp.mass_eV.requires_grad or sp.num_elementary_charges.requires_grad:
        return None
    if lp.count != 2 or len(lp.screens) != 1 or lp.bpms or lp.apertures or lp.vshape is not None or lp.items[0][0] != "run" \
            or lp.items[1][1] is not lp.screens[0] or p.dim() != 2 or e.dim() != 0:
        return None
    b = lp.screens[0].__dict__["_buffers"]
    if b["misalignment"].requires_grad or b["pixel_size"].requires_grad:
        return None
    run = lp.items[0][1]
    fr = run.gfast
    if fr is None or fr.dtype != p.dtype or fr.device != p.device:
        fr = run.gfast = _FastRun(run, p.dtype, p.device, allow_grad=True)
    elif fr.epoch != Element._epoch:
        fr.refresh()
    if not fr.ok or fr.grad_meta is None or fr.E != lp.shape[1]:
        return None
    if segment._CHECK_PLANS:
        fr.verify()
    return run, fr


def _run_screen_grad(seg, incoming, lp, x, run, fr) -> ParticleBeam:
    """[run | Screen] with trainable settings in the run: one differentiable node that leaves the screen's record as well."""
    p, e, s_in, sp = incoming.particles, incoming.energy, incoming.s, incoming.species
    q, w, N = incoming.particle_charges, incoming.survival_probabilities, p.shape[-2]
    out, rows, C, q_at, w_at, e_at, s_at, sums, maps = segment._TORCH_HOST.run_screen_track(
        lp.capsule_s, x, e, s_in, q, w, fr.distinct, fr.grad_meta, sp.mass_eV_float, sp.num_elementary_charges_float)
    x1, origin = x.reshape(1, N, 7), _ops._origin(p)
    # the recorded survival probabilities are the incoming ones (no aperture in a [run | Screen] stretch): tagged as
    # their copy, so that the incoming beam's memoised moments are found again on the next step of a loop; the one-pass
    # sums of the recorded rows ride on the rows (a beam property of them: one small launch, _ops.moment_entry)
    _ops.mark_copy_of(w_at, w)
    rows._chx_partials = (sums, rows._version, w_at,
                          (C, e, fr.distinct, fr.grad_meta, sp.mass_eV_float, sp.num_elementary_charges_float, maps))
    out._chx_lin = _ops._LinearSource(origin, x1, C, (), out._version)
    lp.screens[0]._record_stretch((rows, q_at, w_at, e_at, s_at, x1, C, origin), N, sp, None, "particles_grad")
    return ParticleBeam(out, e, particle_charges=q, survival_probabilities=w, s=seg._run_s(run, s_in), species=sp)


def _particles_diag(lp, p, e, sp, w_in, x, lead, lead_x, B, Bm, s_dev, energy_rows):
    """Active BPMs / apertures in the stretch, or rows of settings / beams (chx_lattice_track_diag): the particle pass leaves the
    weighted sums of x and y at every monitor (one more launch forms all readings) and thins the survival probabilities at every
    aperture — three launches for the lattice instead of six per monitor and a stop per aperture. (out, e_out, s_out, w_out) or None."""
    N, w_out, w, Bw = p.shape[-2], w_in, None, B
    if lp.bpms or lp.apertures:
        w = w_out
        if w.dtype != p.dtype or w.device != p.device or (torch.is_grad_enabled() and w.requires_grad) \
                or w.shape[-1] != N or w.dim() > len(lead) + 1:
            return None
        if w.numel() == N and B > 1:
            w, Bw = w.reshape(N), 1             # one row of weights for all beams: read as it is, not spread over the rows
        elif tuple(w.shape) != lead + (N,):
            try:
                w = w.expand(*lead, N)
            except RuntimeError:
                return None
        if not w.is_contiguous():
            w = w.contiguous()
    for ap in lp.apertures:
        ap._check_limits()           # (aperture.py:72-73; a host read once per value of the two limits)
    n_bpm, readings, ws, ws_bytes = _bpm_buffers(lp, p, B, N)
    if lp.apertures:
        w_out = torch.empty((*lead, N), dtype=p.dtype, device=p.device)
    out = None if lead == lead_x else torch.empty((*lead, N, 7), dtype=p.dtype, device=p.device)
    out, e_out, s_out = segment._HOST.lattice_track(
        lp.capsule, x, N, e, s_dev, sp.mass_eV_float, sp.num_elementary_charges_float, lp.device.index, w,
        w_out if lp.apertures else None, n_bpm, readings, ws, ws_bytes, B, _ops.numel(lead_x), Bm, Bw, _flags(lp, energy_rows), out,
        torch.empty(lead, dtype=p.dtype, device=p.device) if (lp.e_out_rows and not energy_rows) else None)
    e_out = _narrow_e_out(lp, e_out, e, lead, energy_rows)
    _store_readings(lp, readings, lead, lead_x, e, energy_rows)
    if lp.apertures and lead != lead_x:
        # (the beam at the LAST aperture is not spread over the whole scan yet)
        here = _lead_at(torch.broadcast_shapes(lead_x, w_in.shape[:-1]), lp.ap_acc[-1], e.shape if (energy_rows and lp.ap_after[-1]) else ())
        w_out = _narrow(w_out, here, lead, (N,))
    return out, e_out, s_out, w_out


# ---- a ParameterBeam -------------------------------------------------------------------------------------------------------------------
def track_parameter(seg, plan, i: int, incoming: ParameterBeam):
    """The stretch of `track_particles` for a ParameterBeam (`chx_parameter_lattice_track`: the same preparation launch, then one
    wavefront per batch row walks the items): (outgoing beam, index behind the stretch) or None. The walk item by item costs
    ~80-160 us of host time per cavity / monitor cell for 49 numbers of beam state."""
    mu, cov, e = incoming.mu, incoming.cov, incoming.energy
    if not mu.is_cuda or cov.dtype != mu.dtype or cov.device != mu.device:
        return None
    with_screens = segment.Segment._STRETCH_SCREENS and mu.dim() == 1 and cov.dim() == 2 and e.dim() == 0       # (one beam: active Screens are items of the stretch)
    entry = _entry(seg, plan, i, (i, mu.dtype, mu.device, "moments", with_screens))
    energy_rows = e.dim() != 0          # a scan of beam energies: row b of the maps is built for energy b
    lp = _plan_of(entry, plan, i, mu, e, with_screens, particles=False)
    if lp is None:
        return None
    s_in, sp = incoming.s, incoming.species
    if torch.is_grad_enabled() and _carries_graph(lp, sp, mu, cov, e):
        return None
    s_dev = s_in if _on_device(s_in, mu) else None
    if lp.screens:
        return _parameter_screens(i, incoming, lp, s_dev)
    try:        # (one beam under scalar settings at one energy, the usual case: no shape arithmetic — `torch.broadcast_shapes` costs ~6 us)
        in_lead = tuple(torch.broadcast_shapes(mu.shape[:-1], cov.shape[:-2])) if (mu.dim() > 1 or cov.dim() > 2) else ()
        lead = in_lead if (lp.vshape is None and not energy_rows) else \
            tuple(torch.broadcast_shapes(in_lead, lp.vshape if lp.vshape is not None else (), e.shape))
    except RuntimeError:
        return None
    Bm = _map_rows(lp, lead, e, energy_rows)
    if Bm is None:
        return None
    if lp.expanded:
        seg._refresh_expanded(lp.expanded)
    B = _ops.numel(lead)
    m2 = mu.reshape(-1, 7) if mu.is_contiguous() else mu.reshape(-1, 7).contiguous()
    c2 = cov.reshape(-1, 49) if cov.is_contiguous() else cov.reshape(-1, 49).contiguous()
    if m2.shape[0] not in (1, B) or c2.shape[0] not in (1, B):
        return None
    _ops.check_current_device(lp.device)
    mu_out = torch.empty((*lead, 7), dtype=mu.dtype, device=mu.device)
    cov_out = torch.empty((*lead, 7, 7), dtype=mu.dtype, device=mu.device)
    e_out = torch.empty(lead, dtype=e.dtype, device=e.device) if (lp.e_out_rows and not energy_rows) else torch.empty_like(e)
    s_out = None if s_dev is None else torch.empty_like(s_in)
    n_bpm, readings, _, _ = _bpm_buffers(lp, mu, B)
    _ops.check(_lib.lib().chx_parameter_lattice_track(
        lp.table.data_ptr(), *lp.shape, e.data_ptr(), sp.mass_eV_float, sp.num_elementary_charges_float, lp.code,
        lp.state.data_ptr(), lp.state.numel() * 8, m2.data_ptr(), c2.data_ptr(), B, m2.shape[0], c2.shape[0], Bm,
        _flags(lp, energy_rows), mu_out.data_ptr(), cov_out.data_ptr(), e_out.data_ptr(),
        None if s_dev is None else s_in.data_ptr(), None if s_dev is None else s_out.data_ptr(),
        n_bpm, readings.data_ptr() if n_bpm else None, _ops.stream_ptr()), "chx_parameter_lattice_track")
    e_out = _narrow_e_out(lp, e_out, e, lead, energy_rows)
    _store_readings(lp, readings, lead, in_lead, e, energy_rows)
    if s_out is None:
        s_out = _s_out_host(seg, lp, s_in)
    return ParameterBeam(mu_out, cov_out, e_out, total_charge=incoming.total_charge, s=s_out, species=sp), i + lp.count


def _parameter_screens(i, incoming, lp, s_dev):
    """One ParameterBeam through [run | cavity | monitor | active Screen]+: the C++ host step allocates the outgoing moments, every
    screen's record and its image (the bivariate normal density, screen.py:255-291) and enqueues the launches."""
    mu, cov, e, sp, q = incoming.mu, incoming.cov, incoming.energy, incoming.species, incoming.total_charge
    if s_dev is None or not mu.is_contiguous() or not cov.is_contiguous() or q.dim() != 0 or q.dtype != mu.dtype \
            or q.device != mu.device or (torch.is_grad_enabled() and q.requires_grad):       # (the energy: `_plan_of`)
        return None
    _ops.check_current_device(lp.device)
    geoms = []
    for screen in lp.screens:
        nx, ny = screen._geometry("sample_counts")
        geoms.append((screen._geometry("gauss_geom"), screen.__dict__["_buffers"]["misalignment"], nx, ny))
    n_bpm, readings, _, _ = _bpm_buffers(lp, mu, 1)
    mu_out, cov_out, e_out, s_out, records, images = segment._TORCH_HOST.parameter_lattice_track_screens(
        lp.capsule_s, mu, cov, e, s_dev, q, sp.mass_eV_float, sp.num_elementary_charges_float, lp.device.index, tuple(geoms),
        n_bpm, readings)
    _store_readings(lp, readings, (), (), e, False)
    for screen, record, image in zip(lp.screens, records, images):
        screen._record_stretch(record, 0, sp, image, "moments")
    return ParameterBeam(mu_out, cov_out, e_out, total_charge=q, s=s_out, species=sp), i + lp.count
