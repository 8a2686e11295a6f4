"""Wakefield: the short-range wake of a structure (accelerating cavity, collimator, any impedance given as a tabulated point-charge
wake), applied as one instantaneous kick — the longitudinal wake as an energy change that follows the current profile, the
transverse dipole wake as a kick towards the offset of the charge ahead.

The kick is one `chx_wake_kick` call (`_ops.wake_kick`): per batch row, the surviving particles (survival probability > 0, finite
tau) are deposited on `num_bins` nodes spanning their tau range, the deposits are convolved causally with the wake sampled at the
node spacing (the self term at s = 0 halved: beam loading), and the result is interpolated back to every particle:

    delta += factor |Z| V(tau) / p0c,    px += factor |Z| Ux(tau) / p0c,    py += factor |Z| Uy(tau) / p0c

A larger tau is later in time (the tail). Deterministic, no host synchronisation, capturable in a device graph, differentiable with
respect to the particles, charges, survival probabilities, the beam energy, `factor` and both tables (the node grid and
`wake_spacing` are constants)."""

from __future__ import annotations

import torch

from .. import _ops
from ._binned_kick import BinnedKick, _as_tensor, check_cutoff_wavelength, check_num_bins


class Wakefield(BinnedKick):
    """Short-range wakefield of a structure as one zero-length kick.

    :param wake_spacing: scalar tensor h > 0 (m): entry n of a table is the wake at s = n h behind the source.
    :param longitudinal_wake: 1-D tensor, point-charge wake W_par(s) in V/C; positive = the witness loses energy.
    :param transverse_wake: 1-D tensor, dipole wake W_perp(s) in V/(C m); positive = the witness is kicked towards the source's
        offset. At least one of the two tables is required; an absent one is stored as an empty (0,) tensor.
    :param factor: scaling of the wake (structure length, number of cells), default 1; may carry a batch shape that broadcasts
        with the beam's.
    :param num_bins: number of nodes M of the grid in tau, 2 <= M <= 4096.
    :param cutoff_wavelength: `None`, or the cutoff wavelength lambda_c > 0 (m) of the Gaussian low-pass filter of the deposits Q, X, Y
        (`BinnedKick`); may carry a batch shape. A constant like `num_bins`: it must not require grad.
    """

    _follows = "the wake"

    def __init__(self, wake_spacing, longitudinal_wake=None, transverse_wake=None, factor=None, num_bins: int = 200, name=None,
                 sanitize_name=None, metadata=None, device=None, dtype=None, *, cutoff_wavelength=None):
        num_bins = check_num_bins(num_bins, "Wakefield")
        longitudinal_wake = _as_tensor(longitudinal_wake, device, dtype)
        transverse_wake = _as_tensor(transverse_wake, device, dtype)
        for label, table in (("longitudinal_wake", longitudinal_wake), ("transverse_wake", transverse_wake)):
            if table is not None and table.dim() != 1:
                raise ValueError(f"Wakefield: {label} must be a 1-D table, got shape {tuple(table.shape)}")
        present = [t for t in (longitudinal_wake, transverse_wake) if t is not None and t.numel() > 0]
        if not present:
            raise ValueError("Wakefield: give a longitudinal_wake or a transverse_wake table (or both)")
        # defaults live where the tables live unless the factory arguments say otherwise
        fk = {"device": device if device is not None else present[0].device,
              "dtype": dtype if dtype is not None else present[0].dtype}
        wake_spacing = _as_tensor(wake_spacing, fk["device"], fk["dtype"])
        if wake_spacing is None or wake_spacing.dim() != 0 or not bool(torch.isfinite(wake_spacing.detach()) & (wake_spacing.detach() > 0)):
            raise ValueError(f"Wakefield: wake_spacing must be a positive scalar (metres), got {wake_spacing!r}")
        cutoff_wavelength = check_cutoff_wavelength(cutoff_wavelength, "Wakefield", **fk)
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        self._register_cutoff(cutoff_wavelength)
        empty = lambda t: t if t is not None and t.numel() > 0 else torch.zeros(0, **fk)  # noqa: E731
        self.num_bins = num_bins
        self.register_buffer_or_parameter("wake_spacing", wake_spacing)
        self.register_buffer_or_parameter("longitudinal_wake", empty(longitudinal_wake))
        self.register_buffer_or_parameter("transverse_wake", empty(transverse_wake))
        self.register_buffer_or_parameter("factor", _as_tensor(factor, fk["device"], fk["dtype"]) if factor is not None
                                          else torch.ones((), **fk))

    def _kick(self, incoming, species):
        wl, wt = self.longitudinal_wake, self.transverse_wake
        return _ops.wake_kick(incoming.particles, incoming.particle_charges, incoming.survival_probabilities, incoming.energy,
                              species.mass_eV_float, abs(species.num_elementary_charges_float), self.factor,
                              wl if wl.numel() > 0 else None, wt if wt.numel() > 0 else None, self.wake_spacing, self.num_bins,
                              self.cutoff_wavelength)

    @property
    def defining_features(self) -> list[str]:
        return self._with_cutoff(super().defining_features
                                 + ["wake_spacing", "longitudinal_wake", "transverse_wake", "factor", "num_bins"])
