"""BinnedKick: the base of the elements whose kick follows the beam's current profile, binned on `num_bins` nodes in tau (`Wakefield`,
`CSRKick`, `TransientCSRKick`, `CSRDriftKick`, `LSCKick`, `IBSKick`), and the argument checks they share with the methods that put such kicks into a lattice."""

from __future__ import annotations

import numbers

import torch

from .. import _ops
from ..particles.particle_beam import ParticleBeam
from ..sharding import _ACTIVE_GROUP as _SHARDING_STACK
from .element import Element


def _as_tensor(v, device, dtype):
    if v is None or isinstance(v, torch.Tensor):
        return v
    return torch.as_tensor(v, device=device, dtype=dtype if dtype is not None else torch.get_default_dtype())


def check_num_bins(num_bins, owner: str) -> int:
    if isinstance(num_bins, bool) or not isinstance(num_bins, numbers.Integral) or not 2 <= int(num_bins) <= _ops.WAKE_MAX_BINS:
        raise ValueError(f"{owner}: num_bins must be an integer in 2 ... {_ops.WAKE_MAX_BINS}, got {num_bins!r}")
    return int(num_bins)


def check_num_kicks(num_kicks, owner: str) -> int:
    if isinstance(num_kicks, bool) or not isinstance(num_kicks, numbers.Integral) or int(num_kicks) < 1:
        raise ValueError(f"{owner}: num_kicks must be an integer >= 1, got {num_kicks!r}")
    return int(num_kicks)


def check_effect_length(effect_length, owner: str) -> None:
    if not bool(torch.isfinite(effect_length.detach()).all() & (effect_length.detach() >= 0).all()):
        raise ValueError(f"{owner}: effect_length must be finite and >= 0 (metres), got {effect_length!r}")


class BinnedKick(Element):
    """A zero-length kick computed from the binned beam. A subclass gives `_follows` (what follows the current profile, for the
    messages) and `_kick(incoming, species) -> particles`."""

    _follows: str

    @property
    def is_skippable(self) -> bool:
        return False

    def first_order_transfer_map(self, energy, species):
        raise NotImplementedError(f"{type(self).__name__} has no linear transfer map")

    def _kick(self, incoming: ParticleBeam, species) -> torch.Tensor:
        raise NotImplementedError

    def track(self, incoming: ParticleBeam) -> ParticleBeam:
        if not isinstance(incoming, ParticleBeam):
            raise TypeError(f"{type(self).__name__} tracking needs a ParticleBeam: {self._follows} follows the beam's current "
                            f"profile, which a {type(incoming).__name__} does not carry")
        if _SHARDING_STACK:
            raise NotImplementedError(f"{type(self).__name__} tracking of a particle-sharded beam (inside sharding.particle_sharded) is not "
                                      "implemented: the tau range and the deposited grid of all ranks are not merged yet; gather "
                                      "the particles on one rank first")
        species = incoming.species
        out = self._kick(incoming, species)
        return ParticleBeam(out, incoming.energy, particle_charges=incoming.particle_charges,
                            survival_probabilities=incoming.survival_probabilities, s=incoming.s, species=species)
