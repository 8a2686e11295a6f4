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


def check_cutoff_wavelength(cutoff_wavelength, owner: str, device=None, dtype=None):
    """None (no filter), or the cutoff wavelength as a tensor on `device` in `dtype` (a tensor that is there already stays itself):
    finite and > 0 (metres), and not part of a graph."""
    if cutoff_wavelength is None:
        return None
    if isinstance(cutoff_wavelength, torch.Tensor) and cutoff_wavelength.requires_grad:
        raise ValueError(f"{owner}: cutoff_wavelength must not require grad: it is a constant of the kick like num_bins (it sets the "
                         "filter's width in nodes and its weights), so no gradient flows to it; pass a detached tensor")
    if not isinstance(cutoff_wavelength, torch.Tensor) and dtype is None:
        dtype = torch.get_default_dtype()
    cutoff_wavelength = torch.as_tensor(cutoff_wavelength, device=device, dtype=dtype)
    if not bool(torch.isfinite(cutoff_wavelength).all() & (cutoff_wavelength > 0).all()):
        raise ValueError(f"{owner}: cutoff_wavelength must be finite and > 0 (metres) or None, got {cutoff_wavelength!r}")
    return cutoff_wavelength


class BinnedKick(Element):
    """A zero-length kick computed from the binned beam. A subclass gives `_follows` (what follows the current profile, for the
    messages) and `_kick(incoming, species) -> particles`; it hands `cutoff_wavelength` (checked with `check_cutoff_wavelength`) to
    `_register_cutoff` and lists its features through `_with_cutoff`.

    `cutoff_wavelength`: `None` (the raw deposit), or the cutoff lambda_c > 0 (m) of a Gaussian low-pass filter of the deposit; may
    carry a batch shape. Per batch row, with h the node spacing, every deposited channel is smoothed before the node pass:

        s = lambda_c / (2 pi h),   R = max(1, min(ceil(4 s), M - 1)),   g_d = exp(-d^2 / 2 s^2) / sum_{|e| <= R} g_e,
        D'_j = sum_{|d| <= R} g_d D_refl(j - d),   refl(i) = -1 - i for i < 0, 2 M - 1 - i for i >= M

    (the row mirrored about its ends, numpy's pad(mode="symmetric")). The amplitude response is exp(-(lambda_c / lambda)^2 / 2); the
    charge is kept and no weight is negative. With a cutoff the kick no longer depends on `num_bins` once h << lambda_c: M sets
    the resolution, lambda_c the noise. A constant of the kick like `num_bins` (no gradient flows to it); a buffer, so an in-place
    edit is followed by the next track, also by a captured one."""

    _follows: str

    def _register_cutoff(self, cutoff_wavelength) -> None:
        self.register_buffer("cutoff_wavelength", cutoff_wavelength)

    def _with_cutoff(self, features: list[str]) -> list[str]:
        """`features` with `cutoff_wavelength` behind `num_bins` if the element has a cutoff."""
        if self.cutoff_wavelength is None:
            return features
        i = features.index("num_bins") + 1
        return features[:i] + ["cutoff_wavelength"] + features[i:]

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
