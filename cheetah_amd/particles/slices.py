"""Slice statistics of a ParticleBeam (`ParticleBeam.slice_statistics`): the current profile I(tau) and the moments of every
longitudinal slice — slice emittance, Twiss parameters, centroid and energy spread — from one `chx_slice_moments` call."""
from __future__ import annotations

import numbers

import torch

from .. import _ops
from ..sharding import _ACTIVE_GROUP as _SHARDING_STACK
from ..utils import elementwise_linspace

speed_of_light = 299792458.0


class BeamSlices:
    """The slices of a beam in tau. Shapes are (*batch, S) unless stated.

    - `edges` (*batch, S + 1), `centres`, `widths`: the slice intervals in metres of tau (beam dtype, never differentiated);
    - `charge`: sum of charge x survival probability of the slice's particles (C, float64);
    - `current`: charge x c / width (A, float64); exactly 0 for a slice without charge. A slice of width 0 that holds charge
      has an infinite current;
    - `num_particles_survived`: sum of the survival probabilities (float64);
    - `moments` (*batch, S, 29): the chx_moments vector of every slice (float64: W, W2, mu[6], covariance upper triangle[21]);
    - `beam`: a ParameterBeam of batch shape (*batch, S) with the slices' weighted means and unbiased covariances
      (utils/statistics.py:4-62), the beam's species and `s`, its reference energy broadcast over the slices and the slice
      charge as `total_charge`, so that every beam property is a slice property: `beam.sigma_x`, `beam.emittance_x`,
      `beam.normalized_emittance_x`, `beam.beta_x`, `beam.alpha_x`, `beam.mu_p`, `beam.sigma_p` (slice energy spread), ...

    A slice without weight, or with a single particle of weight, has the NaN statistics `_ops.moments` gives such a set of
    particles (means and covariances NaN, or covariances NaN). Gradients: such a slice contributes nothing as long as its
    cotangent is zero — select the populated slices before applying a function that is NaN on the others (`beam.cov[populated]`
    rather than `beam.emittance_x[populated]`), since torch's backward of e.g. sqrt at a NaN is NaN even for a zero cotangent."""

    def __init__(self, edges: torch.Tensor, moments: torch.Tensor, charge: torch.Tensor, beam) -> None:
        self.edges = edges
        self.centres = 0.5 * (edges[..., :-1] + edges[..., 1:])
        self.widths = edges[..., 1:] - edges[..., :-1]
        self.moments = moments
        self.charge = charge
        # (the factor is 0 where there is no charge: an empty slice of width 0 gets 0, not 0 * inf, and no NaN gradient)
        self.current = charge * torch.where(charge == 0, 0.0, speed_of_light / self.widths.to(torch.float64))
        self.num_particles_survived = moments[..., 0]
        self.beam = beam

    @property
    def num_slices(self) -> int:
        return self.edges.shape[-1] - 1

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(edges={self.edges!r}, charge={self.charge!r}, beam={self.beam!r})"


def _scalar_or_tensor(v, like: torch.Tensor) -> torch.Tensor:
    if isinstance(v, numbers.Real):          # a fill on the device, not a host-to-device copy
        return torch.full((), float(v), dtype=like.dtype, device=like.device)
    return torch.as_tensor(v, device=like.device).to(like.dtype)


def check_slice_arguments(num_slices, tau_range, edges) -> None:
    """The argument errors of `slice_statistics`, raised before any device work."""
    if edges is not None and tau_range is not None:
        raise ValueError("slice_statistics takes either `edges` or `tau_range`, not both")
    if isinstance(num_slices, bool) or not isinstance(num_slices, numbers.Integral) or num_slices < 1:
        raise ValueError(f"num_slices must be an integer >= 1, got {num_slices!r}")
    if edges is not None:
        shape = edges.shape if isinstance(edges, torch.Tensor) else torch.as_tensor(edges).shape
        if len(shape) < 1 or shape[-1] < 2:
            raise ValueError(f"edges must have a last dimension of at least 2 (S + 1 edges of S slices), got shape {tuple(shape)}")
        S = shape[-1] - 1
    else:
        S = int(num_slices)
    if S > _ops.SLICES_MAX:
        raise ValueError(f"at most {_ops.SLICES_MAX} slices are supported, got {S}")
    if tau_range is not None and len(tau_range) != 2:
        raise ValueError("tau_range must be a (lo, hi) pair")


def slice_statistics(beam, num_slices: int = 50, tau_range=None, edges=None) -> BeamSlices:
    check_slice_arguments(num_slices, tau_range, edges)
    if _SHARDING_STACK:
        raise NotImplementedError("slice_statistics of a particle-sharded beam (inside sharding.particle_sharded) is not implemented: "
                                  "merging the slices of all ranks is not supported yet; gather the particles on one rank first")
    p, w, q = beam.particles, beam.survival_probabilities, beam.particle_charges
    _ops.require_device(p)
    with torch.no_grad():
        if edges is not None:
            e = torch.as_tensor(edges, device=p.device).to(p.dtype)
        else:
            if tau_range is None:
                lo, hi = _ops.default_tau_range(p, w)
            else:
                lo, hi = _scalar_or_tensor(tau_range[0], p), _scalar_or_tensor(tau_range[1], p)
                lo, hi = torch.broadcast_tensors(lo, hi)
            e = elementwise_linspace(lo, hi, int(num_slices) + 1)
    e = e.detach()
    mom, charge = _ops.slice_moments(p, w, q, e)
    batch_shape = mom.shape[:-2]
    S = mom.shape[-2]
    e = e.expand(*batch_shape, S + 1) if e.shape[:-1] != batch_shape else e
    from .parameter_beam import ParameterBeam

    energy = beam.energy.unsqueeze(-1)
    energy = energy.expand(*torch.broadcast_shapes(energy.shape, (*batch_shape, S)))
    slice_beam = ParameterBeam._from_moment_vector(mom, p.dtype, energy, total_charge=charge.to(p.dtype), s=beam.s,
                                                   species=beam.species)
    return BeamSlices(e, mom, charge, slice_beam)
