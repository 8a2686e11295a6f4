"""LSCKick: the longitudinal space-charge (LSC) field of a straight section, applied as one instantaneous energy kick that follows the
bunch's current profile. Put kicks into a lattice with `Segment.with_lsc_kicks`.

The kick is one `chx_lsc_kick` call (`_ops.lsc_kick`): per batch row, the surviving particles (survival probability > 0, finite tau)
are deposited with c = |q| w on `num_bins` = M nodes spanning their tau range, exactly as `CSRKick` and `Wakefield` deposit them,
which gives the deposits D_k and the node spacing h. The line density is taken piecewise linear between the nodes,
lambda_k = D_k / h, and the field is the on-axis field of a uniformly charged disc of radius a moving with Lorentz factor gamma,

    E_z(tau) = (2 k_e / a^2) int lambda(tau') g(tau' - tau) dtau',    g(u) = sgn(u) - u / sqrt(u^2 + (a / gamma)^2)

A larger tau is the tail: charge behind a witness pushes it forward, so that witness gains energy. g is integrated exactly against
every hat function. With rho = a / (gamma h), and c^_j = c_j / rho^2 so that the scale stays finite as rho -> 0,

    kick_k = S sum_j c^_j D_(k+j)      (j runs over BOTH signs: -k <= j <= M - 1 - k)
    S      = |Z| 2 k_e L / (gamma^2 h^2 p0c)
    c^_0 = 0,   c^_(-j) = -c^_j,   c^_j = -1/2 [P(j+1) - 2 P(j) + P(j-1)]
    P(v)   = v / (|v| + sqrt(v^2 + rho^2)) + asinh(v / rho)

and every particle gets delta += (1 - f) kick_k + f kick_(k+1) at its node coordinate, evaluated in fp64 and rounded once. P is
the cancellation-free form of the second antiderivative of g (|v| - sqrt(v^2 + rho^2) = -rho^2 / (|v| + sqrt(v^2 + rho^2))); for
large lags c^_j -> 1 / (2 j^2), the Coulomb field with its 1 / gamma^2 suppression. The coefficients are antisymmetric, so the kicks
weighted with the charges sum to zero. Deterministic, no host synchronisation, capturable in a device graph, differentiable with
respect to the particles, charges, survival probabilities, the beam energy, `effect_length` and `beam_radius` (the node grid is a
constant)."""

from __future__ import annotations

import math

import torch

from .. import _ops
from ._binned_kick import BinnedKick, _as_tensor, check_cutoff_wavelength, check_effect_length, check_num_bins


def check_radius_factor(radius_factor, owner: str = "LSCKick") -> float:
    """A finite factor > 0 as a Python float (a LatticeJSON file hands it over as a 0-d tensor)."""
    if isinstance(radius_factor, torch.Tensor) and radius_factor.numel() == 1:
        radius_factor = radius_factor.item()
    if isinstance(radius_factor, bool) or not isinstance(radius_factor, (int, float)) or not math.isfinite(radius_factor) \
            or not radius_factor > 0:
        raise ValueError(f"{owner}: radius_factor must be a finite number > 0, got {radius_factor!r}")
    return float(radius_factor)


def check_beam_radius(beam_radius, owner: str = "LSCKick") -> None:
    r = beam_radius.detach()
    if not bool(torch.isfinite(r).all() & (r > 0).all()):
        raise ValueError(f"{owner}: beam_radius must be finite and > 0 (metres), got {beam_radius!r}")


class LSCKick(BinnedKick):
    """Longitudinal space charge of a straight section, as one zero-length energy kick.

    Limits of the model: 1-D (the on-axis field of a transversely uniform disc for every particle: no transverse forces, no
    dependence on a particle's own offset); the beam's size and energy are taken constant over `effect_length`. Without a
    `cutoff_wavelength` the deposit is used raw: at a fixed number of particles the shot noise of the kick then grows with `num_bins`.
    With one, `num_bins` sets the resolution and the cutoff the noise, and the kick converges as M grows.

    :param effect_length: length L >= 0 (m) of the straight section the kick stands for; may carry a batch shape that broadcasts
        with the beam's.
    :param beam_radius: radius a > 0 (m) of the uniformly charged disc; may carry a batch shape. `None`: the radius is
        `radius_factor * (sigma_x + sigma_y) / 2` of the incoming beam, per batch row, formed on the device (differentiable through
        the beam's moments). A row whose radius is not > 0 or not finite gets NaN in delta: a line charge has no finite on-axis field.
    :param radius_factor: factor of the beam's mean rms size when `beam_radius` is `None`; 1.7 is elegant's convention for a Gaussian
        beam.
    :param num_bins: number of nodes M of the grid in tau, 2 <= M <= 4096.
    :param cutoff_wavelength: `None`, or the cutoff wavelength lambda_c > 0 (m) of the Gaussian low-pass filter of the deposit
        (`BinnedKick`); may carry a batch shape. A constant like `num_bins`: it must not require grad.
    """

    #: LatticeJSON: read back as the Python number it was written as, not as a tensor of the file's dtype
    _plain_features = ("radius_factor",)
    _follows = "the LSC kick"

    def __init__(self, effect_length, beam_radius=None, radius_factor: float = 1.7, num_bins: int = 200, name=None,
                 sanitize_name=None, metadata=None, device=None, dtype=None, *, cutoff_wavelength=None):
        num_bins = check_num_bins(num_bins, "LSCKick")
        radius_factor = check_radius_factor(radius_factor)
        effect_length = _as_tensor(effect_length, device, dtype)
        check_effect_length(effect_length, "LSCKick")
        if beam_radius is not None:
            beam_radius = _as_tensor(beam_radius, device, dtype)
            check_beam_radius(beam_radius)
        fk = {"device": device if device is not None else effect_length.device,
              "dtype": dtype if dtype is not None else effect_length.dtype}
        cutoff_wavelength = check_cutoff_wavelength(cutoff_wavelength, "LSCKick", **fk)
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        self.num_bins = num_bins
        self._register_cutoff(cutoff_wavelength)
        self.radius_factor = radius_factor
        self.register_buffer_or_parameter("effect_length", effect_length)
        self.register_buffer_or_parameter("beam_radius", beam_radius)

    def _kick(self, incoming, species):
        radius = self.beam_radius
        if radius is None:
            _ops.require_device(incoming.particles)
            radius = (self.radius_factor / 2) * (incoming.sigma_x + incoming.sigma_y)
        return _ops.lsc_kick(incoming.particles, incoming.particle_charges, incoming.survival_probabilities, incoming.energy,
                             species.mass_eV_float, abs(species.num_elementary_charges_float), self.effect_length, radius,
                             self.num_bins, self.cutoff_wavelength)

    @property
    def defining_features(self) -> list[str]:
        return self._with_cutoff(super().defining_features + ["effect_length", "beam_radius", "radius_factor", "num_bins"])
