"""LaserModulator: the energy modulation a laser imprints on the beam inside an undulator whose radiation it is resonant with — the
laser heater that damps the microbunching instability (the chicane around its undulator smears the modulation into slice energy
spread) and the modulator of seeded FELs (HGHG, EEHG) and of optical diagnostics — applied as one zero-length kick at the middle
of an undulator piece (Huang et al., PRSTAB 7, 074401 (2004), eq. 8). Put kicks into an undulator with `Undulator.with_laser`;
`laser_modulation_amplitude` gives the amplitude from the laser's peak power.

The kick is one `chx_laser_kick` call (`_ops.laser_kick`), one pass over the particles. With gamma0 = E0 / mc^2 and P0 = beta0 gamma0
of the reference particle, per batch row

    a = A / (P0 mc^2),   nu = 1 / lambda,   phi_t = phi / (2 pi),   g = 1 / (4 sigma_r^2),   h = 1 / (4 sigma_t^2)   (0 without envelope)

and per particle, in float64 whatever the beam dtype, with u = x - x0, v = y - y0, w = tau - tau0,

    t = tau nu + phi_t               (the phase in turns; product and sum rounded separately)
    f = t - rint(t)                  (exact: 10^4 turns along a bunch cost no digits)
    delta' = delta + a exp(-g (u^2 + v^2) - h w^2) sin(2 pi f)

Every other coordinate keeps its bits, and a row with A = 0 keeps all of them. No host synchronisation, bitwise reproducible,
capturable in a device graph (an in-place edit of a setting is followed), differentiable with respect to the particles, the beam
energy and all eight settings."""

from __future__ import annotations

import torch

from .. import _ops
from ..particles.particle_beam import ParticleBeam
from ..particles.species import Species, electron_mass_eV, elementary_charge
from ._binned_kick import _as_tensor
from .element import Element

_SPEED_OF_LIGHT = 299792458.0             # m / s
_ELECTRON_RADIUS = 2.8179403205e-15       # r_e, m (CODATA 2022)
#: P_0 for an electron: (e c / r_e) m_e c^2 / e = 8.710023 GW
_ELECTRON_P0_WATT = elementary_charge * _SPEED_OF_LIGHT / _ELECTRON_RADIUS * electron_mass_eV


def _bessel_jj(xi: torch.Tensor) -> torch.Tensor:
    """[JJ] = J0(xi) - J1(xi) from the power series, for the planar undulator's 0 <= xi < 1/2: ten terms each leave less than 1e-19,
    and plain torch arithmetic is differentiable where `torch.special.bessel_j0` is not."""
    q = (xi / 2).square()
    j0 = torch.ones_like(xi)
    j1 = torch.ones_like(xi)
    t0 = torch.ones_like(xi)
    t1 = torch.ones_like(xi)
    for m in range(1, 11):
        t0 = -t0 * q / (m * m)
        t1 = -t1 * q / (m * (m + 1))
        j0 = j0 + t0
        j1 = j1 + t1
    return j0 - (xi / 2) * j1


def laser_modulation_amplitude(peak_power, undulator_k, undulator_length, laser_sigma, energy, species: Species | None = None):
    """The on-axis energy-modulation amplitude A (eV) of a laser of peak power P_L (W) and rms intensity size sigma_r (m) in a planar
    undulator of strength K and length L_u (m), for a beam of reference energy E0 (eV), the laser waist long against the undulator
    (Huang et al. 2004, eq. 8):

        A = mc^2 sqrt(P_L / P_0) K L_u [JJ] / (gamma0 sigma_r),   [JJ] = J0(xi) - J1(xi),   xi = K^2 / (4 + 2 K^2)

    with P_0 = (e c / r_e) (m_e c^2 / e) (m / m_e)^2 / Z^2, 8.710023 GW for an electron. Plain torch on the arguments' device,
    differentiable in all of them; `species=None` is an electron."""
    args = [t if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=torch.get_default_dtype())
            for t in (peak_power, undulator_k, undulator_length, laser_sigma, energy)]
    P, K, L, sigma, E = args
    if species is None:
        mass, z2 = electron_mass_eV, 1.0
    else:
        mass, z2 = species.mass_eV.to(E.device), species.num_elementary_charges.to(E.device).square()
    p0 = _ELECTRON_P0_WATT * (mass / electron_mass_eV) ** 2 / z2
    xi = K.square() / (4 + 2 * K.square())
    gamma = E / mass
    return mass * torch.sqrt(P / p0) * K * L * _bessel_jj(xi) / (gamma * sigma)


class LaserModulator(Element):
    """Energy modulation by a laser in an undulator, as one zero-length kick: delta' = delta + A / (p0 c) exp(-r^2 / 4 sigma_r^2)
    exp(-(tau - tau0)^2 / 4 sigma_t^2) sin(2 pi tau / lambda + phi).

    Limits of the model: no slippage and no harmonics (the laser is taken resonant with the undulator's fundamental: the
    resonance condition is the user's, `Undulator.resonant_wavelength` gives it); no transverse kick (the Panofsky-Wenzel partner
    of d delta / dx is about lambda / (2 pi sigma_r) of the energy kick, 1e-9 in px, and is left out, so the kick is not exactly
    symplectic); the reference energy is unchanged.

    Every setting may carry a batch shape that broadcasts with the beam's and the energy's.

    :param amplitude: on-axis energy-modulation amplitude A (eV), of either sign; `laser_modulation_amplitude` gives it.
    :param wavelength: laser wavelength lambda (m), > 0.
    :param laser_sigma: rms size sigma_r (m) of the laser INTENSITY, > 0; the field falls as exp(-r^2 / 4 sigma_r^2).
    :param phase: phase phi (rad) of the modulation at tau = 0.
    :param offset_x: horizontal position x0 (m) of the laser axis.
    :param offset_y: vertical position y0 (m) of the laser axis.
    :param pulse_sigma: rms length sigma_t (m) of the intensity envelope along tau, > 0, or None for no envelope.
    :param pulse_center: centre tau0 (m) of the envelope.
    """

    _SETTINGS = ("amplitude", "wavelength", "phase", "laser_sigma", "offset_x", "offset_y", "pulse_sigma", "pulse_center")

    def __init__(self, amplitude, wavelength, laser_sigma, phase=0.0, offset_x=0.0, offset_y=0.0, pulse_sigma=None,
                 pulse_center=0.0, name=None, sanitize_name=None, metadata=None, device=None, dtype=None):
        owner = "LaserModulator"
        given = dict(zip(self._SETTINGS, (amplitude, wavelength, phase, laser_sigma, offset_x, offset_y, pulse_sigma, pulse_center)))
        amplitude = _as_tensor(amplitude, device, dtype)
        fk = {"device": device if device is not None else amplitude.device, "dtype": dtype if dtype is not None else amplitude.dtype}
        values = {k: _as_tensor(v, fk["device"], fk["dtype"]) for k, v in given.items()}
        values["amplitude"] = amplitude
        for k, v in values.items():
            if v is None:
                if k != "pulse_sigma":
                    raise ValueError(f"{owner}: {k} must be given")
                continue
            if not bool(torch.isfinite(v.detach()).all()):
                raise ValueError(f"{owner}: {k} must be finite, got {v!r}")
            if k in ("wavelength", "laser_sigma", "pulse_sigma") and not bool((v.detach() > 0).all()):
                raise ValueError(f"{owner}: {k} must be > 0 (metres){' or None' if k == 'pulse_sigma' else ''}, got {v!r}")
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        for k, v in values.items():
            if v is None:
                self.pulse_sigma = None
            else:
                self.register_buffer_or_parameter(k, v)

    @property
    def is_skippable(self) -> bool:
        return False

    def first_order_transfer_map(self, energy, species):
        raise NotImplementedError("LaserModulator has no linear transfer map")

    def track(self, incoming: ParticleBeam) -> ParticleBeam:
        if not isinstance(incoming, ParticleBeam):
            raise TypeError(f"LaserModulator tracking needs a ParticleBeam: the modulation follows every particle's own x, y and tau "
                            f"at the optical wavelength, which a {type(incoming).__name__} does not carry")
        species = incoming.species
        out = _ops.laser_kick(incoming.particles, incoming.energy, species.mass_eV_float, self.amplitude, self.wavelength, self.phase,
                              self.laser_sigma, self.offset_x, self.offset_y, self.pulse_sigma, self.pulse_center)
        return ParticleBeam(out, incoming.energy, particle_charges=incoming.particle_charges,
                            survival_probabilities=incoming.survival_probabilities, s=incoming.s, species=species)

    @property
    def defining_features(self) -> list[str]:
        return super().defining_features + list(self._SETTINGS)
