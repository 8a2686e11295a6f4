"""SynchrotronRadiationKick: the incoherent synchrotron radiation of a bending magnet's arc — the classical energy loss and the
quantum excitation that sets the floor of slice energy spread and of emittance growth in a chicane or an arc — applied as one
instantaneous kick per particle. It is what elegant's CSRCSBEND switches on with ISR=1, SYNCH_RAD=1 and what Bmad calls radiation
damping and fluctuations; the coherent part is `CSRKick`'s. Put kicks into a lattice with `Dipole.split_for_radiation` or
`Segment.with_radiation_kicks`.

The kick is one `chx_sr_kick` call (`_ops.sr_kick`), one pass over the particles. With gamma0 = E0 / mc^2 and P0 = beta0 gamma0 of
the reference particle, r_c = Z^2 r_e m_e / m and lambda_c = hbar c / mc^2 of the species, per batch row

    a = (2/3) r_c theta^2 / L,    b = 55 / (24 sqrt 3) r_c lambda_c |theta|^3 / L^2        (both 0 where L = 0 or theta = 0)

and per particle, in float64 whatever the beam dtype,

    g  = gamma0 + delta P0,   pi = sqrt(g^2 - 1)
    g' = g - a P0^2 pi g - sqrt(b P0^3 g^7 / pi^3) xi
    delta' = delta + (g' - g) / P0,   px' = px pi' / pi,   py' = py pi' / pi,   pi' = sqrt(g'^2 - 1)

The a term is the loss (2/3) r_c mc^2 beta^3 gamma^4 L / rho_i^2 at fixed field, 1 / rho_i = (theta / L) P0 / pi; the b term is the
Gaussian approximation of <dE^2> = 55 / (24 sqrt 3) r_c lambda_c (mc^2)^2 gamma^7 L / |rho_i|^3; the photons leave along the
momentum, so px and py shrink with it. x, y and tau keep their bits.

xi is one standard normal per (kick, call, batch row, particle), evaluated inside the kernel from the counter-based generator
Philox4x32-10: key = (`seed`, `stream`), counter = (particle index, flat batch row, call index). The deviate of particle n therefore
does not depend on the number of particles, the launch geometry or the dtype, and a track is bitwise reproducible. The call index is
a one-element int64 device buffer of the element that the kernel reads and `track` advances in place behind the kick: no host
synchronisation, capturable in a device graph (a replay draws the next call's deviates), differentiable with respect to the
particles, the beam energy, `effect_length` and `angle` (the backward pass draws the same deviates again instead of keeping them).
Two kicks with the same seed, the same stream and equal call indices draw identical deviates: give every kick of a lattice its own
stream, as `Segment.with_radiation_kicks` does."""

from __future__ import annotations

import numbers

import torch

from .. import _ops
from ..particles.particle_beam import ParticleBeam
from ..sharding import _ACTIVE_GROUP as _SHARDING_STACK
from ._binned_kick import _as_tensor, check_effect_length
from .element import Element


def check_key_word(value, what: str, owner: str = "SynchrotronRadiationKick") -> int:
    """One 32-bit half of the generator's key as a Python int."""
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or not 0 <= int(value) < 2**32:
        raise ValueError(f"{owner}: {what} must be an integer in 0 ... 2^32 - 1, got {value!r}")
    return int(value)


class SynchrotronRadiationKick(Element):
    """Incoherent synchrotron radiation of an arc of a bend, as one zero-length kick: energy loss and quantum excitation.

    Limits of the model: Gaussian photon statistics (the energy a particle radiates in the arc is drawn from a normal distribution
    with the exact mean and variance, not from the photon-number spectrum: right where a particle emits many photons per kick, and
    without the spectrum's long tail); no path-length change (tau keeps its bits; the bend's own map carries the dispersion of the
    energy the particle arrives with); the reference energy is not lowered (the mean loss shows as a negative mean delta). The
    field is taken constant over `effect_length`.

    :param effect_length: arc length L >= 0 (m) the kick stands for; may carry a batch shape that broadcasts with the beam's.
    :param angle: bend angle theta (rad) of that arc, L / rho; may carry a batch shape.
    :param quantum_excitation: False leaves the fluctuation out: only the mean loss, and nothing is drawn.
    :param seed: first half of the generator's key, an integer in 0 ... 2^32 - 1.
    :param stream: second half of the key, an integer in 0 ... 2^32 - 1: the kick's number within its lattice.
    """

    #: LatticeJSON: read back as the Python values they were written as
    _plain_features = ("quantum_excitation", "seed", "stream")

    def __init__(self, effect_length, angle, quantum_excitation: bool = True, seed: int = 0, stream: int = 0, name=None,
                 sanitize_name=None, metadata=None, device=None, dtype=None):
        owner = "SynchrotronRadiationKick"
        seed, stream = check_key_word(seed, "seed"), check_key_word(stream, "stream")
        effect_length = _as_tensor(effect_length, device, dtype)
        angle = _as_tensor(angle, device, dtype)
        check_effect_length(effect_length, owner)
        if not bool(torch.isfinite(angle.detach()).all()):
            raise ValueError(f"{owner}: angle must be finite (rad), got {angle!r}")
        fk = {"device": device if device is not None else effect_length.device,
              "dtype": dtype if dtype is not None else effect_length.dtype}
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        self.quantum_excitation = bool(quantum_excitation)
        self.seed, self.stream = seed, stream
        self.register_buffer_or_parameter("effect_length", effect_length)
        self.register_buffer_or_parameter("angle", angle)
        # how many excited kicks this element has applied: the upper half of the generator's counter. Not persistent: a saved
        # lattice starts at call 0
        self.register_buffer("_call_index", torch.zeros(1, dtype=torch.int64, device=fk["device"]), persistent=False)

    @property
    def is_skippable(self) -> bool:
        return False

    def first_order_transfer_map(self, energy, species):
        raise NotImplementedError("SynchrotronRadiationKick has no linear transfer map")

    @property
    def call_index(self) -> int:
        """The call index the next track draws with (reads the device back: not for the tracking path)."""
        return int(self._call_index.item())

    def reseed(self, seed=None, call_index: int = 0) -> None:
        """Set the call index (to 0: the sequence of tracks starts again, bit for bit) and, if given, the seed."""
        if isinstance(call_index, bool) or not isinstance(call_index, numbers.Integral) or not 0 <= int(call_index) < 2**63:
            raise ValueError(f"SynchrotronRadiationKick.reseed: call_index must be an integer in 0 ... 2^63 - 1, got {call_index!r}")
        if seed is not None:
            self.seed = check_key_word(seed, "seed")
        self._call_index.fill_(int(call_index))

    def clone(self) -> "SynchrotronRadiationKick":
        c = super().clone()
        c._call_index.copy_(self._call_index)
        return c

    def track(self, incoming: ParticleBeam) -> ParticleBeam:
        if not isinstance(incoming, ParticleBeam):
            raise TypeError(f"SynchrotronRadiationKick tracking needs a ParticleBeam: every particle radiates on its own, which a "
                            f"{type(incoming).__name__} does not carry")
        if _SHARDING_STACK:
            raise NotImplementedError("SynchrotronRadiationKick tracking of a particle-sharded beam (inside "
                                      "sharding.particle_sharded) is not implemented: the deviates are numbered with the LOCAL "
                                      "particle index, so every rank would draw the same ones; gather the particles on one rank first")
        species = incoming.species
        out = _ops.sr_kick(incoming.particles, incoming.energy, species.mass_eV_float, abs(species.num_elementary_charges_float),
                           self.effect_length, self.angle, self.quantum_excitation, self.seed, self.stream, self._call_index)
        if self.quantum_excitation:
            self._call_index.add_(1)
        return ParticleBeam(out, incoming.energy, particle_charges=incoming.particle_charges,
                            survival_probabilities=incoming.survival_probabilities, s=incoming.s, species=species)

    @property
    def defining_features(self) -> list[str]:
        return super().defining_features + ["effect_length", "angle", "quantum_excitation", "seed", "stream"]
