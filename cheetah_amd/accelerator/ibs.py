"""IBSKick: intrabeam scattering (IBS) — multiple small-angle Coulomb scattering inside the bunch, which raises the slice energy
spread all along a linac, most where the bunch is compressed — applied as one instantaneous kick that follows the bunch's current
profile. It belongs in a microbunching-gain calculation next to the laser heater (Huang, LCLS-TN-02-8; Di Mitri et al., New J. Phys.
22 (2020) 083053). Put kicks into a lattice with `Segment.with_ibs_kicks`.

The rate is Bane's high-energy approximation of the Bjorken-Mtingwa formula (EPAC 2002, "A simplified model of intrabeam
scattering") without dispersion and with beta = 1; Bane's bunch average N / sigma_s is replaced by the local line density,
2 sqrt(pi) n(tau), so that the charge-weighted mean over a Gaussian bunch is Bane's bunch formula. The kick is one `chx_ibs_kick` call
(`_ops.ibs_kick`): per batch row, the surviving particles (survival probability > 0, finite tau) are deposited with c = |q| w on
`num_bins` = M nodes spanning their tau range, exactly as `LSCKick` deposits them, which gives the deposits D_k and the node spacing
h. With gamma = E / mc^2, r_c = Z^2 r_e m_e / m, the rms sizes sigma and the geometric emittances eps, in float64,

    alpha = (sigma_x eps_y) / (sigma_y eps_x),    g(alpha) = sqrt(alpha) / AGM(1, alpha)
    K     = sqrt(pi) r_c^2 Lambda L g(alpha) / (4 gamma^3 sqrt(eps_x eps_y sigma_x sigma_y) |Z| e)
    V_k   = K D_k / h                                 the variance of delta that node k's density adds over the length L

and every particle gets delta += sqrt((1 - f) V_k + f V_(k+1)) xi at its node coordinate, evaluated in float64 and rounded once. g is
Bane's function (2 sqrt(alpha) / pi) int_0^inf du / sqrt((1 + u^2)(alpha^2 + u^2)) in closed form (the arithmetic-geometric mean,
8 steps), symmetric in alpha <-> 1 / alpha with g(1) = 1. Every other column keeps its bits, and so does delta where the variance is 0
(empty nodes, L = 0, a row without a grid).

xi is one standard normal per (kick, call, batch row, particle), evaluated inside the kernel from the counter-based generator
Philox4x32-10 as `SynchrotronRadiationKick` draws it: key = (`seed`, `stream`), counter = (particle index, flat batch row + 2^31,
call index). Bit 31 of the second counter word keeps an `IBSKick` and a `SynchrotronRadiationKick` with equal seed, stream and call
index from drawing the same numbers. The call index is a one-element int64 device buffer of the element that the kernel reads and
`track` advances in place behind the kick: no host synchronisation, capturable in a device graph (a replay draws the next call's
deviates), bitwise reproducible, differentiable with respect to the particles, charges, survival probabilities, the beam energy,
`effect_length`, `coulomb_log` and the four moments (the node grid and the deviates are constants; the backward pass draws the same
deviates again instead of keeping them). A particle whose variance is 0 has zero gradients through the variance."""

from __future__ import annotations

import numbers

import torch

from .. import _ops
from ._binned_kick import BinnedKick, _as_tensor, check_cutoff_wavelength, check_effect_length, check_num_bins
from .synchrotron_radiation import check_key_word

_MOMENTS = ("sigma_x", "sigma_y", "emittance_x", "emittance_y")


def check_positive(value, what: str, owner: str = "IBSKick") -> None:
    v = value.detach() if isinstance(value, torch.Tensor) else torch.as_tensor(value)
    if not bool(torch.isfinite(v).all() & (v > 0).all()):
        raise ValueError(f"{owner}: {what} must be finite and > 0, got {value!r}")


class IBSKick(BinnedKick):
    """Intrabeam scattering of a section of beamline, as one zero-length kick that adds slice energy spread where the current is.

    Limits of the model: beta = 1 (ultra-relativistic); no dispersion term (the sigma_H of Bane's formula is the dispersion-free
    one), so in a chicane pass the moments explicitly or leave the bends out; Bane's condition sigma_delta sigma_x / (gamma eps_x)
    << 1 (the beam is much colder longitudinally than transversely in its rest frame); only delta is excited, the transverse
    emittance growth is neglected; the moments, the energy and the current profile are taken constant over `effect_length`. Without a
    `cutoff_wavelength` the deposit is used raw, as in `LSCKick`: at a fixed number of particles the shot noise of the variance then
    grows with `num_bins`. The filter's weights are not negative, so a filtered variance is not either.

    :param effect_length: length L >= 0 (m) of the section the kick stands for; may carry a batch shape that broadcasts with the
        beam's.
    :param coulomb_log: Coulomb logarithm Lambda > 0; may carry a batch shape.
    :param sigma_x, sigma_y: rms beam sizes (m) > 0; may carry a batch shape. `None`: the incoming beam's, per batch row, formed on
        the device (differentiable through the beam's moments).
    :param emittance_x, emittance_y: geometric emittances (m) > 0; may carry a batch shape. `None`: the incoming beam's.
    :param num_bins: number of nodes M of the grid in tau, 2 <= M <= 4096.
    :param cutoff_wavelength: `None`, or the cutoff wavelength lambda_c > 0 (m) of the Gaussian low-pass filter of the deposit
        (`BinnedKick`); may carry a batch shape. A constant like `num_bins`: it must not require grad.
    :param seed: first half of the generator's key, an integer in 0 ... 2^32 - 1.
    :param stream: second half of the key, an integer in 0 ... 2^32 - 1: the kick's number within its lattice.

    A row in which the Coulomb logarithm, a size or an emittance is not > 0 or not finite gets NaN in delta.
    """

    #: LatticeJSON: read back as the Python values they were written as
    _plain_features = ("seed", "stream")
    _follows = "the intrabeam-scattering kick"

    def __init__(self, effect_length, coulomb_log=10.0, sigma_x=None, sigma_y=None, emittance_x=None, emittance_y=None,
                 num_bins: int = 200, seed: int = 0, stream: int = 0, name=None, sanitize_name=None, metadata=None, device=None,
                 dtype=None, *, cutoff_wavelength=None):
        owner = "IBSKick"
        num_bins = check_num_bins(num_bins, owner)
        seed, stream = check_key_word(seed, "seed", owner), check_key_word(stream, "stream", owner)
        effect_length = _as_tensor(effect_length, device, dtype)
        check_effect_length(effect_length, owner)
        fk = {"device": device if device is not None else effect_length.device,
              "dtype": dtype if dtype is not None else effect_length.dtype}
        if coulomb_log is None:
            raise ValueError(f"{owner}: coulomb_log must be finite and > 0, got None")
        coulomb_log = _as_tensor(coulomb_log, fk["device"], fk["dtype"])
        check_positive(coulomb_log, "coulomb_log")
        moments = {}
        for what, v in zip(_MOMENTS, (sigma_x, sigma_y, emittance_x, emittance_y)):
            if v is not None:
                v = _as_tensor(v, fk["device"], fk["dtype"])
                check_positive(v, f"{what} (metres)")
            moments[what] = v
        cutoff_wavelength = check_cutoff_wavelength(cutoff_wavelength, owner, **fk)
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        self.num_bins = num_bins
        self._register_cutoff(cutoff_wavelength)
        self.seed, self.stream = seed, stream
        self.register_buffer_or_parameter("effect_length", effect_length)
        self.register_buffer_or_parameter("coulomb_log", coulomb_log)
        for what, v in moments.items():
            self.register_buffer_or_parameter(what, v)
        # how many kicks this element has applied: the upper half of the generator's counter. Not persistent: a saved lattice
        # starts at call 0
        self.register_buffer("_call_index", torch.zeros(1, dtype=torch.int64, device=fk["device"]), persistent=False)

    @property
    def call_index(self) -> int:
        """The call index the next track draws with (reads the device back: not for the tracking path)."""
        return int(self._call_index.item())

    def reseed(self, seed=None, call_index: int = 0) -> None:
        """Set the call index (to 0: the sequence of tracks starts again, bit for bit) and, if given, the seed."""
        if isinstance(call_index, bool) or not isinstance(call_index, numbers.Integral) or not 0 <= int(call_index) < 2**63:
            raise ValueError(f"IBSKick.reseed: call_index must be an integer in 0 ... 2^63 - 1, got {call_index!r}")
        if seed is not None:
            self.seed = check_key_word(seed, "seed", "IBSKick")
        self._call_index.fill_(int(call_index))

    def clone(self) -> "IBSKick":
        c = super().clone()
        c._call_index.copy_(self._call_index)
        return c

    def _kick(self, incoming, species):
        given = [getattr(self, what) for what in _MOMENTS]
        if any(v is None for v in given):
            _ops.require_device(incoming.particles)
        moments = [getattr(incoming, what) if v is None else v for what, v in zip(_MOMENTS, given)]
        out = _ops.ibs_kick(incoming.particles, incoming.particle_charges, incoming.survival_probabilities, incoming.energy,
                            species.mass_eV_float, abs(species.num_elementary_charges_float), self.effect_length, self.coulomb_log,
                            *moments, self.num_bins, self.seed, self.stream, self._call_index, self.cutoff_wavelength)
        self._call_index.add_(1)
        return out

    @property
    def defining_features(self) -> list[str]:
        return self._with_cutoff(super().defining_features + ["effect_length", "coulomb_log", *_MOMENTS, "num_bins", "seed", "stream"])
