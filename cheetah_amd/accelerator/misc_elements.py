"""Remaining linear elements of SURVEY section 8 row f3 (mirror of cheetah/accelerator/solenoid.py:41-116,
undulator.py:41-125, sextupole.py:47-88): their first-order maps come from the same `chx_build_rmatrix`
kernel (kinds SOLENOID / UNDULATOR / DRIFT) and are tracked by the same apply kernel."""

from __future__ import annotations

import operator

import torch

from .. import _ops
from .element import Element


class Solenoid(Element):
    """Hard-edge solenoid with transverse misalignment."""

    supported_tracking_methods = ["linear"]
    _chx_kind = _ops.KIND["solenoid"]

    def __init__(self, length, k=None, misalignment=None, name=None, sanitize_name=None, metadata=None, device=None,
                 dtype=None) -> None:
        fk = {"device": device, "dtype": dtype}
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        self.length = length
        self.register_buffer_or_parameter("k", k if k is not None else torch.tensor(0.0, **fk))
        self.register_buffer_or_parameter(
            "misalignment", misalignment if misalignment is not None else torch.tensor((0.0, 0.0), **fk))

    def _builder_params(self):
        return [self.length, self.k, self.misalignment[..., 0], self.misalignment[..., 1]]

    def _builder_scalar_refs(self):
        m = self.misalignment
        return [(self.length, None), (self.k, None), (m, 0), (m, 1)]

    _merge_equal = ("misalignment",)
    _merge_weighted = ("k",)

    def split(self, resolution):
        return self._split_evenly(resolution)

    @property
    def is_active(self) -> bool:
        return bool((self.k != 0).any().item())

    @property
    def is_skippable(self) -> bool:
        return True

    @property
    def defining_features(self) -> list[str]:
        return super().defining_features + ["length", "k", "misalignment"]


class Undulator(Element):
    """Planar / helical undulator (linear focusing only, no radiation)."""

    supported_tracking_methods = ["linear"]
    _chx_kind = _ops.KIND["undulator"]

    def __init__(self, length, period=None, kx=None, ky=None, name=None, sanitize_name=None, metadata=None, device=None,
                 dtype=None) -> None:
        fk = {"device": device, "dtype": dtype}
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        self.length = length
        self.register_buffer_or_parameter("kx", kx if kx is not None else torch.tensor(0.0, **fk))
        self.register_buffer_or_parameter("ky", ky if ky is not None else torch.tensor(0.0, **fk))
        self.register_buffer_or_parameter("period", period if period is not None else torch.tensor(1.0, **fk))

    def _builder_params(self):
        return [self.length, self.kx, self.ky, self.period]

    @property
    def is_active(self) -> bool:
        return bool(torch.logical_or(self.kx != 0.0, self.ky != 0.0).any().item())

    @property
    def is_skippable(self) -> bool:
        return True

    def resonant_wavelength(self, energy, species=None) -> torch.Tensor:
        """The wavelength lambda_u (1 + K^2 / 2) / (2 gamma0^2) of the undulator's fundamental on axis for a beam of reference
        energy `energy` (eV), K^2 = kx^2 + ky^2; `species=None` is an electron."""
        from ..particles.species import electron_mass_eV

        energy = torch.as_tensor(energy, dtype=self.period.dtype, device=self.period.device)
        gamma = energy / (electron_mass_eV if species is None else species.mass_eV.to(energy.device))
        return self.period * (1 + (self.kx.square() + self.ky.square()) / 2) / (2 * gamma.square())

    def with_laser(self, peak_power, laser_sigma, energy, wavelength=None, phase=0.0, offset_x=0.0, offset_y=0.0, pulse_sigma=None,
                   pulse_center=0.0, num_kicks: int = 1):
        """The undulator with a laser in it, as a `Segment` of `num_kicks` x [Undulator of L / 2n, LaserModulator, Undulator of
        L / 2n]: the energy modulation of a laser of peak power `peak_power` (W) and rms intensity size `laser_sigma` (m) on a beam
        of electrons of reference energy `energy` (eV), every kick with the amplitude `laser_modulation_amplitude` gives for L / n.
        `wavelength=None` takes the resonant one. For a planar undulator: K is the one non-zero of `kx`, `ky`. The pieces are
        named `{name}_laser_{j}`, the kicks `{name}_laser_kick_{i}`; the pieces' total map is the undulator's own."""
        from ._binned_kick import check_num_kicks
        from .laser_modulator import LaserModulator, laser_modulation_amplitude
        from .segment import Segment

        owner = "Undulator.with_laser"
        n = check_num_kicks(num_kicks, owner)
        has_kx, has_ky = bool((self.kx != 0).any()), bool((self.ky != 0).any())
        if has_kx == has_ky:
            raise ValueError(f"{owner}: a planar undulator has exactly one of kx and ky non-zero, got kx={self.kx!r}, ky={self.ky!r}")
        K = self.kx if has_kx else self.ky
        fk = {"device": self.length.device, "dtype": self.length.dtype}
        t = lambda v: v if v is None or isinstance(v, torch.Tensor) else torch.as_tensor(v, **fk)  # noqa: E731
        energy = t(energy)
        if wavelength is None:
            wavelength = self.resonant_wavelength(energy)
        amplitude = laser_modulation_amplitude(t(peak_power), K, self.length / n, t(laser_sigma), energy)
        elements = []
        for i in range(n):
            halves = [Undulator(self.length / (2 * n), period=self.period, kx=self.kx, ky=self.ky, name=f"{self.name}_laser_{2 * i + j}",
                                sanitize_name=False, **fk) for j in range(2)]
            kick = LaserModulator(amplitude, t(wavelength), t(laser_sigma), phase=t(phase), offset_x=t(offset_x), offset_y=t(offset_y),
                                  pulse_sigma=t(pulse_sigma), pulse_center=t(pulse_center), name=f"{self.name}_laser_kick_{i}",
                                  sanitize_name=False, **fk)
            elements += [halves[0], kick, halves[1]]
        return Segment(elements, name=self.name, sanitize_name=False)

    @property
    def defining_features(self) -> list[str]:
        return super().defining_features + ["length", "period", "kx", "ky"]


class Sextupole(Element):
    """Sextupole (sextupole.py:45-132): a drift in first order, the k2 kick through the second-order tensor. With
    `tracking_method="drift_kick_drift"` (not in the reference): Bmad's exact drifts around `num_steps` thin kicks of k2 L /
    num_steps each — drift L / 2n, then n x (kick, drift L / n; L / 2n behind the last kick) inside the misalignment and tilt
    transformations. Symplectic, unlike the truncated second-order map; k2 = 0 is a drift-kick-drift Drift. `num_steps` is
    read by this method only."""

    supported_tracking_methods = ["linear", "second_order", "drift_kick_drift"]
    _chx_kind = _ops.KIND["drift"]
    _dkd_kind = _ops.DKD_KIND["sextupole"]
    _t_kind = _ops.T_KIND["sextupole"]

    def __init__(self, length, k2=None, misalignment=None, tilt=None, tracking_method="second_order", name=None,
                 sanitize_name=None, metadata=None, device=None, dtype=None, num_steps=1) -> None:
        fk = {"device": device, "dtype": dtype}
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        self.length = length
        self.register_buffer_or_parameter("k2", k2 if k2 is not None else torch.tensor(0.0, **fk))
        self.register_buffer_or_parameter(
            "misalignment", misalignment if misalignment is not None else torch.tensor((0.0, 0.0), **fk))
        self.register_buffer_or_parameter("tilt", tilt if tilt is not None else torch.tensor(0.0, **fk))
        self.num_steps = num_steps
        self.tracking_method = tracking_method

    @property
    def num_steps(self) -> int:
        """Number of thin kicks of the drift-kick-drift method (an int of 1 .. 2^25 - 1, what the chain's packing holds)."""
        return self._num_steps

    @num_steps.setter
    def num_steps(self, value) -> None:
        try:
            steps = None if isinstance(value, bool) else operator.index(value)
        except TypeError:
            steps = None
        if steps is None or not 1 <= steps < (1 << 25):
            raise ValueError(f"Sextupole.num_steps must be an int of 1 .. {(1 << 25) - 1}, got {value!r}")
        self._num_steps = steps

    def _builder_params(self):
        return [self.length]

    def _t_params(self):
        return [self.length, self.k2, self.tilt, self.misalignment[..., 0], self.misalignment[..., 1]]

    def _dkd_params(self):
        return self._t_params()

    def _dkd_scalar_refs(self):
        length, k2, tilt, m = self._settings("length", "k2", "tilt", "misalignment")
        return [(length, None), (k2, None), (tilt, None), (m, 0), (m, 1)]

    def _dkd_options(self):
        return self._num_steps, 3

    _merge_equal = ("tracking_method", "k2", "misalignment", "tilt")

    def merge(self, other):
        merged = super().merge(other)
        if merged is not None and self._tracking_method == "drift_kick_drift":
            merged.num_steps = self._num_steps + other._num_steps       # (summed like a Quadrupole's; the other methods never read it)
        return merged

    @property
    def is_active(self) -> bool:
        return bool((self.k2 != 0).any().item())

    @property
    def is_skippable(self) -> bool:
        return self.tracking_method == "linear"

    @property
    def defining_features(self) -> list[str]:
        # (`num_steps` is not among them: the reference's Sextupole has no such feature, and the files the two projects write
        # for one lattice are compared key by key — `clone` and LatticeJSON carry it on their own)
        return super().defining_features + ["length", "k2", "misalignment", "tilt"]

    def clone(self) -> "Sextupole":
        clone = super().clone()
        clone.num_steps = self._num_steps
        return clone

    def _json_extras(self) -> dict:
        # only where it is read and is not the default: every other Sextupole writes the reference's keys and nothing else (the
        # reference's constructor has no such argument, so its loader would refuse the file)
        return {"num_steps": self._num_steps} if self._tracking_method == "drift_kick_drift" and self._num_steps != 1 else {}

    def __repr__(self) -> str:
        text = super().__repr__()
        return text if self._num_steps == 1 else f"{text[:-1]}, num_steps={self._num_steps})"


class TransverseDeflectingCavity(Element):
    """Transverse deflecting cavity (transverse_deflecting_cavity.py:44-209): half drift, transverse RF kick with the
    matching energy change, half drift, tracked per particle by chx_dkd_track (drift_kick_drift only)."""

    supported_tracking_methods = ["drift_kick_drift"]
    _dkd_kind = _ops.DKD_KIND["tdc"]

    def __init__(self, length, voltage=None, phase=None, frequency=None, misalignment=None, tilt=None, num_steps=1,
                 tracking_method="drift_kick_drift", name=None, sanitize_name=None, metadata=None, device=None,
                 dtype=None) -> None:
        fk = {"device": device, "dtype": dtype}
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        z = lambda v: v if v is not None else torch.tensor(0.0, **fk)  # noqa: E731
        self.length = length
        self.register_buffer_or_parameter("voltage", z(voltage))
        self.register_buffer_or_parameter("phase", z(phase))
        self.register_buffer_or_parameter("frequency", z(frequency))
        self.register_buffer_or_parameter(
            "misalignment", misalignment if misalignment is not None else torch.tensor((0.0, 0.0), **fk))
        self.register_buffer_or_parameter("tilt", z(tilt))
        self.num_steps = num_steps
        self._tracking_method = "drift_kick_drift"
        self.tracking_method = tracking_method

    def _dkd_params(self):
        return [self.length, self.voltage, self.phase, self.frequency, self.tilt, self.misalignment[..., 0],
                self.misalignment[..., 1]]

    @property
    def is_active(self) -> bool:
        return bool((self.voltage != 0).any().item())

    @property
    def is_skippable(self) -> bool:
        return False

    @property
    def defining_features(self) -> list[str]:
        return super().defining_features + ["length", "voltage", "phase", "frequency", "misalignment", "tilt",
                                            "num_steps"]


class RFCavity(Element):
    """RF cavity of a storage ring (not in the reference; Bmad's `rfcavity`, bmad_standard, from the reference's Bmad-X building
    blocks): half a drift, the energy kick dE = |n_q| V sin(2 pi (phase - frequency t)) at the particle's own time offset
    t = tau / c, half a drift — tracked per particle by chx_dkd_track (drift_kick_drift only), symplectic, in one chain call with
    its neighbours (`Segment.track`) and inside the fused ring (`Segment.track_turns`). Unlike the linac `Cavity` it does NOT change
    the reference energy: the storage-ring convention. `phase` is in units of 2 pi, as for the TransverseDeflectingCavity and
    Bmad: phase = 0 is the stable zero crossing above transition, phase = 0.5 the stable one below. With sin(2 pi phase) != 0 the
    synchronous particle gains |n_q| V sin(2 pi phase) per pass while the reference energy stays. A thin cavity (`length = 0`)
    is allowed; the kick depends on neither x nor y, so there is no tilt and no misalignment. A particle whose total energy
    falls below its rest mass becomes NaN and is lost by the loss rule of `track_turns`."""

    supported_tracking_methods = ["drift_kick_drift"]
    _dkd_kind = _ops.DKD_KIND["rfcavity"]

    def __init__(self, length, voltage=None, phase=None, frequency=None, tracking_method="drift_kick_drift", name=None,
                 sanitize_name=None, metadata=None, device=None, dtype=None) -> None:
        fk = {"device": device, "dtype": dtype}
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        z = lambda v: v if v is not None else torch.tensor(0.0, **fk)  # noqa: E731
        if bool((torch.as_tensor(length) < 0).any()):
            raise ValueError(f"RFCavity.length must not be negative, got {length!r}")
        self.length = length
        self.register_buffer_or_parameter("voltage", z(voltage))
        self.register_buffer_or_parameter("phase", z(phase))
        self.register_buffer_or_parameter("frequency", z(frequency))
        self._tracking_method = "drift_kick_drift"
        self.tracking_method = tracking_method

    def _dkd_params(self):
        return [self.length, self.voltage, self.phase, self.frequency]

    def _dkd_scalar_refs(self):
        return [(t, None) for t in self._settings("length", "voltage", "phase", "frequency")]

    def _dkd_options(self):
        return 1, 0         # (num_steps is not read; no fringe)

    @staticmethod
    def harmonic_frequency(circumference, harmonic, energy, species=None) -> torch.Tensor:
        """The RF frequency h beta0 c / C (Hz) of harmonic number `harmonic` in a ring of circumference `circumference` (m) for a
        beam of reference energy `energy` (eV); `species=None` is an electron."""
        from ..particles.particle_beam import speed_of_light
        from ..particles.species import electron_mass_eV

        energy = torch.as_tensor(energy)
        if not energy.is_floating_point():
            energy = energy.to(torch.get_default_dtype())
        mass = electron_mass_eV if species is None else species.mass_eV.to(energy.device)
        beta0 = torch.sqrt(1 - (mass / energy).square())
        return harmonic * beta0 * speed_of_light / circumference

    @property
    def is_active(self) -> bool:
        return bool((self.voltage != 0).any().item())

    @property
    def is_skippable(self) -> bool:
        return False

    @property
    def defining_features(self) -> list[str]:
        return super().defining_features + ["length", "voltage", "phase", "frequency"]


class Multipole(Element):
    """Thin multipole kicks of ONE order m between Bmad's exact drifts (not in the reference; MAD-X's `MULTIPOLE`, Elegant's `MULT`,
    from the reference's Bmad-X building blocks): drift L / 2n, then n x (kick, drift L / n; L / 2n behind the last kick) inside
    the misalignment and tilt transformations, every kick

        d px - i d py = -(knl + i ksl) / n (x + i y)^m / m!

    `order` m is a Python int and a constant of the element: 0 a dipole kick, 1 a quadrupole, 2 a sextupole, 3 an octupole. `knl`
    and `ksl` are the INTEGRATED normal and skew strengths in m^-m (MAD-X's knl / ksl), so a thin element (`length = 0`) is the
    common case: the drifts then leave the coordinates alone and `s` stays. `Sextupole(L, k2)` is `Multipole(L, 2, knl=k2 L)`, a
    horizontal corrector of angle theta is order 0 with knl = -theta, a skew quadrupole order 1 with `ksl`. Tracked per particle by
    chx_dkd_track (drift_kick_drift only), symplectic, in one chain call with its neighbours (`Segment.track`) and inside the
    fused ring (`Segment.track_turns`). `num_steps` = n as for the Sextupole."""

    supported_tracking_methods = ["drift_kick_drift"]
    _dkd_kind = _ops.DKD_KIND["multipole"]

    def __init__(self, length, order, knl=None, ksl=None, misalignment=None, tilt=None, num_steps=1,
                 tracking_method="drift_kick_drift", name=None, sanitize_name=None, metadata=None, device=None, dtype=None) -> None:
        fk = {"device": device, "dtype": dtype}
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        z = lambda v: v if v is not None else torch.tensor(0.0, **fk)  # noqa: E731
        if bool((torch.as_tensor(length) < 0).any()):
            raise ValueError(f"Multipole.length must not be negative, got {length!r}")
        self.length = length
        self.order = order
        self.register_buffer_or_parameter("knl", z(knl))
        self.register_buffer_or_parameter("ksl", z(ksl))
        self.register_buffer_or_parameter(
            "misalignment", misalignment if misalignment is not None else torch.tensor((0.0, 0.0), **fk))
        self.register_buffer_or_parameter("tilt", z(tilt))
        self.num_steps = num_steps
        self._tracking_method = "drift_kick_drift"
        self.tracking_method = tracking_method

    @property
    def order(self) -> int:
        """The order m of the kick (x + i y)^m: an int of 0 .. 3 (what the two `fringe_at` bits of the kernels' arguments hold)."""
        return self._order

    @order.setter
    def order(self, value) -> None:
        if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= 3:
            raise ValueError(f"Multipole.order must be an int of 0 .. 3 (dipole, quadrupole, sextupole, octupole), got {value!r}")
        self._order = value

    @property
    def num_steps(self) -> int:
        """Number of thin kicks (an int of 1 .. 2^25 - 1, what the chain's packing holds)."""
        return self._num_steps

    @num_steps.setter
    def num_steps(self, value) -> None:
        try:
            steps = None if isinstance(value, bool) else operator.index(value)
        except TypeError:
            steps = None
        if steps is None or not 1 <= steps < (1 << 25):
            raise ValueError(f"Multipole.num_steps must be an int of 1 .. {(1 << 25) - 1}, got {value!r}")
        self._num_steps = steps

    def _dkd_params(self):
        return [self.length, self.knl, self.ksl, self.tilt, self.misalignment[..., 0], self.misalignment[..., 1]]

    def _dkd_scalar_refs(self):
        length, knl, ksl, tilt, m = self._settings("length", "knl", "ksl", "tilt", "misalignment")
        return [(length, None), (knl, None), (ksl, None), (tilt, None), (m, 0), (m, 1)]

    def _dkd_options(self):
        return self._num_steps, self._order         # (the order travels where a Dipole's fringe bits do: include/chx.h)

    @property
    def is_active(self) -> bool:
        return bool(torch.logical_or(self.knl != 0, self.ksl != 0).any().item())

    @property
    def is_skippable(self) -> bool:
        return False

    @property
    def defining_features(self) -> list[str]:
        return super().defining_features + ["length", "order", "knl", "ksl", "misalignment", "tilt"]

    def clone(self) -> "Multipole":
        clone = super().clone()
        clone.num_steps = self._num_steps
        return clone

    def _json_extras(self) -> dict:
        return {"num_steps": self._num_steps} if self._num_steps != 1 else {}

    def __repr__(self) -> str:
        text = super().__repr__()
        return text if self._num_steps == 1 else f"{text[:-1]}, num_steps={self._num_steps})"
