"""Dipole and RBend (mirror of cheetah/accelerator/dipole.py:58-135,372-466 and rbend.py:49-116)."""

from __future__ import annotations

import torch

from .. import _ops
from .element import Element


class Dipole(Element):
    """Sector bend: R = rot^T (R_exit_face @ base_rmatrix(L, k1, angle/L) @ R_enter_face) rot."""

    supported_tracking_methods = ["linear", "second_order", "drift_kick_drift"]
    _chx_kind = _ops.KIND["dipole"]
    _dkd_kind = _ops.DKD_KIND["dipole"]
    _t_kind = _ops.T_KIND["dipole"]

    def __init__(self, length, angle=None, k1=None, dipole_e1=None, dipole_e2=None, tilt=None, gap=None,
                 gap_exit=None, fringe_integral=None, fringe_integral_exit=None, fringe_at="both",
                 fringe_type="linear_edge", tracking_method="linear", name=None, sanitize_name=None,
                 metadata=None, device=None, dtype=None):
        fk = {"device": device, "dtype": dtype}
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        z = lambda v: v if v is not None else torch.tensor(0.0, **fk)  # noqa: E731
        self.length = length
        self.register_buffer_or_parameter("angle", z(angle))
        self.register_buffer_or_parameter("k1", z(k1))
        self.register_buffer_or_parameter("_e1", z(dipole_e1))
        self.register_buffer_or_parameter("_e2", z(dipole_e2))
        self.register_buffer_or_parameter("fringe_integral", z(fringe_integral))
        self.register_buffer_or_parameter(
            "fringe_integral_exit", fringe_integral_exit if fringe_integral_exit is not None else self.fringe_integral)
        self.register_buffer_or_parameter("gap", z(gap))
        self.register_buffer_or_parameter("gap_exit", gap_exit if gap_exit is not None else self.gap)
        self.register_buffer_or_parameter("tilt", z(tilt))
        self.fringe_at = fringe_at
        self.fringe_type = fringe_type
        self.tracking_method = tracking_method

    @property
    def hx(self) -> torch.Tensor:
        return self.angle / self.length

    @property
    def dipole_e1(self) -> torch.Tensor:
        return self._e1

    @dipole_e1.setter
    def dipole_e1(self, value) -> None:
        self._e1 = value
        self._touch()

    @property
    def dipole_e2(self) -> torch.Tensor:
        return self._e2

    @dipole_e2.setter
    def dipole_e2(self, value) -> None:
        self._e2 = value
        self._touch()

    def _builder_params(self):
        # NB: like the reference (dipole.py:453-459) the exit face uses `gap`, not `gap_exit`
        return [self.length, self.angle, self.k1, self._e1, self._e2, self.tilt, self.fringe_integral,
                self.fringe_integral_exit, self.gap]

    def _dkd_params(self):
        # dipole.py:183-370 (Bmad-X body + linear_edge fringes); unlike the linear map the exit face uses gap_exit
        return [self.length, self.angle, self._e1, self._e2, self.tilt, self.fringe_integral,
                self.fringe_integral_exit, self.gap, self.gap_exit]

    def _dkd_scalar_refs(self):
        return [(t, None) for t in self._dkd_params()]       # (buffers of the element, RBend's derived face angles included)

    def _dkd_options(self):
        return 1, _ops.FRINGE_AT[self.fringe_at]

    @property
    def is_skippable(self) -> bool:
        return self.tracking_method == "linear"

    @property
    def is_active(self) -> bool:
        return bool((self.angle != 0).any().item())

    def split_for_csr(self, num_kicks: int, num_bins: int = 200, transient: bool = False, cutoff_wavelength=None) -> list[Element]:
        """The bend as `num_kicks` x [Dipole of L / n and theta / n, CSRKick(L / n, theta / n, num_bins)]: steady-state CSR kicks
        spread along the arc. With `transient`, piece i gets `TransientCSRKick(L / n, theta / n, entrance_distance=(i + 1/2) L / n,
        num_bins)` instead: the wake at the piece's midpoint (the midpoint rule) of a bend behind a long straight. Only the first
        piece keeps the entrance face (dipole_e1, fringe_integral, the entrance fringe of `fringe_at`) and only the last keeps the
        exit face; k1, tilt, gap, gap_exit, fringe_type and tracking_method are kept. An RBend becomes Dipole pieces with its
        effective face angles. A bend of zero angle is returned unchanged, as [self]. Every kick gets `cutoff_wavelength`
        (`None`, or the cutoff of the low-pass filter of its deposit; a tensor of the bend's device and dtype is shared by the kicks)."""
        from ._binned_kick import check_cutoff_wavelength, check_num_bins, check_num_kicks
        from .csr import CSRKick, TransientCSRKick

        n = check_num_kicks(num_kicks, "Dipole.split_for_csr")
        num_bins = check_num_bins(num_bins, "Dipole.split_for_csr")
        fk = {"device": self.angle.device, "dtype": self.angle.dtype}
        cutoff_wavelength = check_cutoff_wavelength(cutoff_wavelength, "Dipole.split_for_csr", **fk)
        if not bool((self.angle != 0).any()):
            return [self]
        parts = []
        for i, piece in enumerate(self._arc_pieces(n, "csr")):
            parts.append(piece)
            kk = {"num_bins": num_bins, "cutoff_wavelength": cutoff_wavelength, "name": f"{self.name}_csr_kick_{i}",
                  "sanitize_name": False, **fk}
            parts.append(TransientCSRKick(piece.length, piece.angle, (i + 0.5) * piece.length, **kk) if transient
                         else CSRKick(piece.length, piece.angle, **kk))
        return parts

    def _arc_pieces(self, n: int, tag: str) -> list["Dipole"]:
        """The bend as n Dipoles of L / n and theta / n named `{name}_{tag}_{i}`, which share one length and one angle tensor: only the
        first keeps the entrance face and only the last the exit face (see `split_for_csr`)."""
        fk = {"device": self.angle.device, "dtype": self.angle.dtype}
        length, angle = self.length / n, self.angle / n
        entrance, exit_ = self.fringe_at in ("both", "entrance"), self.fringe_at in ("both", "exit")
        parts = []
        for i in range(n):
            first, last = i == 0, i == n - 1
            fringe_in, fringe_out = entrance and first, exit_ and last
            fringe_at = ("both" if fringe_out else "entrance") if fringe_in else ("exit" if fringe_out else "neither")
            parts.append(Dipole(
                length, angle=angle, k1=self.k1, dipole_e1=self._e1 if first else torch.zeros_like(self._e1),
                dipole_e2=self._e2 if last else torch.zeros_like(self._e2), tilt=self.tilt, gap=self.gap, gap_exit=self.gap_exit,
                fringe_integral=self.fringe_integral if first else torch.zeros_like(self.fringe_integral),
                fringe_integral_exit=self.fringe_integral_exit if last else torch.zeros_like(self.fringe_integral_exit),
                fringe_at=fringe_at, fringe_type=self.fringe_type, tracking_method=self.tracking_method,
                name=f"{self.name}_{tag}_{i}", sanitize_name=False, **fk))
        return parts

    def split_for_radiation(self, num_kicks: int, quantum_excitation: bool = True, seed: int = 0,
                            first_stream: int = 0) -> list[Element]:
        """The bend as `num_kicks` x [Dipole of L / n and theta / n, SynchrotronRadiationKick(L / n, theta / n, quantum_excitation,
        seed, stream=first_stream + i)]: the incoherent radiation spread along the arc, every kick with a stream of its own. The
        pieces are `split_for_csr`'s (faces, k1, tilt, gaps, fringe_type and tracking_method likewise), named `{name}_sr_{i}` with
        the kicks `{name}_sr_kick_{i}`. A bend of zero angle is returned unchanged, as [self]."""
        from ._binned_kick import check_num_kicks
        from .synchrotron_radiation import SynchrotronRadiationKick, check_key_word

        owner = "Dipole.split_for_radiation"
        n = check_num_kicks(num_kicks, owner)
        seed = check_key_word(seed, "seed", owner)
        first_stream = check_key_word(first_stream, "first_stream", owner)
        check_key_word(first_stream + n - 1, "first_stream + num_kicks - 1", owner)
        if not bool((self.angle != 0).any()):
            return [self]
        fk = {"device": self.angle.device, "dtype": self.angle.dtype}
        parts = []
        for i, piece in enumerate(self._arc_pieces(n, "sr")):
            parts.append(piece)
            parts.append(SynchrotronRadiationKick(piece.length, piece.angle, quantum_excitation=quantum_excitation, seed=seed,
                                                  stream=first_stream + i, name=f"{self.name}_sr_kick_{i}", sanitize_name=False, **fk))
        return parts

    @property
    def defining_features(self) -> list[str]:
        return super().defining_features + ["length", "angle", "k1", "dipole_e1", "dipole_e2", "tilt", "gap",
                                            "gap_exit", "fringe_integral", "fringe_integral_exit", "fringe_at",
                                            "fringe_type"]


class RBend(Dipole):
    """Rectangular bend: a Dipole whose pole-face angles include half the bend angle (rbend.py:104-116)."""

    def __init__(self, length, angle=None, k1=None, rbend_e1=None, rbend_e2=None, tilt=None, gap=None,
                 gap_exit=None, fringe_integral=None, fringe_integral_exit=None, fringe_at="both",
                 fringe_type="linear_edge", tracking_method="linear", name=None, sanitize_name=None,
                 metadata=None, device=None, dtype=None):
        fk = {"device": device, "dtype": dtype}
        angle = angle if angle is not None else torch.tensor(0.0, **fk)
        e1 = rbend_e1 if rbend_e1 is not None else torch.tensor(0.0, **fk)
        e2 = rbend_e2 if rbend_e2 is not None else torch.tensor(0.0, **fk)
        super().__init__(length=length, angle=angle, k1=k1, dipole_e1=e1 + angle / 2, dipole_e2=e2 + angle / 2,
                         tilt=tilt, gap=gap, gap_exit=gap_exit, fringe_integral=fringe_integral,
                         fringe_integral_exit=fringe_integral_exit, fringe_at=fringe_at, fringe_type=fringe_type,
                         tracking_method=tracking_method, name=name, sanitize_name=sanitize_name,
                         metadata=metadata, **fk)

    @property
    def rbend_e1(self) -> torch.Tensor:
        return self._e1 - self.angle / 2

    @rbend_e1.setter
    def rbend_e1(self, value: torch.Tensor) -> None:  # rbend.py:107-110
        self.dipole_e1 = value + self.angle / 2

    @property
    def rbend_e2(self) -> torch.Tensor:
        return self._e2 - self.angle / 2

    @rbend_e2.setter
    def rbend_e2(self, value: torch.Tensor) -> None:  # rbend.py:114-117
        self.dipole_e2 = value + self.angle / 2

    @property
    def defining_features(self) -> list[str]:
        feats = [f for f in super().defining_features if f not in ("dipole_e1", "dipole_e2")]
        return feats + ["rbend_e1", "rbend_e2"]
