"""CSRKick, TransientCSRKick and CSRDriftKick: the coherent synchrotron radiation (CSR) of a bending magnet's arc, in the steady
state and with the entrance transient, and in the drift behind the bend, applied as one instantaneous energy kick that follows the
bunch's current profile. Put kicks into a lattice with `Dipole.split_for_csr` or `Segment.with_csr_kicks`.

The kick is one `chx_csr_kick` call (`_ops.csr_kick`): per batch row, the surviving particles (survival probability > 0, finite
tau) are deposited on `num_bins` nodes spanning their tau range, exactly as `Wakefield` deposits them. The line density is taken
piecewise linear between the nodes and the 1-D steady-state kernel (Derbenev, Rossbach, Saldin, Shiltsev, TESLA-FEL 95-05 (1995);
Saldin, Schneidmiller, Yurkov, NIM A 398 (1997) 373)

    dE/ds(z) = -2 Z e / (4 pi eps0 3^(1/3) R^(2/3)) int_{-inf}^{z} (z - z')^(-1/3) lambda'(z') dz'

is integrated exactly over every interval, so there is no singular self term. A larger tau is the tail: the sources of a witness
are the particles behind it, and the head gains energy. Per node, with h the node spacing and D_k the deposited charge,

    dE_k = |Z| 3^(2/3) k_e L^(1/3) |theta|^(2/3) h^(-4/3) sum_j b_j D_(k+j),    delta += dE(tau) / p0c

with b_0 = -1, b_j = a_(j-1) - a_j, a_j = (j+1)^(2/3) - j^(2/3). Deterministic, no host synchronisation, capturable in a device
graph, differentiable with respect to the particles, charges, survival probabilities, the beam energy, `effect_length` and
`angle` (the node grid is a constant).

TransientCSRKick is the same call with the kernel of a bunch that has travelled the arc length d into a bend of radius R behind a
long straight (Saldin, Schneidmiller, Yurkov, section 3). With the slippage length z_L = d^3 / (24 R^2),

    dE/ds(tau) = (2 Z e / (4 pi eps0 3^(1/3) R^(2/3))) { int_0^{z_L} u^(-1/3) lambda'(tau + u) du
                                                       - z_L^(-1/3) [lambda(tau + z_L) - lambda(tau + 4 z_L)] }

which is 0 for z_L -> 0 and the steady state for z_L -> inf. On the nodes, with x = z_L / h (`chx_csr_transient_kick`),

    dE_k = |Z| 3^(2/3) k_e L^(1/3) |theta|^(2/3) h^(-4/3) S_k(x)
    S_k(x) = sum_j a~_j(x) (D_(k+j+1) - D_(k+j)) - (2/3) x^(-1/3) [D~(k + x) - D~(k + 4x)]
    a~_j(x) = min(j+1, x)^(2/3) - min(j, x)^(2/3)

where D~(y) interpolates the deposits linearly at the real index y and is 0 beyond the last node. For x >= M the sum is CSRKick's
term for term, and so is the result, bit for bit. Differentiable with respect to `entrance_distance` as well; S is continuous in x
and its derivative jumps where 4x crosses a node.

CSRDriftKick is the same call with the wake a distance x behind the exit face of a bend of radius R and angle phi: the radiation
emitted inside the bend keeps catching up with the bunch (Stupakov, Emma, EPAC 2002, case D). With xh = x / R and the retarded angle
psi(u) the root of u = (R / 24) psi^3 (psi + 4 xh) / (psi + xh), u_max = u(phi),

    dE/ds(tau) = Z e k_e (4 / R) { int_0^{u_max} lambda'(tau + u) / (psi(u) + 2 xh) du - lambda(tau + u_max) / (phi + 2 xh) }

On the nodes (`chx_csr_drift_kick`), with kappa = 24 h / R, psi_j = min(psi(j h), phi) and y = u_max / h,

    delta_k += (|Z| k_e L / p0c) S_k
    S_k = (1 / (2 h^2)) { sum_j [G(psi_(j+1)) - G(psi_j)] (D_(k+j+1) - D_(k+j)) - kappa / (3 (phi + 2 xh)) D~(k + y) }
    G(psi) = psi^2 / 2 + xh^2 psi / (psi + xh) - xh^2 log1p(psi / xh)

since int du / (psi + 2 xh) = (R / 8) G(psi) in closed form; below psi / xh = 1/4, where the closed form cancels, G is summed as its
series from the cubic term on. At x = 0 and y beyond the grid the sum is CSRKick(L, L / R)'s. Differentiable with respect to
`effect_length`, `bend_length`, `bend_angle` and `exit_distance` (the lags floor(y), floor(y) + 1 held fixed)."""

from __future__ import annotations

import torch

from .. import _ops
from ._binned_kick import BinnedKick, _as_tensor, check_cutoff_wavelength, check_effect_length, check_num_bins


class CSRKick(BinnedKick):
    """Steady-state CSR of an arc of a bend, as one zero-length energy kick.

    Limits of the model: steady state only (no exit transient inside the bend; `TransientCSRKick` has the entrance transient and
    `CSRDriftKick` the CSR in the drifts behind a bend); 1-D (a line charge: no transverse forces, no dependence on the transverse size); the arc is taken as long
    as the formation length (24 sigma_z R^2)^(1/3) or longer, and a shorter arc is overestimated. Without a
    `cutoff_wavelength` the deposit is used raw: at a fixed number of particles N the noise then grows with `num_bins` (for a Gaussian
    bunch of N = 10^6 the pointwise rms error of the kick is about 4 % at M = 200 and 13 % at M = 1000). With one, `num_bins` sets the
    resolution and the cutoff the noise, and the kick converges as M grows.

    :param effect_length: arc length L >= 0 (m) the kick stands for; may carry a batch shape that broadcasts with the beam's.
    :param angle: bend angle theta (rad) of that arc, L / R; may carry a batch shape. The kick scales as L^(1/3) |theta|^(2/3).
    :param num_bins: number of nodes M of the grid in tau, 2 <= M <= 4096.
    :param cutoff_wavelength: `None`, or the cutoff wavelength lambda_c > 0 (m) of the Gaussian low-pass filter of the deposit
        (`BinnedKick`); may carry a batch shape. A constant like `num_bins`: it must not require grad.
    """

    _follows = "the CSR kick"

    def __init__(self, effect_length, angle, num_bins: int = 200, name=None, sanitize_name=None, metadata=None, device=None,
                 dtype=None, *, cutoff_wavelength=None):
        num_bins = check_num_bins(num_bins, "CSRKick")
        effect_length = _as_tensor(effect_length, device, dtype)
        angle = _as_tensor(angle, device, dtype)
        check_effect_length(effect_length, "CSRKick")
        if not bool(torch.isfinite(angle.detach()).all()):
            raise ValueError(f"CSRKick: angle must be finite (rad), got {angle!r}")
        fk = {"device": device if device is not None else effect_length.device,
              "dtype": dtype if dtype is not None else effect_length.dtype}
        cutoff_wavelength = check_cutoff_wavelength(cutoff_wavelength, type(self).__name__, **fk)
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        self.num_bins = num_bins
        self._register_cutoff(cutoff_wavelength)
        self.register_buffer_or_parameter("effect_length", effect_length)
        self.register_buffer_or_parameter("angle", angle)

    def _kick(self, incoming, species):
        return _ops.csr_kick(incoming.particles, incoming.particle_charges, incoming.survival_probabilities, incoming.energy,
                             species.mass_eV_float, abs(species.num_elementary_charges_float), self.effect_length, self.angle,
                             self.num_bins, self.cutoff_wavelength)

    @property
    def defining_features(self) -> list[str]:
        return self._with_cutoff(super().defining_features + ["effect_length", "angle", "num_bins"])


class TransientCSRKick(BinnedKick):
    """CSR of an arc of a bend at a given arc length behind the bend's entrance face, as one zero-length energy kick: the entrance
    transient, in which the wake builds up over the formation length, and the steady state behind it.

    Limits of the model: ultra-relativistic; 1-D (a line charge: no transverse forces, no dependence on the transverse size); a
    long straight in front of the bend (no radiation of an earlier bend catches up with the bunch); the CSR in the drift behind the
    bend (exit transient) is `CSRDriftKick`'s. The deposit is used raw unless a `cutoff_wavelength` is given, as in `CSRKick`.

    :param effect_length: arc length L >= 0 (m) the kick stands for; may carry a batch shape that broadcasts with the beam's.
    :param angle: bend angle theta (rad) of that arc; may carry a batch shape. The bend's radius is R = L / |theta|.
    :param entrance_distance: arc length d >= 0 (m) from the bend's entrance face to the point where the wake is evaluated; may
        carry a batch shape. At d = 0 there is no kick; for d^3 / (24 R^2) beyond the bunch's length the kick is `CSRKick`'s.
    :param num_bins: number of nodes M of the grid in tau, 2 <= M <= 4096.
    :param cutoff_wavelength: `None`, or the cutoff wavelength lambda_c > 0 (m) of the Gaussian low-pass filter of the deposit
        (`BinnedKick`); may carry a batch shape. A constant like `num_bins`: it must not require grad.
    """

    _follows = "the CSR kick"

    def __init__(self, effect_length, angle, entrance_distance, num_bins: int = 200, name=None, sanitize_name=None, metadata=None,
                 device=None, dtype=None, *, cutoff_wavelength=None):
        num_bins = check_num_bins(num_bins, "TransientCSRKick")
        effect_length = _as_tensor(effect_length, device, dtype)
        angle = _as_tensor(angle, device, dtype)
        entrance_distance = _as_tensor(entrance_distance, device, dtype)
        check_effect_length(effect_length, "TransientCSRKick")
        if not bool(torch.isfinite(angle.detach()).all()):
            raise ValueError(f"TransientCSRKick: angle must be finite (rad), got {angle!r}")
        if not bool(torch.isfinite(entrance_distance.detach()).all() & (entrance_distance.detach() >= 0).all()):
            raise ValueError(f"TransientCSRKick: entrance_distance must be finite and >= 0 (metres), got {entrance_distance!r}")
        fk = {"device": device if device is not None else effect_length.device,
              "dtype": dtype if dtype is not None else effect_length.dtype}
        cutoff_wavelength = check_cutoff_wavelength(cutoff_wavelength, type(self).__name__, **fk)
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        self.num_bins = num_bins
        self._register_cutoff(cutoff_wavelength)
        self.register_buffer_or_parameter("effect_length", effect_length)
        self.register_buffer_or_parameter("angle", angle)
        self.register_buffer_or_parameter("entrance_distance", entrance_distance)

    def _kick(self, incoming, species):
        return _ops.csr_transient_kick(incoming.particles, incoming.particle_charges, incoming.survival_probabilities,
                                       incoming.energy, species.mass_eV_float, abs(species.num_elementary_charges_float),
                                       self.effect_length, self.angle, self.entrance_distance, self.num_bins, self.cutoff_wavelength)

    @property
    def defining_features(self) -> list[str]:
        return self._with_cutoff(super().defining_features + ["effect_length", "angle", "entrance_distance", "num_bins"])


class CSRDriftKick(BinnedKick):
    """CSR in a piece of drift behind a bend, as one zero-length energy kick: the radiation emitted inside the bend that catches up
    with the bunch a given distance behind the bend's exit face.

    Limits of the model: ultra-relativistic; 1-D (a line charge: no transverse forces, no dependence on the transverse size); the
    sources are in this one bend only (no radiation of an earlier bend); the straight in front of the bend is ignored (the bend's
    own entrance transient is not carried into the drift). The deposit is used raw unless a `cutoff_wavelength` is given, as in `CSRKick`.

    :param effect_length: length L >= 0 (m) of the piece of drift the kick stands for; may carry a batch shape that broadcasts with
        the beam's.
    :param bend_length: arc length L_b >= 0 (m) of the bend in front of the drift; may carry a batch shape.
    :param bend_angle: angle theta (rad) of that bend; may carry a batch shape. The bend's radius is R = L_b / |theta|.
    :param exit_distance: distance x >= 0 (m) from the bend's exit face to the point where the wake is evaluated; may carry a batch
        shape. The kick decays with x; at x = 0 it is `TransientCSRKick`'s at the end of the bend without the term of the straight
        in front of the bend.
    :param num_bins: number of nodes M of the grid in tau, 2 <= M <= 4096.
    :param cutoff_wavelength: `None`, or the cutoff wavelength lambda_c > 0 (m) of the Gaussian low-pass filter of the deposit
        (`BinnedKick`); may carry a batch shape. A constant like `num_bins`: it must not require grad.
    """

    _follows = "the CSR kick"

    def __init__(self, effect_length, bend_length, bend_angle, exit_distance, num_bins: int = 200, name=None, sanitize_name=None,
                 metadata=None, device=None, dtype=None, *, cutoff_wavelength=None):
        num_bins = check_num_bins(num_bins, "CSRDriftKick")
        effect_length = _as_tensor(effect_length, device, dtype)
        bend_length = _as_tensor(bend_length, device, dtype)
        bend_angle = _as_tensor(bend_angle, device, dtype)
        exit_distance = _as_tensor(exit_distance, device, dtype)
        check_effect_length(effect_length, "CSRDriftKick")
        for what, v in (("bend_length", bend_length), ("exit_distance", exit_distance)):
            if not bool(torch.isfinite(v.detach()).all() & (v.detach() >= 0).all()):
                raise ValueError(f"CSRDriftKick: {what} must be finite and >= 0 (metres), got {v!r}")
        if not bool(torch.isfinite(bend_angle.detach()).all()):
            raise ValueError(f"CSRDriftKick: bend_angle must be finite (rad), got {bend_angle!r}")
        fk = {"device": device if device is not None else effect_length.device,
              "dtype": dtype if dtype is not None else effect_length.dtype}
        cutoff_wavelength = check_cutoff_wavelength(cutoff_wavelength, type(self).__name__, **fk)
        super().__init__(name=name, sanitize_name=sanitize_name, metadata=metadata, **fk)
        self.num_bins = num_bins
        self._register_cutoff(cutoff_wavelength)
        self.register_buffer_or_parameter("effect_length", effect_length)
        self.register_buffer_or_parameter("bend_length", bend_length)
        self.register_buffer_or_parameter("bend_angle", bend_angle)
        self.register_buffer_or_parameter("exit_distance", exit_distance)

    def _kick(self, incoming, species):
        return _ops.csr_drift_kick(incoming.particles, incoming.particle_charges, incoming.survival_probabilities, incoming.energy,
                                   species.mass_eV_float, abs(species.num_elementary_charges_float), self.effect_length,
                                   self.bend_length, self.bend_angle, self.exit_distance, self.num_bins,
                                   self.cutoff_wavelength)

    @property
    def defining_features(self) -> list[str]:
        return self._with_cutoff(super().defining_features
                                 + ["effect_length", "bend_length", "bend_angle", "exit_distance", "num_bins"])
