"""The kicks of `cheetah_amd._ops` that bin the surviving particles' charge on M nodes in tau and kick every particle with what a sum
over the nodes gives at its node coordinate: the short-range wake (Wakefield: causal convolution with the sampled wake, kicks to
delta, px, py), the steady-state CSR (CSRKick: the anti-causal Toeplitz sum with the exactly integrated (z - z')^(-1/3) kernel), its
entrance transient (TransientCSRKick: the same sum with the table of the slippage length reached inside the bend), the CSR in the
drift behind a bend (CSRDriftKick: the same sum with the table of the radiation that left the bend and catches up) and the
longitudinal space charge (LSCKick: the two-sided Toeplitz sum with the on-axis field of a charged disc). Each is one
`chx_*_kick` call (four launches, five with a `cutoff_wavelength`: the Gaussian low-pass filter of the deposit between the deposit
and the node pass; deterministic, no host synchronisation) and an autograd node whose backward is `chx_*_kick_bwd`.
The CSR and LSC kicks form their per-row factors on the device from the energy and their further settings (length, angle, radius,
distance); they share one node. So does the intrabeam-scattering kick (IBSKick), whose node quantity is a variance V_k = K D_k / h:
every particle gets delta += sqrt(V(u)) xi with a deviate drawn inside the kernel (Philox4x32-10, as `_ops_sr`).

Part of `_ops` (which re-exports every name here). Imported at the END of `_ops`, whose helpers it uses."""
from __future__ import annotations

import math
from operator import attrgetter
from typing import Callable, NamedTuple

import torch

from . import _lib
from ._ops import MAX_GRID_ROWS, aligned, bshapes, check, dtype_code, flat_bcast, numel, ptr, require_device, stream_ptr, workspace

__all__ = ["WAKE_MAX_BINS", "CSR_MAX_BINS", "LSC_MAX_BINS", "WakeKick", "wake_kick", "wake_scale", "csr_kick", "csr_scale", "csr_transient_kick",
           "csr_transient_x", "csr_drift_kick", "csr_drift_factors", "lsc_kick", "lsc_scale_rho", "IBS_MAX_BINS", "ibs_kick",
           "ibs_strength", "ibs_g", "ibs_normals"]

#: CHX_WAKE_MAX_BINS of include/chx.h: the deposit's per-workgroup LDS histograms hold up to 3 channels of M 64-bit nodes; one grid
#: and one deposit for the three kicks
WAKE_MAX_BINS = CSR_MAX_BINS = LSC_MAX_BINS = IBS_MAX_BINS = 4096
#: k_e = 1 / (4 pi eps0), V m / C (chx_grid1d_dev.h)
_K_E = 8.9875517923e9
#: r_e (m), m_e c^2 (eV) and e (C), as csrc/chx_ibs.hip
_R_E = 2.8179403205e-15
_M_E = 510998.95069
_E_CHARGE = 1.602176634e-19


class _Kick(NamedTuple):
    """What the shared callers need to know about a kick; built once at import."""
    owner: str                  # the element's name in messages
    workspace: str              # C entry points
    forward: str
    backward: str
    state_doubles: tuple        # (s0, s1): s0 + s1 M doubles per batch row of the state the forward pass leaves for the backward pass
    cotangents: int             # per-row float64 cotangents the backward call returns (d_scale[, d_rho])
    factors: Callable | None    # (state, mass_eV, abs_z, *settings) -> the per-row factors, for the chain rule of the settings


def _kick(owner: str, tag: str, state_doubles, cotangents: int, factors=None) -> _Kick:
    return _Kick(owner, f"chx_{tag}_workspace_bytes", f"chx_{tag}_kick", f"chx_{tag}_kick_bwd", state_doubles, cotangents, factors)


_shape = attrgetter("shape")


def _rows(t: torch.Tensor, batch_shape, B: int, dtype):
    """A setting as flat rows of the beam's dtype: (1,) view of a single value (an in-place edit reaches the kernel) or (B,)."""
    t = t.to(dtype)
    if t.numel() == 1:
        return t.reshape(1)
    return t.expand(batch_shape).reshape(B).contiguous()


def _opt(t) -> tuple:
    """An optional tensor as the arguments it adds to a call: none, or itself."""
    return () if t is None else (t,)


# The low-pass filter every kick of this module takes as `cutoff_wavelength` (metres; None: the raw deposit), as include/chx.h states
# it. Per batch row, with h the row's node spacing: s = cutoff / (2 pi h), R = max(1, min(ceil(4 s), M - 1)), g_d = exp(-d^2 / 2 s^2)
# for |d| <= R, normalised to sum 1; D'_j = sum_d g_d D_refl(j - d) with the row mirrored about its ends (numpy's
# pad(mode="symmetric")). Amplitude response exp(-(cutoff / lambda)^2 / 2); the charge is kept; a constant of the kick (no gradient).


def _beam_rows(kick: _Kick, particles, charges, survival, *row_settings, others=()):
    """The beam as flat rows: x (Bx, N, 7) aligned, q (Bq, N), w (Bw, N) in the particles' dtype, and the batch shape (broadcast of
    the particles', charges', survival probabilities' and row settings' batch shapes) with its number of rows B. `others`: further
    tensors (or None) that must live on the device."""
    require_device(particles, charges, survival, *row_settings, *others)
    dt = particles.dtype
    batch_shape = bshapes(particles.shape[:-2], charges.shape[:-1], survival.shape[:-1], *map(_shape, row_settings))
    B = numel(batch_shape)
    if B > MAX_GRID_ROWS:
        raise ValueError(f"{kick.owner}: at most {MAX_GRID_ROWS} batch rows per kick, got {B}")
    x, _ = flat_bcast(particles, batch_shape, 2)
    q, _ = flat_bcast(charges.to(dt), batch_shape, 1)
    w, _ = flat_bcast(survival.to(dt), batch_shape, 1)
    return aligned(x), q.contiguous(), w.contiguous(), batch_shape, B


def _cutoff_rows(cutoff, batch_shape, B: int):
    """The cutoff wavelength as float64 rows, (1,) or (B,), or None. A constant of the kick: detached."""
    return None if cutoff is None else _rows(cutoff.detach(), batch_shape, B, torch.float64)


def _cut_call(kick: _Kick, name: str, cut, B: int, N: int, M: int, device):
    """(entry point, its arguments in front of the workspace, workspace, its bytes): the call itself without a cutoff, its twin and
    the twin's workspace with cutoff rows."""
    lib = _lib.lib()
    suffix, cut_args = ("", ()) if cut is None else ("_cut", (ptr(cut), cut.shape[0]))
    ws_bytes = getattr(lib, kick.workspace + suffix)(B, N, M)
    return getattr(lib, name + suffix), name + suffix, cut_args, workspace(ws_bytes, device), ws_bytes


def _kick_raw(kick: _Kick, x, q, w, head, tail, B: int, N: int, M: int, cut=None):
    """The forward entry point on flat inputs x (Bx, N, 7), q (Bq, N), w (Bw, N) -> (out (B, N, 7), state (B, state_doubles)
    float64), state_doubles = s0 + s1 M. `head`: the kick's own arguments between w and B, `tail`: those between Bw and N. `cut`:
    None, or the cutoff wavelengths of the low-pass filter of the deposit as float64 rows (1,) or (B,)."""
    call, name, cut_args, ws, ws_bytes = _cut_call(kick, kick.forward, cut, B, N, M, x.device)
    out = torch.empty((B, N, 7), dtype=x.dtype, device=x.device)
    state = torch.empty((B, kick.state_doubles[0] + kick.state_doubles[1] * M), dtype=torch.float64, device=x.device)
    check(call(ptr(x), ptr(q), ptr(w), *head, B, x.shape[0], q.shape[0], w.shape[0], *tail, N, M, dtype_code(x.dtype), ptr(out),
               ptr(state), *cut_args, ptr(ws), ws_bytes, stream_ptr()), name)
    return out, state


def _kick_bwd_raw(kick: _Kick, x, q, w, head, state, d_out, B: int, N: int, M: int, need_c: bool, extra=(), cut=None):
    """The backward entry point: (dX (B, N, 7), dC (B, N) | None, the per-row cotangents (B,) float64); rows of broadcast inputs not
    summed. `extra`: the kick's own gradient outputs (or None) behind the per-row cotangents. `cut`: as the forward call's."""
    kw = {"dtype": x.dtype, "device": x.device}
    dX = torch.empty((B, N, 7), **kw)
    dC = torch.empty((B, N), **kw) if need_c else None
    d_rows = [torch.empty((B,), dtype=torch.float64, device=x.device) for _ in range(kick.cotangents)]
    call, name, cut_args, ws, ws_bytes = _cut_call(kick, kick.backward, cut, B, N, M, x.device)
    check(call(ptr(x), ptr(q), ptr(w), *head, B, x.shape[0], q.shape[0], w.shape[0], N, M, dtype_code(x.dtype), ptr(state),
               ptr(d_out), ptr(dX), ptr(dC), *map(ptr, d_rows), *map(ptr, extra), *cut_args, ptr(ws), ws_bytes, stream_ptr()), name)
    return dX, dC, d_rows


def _beam_grads(dX, dC, x, q, w, B: int, need):
    """(dX, dq, dw) from the backward call's dX and dC (through c = |q| w), as `need`[0:3] asks, rows of broadcast inputs summed."""
    dq = dw = None
    if need[1]:
        dq = dC * w * torch.sign(q)
        if q.shape[0] == 1 and B > 1:
            dq = dq.sum(dim=0, keepdim=True)
    if need[2]:
        dw = dC * q.abs()
        if w.shape[0] == 1 and B > 1:
            dw = dw.sum(dim=0, keepdim=True)
    if need[0] and x.shape[0] == 1 and B > 1:
        dX = dX.sum(dim=0, keepdim=True)
    return (dX if need[0] else None), dq, dw


def _gamma_beta(energy: torch.Tensor, mass_eV: float):
    """(gamma, beta) of the reference energy in float64."""
    gamma = energy.to(torch.float64) / mass_eV
    beta = torch.where(gamma.abs() > 0, (1 - gamma.square().reciprocal()).clamp_min(0).sqrt(), torch.ones_like(gamma))
    return gamma, beta


def _p0c(energy: torch.Tensor, mass_eV: float) -> torch.Tensor:
    """p0c = beta gamma m c^2 of the reference energy in float64, as `Beam.p0c`."""
    gamma, beta = _gamma_beta(energy, mass_eV)
    return beta * gamma * mass_eV


# ---- the wake --------------------------------------------------------------------------------------------------------------------
_WAKE = _kick("Wakefield", "wake", (8, 6), 1)      # CHX_WAKE_STATE_DOUBLES


def _wake_head(scale, wl, wt, h):
    """scale (B,), wl, wt (L,) or None, h (1,), all float64."""
    return ptr(scale), ptr(wl), 0 if wl is None else wl.numel(), ptr(wt), 0 if wt is None else wt.numel(), ptr(h)


class WakeKick(torch.autograd.Function):
    """out (B, N, 7) = chx_wake_kick(x, q, w, scale, wl, wt); backward = chx_wake_kick_bwd: gradients of the particles, the charges
    and survival probabilities (through c = |q| w), the per-row scale factor |Z| / p0c and both tables (summed over the rows). The
    node grid (tau range), the wake spacing h and the cutoff rows `cut` (or None) are constants."""

    @staticmethod
    def forward(ctx, x, q, w, scale, wl, wt, h, B, M, cut=None):
        out, state = _kick_raw(_WAKE, x, q, w, _wake_head(scale, wl, wt, h), (), B, x.shape[1], M, cut)
        ctx.save_for_backward(x, q, w, scale, wl, wt, h, state, cut)
        ctx.B, ctx.M = B, M
        return out

    @staticmethod
    def backward(ctx, d_out):
        x, q, w, scale, wl, wt, h, state, cut = ctx.saved_tensors
        B, M, N = ctx.B, ctx.M, x.shape[1]
        need = ctx.needs_input_grad
        f64 = {"dtype": torch.float64, "device": x.device}
        d_wl = torch.empty((wl.numel(),), **f64) if need[4] and wl is not None else None
        d_wt = torch.empty((wt.numel(),), **f64) if need[5] and wt is not None else None
        dX, dC, (d_scale,) = _kick_bwd_raw(_WAKE, x, q, w, _wake_head(scale, wl, wt, h), state, d_out.contiguous().to(x.dtype), B, N, M,
                                           need[1] or need[2], (d_wl, d_wt), cut)
        return *_beam_grads(dX, dC, x, q, w, B, need), (d_scale if need[3] else None), d_wl, d_wt, None, None, None, None


def wake_scale(energy: torch.Tensor, mass_eV: float, abs_charge_number: float, factor: torch.Tensor) -> torch.Tensor:
    """factor |Z| / p0c in float64 (p0c as `Beam.p0c`), broadcast of the two shapes."""
    return factor.to(torch.float64) * abs_charge_number / _p0c(energy, mass_eV)


def wake_kick(particles: torch.Tensor, charges: torch.Tensor, survival: torch.Tensor, energy: torch.Tensor, mass_eV: float,
              abs_charge_number: float, factor: torch.Tensor, longitudinal_wake, transverse_wake, wake_spacing: torch.Tensor,
              num_bins: int, cutoff_wavelength: torch.Tensor | None = None) -> torch.Tensor:
    """The wake kick of a beam of any batch shape (broadcast of the particles', charges', survival probabilities', energy's,
    factor's and cutoff's batch shapes) -> particles (*batch, N, 7). `longitudinal_wake` / `transverse_wake`: 1-D tables (V/C,
    V/(C m)) or None; `wake_spacing`: 0-d tensor h (metres between table entries); `cutoff_wavelength`: None, or the cutoff (metres)
    of the Gaussian low-pass filter of the deposits Q, X, Y. Differentiable with respect to the particles, charges,
    survival probabilities, energy, factor and both tables."""
    x, q, w, batch_shape, B = _beam_rows(_WAKE, particles, charges, survival, energy, factor, *_opt(cutoff_wavelength),
                                         others=(wake_spacing, longitudinal_wake, transverse_wake))
    cut = _cutoff_rows(cutoff_wavelength, batch_shape, B)
    N = particles.shape[-2]
    scale = wake_scale(energy, mass_eV, abs_charge_number, factor).expand(batch_shape).reshape(B).contiguous()
    wl = None if longitudinal_wake is None else longitudinal_wake.to(torch.float64).contiguous()
    wt = None if transverse_wake is None else transverse_wake.to(torch.float64).contiguous()
    h = wake_spacing.detach().to(torch.float64).reshape(1)
    grads = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, q, w, scale, wl, wt))
    if grads:
        out = WakeKick.apply(x, q, w, scale, wl, wt, h, B, num_bins, *_opt(cut))
    else:
        out, _ = _kick_raw(_WAKE, x, q, w, _wake_head(scale, wl, wt, h), (), B, N, num_bins, cut)
    return out.reshape(*batch_shape, N, 7)


# ---- the kicks with per-row settings: CSR and LSC ------------------------------------------------------------------------------------
def _safe_pow(v: torch.Tensor, p: float) -> torch.Tensor:
    """v^p for v > 0, 0 at v = 0 with a zero gradient there (the kick is 0 at L = 0 or theta = 0), NaN for v < 0."""
    pos = v > 0
    r = torch.where(pos, v, torch.ones_like(v)).pow(p)
    return torch.where(pos, r, torch.where(v == 0, torch.zeros_like(v), torch.full_like(v, float("nan"))))


def csr_scale(energy: torch.Tensor, mass_eV: float, abs_charge_number: float, length: torch.Tensor,
              angle: torch.Tensor) -> torch.Tensor:
    """|Z| L^(1/3) |theta|^(2/3) / p0c in float64 (p0c as `Beam.p0c`), broadcast of the three shapes: the factor the kernels form on
    the device, restated here for the chain rule of the backward pass."""
    p0c = _p0c(energy, mass_eV)
    return abs_charge_number * _safe_pow(length.to(torch.float64), 1 / 3) * _safe_pow(angle.to(torch.float64).abs(), 2 / 3) / p0c


def lsc_scale_rho(energy: torch.Tensor, mass_eV: float, abs_charge_number: float, length: torch.Tensor, radius: torch.Tensor,
                  h: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(S, rho) = (|Z| 2 k_e L / (gamma^2 h^2 p0c), a / (gamma h)) in float64 (p0c as `Beam.p0c`), broadcast of the four shapes: the
    factors the kernels form on the device, restated here for the chain rule of the backward pass. `h` is the node spacing of the
    forward's state header, a constant; a row without a grid (h = 0) has S = 0 and a constant rho."""
    gamma, beta = _gamma_beta(energy, mass_eV)
    grid = h > 0
    hs = torch.where(grid, h, torch.ones_like(h))
    # p0c is formed here, behind gamma^2: autograd adds the energy's gradient contributions in the order the operations were
    # recorded, and that sum is not associative
    S = abs_charge_number * 2 * _K_E * length.to(torch.float64) / (gamma.square() * hs.square() * (beta * gamma * mass_eV))
    rho = radius.to(torch.float64) / (gamma * hs)
    return torch.where(grid, S, torch.zeros_like(S)), torch.where(grid, rho, torch.ones_like(rho))


def csr_transient_x(length: torch.Tensor, angle: torch.Tensor, distance: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """x = z_L / h = d^3 theta^2 / (24 L^2 h) in float64, broadcast of the four shapes: the slippage length an arc length d into the
    bend in node spacings, which the kernels form on the device, restated here for the chain rule of the backward pass. `h` is the
    node spacing of the forward's state header, a constant. Where L, theta or d is 0 or the row has no grid (h = 0) there is no
    kick: x = 0 with zero gradients."""
    L, th, d = (t.to(torch.float64) for t in (length, angle, distance))
    kicks = (L != 0) & (th != 0) & (d != 0) & (h > 0)
    one = torch.ones((), dtype=torch.float64, device=h.device)
    Ls, ds, hs = torch.where(kicks, L, one), torch.where(kicks, d, one), torch.where(kicks, h, one)
    x = ds.pow(3) * th.square() / (24 * Ls.square() * hs)
    x = torch.where((Ls > 0) & (ds > 0), x, torch.full_like(x, float("nan")))
    return torch.where(kicks, x, torch.zeros_like(x))


def csr_drift_factors(energy: torch.Tensor, mass_eV: float, abs_charge_number: float, length: torch.Tensor, bend_length: torch.Tensor,
                      bend_angle: torch.Tensor, distance: torch.Tensor, h: torch.Tensor):
    """(scale, xh, phi, kappa) = (|Z| L / p0c, x |theta| / L_b, |theta|, 24 h |theta| / L_b) in float64 (p0c as `Beam.p0c`), broadcast
    of the shapes: the scale and the three shape numbers of the CSR wake a distance x behind a bend of length L_b and angle theta,
    which the kernels form on the device, restated here for the chain rule of the backward pass. `h` is the node spacing of the
    forward's state header, a constant. Where L, L_b or theta is 0 or the row has no grid (h = 0) there is no kick: all four are 0
    with zero gradients."""
    L, Lb, th, d = (t.to(torch.float64) for t in (length, bend_length, bend_angle, distance))
    kicks = (L != 0) & (Lb != 0) & (th != 0) & (h > 0)
    one = torch.ones((), dtype=torch.float64, device=h.device)
    Ls, Lbs, hs = torch.where(kicks, L, one), torch.where(kicks, Lb, one), torch.where(kicks, h, one)
    phi = th.abs()
    nan = torch.full((), float("nan"), dtype=torch.float64, device=h.device)
    valid = (Ls > 0) & (Lbs > 0) & (d >= 0)
    zero = torch.zeros((), dtype=torch.float64, device=h.device)
    factors = (abs_charge_number * Ls / _p0c(energy, mass_eV), d * phi / Lbs, phi, 24 * hs * phi / Lbs)
    return tuple(torch.where(kicks, torch.where(valid, f, nan), zero) for f in factors)


def ibs_g(alpha: torch.Tensor) -> torch.Tensor:
    """Bane's g(alpha) = (2 sqrt(alpha) / pi) int_0^inf du / sqrt((1 + u^2)(alpha^2 + u^2)) in closed form, sqrt(alpha) / AGM(1, alpha),
    with exactly 8 steps of the arithmetic-geometric mean (a, b) <- ((a + b) / 2, sqrt(a b)), as the kernel forms it."""
    a, c = torch.ones_like(alpha), alpha
    for _ in range(8):
        a, c = 0.5 * (a + c), (a * c).sqrt()
    return alpha.sqrt() / a


def ibs_strength(energy: torch.Tensor, mass_eV: float, abs_z: float, length: torch.Tensor, coulomb_log: torch.Tensor,
                 sigma_x: torch.Tensor, sigma_y: torch.Tensor, eps_x: torch.Tensor, eps_y: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """K / h in float64, K = sqrt(pi) r_c^2 Lambda L g(alpha) / (4 gamma^3 sqrt(eps_x eps_y sigma_x sigma_y) |Z| e) with alpha =
    (sigma_x eps_y) / (sigma_y eps_x) and r_c = Z^2 r_e m_e / m, broadcast of the shapes: the factor between the deposits D_k (coulomb)
    and the node variances of delta that the kernels form on the device, restated here for the chain rule of the backward pass. `h`
    is the node spacing of the forward's state header, a constant; a row without a grid (h = 0) has the factor 0. A row in which
    Lambda, a size or an emittance is not > 0 or not finite has NaN."""
    gamma = energy.to(torch.float64) / mass_eV
    L, lam, sx, sy, ex, ey = (t.to(torch.float64) for t in (length, coulomb_log, sigma_x, sigma_y, eps_x, eps_y))
    ok = torch.ones((), dtype=torch.bool, device=h.device)
    for t in (lam, sx, sy, ex, ey):
        ok = ok & (t > 0) & torch.isfinite(t)
    one = torch.ones((), dtype=torch.float64, device=h.device)
    sx, sy, ex, ey = (torch.where(ok, t, one) for t in (sx, sy, ex, ey))
    rc = abs_z * abs_z * _R_E * _M_E / mass_eV
    g = ibs_g((sx * ey) / (sy * ex))
    K = math.sqrt(math.pi) * (rc * rc) * lam * L * g / (4.0 * (gamma * gamma * gamma) * (ex * ey * sx * sy).sqrt() * abs_z * _E_CHARGE)
    grid = h > 0
    Kh = K / torch.where(grid, h, torch.ones_like(h))
    Kh = torch.where(ok, Kh, torch.full_like(Kh, float("nan")))
    return torch.where(grid, Kh, torch.zeros_like(Kh))


_CSR = _kick("CSRKick", "csr", (8, 1), 1,                                           # CHX_CSR_STATE_DOUBLES
             lambda state, mass_eV, abs_z, e, L, a: (csr_scale(e, mass_eV, abs_z, L, a),))
_CSR_TRANSIENT = _kick("TransientCSRKick", "csr_transient", (8 + 2, 2), 2,          # CHX_CSR_TRANSIENT_STATE_DOUBLES
                       lambda state, mass_eV, abs_z, e, L, a, d: (csr_scale(e, mass_eV, abs_z, L, a),
                                                                  csr_transient_x(L, a, d, state[:, 2])))
_CSR_DRIFT = _kick("CSRDriftKick", "csr_drift", (8 + 4, 2), 4,                         # CHX_CSR_DRIFT_STATE_DOUBLES
                   lambda state, mass_eV, abs_z, e, L, Lb, a, d: csr_drift_factors(e, mass_eV, abs_z, L, Lb, a, d, state[:, 2]))
_LSC = _kick("LSCKick", "lsc", (8 + 2, 2), 2,                                       # CHX_LSC_STATE_DOUBLES
             lambda state, mass_eV, abs_z, e, L, a: lsc_scale_rho(e, mass_eV, abs_z, L, a, state[:, 2]))
_IBS = _kick("IBSKick", "ibs", (8, 2), 1,                                           # CHX_IBS_STATE_DOUBLES
             lambda state, mass_eV, abs_z, e, L, lam, sx, sy, ex, ey: (ibs_strength(e, mass_eV, abs_z, L, lam, sx, sy, ex, ey,
                                                                                    state[:, 2]),))


def _settings_args(settings, mass_eV: float, abs_z: float, rng=None):
    """(head, tail) of `_kick_raw`. `rng`: (seed, stream, call index) of a kick that draws, the call index a one-element int64 device
    tensor that the kernel reads."""
    key = () if rng is None else (rng[0], rng[1], ptr(rng[2]))
    return (*map(ptr, settings), mass_eV, abs_z, *key), tuple(t.shape[0] for t in settings)


class _SettingsKick(torch.autograd.Function):
    """out (B, N, 7) = chx_{csr,csr_transient,csr_drift,lsc,ibs}_kick(x, q, w, *settings): the energy e, the length L and the kick's further
    settings (angle, radius, distance, Coulomb logarithm, moments), each (1,) or (B,) in the beam dtype; backward = the kick's _bwd call: gradients of the
    particles, the charges and survival probabilities (through c = |q| w), and of the settings through the per-row cotangents of the
    kick's factors. The node grid (tau range) is a constant. `rng`: None, or (seed, stream, call index) of a kick that draws (IBS): the
    backward pass draws the same deviates again from a clone of the call index the forward pass used; the deviates are constants.
    `cut`: None, or the cutoff rows of the low-pass filter, a constant."""

    @staticmethod
    def forward(ctx, kick, mass_eV, abs_z, B, M, rng, cut, x, q, w, *settings):
        out, state = _kick_raw(kick, x, q, w, *_settings_args(settings, mass_eV, abs_z, rng), B, x.shape[1], M, cut)
        # the value this call used: the element advances its own buffer in place right after the kick
        call = () if rng is None else (rng[2].clone(),)
        ctx.save_for_backward(cut, x, q, w, state, *call, *settings)
        ctx.kick, ctx.B, ctx.M, ctx.mass_eV, ctx.abs_z = kick, B, M, mass_eV, abs_z
        ctx.key = None if rng is None else rng[:2]
        return out

    @staticmethod
    def backward(ctx, d_out):
        cut, x, q, w, state, *given = ctx.saved_tensors
        head = ()
        if ctx.key is not None:
            call, *given = given
            head = (*ctx.key, ptr(call))
        kick, B, M, N = ctx.kick, ctx.B, ctx.M, x.shape[1]
        need = ctx.needs_input_grad[7:]
        dX, dC, d_rows = _kick_bwd_raw(kick, x, q, w, head, state, d_out.contiguous().to(x.dtype), B, N, M, need[1] or need[2], cut=cut)
        settings = [None] * len(given)
        wanted = [i for i in range(len(given)) if need[3 + i]]
        if wanted:
            with torch.enable_grad():
                leaves = [t.detach().requires_grad_(need[3 + i]) for i, t in enumerate(given)]
                factors = kick.factors(state, ctx.mass_eV, ctx.abs_z, *leaves)
                # a factor need not see every setting (the LSC's S does not see the radius, its rho does not see L): only what
                # carries a graph goes into the chain rule
                outs = [(o.expand(B), d) for o, d in zip(factors, d_rows) if o.requires_grad]
                grads = torch.autograd.grad([o for o, _ in outs], [leaves[i] for i in wanted], [d for _, d in outs])
            for i, g in zip(wanted, grads):
                settings[i] = g.to(x.dtype)
        return None, None, None, None, None, None, None, *_beam_grads(dX, dC, x, q, w, B, need), *settings


def _settings_kick(kick: _Kick, particles, charges, survival, mass_eV, abs_charge_number, settings, num_bins, rng=None, cutoff=None):
    """`settings`: the energy, the length and the kick's further settings, in the order of the C entry point. `rng`: (seed, stream,
    call index) of a kick that draws. `cutoff`: None, or the cutoff wavelength of the low-pass filter of the deposit."""
    x, q, w, batch_shape, B = _beam_rows(kick, particles, charges, survival, *settings, *_opt(cutoff),
                                         others=() if rng is None else (rng[2],))
    cut = _cutoff_rows(cutoff, batch_shape, B)
    N = particles.shape[-2]
    rows = tuple(_rows(t, batch_shape, B, particles.dtype) for t in settings)
    grads = torch.is_grad_enabled() and any(t.requires_grad for t in (x, q, w, *rows))
    if grads:
        out = _SettingsKick.apply(kick, float(mass_eV), float(abs_charge_number), B, num_bins, rng, cut, x, q, w, *rows)
    else:
        out, _ = _kick_raw(kick, x, q, w, *_settings_args(rows, float(mass_eV), float(abs_charge_number), rng), B, N, num_bins, cut)
    return out.reshape(*batch_shape, N, 7)


def csr_kick(particles: torch.Tensor, charges: torch.Tensor, survival: torch.Tensor, energy: torch.Tensor, mass_eV: float,
             abs_charge_number: float, length: torch.Tensor, angle: torch.Tensor, num_bins: int,
             cutoff_wavelength: torch.Tensor | None = None) -> torch.Tensor:
    """The steady-state CSR kick of an arc of length `length` and bend angle `angle` on a beam of any batch shape (broadcast of the
    particles', charges', survival probabilities', energy's, length's and angle's batch shapes) -> particles (*batch, N, 7).
    Differentiable with respect to the particles, charges, survival probabilities, energy, length and angle.
    `cutoff_wavelength`: None, or the cutoff (metres) of the Gaussian low-pass
    filter of the deposit, a constant whose batch shape broadcasts as well."""
    return _settings_kick(_CSR, particles, charges, survival, mass_eV, abs_charge_number, (energy, length, angle), num_bins,
                          cutoff=cutoff_wavelength)


def csr_transient_kick(particles: torch.Tensor, charges: torch.Tensor, survival: torch.Tensor, energy: torch.Tensor, mass_eV: float,
                       abs_charge_number: float, length: torch.Tensor, angle: torch.Tensor, distance: torch.Tensor,
                       num_bins: int, cutoff_wavelength: torch.Tensor | None = None) -> torch.Tensor:
    """The CSR kick of an arc of length `length` and bend angle `angle` at the arc length `distance` behind the entrance face of a bend
    that follows a long straight (the entrance transient; the steady state for a large distance), on a beam of any batch shape
    (broadcast of the particles', charges', survival probabilities', energy's, length's, angle's and distance's batch shapes) ->
    particles (*batch, N, 7). Differentiable with respect to the particles, charges, survival probabilities, energy, length, angle
    and distance. `cutoff_wavelength`: None, or the cutoff (metres) of the Gaussian low-pass
    filter of the deposit, a constant whose batch shape broadcasts as well."""
    return _settings_kick(_CSR_TRANSIENT, particles, charges, survival, mass_eV, abs_charge_number,
                          (energy, length, angle, distance), num_bins, cutoff=cutoff_wavelength)


def csr_drift_kick(particles: torch.Tensor, charges: torch.Tensor, survival: torch.Tensor, energy: torch.Tensor, mass_eV: float,
                   abs_charge_number: float, length: torch.Tensor, bend_length: torch.Tensor, bend_angle: torch.Tensor,
                   distance: torch.Tensor, num_bins: int, cutoff_wavelength: torch.Tensor | None = None) -> torch.Tensor:
    """The CSR kick of a piece of drift of length `length` at the distance `distance` behind the exit face of a bend of arc length
    `bend_length` and angle `bend_angle` (the radiation emitted inside that bend catching up with the bunch), on a beam of any batch
    shape (broadcast of the particles', charges', survival probabilities', energy's and the four settings' batch shapes) ->
    particles (*batch, N, 7). Differentiable with respect to the particles, charges, survival probabilities, energy and the four
    settings. `cutoff_wavelength`: None, or the cutoff (metres) of the Gaussian low-pass
    filter of the deposit, a constant whose batch shape broadcasts as well."""
    return _settings_kick(_CSR_DRIFT, particles, charges, survival, mass_eV, abs_charge_number,
                          (energy, length, bend_length, bend_angle, distance), num_bins, cutoff=cutoff_wavelength)


def lsc_kick(particles: torch.Tensor, charges: torch.Tensor, survival: torch.Tensor, energy: torch.Tensor, mass_eV: float,
             abs_charge_number: float, length: torch.Tensor, radius: torch.Tensor, num_bins: int,
             cutoff_wavelength: torch.Tensor | None = None) -> torch.Tensor:
    """The longitudinal space-charge kick of a straight section of length `length` on a beam of disc radius `radius` and of any batch
    shape (broadcast of the particles', charges', survival probabilities', energy's, length's and radius' batch shapes) ->
    particles (*batch, N, 7). Differentiable with respect to the particles, charges, survival probabilities, energy, length and
    radius. `cutoff_wavelength`: None, or the cutoff (metres) of the Gaussian low-pass
    filter of the deposit, a constant whose batch shape broadcasts as well."""
    return _settings_kick(_LSC, particles, charges, survival, mass_eV, abs_charge_number, (energy, length, radius), num_bins,
                          cutoff=cutoff_wavelength)


def ibs_kick(particles: torch.Tensor, charges: torch.Tensor, survival: torch.Tensor, energy: torch.Tensor, mass_eV: float,
             abs_charge_number: float, length: torch.Tensor, coulomb_log: torch.Tensor, sigma_x: torch.Tensor, sigma_y: torch.Tensor,
             eps_x: torch.Tensor, eps_y: torch.Tensor, num_bins: int, seed: int, stream: int, call_index: torch.Tensor,
             cutoff_wavelength: torch.Tensor | None = None) -> torch.Tensor:
    """The intrabeam-scattering kick of a section of length `length` on a beam of rms sizes `sigma_x`, `sigma_y` and geometric
    emittances `eps_x`, `eps_y`, with the Coulomb logarithm `coulomb_log`, of any batch shape (broadcast of the particles', charges',
    survival probabilities', energy's and the six settings' batch shapes) -> particles (*batch, N, 7). `seed`, `stream`: the 32-bit
    halves of the generator's key; `call_index`: a one-element int64 device tensor, the upper half of its counter, which the kernel
    reads and the caller advances. Differentiable with respect to the particles, charges, survival probabilities, energy and the six
    settings; the deviates are constants. `cutoff_wavelength`: None, or the cutoff (metres) of the Gaussian low-pass
    filter of the deposit, a constant whose batch shape broadcasts as well."""
    if call_index.dtype != torch.int64 or call_index.numel() != 1:
        raise TypeError("ibs_kick: call_index must be a one-element int64 tensor")
    return _settings_kick(_IBS, particles, charges, survival, mass_eV, abs_charge_number,
                          (energy, length, coulomb_log, sigma_x, sigma_y, eps_x, eps_y), num_bins, (int(seed), int(stream), call_index),
                          cutoff=cutoff_wavelength)


def ibs_normals(seed: int, stream: int, call: int, B: int, N: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """The kick's draw for call index `call`: (words (B, N, 4) as int64 values 0 ... 2^32 - 1, xi (B, N) float64) — the raw
    Philox4x32-10 output for the counter (n, b + 2^31, call_lo, call_hi) and the standard normal deviate of every (batch row, particle)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("cheetah_amd draws on the GPU only (HIP kernels, no CPU fallback)")
    words = torch.empty((B, N, 4), dtype=torch.int32, device=device)
    xi = torch.empty((B, N), dtype=torch.float64, device=device)
    check(_lib.lib().chx_ibs_normals(int(seed), int(stream), int(call), B, N, ptr(words), ptr(xi), stream_ptr()), "chx_ibs_normals")
    return words.to(torch.int64) & 0xFFFFFFFF, xi
