"""Restatements shared by the quiet-start and density-modulation tests: the Halton sequence in numpy `uint64` arithmetic, and the
seeded density modulation (safeguarded Newton, the phase in turns) in float64 torch. No GPU needed."""
import math

import numpy as np
import torch

F64 = torch.float64
TWO_PI = 2 * math.pi
QUIET_BASES = (5, 7, 11, 13, 2, 3)              # the columns (x, px, y, py, tau, p) of a quiet-start beam
PRIMES = (2, 3, 5, 7, 11, 13, 17, 19)
ITERATIONS = 32                                  # the solver's cap


def radical_inverse(index, base: int) -> np.ndarray:
    """u = r / p of the indices (array of uint64) in `base`: the digits peeled off in unsigned 64-bit integers, r = r b + digit and
    p = p b per digit, then ONE float64 division (r, p < 2^53 for index < 2^40 and base <= 19: both conversions are exact)."""
    i = np.asarray(index, dtype=np.uint64).copy()
    b = np.uint64(base)
    r = np.zeros_like(i)
    p = np.ones_like(i)
    while bool((i > 0).any()):
        on = i > 0
        q = i // b
        r = np.where(on, r * b + (i - q * b), r)
        p = np.where(on, p * b, p)
        i = q
    assert int(p.max()) < 2**53 and int(r.max()) < 2**53
    return r.astype(np.float64) / p.astype(np.float64)


def halton(n: int, bases, offset: int = 0) -> np.ndarray:
    """(n, len(bases)) float64: row r has the index offset + 1 + r."""
    idx = np.arange(n, dtype=np.uint64) + np.uint64(offset + 1)
    return np.stack([radical_inverse(idx, b) for b in bases], axis=1)


def modulation_phase(t, nu, phit):
    """(sin, cos) of the modes' phases at t (…, N) for nu, phit (…, K) -> (…, N, K); in turns: w = fl(fl(t nu) + phi_t),
    f = w - rint(w) (torch rounds the product and the sum separately, and `round` is to even)."""
    w = t[..., None] * nu[..., None, :] + phit[..., None, :]
    f = w - torch.round(w)
    return torch.sin(TWO_PI * f), torch.cos(TWO_PI * f)


def modulate_tau(tau, amplitudes, wavelengths, phases, iterations: int = ITERATIONS):
    """tau' (…, N) float64 with tau' + sum_m A_m / (2 pi nu_m) sin(2 pi (tau' nu_m + phi_t,m)) = tau, the kernel's solver restated:
    at most `iterations` steps from t = tau; the bracket [lo, hi] from tau -+ sum |c_m| takes t on the side of the sign of g; the
    step is Newton's where it stays inside the bracket, the bracket's middle otherwise; a particle is done after a Newton step no
    longer than 2^-30 of the row's shortest wavelength. Settings (…, K) float64; differentiable."""
    A, nu, phit = amplitudes.to(F64), 1 / wavelengths.to(F64), phases.to(F64) / TWO_PI
    c = A / (TWO_PI * nu)
    tau = tau.to(F64)

    def evaluate(t):
        s, co = modulation_phase(t, nu, phit)
        gt, D = t, torch.ones_like(t)
        for m in range(A.shape[-1]):                       # the modes added in order, as the kernel adds them
            gt = gt + c[..., None, m] * s[..., m]
            D = D + A[..., None, m] * co[..., m]
        return gt - tau, D

    with torch.no_grad():
        W = c.abs().sum(-1, keepdim=True)
        tol = 2.0 ** -30 / nu.abs().max(dim=-1, keepdim=True).values
        lo, hi, t = tau - W, tau + W, tau + torch.zeros_like(W)
        done = torch.zeros_like(t, dtype=torch.bool)
        for _ in range(iterations):
            g, D = evaluate(t)
            lo, hi = torch.where(g < 0, t, lo), torch.where(g < 0, hi, t)      # (of a particle that is done: no longer read)
            tn = t - g / D
            inside = (tn >= lo) & (tn <= hi)
            tn = torch.where(inside, tn, 0.5 * (lo + hi))
            stop = inside & ((tn - t).abs() <= tol)
            t = torch.where(done, t, tn)
            done = done | stop
    if not (torch.is_grad_enabled() and any(v.requires_grad for v in (tau, A, nu, phit))):
        return t
    # The derivative is the implicit function's: one more Newton step from the root, through which autograd goes (g = 0 there, so
    # d(t - g / D) = -dg / D); the value stays the solver's. Autograd through the steps themselves would lose the particles whose
    # last step is the bracket's middle, which carries no graph.
    g, D = evaluate(t)
    step = t - g / D
    return t + (step - step.detach())


def modulation_residual(tau_out, tau_in, amplitudes, wavelengths, phases):
    """|tau' + sum c_m sin(theta_m) - tau| in units of the shortest wavelength of the row, (…, N) float64."""
    A, nu, phit = amplitudes.to(F64), 1 / wavelengths.to(F64), phases.to(F64) / TWO_PI
    s, _ = modulation_phase(tau_out.to(F64), nu, phit)
    g = tau_out.to(F64) + (A / (TWO_PI * nu))[..., None, :].mul(s).sum(-1) - tau_in.to(F64)
    return g.abs() * nu.max(dim=-1, keepdim=True).values
