"""Restatements shared by the beam-moment path tests (tests/test_gpu_moments_paths.py): seeded beams that are hard on a one-pass
moment sum, the reference's two-pass weighted statistics (utils/statistics.py:4-62: mean first, then the centred sum, divisor
W - W2 / W) in `np.longdouble`, the worst-case bound of a float64 sum of N terms taken in another order, and a float64 numpy
restatement of the device's shifted one-pass formulas. No GPU needed.

Layout of a moment row, as chx_moments writes it: [W, W2, mu(6), cov upper triangle (21)].

The bound. The kernels sum N float64 terms in some order about a provisional centre c (the weighted mean of the row's first
min(16, N) particles; particle 0 when those carry no weight or the mean is not finite). With d = x - c and u = 2^-52 a sum of N
terms t_n taken in any order is within N u sum |t_n| of the exact one, so
  W, W2     N u sum w,  N u sum w^2
  mu_j      N u sum w |d_j| / W + 2 spacing(|mu_j|)                 (the sum, then c + s / W rounded twice)
  cov_ij    N u (sum w |d_i d_j| + (sum w |d_i|) (sum w |d_j|) / W) / (W - W2 / W)
(the second term of cov_ij: the error of s_i and s_j in the re-centring s_i s_j / W). The bound is derived, not measured."""
import math

import numpy as np

LD = np.longdouble
LD_IS_EXTENDED = bool(np.finfo(LD).eps < 1e-18)
U = 2.0 ** -52
SIG = np.array([2e-4, 3e-5, 2e-4, 3e-5, 1e-4, 1e-3])          # as tests/golden/generate_golden_moment_outliers.py
HARD_BEAMS = ("dead_outlier_slot0", "alive_outlier_slot0", "dead_first_wave", "offset_beam", "weighted_tail")
BEAMS = ("plain_weighted",) + HARD_BEAMS
IU = np.triu_indices(6)                                         # (i, j) of the 21 covariance entries, in storage order
DIAG = [8 + int(np.flatnonzero((IU[0] == a) & (IU[1] == a))[0]) for a in range(6)]      # cov_aa within the 29-row
NP_DT = {"f32": np.float32, "f64": np.float64}


def beam(name: str, N: int, seed: int = 0):
    """(x (N, 7) float64, w (N,) float64) of the named beam at N particles: the cases of generate_golden_moment_outliers.py with
    the dead first wave scaled to N (its first min(64, N // 2) particles), and `plain_weighted` (uniform weights in (0, 1))."""
    rng = np.random.default_rng([77, BEAMS.index(name), N, seed])
    x = np.empty((N, 7))
    x[:, 6] = 1.0
    w = np.ones(N)
    if name == "offset_beam":
        x[:, :6] = rng.standard_normal((N, 6)) * 1e-7 + 0.3
    elif name == "weighted_tail":
        x[:, :6] = rng.standard_t(3, size=(N, 6)) * SIG
        w = 0.5 + 0.5 * np.sin(np.arange(N) * 0.01) ** 2
    else:
        x[:, :6] = rng.standard_normal((N, 6)) * SIG
    if name == "plain_weighted":
        w = 1.0 - rng.random(N)                                 # (0, 1]
    elif name == "dead_outlier_slot0":
        x[0, :6] += 1e8 * SIG
        w[0] = 0.0
    elif name == "alive_outlier_slot0":
        x[0, :6] -= 1e5 * SIG
    elif name == "dead_first_wave":
        k = min(64, N // 2)
        x[:k, :6] += 1e3 * SIG
        w[:k] = 0.0
    return x, w


def _sum(a):
    """Sum over the last axis of a longdouble array; without an extended longdouble, exactly rounded float64 sums instead."""
    if LD_IS_EXTENDED:
        return a.sum(axis=-1)
    flat = a.reshape(-1, a.shape[-1])
    return np.array([math.fsum(float(v) for v in row) for row in flat], dtype=LD).reshape(a.shape[:-1])


def _rows(x, w):
    """x (R, N, 7) -> float64 (R, N, 6); w (R, N) or None -> float64 (R, N) (unit weights)."""
    x = np.asarray(x)
    x64 = x[..., :6].astype(np.float64)
    w64 = np.ones(x64.shape[:2]) if w is None else np.broadcast_to(np.asarray(w).astype(np.float64), x64.shape[:2])
    return x64, w64


def degenerate(x, w):
    """Rows whose statistics have the divisor 0: at most one particle with a weight."""
    _, w64 = _rows(x, w)
    return (w64 != 0.0).sum(axis=-1) <= 1


def reference(x, w):
    """(R, 29) longdouble: the two-pass weighted statistics of the rows x (R, N, 7), w (R, N) or None, on the very values given
    (float32 rows convert exactly). Covariances of degenerate rows are NaN (0 / 0)."""
    x64, w64 = _rows(x, w)
    xl, wl = x64.astype(LD), w64.astype(LD)
    out = np.full((xl.shape[0], 29), np.nan, dtype=LD)
    with np.errstate(all="ignore"):
        W, W2 = _sum(wl), _sum(wl * wl)
        out[:, 0], out[:, 1] = W, W2
        mu = np.stack([_sum(wl * xl[..., j]) for j in range(6)], axis=-1) / W[:, None]
        out[:, 2:8] = mu
        d = xl - mu[:, None, :]
        cf = W - W2 / W
        for k, (i, j) in enumerate(zip(*IU)):
            out[:, 8 + k] = _sum(wl * d[..., i] * d[..., j]) / cf
    out[degenerate(x, w), 8:] = np.nan
    return out


def centre(x, w):
    """(R, 6) float64: the provisional centre of the one-pass sums, the arithmetic of the kernels restated in float64."""
    x64, w64 = _rows(x, w)
    k = min(16, x64.shape[1])
    ww = w64[:, :k]
    with np.errstate(all="ignore"):
        Wk = ww.sum(axis=-1)
        inv = 1.0 / Wk
        m = (ww[..., None] * x64[:, :k]).sum(axis=1) * inv[:, None]
    return np.where((Wk > 0.0)[:, None] & np.isfinite(m), m, x64[:, 0])


def bounds(x, w, ref):
    """(R, 29) float64: the bound of every entry (module docstring) about `centre(x, w)`, for the reference values `ref`."""
    x64, w64 = _rows(x, w)
    N = x64.shape[1]
    d = np.abs(x64 - centre(x, w)[:, None, :])
    out = np.empty((x64.shape[0], 29))
    with np.errstate(all="ignore"):
        W, W2 = w64.sum(axis=-1), (w64 * w64).sum(axis=-1)
        cf = W - W2 / W
        s = (w64[..., None] * d).sum(axis=1)
        out[:, 0], out[:, 1] = N * U * W, N * U * W2
        out[:, 2:8] = N * U * s / W[:, None] + 2.0 * np.spacing(np.abs(ref[:, 2:8].astype(np.float64)))
        for k, (i, j) in enumerate(zip(*IU)):
            out[:, 8 + k] = N * U * ((w64 * d[..., i] * d[..., j]).sum(axis=-1) + s[:, i] * s[:, j] / W) / cf
    return out


def onepass(x, w, order=None, divisor="sums"):
    """(R, 29) float64: the shifted one-pass formulas of chx_moments in numpy float64, the particles taken in `order`:
    sums about c, then mu = c + s / W, cov = (m - W (s_i / W) (s_j / W)) / cf. A row of ONE particle has no order of
    summation: there this is the device's arithmetic operation by operation.
    divisor: "sums" -> cf = W - W2 / W (the one-pass kernel's finalize step); "pairs" -> cf = 2 (sum of w_n w_m over n < m) / W,
    the same number without the cancellation (the wave-per-row kernel)."""
    x64, w64 = _rows(x, w)
    c = centre(x, w)
    if order is not None:
        x64, w64 = x64[:, order], w64[:, order]
    out = np.empty((x64.shape[0], 29))
    with np.errstate(all="ignore"):
        d = x64 - c[:, None, :]
        W, W2 = w64.sum(axis=-1), (w64 * w64).sum(axis=-1)
        out[:, 0], out[:, 1] = W, W2
        wd = w64[..., None] * d
        m = wd.sum(axis=1) / W[:, None]
        out[:, 2:8] = c + m
        if divisor == "pairs":
            before, pairs = np.zeros_like(W), np.zeros_like(W)
            for n in range(w64.shape[1]):
                pairs = pairs + w64[:, n] * before
                before = before + w64[:, n]
            cf = (2.0 * pairs) / W
        else:
            assert divisor == "sums"
            cf = W - W2 / W
        for k, (i, j) in enumerate(zip(*IU)):
            out[:, 8 + k] = ((wd[..., i] * d[..., j]).sum(axis=-1) - W * m[:, i] * m[:, j]) / cf
    return out


def check_caps(ref, bnd, cap_cov, label=""):
    """The caps that keep the bound from hiding a failure, on the reference alone: bound_cov_ij <= cap_cov sigma_i sigma_j (per row:
    1e-6, and 1e-3 for `dead_first_wave`, whose centre is particle 0, 1e3 sigma off) and bound_mu_j <= 1e-6 sigma_j."""
    sig = np.sqrt(ref[:, DIAG].astype(np.float64))
    cap_cov = np.broadcast_to(np.asarray(cap_cov, dtype=np.float64), (ref.shape[0],))
    rel_cov = bnd[:, 8:] / (sig[:, IU[0]] * sig[:, IU[1]])
    rel_mu = bnd[:, 2:8] / sig
    assert np.isfinite(rel_cov).all() and (rel_cov <= cap_cov[:, None]).all(), (label, float(rel_cov.max()))
    assert np.isfinite(rel_mu).all() and (rel_mu <= 1e-6).all(), (label, float(rel_mu.max()))
    return float(rel_cov.max()), float(rel_mu.max())


def error_over_bound(got, ref, bnd):
    """|got - ref| / bound entry by entry (float64); 0 where both the error and the bound are 0, inf where got is not finite."""
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(LD) - ref).astype(np.float64)
        ratio = np.where(err == 0.0, 0.0, err / bnd)
    return np.where(np.isfinite(ratio), ratio, np.inf)


def check_rows(got, x, w, cap_cov=1e-6, label="", divisor="sums"):
    """Device rows `got` (R, 29) float64 against the reference of x (R, N, 7), w (R, N) or None -> the largest error / bound.
    Ordinary rows: the caps hold and every entry is within its bound. Degenerate rows (one particle, or no weight at all): W and
    W2 within bounds, mu within bounds where the row has weight, every other entry NaN exactly where `onepass` is NaN and equal
    to it elsewhere (no sum of more than one term enters such an entry in the rows this file builds)."""
    ref = reference(x, w)
    bnd = bounds(x, w, ref)
    deg = degenerate(x, w)
    assert got.shape == ref.shape and got.dtype == np.float64, (label, got.shape, got.dtype)
    worst = 0.0
    if (~deg).any():
        caps = np.broadcast_to(np.asarray(cap_cov, dtype=np.float64), deg.shape)[~deg]
        check_caps(ref[~deg], bnd[~deg], caps, label)
        ratio = error_over_bound(got[~deg], ref[~deg], bnd[~deg])
        worst = float(ratio.max())
        assert worst <= 1.0, (label, worst, np.argwhere(ratio > 1.0)[:8].tolist())
    if deg.any():
        g, r, b = got[deg], ref[deg], bnd[deg]
        rest = onepass(x, w, divisor=divisor)[deg]
        ratio = error_over_bound(g[:, :2], r[:, :2], b[:, :2])
        assert float(ratio.max()) <= 1.0, (label, "W, W2 of a degenerate row", float(ratio.max()))
        assert (np.isnan(g[:, 2:]) == np.isnan(rest[:, 2:])).all(), (label, "NaN positions of a degenerate row", g, rest)
        live = r[:, 0] > 0
        if live.any():
            ratio_mu = error_over_bound(g[live, 2:8], r[live, 2:8], b[live, 2:8])
            assert float(ratio_mu.max()) <= 1.0, (label, "mu of a one-particle row", float(ratio_mu.max()))
            ratio = np.concatenate([ratio.ravel(), ratio_mu.ravel()])
        same = np.isnan(rest[:, 8:]) | (g[:, 8:] == rest[:, 8:])
        assert same.all(), (label, "cov of a degenerate row", g[:, 8:], rest[:, 8:])
        worst = max(worst, float(ratio.max()))
    return worst
