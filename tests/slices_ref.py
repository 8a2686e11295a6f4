"""Restatements shared by the slice-statistics path tests (tests/test_slices_ref_host.py, tests/test_gpu_slice_paths.py): beams
built so that every launch of csrc/chx_slices.hip meets the sizes at which its indexing changes, the per-slice two-pass weighted
statistics (utils/statistics.py:4-62: mean first, then the centred sum, divisor W - W2 / W) in `np.longdouble`, a derived
worst-case bound for the arithmetic the kernels perform, a float64 numpy restatement of that arithmetic, and a differentiable
torch restatement for the gradients. No GPU needed.

Layout of a slice's row, as chx_slice_moments writes it: [W, W2, mu(6), cov upper triangle (21)] (float64), and the charge
Q = sum q w beside it. The constants of the kernels: tiles of 1024 particles in the ranking pass (kSliceTile), pieces of at most
1024 sorted particles in the reduction (kPiece), workgroups of 256 threads (CHX_BLOCK), at most 2048 slices (CHX_SLICES_MAX).

Membership is torch.histogram's with explicit edges, evaluated in the beam's dtype (`membership`).

Patterned beams (`patterned`). Coordinates 0-3 and 5 are integers in [-2^20, 2^20), tau = k + m / 1024 with m in 1 ... 1023
(exact in float32 for k < 2048, never on an edge, distinct inside a slice of fewer than 1024 particles so that no slice of two
has a variance of 0), edges 0 ... S, weights from {1, 1/2, 1/4, 1/8, 0}, charges from {1, 2, 4}. Every value is exact in float32:
both dtypes see the same numbers, and W, W2 and sum q w are sums of multiples of 1/64 below 2^53: exact in ANY order of summation.
They are asserted with ==.

The bound. With u = 2^-52, a float64 sum of n terms t taken in any order is within n u sum |t| of the exact one. The kernels
sum, per piece of a slice (n_p <= 1024 members, in the order of a fixed tree), w, w^2, q w and the UNCENTRED w x_j; divide for the
piece mean; sum w (x_i - m_i)(x_j - m_j) about that rounded mean m; and merge the pieces in order (Chan et al.), leaving out
pieces without weight. With n the member count of the slice (weightless members included: they are terms of the sums):
  W, W2, Q  n u sum |t|
  mu_j      n u sum w |x_j| / W + 2 spacing(|mu_j|)          (the sums of all pieces hold n terms; the quotient, the product
                                                             W_p m_p and the last quotient are rounded)
  cov_ij    n u sum w |d_i d_j| / cf                         (the centred sums, d = x - mu)
            + W b_i b_j / cf                                 (a centre off by e adds W e_i e_j exactly: sum w d = 0 removes the
                                                             first order; b is the bound of mu above)
            + c u (W + 2 W2 / W) / cf |cov_ij|               (the DIVISOR term, kept apart: cf = W - W2 / W is formed as that
                                                             difference, and cancels when one weight dominates)
The divisor term is the error of W - W2 / W relative to what the subtraction leaves: the rounding of the quotient and of the
difference (c = 1: all there is when W and W2 are exact, as in the patterned beams, and the whole of it at n = 2), and for weights
that do not sum exactly the errors n u W and n u W2 of the two sums themselves, which the cancellation amplifies in the same way
(c = n: d cf = dW (1 + W2 / W^2) + dW2 / W; a float64 numpy restatement of the scheme leaves the c = 1 term by a factor 3 on one
weight of 1 among a thousand of 1e-6). It is the cancellation profiles/moments_paths.md documents for chx_moments at N = 2, and
it is part of the arithmetic (a correct kernel can be off by it), so `compare` asserts base + divisor and reports the error over
the base bound beside it: a ratio above 1 against the base alone is attributed to the divisor. `check_caps` holds the BASE bound (the divisor term left out) against the reference alone:
bound_mu <= 1e-6 sigma and bound_cov <= 1e-6 sigma_i sigma_j in every slice with at least two weighted particles.
A slice merged from several pieces has one more term, first order in the errors e_p of its piece means: sum_p W_p D_p,i e_p,j
(D_p the distance of a piece mean from the slice mean). The multi-piece slices of these tests are patterned: their first-moment
sums are exact, e_p is one rounding of a quotient, and the term is below u / 2 |mu_j| sum w |d_i| / cf, orders under the first
line at n > 1024. It is left out; a real-valued slice of several pieces far off its centroid would need it.
The bound is derived, not measured."""
import dataclasses
import functools
import math

import numpy as np
import torch

from tests import moments_ref as mr

LD, U, IU, DIAG = mr.LD, mr.U, mr.IU, mr.DIAG
TILE = 1024                      # kSliceTile
PIECE = 1024                     # kPiece
ORDERS = ("ascending", "descending", "shuffled", "round_robin")
HARD = ("offset_centroid", "uneven_pairs", "heavy_and_light")
PIECE_COUNTS = (1024, 1025, 0, 1, 2048, 2049, 1023, 2, 3073)
#: the three weightless-piece cases: slice -> which of its members (in particle order) carry no weight
DEAD_SETS = {"first_piece_of_2049": {5: slice(0, 1024)}, "all_but_last_of_3073": {8: slice(0, 3072)}, "all_of_1025": {1: slice(None)}}


def membership(tau: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """torch.histogram / ATen histogramdd with explicit edges: upper_bound - 1, tau == e_S in the last slice, outside / NaN -> -1.
    tau (N,) and edges (S + 1,) in the beam's dtype."""
    S = edges.shape[-1] - 1
    k = torch.bucketize(tau, edges, right=True) - 1
    k = torch.where(tau == edges[-1], torch.full_like(k, S - 1), k)
    bad = torch.isnan(tau) | (tau < edges[0]) | (tau > edges[-1])
    return torch.where(bad, torch.full_like(k, -1), k)


@dataclasses.dataclass
class Beam:
    """One row: x (N, 7), w (N,), q (N,) float64 arrays of values exact in float32, k (N,) the prescribed slice (-1: none),
    edges (S + 1,) float64."""
    x: np.ndarray
    w: np.ndarray
    q: np.ndarray
    k: np.ndarray
    edges: np.ndarray

    @property
    def S(self):
        return self.edges.shape[0] - 1

    @property
    def N(self):
        return self.x.shape[0]


def _order(counts, order, rng):
    S = counts.shape[0]
    sorted_k = np.repeat(np.arange(S, dtype=np.int64), counts)
    if order == "ascending":
        return sorted_k
    if order == "descending":
        return sorted_k[::-1].copy()
    if order == "shuffled":
        return rng.permutation(sorted_k)
    assert order == "round_robin", order
    # particle n takes the next slice, cyclically, that still has room: round r visits the slices with more than r members
    rank = np.arange(sorted_k.shape[0]) - np.repeat(np.cumsum(counts) - counts, counts)
    return sorted_k[np.lexsort((sorted_k, rank))]


def patterned(counts, order, seed, dead=None) -> Beam:
    """The patterned beam (module docstring) with `counts[k]` particles in slice k, laid out in `order`; `dead` {slice: selector
    of its members in particle order} sets those members' weights to 0."""
    counts = np.asarray(counts, dtype=np.int64)
    S, N = counts.shape[0], int(counts.sum())
    assert 1 <= S <= 2048 and N >= 1
    rng = np.random.default_rng([2048, seed])
    k = _order(counts, order, rng)
    x = np.empty((N, 7))
    x[:, [0, 1, 2, 3, 5]] = rng.integers(-2 ** 20, 2 ** 20, size=(N, 5))
    x[:, 6] = 1.0
    m = rng.integers(1, 1024, size=N)
    by_slice = np.argsort(k, kind="stable")
    start = np.cumsum(counts) - counts
    for s in np.flatnonzero((counts >= 2) & (counts < 1024)):
        m[by_slice[start[s]:start[s] + counts[s]]] = 1 + rng.permutation(1023)[:counts[s]]
    x[:, 4] = k + m / 1024.0
    w = rng.choice(np.array([1.0, 0.5, 0.25, 0.125, 0.0]), size=N, p=[0.3, 0.2, 0.2, 0.2, 0.1])
    q = rng.choice(np.array([1.0, 2.0, 4.0]), size=N)
    for s, sel in (dead or {}).items():
        w[by_slice[start[s]:start[s] + counts[s]][sel]] = 0.0
    return Beam(x, w, q, k, np.arange(S + 1, dtype=np.float64))


def outside(beam: Beam, idx, kind) -> Beam:
    """The beam with the particles `idx` taken out of every slice: tau NaN ("nan"), below e_0 ("below"), above e_S ("above"), or
    the three in turn ("mixed")."""
    idx = np.arange(beam.N)[idx]
    x, k = beam.x.copy(), beam.k.copy()
    values = {"nan": np.nan, "below": -0.5, "above": beam.S + 0.5}
    if kind == "mixed":
        x[idx, 4] = np.array([values[n] for n in ("nan", "below", "above")])[np.arange(idx.shape[0]) % 3]
    else:
        x[idx, 4] = values[kind]
    k[idx] = -1
    return Beam(x, beam.w, beam.q, k, beam.edges)


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def hard(name, seed=0) -> Beam:
    """Real-valued beams (rounded to float32, so both dtypes see the same numbers) of S = 8 slices with edges 0 ... 8:
    offset_centroid   3000 particles, every slice's mean 1e3 sigma off in x and in delta
    uneven_pairs      slices 0-2 hold two particles with weight ratios 1e-3, 1e-6, 1e-8, slices 3-5 three particles (1, r, r) with
                      the same ratios, slices 6 and 7 share 2985 particles with weights in (0, 1]
    heavy_and_light   slices 0, 1, 2 hold one weight of 1 among a thousand of 1e-6; slices 3-7 are empty"""
    S = 8
    rng = np.random.default_rng([4096, HARD.index(name), seed])
    if name == "offset_centroid":
        counts = rng.multinomial(3000, np.full(S, 1.0 / S))
    elif name == "uneven_pairs":
        counts = np.array([2, 2, 2, 3, 3, 3, 1400, 1585])
    else:
        counts = np.array([1001, 1001, 1001, 0, 0, 0, 0, 0])
    N = int(counts.sum())
    k = rng.permutation(np.repeat(np.arange(S, dtype=np.int64), counts))
    x = np.empty((N, 7))
    x[:, :6] = rng.standard_normal((N, 6)) * mr.SIG
    x[:, 6] = 1.0
    x[:, 4] = k + 0.05 + 0.9 * rng.random(N)
    w = 1.0 - rng.random(N)
    if name == "offset_centroid":
        x[:, 0] += 1e3 * mr.SIG[0]
        x[:, 5] -= 1e3 * mr.SIG[5]
    elif name == "uneven_pairs":
        for s, r in zip(range(6), (1e-3, 1e-6, 1e-8) * 2):
            members = np.flatnonzero(k == s)
            w[members] = r
            w[members[0]] = 1.0
    elif name == "heavy_and_light":
        w[:] = 1e-6
        for s in range(3):
            w[np.flatnonzero(k == s)[s * 400]] = 1.0          # the heavy particle early, in the middle, late in its slice
    x[:, :6] = _f32(x[:, :6])
    assert (np.floor(x[:, 4]) == k).all()
    q = _f32(1e-15 * (1.0 + rng.random(N)))
    return Beam(x, _f32(w), q, k, np.arange(S + 1, dtype=np.float64))


# ---------------------------------------------------------------------------------------------------------------- reference
def _seg_sum(v, k, S):
    """Per-slice sums of the members' values v (n,) or (n, c) longdouble; without an extended longdouble, exactly rounded sums."""
    out = np.zeros((S,) + v.shape[1:], dtype=LD)
    if mr.LD_IS_EXTENDED:
        np.add.at(out, k, v)
        return out
    v2 = v.reshape(v.shape[0], -1)
    o2 = out.reshape(S, -1)
    for s in range(S):
        rows = v2[k == s]
        for c in range(v2.shape[1]):
            o2[s, c] = math.fsum(float(t) for t in rows[:, c])
    return out


def weighted_members(w, k, S):
    """(S,) the number of members of every slice with a weight other than 0."""
    m = (k >= 0) & (w != 0.0)
    return np.bincount(k[m], minlength=S)


def reference(x, w, q, k, S):
    """((S, 29) moments, (S,) charge) in longdouble: the two-pass weighted statistics of every slice on the very values given.
    Means of a slice without weight and covariances of a slice with at most one weighted particle are NaN (0 / 0)."""
    m = k >= 0
    kk = k[m]
    xl, wl, ql = x[m, :6].astype(LD), w[m].astype(LD), q[m].astype(LD)
    out = np.full((S, 29), np.nan, dtype=LD)
    with np.errstate(all="ignore"):
        W, W2 = _seg_sum(wl, kk, S), _seg_sum(wl * wl, kk, S)
        out[:, 0], out[:, 1] = W, W2
        charge = _seg_sum(ql * wl, kk, S)
        mu = _seg_sum(wl[:, None] * xl, kk, S) / W[:, None]
        out[:, 2:8] = mu
        d = xl - mu[kk]
        cf = W - W2 / W
        out[:, 8:] = _seg_sum(wl[:, None] * d[:, IU[0]] * d[:, IU[1]], kk, S) / cf[:, None]
    nw = weighted_members(w, k, S)
    out[nw == 0, 2:8] = np.nan
    out[nw <= 1, 8:] = np.nan
    return out, charge


@dataclasses.dataclass
class Bounds:
    mom: np.ndarray            # (S, 29) the base bound of every entry
    charge: np.ndarray         # (S,)
    divisor: np.ndarray        # (S, 29) the divisor term (covariances only)


def bounds(x, w, q, k, S, ref, exact_sums=False) -> Bounds:
    """The bound of every entry (module docstring) for the reference moments `ref` (S, 29); `exact_sums`: W and W2 are exact in any
    order of summation (c = 1 in the divisor term)."""
    m = k >= 0
    kk = k[m]
    x64, w64, q64 = x[m, :6].astype(np.float64), w[m].astype(np.float64), q[m].astype(np.float64)

    def seg(v):
        return np.bincount(kk, weights=v, minlength=S)

    n = np.bincount(kk, minlength=S).astype(np.float64)
    r64 = ref.astype(np.float64)
    mom, div = np.zeros((S, 29)), np.zeros((S, 29))
    with np.errstate(all="ignore"):
        W, W2 = seg(w64), seg(w64 * w64)
        cf = W - W2 / W
        mom[:, 0], mom[:, 1] = n * U * W, n * U * W2
        charge = n * U * seg(np.abs(q64 * w64))
        for j in range(6):
            mom[:, 2 + j] = n * U * seg(w64 * np.abs(x64[:, j])) / W + 2.0 * np.spacing(np.abs(r64[:, 2 + j]))
        d = np.abs(x64 - np.nan_to_num(r64[:, 2:8])[kk])
        for t, (i, j) in enumerate(zip(*IU)):
            mom[:, 8 + t] = (n * U * seg(w64 * d[:, i] * d[:, j]) + W * mom[:, 2 + i] * mom[:, 2 + j]) / cf
        c = 1.0 if exact_sums else np.maximum(n, 1.0)
        div[:, 8:] = (c * U * (W + 2.0 * W2 / W) / cf)[:, None] * np.abs(r64[:, 8:])
    return Bounds(mom, charge, div)


def check_caps(ref, bnd: Bounds, nw, label=""):
    """The caps that keep the bound from hiding a failure, on the reference alone and with the divisor term left out: in every
    slice with at least two weighted particles bound_mu_j <= 1e-6 sigma_j and bound_cov_ij <= 1e-6 sigma_i sigma_j.
    -> (largest bound_cov / sigma sigma, largest bound_mu / sigma, largest divisor term / sigma sigma)."""
    rows = nw >= 2
    if not rows.any():
        return 0.0, 0.0, 0.0
    sig = np.sqrt(ref[rows][:, DIAG].astype(np.float64))
    rel_cov = bnd.mom[rows, 8:] / (sig[:, IU[0]] * sig[:, IU[1]])
    rel_mu = bnd.mom[rows, 2:8] / sig
    rel_div = bnd.divisor[rows, 8:] / (sig[:, IU[0]] * sig[:, IU[1]])
    assert np.isfinite(rel_cov).all() and (rel_cov <= 1e-6).all(), (label, "cov", float(np.nanmax(rel_cov)))
    assert np.isfinite(rel_mu).all() and (rel_mu <= 1e-6).all(), (label, "mu", float(np.nanmax(rel_mu)))
    return float(rel_cov.max()), float(rel_mu.max()), float(rel_div.max())


@dataclasses.dataclass
class Case:
    """A beam with its reference, bounds and caps (computed once, shared by the dtypes and the tests that use the case)."""
    label: str
    beam: Beam
    exact: bool
    ref: np.ndarray = None
    ref_q: np.ndarray = None
    bnd: Bounds = None
    nw: np.ndarray = None
    caps: tuple = None

    def __post_init__(self):
        b = self.beam
        self.ref, self.ref_q = reference(b.x, b.w, b.q, b.k, b.S)
        self.bnd = bounds(b.x, b.w, b.q, b.k, b.S, self.ref, self.exact)
        self.nw = weighted_members(b.w, b.k, b.S)
        self.caps = check_caps(self.ref, self.bnd, self.nw, self.label)


@dataclasses.dataclass
class Worst:
    ratio: float = 0.0         # largest error / (base + divisor term): asserted <= 1
    base: float = 0.0          # largest error / base bound (above 1 only through the divisor term)

    def merge(self, other):
        self.ratio, self.base = max(self.ratio, other.ratio), max(self.base, other.base)
        return self


def compare(got_m, got_q, case: Case) -> Worst:
    """Moments (S, 29) and charge (S,) float64 of some implementation against the case's reference. Exact cases (patterned):
    W, W2 and the charge are EQUAL to the reference; otherwise within their bounds. NaN exactly where the reference has NaN, no
    infinity anywhere, every mean and covariance within base bound + divisor term. -> the largest ratios."""
    label, ref, bnd = case.label, case.ref, case.bnd
    got_m, got_q = np.asarray(got_m), np.asarray(got_q)
    assert got_m.shape == ref.shape and got_m.dtype == np.float64 and got_q.shape == case.ref_q.shape, (label, got_m.shape, got_m.dtype)
    sums = np.concatenate([got_m[:, :2], got_q[:, None]], axis=1)
    ref_sums = np.concatenate([ref[:, :2], case.ref_q[:, None]], axis=1)
    if case.exact:
        bad = np.argwhere(sums.astype(LD) != ref_sums)
        assert bad.size == 0, (label, "W, W2, Q are not the exact sums at (slice, entry)", bad[:8].tolist())
        worst = Worst()
    else:
        r = mr.error_over_bound(sums, ref_sums, np.concatenate([bnd.mom[:, :2], bnd.charge[:, None]], axis=1))
        assert float(r.max()) <= 1.0, (label, "W, W2, Q", float(r.max()), np.argwhere(r > 1.0)[:8].tolist())
        worst = Worst(float(r.max()), float(r.max()))
    bad = np.argwhere(np.isnan(got_m) != np.isnan(ref))
    assert bad.size == 0, (label, "NaN pattern differs at (slice, entry)", bad[:8].tolist())
    assert not np.isinf(got_m).any(), (label, "infinite entries", np.argwhere(np.isinf(got_m))[:8].tolist())
    fin = ~np.isnan(ref)
    fin[:, :2] = False
    if fin.any():
        with np.errstate(all="ignore"):
            full = mr.error_over_bound(got_m[fin], ref[fin], (bnd.mom + bnd.divisor)[fin])
            base = mr.error_over_bound(got_m[fin], ref[fin], bnd.mom[fin])
        worst.merge(Worst(float(full.max()), float(base.max())))
        assert float(full.max()) <= 1.0, (label, "error / bound", float(full.max()), "without the divisor term", float(base.max()),
                                          "at (slice, entry)", np.argwhere(fin)[full > 1.0][:8].tolist())
    return worst


# ---------------------------------------------------------------------------------------------------------------- the kernels' scheme
def scheme(x, w, q, k, S, wrong=None):
    """((S, 29), (S,)) float64: the arithmetic of slice_piece_kernel and slice_finalize_kernel restated in numpy float64 — the
    members of a slice in particle order (the stable counting sort), pieces of 1024, per piece W, W2, sum q w, the mean from the
    uncentred sums and the second moments about that mean, then the pieces merged in order, those without weight left out.
    `wrong` builds a deliberately wrong variant (tests/test_slices_ref_host.py shows that `compare` rejects each):
      "neighbour"   the first member of the fullest slice is counted in the slice beside it
      "boundary"    every piece but a slice's last ends one particle early: the particle at the boundary is dropped
      "nan_merge"   pieces without weight are merged like the others, with their mean of 0 / 0"""
    k = k.copy()
    if wrong == "neighbour":
        s = int(np.argmax(np.bincount(k[k >= 0], minlength=S)))
        k[np.flatnonzero(k == s)[0]] = s + 1 if s + 1 < S else s - 1
    out, charge = np.empty((S, 29)), np.empty(S)
    x64 = x[:, :6].astype(np.float64)
    with np.errstate(all="ignore"):
        for s in range(S):
            members = np.flatnonzero(k == s)
            parts = []
            for p0 in range(0, members.shape[0], PIECE):
                p1 = min(p0 + PIECE, members.shape[0])
                if wrong == "boundary" and p1 < members.shape[0]:
                    p1 -= 1
                idx = members[p0:p1]
                ws, xs = w[idx], x64[idx]
                Wp = ws.sum()
                mp = (ws[:, None] * xs).sum(axis=0) / Wp
                d = xs - mp
                parts.append((Wp, (ws * ws).sum(), mp, (ws[:, None] * d[:, IU[0]] * d[:, IU[1]]).sum(axis=0), (q[idx] * ws).sum()))
            W = W2 = Q = np.float64(0.0)
            mu = np.zeros(6)
            for Wp, W2p, mp, Mp, Qp in parts:
                Q += Qp
                if not Wp > 0.0 and wrong != "nan_merge":
                    continue
                W, W2, mu = W + Wp, W2 + W2p, mu + Wp * mp
            mu = mu / W
            M = np.zeros(21)
            for Wp, W2p, mp, Mp, Qp in parts:
                if not Wp > 0.0 and wrong != "nan_merge":
                    continue
                d = mp - mu
                M = M + (Mp + Wp * d[IU[0]] * d[IU[1]])
            out[s, 0], out[s, 1], out[s, 2:8], out[s, 8:] = W, W2, mu, M / (W - W2 / W)
            charge[s] = Q
    return out, charge


# ---------------------------------------------------------------------------------------------------------------- gradients
def autograd_restatement(x, w, q, k, S):
    """((S, 29), (S,)) torch float64, differentiable in x (N, 7), w (N,), q (N,): the same statistics with `index_add` for the
    slices k (N,) int64 (-1: none). Degenerate slices are NaN as in `reference`, selected AFTER a division by 1, so that a slice
    that takes no part in a loss hands back zeros (torch's own backward of 0 / 0 would be NaN even for a zero cotangent)."""
    m = k >= 0
    idx = k[m]
    xs, ws, qs = x[m][:, :6], w[m], q[m]
    kw = {"dtype": torch.float64}
    W = torch.zeros(S, **kw).index_add(0, idx, ws)
    W2 = torch.zeros(S, **kw).index_add(0, idx, ws * ws)
    Q = torch.zeros(S, **kw).index_add(0, idx, qs * ws)
    nw = torch.bincount(idx[ws.detach() != 0], minlength=S)
    has_w, has_cov = nw >= 1, nw >= 2
    one = torch.ones((), **kw)
    Ws = torch.where(has_w, W, one)
    mu = torch.zeros(S, 6, **kw).index_add(0, idx, ws[:, None] * xs) / Ws[:, None]
    d = xs - mu[idx]
    iu0, iu1 = torch.from_numpy(IU[0]), torch.from_numpy(IU[1])
    M = torch.zeros(S, 21, **kw).index_add(0, idx, ws[:, None] * d[:, iu0] * d[:, iu1])
    cf = torch.where(has_cov, W - W2 / Ws, one)
    nan = torch.full((), float("nan"), **kw)
    mu = torch.where(has_w[:, None], mu, nan)
    cov = torch.where(has_cov[:, None], M / cf[:, None], nan)
    return torch.cat([W[:, None], W2[:, None], mu, cov], dim=1), Q


# ---------------------------------------------------------------------------------------------------------------- the cases
def spread_counts(N, S, seed):
    """N particles thrown into S slices at random."""
    return np.random.default_rng([512, N, S, seed]).multinomial(N, np.full(S, 1.0 / S))


def drawn_counts(N, S, seed):
    """Counts drawn from 0 ... 2 N / S with about 5 % empty slices and (for S >= 8) one slice of one particle and one of two,
    brought to the sum N by single particles added to or taken from the other populated slices."""
    rng = np.random.default_rng([1024, N, S, seed])
    cap = max(2 * N // S, 1)
    c = rng.integers(0, cap + 1, size=S)
    c[rng.random(S) < 0.05] = 0
    free = np.ones(S, dtype=bool)
    if S >= 8:
        one, two = rng.choice(S, size=2, replace=False)
        c[one], c[two] = 1, 2
        free[[one, two]] = False
    if not (free & (c > 0)).any():
        c[np.flatnonzero(free)[0]] = 1
    while c.sum() != N:
        diff = N - int(c.sum())
        ok = free & (c > 0) & ((c < cap) if diff > 0 else (c > 1))
        if not ok.any():                                   # (every populated slice is full: a few go over the cap)
            ok = free & (c > 0)
            c[np.flatnonzero(ok)[0]] += diff
            continue
        pick = rng.permutation(np.flatnonzero(ok))[:abs(diff)]
        c[pick] += 1 if diff > 0 else -1
    assert c.sum() == N and (c >= 0).all()
    return c


TILE_N = (1, 63, 64, 65, 1023, 1024, 1025, 4097)
SCAN_N = (65536, 65537)
COUNT_S = (2, 63, 64, 65, 255, 256, 257, 1024, 2047, 2048)
LANE_CASES = ("ascending", "round_robin_64", "round_robin_65", "alternating_nan", "alternating_below", "alternating_above",
              "tile_outside", "all_outside")


def _builders():
    """name -> (exact?, function that builds the beam): every forward case of tests/test_gpu_slice_paths.py."""
    b = {}
    for N in TILE_N:
        for S in (3, 1):
            b[f"tiles N={N} S={S}"] = (True, functools.partial(lambda N, S: patterned(spread_counts(N, S, 0), "shuffled", 1), N, S))
    for N in SCAN_N:
        for S in (1, 257):
            for order in ("shuffled", "ascending"):
                b[f"scan N={N} S={S} {order}"] = (True, functools.partial(
                    lambda N, S, order: patterned(spread_counts(N, S, 1), order, 2), N, S, order))
    for S in COUNT_S:
        b[f"slice_count N=4099 S={S}"] = (True, functools.partial(lambda S: patterned(drawn_counts(4099, S, 0), "shuffled", 3), S))
    b["slice_count N=65537 S=2048"] = (True, lambda: patterned(drawn_counts(65537, 2048, 0), "shuffled", 3))
    for order in ORDERS:
        b[f"pieces {order}"] = (True, functools.partial(lambda order: patterned(PIECE_COUNTS, order, 4), order))
    for name, dead in DEAD_SETS.items():
        b[f"weightless {name}"] = (True, functools.partial(lambda dead: patterned(PIECE_COUNTS, "ascending", 4, dead), dead))
    b["lanes ascending"] = (True, lambda: patterned(spread_counts(4099, 3, 2), "ascending", 5))
    b["lanes round_robin_64"] = (True, lambda: patterned(np.full(64, 65), "round_robin", 5))
    b["lanes round_robin_65"] = (True, lambda: patterned(np.full(65, 63), "round_robin", 5))
    for kind in ("nan", "below", "above"):
        b[f"lanes alternating_{kind}"] = (True, functools.partial(
            lambda kind: outside(patterned(spread_counts(4099, 5, 3), "shuffled", 5), slice(1, None, 2), kind), kind))
    b["lanes tile_outside"] = (True, lambda: outside(patterned(spread_counts(4099, 5, 3), "shuffled", 5), slice(1024, 2048), "mixed"))
    b["lanes all_outside"] = (True, lambda: outside(patterned(spread_counts(4099, 5, 3), "shuffled", 5), slice(None), "mixed"))
    for name in HARD:
        b[f"hard {name}"] = (False, functools.partial(hard, name))
    return b


BUILDERS = _builders()


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    exact, build = BUILDERS[name]
    return Case(name, build(), exact)
