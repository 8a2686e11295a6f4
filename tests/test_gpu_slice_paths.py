"""Every launch of ParticleBeam.slice_statistics (csrc/chx_slices.hip) at the sizes where its indexing changes, against the
per-slice two-pass statistics in np.longdouble within a derived bound (tests/slices_ref.py), and its backward pass against torch
autograd through a float64 restatement on the CPU.

The constants the cases are built around: kSliceTile = 1024 particles per wave tile of slice_rank_kernel (16 rounds of 64 lanes),
64 tiles per round of slice_scan_kernel, CHX_BLOCK = 256 threads in slice_start_kernel (ceil(S / 256) slices per thread),
kPiece = 1024 sorted particles per workgroup of slice_piece_kernel, CHX_SLICES_MAX = 2048 slices (edges and 4 x S counters in LDS),
nbits = ceil(log2 S) ballots per round, one thread per particle in workgroups of 256 in slice_bwd_kernel.

Patterned cases assert W, W2 and the charge with ==, the NaN pattern of the reference, and every mean and covariance within its
bound; every test prints the largest error / bound it saw ("slice_paths <group> <dtype> ...": profiles/slice_paths.md)."""
import functools

import numpy as np
import pytest
import torch

from tests import moments_ref as mr
from tests import slices_ref as sr

pytestmark = pytest.mark.gpu
DTYPES = ["f32", "f64"]
DT = {"f32": torch.float32, "f64": torch.float64}


def report(group, tag, what, worst):
    print(f"slice_paths {group} {tag} {what}: max err/bound {worst.ratio:.3g} (without the divisor term {worst.base:.3g})")


def on_device(beam, tag):
    """(x, w, q, edges) of a slices_ref.Beam as device tensors of the dtype `tag` (every value converts exactly)."""
    def put(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(DT[tag]).cuda()

    return put(beam.x), put(beam.w), put(beam.q), put(beam.edges)


def slices_of(x, w, q, edges):
    import cheetah_amd as ca

    energy = torch.tensor(1e8, dtype=x.dtype, device=x.device)
    return ca.ParticleBeam(x, energy, particle_charges=q, survival_probabilities=w).slice_statistics(edges=edges)


def run(beam, tag):
    """slice_statistics of the beam -> (moments (S, 29), charge (S,)) float64 numpy."""
    sl = slices_of(*on_device(beam, tag))
    assert sl.moments.dtype == torch.float64 and sl.charge.dtype == torch.float64 and sl.moments.shape == (beam.S, 29)
    assert torch.equal(sl.num_particles_survived, sl.moments[..., 0])
    return sl.moments.cpu().numpy(), sl.charge.cpu().numpy()


def check(name, tag, group):
    case = sr.case(name)
    got_m, got_q = run(case.beam, tag)
    worst = sr.compare(got_m, got_q, case)
    report(group, tag, name, worst)
    return case, got_m, got_q


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("S", [3, 1])
@pytest.mark.parametrize("N", sr.TILE_N)
def test_tiles(N, S, tag):
    """Fewer particles than a wave, a partial round of 64, a full tile, a last tile of one particle (1025, 4097); S = 1 has
    nbits = 0 (no ballot but the first), S = 3 is no power of two."""
    check(f"tiles N={N} S={S}", tag, "tiles")


@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("order", ["shuffled", "ascending"])
@pytest.mark.parametrize("S", [1, 257])
@pytest.mark.parametrize("N", sr.SCAN_N)
def test_scan(N, S, order, tag):
    """64 tiles (one round of slice_scan_kernel) and 65 (a second round with the carry), with one slice and with 257."""
    assert -(-N // sr.TILE) == (64 if N == 65536 else 65)
    check(f"scan N={N} S={S} {order}", tag, "scan")


@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("S", sr.COUNT_S)
def test_slice_count(S, tag):
    """The nbits edges (63 | 64 | 65, 2047 | 2048), one and two slices per thread of slice_start_kernel (256 | 257), the largest
    LDS request (2048), the piece search over empty slices."""
    check(f"slice_count N=4099 S={S}", tag, "slice_count")


@pytest.mark.parametrize("tag", DTYPES)
def test_slice_count_most_slices_on_many_tiles(tag):
    check("slice_count N=65537 S=2048", tag, "slice_count")


@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("order", sr.ORDERS)
def test_pieces(order, tag):
    """Slices of 1024 | 1025, 2048 | 2049, 3073, 1023, 0, 1 and 2 particles: one to four pieces per slice, a last piece of one."""
    check(f"pieces {order}", tag, "pieces")


@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("dead", list(sr.DEAD_SETS))
def test_pieces_without_weight(dead, tag):
    """A first piece without weight (the `continue` of the merge), a slice whose only weight sits in its last piece, and a slice
    of 1025 members with W = 0: charge 0 and the NaN pattern `_ops.moments` gives those particles."""
    import cheetah_amd as ca

    case, got_m, got_q = check(f"weightless {dead}", tag, "pieces_weightless")
    if dead == "all_of_1025":
        x, w, _, _ = on_device(case.beam, tag)
        members = torch.from_numpy(np.flatnonzero(case.beam.k == 1)).cuda()
        alone = ca._ops.moments(x[members], w[members]).cpu().numpy()
        assert got_q[1] == 0 and got_m[1, 0] == 0 and got_m[1, 1] == 0
        assert (np.isnan(got_m[1]) == np.isnan(alone)).all()


@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("lanes", sr.LANE_CASES)
def test_lanes(lanes, tag):
    """All 64 lanes of a round in one slice (sorted), in 64 distinct slices (round robin), members alternating with NaN / low / high
    particles, a whole tile without a member, no member at all."""
    case, got_m, got_q = check(f"lanes {lanes}", tag, "lanes")
    if lanes == "all_outside":
        assert (got_m[:, :2] == 0).all() and np.isnan(got_m[:, 2:]).all() and (got_q == 0).all()


@pytest.mark.parametrize("tag", DTYPES)
def test_membership_of_special_values(tag):
    """hist_bin on -0.0 at an edge of 0.0, +-inf, NaN, every edge value, the neighbours of an interior edge and of both ends,
    non-uniform edges with a duplicated interior edge: the counts and the weighted counts equal `membership` exactly; with strictly
    increasing float64 edges also torch.histogram(weight=w)."""
    dt = DT[tag]
    for duplicate in (True, False):
        edges = torch.tensor([0.0, 0.5, 0.75] + ([0.75] if duplicate else []) + [2.0, 3.5, 7.0], dtype=dt)
        S = edges.shape[0] - 1
        inf = torch.tensor(float("inf"), dtype=dt)
        special = torch.cat([torch.tensor([-0.0, float("inf"), float("-inf"), float("nan")], dtype=dt), edges,
                             torch.nextafter(edges, inf), torch.nextafter(edges, -inf)])
        g = torch.Generator().manual_seed(3)
        tau = torch.cat([special, (torch.rand(1100 - special.shape[0], generator=g, dtype=torch.float64) * 9.0 - 1.0).to(dt)])
        tau = tau[torch.randperm(tau.shape[0], generator=g)]
        N = tau.shape[0]
        base = sr.patterned([N], "ascending", 6)
        x = torch.from_numpy(base.x).to(dt)
        x[:, 4] = tau
        k = sr.membership(tau, edges)
        assert (k == -1).sum() > 100 and all((k == s).sum() > 0 or (duplicate and s == 2) for s in range(S))
        assert k[tau == 0].eq(0).all() and (tau == 0).sum() == 2 and k[tau == 7.0].eq(S - 1).all()       # -0.0 and 0.0; tau == e_S
        m = k >= 0
        for w in (torch.ones(N, dtype=torch.float64), torch.from_numpy(base.w)):
            sl = slices_of(x.cuda(), w.to(dt).cuda(), torch.from_numpy(base.q).to(dt).cuda(), edges.cuda())
            want = torch.zeros(S, dtype=torch.float64).index_add_(0, k[m], w[m])
            assert torch.equal(sl.num_particles_survived.cpu(), want)
            want_q = torch.zeros(S, dtype=torch.float64).index_add_(0, k[m], (w * torch.from_numpy(base.q))[m])
            assert torch.equal(sl.charge.cpu(), want_q)
            if not duplicate and tag == "f64":
                hist = torch.histogram(tau, bins=edges, weight=w)[0]
                assert torch.equal(sl.num_particles_survived.cpu(), hist)
    print(f"slice_paths membership {tag}: counts exact")


def _row_case(label, x, w, q, edges, tag):
    """The case of one batch row whose slices follow from `membership` in the dtype `tag` (all values exact in float32)."""
    k = sr.membership(torch.from_numpy(np.ascontiguousarray(x[:, 4])).to(DT[tag]), torch.from_numpy(edges).to(DT[tag])).numpy()
    return sr.Case(label, sr.Beam(x, w, q, k, edges), True)


@pytest.mark.parametrize("tag", DTYPES)
def test_batch_rows_with_shared_particles(tag):
    """B = 3: one particle array, (3, N) weights, (3, S + 1) edges that populate different slices in every row (the strides Bx = 1,
    Bw = Be = 3), N = 1025."""
    base = sr.patterned(sr.spread_counts(1025, 6, 5), "shuffled", 7)
    S = base.S
    ws = np.stack([sr.patterned(sr.spread_counts(1025, 6, 5), "shuffled", 7 + b).w for b in range(3)])
    edges = np.stack([np.arange(S + 1.0), np.arange(S + 1.0) + 2.0, np.arange(S + 1.0) * 0.5 + 4.5])
    x, _, q, _ = on_device(base, tag)
    sl = slices_of(x, torch.from_numpy(ws).to(DT[tag]).cuda(), q, torch.from_numpy(edges).to(DT[tag]).cuda())
    assert sl.moments.shape == (3, S, 29) and sl.charge.shape == (3, S)
    worst = sr.Worst()
    populated = []
    for b in range(3):
        case = _row_case(f"batch row {b}", base.x, ws[b], base.q, edges[b], tag)
        populated.append(tuple(case.nw > 0))
        worst.merge(sr.compare(sl.moments[b].cpu().numpy(), sl.charge[b].cpu().numpy(), case))
    assert len(set(populated)) == 3
    report("batch", tag, "B=3 shared particles, per-row weights and edges, N=1025", worst)


@pytest.mark.parametrize("tag", DTYPES)
def test_batch_of_particles_with_shared_edges(tag):
    """A (2, 3) batch of particle arrays, weights and charges with one set of edges (Bx = Bw = Bq = 6, Be = 1)."""
    beams = [sr.patterned(sr.spread_counts(1025, 4, 10 + b), "shuffled", 20 + b) for b in range(6)]
    dt = DT[tag]
    x = torch.from_numpy(np.stack([b.x for b in beams])).to(dt).reshape(2, 3, 1025, 7).cuda()
    w = torch.from_numpy(np.stack([b.w for b in beams])).to(dt).reshape(2, 3, 1025).cuda()
    q = torch.from_numpy(np.stack([b.q for b in beams])).to(dt).reshape(2, 3, 1025).cuda()
    sl = slices_of(x, w, q, torch.from_numpy(beams[0].edges).to(dt).cuda())
    assert sl.moments.shape == (2, 3, 4, 29)
    worst = sr.Worst()
    for b, beam in enumerate(beams):
        worst.merge(sr.compare(sl.moments[b // 3, b % 3].cpu().numpy(), sl.charge[b // 3, b % 3].cpu().numpy(), sr.Case(f"batch {b}", beam, True)))
    report("batch", tag, "(2, 3) batch of particles, shared edges, N=1025", worst)


@pytest.mark.parametrize("tag", DTYPES)
def test_row_chunks_give_the_same_bits(tag, monkeypatch):
    """B = 5 with MAX_GRID_ROWS = 2: the host cuts the rows into chunks of 2, 2 and 1 (`_rows` keeps the shared particles whole,
    `out[b0:b1]` slices outputs and cotangents). Forward and backward are bit-equal to the call in one chunk; row 4 against the
    reference."""
    import cheetah_amd as ca
    from cheetah_amd import _ops_slices

    base = sr.patterned(sr.spread_counts(1025, 5, 6), "shuffled", 8)
    ws = np.stack([sr.patterned(sr.spread_counts(1025, 5, 6), "shuffled", 30 + b).w for b in range(5)])
    x, _, q, edges = on_device(base, tag)
    w = torch.from_numpy(ws).to(DT[tag]).cuda()
    g = torch.Generator().manual_seed(4)
    gm = torch.randn(5, base.S, 29, generator=g, dtype=torch.float64).cuda()
    gm[..., 8:] *= 1e-10
    gq = torch.randn(5, base.S, generator=g, dtype=torch.float64).cuda()

    def call():
        xs, wr, qs = (t.clone().requires_grad_() for t in (x, w, q))
        m, c = ca._ops.slice_moments(xs, wr, qs, edges)
        grads = torch.autograd.grad((m, c), (xs, wr, qs), (torch.where(torch.isnan(m), 0.0, gm), gq))
        return (m.detach(), c.detach()) + grads

    whole = call()
    assert _ops_slices.MAX_GRID_ROWS >= 5
    monkeypatch.setattr(_ops_slices, "MAX_GRID_ROWS", 2)
    chunked = call()
    view = {torch.float32: torch.int32, torch.float64: torch.int64}
    for a, b in zip(whole, chunked):
        assert a.shape == b.shape and torch.equal(a.view(view[a.dtype]), b.view(view[b.dtype]))
    assert whole[2].shape == (1025, 7) and whole[3].shape == (5, 1025)
    worst = sr.compare(chunked[0][4].cpu().numpy(), chunked[1][4].cpu().numpy(), sr.Case("row 4 of 5", sr.Beam(base.x, ws[4], base.q, base.k, base.edges), True))
    report("row_chunks", tag, "B=5 in chunks of 2", worst)


@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("name", sr.HARD)
def test_hard_beams(name, tag):
    """Slice means 1e3 sigma off (the first-moment sums are uncentred), slices of two and three particles with weight ratios down to
    1e-8 and one weight of 1 among a thousand of 1e-6 (the divisor W - W2 / W cancels). Every populated slice also against
    `_ops.moments` of that slice's particles, to the sum of the two bounds (the one-pass kernel forms the divisor the same way)."""
    import cheetah_amd as ca

    case, got_m, got_q = check(f"hard {name}", tag, "hard_beams")
    b = case.beam
    x, w, _, _ = on_device(b, tag)
    worst = sr.Worst()
    for s in np.flatnonzero(case.nw >= 1):
        members = np.flatnonzero(b.k == s)
        idx = torch.from_numpy(members).cuda()
        alone = ca._ops.moments(x[idx], w[idx]).cpu().numpy()
        assert (np.isnan(alone) == np.isnan(got_m[s])).all(), (name, s)
        own = mr.bounds(b.x[None, members], b.w[None, members], case.ref[None, s])[0]
        base = case.bnd.mom[s] + own
        full = base + 2.0 * case.bnd.divisor[s]
        fin = ~np.isnan(got_m[s])
        err = np.abs(got_m[s] - alone)
        with np.errstate(all="ignore"):
            ratio, ratio_base = np.where(err == 0, 0.0, err / full)[fin], np.where(err == 0, 0.0, err / base)[fin]
        worst.merge(sr.Worst(float(ratio.max()), float(ratio_base.max())))
        assert float(ratio.max()) <= 1.0, (name, s, float(ratio.max()), float(ratio_base.max()))
    report("hard_beams_vs_moments", tag, name, worst)


@pytest.mark.parametrize("tag", DTYPES)
def test_two_calls_give_the_same_bits(tag):
    b = sr.case("pieces shuffled").beam
    (m0, q0), (m1, q1) = run(b, tag), run(b, tag)
    assert (m0.view(np.int64) == m1.view(np.int64)).all() and (q0.view(np.int64) == q1.view(np.int64)).all()


# ---------------------------------------------------------------------------------------------------------------- backward
BWD_BEAMS = {
    "N=255 S=3": lambda: sr.Case("bwd N=255", sr.patterned(sr.spread_counts(255, 3, 7), "shuffled", 40), True),
    "N=256 S=3": lambda: sr.Case("bwd N=256", sr.patterned(sr.spread_counts(256, 3, 7), "shuffled", 41), True),
    "N=257 S=3": lambda: sr.Case("bwd N=257", sr.patterned(sr.spread_counts(257, 3, 7), "shuffled", 42), True),
    "N=1025 S=3": lambda: sr.Case("bwd N=1025", sr.patterned(sr.spread_counts(1025, 3, 7), "shuffled", 43), True),
    "N=4099 S=2048": lambda: sr.case("slice_count N=4099 S=2048"),
    "degenerate": lambda: sr.Case("bwd degenerate", sr.patterned([300, 0, 1, 400, 2, 322], "shuffled", 44), True),
}


@functools.lru_cache(maxsize=None)
def bwd_case(name):
    return BWD_BEAMS[name]()


def cotangent(case, seed, parts):
    """Fixed-seed cotangents (S, 29) of the moments and (S,) of the charge. `parts` of "sums" (W, W2: every slice), "mu", "cov"
    (slices with at least two weighted particles, the others are NaN or need not be read) and "charge" (every slice). The means'
    cotangents are scaled by W / sigma_j and the covariances' by cf / (sigma_i sigma_j), so that every term of a weight's gradient
    is of order 1 and every term of a coordinate's gradient of order 1 / sigma_j."""
    S = case.beam.S
    g = torch.Generator().manual_seed(seed)
    r, rq = torch.randn(S, 29, generator=g, dtype=torch.float64), torch.randn(S, generator=g, dtype=torch.float64)
    ref = torch.from_numpy(case.ref.astype(np.float64))
    rows = torch.from_numpy(case.nw >= 2)
    sig = ref[rows][:, sr.DIAG].median(dim=0).values.sqrt()
    W, W2 = ref[:, 0], ref[:, 1]
    cf = W - W2 / W
    coef = torch.zeros(S, 29, dtype=torch.float64)
    if "sums" in parts:
        coef[:, :2] = r[:, :2]
    if "mu" in parts:
        coef[rows, 2:8] = (r[:, 2:8] * W[:, None] / sig)[rows]
    if "cov" in parts:
        coef[rows, 8:] = (r[:, 8:] * cf[:, None] / (sig[sr.IU[0]] * sig[sr.IU[1]]))[rows]
    return coef, (rq if "charge" in parts else torch.zeros(S, dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def reference_grads(name, seed, parts):
    case = bwd_case(name)
    b = case.beam
    x, w, q = (torch.from_numpy(a).clone().requires_grad_() for a in (b.x, b.w, b.q))
    m, c = sr.autograd_restatement(x, w, q, torch.from_numpy(b.k), b.S)
    assert torch.equal(torch.isnan(m), torch.from_numpy(np.isnan(case.ref)))
    return torch.autograd.grad((m, c), (x, w, q), cotangent(case, seed, parts))


def device_grads(beam, tag, coef, cq):
    import cheetah_amd as ca

    x, w, q, edges = on_device(beam, tag)
    x, w, q = x.requires_grad_(), w.requires_grad_(), q.requires_grad_()
    m, c = ca._ops.slice_moments(x, w, q, edges)
    gx, gw, gq = torch.autograd.grad((m, c), (x, w, q), (coef.cuda(), cq.cuda()))
    assert gx.dtype == gw.dtype == gq.dtype == DT[tag]
    return gx.cpu().double(), gw.cpu().double(), gq.cpu().double()


def gradient_ratio(got, want, tag, what):
    """|got - want| over the bound, the largest per tensor (every coordinate column of the particles' gradient is a tensor of
    its own: their scales differ by 1 / sigma_j). float64: 1e-9 max |want|, the bound of
    test_gradients_match_autograd_through_the_restatement. float32: the kernel rounds a float64 value once, so 2^-24 |want| more,
    entry by entry. A tensor whose reference is all zero must be all zero."""
    gx, gw, gq = got
    rx, rw, rq = want
    assert torch.isfinite(gx).all() and torch.isfinite(gw).all() and torch.isfinite(gq).all(), (what, "gradients that are not finite")
    assert (gx[:, 6] == 0).all() and (rx[:, 6] == 0).all()
    worst = 0.0
    for name, g, r in [(f"x[{j}]", gx[:, j], rx[:, j]) for j in range(6)] + [("w", gw, rw), ("q", gq, rq)]:
        scale = r.abs().max()
        if scale == 0:
            assert (g == 0).all(), (what, name, "must be exactly zero")
            continue
        tol = 1e-9 * scale + (2.0 ** -24 * r.abs() if tag == "f32" else 0.0)
        ratio = float(((g - r).abs() / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (what, name, ratio)
    return worst


ALL = ("sums", "mu", "cov", "charge")


@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("name", ["N=255 S=3", "N=256 S=3", "N=257 S=3", "N=1025 S=3", "N=4099 S=2048"])
def test_backward_sizes(name, tag):
    """One thread per particle at the workgroup edges 255 | 256 | 257, several workgroups, and the edge table in LDS at its largest
    with 2048 slices (empty, one- and two-particle slices among them): a cotangent on all 29 entries and on the charge."""
    case = bwd_case(name)
    got = device_grads(case.beam, tag, *cotangent(case, 50, ALL))
    worst = gradient_ratio(got, reference_grads(name, 50, ALL), tag, name)
    dead = torch.from_numpy((case.beam.w == 0) & (case.beam.k >= 0))
    assert dead.any() and (got[0][dead] == 0).all()                    # a member without weight: dX = 0, dW the reference's
    print(f"slice_paths backward_sizes {tag} {name}: max gradient error / bound {worst:.3g}")


@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("parts", [("charge",), ("mu",), ("sums",), ("cov",)])
def test_backward_cotangent_shapes(parts, tag):
    """Slices of 300, 0, 1, 400, 2 and 322 particles. Charge only: no moment cotangent at all (flag 0). Means only: no 1 / cf term
    (the `any_cov` branch); the empty and the one-particle slice take no part and their particles get exactly 0. W and W2 only:
    table entries 34 / 35. Covariances of the slices with two weighted particles or more."""
    case = bwd_case("degenerate")
    got = device_grads(case.beam, tag, *cotangent(case, 51, parts))
    worst = gradient_ratio(got, reference_grads("degenerate", 51, parts), tag, parts)
    lone = torch.from_numpy(case.beam.k == 2)
    if parts in (("mu",), ("cov",)):
        assert (got[0][lone] == 0).all() and (got[1][lone] == 0).all() and (got[2][lone] == 0).all()
    if parts != ("charge",):
        assert got[1].abs().max() > 0
    print(f"slice_paths backward_cotangents {tag} {parts[0]}: max gradient error / bound {worst:.3g}")


@pytest.mark.parametrize("tag", DTYPES)
def test_backward_sums_of_a_slice_whose_members_carry_no_weight(tag):
    """W, W2 and the charge of a slice whose members all have w = 0 are sums like any other: dW = g_W + 2 w g_W2 + q g_Q there,
    not NaN from the slice's undefined mean."""
    beam = sr.patterned([200, 57, 0, 100], "shuffled", 45, dead={1: slice(None)})
    case = sr.Case("bwd weightless slice", beam, True)
    coef, cq = cotangent(case, 52, ("sums", "charge"))
    got = device_grads(beam, tag, coef, cq)
    x, w, q = (torch.from_numpy(a).clone().requires_grad_() for a in (beam.x, beam.w, beam.q))
    m, c = sr.autograd_restatement(x, w, q, torch.from_numpy(beam.k), beam.S)
    want = torch.autograd.grad((m, c), (x, w, q), (coef, cq))
    members = torch.from_numpy(beam.k == 1)
    assert torch.equal(want[1][members], coef[1, 0] + cq[1] * q.detach()[members])
    worst = gradient_ratio(got, want, tag, "weightless slice")
    print(f"slice_paths backward_weightless_slice {tag}: max gradient error / bound {worst:.3g}")


@pytest.mark.parametrize("tag", DTYPES)
def test_backward_of_broadcast_rows(tag):
    """B = 3 with shared particles and charges, per-row weights and edges: the gradient of a shared input is the sum over the rows
    (`dX.sum(0)`): equal to the sum of three single-row runs to the two roundings of a three-term sum, and within the bound of the
    reference's."""
    import cheetah_amd as ca

    dt = DT[tag]
    base = sr.patterned(sr.spread_counts(1025, 6, 5), "shuffled", 7)
    S = base.S
    ws = np.stack([sr.patterned(sr.spread_counts(1025, 6, 5), "shuffled", 7 + b).w for b in range(3)])
    edges = np.stack([np.arange(S + 1.0), np.arange(S + 1.0) + 2.0, np.arange(S + 1.0) * 0.5 + 4.5])
    cases = [_row_case(f"broadcast row {b}", base.x, ws[b], base.q, edges[b], tag) for b in range(3)]
    cots = [cotangent(c, 60 + b, ALL) for b, c in enumerate(cases)]
    x, _, q, _ = on_device(base, tag)
    x, q = x.requires_grad_(), q.requires_grad_()
    w = torch.from_numpy(ws).to(dt).cuda().requires_grad_()
    m, c = ca._ops.slice_moments(x, w, q, torch.from_numpy(edges).to(dt).cuda())
    gx, gw, gq = torch.autograd.grad((m, c), (x, w, q), (torch.stack([t[0] for t in cots]).cuda(), torch.stack([t[1] for t in cots]).cuda()))
    assert gx.shape == (1025, 7) and gw.shape == (3, 1025) and gq.shape == (1025,)
    single, wanted = [], []
    for b in range(3):
        single.append(device_grads(cases[b].beam, tag, *cots[b]))
        xr, wr, qr = (torch.from_numpy(a).clone().requires_grad_() for a in (base.x, ws[b], base.q))
        mm, cr = sr.autograd_restatement(xr, wr, qr, torch.from_numpy(cases[b].beam.k), S)
        wanted.append(torch.autograd.grad((mm, cr), (xr, wr, qr), cots[b]))
    eps = 2.0 ** -24 if tag == "f32" else 2.0 ** -53
    for got, rows in ((gx, [s[0] for s in single]), (gq, [s[2] for s in single])):
        total, size = sum(rows), sum(r.abs() for r in rows)
        assert ((got.cpu().double() - total).abs() <= 2.0 * eps * size).all()
    for b in range(3):
        assert torch.equal(gw[b].cpu().double(), single[b][1])
    # against the reference: the float32 rounding of each row's gradient, then of their sum
    want_x, want_q = sum(t[0] for t in wanted), sum(t[2] for t in wanted)
    gxr, gqr = gx.cpu().double(), gq.cpu().double()
    worst = 0.0
    for name, g, r, size in [(f"x[{j}]", gxr[:, j], want_x[:, j], sum(t[0][:, j].abs() for t in wanted)) for j in range(6)] + \
            [("q", gqr, want_q, sum(t[2].abs() for t in wanted))]:
        tol = 1e-9 * r.abs().max() + (3.0 * 2.0 ** -24 * size if tag == "f32" else 0.0)
        ratio = float(((g - r).abs() / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)
    for b in range(3):
        worst = max(worst, gradient_ratio(single[b], wanted[b], tag, f"row {b}"))
    print(f"slice_paths backward_broadcast {tag}: max gradient error / bound {worst:.3g}")
