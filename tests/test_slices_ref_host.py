"""The restatements of tests/slices_ref.py on the CPU: the vectorised longdouble reference against the loop restatement of
tests/test_gpu_slice_statistics.py, the exactness of the patterned beams, the caps of every case the GPU file uses, the bound
against a float64 numpy restatement of the kernels' scheme — and the same comparison REJECTING three deliberately wrong
restatements, so that the assertions of tests/test_gpu_slice_paths.py are not vacuous. No GPU."""
import numpy as np
import pytest
import torch

from tests import slices_ref as sr
from tests.test_gpu_slice_statistics import _restate_row


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 1e-18


def test_vectorised_reference_equals_the_loop_restatement():
    """A small Gaussian beam with weights, NaN and outside particles, an empty and a one-particle slice: the longdouble reference
    against `_restate_row` (float64) to 1e-12 of sigma, W, W2 and Q to 1e-14 relative, NaN at the same places."""
    g = torch.Generator().manual_seed(5)
    N, S = 3000, 9
    x = torch.randn(N, 7, generator=g, dtype=torch.float64) * torch.tensor([1e-4, 2e-5, 1e-4, 2e-5, 1e-5, 1e-3, 0.0], dtype=torch.float64)
    x[:, 6] = 1.0
    x[:20, 4] = float("nan")
    x[20:40, 4] = 1.0
    x[40, 4] = 1.5e-3                                       # the only particle of slice 7; slice 8 is empty
    w = torch.rand(N, generator=g, dtype=torch.float64)
    w[::7] = 0.0
    q = torch.rand(N, generator=g, dtype=torch.float64) * 1e-15
    edges = torch.cat([torch.linspace(-2e-5, 2e-5, S - 2, dtype=torch.float64), torch.tensor([1e-3, 2e-3, 3e-3], dtype=torch.float64)])
    k = sr.membership(x[:, 4].contiguous(), edges)
    assert (k == 7).sum() == 1 and (k == 8).sum() == 0 and (k == -1).sum() >= 40
    want_m, want_q = _restate_row(x, w, q, edges)
    got_m, got_q = sr.reference(x.numpy(), w.numpy(), q.numpy(), k.numpy(), S)
    got_m, got_q, want_m, want_q = got_m.astype(np.float64), got_q.astype(np.float64), want_m.numpy(), want_q.numpy()
    # (the loop's one-particle slice has cov = 0 / 0 = NaN and its empty slice has NaN means too)
    assert (np.isnan(got_m) == np.isnan(want_m)).all()
    np.testing.assert_allclose(got_m[:, :2], want_m[:, :2], rtol=1e-14, atol=0)
    np.testing.assert_allclose(got_q, want_q, rtol=1e-14, atol=0)
    pop = ~np.isnan(want_m[:, 8])
    sig = np.sqrt(want_m[pop][:, sr.DIAG])
    assert (np.abs(got_m[pop, 2:8] - want_m[pop, 2:8]) <= 1e-12 * sig).all()
    assert (np.abs(got_m[pop, 8:] - want_m[pop, 8:]) <= 1e-12 * sig[:, sr.IU[0]] * sig[:, sr.IU[1]]).all()
    # ... and the differentiable restatement says the same
    tm, tq = sr.autograd_restatement(x, w, q, k, S)
    assert (np.isnan(tm.numpy()) == np.isnan(want_m)).all()
    np.testing.assert_allclose(tm.numpy()[pop], want_m[pop], rtol=1e-9, atol=1e-30)
    np.testing.assert_allclose(tq.numpy(), want_q, rtol=1e-14, atol=0)


@pytest.mark.parametrize("order", sr.ORDERS)
def test_patterned_beams_are_exact_in_both_dtypes(order):
    """Every value survives float32; the membership of tau in both dtypes is the prescribed slice; W, W2 and Q are the same bits
    in float64 and in longdouble, in the given and in a shuffled order of summation."""
    for counts, seed in ((sr.PIECE_COUNTS, 4), (sr.drawn_counts(4099, 2048, 0), 3), (sr.spread_counts(4097, 3, 0), 1)):
        b = sr.patterned(counts, order, seed)
        for a in (b.x, b.w, b.q, b.edges):
            assert (a.astype(np.float32).astype(np.float64) == a).all()
        assert (np.bincount(b.k, minlength=b.S) == np.asarray(counts)).all()
        for dt in (torch.float32, torch.float64):
            k = sr.membership(torch.from_numpy(b.x[:, 4]).to(dt), torch.from_numpy(b.edges).to(dt))
            assert torch.equal(k, torch.from_numpy(b.k))
        ref, ref_q = sr.reference(b.x, b.w, b.q, b.k, b.S)
        perm = np.random.default_rng(0).permutation(b.N)
        for idx in (np.arange(b.N), perm):
            kk = b.k[idx]
            for got, want in ((np.bincount(kk, b.w[idx], b.S), ref[:, 0]), (np.bincount(kk, b.w[idx] ** 2, b.S), ref[:, 1]),
                              (np.bincount(kk, (b.q * b.w)[idx], b.S), ref_q)):
                assert (got.astype(np.longdouble) == want).all()
    if order == "round_robin":
        b = sr.patterned([3, 0, 1, 2], order, 0)
        assert b.k.tolist() == [0, 2, 3, 0, 3, 0]


def test_the_piece_cases_reach_their_edges():
    b = sr.case("pieces ascending").beam
    assert b.N == 10245 and np.bincount(b.k).tolist() == list(sr.PIECE_COUNTS)
    for name, slice_ in (("first_piece_of_2049", 5), ("all_but_last_of_3073", 8), ("all_of_1025", 1)):
        c = sr.case(f"weightless {name}")
        members = np.flatnonzero(c.beam.k == slice_)
        assert (c.beam.w[members[:1024]] == 0).all()                          # the first piece carries no weight
        assert c.ref_q[slice_] == (c.beam.q * c.beam.w)[members].sum()
    assert sr.case("weightless all_of_1025").ref[1, 0] == 0 and np.isnan(sr.case("weightless all_of_1025").ref[1, 2:]).all()
    last = sr.case("weightless all_but_last_of_3073")
    if last.beam.w[np.flatnonzero(last.beam.k == 8)[-1]] != 0:
        assert np.isfinite(last.ref[8, :8].astype(np.float64)).all() and np.isnan(last.ref[8, 8:]).all()
    for S, nbits in ((63, 6), (64, 6), (65, 7), (2047, 11), (2048, 11), (1, 0), (3, 2)):
        assert (S - 1).bit_length() == nbits
    rr = sr.case("lanes round_robin_65").beam
    for r in range(0, rr.N - 63, 64):                                          # no two of 64 consecutive particles share a slice
        assert np.unique(rr.k[r:r + 64]).shape[0] == 64
    assert (sr.case("lanes tile_outside").beam.k[1024:2048] == -1).all() and (sr.case("lanes all_outside").beam.k == -1).all()
    for S in (255, 2048):
        c = np.bincount(sr.case(f"slice_count N=4099 S={S}").beam.k, minlength=S)
        assert (c == 0).any() and (c == 1).any() and (c == 2).any() and c.sum() == 4099


@pytest.mark.parametrize("name", list(sr.BUILDERS))
def test_caps_and_the_kernels_scheme_within_the_bound(name):
    """Building a case asserts its caps (bound <= 1e-6 sigma, divisor term left out). The float64 numpy restatement of the
    kernels' scheme stays within the bound; what it needs of the divisor term is printed."""
    c = sr.case(name)
    b = c.beam
    got_m, got_q = sr.scheme(b.x, b.w, b.q, b.k, b.S)
    worst = sr.compare(got_m, got_q, c)
    print(f"slice_paths numpy_scheme {name}: max err/bound {worst.ratio:.3g} (without the divisor term {worst.base:.3g}); "
          f"caps cov {c.caps[0]:.2g} mu {c.caps[1]:.2g} divisor term {c.caps[2]:.2g}")
    if name in ("hard uneven_pairs", "hard heavy_and_light"):          # the cancellation is there, and only there
        assert c.caps[2] > 100 * c.caps[0]


@pytest.mark.parametrize("wrong", ["neighbour", "boundary", "nan_merge"])
def test_wrong_restatements_are_rejected(wrong):
    """One particle counted in the neighbouring slice, one particle dropped at a piece boundary, a weightless first piece merged
    with its NaN mean: `compare` fails for each — on the exact sums AND, with those left aside, on the means and covariances."""
    name = "weightless first_piece_of_2049" if wrong == "nan_merge" else "pieces shuffled"
    c = sr.case(name)
    b = c.beam
    good = sr.scheme(b.x, b.w, b.q, b.k, b.S)
    sr.compare(*good, c)
    got_m, got_q = sr.scheme(b.x, b.w, b.q, b.k, b.S, wrong=wrong)
    with pytest.raises(AssertionError):
        sr.compare(got_m, got_q, c)
    # with W, W2 and Q of the correct run put back, the NaN pattern or the bound still rejects it
    got_m[:, :2] = good[0][:, :2]
    with pytest.raises(AssertionError, match="NaN pattern|error / bound"):
        sr.compare(got_m, good[1], c)


def test_a_wrong_neighbour_is_rejected_on_a_real_valued_beam_too():
    c = sr.case("hard offset_centroid")
    b = c.beam
    sr.compare(*sr.scheme(b.x, b.w, b.q, b.k, b.S), c)
    with pytest.raises(AssertionError):
        sr.compare(*sr.scheme(b.x, b.w, b.q, b.k, b.S, wrong="neighbour"), c)


def test_autograd_restatement_hands_zeros_to_slices_outside_the_loss():
    """An empty and a one-particle slice next to populated ones: a loss over the populated slices has finite gradients, exactly 0
    for the particle of the one-particle slice."""
    b = sr.patterned([40, 0, 1, 30], "shuffled", 9)
    x, w, q = (torch.from_numpy(a).clone().requires_grad_() for a in (b.x, b.w, b.q))
    m, c = sr.autograd_restatement(x, w, q, torch.from_numpy(b.k), b.S)
    assert torch.isnan(m[1, 2:]).all() and torch.isnan(m[2, 8:]).all()
    (m[[0, 3]][:, 2:].sum() + c[[0, 3]].sum()).backward()
    lone = int(np.flatnonzero(b.k == 2)[0])
    for g in (x.grad, w.grad, q.grad):
        assert torch.isfinite(g).all() and (g[lone] == 0).all()
    assert x.grad.abs().max() > 0
