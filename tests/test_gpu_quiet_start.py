"""Quiet-start beams on the GPU: `chx_quiet_sequence` against the numpy `uint64` restatement of the Halton sequence (bit for bit),
its normal deviates against `torch.special.ndtri` of those exact uniforms, and `ParticleBeam.from_distribution(quiet_start=True)`:
moments, bunching factor far below 1 / sqrt(N), the keywords through `from_parameters` and `from_twiss`, one block shared by a
batch of covariances, the unchanged `randn` path and a gradient through a quiet beam. One process, no workers.

Every floating-point bound is 4x the deviation measured on an MI355X, which stands in the comment next to it;
the bounds on |b| are fixed: 0.1 / sqrt(N)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.quiet_ref import PRIMES, QUIET_BASES, halton

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
N_BEAM = 65536
SIGMA_TAU = 1e-4


def _quiet(n, bases, offset=0, normal=False, dtype=F64):
    import cheetah_amd as ca

    return ca._ops.quiet_sequence(n, bases, offset=offset, normal=normal, dtype=dtype, device="cuda")


def _bit_equal(a, b):
    it = torch.int64 if a.dtype == F64 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---- 1. the uniforms, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, bases, offset", [
    (5000, QUIET_BASES, 0), (5000, QUIET_BASES, 1), (5000, PRIMES, 0), (5000, PRIMES, 1),
    (16, PRIMES, 2**32 - 8),                                  # crosses the 32-bit boundary
    (16, PRIMES, 2**40 - 17),                                 # the top of the range: the last index is 2^40 - 1
])
def test_uniforms_are_bit_equal_to_the_uint64_restatement(n, bases, offset):
    ref = halton(n, bases, offset)
    got = _quiet(n, bases, offset)
    assert got.shape == (n, len(bases)) and got.dtype == F64
    assert np.array_equal(got.cpu().numpy().view(np.uint64), ref.view(np.uint64))
    got32 = _quiet(n, bases, offset, dtype=F32)
    assert np.array_equal(got32.cpu().numpy().view(np.uint32), ref.astype(np.float32).view(np.uint32))
    assert _bit_equal(_quiet(n, bases, offset), got) and _bit_equal(_quiet(n, bases, offset, dtype=F32), got32)
    assert float(got.min()) > 0 and float(got.max()) < 1


@pytest.mark.parametrize("normal", [False, True])
@pytest.mark.parametrize("dtype", [F64, F32])
def test_rows_of_a_call_equal_a_call_with_an_offset(dtype, normal):
    whole = _quiet(5000, QUIET_BASES, 0, normal, dtype)
    parts = torch.cat([_quiet(2048, QUIET_BASES, 0, normal, dtype), _quiet(5000 - 2048, QUIET_BASES, 2048, normal, dtype)])
    assert _bit_equal(whole, parts)
    assert _bit_equal(_quiet(5000, QUIET_BASES, 0, normal, dtype), whole)


# ---- 2. the normal deviates -----------------------------------------------------------------------------------------------------------
# measured on an MI355X: largest |z - ndtri(u)| / |ndtri(u)| over the cases below, u = 1/2 left out: 8.115e-16 (the tail at
# u = 2^-40: 0)
NORMAL_BOUND = 4 * 8.115e-16


def test_normals_against_ndtri_of_the_exact_uniforms():
    worst = 0.0
    cases = [(5000, PRIMES, 0), (5000, QUIET_BASES, 1), (16, PRIMES, 2**32 - 8), (16, PRIMES, 2**40 - 17),
             (1, (2,), 2**39 - 1)]                            # the deepest tail of the range: u = 2^-40, z = -7.03
    for n, bases, offset in cases:
        u = torch.from_numpy(halton(n, bases, offset))
        ref = torch.special.ndtri(u)
        z = _quiet(n, bases, offset, normal=True)
        assert torch.isfinite(z).all()
        assert _bit_equal(_quiet(n, bases, offset, normal=True, dtype=F32), z.to(F32))       # rounded once on the store
        z = z.cpu()
        assert torch.equal(z < 0, u < 0.5) and torch.equal(z == 0, u == 0.5)
        on = u != 0.5
        dev = float(((z - ref).abs() / ref.abs())[on].max())
        print(f"normals n={n} D={len(bases)} offset={offset}: {dev:.3e}")
        worst = max(worst, dev)
    tail = _quiet(1, (2,), 2**39 - 1, normal=True).cpu()
    assert float(halton(1, (2,), 2**39 - 1)[0, 0]) == 2.0**-40 and -7.1 < float(tail) < -7.0
    first = _quiet(1, (2, 3), 0, normal=True).cpu()
    assert float(first[0, 0]) == 0.0 and not math.copysign(1.0, float(first[0, 0])) < 0           # u = 1/2 gives exactly +0
    print(f"normals: worst {worst:.3e}")
    assert worst <= NORMAL_BOUND


# ---- 3. the quiet beam ----------------------------------------------------------------------------------------------------------------
def _mu_cov(dtype=F64, device="cuda"):
    mu = torch.tensor([1e-5, -2e-6, 3e-5, 1e-6, 2e-5, 1e-4], dtype=dtype, device=device)
    sig = torch.tensor([175e-6, 4e-6, 175e-6, 4e-6, SIGMA_TAU, 2e-3], dtype=dtype, device=device)
    cov = torch.diag(sig.square())
    cov[0, 1] = cov[1, 0] = 0.5 * sig[0] * sig[1]
    cov[2, 3] = cov[3, 2] = -0.3 * sig[2] * sig[3]
    cov[4, 5] = cov[5, 4] = 0.2 * sig[4] * sig[5]
    return mu, cov


@functools.lru_cache(maxsize=None)
def _quiet_beam():
    import cheetah_amd as ca

    mu, cov = _mu_cov()
    return ca.ParticleBeam.from_distribution(mu, cov, N_BEAM, dtype=F64, device="cuda", quiet_start=True)


# measured on an MI355X: largest |mean - mu| / sigma, 6.776e-17, and largest |C_ij - cov_ij| / (sigma_i sigma_j), 1.292e-14, of the
# sample (the whitening makes both exact up to rounding)
MEAN_BOUND = 4 * 6.776e-17
COV_BOUND = 4 * 1.292e-14


def test_quiet_beam_has_the_moments_it_was_given():
    mu, cov = _mu_cov()
    p = _quiet_beam().particles
    assert p.shape == (N_BEAM, 7) and p.dtype == F64 and bool((p[:, 6] == 1).all())
    x = p[:, :6]
    sig = cov.diagonal().sqrt()
    mean = x.mean(dim=0)
    c = (x - mean).mT @ (x - mean) / (N_BEAM - 1)
    dev_mean = float(((mean - mu).abs() / sig).max())
    dev_cov = float(((c - cov).abs() / torch.outer(sig, sig)).max())
    print(f"quiet beam: mean {dev_mean:.3e}, cov {dev_cov:.3e}")
    assert dev_mean <= MEAN_BOUND and dev_cov <= COV_BOUND


def test_quiet_beam_bunching_is_far_below_sampling_noise():
    """|b| <= 0.1 / sqrt(N) = 3.9e-4 at three wavelengths: a CPU float64 run of the scheme gave at most 9.2e-5, drawn deviates give
    about 1e-3 (and this test fails on them, as it does where the keyword does not exist)."""
    lam = [SIGMA_TAU / 5, SIGMA_TAU / 20, SIGMA_TAU / 50]
    b = _quiet_beam().bunching_factor(lam).abs().cpu()
    print("quiet beam |b|:", [f"{float(v):.3e}" for v in b])
    assert b.shape == (3,) and float(b.max()) <= 0.1 / math.sqrt(N_BEAM)


def test_quiet_beam_is_the_same_whatever_the_seed_and_follows_its_offset():
    import cheetah_amd as ca

    mu, cov = _mu_cov()
    make = lambda **kw: ca.ParticleBeam.from_distribution(mu, cov, 4096, dtype=F64, device="cuda", quiet_start=True, **kw).particles  # noqa: E731
    torch.manual_seed(1)
    a = make()
    torch.manual_seed(2)
    assert _bit_equal(make(), a)
    assert _bit_equal(make(sequence_offset=0), a) and not torch.equal(make(sequence_offset=4096), a)


def test_from_parameters_and_from_twiss_hand_the_keywords_through():
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, dtype=F64, device="cuda")  # noqa: E731
    kw = {"dtype": F64, "device": "cuda"}
    sig = [175e-6, 4e-6, 175e-6, 4e-6, SIGMA_TAU, 2e-3]
    names = ["sigma_x", "sigma_px", "sigma_y", "sigma_py", "sigma_tau", "sigma_p"]
    args = {n: t(v) for n, v in zip(names, sig)}
    for offset in (0, 777):
        torch.manual_seed(offset)
        got = ca.ParticleBeam.from_parameters(num_particles=3000, **args, **kw, quiet_start=True, sequence_offset=offset).particles
        torch.manual_seed(offset + 1)
        ref = ca.ParticleBeam.from_distribution(torch.zeros(6, **kw), torch.diag(t(sig).square()), 3000, **kw, quiet_start=True,
                                                sequence_offset=offset).particles
        assert _bit_equal(got, ref), offset
    twiss = dict(num_particles=3000, beta_x=t(5.0), alpha_x=t(0.5), emittance_x=t(1e-9), beta_y=t(3.0), alpha_y=t(-0.2),
                 emittance_y=t(1e-9), sigma_tau=t(SIGMA_TAU), sigma_p=t(1e-3), **kw)
    beams = []
    for seed, offset in ((1, 0), (2, 0), (3, 3000)):
        torch.manual_seed(seed)
        beams.append(ca.ParticleBeam.from_twiss(**twiss, quiet_start=True, sequence_offset=offset).particles)
    assert _bit_equal(beams[0], beams[1]) and not torch.equal(beams[0], beams[2])
    # ranks of a sharded beam: two halves with offsets 0 and N/2 hold the deviates of one whole sequence
    whole = ca._ops.quiet_sequence(3000, QUIET_BASES, dtype=F64)
    halves = torch.cat([ca._ops.quiet_sequence(1500, QUIET_BASES, offset=r * 1500, dtype=F64) for r in range(2)])
    assert _bit_equal(whole, halves)


# measured on an MI355X: largest |row 0 of the batch - the single beam| / sigma = 8.674e-16
SHARED_BLOCK_BOUND = 4 * 8.674e-16


def test_a_batch_of_covariances_shares_one_block():
    """cov, 4 cov, 16 cov: the Cholesky factors are exact multiples, so the rows are exact multiples of one block."""
    import cheetah_amd as ca

    _, cov = _mu_cov()
    covs = torch.stack([cov, 4 * cov, 16 * cov])
    p = ca.ParticleBeam.from_distribution(torch.zeros(6, dtype=F64, device="cuda"), covs, 3000, dtype=F64, device="cuda",
                                          quiet_start=True).particles
    assert p.shape == (3, 3000, 7)
    assert torch.equal(p[1, :, :6], 2 * p[0, :, :6]) and torch.equal(p[2, :, :6], 4 * p[0, :, :6])
    single = ca.ParticleBeam.from_distribution(torch.zeros(6, dtype=F64, device="cuda"), cov, 3000, dtype=F64, device="cuda",
                                               quiet_start=True).particles
    # (a batched product against a single one: other kernels, other orders of the six terms)
    dev = float(((p[0, :, :6] - single[:, :6]).abs() / cov.diagonal().sqrt()).max())
    print(f"row 0 of the batch against a single beam, in sigmas: {dev:.3e}")
    assert dev <= SHARED_BLOCK_BOUND


@pytest.mark.parametrize("dtype", [F64, F32])
def test_without_quiet_start_the_beam_is_todays_bit_for_bit(dtype):
    """`quiet_start=False` is the `randn` composition as it stood: the same call, the same bits under the same torch seed."""
    import cheetah_amd as ca

    n = 5000
    mu, cov = _mu_cov(dtype)
    kw = {"dtype": dtype, "device": "cuda"}
    torch.manual_seed(1234)
    z = torch.randn(n, 6, **kw)
    z = z - z.mean(dim=0, keepdim=True)
    c = (z.mT @ z) / (n - 1)
    z = torch.linalg.solve_triangular(torch.linalg.cholesky(c), z.mT, upper=False).mT
    chol = torch.linalg.cholesky(cov + torch.eye(6, **kw) * torch.finfo(dtype).tiny)
    p6 = z @ chol.mT + mu.unsqueeze(-2)
    ref = torch.cat([p6, torch.ones_like(p6[..., :1])], dim=-1)
    for extra in ({}, {"quiet_start": False}, {"quiet_start": False, "sequence_offset": 5}):
        torch.manual_seed(1234)
        got = ca.ParticleBeam.from_distribution(mu, cov, n, **kw, **extra).particles
        assert _bit_equal(got, ref), extra


# measured on an MI355X: |d sigma_x / d cov_00 - 1 / (2 sigma_x)| (2 sigma_x) = 1.273e-15
GRAD_BOUND = 4 * 1.273e-15


def test_gradient_through_a_quiet_beam():
    import cheetah_amd as ca

    mu, cov = _mu_cov()
    cov.requires_grad_(True)
    mu.requires_grad_(True)
    beam = ca.ParticleBeam.from_distribution(mu, cov, 4096, dtype=F64, device="cuda", quiet_start=True)
    sigma_x = beam.sigma_x
    (sigma_x + beam.mu_y).backward()
    want = 1 / (2 * float(sigma_x.detach()))
    dev = abs(float(cov.grad[0, 0]) - want) / want
    print(f"d sigma_x / d cov_00: {float(cov.grad[0, 0]):.12e} against {want:.12e}: {dev:.3e}")
    assert dev <= GRAD_BOUND
    print(f"d mu_y / d mu_2: {float(mu.grad[2]):.17g}")
    assert float(mu.grad[2]) == 1.0                              # 4096 cotangents of 2^-12: every partial sum is exact
