"""The IBSKick element on the GPU: the generator's words against the integer Philox4x32-10 of `tests/test_sr_host.py` with the
counter word b + 2^31, the kick against a float64 torch restatement of the model (deposit by scatter_add_, V(u) by gather) fed with
the deviates of `_ops.ibs_normals`, edge cases (NaN tau, one tau, an invalid moment), the statistics of the kick against Bane's
closed form and along the bunch, the sequence of calls, gradients (autograd through the restatement with the same deviates), graph
capture and a lattice. One process, no workers.

Every floating-point bound is 4x the deviation measured on an MI355X, which stands in the comment next to it;
the statistical bounds are four standard errors. Deviations are max |got - ref| over max |ref|."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_no_sync import sync_warnings
from tests.test_gpu_synchrotron_radiation import _bit_equal, _np_normals, _np_philox
from tests.test_sr_host import philox4x32_10

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
R_E = 2.8179403205e-15                        # m
M_E = 510998.95069                            # eV
E_CHARGE = 1.602176634e-19                    # C
# the physical case of the host test, compressed: gamma = 500, 1 nm and 100 um in both planes, Lambda = 10
GAMMA, LENGTH, COULOMB_LOG, SIGMA, EPS = 500.0, 100.0, 10.0, 1e-4, 1e-9
CHARGE, SIGMA_TAU = 2.5e-10, 3e-5              # 1 kA peak: V ~ 5.9e-9 there, sigma_delta ~ 7.7e-5 per 100 m


@functools.lru_cache(maxsize=None)
def _mass(dtype=F64):
    """The electron mass in eV as a beam of this dtype hands it to the kernels."""
    import cheetah_amd as ca

    return ca.Species("electron", dtype=dtype).mass_eV_float


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def _strength(energy, length, coulomb_log, sx, sy, ex, ey, mass, absz=1.0):
    """K of the issue in float64, NaN for a row with an invalid moment."""
    e, L, lam, sx, sy, ex, ey = torch.broadcast_tensors(*(t.to(F64) for t in (energy, length, coulomb_log, sx, sy, ex, ey)))
    ok = torch.ones_like(e, dtype=torch.bool)
    for t in (lam, sx, sy, ex, ey):
        ok = ok & (t > 0) & torch.isfinite(t)
    sx, sy, ex, ey = (torch.where(ok, t, torch.ones_like(t)) for t in (sx, sy, ex, ey))
    gamma = e / mass
    alpha = sx * ey / (sy * ex)
    a, b = torch.ones_like(alpha), alpha
    for _ in range(8):
        a, b = (a + b) / 2, torch.sqrt(a * b)
    g = torch.sqrt(alpha) / a
    rc = absz**2 * R_E * M_E / mass
    K = math.sqrt(math.pi) * rc**2 * lam * L * g / (4 * gamma**3 * torch.sqrt(ex * ey * sx * sy) * absz * E_CHARGE)
    return torch.where(ok, K, torch.full_like(K, float("nan")))


def _restate(particles, charges, survival, K, M, xi, details=False):
    """The issue's model in float64 torch: particles (Bx, N, 7), charges (Bq, N), survival (Bw, N), K (B,), xi (B, N) ->
    (B, N, 7). The node grid is a constant; the deposit is a scatter_add_, V(u) a gather."""
    B, N = xi.shape
    x = particles.to(F64).expand(B, N, 7)
    q, w = charges.to(F64).expand(B, N), survival.to(F64).expand(B, N)
    tau, delta = x[..., 4], x[..., 5]
    t0 = tau.detach()
    alive = (w > 0) & torch.isfinite(t0)
    inf = torch.full_like(t0, float("inf"))
    lo, hi = torch.where(alive, t0, inf).amin(-1), torch.where(alive, t0, -inf).amax(-1)
    valid = hi >= lo
    h = torch.where(valid, (hi - lo) / (M - 1), torch.zeros_like(lo))
    live = valid & (h > 0)
    hs = torch.where(live, h, torch.ones_like(h))
    u = ((tau - torch.where(valid, lo, torch.zeros_like(lo))[:, None]) / hs[:, None]).clamp(0.0, float(M - 1))
    u = torch.where(live[:, None], u, torch.zeros_like(u))
    k = torch.nan_to_num(u.detach(), nan=0.0).floor().clamp(max=M - 2).to(torch.int64)
    f = u - k
    c = torch.where(alive, q.abs() * w, torch.zeros_like(w))
    f0 = torch.where(alive, f, torch.zeros_like(f))
    D = torch.zeros(B, M, dtype=F64, device=x.device).scatter_add(1, k, (1 - f0) * c).scatter_add(1, k + 1, f0 * c)
    V = (K.to(F64) / hs)[:, None] * D
    v0, v1 = V.gather(1, k), V.gather(1, k + 1)
    Vu = (1 - f) * v0 + f * v1
    kicked = live[:, None] & ~((v0 == 0) & (v1 == 0)) & (Vu != 0)
    pos = Vu > 0
    root = torch.where(pos, torch.sqrt(torch.where(pos, Vu, torch.ones_like(Vu))), torch.full_like(Vu, float("nan")))
    d1 = torch.where(kicked, delta + root * xi, delta)
    out = torch.cat([x[..., :5], d1[..., None], x[..., 6:]], dim=-1)
    if details:
        return out, torch.where(kicked, Vu, torch.zeros_like(Vu)), live
    return out


def _particles(N, dtype, seed=0, batch=(), sigma_tau=SIGMA_TAU):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*batch, N, 7, generator=g, dtype=F64) * torch.tensor([SIGMA, 1e-5, SIGMA, 1e-5, sigma_tau, 1e-4, 0.0], dtype=F64)
    x[..., 6] = 1.0
    return x.to(dtype).cuda()


def _t(v, dtype=F64):
    return v.to(dtype).cuda() if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=dtype, device="cuda")


def _beam(x, energy=None, charges=None, survival=None):
    import cheetah_amd as ca

    e = _t(GAMMA * _mass(x.dtype), x.dtype) if energy is None else energy
    N = x.shape[-2]
    q = torch.full((N,), CHARGE / N, dtype=x.dtype, device="cuda") if charges is None else charges
    return ca.ParticleBeam(x, e, particle_charges=q, survival_probabilities=survival, dtype=x.dtype, device="cuda")


def _kick(dtype=F64, length=LENGTH, moments=True, **kw):
    import cheetah_amd as ca

    m = dict(sigma_x=_t(SIGMA, dtype), sigma_y=_t(SIGMA, dtype), emittance_x=_t(EPS, dtype), emittance_y=_t(EPS, dtype)) if moments else {}
    m.update(kw)
    return ca.IBSKick(_t(length, dtype), coulomb_log=_t(COULOMB_LOG, dtype), dtype=dtype, device="cuda", **m)


def _K(kick, beam):
    return _strength(beam.energy, kick.effect_length, kick.coulomb_log, kick.sigma_x, kick.sigma_y, kick.emittance_x, kick.emittance_y,
                     _mass(beam.particles.dtype))


def _rel(got, ref):
    return float((got.to(F64) - ref.to(F64)).abs().max() / ref.to(F64).abs().max())


PASS_THROUGH = (0, 1, 2, 3, 4, 6)


# ---- 1. the stream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, stream, call", [(0, 0, 0), (12345, 3, 7), (2**32 - 1, 5, 2**33 + 1)])
def test_stream_words_and_normals(seed, stream, call):
    import cheetah_amd as ca

    worst = 0.0
    for N in (1, 63, 65, 4099):
        for B in (1, 3):
            words, xi = ca._ops.ibs_normals(seed, stream, call, B, N, "cuda")
            assert words.shape == (B, N, 4) and xi.shape == (B, N) and xi.dtype == F64
            sr_words, _ = ca._ops.sr_normals(seed, stream, call, B, N, "cuda")
            assert not bool((words == sr_words).all(dim=-1).any())                 # no draw shared with the radiation kick
            words, xi = words.cpu().numpy(), xi.cpu().numpy()
            ref = np.stack([_np_philox(np.arange(N), b + 2**31, call, seed, stream) for b in range(B)])
            assert np.array_equal(words.astype(np.uint64), ref), (N, B)
            ref_xi = _np_normals(ref)
            worst = max(worst, float(np.max(np.abs(xi - ref_xi) / np.maximum(1.0, np.abs(ref_xi)))))
    n, b = 4098, 2
    assert tuple(int(v) for v in _np_philox(np.array([n]), b + 2**31, call, seed, stream)[0]) == \
        philox4x32_10((n, b + 2**31, call & 0xFFFFFFFF, call >> 32), (seed, stream))
    print(f"normals against the numpy restatement, relative to max(1, |xi|): {worst:.3e}")
    # 64 ulp of max(1, |xi|), as for the radiation kick's draw: the conversion is the same code
    assert worst <= 64 * 2.0 ** -53


# ---- 2. forward ------------------------------------------------------------------------------------------------------------------
# measured on an MI355X, largest over N = 1, 2, 65, 2049, 4099 and M = 2, 65, 200, 4096, of delta' against the restatement:
# float64 1.392e-14 (N = 65: a particle next to a node leaves a deposit of 1e-5 of its charge on the other one, which the 64-bit
# fixed point holds to 2^-62 of the row's charge), float32 2.033e-07 (the arithmetic is float64, rounded once: an ulp of delta)
FORWARD_BOUND = {F64: 4 * 1.392e-14, F32: 4 * 2.033e-07}


def _forward_case(N, M, dtype, seed=3, stream=2, call=4):
    """Particles (1, N, 7) against effect_length (3,) with a row of L = 0, charges (3, N), survival (N,) with zeros mixed in."""
    import cheetah_amd as ca

    g = torch.Generator().manual_seed(1000 * N + M)
    x = _particles(N, dtype, seed=N + M, batch=(1,))
    q = (CHARGE / N * (0.5 + torch.rand(3, N, generator=g, dtype=F64))).to(dtype).cuda()
    w = torch.where(torch.rand(N, generator=g) < 0.2, 0.0, 1.0).to(dtype).cuda() * torch.rand(N, generator=g, dtype=F64).to(dtype).cuda()
    w[:2] = 1.0
    L = _t([LENGTH, 0.0, 0.3 * LENGTH], dtype)
    kick = _kick(dtype, length=L, num_bins=M, seed=seed, stream=stream)
    kick.reseed(call_index=call)
    beam = _beam(x, charges=q, survival=w)
    out = kick.track(beam).particles
    _, xi = ca._ops.ibs_normals(seed, stream, call, 3, N, "cuda")
    ref, Vu, live = _restate(x, q, w[None], _K(kick, beam), M, xi, details=True)
    return x, out, ref, Vu, live


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("N", [1, 2, 65, 2049, 4099])
def test_forward_against_the_restatement(N, dtype):
    worst = 0.0
    for M in (2, 65, 200, 4096):
        x, out, ref, Vu, live = _forward_case(N, M, dtype)
        assert out.shape == (3, N, 7) and out.dtype == dtype
        for c in PASS_THROUGH:
            assert _bit_equal(out[..., c], x[..., c].expand(3, N)), (M, c)
        assert _bit_equal(out[1], x[0]), M                                          # the row with L = 0: every column
        unkicked = (Vu == 0)
        assert _bit_equal(out[..., 5][unkicked], x[..., 5].expand(3, N)[unkicked]), M
        assert torch.isfinite(out).all()
        if bool(live[0]):
            assert float((out[0, :, 5] - x[0, :, 5]).abs().max()) > 0, M
            assert not torch.equal(out[0, :, 5], out[2, :, 5])
            worst = max(worst, _rel(out[..., 5].to(F64) - x[..., 5].to(F64), ref[..., 5] - x[..., 5].to(F64)))
        else:
            assert N == 1 and _bit_equal(out, x.expand(3, N, 7))                    # one particle: no grid, no kick
    print(f"forward N={N} {dtype}: the kick's deviation {worst:.3e}")
    assert worst <= FORWARD_BOUND[dtype]


# ---- 3. edge cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_nan_tau_one_tau_and_an_invalid_moment(dtype):
    N, M = 257, 65
    x = _particles(N, dtype, seed=5)
    clean = _kick(dtype, num_bins=M).track(_beam(x)).particles
    # a NaN tau: that particle's delta is NaN (its V(u) is), it deposits nothing, and nobody else notices beyond its missing charge
    x2 = x.clone()
    x2[100, 4] = float("nan")
    w = torch.ones(N, dtype=dtype, device="cuda")
    w[100] = 0.0
    out = _kick(dtype, num_bins=M).track(_beam(x2)).particles
    without = _kick(dtype, num_bins=M).track(_beam(x, survival=w)).particles
    assert torch.isnan(out[100, 5]) and _bit_equal(out[100, list(PASS_THROUGH)], x2[100, list(PASS_THROUGH)])
    others = [n for n in range(N) if n != 100]
    assert _bit_equal(out[others], without[others]) and torch.isfinite(out[others]).all()
    # all particles at one tau: no grid, no kick
    x3 = x.clone()
    x3[:, 4] = 1e-5
    kick = _kick(dtype, num_bins=M)
    assert _bit_equal(kick.track(_beam(x3)).particles, x3)
    assert kick.call_index == 1                                                     # the call is counted all the same
    # a non-positive sigma_x: that row's delta is NaN, the other rows are untouched
    kick = _kick(dtype, num_bins=M, sigma_x=_t([SIGMA] * 4, dtype))
    kick.sigma_x.copy_(_t([SIGMA, -SIGMA, SIGMA, 0.0], dtype))                       # the constructor refuses them: edited in place
    out = kick.track(_beam(x)).particles
    assert out.shape == (4, N, 7)
    for b in (1, 3):
        assert torch.isnan(out[b, :, 5]).all() and _bit_equal(out[b][:, list(PASS_THROUGH)], x[:, list(PASS_THROUGH)])
    assert _bit_equal(out[0], clean) and torch.isfinite(out[2]).all() and not torch.equal(out[2, :, 5], clean[:, 5])


# ---- 4. statistics ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gaussian_bunch(seed):
    """N = 2^18 particles, Gaussian in tau, delta = 0, explicit moments, M = 200: (tau, delta', V(u_n) of the restatement, K)."""
    N = 2**18
    x = _particles(N, F64, seed=100 + seed)
    x[:, 5] = 0.0
    kick = _kick(F64, num_bins=200, seed=seed)
    beam = _beam(x)
    out = kick.track(beam).particles
    K = _K(kick, beam).reshape(1)
    _, Vu, _ = _restate(x[None], beam.particle_charges[None], torch.ones(1, N, dtype=F64, device="cuda"), K, 200,
                        torch.zeros(1, N, dtype=F64, device="cuda"), details=True)
    return x[:, 4], out, Vu[0], float(K)


@pytest.mark.parametrize("seed", [0, 1])
def test_variance_follows_banes_formula(seed):
    tau, out, Vu, K = _gaussian_bunch(seed)
    N = tau.numel()
    d = out[:, 5]
    mean_V = float(Vu.mean())
    bane = K * CHARGE / (2 * math.sqrt(math.pi) * float(tau.std()))
    assert abs(K * CHARGE / (math.sqrt(2 * math.pi) * SIGMA_TAU) / 5.86e-9 - 1) < 0.01      # the physical case: 1 kA at the peak
    var_err = abs(float(d.var(unbiased=False)) / mean_V - 1) / math.sqrt(2 / N)
    # a mixture of normals of variances V_n: Var(d^2) = 3 <V^2> - <V>^2 rather than 2 <V>^2
    mix_err = abs(float(d.square().mean()) - mean_V) / math.sqrt(float(3 * Vu.square().mean() - mean_V**2) / N)
    z = d / Vu.sqrt()
    mean_err = abs(float(z.mean())) * math.sqrt(N)
    kurt_err = abs(float((z**4).mean() / z.square().mean() ** 2) - 3) / math.sqrt(24 / N)
    print(f"seed {seed}: variance {var_err:.2f} (mixture {mix_err:.2f}), mean {mean_err:.2f}, kurtosis {kurt_err:.2f} standard errors; "
          f"the restatement's mean V against Bane's closed form {abs(mean_V / bane - 1):.2e}")
    assert float(Vu.min()) > 0
    assert var_err <= 4 and mean_err <= 4 and kurt_err <= 4
    assert abs(mean_V / bane - 1) <= 0.01


@pytest.mark.parametrize("seed", [0, 1])
def test_slice_variance_follows_the_local_density(seed):
    import cheetah_amd as ca

    tau, out, Vu, _ = _gaussian_bunch(seed)
    beam = _beam(out)
    S = 9
    slices = beam.slice_statistics(num_slices=S, tau_range=(-2 * SIGMA_TAU, 2 * SIGMA_TAU))
    got = slices.beam.sigma_p.square().to(F64)
    assert got.shape == (S,)
    idx = torch.bucketize(tau.contiguous(), slices.edges.to(F64).contiguous()) - 1
    worst = 0.0
    for s in range(S):
        v = Vu[idx == s]
        n = v.numel()
        assert n > 1000
        se = math.sqrt(float(3 * v.square().mean() - v.mean() ** 2) / n)
        worst = max(worst, abs(float(got[s]) - float(v.mean())) / se)
    print(f"seed {seed}: slice variance against the restatement's slice mean of V, worst of {S} slices: {worst:.2f} standard errors; "
          f"centre / edge {float(got[S // 2] / got[0]):.2f}")
    assert worst <= 4
    assert float(got[S // 2]) > 3 * float(got[0]) and float(got[S // 2]) > 3 * float(got[-1])     # exp(-1.6) at the edge slices' centres
    assert isinstance(slices, ca.particles.slices.BeamSlices)


# ---- 5. sequence -----------------------------------------------------------------------------------------------------------------
def test_sequence_of_calls_reseed_clone_and_streams():
    import cheetah_amd as ca

    N = 2**14
    x = _particles(N, F64, seed=8)
    x[:, 5] = 0.0
    beam = _beam(x)
    kick = _kick(F64, seed=21)
    run1 = [kick.track(beam).particles for _ in range(3)]
    assert kick.call_index == 3
    for i in range(3):
        for j in range(i):
            assert not torch.equal(run1[i][:, 5], run1[j][:, 5])
    kick.reseed()
    first = kick.track(beam).particles
    twin = kick.clone()                                         # taken after track 1: it goes on with track 2
    assert twin.call_index == 1
    run2 = [first] + [kick.track(beam).particles for _ in range(2)]
    for u, v in zip(run1, run2):
        assert _bit_equal(u, v)
    assert _bit_equal(twin.track(beam).particles, run1[1])
    kick.reseed(seed=22)
    assert not torch.equal(kick.track(beam).particles[:, 5], run1[0][:, 5])
    # two kicks with different streams, and two calls of one kick: uncorrelated within four standard errors
    other = _kick(F64, seed=21, stream=1).track(beam).particles

    def corr(u, v):
        u, v = u - u.mean(), v - v.mean()
        return float((u * v).mean() / (u.std(unbiased=False) * v.std(unbiased=False)))

    streams, calls = corr(run1[0][:, 5], other[:, 5]), corr(run1[0][:, 5], run1[1][:, 5])
    print(f"correlation between streams {streams:.2e}, between calls {calls:.2e}, 1 / sqrt(N) = {1 / math.sqrt(N):.2e}")
    assert abs(streams) <= 4 / math.sqrt(N) and abs(calls) <= 4 / math.sqrt(N)
    # xi of particle n does not depend on N
    a, b = ca._ops.ibs_normals(21, 0, 0, 3, 64, "cuda")[1], ca._ops.ibs_normals(21, 0, 0, 3, 65, "cuda")[1]
    assert _bit_equal(b[:, :64], a)


# ---- 6. gradients ----------------------------------------------------------------------------------------------------------------
# measured on an MI355X against autograd through the restatement, largest over N = 65, 2049 and M = 65, 4096:
# float64 tau 1.472e-14, delta 0, charges 7.694e-16, survival 9.995e-16, energy 4.456e-16, effect_length 8.738e-16, coulomb_log
# 4.389e-16, sigma_x 3.392e-16, sigma_y 7.763e-16, emittance_x 6.783e-16, emittance_y 4.445e-16; float32 tau 8.471e-08, delta
# 8.610e-08, charges 1.066e-07, survival 8.856e-08 (sums over the three rows formed in float32) and 0 for the seven settings: their
# float64 gradients agree as in the float64 case and both sides round them once to float32, to the same bits
GRAD_NAMES = ("tau", "delta", "charges", "survival", "energy", "effect_length", "coulomb_log", "sigma_x", "sigma_y", "emittance_x",
              "emittance_y")
GRAD_BOUND = {F64: {"tau": 4 * 1.472e-14, "delta": 0.0, "charges": 4 * 7.694e-16, "survival": 4 * 9.995e-16, "energy": 4 * 4.456e-16,
                    "effect_length": 4 * 8.738e-16, "coulomb_log": 4 * 4.389e-16, "sigma_x": 4 * 3.392e-16, "sigma_y": 4 * 7.763e-16,
                    "emittance_x": 4 * 6.783e-16, "emittance_y": 4 * 4.445e-16},
              F32: {**dict.fromkeys(GRAD_NAMES, 0.0), "tau": 4 * 8.471e-08, "delta": 4 * 8.610e-08, "charges": 4 * 1.066e-07,
                    "survival": 4 * 8.856e-08}}
# the four moments taken from the beam: the gradient arrives in the particles and the survival probabilities. Measured, largest over
# the six coordinates and the survival probabilities: float64 1.270e-14, float32 1.977e-07
BEAM_GRAD_BOUND = {F64: 4 * 1.270e-14, F32: 4 * 1.977e-07}


def _grad_inputs(N, M, dtype):
    g = torch.Generator().manual_seed(N + M)
    leaf = lambda v: v.clone().requires_grad_(True)  # noqa: E731
    x = leaf(_particles(N, dtype, seed=N + M + 1, batch=(1,)))
    q = leaf((CHARGE / N * (0.5 + torch.rand(3, N, generator=g, dtype=F64))).to(dtype).cuda())
    w0 = torch.where(torch.rand(N, generator=g) < 0.2, 0.0, 1.0).to(F64) * (0.25 + 0.75 * torch.rand(N, generator=g, dtype=F64))
    w0[:3] = 1.0
    w = leaf(w0.to(dtype).cuda())
    W = torch.randn(3, N, 7, generator=g, dtype=F32).to(F64).cuda()         # float32 values: the same cotangent for either beam dtype
    e = leaf(_t(GAMMA * _mass(dtype), dtype))
    L = leaf(_t([LENGTH, 0.0, 0.3 * LENGTH], dtype))
    return x, q, w, W, e, L


def _gradients(N, M, dtype, through_kernel):
    import cheetah_amd as ca

    x, q, w, W, e, L = _grad_inputs(N, M, dtype)
    leaf = lambda v: _t(v, dtype).requires_grad_(True)  # noqa: E731
    s = {"coulomb_log": leaf(COULOMB_LOG), "sigma_x": leaf(1.5 * SIGMA), "sigma_y": leaf(SIGMA), "emittance_x": leaf(EPS),
         "emittance_y": leaf(2 * EPS)}
    if through_kernel:
        par = lambda v: torch.nn.Parameter(v.detach().clone())  # noqa: E731
        kick = ca.IBSKick(par(L), **{k: par(v) for k, v in s.items()}, num_bins=M, seed=5, stream=1, dtype=dtype, device="cuda")
        kick.reseed(call_index=2)
        beam = ca.ParticleBeam(x, e, particle_charges=q, survival_probabilities=w, dtype=dtype, device="cuda")
        out = kick.track(beam).particles
        assert out.shape == (3, N, 7) and out.dtype == dtype
        L, s = kick.effect_length, {k: getattr(kick, k) for k in s}
    else:
        _, xi = ca._ops.ibs_normals(5, 1, 2, 3, N, "cuda")
        K = _strength(e, L, s["coulomb_log"], s["sigma_x"], s["sigma_y"], s["emittance_x"], s["emittance_y"], _mass(dtype))
        out = _restate(x, q, w[None], K, M, xi)
    (out.to(F64) * W).sum().backward()
    grads = {"tau": x.grad[..., 4], "delta": x.grad[..., 5], "charges": q.grad, "survival": w.grad, "energy": e.grad,
             "effect_length": L.grad, **{k: v.grad for k, v in s.items()}}
    return grads, x.grad, (x.detach(), q.detach(), w.detach())


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("N, M", [(65, 65), (65, 4096), (2049, 65), (2049, 4096)])
def test_gradients_against_autograd_of_the_restatement(N, M, dtype):
    got, gx, (x, q, w) = _gradients(N, M, dtype, True)
    ref, rx, _ = _gradients(N, M, dtype, False)
    again, ax, _ = _gradients(N, M, dtype, True)
    assert gx.shape == (1, N, 7) and got["charges"].shape == (3, N) and got["survival"].shape == (N,) and got["energy"].shape == () \
        and got["effect_length"].shape == (3,) and got["sigma_x"].shape == ()
    assert _bit_equal(gx, ax)
    for name in GRAD_NAMES:
        assert got[name].dtype == dtype, name
        assert _bit_equal(got[name], again[name]), name                       # two backward runs
        assert torch.isfinite(got[name]).all(), name
    # the columns that only pass their cotangent on, summed over the three rows in the beam's dtype: two roundings of partial sums
    # of at most 3 max |W| against a largest sum of about 1.5 max |W| -> 4 ulp; twice that
    for c in (0, 1, 2, 3, 6):
        assert _rel(gx[..., c], rx[..., c]) <= 8 * torch.finfo(dtype).eps, c
    assert float(got["effect_length"][1]) == 0.0                              # the row with L = 0: no gradient through V = 0
    devs = {name: _rel(got[name], ref[name]) for name in GRAD_NAMES}
    print(f"gradients N={N} M={M} {dtype}: " + ", ".join(f"{k} {v:.3e}" for k, v in devs.items()))
    for name, dev in devs.items():
        assert dev <= GRAD_BOUND[dtype][name], name


@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_particle_without_variance_has_zero_gradients(dtype):
    """Dead particles far from every live one sit between empty nodes: V(u) = 0, delta keeps its bits and nothing but the cotangent
    that passes through comes back; a row with L = 0 likewise."""
    import cheetah_amd as ca

    N, M = 65, 4096
    x = _particles(N, dtype, seed=12)
    x[:8, 4] = torch.linspace(-3.9, -3.2, 8, dtype=F64).to(dtype).cuda() * SIGMA_TAU * 0.5
    x[8, 4], x[9, 4] = -2.0 * SIGMA_TAU, 2.0 * SIGMA_TAU
    x[10:, 4] = x[10:, 4].clamp(-SIGMA_TAU, SIGMA_TAU) * 0.1 + SIGMA_TAU
    w = torch.ones(N, dtype=dtype, device="cuda")
    w[:8] = 0.0
    x, w = x.requires_grad_(True), w.requires_grad_(True)
    L = _t([LENGTH, 0.0], dtype).requires_grad_(True)
    kick = ca.IBSKick(L, sigma_x=_t(SIGMA, dtype), sigma_y=_t(SIGMA, dtype), emittance_x=_t(EPS, dtype), emittance_y=_t(EPS, dtype),
                      coulomb_log=_t(COULOMB_LOG, dtype), num_bins=M, dtype=dtype, device="cuda")
    out = kick.track(_beam(x, survival=w)).particles
    assert _bit_equal(out[0, :8], x[:8].detach()) and _bit_equal(out[1], x.detach())
    assert float((out[0, 8:, 5] - x[8:, 5]).detach().abs().min()) > 0
    W = torch.arange(1, 2 * N * 7 + 1, dtype=dtype, device="cuda").reshape(2, N, 7)
    (out * W).sum().backward()
    assert torch.isfinite(x.grad).all() and torch.isfinite(w.grad).all() and torch.isfinite(L.grad).all()
    assert torch.equal(x.grad[:8], (W[0, :8] + W[1, :8]))                     # the cotangent passes through, nothing is added
    assert torch.equal(w.grad[:8], torch.zeros_like(w.grad[:8]))
    assert float(L.grad[1]) == 0.0 and float(L.grad[0]) != 0.0
    assert float(x.grad[8:, 4].abs().max()) > 0


def _beam_moment_gradients(N, M, dtype, through_kernel):
    """The four moments taken from the beam (`None`): d(sum(out * W)) / d(particles, survival) with the moments' graphs."""
    import cheetah_amd as ca

    x, q, w, W, e, L = _grad_inputs(N, M, dtype)
    q = q.detach()[0]
    beam = ca.ParticleBeam(x[0], e, particle_charges=q, survival_probabilities=w, dtype=dtype, device="cuda")
    if through_kernel:
        kick = ca.IBSKick(L, coulomb_log=_t(COULOMB_LOG, dtype), num_bins=M, seed=5, stream=1, dtype=dtype, device="cuda")
        kick.reseed(call_index=2)
        out = kick.track(beam).particles
        assert out.shape == (3, N, 7)
    else:
        _, xi = ca._ops.ibs_normals(5, 1, 2, 3, N, "cuda")
        K = _strength(e, L, _t(COULOMB_LOG, dtype), beam.sigma_x, beam.sigma_y, beam.emittance_x, beam.emittance_y, _mass(dtype))
        out = _restate(x, q[None], w[None], K, M, xi)
    (out.to(F64) * W).sum().backward()
    return x.grad, w.grad


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("N, M", [(65, 65), (2049, 4096)])
def test_gradients_through_the_beams_own_moments(N, M, dtype):
    got, ref, again = (_beam_moment_gradients(N, M, dtype, k) for k in (True, False, True))
    assert _bit_equal(got[0], again[0]) and _bit_equal(got[1], again[1])
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    # x, px, y, py get a gradient only through the moments
    assert float(got[0][..., 0].abs().max()) > 0 and float(got[0][..., 3].abs().max()) > 0
    dev = max(max(_rel(got[0][..., c], ref[0][..., c]) for c in range(6)), _rel(got[1], ref[1]))
    print(f"gradients through the beam's moments N={N} M={M} {dtype}: {dev:.3e}")
    assert dev <= BEAM_GRAD_BOUND[dtype]


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------
def test_graph_capture_follows_the_call_index_and_the_length_without_synchronising():
    import cheetah_amd as ca

    beam = _beam(_particles(2049, F32, seed=10))
    kick = _kick(F32, seed=31, stream=2, moments=False)                             # the moments from the beam: inside the graph
    with torch.no_grad():
        assert not sync_warnings(lambda: kick.track(beam).particles)
        step = ca.graph.capture(lambda: kick.track(beam).particles)
        index = kick.call_index
        twin = kick.clone()
        twin.reseed(call_index=index)
        replays = []
        for _ in range(2):
            replays.append(step().clone())
            assert _bit_equal(replays[-1], twin.track(beam).particles)
        assert not torch.equal(replays[0][:, 5], replays[1][:, 5])
        assert kick.call_index == index + 2
        assert not sync_warnings(step, warm=0)
        twin.reseed(call_index=kick.call_index)
        # an in-place edit of a setting between replays is followed
        unedited = twin.clone()
        kick.effect_length.mul_(4.0)
        twin.effect_length.mul_(4.0)
        third = step().clone()
        assert _bit_equal(third, twin.track(beam).particles)
        assert not torch.equal(third[:, 5], unedited.track(beam).particles[:, 5])


# ---- 8. in a lattice -------------------------------------------------------------------------------------------------------------
def _walk(elements, beam):
    for e in elements:
        beam = e.track(beam)
    return beam


def test_in_a_lattice_equals_the_element_walk():
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(3)
    beam = ca.ParticleBeam.from_parameters(num_particles=10_000, sigma_x=t(1e-4), sigma_y=t(1e-4), sigma_px=t(1e-5), sigma_py=t(1e-5),
                                           sigma_tau=t(SIGMA_TAU), sigma_p=t(1e-5), energy=t(GAMMA * _mass()), total_charge=t(CHARGE), **kw)
    seg = ca.Segment([ca.Drift(t(30.0), name="d1", **kw), ca.Quadrupole(t(0.2), k1=t(0.5), name="q", **kw),
                      ca.Drift(t(20.0), name="d2", **kw)]).with_ibs_kicks(max_step=15.0, seed=6)
    els = list(seg.elements)
    assert [type(e).__name__ for e in els] == ["Drift", "IBSKick"] * 2 + ["Quadrupole", "IBSKick"] + ["Drift", "IBSKick"] * 2
    kicks = [e for e in els if isinstance(e, ca.IBSKick)]
    assert [k.stream for k in kicks] == [0, 1, 2, 3, 4]
    with torch.no_grad():
        got = seg.track(beam)
        assert [k.call_index for k in kicks] == [1] * 5
        for k in kicks:
            k.reseed()
        ref = _walk(els, beam)
        quiet = _walk([e for e in els if not isinstance(e, ca.IBSKick)], beam)
    assert torch.isfinite(got.particles).all()
    assert _bit_equal(got.particles, ref.particles) and torch.equal(got.s, ref.s)
    # the spread is there: 50 m at about 1 kA, sigma_delta^2 = 1e-10 before
    grown, before = float(got.sigma_p) ** 2, float(quiet.sigma_p) ** 2
    print(f"sigma_delta^2 {before:.3e} -> {grown:.3e}")
    assert grown > 2 * before
