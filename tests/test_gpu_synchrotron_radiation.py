"""The SynchrotronRadiationKick element on the GPU: the generator's words against the integer Philox4x32-10 of
`tests/test_sr_host.py` and its deviates against a numpy restatement, the kick against a float64 torch restatement of the formulas fed
with the deviates of `_ops.sr_normals`, the switches (no excitation, L = 0, theta = 0, NaN), the statistics of the deviates, the
sequence of calls, gradients (autograd through the restatement with the same deviates), graph capture and a lattice. One process,
no workers.

Every floating-point bound is 4x the deviation measured on an MI355X, which stands in the comment next to it;
the statistical bounds are four standard errors. Deviations are per column: max |got - ref| over max |ref|."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_sr_host import philox4x32_10

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
ENERGY, LENGTH, ANGLE = 5e9, 0.5, 0.05        # the physical case: electrons, mean loss ~ 44 keV, rms ~ 40 keV per kick
R_E = 2.8179403205e-15                        # m
M_E = 510998.95069                            # eV
HBAR_C = 1.973269804593025e-7                 # eV m
QUANTUM = 55 / (24 * math.sqrt(3))


@functools.lru_cache(maxsize=None)
def _mass(dtype=F64):
    """The electron mass in eV as a beam of this dtype hands it to the kernels."""
    import cheetah_amd as ca

    return ca.Species("electron", dtype=dtype).mass_eV_float


# ---- restatements ----------------------------------------------------------------------------------------------------------------
def _np_philox(n, b, call, seed, stream):
    """Philox4x32-10 on numpy uint64 arrays holding 32-bit values: counter (n, b, call_lo, call_hi), key (seed, stream)."""
    m32 = np.uint64(0xFFFFFFFF)
    c0 = np.asarray(n, dtype=np.uint64)
    c1 = np.full_like(c0, b)
    c2 = np.full_like(c0, call & 0xFFFFFFFF)
    c3 = np.full_like(c0, call >> 32)
    k0, k1 = seed, stream
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1)


def _np_cospi(t):
    """cos(pi t) for 0 <= t <= 2 in float64, the argument reduced exactly to [0, 1/4] before pi is multiplied in."""
    s = np.abs(t - 2.0 * np.round(t / 2.0))                    # in [0, 1], exact
    flip = s > 0.5
    s = np.where(flip, 1.0 - s, s)                             # cos(pi s) = -cos(pi (1 - s)); in [0, 1/2], exact
    c = np.where(s > 0.25, np.sin(np.pi * (0.5 - s)), np.cos(np.pi * s))
    return np.where(flip, -c, c)


def _np_normals(words):
    w = words.astype(np.uint64)
    k1 = ((w[..., 0] << np.uint64(32)) | w[..., 1]) >> np.uint64(11)
    k2 = ((w[..., 2] << np.uint64(32)) | w[..., 3]) >> np.uint64(11)
    u1, u2 = (k1.astype(np.float64) + 0.5) * 2.0 ** -53, (k2.astype(np.float64) + 0.5) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * _np_cospi(2.0 * u2)


def _factors(energy, length, angle, mass, absz=1.0):
    """(gamma0, P0, a, b) in float64, every one of the broadcast batch shape."""
    e, L, th = torch.broadcast_tensors(energy.to(F64), length.to(F64), angle.to(F64))
    gamma = e / mass
    P0 = (1 - gamma.square().reciprocal()).clamp_min(0).sqrt() * gamma
    rc, lc = absz**2 * R_E * M_E / mass, HBAR_C / mass
    kicks = (L != 0) & (th != 0)
    Ls = torch.where(kicks, L, torch.ones_like(L))
    a = torch.where(kicks, (2 / 3) * rc * th**2 / Ls, torch.zeros_like(L))
    b = torch.where(kicks, QUANTUM * rc * lc * th.abs() ** 3 / Ls**2, torch.zeros_like(L))
    return gamma, P0, a, b


def _restate(particles, energy, length, angle, xi, mass, excite=True):
    """The issue's formulas in float64 torch: particles (*, N, 7), settings of batch shapes, xi (*batch, N) -> (*batch, N, 7)."""
    gamma, P0, a, b = (t[..., None] for t in _factors(energy, length, angle, mass))
    x = particles.to(F64)
    x = x.expand(*gamma.shape[:-1], *x.shape[-2:])
    px, py, delta = x[..., 1], x[..., 3], x[..., 5]
    g = gamma + delta * P0
    pi = torch.sqrt(g**2 - 1)
    g1 = g - a * P0**2 * pi * g
    if excite:
        g1 = g1 - torch.sqrt(b * P0**3 * g**7 / pi**3) * xi
    d1 = delta + (g1 - g) / P0
    pi1 = torch.sqrt(g1**2 - 1)
    cols = list(x.unbind(-1))
    cols[1], cols[3], cols[5] = px * pi1 / pi, py * pi1 / pi, d1
    out = torch.stack(cols, dim=-1)
    keep = ((a == 0) & (b == 0))[..., None]                     # a row that is not kicked keeps its bits
    return torch.where(keep, x, out)


def _particles(N, dtype, seed=0, batch=()):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*batch, N, 7, generator=g, dtype=F64) * torch.tensor([1e-4, 1e-4, 1e-4, 1e-4, 1e-4, 1e-3, 0.0], dtype=F64)
    x[..., 6] = 1.0
    return x.to(dtype).cuda()


def _beam(x, energy=ENERGY):
    import cheetah_amd as ca

    e = energy if isinstance(energy, torch.Tensor) else torch.tensor(energy, dtype=x.dtype, device="cuda")
    return ca.ParticleBeam(x, e, dtype=x.dtype, device="cuda")


def _kick(dtype=F64, length=LENGTH, angle=ANGLE, **kw):
    import cheetah_amd as ca

    t = lambda v: v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=dtype, device="cuda")  # noqa: E731
    return ca.SynchrotronRadiationKick(t(length), t(angle), dtype=dtype, device="cuda", **kw)


def _dev(got, ref, cols=(1, 3, 5)):
    """Per column: max |got - ref| / max |ref| -> the largest over `cols`."""
    got, ref = got.to(F64).reshape(-1, 7), ref.to(F64).reshape(-1, 7)
    return max(float((got[:, c] - ref[:, c]).abs().max() / ref[:, c].abs().max()) for c in cols)


def _rel(got, ref):
    return float((got.to(F64) - ref.to(F64)).abs().max() / ref.to(F64).abs().max())


PASS_THROUGH = (0, 2, 4, 6)


def _bit_equal(a, b):
    """Equal as bits (NaN payloads and signed zeros included)."""
    it = torch.int64 if a.dtype == F64 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---- 1. the stream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, stream, call", [(0, 0, 0), (12345, 0, 7), (2**32 - 1, 5, 2**33 + 1)])
def test_stream_words_and_normals(seed, stream, call):
    import cheetah_amd as ca

    worst = 0.0
    draws = {}
    for N in (1, 63, 64, 65, 257, 4099):
        for B in (1, 3):
            words, xi = ca._ops.sr_normals(seed, stream, call, B, N, "cuda")
            assert words.shape == (B, N, 4) and xi.shape == (B, N) and xi.dtype == F64
            words, xi = words.cpu().numpy(), xi.cpu().numpy()
            draws[N, B] = xi
            ref = np.stack([_np_philox(np.arange(N), b, call, seed, stream) for b in range(B)])
            assert np.array_equal(words.astype(np.uint64), ref), (N, B)
            ref_xi = _np_normals(ref)
            worst = max(worst, float(np.max(np.abs(xi - ref_xi) / np.maximum(1.0, np.abs(ref_xi)))))
    # the vectorised Philox above is the integer one of the host tests
    n, b = 4098, 2
    assert tuple(int(v) for v in _np_philox(np.array([n]), b, call, seed, stream)[0]) == \
        philox4x32_10((n, b, call & 0xFFFFFFFF, call >> 32), (seed, stream))
    print(f"normals against the numpy restatement, relative to max(1, |xi|): {worst:.3e}")
    # 64 ulp of max(1, |xi|): a few ulp each for log, sqrt and cospi times the condition of the product is far below
    assert worst <= 64 * 2.0 ** -53
    # xi of particle n does not depend on N
    for B in (1, 3):
        assert np.array_equal(draws[65, B][:, :64].view(np.uint64), draws[64, B].view(np.uint64))


# ---- 2. forward ------------------------------------------------------------------------------------------------------------------
# measured on an MI355X, largest over the cases below of each dtype (N = 1, 65, 1025 and the two broadcasts): float64 3.888e-16,
# float32 4.677e-08 (under one float32 ulp of the column's largest value: the arithmetic is float64, rounded once)
FORWARD_BOUND = {F64: 4 * 3.888e-16, F32: 4 * 4.677e-08}


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("N", [1, 65, 1025])
def test_forward_against_the_restatement(N, dtype):
    import cheetah_amd as ca

    x = _particles(N, dtype, seed=N)
    kick = _kick(dtype, seed=3, stream=2)
    kick.reseed(call_index=4)
    out = kick.track(_beam(x)).particles
    assert out.shape == (N, 7) and out.dtype == dtype
    _, xi = ca._ops.sr_normals(3, 2, 4, 1, N, "cuda")
    e = torch.tensor(ENERGY, dtype=dtype, device="cuda")
    ref = _restate(x, e, kick.effect_length, kick.angle, xi[0], _mass(dtype))
    for c in PASS_THROUGH:
        assert _bit_equal(out[:, c], x[:, c]), c
    assert float((out[:, 5] - x[:, 5]).abs().max()) > 0 and torch.isfinite(out).all()
    dev = _dev(out, ref)
    print(f"forward N={N} {dtype}: {dev:.3e}")
    assert dev <= FORWARD_BOUND[dtype]


@pytest.mark.parametrize("dtype", [F64, F32])
def test_forward_broadcast_shapes(dtype):
    import cheetah_amd as ca

    N = 65
    call = torch.tensor([6], dtype=torch.int64, device="cuda")
    t = lambda v: torch.tensor(v, dtype=dtype, device="cuda")  # noqa: E731
    mass = _mass(dtype)
    devs = []
    # particles (1, N, 7) against angle (3,)
    x = _particles(N, dtype, seed=1, batch=(1,))
    th = t([0.05, -0.03, 0.08])
    out = ca._ops.sr_kick(x, t(ENERGY), mass, 1.0, t(LENGTH), th, True, 9, 1, call)
    assert out.shape == (3, N, 7)
    _, xi = ca._ops.sr_normals(9, 1, 6, 3, N, "cuda")
    devs.append(_dev(out, _restate(x, t(ENERGY), t(LENGTH), th, xi, mass)))
    for c in PASS_THROUGH:
        assert _bit_equal(out[..., c], x[..., c].expand(3, N))
    assert not torch.equal(out[0, :, 5], out[1, :, 5])
    # energy (2, 1) against length (1, 3): flat batch row b = 3 i + j
    x = _particles(N, dtype, seed=2)
    e, L = t([[5e9], [3e9]]), t([[0.5, 0.25, 1.0]])
    out = ca._ops.sr_kick(x, e, mass, 1.0, L, t(ANGLE), True, 9, 1, call)
    assert out.shape == (2, 3, N, 7)
    xi = ca._ops.sr_normals(9, 1, 6, 6, N, "cuda")[1].reshape(2, 3, N)
    devs.append(_dev(out, _restate(x, e, L, t(ANGLE), xi, mass)))
    for c in PASS_THROUGH:
        assert _bit_equal(out[..., c], x[..., c].expand(2, 3, N))
    print(f"forward broadcast {dtype}: {max(devs):.3e}")
    assert max(devs) <= FORWARD_BOUND[dtype]


# ---- 3. switches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_without_excitation_nothing_is_drawn(dtype):
    x = _particles(1025, dtype, seed=5)
    beam = _beam(x)
    kick = _kick(dtype, quantum_excitation=False, seed=1)
    a = kick.track(beam).particles
    kick.reseed(seed=77, call_index=123)
    b = kick.track(beam).particles
    assert _bit_equal(a, b)
    assert kick.call_index == 123                               # not advanced: nothing was drawn
    ref = _restate(x, beam.energy, kick.effect_length, kick.angle, None, _mass(dtype), excite=False)
    dev = _dev(a, ref)
    print(f"forward without excitation {dtype}: {dev:.3e}")
    assert dev <= FORWARD_BOUND[dtype]
    assert float((a[:, 5].to(F64) - x[:, 5].to(F64)).max()) < 0  # every particle loses energy
    excited = _kick(dtype, seed=1).track(beam).particles
    assert not torch.equal(excited[:, 5], a[:, 5])


@pytest.mark.parametrize("dtype", [F64, F32])
def test_zero_length_or_angle_returns_the_input_bits(dtype):
    x = _particles(257, dtype, seed=6)
    x[3, 5] = float("nan")
    x[4, 1] = -0.0
    beam = _beam(x)
    for L, th in ((0.0, ANGLE), (LENGTH, 0.0), (0.0, 0.0)):
        kick = _kick(dtype, length=L, angle=th)
        assert _bit_equal(kick.track(beam).particles, x), (L, th)
    # as one row of a batch
    for L, th in (([LENGTH, 0.0, LENGTH], ANGLE), (LENGTH, [ANGLE, ANGLE, 0.0])):
        out = _kick(dtype, length=L, angle=th).track(beam).particles
        assert out.shape == (3, 257, 7)
        quiet = 1 if isinstance(L, list) else 2
        assert _bit_equal(out[quiet], x)
        for b in set(range(3)) - {quiet}:
            assert not torch.equal(out[b, :3, 5], x[:3, 5])


@pytest.mark.parametrize("dtype", [F64, F32])
def test_nan_delta_stays_in_its_particle(dtype):
    x = _particles(257, dtype, seed=7)
    clean = _kick(dtype).track(_beam(x)).particles
    x2 = x.clone()
    x2[100, 5] = float("nan")
    x2[200, 5] = -2.0                                           # g' <= 1: no such particle
    out = _kick(dtype).track(_beam(x2)).particles
    for n in (100, 200):
        assert torch.isnan(out[n, [1, 3, 5]]).all()
        assert _bit_equal(out[n, list(PASS_THROUGH)], x2[n, list(PASS_THROUGH)])
    others = [n for n in range(257) if n not in (100, 200)]
    assert _bit_equal(out[others], clean[others])


# ---- 4. statistics ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _delta_gamma(seed, call):
    """Delta gamma (3, N) of N = 2^16 particles at delta = 0 in three equal batch rows."""
    N = 2**16
    x = torch.zeros(N, 7, dtype=F64, device="cuda")
    x[:, 6] = 1.0
    kick = _kick(F64, angle=[ANGLE] * 3, seed=seed)
    kick.reseed(call_index=call)
    out = kick.track(_beam(x)).particles
    gamma, P0, a, b = (float(v) for v in _factors(*(torch.tensor(v, dtype=F64) for v in (ENERGY, LENGTH, ANGLE)), _mass()))
    return out[..., 5] * P0, (gamma, P0, a, b)


@pytest.mark.parametrize("seed, call, row", [(0, 0, 0), (0, 1, 0), (0, 0, 1), (12345, 0, 0), (12345, 7, 2)])
def test_mean_and_variance_of_the_energy_change(seed, call, row):
    dg, (gamma, P0, a, b) = _delta_gamma(seed, call)
    dg = dg[row]
    N = dg.numel()
    pi = math.sqrt(gamma**2 - 1)
    loss, sigma = a * P0**2 * pi * gamma, math.sqrt(b * P0**3 * gamma**7 / pi**3)
    assert abs(loss * _mass() - 44e3) < 1e3 and abs(sigma * _mass() - 40e3) < 1e3      # eV: the physical case
    mean_err = abs(float(dg.mean()) + loss) / (sigma / math.sqrt(N))
    var_err = abs(float(dg.var(unbiased=False)) / sigma**2 - 1) / math.sqrt(2 / N)
    print(f"seed {seed} call {call} row {row}: mean {mean_err:.2f}, variance {var_err:.2f} standard errors")
    assert mean_err <= 4 and var_err <= 4


def test_calls_and_rows_are_uncorrelated():
    first, _ = _delta_gamma(0, 0)
    second, _ = _delta_gamma(0, 1)
    N = first.shape[1]

    def corr(u, v):
        u, v = u - u.mean(), v - v.mean()
        return float((u * v).mean() / (u.std(unbiased=False) * v.std(unbiased=False)))

    calls, rows = corr(first[0], second[0]), corr(first[0], first[1])
    print(f"correlation between calls {calls:.2e}, between rows {rows:.2e}, 1 / sqrt(N) = {1 / math.sqrt(N):.2e}")
    assert abs(calls) <= 4 / math.sqrt(N) and abs(rows) <= 4 / math.sqrt(N)


# ---- 5. sequence -----------------------------------------------------------------------------------------------------------------
def test_sequence_of_calls_reseed_and_clone():
    x = _particles(1025, F64, seed=8)
    beam = _beam(x)
    kick = _kick(F64, seed=21)
    kick.reseed()
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


def test_two_kicks_of_a_lattice_draw_different_deviates():
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    seg = ca.Segment([ca.Dipole(t(0.5), angle=t(0.05), name="b1", **kw), ca.Dipole(t(0.5), angle=t(0.05), name="b2", **kw)])
    k1, k2 = [e for e in seg.with_radiation_kicks(seed=4).elements if isinstance(e, ca.SynchrotronRadiationKick)]
    assert (k1.stream, k2.stream) == (0, 1)
    beam = _beam(_particles(1025, F64, seed=9))
    d1, d2 = k1.track(beam).particles[:, 5], k2.track(beam).particles[:, 5]
    assert float((d1 - d2).abs().min()) > 0
    k2.stream = 0                                               # the same key and call index: the same deviates
    k2.reseed()
    assert _bit_equal(k2.track(beam).particles[:, 5], d1)


# ---- 6. gradients ----------------------------------------------------------------------------------------------------------------
# measured on an MI355X against the restatement, largest over N = 1025 and N = 70 001: float64 particles 3.572e-16, energy 9.626e-13
# (the energy's gradient is what is left of terms that cancel to 1e-3 of their size), effect_length 8.476e-16, angle 4.078e-16;
# float32 particles 8.344e-08 (the sum over the three rows is formed in float32) and 0 for the three settings: their float64
# gradients agree as in the float64 case and both sides round them once to float32, to the same bits
GRAD_BOUND = {F64: {"particles": 4 * 3.572e-16, "energy": 4 * 9.626e-13, "effect_length": 4 * 8.476e-16, "angle": 4 * 4.078e-16},
              F32: {"particles": 4 * 8.344e-08, "energy": 0.0, "effect_length": 0.0, "angle": 0.0}}


def _gradients(N, dtype, through_kernel):
    """d(sum(out * W)) / d(particles (1, N, 7), energy (), effect_length (), angle (3,)), float64 weights W (3, N, 7)."""
    import cheetah_amd as ca

    g = torch.Generator().manual_seed(N)
    W = torch.randn(3, N, 7, generator=g, dtype=F32).to(F64).cuda()     # float32 values: the same cotangent for either beam dtype
    leaf = lambda v: v.clone().requires_grad_(True)  # noqa: E731
    x = leaf(_particles(N, dtype, seed=N + 1, batch=(1,)))
    e = leaf(torch.tensor(ENERGY, dtype=dtype, device="cuda"))
    L = leaf(torch.tensor(LENGTH, dtype=dtype, device="cuda"))
    th = leaf(torch.tensor([0.05, -0.03, 0.08], dtype=dtype, device="cuda"))
    if through_kernel:
        kick = ca.SynchrotronRadiationKick(torch.nn.Parameter(L.detach().clone()), torch.nn.Parameter(th.detach().clone()), seed=5,
                                           stream=1, dtype=dtype, device="cuda")
        kick.reseed(call_index=2)
        out = kick.track(_beam(x, e)).particles
        assert out.shape == (3, N, 7) and out.dtype == dtype
        (out.to(F64) * W).sum().backward()
        return {"particles": x.grad, "energy": e.grad, "effect_length": kick.effect_length.grad, "angle": kick.angle.grad}
    _, xi = ca._ops.sr_normals(5, 1, 2, 3, N, "cuda")
    (_restate(x, e, L, th, xi, _mass(dtype)) * W).sum().backward()
    return {"particles": x.grad, "energy": e.grad, "effect_length": L.grad, "angle": th.grad}


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("N", [1025, 70_001])
def test_gradients_against_autograd_of_the_restatement(N, dtype):
    got, ref = _gradients(N, dtype, True), _gradients(N, dtype, False)
    again = _gradients(N, dtype, True)
    assert got["particles"].shape == (1, N, 7) and got["angle"].shape == (3,) and got["energy"].shape == ()
    for name in got:
        assert got[name].dtype == dtype, name                  # a float32 beam's settings gradients come back in float32
        assert _bit_equal(got[name], again[name]), name         # two backward runs
    # the pass-through columns hand their cotangent on, summed over the three rows in the beam's dtype
    devs = {"particles": max(_rel(got["particles"][..., c], ref["particles"][..., c]) for c in (0, 1, 3, 5))}
    for name in ("energy", "effect_length", "angle"):
        devs[name] = _rel(got[name], ref[name])
    print(f"gradients N={N} {dtype}: " + ", ".join(f"{k} {v:.3e}" for k, v in devs.items()))
    for name, dev in devs.items():
        assert dev <= GRAD_BOUND[dtype][name], name


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------
def test_graph_capture_follows_the_call_index_and_the_angle():
    import cheetah_amd as ca

    beam = _beam(_particles(1025, F32, seed=10))
    kick = _kick(F32, seed=31, stream=2)
    with torch.no_grad():
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
        # an in-place edit of a setting between replays is followed
        unedited = twin.clone()
        kick.angle.mul_(2.0)
        twin.angle.mul_(2.0)
        third = step().clone()
        assert _bit_equal(third, twin.track(beam).particles)
        assert not torch.equal(third[:, 5], unedited.track(beam).particles[:, 5])


# ---- 8. in a lattice -------------------------------------------------------------------------------------------------------------
def _walk(elements, beam):
    for e in elements:
        beam = e.track(beam)
    return beam


def test_in_a_lattice_with_csr_kicks():
    """`Segment([Drift, Dipole, Drift]).with_csr_kicks(2).with_radiation_kicks(1)` against the element-by-element walk at equal
    call indices. The segment composes its leading run [Drift, first Dipole piece] into one map before it applies it, which rounds
    differently from two separate passes (`tests/test_gpu_csr_transient.py::test_segment_track_equals_the_element_walk`), so the
    walk tracks that run as the segment forms it; every other run is one element and the walk is plain. Bit for bit."""
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(3)
    beam = ca.ParticleBeam.from_parameters(num_particles=10_000, sigma_x=t(3e-4), sigma_y=t(2e-4), sigma_tau=t(3e-5), sigma_p=t(1e-3),
                                           energy=t(ENERGY), total_charge=t(1e-9), **kw)
    seg = ca.Segment([ca.Drift(t(0.4), name="d1", **kw), ca.Dipole(t(0.5), angle=t(0.05), dipole_e1=t(0.01), name="b", **kw),
                      ca.Drift(t(0.3), name="d2", **kw)]).with_csr_kicks(2).with_radiation_kicks(1, seed=6)
    els = list(seg.elements)
    assert [type(e).__name__ for e in els] == ["Drift", "Dipole", "SynchrotronRadiationKick", "CSRKick", "Dipole",
                                               "SynchrotronRadiationKick", "CSRKick", "Drift"]
    kicks = [e for e in els if isinstance(e, ca.SynchrotronRadiationKick)]
    with torch.no_grad():
        got = seg.track(beam)
        assert [k.call_index for k in kicks] == [1, 1]
        for k in kicks:
            k.reseed()
        ref = _walk([ca.Segment(els[:2])] + els[2:], beam)
        quiet = _walk([e for e in els if not isinstance(e, ca.SynchrotronRadiationKick)], beam)
    assert torch.isfinite(got.particles).all()
    assert _bit_equal(got.particles, ref.particles) and torch.equal(got.s, ref.s)
    # the radiation is there: two kicks of half the arc, theta^2 / L and so half of the 44 keV each, on 5 GeV
    loss = float((quiet.particles[:, 5] - got.particles[:, 5]).mean())
    assert 0.8 * 44e3 / ENERGY < loss < 1.2 * 44e3 / ENERGY
