"""The CSRKick element on the GPU against a float64 restatement in torch on the CPU (`_reference_row`: the element's discrete
algorithm written out directly), the Gaussian-bunch steady-state CSR energy change against its quadrature, scaling laws, degenerate
inputs, vectorised beams and settings, gradients (autograd through the restatement, gradcheck), determinism, no host
synchronisation, graph capture and lattices (Segment tracking, split bends, a compressing chicane). One process, no workers."""
import math
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

MASS = 510998.95          # electron, eV
ENERGY = 1e8
K_E = 8.9875517923e9      # 1 / (4 pi eps0), V m / C


def _b_table(M):
    """b_0 = -1, b_j = a_(j-1) - a_j with a_j = (j+1)^(2/3) - j^(2/3) in its cancellation-free form."""
    j = torch.arange(M, dtype=torch.float64)
    a = (2 * j + 1) / ((j + 1).pow(4 / 3) + (j * (j + 1)).pow(2 / 3) + j.pow(4 / 3))
    return torch.cat([torch.tensor([-1.0], dtype=torch.float64), a[:-1] - a[1:]])


def _p0c(energy):
    e = energy.to(torch.float64)
    gamma = e / MASS
    beta = torch.where(gamma.abs() > 0, (1 - gamma.square().reciprocal()).clamp_min(0).sqrt(), torch.ones_like(gamma))
    return beta * gamma * MASS


def _reference_row(x, q, w, energy, L, theta, M, Z=1.0):
    """One batch row, float64 on the CPU: x (N, 7), q, w (N), energy / L / theta 0-d. The grid is detached."""
    tau = x[:, 4]
    td = tau.detach()
    alive = (w.detach() > 0) & torch.isfinite(td)
    if not bool(alive.any()):
        return x
    lo, hi = td[alive].min(), td[alive].max()
    h = (hi - lo) / (M - 1)
    if not h > 0:
        return x
    u = ((tau - lo) / h).clamp(0, M - 1)
    nan = torch.isnan(td)
    u = torch.where(nan, torch.full_like(u, float("nan")), u)
    k = torch.where(nan, torch.zeros_like(td), torch.floor(u.detach()).clamp(max=M - 2)).long()
    f = u - k
    c = torch.where(alive, q.abs() * w, torch.zeros_like(w))
    fd = torch.where(alive, f, torch.zeros_like(f))
    D = torch.zeros(M, dtype=torch.float64).index_add(0, k, (1 - fd) * c).index_add(0, k + 1, fd * c)
    n = torch.arange(M)
    lag = n[None, :] - n[:, None]                               # T[k, m] = b_(m - k) for m >= k
    T = torch.where(lag >= 0, _b_table(M)[lag.clamp(min=0)], torch.zeros((), dtype=torch.float64))
    S = T @ D
    dE = abs(Z) * 9 ** (1 / 3) * K_E * L.pow(1 / 3) * theta.abs().pow(2 / 3) * h.pow(-4 / 3) * S
    kick = ((1 - f) * dE[k] + f * dE[k + 1]) / _p0c(energy)
    cols = list(x.unbind(-1))
    cols[5] = cols[5] + kick
    return torch.stack(cols, dim=-1)


def _reference(particles, charges, survival, energy, L, theta, M):
    """Broadcast batch rows of the restatement -> (*batch, N, 7) float64 on the CPU (differentiable in every float input)."""
    cpu = lambda t: t.cpu().to(torch.float64)  # noqa: E731
    particles, charges, survival, energy, L, theta = map(cpu, (particles, charges, survival, energy, L, theta))
    batch = torch.broadcast_shapes(particles.shape[:-2], charges.shape[:-1], survival.shape[:-1], energy.shape, L.shape, theta.shape)
    N = particles.shape[-2]
    B = math.prod(batch)
    x = particles.expand(*batch, N, 7).reshape(B, N, 7)
    q = charges.expand(*batch, N).reshape(B, N)
    w = survival.expand(*batch, N).reshape(B, N)
    e, ll, th = (t.expand(batch).reshape(B) for t in (energy, L, theta))
    rows = [_reference_row(x[b], q[b], w[b], e[b], ll[b], th[b], M) for b in range(B)]
    return torch.stack(rows).reshape(*batch, N, 7)


def _beam_tensors(N, dtype, batch=(), seed=0, dead=0.1, sigma_tau=1e-4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*batch, N, 7, generator=g, dtype=torch.float64)
    x[..., 0] *= 2e-4
    x[..., 1] *= 1e-4
    x[..., 2] *= 1e-4
    x[..., 3] *= 1e-4
    x[..., 4] *= sigma_tau
    x[..., 5] *= 1e-3
    x[..., 6] = 1.0
    q = (1e-9 / N) * (0.5 + torch.rand(N, generator=g, dtype=torch.float64))
    w = torch.rand(N, generator=g, dtype=torch.float64).clamp_min(0.05)
    w[torch.rand(N, generator=g) < dead] = 0.0
    kw = {"dtype": dtype, "device": "cuda"}
    return x.to(**kw), q.to(**kw), w.to(**kw)


def _element(L=0.3, theta=0.03, M=200, dtype=torch.float64):
    import cheetah_amd as ca

    kw = {"dtype": dtype, "device": "cuda"}
    L = L if isinstance(L, torch.Tensor) else torch.tensor(L)
    theta = theta if isinstance(theta, torch.Tensor) else torch.tensor(theta)
    return ca.CSRKick(L.to(**kw), theta.to(**kw), num_bins=M, **kw)


def _track(elem, x, q, w, energy=None):
    import cheetah_amd as ca

    energy = torch.tensor(ENERGY, dtype=x.dtype, device="cuda") if energy is None else energy
    return elem.track(ca.ParticleBeam(x, energy, particle_charges=q, survival_probabilities=w))


def _ref_of(elem, x, q, w, energy=None):
    energy = torch.tensor(ENERGY, dtype=x.dtype) if energy is None else energy
    return _reference(x, q, w, energy, elem.effect_length, elem.angle, elem.num_bins)


def _check_against_reference(got, ref, x_in, dtype):
    got, ref, x_in = got.cpu().double(), ref.detach(), x_in.cpu().double()
    kick = (ref - x_in)[..., 5].abs().max()
    assert kick > 0
    err = (got - ref).abs()
    # both sides round delta + kick once: a float64 result may differ by that one rounding (1 ulp of delta); a float32 one by 2 ulp
    r = ref.to(dtype).abs()
    ulp = (torch.nextafter(r, torch.full_like(r, float("inf"))) - r).double()
    tol = (1 if dtype == torch.float64 else 2) * ulp + 1e-12 * kick
    assert torch.all(err <= tol), float((err - tol).max())
    # no other coordinate moves
    assert torch.equal(got[..., [0, 1, 2, 3, 4, 6]], x_in[..., [0, 1, 2, 3, 4, 6]])


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M", [2, 3, 64, 500, 4096])
@pytest.mark.parametrize("N", [1000, 100_000])
def test_matches_the_float64_reference(N, M, dtype):
    x, q, w = _beam_tensors(N, dtype, seed=N + M)
    elem = _element(0.4, -0.05, M, dtype=dtype)
    out = _track(elem, x, q, w)
    assert out.particles.dtype == dtype and out.particles.shape == (N, 7)
    _check_against_reference(out.particles, _ref_of(elem, x, q, w), x, dtype)
    assert out.particle_charges is q and out.survival_probabilities is w


def _gaussian_energy_change(sigma_tau, Q, R, L, M, N=1_000_000, seed=0):
    """(tau, Delta E in eV) of a Gaussian bunch of N float64 particles after one kick of an arc L of radius R."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(N, 7, dtype=torch.float64)
    x[:, 4] = sigma_tau * torch.randn(N, generator=g, dtype=torch.float64)
    x[:, 6] = 1.0
    kw = {"dtype": torch.float64, "device": "cuda"}
    x = x.to(**kw)
    q = torch.full((N,), Q / N, **kw)
    w = torch.ones(N, **kw)
    out = _track(_element(L, L / R, M), x, q, w)
    p0c = float(_p0c(torch.tensor(ENERGY, dtype=torch.float64)))
    return x[:, 4].cpu(), (out.particles[:, 5] - x[:, 5]).cpu() * p0c


def _analytic_gaussian_moments():
    """Mean and rms of the steady-state CSR energy change of a Gaussian bunch, in units of Q k_e L / (R^(2/3) sigma^(4/3)), by
    quadrature: Delta E(z) = -(2 / 3^(1/3)) G(z), G(z) = int_0^inf t^(-1/3) lambda'(z - t) dt (t = v^(3/2): no singularity),
    weighted with lambda(z)."""
    z = torch.linspace(-8, 8, 1601, dtype=torch.float64)
    v = torch.linspace(0, 40, 40001, dtype=torch.float64)
    dv = float(v[1] - v[0])
    phi = lambda s: torch.exp(-0.5 * s * s) / math.sqrt(2 * math.pi)  # noqa: E731
    G = torch.empty_like(z)
    for i in range(0, z.numel(), 200):
        s = z[i:i + 200, None] - v[None, :].pow(1.5)
        f = 1.5 * (-s * phi(s))
        G[i:i + 200] = (f.sum(dim=1) - 0.5 * (f[:, 0] + f[:, -1])) * dv
    dE = -(2 / 3 ** (1 / 3)) * G
    wz = phi(z) / phi(z).sum()
    mean = float((wz * dE).sum())
    rms = math.sqrt(float((wz * (dE - mean) ** 2).sum()))
    return mean, rms


def test_gaussian_bunch_matches_the_steady_state_theory():
    sigma, Q, R, L = 1e-4, 1e-9, 10.0, 1.0
    tau, dE = _gaussian_energy_change(sigma, Q, R, L, 300)
    unit = Q * K_E * L / (R ** (2 / 3) * sigma ** (4 / 3))
    mean, rms = _analytic_gaussian_moments()
    assert abs(mean + 0.3505) < 1e-3 and abs(rms - 0.2460) < 1e-3, (mean, rms)
    got_mean, got_rms = float(dE.mean()) / unit, float(dE.std()) / unit
    assert abs(got_mean - mean) <= 0.01 * abs(mean), (got_mean, mean)
    assert abs(got_rms - rms) <= 0.01 * rms, (got_rms, rms)
    head = tau <= torch.quantile(tau[:100_000], 0.1)
    assert float(dE[head].mean()) > 0          # the head (smallest tau) gains energy
    assert float(dE[tau >= torch.quantile(tau[:100_000], 0.9)].mean()) < 0


def _kick_of(elem, x, q, w):
    return (_track(elem, x, q, w).particles[:, 5] - x[:, 5]).cpu()


def _assert_scaled(a, b, factor):
    assert float((b - factor * a).abs().max()) <= 1e-12 * float(b.abs().max()), float((b - factor * a).abs().max() / b.abs().max())


def test_scaling_laws():
    x, q, w = _beam_tensors(50_000, torch.float64, seed=21)
    x[:, 5] = 0.0                                      # delta_out is the kick itself, rounded once
    base = _kick_of(_element(0.2, 0.01, 250), x, q, w)
    assert float(base.abs().max()) > 0
    _assert_scaled(base, _kick_of(_element(0.2, 0.01, 250), x, 3 * q, w), 3.0)
    _assert_scaled(base, _kick_of(_element(1.6, 0.01, 250), x, q, w), 2.0)
    _assert_scaled(base, _kick_of(_element(0.2, -0.08, 250), x, q, w), 4.0)
    x2 = x.clone()
    x2[:, 4] *= 2
    _assert_scaled(base, _kick_of(_element(0.2, 0.01, 250), x2, q, w), 2 ** (-4 / 3))


def test_zero_angle_length_or_charge_and_no_survivor_leave_the_beam_bit_for_bit():
    for dtype in (torch.float32, torch.float64):
        x, q, w = _beam_tensors(3000, dtype, seed=1)
        x[5, 4] = float("nan")
        for elem, qq, ww in ((_element(0.3, 0.0, 50, dtype), q, w), (_element(0.0, 0.02, 50, dtype), q, w),
                             (_element(0.3, 0.02, 50, dtype), torch.zeros_like(q), w),
                             (_element(0.3, 0.02, 50, dtype), q, torch.zeros_like(w))):
            out = _track(elem, x, qq, ww)
            assert torch.equal(_bits(out.particles), _bits(x))


def test_one_survivor_or_equal_tau_gives_no_kick():
    x, q, w = _beam_tensors(1000, torch.float64, seed=2, dead=0.0)
    one = torch.zeros_like(w)
    one[17] = 0.75
    assert torch.equal(_bits(_track(_element(), x, q, one).particles), _bits(x))
    x2 = x.clone()
    x2[:, 4] = 3e-6
    assert torch.equal(_bits(_track(_element(), x2, q, w).particles), _bits(x2))


def test_nan_tau_poisons_that_particle_only():
    for dtype in (torch.float32, torch.float64):
        x, q, w = _beam_tensors(4000, dtype, seed=5)
        x[10, 4] = float("nan")
        w[10] = 1.0
        elem = _element(0.3, 0.02, 64, dtype)
        out = _track(elem, x, q, w).particles
        assert torch.isnan(out[10, 5])
        others = torch.ones(4000, dtype=torch.bool, device="cuda")
        others[10] = False
        assert torch.isfinite(out[others]).all()
        ref = _ref_of(elem, x, q, w)
        _check_against_reference(out[others], ref[others.cpu()], x[others], dtype)


def test_dead_particles_beyond_the_grid_take_the_end_nodes():
    x, q, w = _beam_tensors(3000, torch.float64, seed=6, dead=0.0)
    x[:, 5] = 0.0
    tau = x[:, 4]
    head, tail = int(tau.argmin()), int(tau.argmax())
    x[0, 4], w[0] = tau[tail] + 1e-3, 0.0     # dead, far behind the tail
    x[1, 4], w[1] = tau[head] - 1e-3, 0.0     # dead, far ahead of the head
    elem = _element(0.3, 0.02, 80)
    out = _track(elem, x, q, w).particles
    _check_against_reference(out, _ref_of(elem, x, q, w), x, torch.float64)
    d = (out - x)[:, 5]
    # node M - 1 (u clamped) for the one behind, node 0 for the one ahead: the kicks of the extreme survivors
    assert torch.allclose(d[0], d[tail], rtol=1e-9, atol=0) and torch.allclose(d[1], d[head], rtol=1e-9, atol=0)
    assert float(d[1]) == float(d[head])


@pytest.mark.parametrize("setting,shape", [("length", (3,)), ("angle", (2, 1)), ("angle", (3,))])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_vectorised_beam_and_settings_equal_single_rows(setting, shape, dtype):
    x, q, w = _beam_tensors(5000, dtype, batch=(3,), seed=7)
    vals = torch.linspace(0.1, 0.5, math.prod(shape), dtype=torch.float64).reshape(shape)
    L, th = (vals, torch.tensor(0.02)) if setting == "length" else (torch.tensor(0.3), -0.1 * vals)
    elem = _element(L, th, 200, dtype)
    out = _track(elem, x, q, w).particles
    batch = torch.broadcast_shapes((3,), shape)
    assert out.shape == (*batch, 5000, 7)
    Lb, tb = elem.effect_length.expand(batch), elem.angle.expand(batch)
    for idx in torch.cartesian_prod(*[torch.arange(s) for s in batch]).reshape(-1, len(batch)).tolist():
        idx = tuple(idx)
        row = _track(_element(Lb[idx].clone(), tb[idx].clone(), 200, dtype), x[idx[-1]], q, w).particles
        assert torch.equal(out[idx], row), idx
    ref = _reference(x, q, w, torch.tensor(ENERGY, dtype=dtype), elem.effect_length, elem.angle, 200)
    _check_against_reference(out, ref, x.expand(*batch, 5000, 7), dtype)


def _grad_inputs(N=1500, M=37, seed=8, batch=()):
    x, q, w = _beam_tensors(N, torch.float64, batch=batch, seed=seed)
    kw = {"dtype": torch.float64, "device": "cuda"}
    energy = torch.tensor(ENERGY, **kw)
    L = torch.tensor([0.3, 0.7] if batch else 0.4, **kw)
    theta = torch.tensor(-0.03, **kw)
    return x, q, w, energy, L, theta, M


@pytest.mark.parametrize("batch", [(), (2,)])
def test_gradients_match_autograd_through_the_reference(batch):
    import cheetah_amd as ca

    x, q, w, energy, L, theta, M = _grad_inputs(batch=batch)
    leaves = [t.clone().requires_grad_() for t in (x, q, w, energy, L, theta)]
    X, Q, W, E, LL, TH = leaves
    elem = _element(0.4, -0.03, M)
    elem.effect_length, elem.angle = LL, TH
    out = elem.track(ca.ParticleBeam(X, E, particle_charges=Q, survival_probabilities=W)).particles
    g = torch.Generator().manual_seed(3)
    cot = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * cot.cuda()).sum().backward()
    got = [t.grad.cpu() for t in leaves]

    rl = [t.detach().cpu().clone().requires_grad_() for t in (x, q, w, energy, L, theta)]
    ref = _reference(*rl, M)
    (ref * cot).sum().backward()
    names = ["particles", "charges", "survival", "energy", "effect_length", "angle"]
    for name, a, r in zip(names, got, rl):
        b = r.grad
        scale = b.abs().max()
        assert scale > 0, name
        assert torch.allclose(a, b, rtol=0, atol=1e-9 * scale), (name, float((a - b).abs().max() / scale))
    # the tau column gets the node coordinate's term
    assert float(got[0][..., 4].abs().max()) > 0


def test_gradcheck_small_case():
    import cheetah_amd as ca

    kw = {"dtype": torch.float64, "device": "cuda"}
    g = torch.Generator().manual_seed(11)
    N, M = 24, 9
    base = torch.randn(N, 7, generator=g, dtype=torch.float64)
    base[:, 4] *= 1e-3
    base[:, 6] = 1.0
    base = base.to(**kw)
    xc, dc = (base[:, i].clone().requires_grad_() for i in (0, 5))
    # charges of order one (finite differences of step 1e-6 stay linear) and an energy that makes the kick of order 0.1
    q = (0.5 + torch.rand(N, generator=g, dtype=torch.float64)).to(**kw).requires_grad_()
    w = (0.2 + 0.8 * torch.rand(N, generator=g, dtype=torch.float64)).to(**kw).requires_grad_()
    energy = torch.tensor(1e15, **kw).requires_grad_()
    L = torch.tensor(0.5, **kw).requires_grad_()
    theta = torch.tensor(-0.2, **kw).requires_grad_()

    def fn(xc, dc, q, w, energy, L, theta):
        cols = list(base.unbind(-1))
        cols[0], cols[5] = xc, dc
        beam = ca.ParticleBeam(torch.stack(cols, dim=-1), energy, particle_charges=q, survival_probabilities=w)
        return ca.CSRKick(L, theta, num_bins=M, **kw).track(beam).particles

    assert torch.autograd.gradcheck(fn, (xc, dc, q, w, energy, L, theta), eps=1e-6, atol=1e-8, rtol=1e-6)


def test_gradient_at_zero_angle_and_length_is_zero():
    import cheetah_amd as ca

    x, q, w = _beam_tensors(2000, torch.float64, seed=13)
    kw = {"dtype": torch.float64, "device": "cuda"}
    for L0, t0 in ((0.3, 0.0), (0.0, 0.02)):
        L = torch.tensor(L0, **kw).requires_grad_()
        theta = torch.tensor(t0, **kw).requires_grad_()
        beam = ca.ParticleBeam(x, torch.tensor(ENERGY, **kw), particle_charges=q, survival_probabilities=w)
        ca.CSRKick(L, theta, num_bins=50, **kw).track(beam).particles[:, 5].sum().backward()
        assert float(L.grad) == 0.0 and float(theta.grad) == 0.0


def test_two_identical_calls_are_bit_equal():
    import cheetah_amd as ca

    x, q, w = _beam_tensors(1_000_000, torch.float32, seed=12)
    elem = _element(0.3, 0.02, 500, torch.float32)
    a = _track(elem, x, q, w).particles
    b = _track(elem, x, q, w).particles
    assert torch.equal(a, b)
    grads = []
    for _ in range(2):
        xx = x.clone().requires_grad_()
        out = elem.track(ca.ParticleBeam(xx, torch.tensor(ENERGY, device="cuda"), particle_charges=q, survival_probabilities=w))
        out.particles[:, 5].square().sum().backward()
        grads.append(xx.grad)
    assert torch.equal(grads[0], grads[1])


def _sync_warnings(fn, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return [w for w in rec if "synchronizing" in str(w.message).lower() and "prototype" not in str(w.message).lower()]


def test_no_host_synchronisation():
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, device="cuda", dtype=torch.float32)
    assert len(_sync_warnings(lambda: float(beam.sigma_x), warm=0)) == 1          # the switch sees what it should see
    kw = {"dtype": torch.float32, "device": "cuda"}
    elem = ca.CSRKick(torch.tensor(0.3, **kw).requires_grad_(), torch.tensor(0.02, **kw).requires_grad_(), num_bins=500, **kw)
    x = beam.particles.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(x, beam.energy)

    def fwd_bwd():
        x.grad = None
        elem.track(gb).particles[:, 5].sum().backward()

    with torch.no_grad():
        assert _sync_warnings(lambda: elem.track(beam).particles) == []
    assert _sync_warnings(fwd_bwd) == []


def test_captured_step_replays_like_eager_after_an_in_place_angle_change():
    import cheetah_amd as ca

    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, sigma_x=t(2e-4), sigma_tau=t(5e-5), total_charge=t(1e-9), **kw)
    csr = ca.CSRKick(t(0.5), t(0.01), num_bins=300, **kw)
    seg = ca.Segment([ca.Drift(t(0.5), **kw), csr, ca.Quadrupole(t(0.2), k1=t(3.0), **kw)])

    def step():
        return (seg.track(beam).particles,)

    with torch.no_grad():
        for _ in range(3):
            step()
        captured = ca.graph.capture(step)
        first = captured()[0].clone()
        csr.angle.copy_(t(0.2))
        replayed = captured()[0].clone()
        eager = step()[0]
    assert torch.equal(replayed, eager)
    assert not torch.equal(replayed, first)


def _walk(elements, beam):
    for e in elements:
        beam = e.track(beam)
    return beam


def test_segment_track_equals_the_element_walk():
    import cheetah_amd as ca

    kw = {"dtype": torch.float64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(1)
    beam = ca.ParticleBeam.from_parameters(num_particles=100_000, sigma_x=t(3e-4), sigma_y=t(2e-4), sigma_tau=t(3e-5),
                                           total_charge=t(1e-9), **kw)
    bend = ca.Dipole(t(0.4), angle=t(0.08), dipole_e1=t(0.02), dipole_e2=t(0.03), name="b", **kw)
    # one linear element between two kicks: the segment's runs are the elements themselves
    els = [ca.Drift(t(0.4), **kw), ca.CSRKick(t(0.2), t(0.05), num_bins=300, **kw), ca.Quadrupole(t(0.2), k1=t(4.0), **kw),
           ca.CSRKick(t(0.1), t(-0.02), num_bins=100, **kw)]
    els += bend.split_for_csr(2, num_bins=300) + [ca.Drift(t(0.3), **kw)]
    seg = ca.Segment(els)
    with torch.no_grad():
        got = seg.track(beam)
        ref = _walk(els, beam)
        no_csr = _walk([e for e in els if not isinstance(e, ca.CSRKick)], beam)
    assert float((ref.particles - no_csr.particles)[:, 5].abs().max()) > 0
    assert torch.equal(got.particles, ref.particles)
    assert torch.equal(got.s, ref.s)


def _chicane(kw, theta=0.05, Lb=0.5, Ld=1.0):
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    common = {"gap": t(0.02), "fringe_integral": t(0.5), **kw}
    return ca.Segment([
        ca.Dipole(t(Lb), angle=t(theta), dipole_e2=t(theta), k1=t(0.1), tilt=t(1e-3), name="b1", **common),
        ca.Drift(t(Ld), **kw),
        ca.RBend(t(Lb), angle=t(-theta), rbend_e1=t(0.01), rbend_e2=t(-0.01), fringe_at="entrance", name="b2", **common),
        ca.Drift(t(0.3), **kw),
        ca.RBend(t(Lb), angle=t(-theta), fringe_at="exit", name="b3", **common),
        ca.Drift(t(Ld), **kw),
        ca.Dipole(t(Lb), angle=t(theta), dipole_e1=t(theta), gap_exit=t(0.03), fringe_integral_exit=t(0.3), name="b4", **common),
        ca.Drift(t(0.2), **kw),
    ])


def test_with_csr_kicks_at_zero_charge_matches_the_unsplit_chicane():
    import cheetah_amd as ca

    kw = {"dtype": torch.float64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(2)
    beam = ca.ParticleBeam.from_parameters(num_particles=100_000, sigma_x=t(2e-4), sigma_px=t(2e-5), sigma_y=t(1e-4),
                                           sigma_py=t(1e-5), sigma_tau=t(1e-4), sigma_p=t(1e-3), total_charge=t(0.0), **kw)
    chicane = _chicane(kw)
    split = chicane.with_csr_kicks(10, num_bins=200)
    assert sum(isinstance(e, ca.CSRKick) for e in split.elements) == 40
    with torch.no_grad():
        ref = chicane.track(beam).particles
        got = split.track(beam).particles
    scale = ref.abs().max(dim=0).values
    assert torch.all((got - ref).abs().max(dim=0).values <= 1e-12 * scale), ((got - ref).abs().max(dim=0).values / scale)


def test_projected_emittance_grows_with_charge_in_a_compressing_chicane():
    import cheetah_amd as ca

    kw = {"dtype": torch.float64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    chicane = _chicane(kw)
    R56 = float(chicane.first_order_transfer_map(t(ENERGY), ca.Species("electron"))[4, 5])
    split = chicane.with_csr_kicks(10, num_bins=200)
    torch.manual_seed(3)
    base = ca.ParticleBeam.from_parameters(num_particles=200_000, sigma_x=t(1e-4), sigma_px=t(1e-5), sigma_y=t(1e-4),
                                           sigma_py=t(1e-5), sigma_tau=t(1e-4), sigma_p=t(1e-5), energy=t(ENERGY), **kw)
    x = base.particles.clone()
    x[:, 5] += -0.6 / R56 * x[:, 4]                  # chirp: tau_out = tau + R56 delta = 0.4 tau
    emit, sigma_tau = [], []
    with torch.no_grad():
        for Q in (0.0, 0.25e-9, 1e-9):
            q = torch.full((x.shape[0],), Q / x.shape[0], **kw)
            out = split.track(ca.ParticleBeam(x, t(ENERGY), particle_charges=q))
            emit.append(float(out.emittance_x))
            sigma_tau.append(float(out.sigma_tau))
    assert sigma_tau[0] < 0.5 * float(base.sigma_tau)      # the chicane compresses
    assert emit[0] < emit[1] < emit[2], emit
    assert emit[2] > 1.05 * emit[0], emit
