"""The Wakefield element on the GPU against a float64 restatement in torch on the CPU (`_reference`: steps 1-6 of the element's
discrete algorithm written out directly), the beam-loading identity, degenerate inputs, gradients (autograd through the
restatement, gradcheck), determinism, no host synchronisation, graph capture and Segment tracking. One process, no workers."""
import math
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

MASS = 510998.95          # electron, eV
ENERGY = 1e8


def _sample(table, n, D, h):
    """Step 4: the table interpolated linearly at s = n D (0 beyond its last entry), the n = 0 sample halved."""
    M = n.shape[0]
    L = table.shape[0]
    p = (n * D) / h
    if L == 1:
        val = table[0].expand(M)
    else:
        j = torch.floor(p).clamp(0, L - 2).long()
        t = p - j
        val = (1 - t) * table[j] + t * table[j + 1]
    W = torch.where(p <= L - 1, val, torch.zeros_like(val))
    return W * torch.where(n == 0, 0.5, 1.0).to(W.dtype)


def _reference_row(x, q, w, scale, wl, wt, h, M):
    """One batch row, float64 on the CPU: x (N, 7), q, w (N), scale 0-d (= factor |Z| / p0c), wl / wt 1-D or None."""
    tau = x[:, 4]
    td = tau.detach()
    alive = (w.detach() > 0) & torch.isfinite(td)
    if not bool(alive.any()):
        return x
    lo, hi = td[alive].min(), td[alive].max()
    D = (hi - lo) / (M - 1)
    if D > 0:
        u = ((tau - lo) / D).clamp(0, M - 1)
    else:
        u = torch.zeros_like(tau)
    nan = torch.isnan(td)
    u = torch.where(nan, torch.full_like(u, float("nan")), u)
    k = torch.where(nan, torch.zeros_like(td), torch.floor(u.detach()).clamp(max=M - 2)).long()
    f = u - k
    c = torch.where(alive, q.abs() * w, torch.zeros_like(w))
    fd = torch.where(alive, f, torch.zeros_like(f))

    def deposit(v):
        G = torch.zeros(M, dtype=torch.float64)
        return G.index_add(0, k, (1 - fd) * v).index_add(0, k + 1, fd * v)

    n = torch.arange(M, dtype=torch.float64)
    lag = n[:, None] - n[None, :]
    idx = lag.clamp(min=0).long()

    def conv(table, Dep):
        Wn = _sample(table, n, D, h)
        T = torch.where(lag >= 0, Wn[idx], torch.zeros((), dtype=torch.float64))
        return T @ Dep

    zeros = torch.zeros(M, dtype=torch.float64)
    V = -conv(wl, deposit(c)) if wl is not None else zeros
    if wt is not None:
        Ux, Uy = conv(wt, deposit(c * x[:, 0])), conv(wt, deposit(c * x[:, 2]))
    else:
        Ux = Uy = zeros

    def gather(A):
        return (1 - f) * A[k] + f * A[k + 1]

    cols = list(x.unbind(-1))
    cols[5] = cols[5] + scale * gather(V)
    cols[1] = cols[1] + scale * gather(Ux)
    cols[3] = cols[3] + scale * gather(Uy)
    return torch.stack(cols, dim=-1)


def _scale(energy, factor, Z=1.0):
    e = energy.to(torch.float64)
    gamma = e / MASS
    beta = torch.where(gamma.abs() > 0, (1 - gamma.square().reciprocal()).clamp_min(0).sqrt(), torch.ones_like(gamma))
    return factor.to(torch.float64) * abs(Z) / (beta * gamma * MASS)


def _reference(particles, charges, survival, energy, factor, wl, wt, h, M):
    """Broadcast batch rows of the restatement -> (*batch, N, 7) float64 on the CPU (differentiable in every float input)."""
    cpu = lambda t: None if t is None else t.cpu().to(torch.float64)  # noqa: E731
    particles, charges, survival, energy, factor = map(cpu, (particles, charges, survival, energy, factor))
    wl, wt = cpu(wl), cpu(wt)
    batch = torch.broadcast_shapes(particles.shape[:-2], charges.shape[:-1], survival.shape[:-1], energy.shape, factor.shape)
    N = particles.shape[-2]
    B = math.prod(batch)
    x = particles.expand(*batch, N, 7).reshape(B, N, 7)
    q = charges.expand(*batch, N).reshape(B, N)
    w = survival.expand(*batch, N).reshape(B, N)
    s = _scale(energy, factor).expand(batch).reshape(B)
    hh = float(h)
    rows = [_reference_row(x[b], q[b], w[b], s[b], wl, wt, hh, M) for b in range(B)]
    return torch.stack(rows).reshape(*batch, N, 7)


def _tables(kind, L=300, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = torch.linspace(0, 1, L, dtype=torch.float64)
    wl = 3e13 * torch.exp(-3 * s) * (1 + 0.1 * torch.rand(L, generator=g, dtype=torch.float64)) if "l" in kind else None
    wt = 5e15 * (s + 0.05) * torch.exp(-2 * s) if "t" in kind else None
    return wl, wt


def _beam_tensors(N, dtype, batch=(), seed=0, dead=0.1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*batch, N, 7, generator=g, dtype=torch.float64)
    x[..., 0] = x[..., 0] * 2e-4 + 5e-5
    x[..., 1] *= 1e-4
    x[..., 2] = x[..., 2] * 1e-4 - 3e-5
    x[..., 3] *= 1e-4
    x[..., 4] *= 2e-5
    x[..., 5] *= 1e-3
    x[..., 6] = 1.0
    q = (1e-9 / N) * (0.5 + torch.rand(N, generator=g, dtype=torch.float64))
    w = torch.rand(N, generator=g, dtype=torch.float64).clamp_min(0.05)
    w[torch.rand(N, generator=g) < dead] = 0.0
    kw = {"dtype": dtype, "device": "cuda"}
    return x.to(**kw), q.to(**kw), w.to(**kw)


def _element(wl, wt, M, factor=None, dtype=torch.float64, h=2e-7):
    import cheetah_amd as ca

    kw = {"dtype": dtype, "device": "cuda"}
    return ca.Wakefield(torch.tensor(h, **kw), longitudinal_wake=None if wl is None else wl.to(**kw),
                        transverse_wake=None if wt is None else wt.to(**kw),
                        factor=None if factor is None else factor.to(**kw), num_bins=M, **kw)


def _track(elem, x, q, w, energy=None):
    import cheetah_amd as ca

    energy = torch.tensor(ENERGY, dtype=x.dtype, device="cuda") if energy is None else energy
    beam = ca.ParticleBeam(x, energy, particle_charges=q, survival_probabilities=w)
    return elem.track(beam)


def _tabs(elem):
    t = lambda v: v if v.numel() > 0 else None  # noqa: E731
    return t(elem.longitudinal_wake), t(elem.transverse_wake)


def _check_against_reference(got, ref, x_in, dtype):
    got, ref, x_in = got.cpu().double(), ref.detach(), x_in.cpu().double()
    kick = (ref - x_in)[..., [1, 3, 5]].abs().max()
    assert kick > 0
    err = (got - ref).abs()
    # both sides round coordinate + kick once: a float64 result may differ by that one rounding (1 ulp of the coordinate, which
    # exceeds 1e-12 of the kick where the kick is below ~1e-4 of the coordinate); a float32 one by 2 ulp
    r = ref.to(dtype).abs()
    ulp = (torch.nextafter(r, torch.full_like(r, float("inf"))) - r).double()
    tol = (1 if dtype == torch.float64 else 2) * ulp + 1e-12 * kick
    assert torch.all(err <= tol), float((err - tol).max())
    # no other coordinate moves
    assert torch.equal(got[..., [0, 2, 4, 6]], x_in[..., [0, 2, 4, 6]])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["l", "t", "lt"])
@pytest.mark.parametrize("M", [2, 37, 1000, 4096])
@pytest.mark.parametrize("N", [1000, 100_000])
def test_matches_the_float64_reference(N, M, kind, dtype):
    wl, wt = _tables(kind, seed=M)
    x, q, w = _beam_tensors(N, dtype, seed=N + M)
    elem = _element(wl, wt, M, factor=torch.tensor(1.7), dtype=dtype)
    out = _track(elem, x, q, w)
    assert out.particles.dtype == dtype and out.particles.shape == (N, 7)
    energy = torch.tensor(ENERGY, dtype=dtype)
    ref = _reference(x, q, w, energy, elem.factor, *_tabs(elem), elem.wake_spacing, M)
    _check_against_reference(out.particles, ref, x, dtype)
    assert out.particle_charges is q and out.survival_probabilities is w


@pytest.mark.parametrize("factor_shape", [(3,), (2, 1)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_vectorised_beam_and_factor(factor_shape, dtype):
    wl, wt = _tables("lt", seed=3)
    x, q, w = _beam_tensors(5000, dtype, batch=(3,), seed=7)
    factor = torch.linspace(0.5, 2.0, math.prod(factor_shape), dtype=torch.float64).reshape(factor_shape)
    elem = _element(wl, wt, 200, factor=factor, dtype=dtype)
    out = _track(elem, x, q, w)
    batch = torch.broadcast_shapes((3,), factor_shape)
    assert out.particles.shape == (*batch, 5000, 7)
    ref = _reference(x, q, w, torch.tensor(ENERGY, dtype=dtype), elem.factor, *_tabs(elem), elem.wake_spacing, 200)
    _check_against_reference(out.particles, ref, x.expand(*batch, 5000, 7), dtype)


@pytest.mark.parametrize("M", [2, 5, 64, 1000, 4096])
def test_beam_loading_identity(M):
    """Constant wake W0 and factor F: sum_i c_i dE_i = -F |Z| W0 Q^2 / 2 (the gather is the adjoint of the deposit)."""
    x, q, w = _beam_tensors(20_000, torch.float64, seed=M)
    W0, F = 2.5e13, 1.3
    elem = _element(torch.full((4,), W0, dtype=torch.float64), None, M, factor=torch.tensor(F), h=1.0)
    out = _track(elem, x, q, w)
    p0c = 1.0 / float(_scale(torch.tensor(ENERGY, dtype=torch.float64), torch.tensor(1.0)))
    c = (q.abs() * w).double()
    dE = (out.particles[:, 5] - x[:, 5]) * p0c
    lhs = float((c * dE).sum())
    Q = float(c.sum())
    rhs = -float(elem.factor) * W0 * Q * Q / 2
    assert abs(lhs - rhs) <= 1e-12 * abs(rhs), (lhs, rhs)


def test_no_surviving_particle_leaves_the_beam_bit_for_bit():
    wl, wt = _tables("lt")
    for dtype in (torch.float32, torch.float64):
        x, q, w = _beam_tensors(3000, dtype, seed=1)
        x[5, 4] = float("nan")
        out = _track(_element(wl, wt, 50, dtype=dtype), x, q, torch.zeros_like(w))
        bits = torch.int32 if dtype == torch.float32 else torch.int64
        assert torch.equal(out.particles.view(bits), x.view(bits))


def test_one_surviving_particle_gets_the_self_kick():
    W0, F = 4e13, 2.0
    x, q, w = _beam_tensors(1000, torch.float64, seed=2, dead=0.0)
    w = torch.zeros_like(w)
    w[17] = 0.75
    elem = _element(torch.tensor([W0, 1e13, 0.0], dtype=torch.float64), None, 37, factor=torch.tensor(F))
    out = _track(elem, x, q, w)
    scale = float(_scale(torch.tensor(ENERGY, dtype=torch.float64), torch.tensor(1.0)))
    c = float(q[17].abs() * w[17])
    expect = -0.5 * F * W0 * c * scale
    got = float(out.particles[17, 5] - x[17, 5])
    assert abs(got - expect) <= 1e-12 * abs(expect) + 1e-15 * abs(float(x[17, 5]))


def test_all_equal_tau_gives_a_zero_node_spacing():
    wl, wt = _tables("lt")
    x, q, w = _beam_tensors(2000, torch.float64, seed=4)
    x[:, 4] = 3e-6
    elem = _element(wl, wt, 100, factor=torch.tensor(0.9))
    out = _track(elem, x, q, w)
    ref = _reference(x, q, w, torch.tensor(ENERGY, dtype=torch.float64), elem.factor, *_tabs(elem), elem.wake_spacing, 100)
    _check_against_reference(out.particles, ref, x, torch.float64)
    # every particle sits on node 0 and sees the self term only
    assert torch.allclose(out.particles[:, 5] - x[:, 5], (out.particles[0, 5] - x[0, 5]).expand(2000), rtol=1e-12, atol=0)


def test_nan_tau_poisons_that_particle_only():
    wl, wt = _tables("l")
    for dtype in (torch.float32, torch.float64):
        x, q, w = _beam_tensors(4000, dtype, seed=5)
        x[10, 4] = float("nan")
        w[10] = 1.0
        out = _track(_element(wl, wt, 64, dtype=dtype), x, q, w).particles

        assert torch.isnan(out[10, [1, 3, 5]]).all()
        assert torch.equal(out[10, [0, 2, 4, 6]].nan_to_num(), x[10, [0, 2, 4, 6]].nan_to_num())
        others = torch.ones(4000, dtype=torch.bool, device="cuda")
        others[10] = False
        assert torch.isfinite(out[others]).all()
        elem = _element(wl, wt, 64, dtype=dtype)
        ref = _reference(x, q, w, torch.tensor(ENERGY, dtype=dtype), elem.factor, *_tabs(elem), elem.wake_spacing, 64)
        _check_against_reference(out[others], ref[others.cpu()], x[others], dtype)


def test_dead_particles_beyond_the_grid_take_the_end_nodes():
    wl, wt = _tables("lt")
    x, q, w = _beam_tensors(3000, torch.float64, seed=6, dead=0.0)
    tau = x[:, 4]
    head, tail = int(tau.argmin()), int(tau.argmax())
    x[0, 4], w[0] = tau[tail] + 1e-4, 0.0     # dead, far behind the tail
    x[1, 4], w[1] = tau[head] - 1e-4, 0.0     # dead, far ahead of the head
    elem = _element(wl, wt, 80)
    out = _track(elem, x, q, w).particles
    ref = _reference(x, q, w, torch.tensor(ENERGY, dtype=torch.float64), elem.factor, *_tabs(elem), elem.wake_spacing, 80)
    _check_against_reference(out, ref, x, torch.float64)
    d = out - x
    # the same node kick (u = M - 1 / u = 0) up to the rounding of the coordinates it was added to
    assert torch.allclose(d[0, [1, 3, 5]], d[tail, [1, 3, 5]], rtol=1e-9, atol=0)
    assert torch.allclose(d[1, [1, 3, 5]], d[head, [1, 3, 5]], rtol=1e-9, atol=0)


def _grad_inputs(N=1500, M=37, seed=8, batch=()):
    wl, wt = _tables("lt", L=60, seed=seed)
    x, q, w = _beam_tensors(N, torch.float64, batch=batch, seed=seed)
    energy = torch.tensor(ENERGY, dtype=torch.float64, device="cuda")
    factor = torch.tensor([0.8, 1.4] if batch else 1.2, dtype=torch.float64, device="cuda")
    return x, q, w, energy, factor, wl.cuda(), wt.cuda(), M


@pytest.mark.parametrize("batch", [(), (2,)])
def test_gradients_match_autograd_through_the_reference(batch):
    import cheetah_amd as ca

    x, q, w, energy, factor, wl, wt, M = _grad_inputs(batch=batch)
    leaves = [t.clone().requires_grad_() for t in (x, q, w, energy, factor, wl, wt)]
    X, Q, W, E, F, WL, WT = leaves
    elem = _element(wl, wt, M)
    elem.factor, elem.longitudinal_wake, elem.transverse_wake = F, WL, WT
    beam = ca.ParticleBeam(X, E, particle_charges=Q, survival_probabilities=W)
    out = elem.track(beam).particles
    g = torch.Generator().manual_seed(3)
    cot = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * cot.cuda()).sum().backward()
    got = [t.grad.cpu() for t in leaves]

    rl = [t.detach().cpu().clone().requires_grad_() for t in (x, q, w, energy, factor, wl, wt)]
    ref = _reference(rl[0], rl[1], rl[2], rl[3], rl[4], rl[5], rl[6], elem.wake_spacing, M)
    (ref * cot).sum().backward()
    names = ["particles", "charges", "survival", "energy", "factor", "longitudinal_wake", "transverse_wake"]
    for name, a, r in zip(names, got, rl):
        b = r.grad
        scale = b.abs().max()
        assert scale > 0, name
        assert torch.allclose(a, b, rtol=0, atol=1e-9 * scale), (name, float((a - b).abs().max() / scale))


def test_gradcheck_small_case():
    import cheetah_amd as ca

    kw = {"dtype": torch.float64, "device": "cuda"}
    g = torch.Generator().manual_seed(11)
    N, M = 24, 9
    base = torch.randn(N, 7, generator=g, dtype=torch.float64)
    base[:, 4] *= 1e-3
    base[:, 6] = 1.0
    base = base.to(**kw)
    xc, yc, dc = (base[:, i].clone().requires_grad_() for i in (0, 2, 5))
    q = (0.5 + torch.rand(N, generator=g, dtype=torch.float64)).to(**kw).requires_grad_()
    w = (0.2 + 0.8 * torch.rand(N, generator=g, dtype=torch.float64)).to(**kw).requires_grad_()
    energy = torch.tensor(2e6, **kw).requires_grad_()
    factor = torch.tensor(1.5, **kw).requires_grad_()
    wl = (1e5 * torch.rand(12, generator=g, dtype=torch.float64)).to(**kw).requires_grad_()
    wt = (1e6 * torch.rand(10, generator=g, dtype=torch.float64)).to(**kw).requires_grad_()

    def fn(xc, yc, dc, q, w, energy, factor, wl, wt):
        cols = list(base.unbind(-1))
        cols[0], cols[2], cols[5] = xc, yc, dc
        elem = ca.Wakefield(torch.tensor(1.5e-4, **kw), longitudinal_wake=wl, transverse_wake=wt, factor=factor, num_bins=M, **kw)
        beam = ca.ParticleBeam(torch.stack(cols, dim=-1), energy, particle_charges=q, survival_probabilities=w)
        return elem.track(beam).particles

    assert torch.autograd.gradcheck(fn, (xc, yc, dc, q, w, energy, factor, wl, wt), eps=1e-6, atol=1e-8, rtol=1e-6)


def test_two_identical_calls_are_bit_equal():
    import cheetah_amd as ca

    wl, wt = _tables("lt")
    x, q, w = _beam_tensors(1_000_000, torch.float32, seed=12)
    elem = _element(wl, wt, 1000, dtype=torch.float32)
    a = _track(elem, x, q, w).particles
    b = _track(elem, x, q, w).particles
    assert torch.equal(a, b)
    grads = []
    for _ in range(2):
        xx = x.clone().requires_grad_()
        out = elem.track(ca.ParticleBeam(xx, torch.tensor(ENERGY, device="cuda"), particle_charges=q, survival_probabilities=w))
        (out.particles[:, 5].square().sum() + out.particles[:, 1].sum()).backward()
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
    wl, wt = _tables("lt")
    elem = _element(wl, wt, 500, dtype=torch.float32)
    x = beam.particles.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(x, beam.energy)

    def fwd_bwd():
        x.grad = None
        elem.track(gb).particles[:, 5].sum().backward()

    assert _sync_warnings(lambda: elem.track(beam).particles) == []
    assert _sync_warnings(fwd_bwd) == []


def test_captured_step_replays_like_eager_after_an_in_place_factor_change():
    import cheetah_amd as ca

    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, sigma_x=t(2e-4), sigma_tau=t(2e-5), total_charge=t(1e-9), **kw)
    wl, wt = _tables("lt")
    wake = _element(wl, wt, 300, factor=torch.tensor(1.0), dtype=torch.float32)
    seg = ca.Segment([ca.Drift(t(0.5), **kw), wake, ca.Quadrupole(t(0.2), k1=t(3.0), **kw)])

    def step():
        return (seg.track(beam).particles,)

    with torch.no_grad():
        for _ in range(3):
            step()
        captured = ca.graph.capture(step)
        first = captured()[0].clone()
        wake.factor.copy_(t(25.0))
        replayed = captured()[0].clone()
        eager = step()[0]
    assert torch.equal(replayed, eager)
    assert not torch.equal(replayed, first)


def _walk(elements, beam):
    for e in elements:
        beam = e.track(beam)
    return beam


@pytest.mark.parametrize("lattice", ["linear", "space_charge"])
def test_segment_track_equals_the_element_walk(lattice):
    import cheetah_amd as ca

    kw = {"dtype": torch.float64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(1)
    beam = ca.ParticleBeam.from_parameters(num_particles=100_000, sigma_x=t(3e-4), sigma_y=t(2e-4), sigma_tau=t(3e-5),
                                           total_charge=t(1e-9), **kw)
    wl, wt = _tables("lt")
    wake = _element(wl, wt, 400, factor=torch.tensor(30.0))
    if lattice == "linear":
        els = [ca.Drift(t(0.4), **kw), ca.Quadrupole(t(0.2), k1=t(4.0), **kw), wake, ca.Drift(t(0.3), **kw),
               ca.Quadrupole(t(0.2), k1=t(-3.0), **kw)]
    else:
        els = [ca.SpaceChargeKick(t(0.3), grid_shape=(32, 32, 32), **kw), ca.Drift(t(0.4), **kw), wake, ca.Drift(t(0.3), **kw),
               ca.SpaceChargeKick(t(0.3), grid_shape=(32, 32, 32), **kw)]
    seg = ca.Segment(els)
    with torch.no_grad():
        got = seg.track(beam)
        ref = _walk(els, beam)
        no_wake = _walk([e for e in els if e is not wake], beam)
    effect = (ref.particles - no_wake.particles).abs().max(dim=0).values
    assert float(effect[5]) > 0
    err = (got.particles - ref.particles).abs().max(dim=0).values
    ulp = 16 * torch.finfo(torch.float64).eps * ref.particles.abs().max(dim=0).values
    assert torch.all(err <= 1e-9 * effect + ulp), err
    assert torch.equal(got.s, ref.s)
