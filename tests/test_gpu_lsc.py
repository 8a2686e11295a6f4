"""The LSCKick element on the GPU against a float64 restatement in torch on the CPU (`_reference_row`: the element's discrete
algorithm written out directly, the full M x M matrix sign(lag) c^_|lag|), Newton's third law, the on-axis LSC impedance of a
modulated flat-top bunch, symmetry and scaling, degenerate inputs, vectorised beams and settings, the radius taken from the beam,
gradients (autograd through the restatement, gradcheck), determinism, no host synchronisation, graph capture and lattices.
One process, no workers.

Tolerance of a kick against the restatement (`_tolerance`): both sides round delta + kick once, so 1 ulp of delta for float64 and
2 ulp for float32, plus 1e-12 max|kick| for the order of the sums, plus the coefficient table's term: device and host asinh / sqrt
may differ by a few ulp of P, |P| <= 1 + asinh(M / rho), so with eps_c = 64 * 2^-53 * (1 + asinh(M / rho)) no node differs by
more than eps_c * S * sum_k D_k."""
import functools
import math
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

ENERGY = 1e8
K_E = 8.9875517923e9      # 1 / (4 pi eps0), V m / C


@functools.lru_cache(maxsize=None)
def _mass(dtype=torch.float64):
    """The electron mass in eV as a beam of this dtype hands it to the kernels (the species' mass rounded to the beam's dtype): S
    goes with 1 / gamma^3 and rho with 1 / gamma, so the restatement must take the same number (the CSR kick's scale, 1 / p0c, does
    not see the mass' last digits at this energy)."""
    import cheetah_amd as ca

    return ca.Species("electron", dtype=dtype).mass_eV_float


def _gamma(dtype=torch.float64):
    return ENERGY / _mass(dtype)


def _p0c(energy, mass=None):
    mass = _mass() if mass is None else mass
    e = energy.to(torch.float64)
    gamma = e / mass
    beta = torch.where(gamma.abs() > 0, (1 - gamma.square().reciprocal()).clamp_min(0).sqrt(), torch.ones_like(gamma))
    return beta * gamma * mass


def _chat(M, rho):
    """c^_j for j = 0 ... M - 1: -1/2 of the second difference of P(v) = v / (|v| + sqrt(v^2 + rho^2)) + asinh(v / rho)."""
    j = torch.arange(-1, M + 1, dtype=torch.float64)
    p = j / (j.abs() + torch.sqrt(j * j + rho * rho)) + torch.asinh(j / rho)
    return -0.5 * (p[2:] - 2 * p[1:-1] + p[:-2])


def _reference_row(x, q, w, energy, L, radius, M, Z=1.0, info=None, mass=None):
    """One batch row, float64 on the CPU: x (N, 7), q, w (N), energy / L / radius 0-d. The grid is detached."""
    mass = _mass() if mass is None else mass
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
    gamma = energy / mass
    rho = radius / (gamma * h)
    ch = _chat(M, rho)
    full = torch.cat([-ch[1:].flip(0), ch])                      # lags -(M - 1) ... M - 1: sign(lag) c^_|lag|
    V = (full.unfold(0, M, 1) @ D).flip(0)                       # V_k = sum_m full[(m - k) + M - 1] D_m
    S = abs(Z) * 2 * K_E * L / (gamma.square() * h.square() * _p0c(energy, mass))
    node = S * V
    kick = (1 - f) * node[k] + f * node[k + 1]
    if info is not None:
        info.append({"S": float(S), "sumD": float(D.sum()), "rho": float(rho), "h": float(h), "M": M})
    cols = list(x.unbind(-1))
    cols[5] = cols[5] + kick
    return torch.stack(cols, dim=-1)


def _reference(particles, charges, survival, energy, L, radius, M, info=None):
    """Broadcast batch rows of the restatement -> (*batch, N, 7) float64 on the CPU (differentiable in every float input); the
    mass is that of a beam of the particles' dtype."""
    mass = _mass(particles.dtype)
    cpu = lambda t: t.cpu().to(torch.float64)  # noqa: E731
    particles, charges, survival, energy, L, radius = map(cpu, (particles, charges, survival, energy, L, radius))
    batch = torch.broadcast_shapes(particles.shape[:-2], charges.shape[:-1], survival.shape[:-1], energy.shape, L.shape,
                                   radius.shape)
    N = particles.shape[-2]
    B = math.prod(batch)
    x = particles.expand(*batch, N, 7).reshape(B, N, 7)
    q = charges.expand(*batch, N).reshape(B, N)
    w = survival.expand(*batch, N).reshape(B, N)
    e, ll, a = (t.expand(batch).reshape(B) for t in (energy, L, radius))
    rows = [_reference_row(x[b], q[b], w[b], e[b], ll[b], a[b], M, info=info, mass=mass) for b in range(B)]
    return torch.stack(rows).reshape(*batch, N, 7)


def _eps_term(info):
    """The coefficient table's term of the tolerance, from the restatement's own S and D (the largest over the rows)."""
    return max(64 * 2.0 ** -53 * (1 + math.asinh(i["M"] / i["rho"])) * abs(i["S"]) * i["sumD"] for i in info)


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


def _spacing(x, w, M):
    """The node spacing h the kick will find for one row (float64, from the values the device holds)."""
    tau = x[..., 4].double()[w.double() > 0]
    return float(tau.max() - tau.min()) / (M - 1)


def _element(L=2.0, radius=2e-4, M=200, dtype=torch.float64):
    import cheetah_amd as ca

    kw = {"dtype": dtype, "device": "cuda"}
    L = L if isinstance(L, torch.Tensor) else torch.tensor(L)
    if radius is not None:
        radius = (radius if isinstance(radius, torch.Tensor) else torch.tensor(radius)).to(**kw)
    return ca.LSCKick(L.to(**kw), radius, num_bins=M, **kw)


def _track(elem, x, q, w, energy=None):
    import cheetah_amd as ca

    energy = torch.tensor(ENERGY, dtype=x.dtype, device="cuda") if energy is None else energy
    return elem.track(ca.ParticleBeam(x, energy, particle_charges=q, survival_probabilities=w))


def _ref_of(elem, x, q, w, energy=None, info=None):
    energy = torch.tensor(ENERGY, dtype=x.dtype) if energy is None else energy
    return _reference(x, q, w, energy, elem.effect_length, elem.beam_radius, elem.num_bins, info=info)


def _tolerance(ref, kick_max, eps_term, dtype):
    r = ref.to(dtype).abs()
    ulp = (torch.nextafter(r, torch.full_like(r, float("inf"))) - r).double()
    return (1 if dtype == torch.float64 else 2) * ulp + 1e-12 * kick_max + eps_term


def _check_against_reference(got, ref, x_in, dtype, info):
    got, ref, x_in = got.cpu().double(), ref.detach(), x_in.cpu().double()
    kick = (ref - x_in)[..., 5].abs().max()
    assert kick > 0
    err = (got - ref).abs()
    tol = _tolerance(ref, kick, _eps_term(info), dtype)
    print(f"max err {float(err[..., 5].max()):.3e} max |kick| {float(kick):.3e} eps term {_eps_term(info):.3e}")
    assert torch.all(err <= tol), float((err - tol).max())
    # no other coordinate moves
    assert torch.equal(got[..., [0, 1, 2, 3, 4, 6]], x_in[..., [0, 1, 2, 3, 4, 6]])


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---- 1. parity with the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("rho", [1e-2, 1.0, 50.0])
@pytest.mark.parametrize("M", [2, 3, 64, 65, 500, 4096])
@pytest.mark.parametrize("N", [1000, 5000])
def test_matches_the_float64_reference(N, M, rho, dtype):
    x, q, w = _beam_tensors(N, dtype, seed=N + M)
    elem = _element(2.0, rho * _gamma(dtype) * _spacing(x, w, M), M, dtype=dtype)
    out = _track(elem, x, q, w)
    assert out.particles.dtype == dtype and out.particles.shape == (N, 7)
    info = []
    ref = _ref_of(elem, x, q, w, info=info)
    assert abs(info[0]["rho"] / rho - 1) < 1e-5
    _check_against_reference(out.particles, ref, x, dtype, info)
    assert out.particle_charges is q and out.survival_probabilities is w


# ---- 2. Newton's third law -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,rho", [(200, 1.0), (65, 1e-2), (1000, 50.0)])
def test_kicks_weighted_with_the_charges_sum_to_zero(M, rho):
    x, q, w = _beam_tensors(5000, torch.float64, seed=31 + M)
    x[:, 5] = 0.0
    out = _track(_element(2.0, rho * _gamma() * _spacing(x, w, M), M), x, q, w).particles
    c, d = (q * w).cpu(), out[:, 5].cpu()
    assert float(d.abs().max()) > 0
    net, gross = float((c * d).sum().abs()), float((c * d.abs()).sum())
    print(f"net / gross {net / gross:.3e}")
    assert net <= 1e-12 * gross


# ---- 3. the on-axis LSC impedance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xi", [0.3, 1.5])
@pytest.mark.parametrize("N,M,per", [(6000, 301, 20), (50_000, 1001, 25)])
def test_modulated_flat_top_matches_the_on_axis_impedance(N, M, per, xi):
    """A flat-top bunch with a 5 % density modulation of wave number k: the modulated part of the energy change is
    -A sinc^6(k h / 2) sin(k tau) with A = 4 k_e lambda_1 L (1 - xi K_1(xi)) / (k a^2), xi = k a / gamma (the on-axis LSC impedance of
    a uniform disc); one sinc^2 each for the linear deposit, the hat basis and the linear gather."""
    kw = {"dtype": torch.float64, "device": "cuda"}
    length, Q, L, mod = 1e-3, 1e-9, 2.0, 0.05
    tau = torch.linspace(-length / 2, length / 2, N, dtype=torch.float64)
    h = length / (M - 1)
    k = 2 * math.pi / (per * h)
    a = xi * _gamma() / k
    x = torch.zeros(N, 7, dtype=torch.float64)
    x[:, 4] = tau
    x[:, 6] = 1.0
    x = x.to(**kw)
    w = torch.ones(N, **kw)
    elem = _element(L, a, M)
    flat = torch.full((N,), Q / N, dtype=torch.float64)
    kicks = [_track(elem, x, c.to(**kw), w).particles[:, 5].cpu() for c in (flat * (1 + mod * torch.cos(k * tau)), flat)]
    dk = (kicks[0] - kicks[1]) * float(_p0c(torch.tensor(ENERGY)))                       # eV
    win = tau.abs() < 2 * per * h
    A = torch.stack([torch.sin(k * tau[win]), torch.cos(k * tau[win])], dim=1)
    fit = torch.linalg.lstsq(A, dk[win, None]).solution[:, 0]
    K1 = float(torch.special.modified_bessel_k1(torch.tensor(xi, dtype=torch.float64)))
    amp = 4 * K_E * (mod * Q / length) * L * (1 - xi * K1) / (k * a * a)
    sinc = math.sin(k * h / 2) / (k * h / 2)
    expect = -amp * sinc ** 6
    dev = abs(float(fit[0]) / expect - 1)
    print(f"sin amplitude {float(fit[0]):.6e} eV, expected {expect:.6e} eV, relative deviation {dev:.2e}, cos / sin "
          f"{abs(float(fit[1]) / float(fit[0])):.2e}")
    assert dev <= 5e-3
    assert abs(float(fit[1])) <= 1e-2 * abs(float(fit[0]))


# ---- 4. symmetry and scaling -----------------------------------------------------------------------------------------------------------
def test_mirror_symmetry_and_linearity_in_length_and_charge():
    M = 250
    x, q, w = _beam_tensors(5000, torch.float64, seed=21)
    x[:, 5] = 0.0                                      # delta_out is the kick itself, rounded once
    a = 0.7 * _gamma() * _spacing(x, w, M)
    elem = _element(2.0, a, M)
    base = _track(elem, x, q, w).particles[:, 5].cpu()
    info = []
    ref = _ref_of(elem, x, q, w, info=info)[:, 5]
    kick_max, eps = ref.abs().max(), _eps_term(info)
    assert float(base.abs().max()) > 0

    def close(got, want, factor):
        tol = _tolerance(want, abs(factor) * kick_max, abs(factor) * eps, torch.float64)
        print(f"factor {factor}: max difference {float((got - want).abs().max()):.3e}")
        assert torch.all((got - want).abs() <= tol)

    xm = x.clone()
    xm[:, 4] = -xm[:, 4]
    close(_track(elem, xm, q, w).particles[:, 5].cpu(), -base, 1.0)
    close(_track(_element(6.0, a, M), x, q, w).particles[:, 5].cpu(), 3.0 * base, 3.0)
    close(_track(elem, x, 3 * q, w).particles[:, 5].cpu(), 3.0 * base, 3.0)


# ---- 5. degenerate inputs --------------------------------------------------------------------------------------------------------------
def test_zero_length_or_charge_and_no_survivor_leave_the_beam_bit_for_bit():
    for dtype in (torch.float32, torch.float64):
        x, q, w = _beam_tensors(3000, dtype, seed=1)
        x[5, 4] = float("nan")
        for elem, qq, ww in ((_element(0.0, 2e-4, 50, dtype), q, w), (_element(2.0, 2e-4, 50, dtype), torch.zeros_like(q), w),
                             (_element(2.0, 2e-4, 50, dtype), q, torch.zeros_like(w)), (_element(0.0, None, 50, dtype), q, w)):
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
        elem = _element(2.0, 2e-4, 64, dtype)
        out = _track(elem, x, q, w).particles
        assert torch.isnan(out[10, 5])
        others = torch.ones(4000, dtype=torch.bool, device="cuda")
        others[10] = False
        assert torch.isfinite(out[others]).all()
        info = []
        ref = _ref_of(elem, x, q, w, info=info)
        _check_against_reference(out[others], ref[others.cpu()], x[others], dtype, info)


def test_dead_particles_beyond_the_grid_take_the_end_nodes():
    x, q, w = _beam_tensors(3000, torch.float64, seed=6, dead=0.0)
    x[:, 5] = 0.0
    tau = x[:, 4]
    head, tail = int(tau.argmin()), int(tau.argmax())
    x[0, 4], w[0] = tau[tail] + 1e-3, 0.0     # dead, far behind the tail
    x[1, 4], w[1] = tau[head] - 1e-3, 0.0     # dead, far ahead of the head
    elem = _element(2.0, 2e-4, 80)
    out = _track(elem, x, q, w).particles
    info = []
    _check_against_reference(out, _ref_of(elem, x, q, w, info=info), x, torch.float64, info)
    d = (out - x)[:, 5]
    # node M - 1 (u clamped) for the one behind, node 0 for the one ahead: the kicks of the extreme survivors
    assert torch.allclose(d[0], d[tail], rtol=1e-9, atol=0) and torch.allclose(d[1], d[head], rtol=1e-9, atol=0)
    assert float(d[1]) == float(d[head])
    assert float(d[head]) > 0 > float(d[tail])            # the head is pushed forward, the tail held back


def test_a_row_without_a_radius_gets_nan_delta_and_leaves_the_other_rows():
    for dtype in (torch.float32, torch.float64):
        x, q, w = _beam_tensors(2000, dtype, batch=(2,), seed=9)
        x[1, :, 0] = 1e-4                                  # all x and y of row 1 equal: sigma_x = sigma_y = 0
        x[1, :, 2] = -2e-4
        elem = _element(2.0, None, 50, dtype)
        out = _track(elem, x, q, w).particles
        assert torch.isnan(out[1, :, 5]).all()
        assert torch.equal(out[1][:, [0, 1, 2, 3, 4, 6]], x[1][:, [0, 1, 2, 3, 4, 6]])
        row0 = _track(elem, x[0], q, w).particles
        assert torch.isfinite(row0).all() and not torch.equal(row0, x[0])
        assert torch.equal(out[0], row0)


# ---- 6. vectorised beams and settings ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["length", "radius"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_vectorised_beam_and_settings_equal_single_rows(setting, dtype):
    N, M, shape = 2049, 100, (2, 1)
    x, q, w = _beam_tensors(N, dtype, batch=(3,), seed=7)          # beam batch (3,), a shared (N,) charge vector
    vals = torch.tensor([[1.0], [2.5]], dtype=torch.float64)
    L, a = (vals, torch.tensor(2e-4)) if setting == "length" else (torch.tensor(2.0), 1.5e-4 * vals)
    elem = _element(L, a, M, dtype)
    out = _track(elem, x, q, w).particles
    batch = torch.broadcast_shapes((3,), shape)
    assert out.shape == (*batch, N, 7)
    Lb, ab = elem.effect_length.expand(batch), elem.beam_radius.expand(batch)
    for idx in torch.cartesian_prod(*[torch.arange(s) for s in batch]).reshape(-1, len(batch)).tolist():
        idx = tuple(idx)
        row = _track(_element(Lb[idx].clone(), ab[idx].clone(), M, dtype), x[idx[-1]], q, w).particles
        assert torch.equal(out[idx], row), idx
    info = []
    ref = _reference(x, q, w, torch.tensor(ENERGY, dtype=dtype), elem.effect_length, elem.beam_radius, M, info=info)
    _check_against_reference(out, ref, x.expand(*batch, N, 7), dtype, info)


# ---- 7. the radius from the beam -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("batch", [(), (3,)])
def test_radius_from_the_beam_equals_the_explicit_radius(batch, dtype):
    import cheetah_amd as ca

    x, q, w = _beam_tensors(3000, dtype, batch=batch, seed=14)
    beam = ca.ParticleBeam(x, torch.tensor(ENERGY, dtype=dtype, device="cuda"), particle_charges=q, survival_probabilities=w)
    radius = 0.85 * (beam.sigma_x + beam.sigma_y)
    assert radius.shape == batch and bool((radius > 0).all())
    a = _element(2.0, None, 120, dtype).track(beam).particles
    b = _element(2.0, radius, 120, dtype).track(beam).particles
    assert not torch.equal(a, x)
    assert torch.equal(_bits(a), _bits(b))


# ---- 8. gradients ----------------------------------------------------------------------------------------------------------------------------
def _grad_inputs(N=2000, M=40, seed=8, batch=()):
    x, q, w = _beam_tensors(N, torch.float64, batch=batch, seed=seed)
    kw = {"dtype": torch.float64, "device": "cuda"}
    energy = torch.tensor(ENERGY, **kw)
    L = torch.tensor([2.0, 0.7] if batch else 1.5, **kw)
    radius = torch.tensor(1.3 * _gamma() * _spacing(x[0] if batch else x, w, M), **kw)       # rho about 1.3
    return x, q, w, energy, L, radius, M


@pytest.mark.parametrize("batch", [(), (2,)])
def test_gradients_match_autograd_through_the_reference(batch):
    """Bound per input: 1e-9 max|reference gradient|. The radius and the energy reach the kick through rho as well, whose
    coefficients d c^ / d rho come from d P / d rho = -v rho / (s (|v| + s)^2) - v / (rho s), |d P / d rho| <= 1.25 / rho: a few ulp
    of it between device and host move d(rho) by at most eps_r = 64 * 2^-53 * (1.25 / rho) * S * sum_n |cotangent of delta_n| *
    sum_k D_k, which enters the radius' gradient times d rho / d a = rho / a and the energy's times |d rho / d E| = rho / E."""
    import cheetah_amd as ca

    x, q, w, energy, L, radius, M = _grad_inputs(batch=batch)
    leaves = [t.clone().requires_grad_() for t in (x, q, w, energy, L, radius)]
    X, Q, W, E, LL, A = leaves
    elem = _element(1.0, 1e-4, M)
    elem.effect_length, elem.beam_radius = LL, A
    out = elem.track(ca.ParticleBeam(X, E, particle_charges=Q, survival_probabilities=W)).particles
    g = torch.Generator().manual_seed(3)
    cot = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * cot.cuda()).sum().backward()
    got = [t.grad.cpu() for t in leaves]

    rl = [t.detach().cpu().clone().requires_grad_() for t in (x, q, w, energy, L, radius)]
    info = []
    ref = _reference(*rl, M, info=info)
    (ref * cot).sum().backward()
    cot5 = cot[..., 5].abs().reshape(len(info), -1).sum(dim=1)
    eps_r = max(64 * 2.0 ** -53 * (1.25 / i["rho"]) * abs(i["S"]) * float(c5) * i["sumD"] * i["rho"] for i, c5 in zip(info, cot5))
    extra = {"beam_radius": eps_r / float(radius) * len(info), "energy": eps_r / ENERGY * len(info)}
    names = ["particles", "charges", "survival", "energy", "effect_length", "beam_radius"]
    for name, a, r in zip(names, got, rl):
        b = r.grad
        scale = b.abs().max()
        assert scale > 0, name
        print(f"{name}: max difference / max |gradient| {float((a - b).abs().max() / scale):.3e}")
        assert torch.allclose(a, b, rtol=0, atol=1e-9 * float(scale) + extra.get(name, 0.0)), name
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
    # charges of order one (finite differences of step 1e-6 stay linear), an energy that makes the kick of order 0.1 (S is about
    # 0.2 at gamma = 1e4 and h = 5e-4) and a radius that makes rho of order one
    q = (0.5 + torch.rand(N, generator=g, dtype=torch.float64)).to(**kw).requires_grad_()
    w = (0.2 + 0.8 * torch.rand(N, generator=g, dtype=torch.float64)).to(**kw).requires_grad_()
    energy = torch.tensor(5e9, **kw).requires_grad_()
    L = torch.tensor(0.5, **kw).requires_grad_()
    radius = torch.tensor(4.0, **kw).requires_grad_()

    def fn(xc, dc, q, w, energy, L, radius):
        cols = list(base.unbind(-1))
        cols[0], cols[5] = xc, dc
        beam = ca.ParticleBeam(torch.stack(cols, dim=-1), energy, particle_charges=q, survival_probabilities=w)
        return ca.LSCKick(L, radius, num_bins=M, **kw).track(beam).particles

    with torch.no_grad():
        moved = fn(xc, dc, q, w, energy, L, radius)[:, 5] - dc
    assert 1e-3 < float(moved.abs().max()) < 10
    assert torch.autograd.gradcheck(fn, (xc, dc, q, w, energy, L, radius), eps=1e-6, atol=1e-8, rtol=1e-6)


def test_gradient_at_zero_length():
    """At L = 0 the kick is zero and linear in L: every gradient that carries the factor L (charges, survival, radius, energy, and
    the particles' beyond the cotangent passing through) is exactly zero, and all are finite. The gradient of L itself is the kick
    per metre, as autograd through the restatement gives it."""
    import cheetah_amd as ca

    x, q, w = _beam_tensors(2000, torch.float64, seed=13)
    kw = {"dtype": torch.float64, "device": "cuda"}
    M, a = 50, 2e-4
    leaves = [t.clone().requires_grad_() for t in (x, q, w, torch.tensor(ENERGY, **kw), torch.tensor(0.0, **kw),
                                                    torch.tensor(a, **kw))]
    X, Q, W, E, L, A = leaves
    out = ca.LSCKick(L, A, num_bins=M, **kw).track(ca.ParticleBeam(X, E, particle_charges=Q, survival_probabilities=W)).particles
    assert torch.equal(_bits(out.detach()), _bits(x))
    out[:, 5].sum().backward()
    assert all(bool(torch.isfinite(t.grad).all()) for t in leaves)
    expect = torch.zeros_like(x)
    expect[:, 5] = 1.0
    assert torch.equal(X.grad, expect)
    for t in (Q, W, E, A):
        assert float(t.grad.abs().max()) == 0.0
    rl = [t.detach().cpu().clone().requires_grad_() for t in leaves]
    _reference(*rl, M)[:, 5].sum().backward()
    assert abs(float(L.grad) - float(rl[4].grad)) <= 1e-9 * abs(float(rl[4].grad))


def test_radius_from_the_beam_sends_a_gradient_to_x_and_y():
    import cheetah_amd as ca

    x, q, w = _beam_tensors(2000, torch.float64, seed=15)
    kw = {"dtype": torch.float64, "device": "cuda"}
    grads = []
    for radius in (None, "explicit"):
        X = x.clone().requires_grad_()
        beam = ca.ParticleBeam(X, torch.tensor(ENERGY, **kw), particle_charges=q, survival_probabilities=w)
        a = None if radius is None else (0.85 * (beam.sigma_x + beam.sigma_y)).detach()
        out = _element(2.0, a, 60).track(beam).particles
        g = torch.Generator().manual_seed(4)
        (out[:, 5] * torch.randn(2000, generator=g, dtype=torch.float64).cuda()).sum().backward()
        grads.append(X.grad)
    assert bool(torch.isfinite(grads[0]).all())
    for col in (0, 2):
        assert float(grads[0][:, col].abs().max()) > 0 and float(grads[1][:, col].abs().max()) == 0.0
    assert torch.equal(grads[0][:, [1, 3, 5, 6]], grads[1][:, [1, 3, 5, 6]])


# ---- 9. run-time properties ----------------------------------------------------------------------------------------------------------------
def test_two_identical_calls_are_bit_equal():
    import cheetah_amd as ca

    x, q, w = _beam_tensors(200_000, torch.float32, seed=12)
    kw = {"dtype": torch.float32, "device": "cuda"}
    for radius in (2e-4, None):
        elem = _element(2.0, radius, 500, torch.float32)
        a = _track(elem, x, q, w).particles
        b = _track(elem, x, q, w).particles
        assert torch.equal(a, b) and not torch.equal(a, x)
        grads = []
        for _ in range(2):
            xx = x.clone().requires_grad_()
            L = torch.tensor(2.0, **kw).requires_grad_()
            e2 = ca.LSCKick(L, elem.beam_radius, num_bins=500, **kw)
            out = e2.track(ca.ParticleBeam(xx, torch.tensor(ENERGY, device="cuda"), particle_charges=q, survival_probabilities=w))
            out.particles[:, 5].square().sum().backward()
            grads.append((xx.grad, L.grad))
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


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


@pytest.mark.parametrize("from_beam", [False, True])
def test_no_host_synchronisation(from_beam):
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, device="cuda", dtype=torch.float32)
    assert len(_sync_warnings(lambda: float(beam.sigma_x), warm=0)) == 1          # the switch sees what it should see
    kw = {"dtype": torch.float32, "device": "cuda"}
    radius = None if from_beam else torch.tensor(3e-4, **kw).requires_grad_()
    elem = ca.LSCKick(torch.tensor(2.0, **kw).requires_grad_(), radius, num_bins=500, **kw)
    x = beam.particles.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(x, beam.energy)

    def fwd_bwd():
        x.grad = None
        elem.track(gb).particles[:, 5].sum().backward()

    with torch.no_grad():
        assert _sync_warnings(lambda: elem.track(beam).particles) == []
    assert _sync_warnings(fwd_bwd) == []


def test_captured_step_replays_like_eager_after_in_place_changes():
    import cheetah_amd as ca

    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, sigma_x=t(2e-4), sigma_tau=t(5e-5), total_charge=t(1e-9), **kw)
    lsc = ca.LSCKick(t(1.0), t(3e-4), num_bins=300, **kw)
    seg = ca.Segment([ca.Drift(t(0.5), **kw), lsc, ca.Quadrupole(t(0.2), k1=t(3.0), **kw)])

    def step():
        return (seg.track(beam).particles,)

    with torch.no_grad():
        for _ in range(3):
            step()
        captured = ca.graph.capture(step)
        first = captured()[0].clone()
        lsc.effect_length.copy_(t(4.0))
        second = captured()[0].clone()
        assert torch.equal(second, step()[0])
        lsc.beam_radius.copy_(t(1e-4))
        third = captured()[0].clone()
        assert torch.equal(third, step()[0])
    assert not torch.equal(second, first) and not torch.equal(third, second)


# ---- 10. lattices ------------------------------------------------------------------------------------------------------------------------------
def _walk(elements, beam):
    for e in elements:
        beam = e.track(beam)
    return beam


def test_segment_track_equals_the_element_walk():
    import cheetah_amd as ca

    kw = {"dtype": torch.float64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(1)
    beam = ca.ParticleBeam.from_parameters(num_particles=20_000, sigma_x=t(3e-4), sigma_y=t(2e-4), sigma_tau=t(3e-5),
                                           total_charge=t(1e-9), **kw)
    els = [ca.Drift(t(0.4), **kw), ca.LSCKick(t(0.4), num_bins=300, **kw), ca.Quadrupole(t(0.2), k1=t(4.0), **kw),
           ca.LSCKick(t(0.2), t(5e-4), num_bins=100, **kw),
           ca.Cavity(t(1.0377), voltage=t(18.15975e6), phase=t(30.0), frequency=t(1.3e9), **kw), ca.LSCKick(t(1.0377), num_bins=300, **kw)]
    seg = ca.Segment(els)
    with torch.no_grad():
        got = seg.track(beam)
        ref = _walk(els, beam)
        no_lsc = _walk([e for e in els if not isinstance(e, ca.LSCKick)], beam)
    assert float((ref.particles - no_lsc.particles)[:, 5].abs().max()) > 0
    assert torch.equal(got.particles, ref.particles)
    assert torch.equal(got.s, ref.s) and torch.equal(got.energy, ref.energy)


def _line(kw):
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    return ca.Segment([ca.Drift(t(1.0), **kw), ca.Quadrupole(t(0.2), k1=t(2.0), **kw), ca.Drift(t(1.5), **kw),
                       ca.Quadrupole(t(0.2), k1=t(-2.0), **kw), ca.Marker(**kw), ca.Drift(t(1.0), **kw)])


def test_with_lsc_kicks_at_zero_charge_matches_the_original_segment():
    import cheetah_amd as ca

    kw = {"dtype": torch.float64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(2)
    beam = ca.ParticleBeam.from_parameters(num_particles=20_000, sigma_x=t(2e-4), sigma_px=t(2e-5), sigma_y=t(1e-4),
                                           sigma_py=t(1e-5), sigma_tau=t(1e-4), sigma_p=t(1e-3), total_charge=t(0.0), **kw)
    line = _line(kw)
    split = line.with_lsc_kicks(num_bins=200, max_step=0.5)
    assert sum(isinstance(e, ca.LSCKick) for e in split.elements) == 2 + 1 + 3 + 1 + 2
    with torch.no_grad():
        ref = line.track(beam).particles
        got = split.track(beam).particles
    scale = ref.abs().max(dim=0).values
    assert torch.all((got - ref).abs().max(dim=0).values <= 1e-12 * scale), ((got - ref).abs().max(dim=0).values / scale)


def test_energy_chirp_grows_with_the_charge():
    import cheetah_amd as ca

    kw = {"dtype": torch.float64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    split = _line(kw).with_lsc_kicks(num_bins=100)
    torch.manual_seed(3)
    base = ca.ParticleBeam.from_parameters(num_particles=50_000, sigma_x=t(1e-4), sigma_px=t(1e-6), sigma_y=t(1e-4),
                                           sigma_py=t(1e-6), sigma_tau=t(3e-5), sigma_p=t(1e-6), energy=t(ENERGY), **kw)
    x = base.particles
    tau = x[:, 4]
    head, tail = tau < -3e-5, tau > 3e-5
    chirp, gain = [], []
    with torch.no_grad():
        for Q in (0.0, 0.25e-9, 1e-9):
            q = torch.full((x.shape[0],), Q / x.shape[0], **kw)
            out = split.track(ca.ParticleBeam(x, t(ENERGY), particle_charges=q)).particles
            d = out[:, 5] - x[:, 5]
            chirp.append(float(((tau - tau.mean()) * (out[:, 5] - out[:, 5].mean())).mean() / tau.var()))
            gain.append((float(d[head].mean()), float(d[tail].mean())))
    print("chirp", chirp, "head / tail gain", gain)
    assert chirp[0] > chirp[1] > chirp[2] and chirp[2] < 0           # delta falls towards the tail, ever more steeply
    assert gain[0] == (0.0, 0.0)
    assert 0 < gain[1][0] < gain[2][0] and 0 > gain[1][1] > gain[2][1]
