"""The TransientCSRKick element on the GPU against a float64 restatement in torch on the CPU (`_reference_row`: the element's
discrete algorithm written out directly: the deposit of `tests/test_gpu_csr.py`, the table b_j(x), the gather), the steady-state
limit against CSRKick bit for bit, a Gaussian bunch against the quadrature of the continuous formula, a bend shorter than the
formation length, scaling and degenerate inputs, vectorised beams and settings, gradients (autograd through the restatement,
gradcheck), determinism, no host synchronisation, graph capture and lattices. One process, no workers."""
import math

import pytest
import torch

from tests.test_gpu_csr import (ENERGY, K_E, _beam_tensors, _bits, _check_against_reference, _chicane, _p0c, _sync_warnings, _track,
                                _walk)

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _b_table(M, xx):
    """b_j(x), j < M, for a 0-d float64 x > 0 (differentiable in x, p = floor(x) and p4 = floor(4x) held fixed): a~_(j-1) - a~_j with
    a~_j = min(j+1, x)^(2/3) - min(j, x)^(2/3) in the cancellation-free form, -(2/3) x^(-1/3) (1 - f, f) at the lags (p, p + 1) and
    +(2/3) x^(-1/3) (1 - f4, f4) at (p4, p4 + 1); where p4 = p the two interpolations are taken together, (f - f4, f4 - f)."""
    j = torch.arange(M, dtype=F64)
    xd = float(xx.detach())
    p, p4 = int(min(math.floor(xd), M)), int(min(math.floor(4 * xd), M))
    full = (2 * j + 1) / ((j + 1).pow(4 / 3) + (j * (j + 1)).pow(2 / 3) + j.pow(4 / 3))
    pp = float(p)
    partial = xx.pow(2 / 3) if p == 0 else (xx - pp) * (xx + pp) / (xx.pow(4 / 3) + (xx * pp).pow(2 / 3) + pp ** (4 / 3))
    zero = torch.zeros((), dtype=F64)
    a = torch.where(j < p, full, torch.where(j == p, partial, zero))
    b = torch.cat([-a[:1], a[:-1] - a[1:]])
    cx = (2 / 3) * xx.pow(-1 / 3)
    f, f4 = xx - p, 4 * xx - p4
    e = lambda i: (j == i).to(F64)  # noqa: E731     (zero for a lag beyond the grid)
    if p4 == p:
        return b + cx * (f - f4) * (e(p) - e(p + 1))
    return b - cx * ((1 - f) * e(p) + f * e(p + 1)) + cx * ((1 - f4) * e(p4) + f4 * e(p4 + 1))


def _reference_row(x, q, w, energy, L, theta, d, M, Z=1.0):
    """One batch row, float64 on the CPU: x (N, 7), q, w (N), energy / L / theta / d 0-d. The grid is detached."""
    tau = x[:, 4]
    td = tau.detach()
    alive = (w.detach() > 0) & torch.isfinite(td)
    if not bool(alive.any()):
        return x
    lo, hi = td[alive].min(), td[alive].max()
    h = (hi - lo) / (M - 1)
    if not h > 0:
        return x
    xx = d.pow(3) * theta.square() / (24 * L.square() * h)
    if not float(xx) > 0:                                           # L, theta or d is 0: no kick
        return x
    u = ((tau - lo) / h).clamp(0, M - 1)
    nan = torch.isnan(td)
    u = torch.where(nan, torch.full_like(u, float("nan")), u)
    k = torch.where(nan, torch.zeros_like(td), torch.floor(u.detach()).clamp(max=M - 2)).long()
    f = u - k
    c = torch.where(alive, q.abs() * w, torch.zeros_like(w))
    fd = torch.where(alive, f, torch.zeros_like(f))
    D = torch.zeros(M, dtype=F64).index_add(0, k, (1 - fd) * c).index_add(0, k + 1, fd * c)
    n = torch.arange(M)
    lag = n[None, :] - n[:, None]                               # T[k, m] = b_(m - k) for m >= k
    T = torch.where(lag >= 0, _b_table(M, xx)[lag.clamp(min=0)], torch.zeros((), dtype=F64))
    S = T @ D
    dE = abs(Z) * 9 ** (1 / 3) * K_E * L.pow(1 / 3) * theta.abs().pow(2 / 3) * h.pow(-4 / 3) * S
    kick = ((1 - f) * dE[k] + f * dE[k + 1]) / _p0c(energy)
    cols = list(x.unbind(-1))
    cols[5] = cols[5] + kick
    return torch.stack(cols, dim=-1)


def _reference(particles, charges, survival, energy, L, theta, d, M):
    """Broadcast batch rows of the restatement -> (*batch, N, 7) float64 on the CPU (differentiable in every float input)."""
    cpu = lambda t: t.cpu().to(F64)  # noqa: E731
    particles, charges, survival, energy, L, theta, d = map(cpu, (particles, charges, survival, energy, L, theta, d))
    batch = torch.broadcast_shapes(particles.shape[:-2], charges.shape[:-1], survival.shape[:-1], energy.shape, L.shape, theta.shape,
                                   d.shape)
    N = particles.shape[-2]
    B = math.prod(batch)
    x = particles.expand(*batch, N, 7).reshape(B, N, 7)
    q = charges.expand(*batch, N).reshape(B, N)
    w = survival.expand(*batch, N).reshape(B, N)
    e, ll, th, dd = (t.expand(batch).reshape(B) for t in (energy, L, theta, d))
    rows = [_reference_row(x[b], q[b], w[b], e[b], ll[b], th[b], dd[b], M) for b in range(B)]
    return torch.stack(rows).reshape(*batch, N, 7)


def _element(L=0.3, theta=0.03, d=0.15, M=200, dtype=F64):
    import cheetah_amd as ca

    kw = {"dtype": dtype, "device": "cuda"}
    L, theta, d = (v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=F64) for v in (L, theta, d))
    return ca.TransientCSRKick(L.to(**kw), theta.to(**kw), d.to(**kw), num_bins=M, **kw)


def _ref_of(elem, x, q, w, energy=None):
    energy = torch.tensor(ENERGY, dtype=x.dtype) if energy is None else energy
    return _reference(x, q, w, energy, elem.effect_length, elem.angle, elem.entrance_distance, elem.num_bins)


def _node_spacing(x, w, M):
    """h of one batch row's grid, as the deposit forms it, in float64 on the CPU."""
    tau = x[:, 4].detach().cpu().double()
    alive = (w.cpu() > 0) & torch.isfinite(tau)
    return float(tau[alive].max() - tau[alive].min()) / (M - 1)


def _distance(xn, h, L, theta):
    """The arc length d at which the slippage length is xn node spacings: d = (24 R^2 xn h)^(1/3), R = L / |theta|."""
    return (24 * (L / abs(theta)) ** 2 * xn * h) ** (1 / 3)


def _x_cases(M):
    """Sub-node, a few nodes, 4x inside the grid, 4x beyond the grid, the steady-state table."""
    return [0.37, 2.61, M / 8 + 0.3, M / 3 + 0.2, 2.0 * M]


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M", [2, 3, 64, 65, 500, 4096])
@pytest.mark.parametrize("N", [1000, 100_000])
def test_matches_the_float64_restatement(N, M, dtype):
    x, q, w = _beam_tensors(N, dtype, seed=N + M)
    h = _node_spacing(x, w, M)
    L, theta = 0.4, -0.05
    for xn in _x_cases(M):
        elem = _element(L, theta, _distance(xn, h, L, theta), M, dtype=dtype)
        out = _track(elem, x, q, w)
        assert out.particles.dtype == dtype and out.particles.shape == (N, 7)
        # the bound of tests/test_gpu_csr.py as it stands. The restatement's own summation order does not come near it: summed in a
        # second order on the CPU (each node's sources one after the other from the far end instead of a matrix product) it moves
        # by at most 5e-15 of the largest kick (M = 4096, x >= M; N = 100 000), against the bound's 1e-12, so no margin is taken
        _check_against_reference(out.particles, _ref_of(elem, x, q, w), x, dtype)
        assert out.particle_charges is q and out.survival_probabilities is w


# ---- 2. the steady-state limit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M", [64, 500])
def test_at_x_beyond_the_grid_equals_csrkick_bit_for_bit(M, dtype):
    import cheetah_amd as ca

    x, q, w = _beam_tensors(50_000, dtype, seed=M)
    h = _node_spacing(x, w, M)
    kw = {"dtype": dtype, "device": "cuda"}
    L, theta = 0.4, -0.05
    steady = _track(ca.CSRKick(torch.tensor(L, **kw), torch.tensor(theta, **kw), num_bins=M, **kw), x, q, w).particles
    assert float((steady - x)[:, 5].abs().max()) > 0
    for xn in (1.001 * M, 2.0 * M, 1e30):
        out = _track(_element(L, theta, _distance(xn, h, L, theta), M, dtype), x, q, w).particles
        assert torch.equal(_bits(out), _bits(steady)), xn
    inside = _track(_element(L, theta, _distance(0.2 * M, h, L, theta), M, dtype), x, q, w).particles
    assert not torch.equal(inside, steady)


# ---- 3. theory ------------------------------------------------------------------------------------------------------------------
def _analytic_gaussian_moments(zl):
    """Mean and rms of the energy change of a Gaussian bunch at the slippage length zl (in sigma), in units of Q k_e L / (R^(2/3)
    sigma^(4/3)), by quadrature of the continuous formula: Delta E(z) = (2 / 3^(1/3)) { int_0^zl u^(-1/3) lambda'(z + u) du -
    zl^(-1/3) [lambda(z + zl) - lambda(z + 4 zl)] } (u = v^(3/2): no singularity), weighted with lambda(z)."""
    z = torch.linspace(-8, 8, 1601, dtype=F64)
    v = torch.linspace(0, zl ** (2 / 3), 20001, dtype=F64)
    dv = float(v[1] - v[0])
    phi = lambda s: torch.exp(-0.5 * s * s) / math.sqrt(2 * math.pi)  # noqa: E731
    G = torch.empty_like(z)
    for i in range(0, z.numel(), 200):
        s = z[i:i + 200, None] + v[None, :].pow(1.5)
        f = 1.5 * (-s * phi(s))
        G[i:i + 200] = (f.sum(dim=1) - 0.5 * (f[:, 0] + f[:, -1])) * dv
    dE = (2 / 3 ** (1 / 3)) * (G - zl ** (-1 / 3) * (phi(z + zl) - phi(z + 4 * zl)))
    wz = phi(z) / phi(z).sum()
    mean = float((wz * dE).sum())
    rms = math.sqrt(float((wz * (dE - mean) ** 2).sum()))
    return mean, rms


def _gaussian_beam(sigma, Q, N, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(N, 7, dtype=F64)
    x[:, 4] = sigma * torch.randn(N, generator=g, dtype=F64)
    x[:, 6] = 1.0
    kw = {"dtype": F64, "device": "cuda"}
    return x.to(**kw), torch.full((N,), Q / N, **kw), torch.ones(N, **kw)


def test_gaussian_bunch_matches_the_transient_theory():
    sigma, Q, R, L, M = 1e-4, 1e-9, 10.0, 1.0, 300
    d = (24 * sigma * R * R) ** (1 / 3)                         # z_L = sigma
    x, q, w = _gaussian_beam(sigma, Q, 1_000_000)
    out = _track(_element(L, L / R, d, M), x, q, w)
    p0c = float(_p0c(torch.tensor(ENERGY, dtype=F64)))
    tau, dE = x[:, 4].cpu(), (out.particles[:, 5] - x[:, 5]).cpu() * p0c
    unit = Q * K_E * L / (R ** (2 / 3) * sigma ** (4 / 3))
    mean, rms = _analytic_gaussian_moments(1.0)
    assert abs(mean + 0.4025) < 1e-3 and abs(rms - 0.2249) < 1e-3, (mean, rms)
    got_mean, got_rms = float(dE.mean()) / unit, float(dE.std()) / unit
    print(f"mean {got_mean:.5f} (quadrature {mean:.5f}), rms {got_rms:.5f} (quadrature {rms:.5f})")
    # the float64 restatement on these particles, run on the CPU, gives -0.40344 and 0.22589: it deviates from the quadrature by
    # 0.23 % of the mean and 0.45 % of the rms (deposit noise and the piecewise linear density at M = 300); twice that is below
    # 1 %, so the bound is the 1 % of the steady-state test
    assert abs(got_mean - mean) <= 0.01 * abs(mean), (got_mean, mean)
    assert abs(got_rms - rms) <= 0.01 * rms, (got_rms, rms)
    head = tau <= torch.quantile(tau[:100_000], 0.1)
    assert float(dE[head].mean()) > 0          # the head (smallest tau) gains energy
    assert float(dE[tau >= torch.quantile(tau[:100_000], 0.9)].mean()) < 0


# ---- 4. a bend shorter than the formation length -------------------------------------------------------------------------------------
def test_short_bend_loses_a_fraction_of_the_steady_state_energy():
    import cheetah_amd as ca

    sigma, Q, R, L = 1e-4, 1e-9, 10.0, 0.28
    assert L ** 3 / (24 * R * R) < 0.1 * sigma
    kw = {"dtype": F64, "device": "cuda"}
    bend = ca.Dipole(torch.tensor(L, **kw), angle=torch.tensor(L / R, **kw), name="b", **kw)
    x, q, w = _gaussian_beam(sigma, Q, 200_000, seed=4)
    beam = ca.ParticleBeam(x, torch.tensor(ENERGY, **kw), particle_charges=q, survival_probabilities=w)
    loss = []
    for transient in (True, False):
        kicks = bend.split_for_csr(8, transient=transient)[1::2]
        assert len(kicks) == 8 and all(type(k) is (ca.TransientCSRKick if transient else ca.CSRKick) for k in kicks)
        out = _walk(kicks, beam).particles
        assert torch.equal(out[:, [0, 1, 2, 3, 4, 6]], x[:, [0, 1, 2, 3, 4, 6]])            # they change delta only
        loss.append(-float((out[:, 5] - x[:, 5]).mean()))
    print(f"mean loss, transient / steady: {loss[0] / loss[1]:.4f}")
    assert loss[1] > 0 and 0 < loss[0] < 0.2 * loss[1], loss


# ---- 5. scaling and degenerate inputs -------------------------------------------------------------------------------------------
def test_kick_is_proportional_to_the_charge():
    x, q, w = _beam_tensors(50_000, F64, seed=21)
    x[:, 5] = 0.0                                      # delta_out is the kick itself, rounded once
    elem = _element(0.2, 0.01, _distance(7.3, _node_spacing(x, w, 250), 0.2, 0.01), 250)
    base = _track(elem, x, q, w).particles[:, 5].cpu()
    tripled = _track(elem, x, 3 * q, w).particles[:, 5].cpu()
    assert float(base.abs().max()) > 0
    assert float((tripled - 3 * base).abs().max()) <= 1e-12 * float(tripled.abs().max())


def test_degenerate_inputs_leave_the_beam_bit_for_bit():
    for dtype in (torch.float32, torch.float64):
        x, q, w = _beam_tensors(3000, dtype, seed=1)
        x[5, 4] = float("nan")
        one = torch.zeros_like(w)
        one[17] = 0.75
        x2 = x.clone()
        x2[:, 4] = 3e-6
        live = _element(0.3, 0.02, 0.1, 50, dtype)
        assert not torch.equal(_bits(_track(live, x, q, w).particles), _bits(x))
        for elem, xx, qq, ww in ((_element(0.3, 0.02, 0.0, 50, dtype), x, q, w), (_element(0.0, 0.02, 0.1, 50, dtype), x, q, w),
                                 (_element(0.3, 0.0, 0.1, 50, dtype), x, q, w), (_element(0.0, 0.0, 0.0, 50, dtype), x, q, w),
                                 (live, x, torch.zeros_like(q), w), (live, x, q, torch.zeros_like(w)), (live, x, q, one),
                                 (live, x2, q, w)):
            out = _track(elem, xx, qq, ww)
            assert torch.equal(_bits(out.particles), _bits(xx))


def test_nan_tau_poisons_that_particle_only():
    for dtype in (torch.float32, torch.float64):
        x, q, w = _beam_tensors(4000, dtype, seed=5)
        x[10, 4] = float("nan")
        w[10] = 1.0
        elem = _element(0.3, 0.02, _distance(5.4, _node_spacing(x, w, 64), 0.3, 0.02), 64, dtype)
        out = _track(elem, x, q, w).particles
        assert torch.isnan(out[10, 5])
        others = torch.ones(4000, dtype=torch.bool, device="cuda")
        others[10] = False
        assert torch.isfinite(out[others]).all()
        ref = _ref_of(elem, x, q, w)
        _check_against_reference(out[others], ref[others.cpu()], x[others], dtype)


def test_dead_particles_beyond_the_grid_take_the_end_nodes():
    x, q, w = _beam_tensors(3000, F64, seed=6, dead=0.0)
    x[:, 5] = 0.0
    tau = x[:, 4]
    head, tail = int(tau.argmin()), int(tau.argmax())
    x[0, 4], w[0] = tau[tail] + 1e-3, 0.0     # dead, far behind the tail
    x[1, 4], w[1] = tau[head] - 1e-3, 0.0     # dead, far ahead of the head
    elem = _element(0.3, 0.02, _distance(9.7, _node_spacing(x, w, 80), 0.3, 0.02), 80)
    out = _track(elem, x, q, w).particles
    _check_against_reference(out, _ref_of(elem, x, q, w), x, F64)
    d = (out - x)[:, 5]
    # node M - 1 (u clamped) for the one behind, node 0 for the one ahead: the kicks of the extreme survivors
    assert float(d[0]) == float(d[tail]) and float(d[1]) == float(d[head]) and float(d[head]) != 0.0


# ---- 6. vectorised ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting,shape", [("energy", (3,)), ("length", (2, 1)), ("angle", (2, 3)), ("distance", (3,)),
                                           ("distance", (2, 1))])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_vectorised_beam_and_settings_equal_single_rows(setting, shape, dtype):
    N, M, batch = 4000, 100, (2, 3)
    x, q, w = _beam_tensors(N, dtype, batch=batch, seed=7)
    kw = {"dtype": dtype, "device": "cuda"}
    vals = torch.linspace(0.5, 1.5, math.prod(shape), dtype=F64).reshape(shape)
    h = _node_spacing(x[0, 0], w, M)
    s = {"energy": torch.tensor(ENERGY, dtype=F64), "length": torch.tensor(0.3, dtype=F64), "angle": torch.tensor(-0.04, dtype=F64),
         "distance": torch.tensor(_distance(6.3, h, 0.3, 0.04), dtype=F64)}       # x from 0.8 to 21 nodes over the rows
    s[setting] = s[setting] * vals
    s = {k: v.to(**kw) for k, v in s.items()}
    elem = _element(s["length"], s["angle"], s["distance"], M, dtype)
    out = _track(elem, x, q, w, s["energy"]).particles
    assert out.shape == (*batch, N, 7)
    full = {k: v.expand(batch) for k, v in s.items()}
    for i in range(batch[0]):
        for j in range(batch[1]):
            one = {k: v[i, j].clone() for k, v in full.items()}
            row = _track(_element(one["length"], one["angle"], one["distance"], M, dtype), x[i, j], q, w, one["energy"]).particles
            assert torch.equal(_bits(out[i, j]), _bits(row)), (i, j)
    ref = _reference(x, q, w, s["energy"], s["length"], s["angle"], s["distance"], M)
    _check_against_reference(out, ref, x, dtype)


# ---- 7. gradients ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("xcase", ["2.61", "M/8+0.3"])
@pytest.mark.parametrize("batch", [(), (3,)])
def test_gradients_match_autograd_through_the_restatement(batch, xcase):
    import cheetah_amd as ca

    N, M = 1500, 37
    xn = 2.61 if xcase == "2.61" else M / 8 + 0.3               # x and 4x are not integers
    x, q, w = _beam_tensors(N, F64, batch=batch, seed=8)
    kw = {"dtype": F64, "device": "cuda"}
    energy = torch.tensor(ENERGY, **kw)
    L = torch.tensor([0.3, 0.7, 0.5] if batch else 0.4, **kw)
    theta = torch.tensor(-0.03, **kw)
    rows = [x[b] for b in range(batch[0])] if batch else [x]
    Ls = L.tolist() if batch else [float(L)]
    d = torch.tensor([_distance(xn, _node_spacing(r, w, M), Lb, 0.03) for r, Lb in zip(rows, Ls)], **kw).reshape(batch)
    leaves = [t.clone().requires_grad_() for t in (x, q, w, energy, L, theta, d)]
    X, Q, W, E, LL, TH, DD = leaves
    elem = _element(0.4, -0.03, 0.1, M)
    elem.effect_length, elem.angle, elem.entrance_distance = LL, TH, DD
    out = elem.track(ca.ParticleBeam(X, E, particle_charges=Q, survival_probabilities=W)).particles
    g = torch.Generator().manual_seed(3)
    cot = torch.randn(out.shape, generator=g, dtype=F64)
    (out * cot.cuda()).sum().backward()
    got = [t.grad.cpu() for t in leaves]

    rl = [t.detach().cpu().clone().requires_grad_() for t in (x, q, w, energy, L, theta, d)]
    ref = _reference(*rl, M)
    (ref * cot).sum().backward()
    names = ["particles", "charges", "survival", "energy", "effect_length", "angle", "entrance_distance"]
    for name, a, r in zip(names, got, rl):
        b = r.grad
        scale = b.abs().max()
        assert scale > 0, name
        assert torch.allclose(a, b, rtol=0, atol=1e-9 * scale), (name, float((a - b).abs().max() / scale))
    # the tau column gets the node coordinate's term
    assert float(got[0][..., 4].abs().max()) > 0


def test_gradcheck_small_case():
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    g = torch.Generator().manual_seed(11)
    N, M = 64, 8
    base = torch.randn(N, 7, generator=g, dtype=F64)
    base[:, 4] *= 1e-3
    base[:, 6] = 1.0
    base = base.to(**kw)
    xc, dc = (base[:, i].clone().requires_grad_() for i in (0, 5))
    # charges of order one (finite differences of step 1e-6 stay linear) and an energy that makes the kick of order 0.1
    q = (0.5 + torch.rand(N, generator=g, dtype=F64)).to(**kw).requires_grad_()
    w = (0.2 + 0.8 * torch.rand(N, generator=g, dtype=F64)).to(**kw).requires_grad_()
    energy = torch.tensor(1e15, **kw).requires_grad_()
    L = torch.tensor(0.5, **kw).requires_grad_()
    theta = torch.tensor(-0.2, **kw).requires_grad_()
    # x = 1.3, 4x = 5.2: a step of 1e-6 crosses no node
    d = torch.tensor(_distance(1.3, _node_spacing(base, torch.ones(N), M), 0.5, 0.2), **kw).requires_grad_()

    def fn(xc, dc, q, w, energy, L, theta, d):
        cols = list(base.unbind(-1))
        cols[0], cols[5] = xc, dc
        beam = ca.ParticleBeam(torch.stack(cols, dim=-1), energy, particle_charges=q, survival_probabilities=w)
        return ca.TransientCSRKick(L, theta, d, num_bins=M, **kw).track(beam).particles

    assert torch.autograd.gradcheck(fn, (xc, dc, q, w, energy, L, theta, d), eps=1e-6, atol=1e-8, rtol=1e-6)


def test_gradient_at_zero_distance_length_and_angle_is_zero():
    import cheetah_amd as ca

    x, q, w = _beam_tensors(2000, F64, seed=13)
    kw = {"dtype": F64, "device": "cuda"}
    for L0, t0, d0 in ((0.3, 0.02, 0.0), (0.0, 0.02, 0.1), (0.3, 0.0, 0.1), (0.0, 0.0, 0.0)):
        L, theta, d = (torch.tensor(v, **kw).requires_grad_() for v in (L0, t0, d0))
        xx = x.clone().requires_grad_()
        beam = ca.ParticleBeam(xx, torch.tensor(ENERGY, **kw), particle_charges=q, survival_probabilities=w)
        ca.TransientCSRKick(L, theta, d, num_bins=50, **kw).track(beam).particles[:, 5].sum().backward()
        assert float(L.grad) == 0.0 and float(theta.grad) == 0.0 and float(d.grad) == 0.0, (L0, t0, d0)
        assert torch.isfinite(xx.grad).all() and float(xx.grad[:, 4].abs().max()) == 0.0


# ---- 8. determinism, synchronisation, capture -------------------------------------------------------------------------------------
def test_two_identical_calls_are_bit_equal():
    import cheetah_amd as ca

    x, q, w = _beam_tensors(1_000_000, torch.float32, seed=12)
    elem = _element(0.3, 0.02, _distance(500 / 8 + 0.3, _node_spacing(x, w, 500), 0.3, 0.02), 500, torch.float32)
    elem.entrance_distance.requires_grad_()
    with torch.no_grad():
        a = _track(elem, x, q, w).particles
        b = _track(elem, x, q, w).particles
    assert torch.equal(a, b) and not torch.equal(a, x)
    grads = []
    for _ in range(2):
        xx = x.clone().requires_grad_()
        elem.entrance_distance.grad = None
        out = elem.track(ca.ParticleBeam(xx, torch.tensor(ENERGY, device="cuda"), particle_charges=q, survival_probabilities=w))
        out.particles[:, 5].square().sum().backward()
        grads.append((xx.grad, elem.entrance_distance.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert float(grads[0][1]) != 0.0


def test_no_host_synchronisation():
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, device="cuda", dtype=torch.float32)
    assert len(_sync_warnings(lambda: float(beam.sigma_x), warm=0)) == 1          # the switch sees what it should see
    kw = {"dtype": torch.float32, "device": "cuda"}
    elem = ca.TransientCSRKick(*(torch.tensor(v, **kw).requires_grad_() for v in (0.3, 0.02, 0.2)), num_bins=500, **kw)
    x = beam.particles.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(x, beam.energy)

    def fwd_bwd():
        x.grad = None
        elem.track(gb).particles[:, 5].sum().backward()

    with torch.no_grad():
        assert _sync_warnings(lambda: elem.track(beam).particles) == []
    assert _sync_warnings(fwd_bwd) == []


def test_captured_step_replays_like_eager_after_an_in_place_distance_change():
    import cheetah_amd as ca

    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, sigma_x=t(2e-4), sigma_tau=t(5e-5), total_charge=t(1e-9), **kw)
    csr = ca.TransientCSRKick(t(0.5), t(0.05), t(0.1), num_bins=300, **kw)
    seg = ca.Segment([ca.Drift(t(0.5), **kw), csr, ca.Quadrupole(t(0.2), k1=t(3.0), **kw)])

    def step():
        return (seg.track(beam).particles,)

    with torch.no_grad():
        for _ in range(3):
            step()
        captured = ca.graph.capture(step)
        first = captured()[0].clone()
        csr.entrance_distance.copy_(t(0.3))
        replayed = captured()[0].clone()
        eager = step()[0]
    assert torch.equal(replayed, eager)
    assert not torch.equal(replayed, first)


# ---- 9. lattice ------------------------------------------------------------------------------------------------------------------
def test_segment_track_equals_the_element_walk():
    """`Segment.track` over [Drift, pieces of split_for_csr(4, transient=True), Drift] against tracking element by element.
    Run once on an MI355X, `torch.equal(got.particles, plain.particles)` for this lattice does NOT hold: the segment composes
    consecutive linear elements into one map before it applies it, so its leading run [Drift, first Dipole piece] is rounded
    differently from two separate passes (`tests/test_gpu_csr.py` keeps one linear element between two kicks for that reason).
    The size of that deviation has not been measured yet; the test prints it, and the bound on it is the 1e-12 of the largest
    coordinate that the chicane test below puts on composed maps. What is bit for bit: without the leading drift every run is
    one element, all four kicks among them, and the plain element-by-element walk equals `Segment.track`; with it, the walk that
    tracks the leading run as the segment forms it does."""
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(1)
    beam = ca.ParticleBeam.from_parameters(num_particles=100_000, sigma_x=t(3e-4), sigma_y=t(2e-4), sigma_tau=t(3e-5),
                                           total_charge=t(1e-9), **kw)
    bend = ca.Dipole(t(0.4), angle=t(0.08), dipole_e1=t(0.02), dipole_e2=t(0.03), name="b", **kw)
    pieces = bend.split_for_csr(4, num_bins=300, transient=True)
    els = [ca.Drift(t(0.4), **kw)] + pieces + [ca.Drift(t(0.3), **kw)]
    assert sum(isinstance(e, ca.TransientCSRKick) for e in els) == 4
    with torch.no_grad():
        got = ca.Segment(els).track(beam)
        ref = _walk([ca.Segment(els[:2])] + els[2:], beam)
        plain = _walk(els, beam)
        no_csr = _walk([e for e in els if not isinstance(e, ca.TransientCSRKick)], beam)
        tail = ca.Segment(els[1:]).track(beam)
        tail_walk = _walk(els[1:], beam)
    assert float((plain.particles - no_csr.particles)[:, 5].abs().max()) > 0
    assert torch.equal(got.particles, ref.particles)
    assert torch.equal(got.s, ref.s) and torch.equal(got.s, plain.s)
    assert torch.equal(tail.particles, tail_walk.particles)
    scale = plain.particles.abs().max(dim=0).values
    dev = (got.particles - plain.particles).abs().max(dim=0).values
    print("Segment.track against the element-by-element walk, per coordinate, relative:", (dev / scale).tolist())
    assert torch.all(dev <= 1e-12 * scale), (dev / scale)


def test_with_csr_kicks_transient_at_zero_charge_matches_the_unsplit_chicane():
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(2)
    beam = ca.ParticleBeam.from_parameters(num_particles=100_000, sigma_x=t(2e-4), sigma_px=t(2e-5), sigma_y=t(1e-4),
                                           sigma_py=t(1e-5), sigma_tau=t(1e-4), sigma_p=t(1e-3), total_charge=t(0.0), **kw)
    chicane = _chicane(kw)
    split = chicane.with_csr_kicks(4, num_bins=200, transient=True)
    assert sum(isinstance(e, ca.TransientCSRKick) for e in split.elements) == 16
    with torch.no_grad():
        ref = chicane.track(beam).particles
        got = split.track(beam).particles
    scale = ref.abs().max(dim=0).values
    assert torch.all((got - ref).abs().max(dim=0).values <= 1e-12 * scale), ((got - ref).abs().max(dim=0).values / scale)
