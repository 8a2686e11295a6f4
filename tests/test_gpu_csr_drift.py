"""The CSRDriftKick element on the GPU against a float64 restatement in torch on the CPU (`_reference_row`: the element's discrete
algorithm written out directly: the deposit of `tests/test_gpu_csr.py`, the table of `tests/test_csr_drift_host.py`, whose root is
found without a graph and polished by one differentiable Newton step, the gather), the steady-state limit against CSRKick, the
decay along the drift, degenerate inputs, vectorised beams and settings, gradients (autograd through the restatement), determinism,
no host synchronisation, graph capture and a chicane with drift kicks. One process, no workers."""
import math

import pytest
import torch

from tests.test_csr_drift_host import _b_table
from tests.test_gpu_csr import (ENERGY, K_E, _beam_tensors, _bits, _check_against_reference, _chicane, _p0c, _sync_warnings, _track,
                                _walk)

pytestmark = pytest.mark.gpu

F64 = torch.float64
RADIUS = 8.0                  # of the bend whose radiation the tests' kicks carry, metres


def _reference_row(x, q, w, energy, L, Lb, theta, d, M, Z=1.0):
    """One batch row, float64 on the CPU: x (N, 7), q, w (N), energy / L / Lb / theta / d 0-d. The grid is detached."""
    tau = x[:, 4]
    td = tau.detach()
    alive = (w.detach() > 0) & torch.isfinite(td)
    if not bool(alive.any()):
        return x
    lo, hi = td[alive].min(), td[alive].max()
    h = (hi - lo) / (M - 1)
    if not h > 0:
        return x
    if float(L.detach()) == 0 or float(Lb.detach()) == 0 or float(theta.detach()) == 0:        # no kick
        return x
    phi = theta.abs()
    xh, kappa = d * phi / Lb, 24.0 * h * phi / Lb
    u = ((tau - lo) / h).clamp(0, M - 1)
    nan = torch.isnan(td)
    u = torch.where(nan, torch.full_like(u, float("nan")), u)
    k = torch.where(nan, torch.zeros_like(td), torch.floor(u.detach()).clamp(max=M - 2)).long()
    f = u - k
    c = torch.where(alive, q.abs() * w, torch.zeros_like(w))
    fd = torch.where(alive, f, torch.zeros_like(f))
    D = torch.zeros(M, dtype=F64).index_add(0, k, (1 - fd) * c).index_add(0, k + 1, fd * c)
    # S_k = sum_j b_j D_(k+j), the deposits beyond node M zero: a correlation
    S = torch.nn.functional.conv1d(torch.cat([D, torch.zeros(M - 1, dtype=F64)])[None, None], _b_table(M, xh, phi, kappa)[None, None])
    dE = K_E / (2.0 * h * h) * S[0, 0]
    kick = ((1 - f) * dE[k] + f * dE[k + 1]) * (abs(Z) * L / _p0c(energy))
    cols = list(x.unbind(-1))
    cols[5] = cols[5] + kick
    return torch.stack(cols, dim=-1)


def _reference(particles, charges, survival, energy, L, Lb, theta, d, M):
    """Broadcast batch rows of the restatement -> (*batch, N, 7) float64 on the CPU (differentiable in every float input)."""
    cpu = lambda t: t.cpu().to(F64)  # noqa: E731
    particles, charges, survival, energy, L, Lb, theta, d = map(cpu, (particles, charges, survival, energy, L, Lb, theta, d))
    batch = torch.broadcast_shapes(particles.shape[:-2], charges.shape[:-1], survival.shape[:-1], energy.shape, L.shape, Lb.shape,
                                   theta.shape, d.shape)
    N = particles.shape[-2]
    B = math.prod(batch)
    x = particles.expand(*batch, N, 7).reshape(B, N, 7)
    q = charges.expand(*batch, N).reshape(B, N)
    w = survival.expand(*batch, N).reshape(B, N)
    e, ll, lb, th, dd = (t.expand(batch).reshape(B) for t in (energy, L, Lb, theta, d))
    rows = [_reference_row(x[b], q[b], w[b], e[b], ll[b], lb[b], th[b], dd[b], M) for b in range(B)]
    return torch.stack(rows).reshape(*batch, N, 7)


def _element(L=0.3, Lb=0.4, theta=0.05, d=0.15, M=200, dtype=F64):
    import cheetah_amd as ca

    kw = {"dtype": dtype, "device": "cuda"}
    L, Lb, theta, d = (v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=F64) for v in (L, Lb, theta, d))
    return ca.CSRDriftKick(L.to(**kw), Lb.to(**kw), theta.to(**kw), d.to(**kw), num_bins=M, **kw)


def _ref_of(elem, x, q, w, energy=None):
    energy = torch.tensor(ENERGY, dtype=x.dtype) if energy is None else energy
    return _reference(x, q, w, energy, elem.effect_length, elem.bend_length, elem.bend_angle, elem.exit_distance, elem.num_bins)


def _node_spacing(x, w, M):
    """h of one batch row's grid, as the deposit forms it, in float64 on the CPU."""
    tau = x[:, 4].detach().cpu().double()
    alive = (w.cpu() > 0) & torch.isfinite(tau)
    return float(tau[alive].max() - tau[alive].min()) / (M - 1)


def _bend(yn, ratio, h, R=RADIUS):
    """(bend length, bend angle phi, exit distance) of the bend of radius R for which the radiation of its whole arc spans yn node
    spacings (y = u(phi) / h) at xh = ratio phi: phi^3 = 24 yn h (1 + ratio) / (R (1 + 4 ratio))."""
    phi = (24 * yn * h * (1 + ratio) / (R * (1 + 4 * ratio))) ** (1 / 3)
    return R * phi, phi, ratio * phi * R


def _y_cases(M):
    """Sub-node, a few nodes, inside the grid twice, beyond the grid (no boundary term)."""
    return [0.37, 2.61, M / 8 + 0.3, M / 3 + 0.2, 2.0 * M]


RATIOS = [0.0, 1e-3, 1.0, 50.0]           # xh / phi: the bend's exit face, the closed form of G, both branches, the series


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M", [2, 3, 64, 65, 500, 4096])
@pytest.mark.parametrize("N", [1000, 100_000])
def test_matches_the_float64_restatement(N, M, dtype):
    x, q, w = _beam_tensors(N, dtype, seed=N + M)
    h = _node_spacing(x, w, M)
    worst = 0.0
    for yn in _y_cases(M):
        for ratio in RATIOS:
            Lb, phi, d = _bend(yn, ratio, h)
            elem = _element(0.4, Lb, -phi, d, M, dtype=dtype)
            out = _track(elem, x, q, w)
            assert out.particles.dtype == dtype and out.particles.shape == (N, 7)
            ref = _ref_of(elem, x, q, w)
            kick = (ref - x.cpu().double())[:, 5].abs().max()
            worst = max(worst, float((out.particles.cpu().double() - ref).abs().max() / kick))
            # the bound of tests/test_gpu_csr.py as it stands. It holds because the table is the same on both sides bit for bit: with a
            # library cbrt for Newton's start and a library log1p in G (an ulp apart between the device and the CPU in some entries)
            # the M = 4096 cases missed it, the entries' last bits magnified by the second differences of a long table
            _check_against_reference(out.particles, ref, x, dtype)
            assert out.particle_charges is q and out.survival_probabilities is w
    print(f"N {N}, M {M}, {dtype}: largest deviation / largest kick {worst:.3e}")


# ---- 2. the steady-state limit ----------------------------------------------------------------------------------------------------
#: the largest deviation from CSRKick's output relative to the largest kick, measured on an MI355X (float64; 50 000 particles)
STEADY_MEASURED = {64: 1.130e-15, 500: 3.599e-14}


@pytest.mark.parametrize("M", [64, 500])
def test_at_the_exit_face_of_a_long_bend_equals_csrkick(M):
    """xh = 0 and y = 2 M: the table is the steady state's algebraically, formed from Newton-polished cube roots and differences
    of G = psi^2 / 2 instead of CSRKick's cancellation-free a_j, so the two outputs agree to the tables' rounding, not bit for bit.
    The bound is 4 times the measured deviation (`STEADY_MEASURED`)."""
    import cheetah_amd as ca

    x, q, w = _beam_tensors(50_000, F64, seed=M)
    x[:, 5] = 0.0                                      # delta_out is the kick itself, rounded once
    h = _node_spacing(x, w, M)
    kw = {"dtype": F64, "device": "cuda"}
    L = 0.4
    Lb, phi, d = _bend(2.0 * M, 0.0, h)
    assert d == 0.0
    steady = _track(ca.CSRKick(torch.tensor(L, **kw), torch.tensor(L / RADIUS, **kw), num_bins=M, **kw), x, q, w).particles
    out = _track(_element(L, Lb, phi, 0.0, M), x, q, w).particles
    largest = float(steady[:, 5].abs().max())
    assert largest > 0
    dev = float((out - steady)[:, 5].abs().max()) / largest
    print(f"M {M}: deviation from CSRKick / largest kick {dev:.3e}")
    assert dev <= 4 * STEADY_MEASURED[M]
    inside = _track(_element(L, *_bend(0.2 * M, 0.0, h)[:2], 0.0, M), x, q, w).particles
    assert float((inside - steady)[:, 5].abs().max()) > 1e-3 * largest


# ---- 3. decay along the drift -------------------------------------------------------------------------------------------------------
def test_kick_decays_along_the_drift():
    import cheetah_amd as ca

    x, q, w = _beam_tensors(100_000, F64, seed=31)
    x[:, 5] = 0.0
    kw = {"dtype": F64, "device": "cuda"}
    L, Lb, theta, M = 0.2, 0.4, 0.05, 200
    rms = [float(_track(_element(L, Lb, theta, d, M), x, q, w).particles[:, 5].std()) for d in (0.0, 0.1, 1.0, 10.0)]
    steady = float(_track(ca.CSRKick(torch.tensor(L, **kw), torch.tensor(L * theta / Lb, **kw), num_bins=M, **kw), x, q,
                          w).particles[:, 5].std())
    print(f"rms kick at 0, 0.1, 1, 10 m behind the bend: {rms}; CSRKick on the same radius: {steady}")
    assert rms[0] > rms[1] > rms[2] > rms[3] > 0
    assert rms[0] < steady


# ---- 4. degenerate inputs -----------------------------------------------------------------------------------------------------------
def test_degenerate_inputs_leave_the_beam_bit_for_bit():
    for dtype in (torch.float32, torch.float64):
        x, q, w = _beam_tensors(3000, dtype, seed=1)
        x[5, 4] = float("nan")
        x2 = x.clone()
        x2[:, 4] = 3e-6                                 # a single tau value: no grid
        live = _element(0.3, 0.4, 0.05, 0.1, 50, dtype)
        assert not torch.equal(_bits(_track(live, x, q, w).particles), _bits(x))
        for elem, xx, qq, ww in ((_element(0.0, 0.4, 0.05, 0.1, 50, dtype), x, q, w), (_element(0.3, 0.0, 0.05, 0.1, 50, dtype), x, q, w),
                                 (_element(0.3, 0.4, 0.0, 0.1, 50, dtype), x, q, w), (_element(0.0, 0.0, 0.0, 0.0, 50, dtype), x, q, w),
                                 (live, x, torch.zeros_like(q), w), (live, x, q, torch.zeros_like(w)), (live, x2, q, w)):
            out = _track(elem, xx, qq, ww)
            assert torch.equal(_bits(out.particles), _bits(xx))


def test_nan_tau_poisons_that_particle_only():
    for dtype in (torch.float32, torch.float64):
        x, q, w = _beam_tensors(4000, dtype, seed=5)
        w[10] = 0.0                                    # it does not deposit either way: the others' grid is the same
        elem = _element(0.3, *_bend(5.4, 1.0, _node_spacing(x, w, 64)), 64, dtype)
        clean = _track(elem, x, q, w).particles
        x[10, 4] = float("nan")
        out = _track(elem, x, q, w).particles
        assert torch.isnan(out[10, 5])
        others = torch.ones(4000, dtype=torch.bool, device="cuda")
        others[10] = False
        assert torch.equal(_bits(out[others]), _bits(clean[others]))
        assert not torch.equal(out[others], x[others])
        # and a surviving particle with a NaN tau does not deposit
        w[10] = 1.0
        alive = _track(elem, x, q, w).particles
        assert torch.isnan(alive[10, 5]) and torch.equal(_bits(alive[others]), _bits(clean[others]))
        _check_against_reference(out[others], _ref_of(elem, x, q, w)[others.cpu()], x[others], dtype)


# ---- 5. vectorised ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_vectorised_beam_and_settings_equal_single_rows(dtype):
    N, M = 4000, 100
    x, q, w = _beam_tensors(N, dtype, batch=(3,), seed=7)
    kw = {"dtype": dtype, "device": "cuda"}
    h = _node_spacing(x[0], w, M)
    Lb, phi, d = _bend(6.3, 1.0, h)
    dist = (d * torch.tensor([0.0, 1.0, 30.0], dtype=F64)).to(**kw)                       # (3,)
    theta = (phi * torch.tensor([1.0, -1.7], dtype=F64)).reshape(2, 1, 1).to(**kw)        # (2, 1, 1)
    L, Lb = torch.tensor(0.3, **kw), torch.tensor(Lb, **kw)
    out = _track(_element(L, Lb, theta, dist, M, dtype), x, q, w).particles
    assert out.shape == (2, 1, 3, N, 7)
    for i in range(2):
        for j in range(3):
            row = _track(_element(L, Lb, theta[i, 0, 0].clone(), dist[j].clone(), M, dtype), x[j], q, w).particles
            assert torch.equal(_bits(out[i, 0, j]), _bits(row)), (i, j)
    ref = _reference(x, q, w, torch.tensor(ENERGY, dtype=dtype), L, Lb, theta, dist, M)
    _check_against_reference(out, ref, x.expand(2, 1, 3, N, 7), dtype)


# ---- 6. gradients ----------------------------------------------------------------------------------------------------------------
NAMES = ["particles", "charges", "survival", "energy", "effect_length", "bend_length", "bend_angle", "exit_distance"]


@pytest.mark.parametrize("M,yn,ratio,batch", [(64, 8.3, 50.0, ()), (64, 8.3, 1e-3, ()), (64, 21.53, 1.0, (3,)), (64, 130.0, 0.0, ()),
                                              (500, 166.87, 1.0, ()), (500, 62.8, 50.0, ())])
def test_gradients_match_autograd_through_the_restatement(M, yn, ratio, batch):
    """Every input against autograd through the restatement, with the bound of tests/test_gpu_binned_kick_grads.py: 1e-9 of the
    largest reference gradient per leaf. xh / phi = 50 lies in the series branch of G (psi / xh <= 0.02), 1e-3 in the closed form
    (psi_1 / xh = 1000 (1 / y)^(1/3) > 400), 1 in both; y = 130 at M = 64 has no boundary term; M = 500 is beyond one node tile.
    The settings are rounded to four significant digits; y stays at least 0.1 away from an integer (or beyond the grid), so
    floor(y) is the same on both sides."""
    import cheetah_amd as ca

    N = 1000
    x, q, w = _beam_tensors(N, F64, batch=batch, seed=8)
    kw = {"dtype": F64, "device": "cuda"}
    rows = [x[b] for b in range(batch[0])] if batch else [x]
    hs = [_node_spacing(r, w, M) for r in rows]
    r4 = lambda v: float(f"{v:.4g}")  # noqa: E731
    Lb, phi, d = (r4(v) for v in _bend(yn, ratio, hs[0]))
    for hh in hs:                                                    # the rows' grids differ a little: y of every row
        xh, kappa = d * phi / Lb, 24 * hh * phi / Lb
        y = phi ** 3 * (phi + 4 * xh) / (kappa * (phi + xh))
        assert y > M + 1 or abs(y - round(y)) > 0.1, y
    energy = torch.tensor(ENERGY, **kw)
    L = torch.tensor([0.3, 0.7, 0.5] if batch else 0.4, **kw)
    inputs = (x, q, w, energy, L, torch.tensor(Lb, **kw), torch.tensor(-phi, **kw), torch.tensor(d, **kw))
    leaves = [t.clone().requires_grad_() for t in inputs]
    X, Q, W, E, LL, LB, TH, DD = leaves
    elem = _element(0.4, 0.4, 0.05, 0.1, M)
    elem.effect_length, elem.bend_length, elem.bend_angle, elem.exit_distance = LL, LB, TH, DD
    out = elem.track(ca.ParticleBeam(X, E, particle_charges=Q, survival_probabilities=W)).particles
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(3), dtype=F64)
    (out * cot.cuda()).sum().backward()
    got = [t.grad.cpu() for t in leaves]

    rl = [t.detach().cpu().clone().requires_grad_() for t in inputs]
    ref = _reference(*rl, M)
    _check_against_reference(out.detach(), ref, x, F64)
    (ref * cot).sum().backward()
    failed = []
    for name, a, r in zip(NAMES, got, rl):
        b = r.grad
        if name == "exit_distance" and ratio == 0.0:
            assert d == 0.0 and torch.isfinite(a).all()              # the one-sided derivative at the exit face
        scale = b.abs().max()
        assert scale > 0, name
        err = float((a - b).abs().max() / scale)
        print(f"{name}: max error / max |gradient| {err:.3e}")
        if not err <= 1e-9:
            failed.append((name, err))
    assert not failed, failed
    assert float(got[0][..., 4].abs().max()) > 0                      # the tau column gets the node coordinate's term


def test_gradient_where_there_is_no_kick_is_zero():
    import cheetah_amd as ca

    x, q, w = _beam_tensors(2000, F64, seed=13)
    kw = {"dtype": F64, "device": "cuda"}
    for vals in ((0.0, 0.4, 0.05, 0.1), (0.3, 0.0, 0.05, 0.1), (0.3, 0.4, 0.0, 0.1), (0.0, 0.0, 0.0, 0.0)):
        L, Lb, theta, d = (torch.tensor(v, **kw).requires_grad_() for v in vals)
        xx = x.clone().requires_grad_()
        beam = ca.ParticleBeam(xx, torch.tensor(ENERGY, **kw), particle_charges=q, survival_probabilities=w)
        ca.CSRDriftKick(L, Lb, theta, d, num_bins=50, **kw).track(beam).particles[:, 5].sum().backward()
        assert all(float(t.grad) == 0.0 for t in (L, Lb, theta, d)), vals
        assert torch.isfinite(xx.grad).all() and float(xx.grad[:, 4].abs().max()) == 0.0


# ---- 7. determinism, synchronisation, capture -------------------------------------------------------------------------------------
def test_two_identical_calls_are_bit_equal():
    import cheetah_amd as ca

    x, q, w = _beam_tensors(200_000, torch.float32, seed=12)
    elem = _element(0.3, *_bend(500 / 8 + 0.3, 1.0, _node_spacing(x, w, 500)), 500, torch.float32)
    elem.exit_distance.requires_grad_()
    with torch.no_grad():
        a = _track(elem, x, q, w).particles
        b = _track(elem, x, q, w).particles
    assert torch.equal(a, b) and not torch.equal(a, x)
    grads = []
    for _ in range(2):
        xx = x.clone().requires_grad_()
        elem.exit_distance.grad = None
        out = elem.track(ca.ParticleBeam(xx, torch.tensor(ENERGY, device="cuda"), particle_charges=q, survival_probabilities=w))
        out.particles[:, 5].square().sum().backward()
        grads.append((xx.grad, elem.exit_distance.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert float(grads[0][1]) != 0.0


def test_no_host_synchronisation():
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, device="cuda", dtype=torch.float32)
    assert len(_sync_warnings(lambda: float(beam.sigma_x), warm=0)) == 1          # the switch sees what it should see
    kw = {"dtype": torch.float32, "device": "cuda"}
    elem = ca.CSRDriftKick(*(torch.tensor(v, **kw).requires_grad_() for v in (0.3, 0.4, 0.05, 0.2)), num_bins=500, **kw)
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
    csr = ca.CSRDriftKick(t(0.5), t(0.4), t(0.05), t(0.1), num_bins=300, **kw)
    seg = ca.Segment([ca.Drift(t(0.5), **kw), csr, ca.Quadrupole(t(0.2), k1=t(3.0), **kw)])

    def step():
        return (seg.track(beam).particles,)

    with torch.no_grad():
        for _ in range(3):
            step()
        captured = ca.graph.capture(step)
        first = captured()[0].clone()
        csr.exit_distance.copy_(t(0.6))
        replayed = captured()[0].clone()
        eager = step()[0]
    assert torch.equal(replayed, eager)
    assert not torch.equal(replayed, first)


# ---- 8. a chicane ------------------------------------------------------------------------------------------------------------------
def test_chicane_with_drift_kicks_tracks_like_the_element_walk():
    """Every drift of the chicane is split and every piece is followed by its kick, so each run of the segment is one element and
    `Segment.track` is the element-by-element walk bit for bit."""
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(2)
    beam = ca.ParticleBeam.from_parameters(num_particles=100_000, sigma_x=t(2e-4), sigma_px=t(2e-5), sigma_y=t(1e-4),
                                           sigma_py=t(1e-5), sigma_tau=t(1e-4), sigma_p=t(1e-3), total_charge=t(1e-9), **kw)
    chicane = _chicane(kw)
    split = chicane.with_csr_kicks(2, transient=True, drift_kicks=2)
    bends_only = chicane.with_csr_kicks(2, transient=True)
    assert sum(isinstance(e, ca.CSRDriftKick) for e in split.elements) == 8
    assert sum(isinstance(e, ca.TransientCSRKick) for e in split.elements) == 8
    assert len(split.elements) == 32 and len(bends_only.elements) == 20
    with torch.no_grad():
        got = split.track(beam)
        walk = _walk(split.elements, beam)
        without = bends_only.track(beam)
    assert torch.equal(_bits(got.particles), _bits(walk.particles))
    assert torch.equal(got.s, walk.s)
    assert float((got.particles - without.particles)[:, 5].abs().max()) > 0
    assert torch.allclose(got.s, without.s)
