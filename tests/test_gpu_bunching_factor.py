"""ParticleBeam.bunching_factor on the GPU against its float64 definition evaluated in torch on the CPU:

    nu = 1 / lambda (or k / (2 pi)) in float64,  a = q.double() w.double(),
    F = sum a exp(-2 pi i nu tau.double()),  Q = sum a,  b = F / Q.

Every tolerance is computed from the inputs. The weights a / Q are positive and sum to 1, so the absolute error of Re b and of
Im b is at most the largest error of one term, with T = max |nu tau| (turns):

    float64 beam: 2 pi T 2^-52 + 4 * 2^-53        (the rounding of nu tau, and of sincospi)
    float32 beam: 2 pi (T 2^-52 + 2^-26) + E_SC   (... the fraction of the phase rounded to float32, and the float32 evaluator)

E_SC = 2.5 * 2^-24 is the derived bound of the library's own float32 sin / cos evaluator ("Bunching factor";
the derivation stands beside turn_sincos_f32 in csrc/chx_bunching.hip). One process, no workers."""
import functools
import math
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

TWO_PI = 2.0 * math.pi
E_SC = 2.5 * 2.0 ** -24
DTYPES = [torch.float32, torch.float64]
#: (sigma_tau, shortest wavelength, longest wavelength): 1 mm down to 0.1 um is about 4e4 turns, 10 um down to 1 um about 40
SCALES = {"1mm_0.1um": (1e-3, 1e-7, 1e-4), "10um_1um": (1e-5, 1e-6, 1e-4)}


def _sizes():
    import cheetah_amd as ca

    chunk, tile = ca._ops.BUNCHING_CHUNK, ca._ops.BUNCHING_K_TILE
    return [1, 63, 64, 65, chunk - 1, 3 * chunk + 5], [1, 3, 64, 65, tile + 1]


def _term_bound(dtype, T: float) -> float:
    if dtype == torch.float64:
        return TWO_PI * T * 2.0 ** -52 + 4 * 2.0 ** -53
    return TWO_PI * (T * 2.0 ** -52 + 2.0 ** -26) + E_SC


def _definition(tau, w, q, nu):
    """(F_re, F_im, Q) of the definition, float64 on the CPU; tau, w, q (*batch, N), nu (*batch, K) already broadcast;
    differentiable in tau, w and q."""
    a = q * w
    theta = TWO_PI * (nu[..., None, :] * tau[..., :, None])
    return (a[..., None] * torch.cos(theta)).sum(-2), -(a[..., None] * torch.sin(theta)).sum(-2), a.sum(-1)


def _reference(particles, survival, charges, nu):
    """b (*batch, K) complex128 and T = max |nu tau| of the definition, everything broadcast against the batch shape."""
    batch = torch.broadcast_shapes(particles.shape[:-2], survival.shape[:-1], charges.shape[:-1], nu.shape[:-1])
    N, K = particles.shape[-2], nu.shape[-1]
    tau = particles[..., 4].cpu().double().expand(*batch, N)
    w = survival.cpu().double().expand(*batch, N)
    q = charges.cpu().double().expand(*batch, N)
    f = nu.cpu().double().expand(*batch, K)
    re, im, Q = _definition(tau, w, q, f)
    T = (f.abs().amax(-1) * torch.where(q * w != 0, tau.abs(), 0.0).amax(-1)).max().item()     # (of the particles that carry weight)
    return torch.complex(re, im) / Q[..., None], T


def _max_err(got, ref):
    d = torch.view_as_real(got.cpu()) - torch.view_as_real(ref)
    return d.abs().max().item()


@functools.lru_cache(maxsize=None)
def _data(dtype, scale: str, N: int):
    """A (2, 3) batch of N particles with every input the broadcast cases need, and the wavelengths of the largest K."""
    sigma, lam_lo, lam_hi = SCALES[scale]
    K = _sizes()[1][-1]
    g = torch.Generator().manual_seed(1000 + N)
    x = torch.randn(2, 3, N, 7, generator=g, dtype=torch.float64) * 1e-4
    x[..., 4] = torch.randn(2, 3, N, generator=g, dtype=torch.float64) * sigma
    x[..., 6] = 1.0
    w = torch.rand(2, 3, N, generator=g, dtype=torch.float64)
    w[..., 1::5] = 0.0
    q = (0.5 + torch.rand(2, 3, N, generator=g, dtype=torch.float64)) * 1e-15
    lam = torch.logspace(math.log10(lam_lo), math.log10(lam_hi), K, dtype=torch.float64)
    lam3 = lam * (1.0 + torch.rand(3, K, generator=g, dtype=torch.float64))
    lam3[:, 0] = lam_lo
    dev = lambda t: t.to(dtype).cuda()  # noqa: E731
    return {"x": dev(x), "w": dev(w), "q": dev(q), "q_shared": dev(q[0, 0]), "lam": lam.cuda(), "lam3": lam3.cuda()}


def _cases(d):
    """The three broadcast combinations of batch shape (2, 3): (name, particles, survival, charges, wavelengths)."""
    return [("charges (N,)", d["x"], d["w"], d["q_shared"], d["lam"]),
            ("nu per row (3, K)", d["x"], d["w"], d["q"], d["lam3"]),
            ("particles (1, 1, N, 7)", d["x"][:1, :1], d["w"], d["q"], d["lam"])]


@functools.lru_cache(maxsize=None)
def _case_reference(dtype, scale: str, N: int, case: int):
    _, x, w, q, lam = _cases(_data(dtype, scale, N))[case]
    return _reference(x, w, q, 1.0 / lam.cpu())


def _energy(dtype):
    return torch.tensor(1e8, dtype=dtype, device="cuda")


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("N", _sizes()[0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_matches_the_float64_definition(dtype, N, scale):
    import cheetah_amd as ca

    d = _data(dtype, scale, N)
    for case, (name, x, w, q, lam) in enumerate(_cases(d)):
        ref, T = _case_reference(dtype, scale, N, case)      # at the largest K; T of a subset of its wavelengths is no larger
        bound = _term_bound(dtype, T)
        beam = ca.ParticleBeam(x, _energy(dtype), particle_charges=q, survival_probabilities=w)
        for K in _sizes()[1]:
            got = beam.bunching_factor(lam[..., :K])
            assert got.dtype == torch.complex128 and got.shape == (2, 3, K)
            err = _max_err(got, ref[..., :K])
            print(f"{name}: dtype {dtype}, N {N}, K {K}, {scale}: T {T:.3g}, error {err:.3g}, bound {bound:.3g}")
            assert err <= bound, (name, N, K, err, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_equally_spaced_particles(dtype):
    """N equal particles at spacing d: |b(k)| = |sin(N k d / 2) / (N sin(k d / 2))|: 1 at k = 2 pi / d, 0 at k = 2 pi / (N d).
    d is a power of two, so that the positions are exact in float32 as well."""
    import cheetah_amd as ca

    d = 2.0 ** -20
    for N in (1000, 3 * ca._ops.BUNCHING_CHUNK + 5):
        x = torch.zeros(N, 7, dtype=dtype, device="cuda")
        x[:, 4] = torch.arange(N, dtype=dtype, device="cuda") * d
        x[:, 6] = 1.0
        beam = ca.ParticleBeam(x, _energy(dtype), particle_charges=torch.ones(N, dtype=dtype, device="cuda"))   # (exact sums)
        lam = torch.tensor([d, N * d, 2.75 * d, 17.3 * d], dtype=torch.float64)
        b = beam.bunching_factor(lam.cuda()).cpu()
        kd2 = math.pi * d / lam
        # exact: b = exp(-i (N - 1) k d / 2) sin(N k d / 2) / (N sin(k d / 2)); 1 at lambda = d, 0 at lambda = N d
        want = torch.polar((torch.sin(N * kd2) / (N * torch.sin(kd2))), -(N - 1) * kd2)
        want[0], want[1] = 1.0, 0.0
        for i in range(4):
            bound = _term_bound(dtype, (N - 1) * d / lam[i].item())
            err = torch.view_as_real(b[i] - want[i]).abs().max().item()
            print(f"N {N}, lambda / d {lam[i].item() / d:.4g}: b {b[i].item()}, expected {want[i].item()}, error {err:.3g}, bound {bound:.3g}")
            assert err <= bound
        assert b[0].real.item() == 1.0 and b[0].imag.item() == 0.0          # whole turns: every phase reduces to exactly 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_particles_without_weight_contribute_exactly_nothing(dtype):
    """A select, not a product: lost particles keep whatever coordinates they had, NaN and inf among them."""
    import cheetah_amd as ca

    chunk = ca._ops.BUNCHING_CHUNK
    M = chunk + 700
    d = _data(dtype, "10um_1um", 3 * chunk + 5)
    x, q, lam = d["x"][0, 0, :M], d["q"][0, 0, :M], d["lam"][:65]
    live = ca.ParticleBeam(x, _energy(dtype), particle_charges=q).bunching_factor(lam)
    # 1. as many lost particles again, behind the live ones (these keep their places in the sums): bit for bit the beam without them
    x2 = torch.cat([x, x]).clone()
    x2[M:, 4] = float("nan")
    x2[M + 1::3, 4] = float("inf")
    w2 = torch.cat([torch.ones(M, dtype=dtype, device="cuda"), torch.zeros(M, dtype=dtype, device="cuda")])
    both = ca.ParticleBeam(x2, _energy(dtype), particle_charges=torch.cat([q, q]), survival_probabilities=w2).bunching_factor(lam)
    assert torch.equal(torch.view_as_real(both), torch.view_as_real(live))
    # 2. lost particles in between: what their tau holds changes no bit, and the result is the live beam's to the tolerance (the
    #    live particles now sit in other partial sums)
    idx = torch.arange(2 * M, device="cuda")
    x3 = x.repeat_interleave(2, dim=0)
    w3 = (idx % 2 == 0).to(dtype)
    q3 = q.repeat_interleave(2)
    x3_nan = x3.clone()
    x3_nan[1::2, 4] = float("nan")
    x3_nan[1::4, 4] = float("-inf")
    finite = ca.ParticleBeam(x3, _energy(dtype), particle_charges=q3, survival_probabilities=w3).bunching_factor(lam)
    lost = ca.ParticleBeam(x3_nan, _energy(dtype), particle_charges=q3, survival_probabilities=w3).bunching_factor(lam)
    assert torch.isfinite(torch.view_as_real(lost)).all()
    assert torch.equal(torch.view_as_real(lost), torch.view_as_real(finite))
    ref, T = _reference(x, torch.ones_like(q), q, 1.0 / lam)
    assert _max_err(lost, ref) <= _term_bound(dtype, T) and _max_err(live, ref) <= _term_bound(dtype, T)
    # 3. the same with the charge as the factor that is zero
    q0 = torch.where(idx % 2 == 0, q3, torch.zeros_like(q3))
    by_charge = ca.ParticleBeam(x3_nan, _energy(dtype), particle_charges=q0).bunching_factor(lam)
    assert torch.equal(torch.view_as_real(by_charge), torch.view_as_real(finite))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rows(dtype):
    import cheetah_amd as ca

    N = 500
    d = _data(dtype, "10um_1um", 3 * ca._ops.BUNCHING_CHUNK + 5)
    x = d["x"][0, :, :N].clone()                            # (3, N, 7)
    w = torch.ones(3, N, dtype=dtype, device="cuda")
    lam = d["lam"][:5]
    clean = ca.ParticleBeam(x, _energy(dtype), survival_probabilities=w).bunching_factor(lam)
    assert torch.isfinite(torch.view_as_real(clean)).all()
    # a row of total weight 0: 0 / 0
    w0 = w.clone()
    w0[1] = 0.0
    b = ca.ParticleBeam(x, _energy(dtype), survival_probabilities=w0).bunching_factor(lam)
    assert torch.isnan(b[1].real).all() and torch.isnan(b[1].imag).all()
    assert torch.equal(torch.view_as_real(b[[0, 2]]), torch.view_as_real(clean[[0, 2]]))
    # a NaN (an infinite) tau that carries weight: its row is NaN, the other rows keep their bits
    for bad in (float("nan"), float("inf")):
        xn = x.clone()
        xn[1, 17, 4] = bad
        b = ca.ParticleBeam(xn, _energy(dtype), survival_probabilities=w).bunching_factor(lam)
        assert torch.isnan(b[1].real).all() and torch.isnan(b[1].imag).all()
        assert torch.equal(torch.view_as_real(b[[0, 2]]), torch.view_as_real(clean[[0, 2]]))


@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_wavenumbers_and_wavelengths_agree(dtype, scale):
    import cheetah_amd as ca

    N = 3 * ca._ops.BUNCHING_CHUNK + 5
    d = _data(dtype, scale, N)
    x, w, q, lam = d["x"][1, 2], d["w"][1, 2], d["q"][1, 2], d["lam"][:65]
    beam = ca.ParticleBeam(x, _energy(dtype), particle_charges=q, survival_probabilities=w)
    k = TWO_PI / lam
    by_lam = beam.bunching_factor(lam)
    by_k = beam.bunching_factor(wavenumbers=k)
    # each against the definition with its own nu (1 / lambda, k / (2 pi)); then the two differ by at most both bounds
    ref_lam, T = _reference(x, w, q, 1.0 / lam)
    ref_k, Tk = _reference(x, w, q, k / TWO_PI)
    print(f"{dtype}, {scale}: T {T:.3g}, errors {_max_err(by_lam, ref_lam):.3g} {_max_err(by_k, ref_k):.3g}, "
          f"difference {_max_err(by_k, by_lam.cpu()):.3g}, bound {_term_bound(dtype, T):.3g}")
    assert _max_err(by_lam, ref_lam) <= _term_bound(dtype, T)
    assert _max_err(by_k, ref_k) <= _term_bound(dtype, Tk)
    assert _max_err(by_k, by_lam.cpu()) <= _term_bound(dtype, T) + _term_bound(dtype, Tk)
    # a float, a list and a CPU tensor are the same wavelengths
    one = beam.bunching_factor(lam[3].item())
    assert one.shape == (1,) and torch.equal(torch.view_as_real(one), torch.view_as_real(by_lam[3:4]))
    assert torch.equal(torch.view_as_real(beam.bunching_factor(lam.tolist())), torch.view_as_real(by_lam))
    assert torch.equal(torch.view_as_real(beam.bunching_factor(lam.cpu())), torch.view_as_real(by_lam))


def test_two_calls_are_bitwise_equal():
    import cheetah_amd as ca

    N = 3 * ca._ops.BUNCHING_CHUNK + 5
    for dtype in DTYPES:
        d = _data(dtype, "1mm_0.1um", N)
        beam = ca.ParticleBeam(d["x"], _energy(dtype), particle_charges=d["q"], survival_probabilities=d["w"])
        a = beam.bunching_factor(d["lam"][:65])
        torch.cuda.synchronize()
        b = beam.bunching_factor(d["lam"][:65])
        assert torch.equal(torch.view_as_real(a).view(torch.int64), torch.view_as_real(b).view(torch.int64))


def test_gradcheck_small_beam():
    import cheetah_amd as ca

    g = torch.Generator().manual_seed(20)
    N, K = 37, 5
    x = torch.randn(N, 7, generator=g, dtype=torch.float64)           # tau of order 1 m and nu of order 1 / m: phases of order 1
    x[:, 6] = 1.0
    x = x.cuda().requires_grad_()
    w = (0.5 + torch.rand(N, generator=g, dtype=torch.float64)).cuda().requires_grad_()
    q = (1.0 + torch.rand(N, generator=g, dtype=torch.float64)).cuda().requires_grad_()
    lam = (1.0 + 9.0 * torch.rand(K, generator=g, dtype=torch.float64)).cuda()
    energy = _energy(torch.float64)

    def f(x, w, q):
        return torch.view_as_real(ca.ParticleBeam(x, energy, particle_charges=q, survival_probabilities=w).bunching_factor(lam))

    assert torch.autograd.gradcheck(f, (x, w, q), eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_match_autograd_through_the_definition(dtype):
    """Batch (2,) with the charges shared by both rows, so that the backward pass sums its rows. With a cotangent g of F and
    theta = 2 pi nu tau, d tau_i = a_i sum_k 2 pi nu_k (-g_re sin theta - g_im cos theta) and d a_i = sum_k (g_re cos theta -
    g_im sin theta) + g_Q: every term carries the error E of one sin / cos of the forward pass, so d tau_i is within
    a_i sum_k |g_k| 2 pi nu_k E and d a_i within sum_k |g_k| E, plus the rounding of the output to the beam's dtype."""
    import cheetah_amd as ca

    N, K = 3 * ca._ops.BUNCHING_CHUNK + 5, 65
    d = _data(dtype, "10um_1um", N)
    x0, w0, q0, lam = d["x"][0, :2], d["w"][0, :2], d["q_shared"], d["lam"][:K]
    nu = 1.0 / lam
    g = torch.Generator().manual_seed(21)
    G = torch.randn(2, K, 2, generator=g, dtype=torch.float64)
    gQ = torch.randn(2, generator=g, dtype=torch.float64)

    x, w, q = x0.detach().clone().requires_grad_(), w0.detach().clone().requires_grad_(), q0.detach().clone().requires_grad_()
    F, Q = ca._ops.bunching(x, w, q, nu)
    ((torch.view_as_real(F) * G.cuda()).sum() + (Q * gQ.cuda()).sum()).backward()

    tau = x0[..., 4].cpu().double().requires_grad_()
    wr, qr = w0.cpu().double().requires_grad_(), q0.cpu().double().requires_grad_()
    re, im, Qr = _definition(tau, wr, qr.expand(2, N), nu.cpu().expand(2, K))
    ((re * G[..., 0]).sum() + (im * G[..., 1]).sum() + (Qr * gQ).sum()).backward()

    eps = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    T = (nu.max() * x0[..., 4].abs().max()).item()
    E = _term_bound(dtype, T)
    gabs = torch.view_as_complex(G).abs()                               # (2, K)
    S = gabs.sum(-1)[:, None]                                            # sum_k |g_k| per row
    Snu = (gabs * TWO_PI * nu.cpu()).sum(-1)[:, None]                   # sum_k |g_k| 2 pi nu_k
    a = (wr * qr).detach()
    # particles: column 4 carries the gradient, the other columns are exactly 0
    other = [0, 1, 2, 3, 5, 6]
    assert (x.grad[..., other] == 0).all()
    err_tau = (x.grad[..., 4].cpu().double() - tau.grad).abs()
    bound_tau = a * Snu * E + tau.grad.abs() * eps
    print(f"{dtype}: E {E:.3g}; d tau: worst error / bound {(err_tau / bound_tau.clamp_min(1e-300)).max().item():.3g}")
    assert (err_tau <= bound_tau).all()
    assert (x.grad[..., 4][w0 == 0] == 0).all()
    # survival: d w = d a q
    da_max = S + gQ.abs()[:, None]                                       # |d a| <= sum_k |g_k| + |g_Q|
    err_w = (w.grad.cpu().double() - wr.grad).abs()
    bound_w = qr.detach() * (S * E + da_max * eps)
    print(f"{dtype}: d w: worst error / bound {(err_w / bound_w).max().item():.3g}")
    assert (err_w <= bound_w).all()
    # charges: d q = sum over the two rows of d a w, every row rounded to the beam's dtype before the sum, the sum rounded again
    err_q = (q.grad.cpu().double() - qr.grad).abs()
    bound_q = (wr.detach() * (S * E + da_max * eps)).sum(0) + (wr.detach() * da_max).sum(0) * eps
    print(f"{dtype}: d q: worst error / bound {(err_q / bound_q.clamp_min(1e-300)).max().item():.3g}")
    assert (err_q <= bound_q).all()


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
    lam = torch.logspace(-6, -4, 33, dtype=torch.float64, device="cuda")
    lam_list = lam.tolist()
    x = beam.particles.detach().clone().requires_grad_()
    w = beam.survival_probabilities.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(x, beam.energy, survival_probabilities=w)

    def fwd_bwd():
        x.grad = w.grad = None
        gb.bunching_factor(lam).abs().sum().backward()

    flows = {
        "a float": lambda: beam.bunching_factor(1e-6),
        "a wavenumber": lambda: beam.bunching_factor(wavenumbers=6.3e6),
        "a list": lambda: beam.bunching_factor(lam_list),
        "a device tensor": lambda: beam.bunching_factor(lam),
        "device wavenumbers": lambda: beam.bunching_factor(wavenumbers=TWO_PI / lam).abs(),
        "forward + backward": fwd_bwd,
    }
    for name, fn in flows.items():
        assert _sync_warnings(fn) == [], name


def test_captured_track_and_bunching_replay_like_eager():
    import cheetah_amd as ca

    kw = {"dtype": torch.float32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, sigma_tau=t(2e-5), **kw)
    seg = ca.Segment([ca.Drift(t(0.5), **kw), ca.Quadrupole(t(0.2), k1=t(3.0), **kw), ca.Drift(t(0.5), **kw)])
    lam = torch.logspace(-5.5, -4, 40, dtype=torch.float64, device="cuda")

    def step():
        return torch.view_as_real(seg.track(beam).bunching_factor(lam))

    with torch.no_grad():
        for _ in range(3):
            step()
        captured = ca.graph.capture(step)
        first = captured()[...].clone()
        beam.particles[:, 4] *= 0.5                        # the beam edited in place: a bunch half as long
        replayed = captured().clone()
        eager = step()
    assert torch.equal(replayed.view(torch.int64), eager.view(torch.int64))
    assert not torch.allclose(replayed, first, rtol=1e-3, atol=1e-6)
