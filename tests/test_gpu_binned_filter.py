"""`cutoff_wavelength`, the Gaussian low-pass filter of the binned-beam kicks (`Wakefield`, `CSRKick`, `TransientCSRKick`,
`CSRDriftKick`, `LSCKick`, `IBSKick`), on the GPU. One process, no workers.

The oracle is the unfiltered kick itself. The test restates the node-based deposit (as `_reference_row` of test_gpu_lsc.py) and the
filter in float64 on the CPU,

    s = cutoff / (2 pi h),  R = max(1, min(ceil(4 s), M - 1)),  g_d = exp(-d^2 / 2 s^2) / sum g,  D' = conv(pad(D, R, "symmetric"), g),

and builds a synthetic beam: the original particles as witnesses (same indices, same survival probabilities, charge 0) and one
particle exactly on every node k with the charge D'_k. The extreme surviving particles of the original beam sit at tau =
+-(M - 1) / 2 * 2^-20 m, so h = 2^-20 m exactly, every node position is exact, the node particles deposit with f = 0 and both beams
find the same grid bit for bit. The unfiltered kick of the synthetic beam then kicks the witnesses with the node values of D', which
is what the filtered kick of the original beam must give.

Bounds. float64: the two sides differ by the 2^-62 fixed-point rounding, the test's own float64 sums and the order of the device's
sums (1e-12 max|kick| in the project's tests): |difference| <= 1e-9 max|kick| + 1 ulp of the coordinate; for `IBSKick`, whose kick is
the square root of a variance (a relative error eps of a tiny variance becomes sqrt(eps)), 1e-7 max|kick|. A wrong weight, reflection
or R moves the kick by 1e-4 of its scale or more. float32 beams are compared with the filtered kick of the same values held as a
float64 beam (settings that float32 holds exactly): 2 ulp32 of the coordinate + 1e-6 max|kick| (the species' mass rounded to float32).
Cutoffs are set as 2 pi s h and s is formed from them again exactly as the kernel forms it, so R is the same on both sides."""
import math
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
ENERGY = 1e8
H = 2.0 ** -20                 # the node spacing of the pinned beams (m)
TWO_PI = 6.283185307179586     # as the kernel's
KICKS = ["wake", "csr", "csr_transient", "csr_drift", "lsc", "ibs"]
#: the columns a kick moves
MOVED = {"wake": (1, 3, 5)}
#: (M, s): R capped at 1 with both reflections at once; a node-tile boundary; a window wider than a 64-node tile (R = 70); R at the cap
FULL_CASES = [(2, 0.3), (2, 5.0), (64, 1.3), (65, 1.3), (129, 17.3), (129, 40.0)]
SHORT_CASES = [(65, 1.3), (129, 17.3)]
CASES = [(kind, M, s) for kind in KICKS for (M, s) in (FULL_CASES if kind in ("lsc", "csr") else SHORT_CASES)]


# ---- the test's own deposit and filter (float64, CPU) --------------------------------------------------------------------------------
def _cutoff(s, h=H):
    """The cutoff of about s node spacings as a number float32 holds exactly (an element keeps it in its own dtype)."""
    return float(np.float32(TWO_PI * s * h))


def _s_of(cutoff, h):
    return cutoff / (TWO_PI * h)


def _weights(s, M):
    R = int(max(1.0, min(float(math.ceil(4.0 * s)), float(M - 1))))
    d = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-d * d / (2.0 * s * s))
    return g / g.sum(), R


def _smooth(D, s):
    """D' of D (numpy, (M,)): numpy's symmetric padding, then the normalised Gaussian."""
    g, R = _weights(s, len(D))
    return np.convolve(np.pad(D, R, mode="symmetric"), g, mode="valid")


def _smoothing_matrix(s, M):
    return torch.from_numpy(np.stack([_smooth(e, s) for e in np.eye(M)], axis=1))


def _grid(tau, w, M):
    """(alive, lo, h, k, f) of one row as the kernels form them; the grid detached."""
    td = tau.detach()
    alive = (w.detach() > 0) & torch.isfinite(td)
    lo, hi = td[alive].min(), td[alive].max()
    h = (hi - lo) / (M - 1)
    u = ((tau - lo) / h).clamp(0, M - 1)
    k = torch.floor(u.detach()).clamp(max=M - 2).long()
    return alive, lo, h, k, u - k


def _deposit(k, f, c, M):
    return torch.zeros(M, dtype=F64).index_add(0, k, (1 - f) * c).index_add(0, k + 1, f * c)


def _row_deposits(x, q, w, M, transverse=False):
    alive, lo, h, k, f = _grid(x[:, 4], w, M)
    c = torch.where(alive, q.abs() * w, torch.zeros_like(w))
    f = torch.where(alive, f, torch.zeros_like(f))
    chans = [_deposit(k, f, c, M)]
    if transverse:
        chans += [_deposit(k, f, c * x[:, 0], M), _deposit(k, f, c * x[:, 2], M)]
    return lo, h, chans


# ---- beams ---------------------------------------------------------------------------------------------------------------------------
def _pinned_beam(N, M, seed, rows=1, dead_row=None):
    """float64 CPU tensors x (N, 7), q (N,), w (rows, N) whose values float32 holds exactly: the surviving particles' tau inside
    +-(M - 1) / 2 * 2^-20 with particles 0 and 1 (alive in every live row) on the two ends; some dead particles outside the range."""
    g = torch.Generator().manual_seed(seed)
    half = (M - 1) / 2 * H
    x = torch.randn(N, 7, generator=g, dtype=F64)
    x[:, 0] *= 2e-4
    x[:, 1] *= 1e-4
    x[:, 2] *= 1e-4
    x[:, 3] *= 1e-4
    x[:, 4] = (x[:, 4] * 0.3 * half).clamp(-0.999 * half, 0.999 * half)
    x[:, 5] *= 1e-3
    x[:, 6] = 1.0
    q = (1e-9 / N) * (0.5 + torch.rand(N, generator=g, dtype=F64))
    w = torch.rand(rows, N, generator=g, dtype=F64).clamp_min(0.05)
    dead = torch.rand(rows, N, generator=g) < 0.1
    w[dead] = 0.0
    x, q, w = x.float().double(), q.float().double(), w.float().double()
    x[dead.all(dim=0), 4] *= 1.5               # particles dead in every row beyond the ends as well: witnesses in the clamp
    x[0, 4], x[1, 4] = -half, half
    w[:, :2] = 0.5
    if dead_row is not None:
        w[dead_row] = 0.0
    return x.float().double(), q, w


def _synthetic(x, q, w, M, s_rows, transverse=False):
    """The synthetic beam of the module docstring: xs (N + M, 7), qs (rows, N + M), ws (rows, N + M), float64 CPU."""
    N, rows = x.shape[0], w.shape[0]
    nodes = torch.zeros(M, 7, dtype=F64)
    nodes[:, 6] = 1.0
    qs, ws = torch.zeros(rows, N + M, dtype=F64), torch.cat([w, torch.ones(rows, M, dtype=F64)], dim=1)
    for b in range(rows):
        if not bool((w[b] > 0).any()):
            ws[b, N:] = 0.0
            continue
        lo, h, chans = _row_deposits(x, q, w[b], M, transverse)
        assert float(h) == H and float(lo) == -(M - 1) / 2 * H
        nodes[:, 4] = lo + torch.arange(M, dtype=F64) * h
        filtered = [torch.from_numpy(_smooth(c.numpy(), s_rows[b])) for c in chans]
        qs[b, N:] = filtered[0]
        if transverse:
            assert rows == 1
            has = filtered[0] > 0
            one = torch.ones_like(filtered[0])
            nodes[:, 0] = torch.where(has, filtered[1] / torch.where(has, filtered[0], one), 0 * one)
            nodes[:, 2] = torch.where(has, filtered[2] / torch.where(has, filtered[0], one), 0 * one)
    return torch.cat([x, nodes]), qs, ws


_TABLES = {}


def _wake_tables():
    if not _TABLES:
        g = torch.Generator().manual_seed(5)
        _TABLES["wl"] = (1e14 * torch.rand(300, generator=g, dtype=F64)).float().double()
        _TABLES["wt"] = (1e19 * torch.rand(200, generator=g, dtype=F64)).float().double()
    return _TABLES["wl"], _TABLES["wt"]


def _make(kind, M, dtype=F64, cutoff=None):
    """A fresh element with settings float32 holds exactly; `cutoff`: None, a number, or a tensor."""
    import cheetah_amd as ca

    kw = {"dtype": dtype, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    c = {"num_bins": M, **kw}
    if cutoff is not None:
        c["cutoff_wavelength"] = cutoff if isinstance(cutoff, torch.Tensor) else torch.tensor(cutoff, dtype=F64, device="cuda")
    if kind == "wake":
        wl, wt = _wake_tables()
        return ca.Wakefield(t(0.75 * H), longitudinal_wake=wl.to(**kw), transverse_wake=wt.to(**kw), factor=t(1.5), **c)
    if kind == "csr":
        return ca.CSRKick(t(0.5), t(2.0 ** -4), **c)
    if kind == "csr_transient":
        return ca.TransientCSRKick(t(0.5), t(2.0 ** -4), t(0.25), **c)            # x = 10.7 nodes
    if kind == "csr_drift":
        return ca.CSRDriftKick(t(0.25), t(0.5), t(2.0 ** -6), t(0.125), **c)       # y = 8.5 nodes
    if kind == "lsc":
        return ca.LSCKick(t(2.0), t(2.0 ** -12), **c)
    if kind == "ibs":
        return ca.IBSKick(t(2.0), t(8.0), t(2.0 ** -13), t(2.0 ** -13), t(2.0 ** -30), t(2.0 ** -30), seed=7, stream=3, **c)
    raise KeyError(kind)


def _track(elem, x, q, w, dtype=F64):
    import cheetah_amd as ca

    kw = {"dtype": dtype, "device": "cuda"}
    beam = ca.ParticleBeam(x.to(**kw), torch.tensor(ENERGY, **kw), particle_charges=q.to(**kw), survival_probabilities=w.to(**kw))
    return elem.track(beam).particles


def _ulp(t, dtype):
    r = t.to(dtype).abs()
    return (torch.nextafter(r, torch.full_like(r, float("inf"))) - r).double()


def _assert_same_kick(kind, got, ref, x_in, rel, ulps, dtype=F64, label=""):
    """|got - ref| <= rel max|kick| + ulps ulp(dtype) of the coordinate in every moved column; the other columns bit-equal."""
    got, ref, x_in = got.cpu().double(), ref.cpu().double(), x_in.cpu().double().expand_as(ref.cpu())
    moved = MOVED.get(kind, (5,))
    for col in moved:
        kick = (ref - x_in)[..., col].abs().max()
        assert kick > 0, (kind, col)
        err = (got - ref)[..., col].abs()
        tol = rel * kick + ulps * _ulp(ref[..., col], dtype)
        print(f"{kind} {label} col {col}: max |difference| / max|kick| {float(err.max() / kick):.3e} (max|kick| {float(kick):.3e})")
        assert torch.all(err <= tol), (kind, col, float((err - tol).max()))
    rest = [c for c in range(7) if c not in moved]
    assert torch.equal(got[..., rest], x_in[..., rest])


def _rel_bound(kind):
    return 1e-7 if kind == "ibs" else 1e-9


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int64)


# ---- 1. the filtered kick is the unfiltered kick of the filtered deposit -------------------------------------------------------------
def _check_against_synthetic(kind, M, s, N=5000):
    x, q, w = _pinned_beam(N, M, seed=1000 * M + int(10 * s))
    cutoff = _cutoff(s)
    assert _s_of(cutoff, H) == pytest.approx(s, rel=1e-6)
    xs, qs, ws = _synthetic(x, q, w, M, [_s_of(cutoff, H)], transverse=kind == "wake")
    with torch.no_grad():
        got = _track(_make(kind, M, cutoff=cutoff), x, q, w[0])
        ref = _track(_make(kind, M), xs, qs[0], ws[0])[:N]
        raw = _track(_make(kind, M), x, q, w[0])
    _assert_same_kick(kind, got, ref, x, _rel_bound(kind), 1, label=f"M={M} s={s}")
    if M > 2:
        # the filter does something: the unfiltered kick of the original beam is far outside the bound
        col = MOVED.get(kind, (5,))[-1]
        assert float((raw - got)[:, col].abs().max()) > 1e-4 * float((got.cpu() - x)[:, col].abs().max())


@pytest.mark.parametrize("kind,M,s", CASES)
def test_filtered_kick_is_the_unfiltered_kick_of_the_filtered_deposit(kind, M, s):
    _check_against_synthetic(kind, M, s)


def test_largest_grid_needs_the_large_lds_request():
    """M = 4096, s = 20 (R = 80): the channel and the weights take more than 64 KiB of LDS."""
    _check_against_synthetic("lsc", 4096, 20.0)


@pytest.mark.parametrize("kind", [k for k in KICKS if k != "wake"])
def test_three_rows_one_cutoff_per_row_shared_particles_one_row_without_survivors(kind):
    N, M, s_rows = 5000, 129, [1.3, 17.3, 5.3]
    x, q, w = _pinned_beam(N, M, seed=77, rows=3, dead_row=1)
    cutoff = torch.tensor([_cutoff(s) for s in s_rows], dtype=F64, device="cuda")
    xs, qs, ws = _synthetic(x, q, w, M, [_s_of(float(c), H) for c in cutoff.cpu()])
    with torch.no_grad():
        got = _track(_make(kind, M, cutoff=cutoff), x, q, w)
        ref = _track(_make(kind, M), xs, qs, ws)[:, :N]
    assert got.shape == (3, N, 7)
    assert torch.equal(got[1].cpu(), x)                                         # no survivor: copied bit for bit
    live = [0, 2]
    _assert_same_kick(kind, got[live], ref[live], x, _rel_bound(kind), 1, label="rows 0, 2")
    assert not torch.equal(got[0], got[2])


# ---- 2. float32 beams against the same values as a float64 beam ---------------------------------------------------------------------
@pytest.mark.parametrize("M,s", SHORT_CASES)
@pytest.mark.parametrize("kind", KICKS)
def test_float32_beam_against_the_same_values_in_float64(kind, M, s):
    N = 5000
    x, q, w = _pinned_beam(N, M, seed=31 * M)
    cutoff = _cutoff(s)
    with torch.no_grad():
        got = _track(_make(kind, M, F32, cutoff), x, q, w[0], F32)
        ref = _track(_make(kind, M, F64, cutoff), x, q, w[0], F64)
    assert got.dtype == F32
    _assert_same_kick(kind, got, ref, x, 1e-6, 2, F32, label=f"float32 M={M} s={s}")


# ---- 3. identity weights, conservation, determinism ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("kind", KICKS)
def test_cutoff_far_below_the_node_spacing_is_the_unfiltered_kick_bit_for_bit(kind, dtype):
    """cutoff = 1e-3 h: g_1 = exp(-1 / 2 s^2) underflows to 0, so the weights are the identity."""
    N, M = 5000, 129
    x, q, w = _pinned_beam(N, M, seed=9)
    with torch.no_grad():
        got = _track(_make(kind, M, dtype, 1e-3 * H), x, q, w[0], dtype)
        ref = _track(_make(kind, M, dtype), x, q, w[0], dtype)
    assert float((ref.cpu().double() - x)[:, 5].abs().max()) > 0
    assert torch.equal(_bits(got), _bits(ref))


def _lsc_state(x, q, w, M, cutoff):
    """The state the LSC kick leaves (header, node sums, rho, a free slot, the M deposits), read through the ops layer."""
    import cheetah_amd as ca
    from cheetah_amd import _ops_grid1d as g1

    kw = {"dtype": F64, "device": "cuda"}
    sp = ca.Species("electron", dtype=F64)
    rows = tuple(torch.tensor([v], **kw) for v in (ENERGY, 2.0, 2.0 ** -12))
    cut = None if cutoff is None else torch.tensor([cutoff], **kw)
    X, Q, W = x.to(**kw)[None].contiguous(), q.to(**kw)[None].contiguous(), w.to(**kw)[None].contiguous()
    _, state = g1._kick_raw(g1._LSC, X, Q, W, *g1._settings_args(rows, sp.mass_eV_float, 1.0), 1, x.shape[0], M, cut)
    return state[0].cpu()


@pytest.mark.parametrize("s", [17.3, 40.0])
def test_the_filter_keeps_the_charge(s):
    N, M = 5000, 129
    x, q, w = _pinned_beam(N, M, seed=3)
    total = float((q.abs() * w[0]).sum())
    raw, flt = (_lsc_state(x, q, w[0], M, c)[8 + M + 2:8 + 2 * M + 2] for c in (None, _cutoff(s)))
    assert raw.shape == (M,) and not torch.equal(raw, flt)
    print(f"s={s}: sum D / sum c - 1 = {float(raw.sum()) / total - 1:.3e}, sum D' / sum c - 1 = {float(flt.sum()) / total - 1:.3e}")
    assert abs(float(raw.sum()) / total - 1) <= 1e-12
    assert abs(float(flt.sum()) / total - 1) <= 1e-12
    assert float(flt.min()) >= 0.0
    # and D' is the test's own filter of the stored unfiltered deposit
    mine = torch.from_numpy(_smooth(raw.numpy(), _s_of(_cutoff(s), H)))
    assert float((flt - mine).abs().max()) <= 1e-12 * float(raw.max())


@pytest.mark.parametrize("kind", KICKS)
def test_two_identical_calls_are_bit_equal(kind):
    N, M = 5000, 129
    x, q, w = _pinned_beam(N, M, seed=21)
    import cheetah_amd as ca

    outs = []
    for _ in range(2):
        xx = x.to("cuda").requires_grad_()
        qq = q.to("cuda").requires_grad_()
        beam = ca.ParticleBeam(xx, torch.tensor(ENERGY, dtype=F64, device="cuda"), particle_charges=qq,
                               survival_probabilities=w[0].to("cuda"))
        out = _make(kind, M, cutoff=_cutoff(17.3)).track(beam).particles
        out[:, [1, 3, 5]].square().sum().backward()
        outs.append((out.detach(), xx.grad, qq.grad))
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b))
    assert float(outs[0][2].abs().max()) > 0


# ---- 4. no host synchronisation, in-place edits, graph capture ---------------------------------------------------------------------------
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


@pytest.mark.parametrize("kind", ["lsc", "wake"])
def test_no_host_synchronisation(kind):
    import cheetah_amd as ca

    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, device="cuda", dtype=F32)
    assert len(_sync_warnings(lambda: float(beam.sigma_x), warm=0)) == 1          # the switch sees what it should see
    elem = _make(kind, 500, F32, torch.tensor(3e-6, dtype=F32, device="cuda"))
    x = beam.particles.detach().clone().requires_grad_()
    gb = ca.ParticleBeam(x, beam.energy)

    def fwd_bwd():
        x.grad = None
        elem.track(gb).particles[:, 5].sum().backward()

    with torch.no_grad():
        assert _sync_warnings(lambda: elem.track(beam).particles) == []
    assert _sync_warnings(fwd_bwd) == []


@pytest.mark.parametrize("dtype", [F64, F32])
def test_an_in_place_edit_of_the_cutoff_is_followed(dtype):
    N, M = 5000, 129
    x, q, w = _pinned_beam(N, M, seed=41)
    elem = _make("csr", M, dtype, torch.tensor(_cutoff(1.3), dtype=dtype, device="cuda"))
    with torch.no_grad():
        first = _track(elem, x, q, w[0], dtype)
        elem.cutoff_wavelength.fill_(_cutoff(17.3))
        second = _track(elem, x, q, w[0], dtype)
        fresh = _track(_make("csr", M, dtype, torch.tensor(_cutoff(17.3), dtype=dtype, device="cuda")), x, q, w[0], dtype)
    assert torch.equal(_bits(second), _bits(fresh)) and not torch.equal(second, first)


def test_captured_track_follows_an_edit_of_the_cutoff():
    import cheetah_amd as ca

    kw = {"dtype": F32, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(0)
    beam = ca.ParticleBeam.from_parameters(num_particles=50_000, sigma_x=t(2e-4), sigma_tau=t(5e-5), total_charge=t(1e-9), **kw)
    lsc = ca.LSCKick(t(1.0), t(3e-4), num_bins=300, cutoff_wavelength=t(4e-6), **kw)
    seg = ca.Segment([ca.Drift(t(0.5), **kw), lsc, ca.Quadrupole(t(0.2), k1=t(3.0), **kw)])

    def step():
        return (seg.track(beam).particles,)

    with torch.no_grad():
        for _ in range(3):
            step()
        captured = ca.graph.capture(step)
        first = captured()[0].clone()
        assert torch.equal(first, step()[0])
        lsc.cutoff_wavelength.copy_(t(2e-5))
        second = captured()[0].clone()
        assert torch.equal(second, step()[0])
    assert not torch.equal(second, first)


# ---- 5. gradients ------------------------------------------------------------------------------------------------------------------------
def _gradcheck_case(kind):
    """(fn, leaves): N = 40 particles, M = 8 nodes, s = 1.3; tau a constant. Charges of order one (finite differences of step 1e-6
    stay linear) and settings that make the kick of order 0.1, as the kicks' own gradchecks."""
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    g = torch.Generator().manual_seed(11)
    N, M = 40, 8
    base = torch.randn(N, 7, generator=g, dtype=F64)
    base[:, 4] *= 1e-6 if kind == "ibs" else 1e-3
    base[:, 6] = 1.0
    h = float(base[:, 4].max() - base[:, 4].min()) / (M - 1)
    cutoff = torch.tensor(_cutoff(1.3, h), **kw)
    base = base.to(**kw)
    leaf = lambda v: (v if isinstance(v, torch.Tensor) else torch.tensor(v, dtype=F64)).to(**kw).requires_grad_()  # noqa: E731
    xc, yc, dc = (leaf(base[:, i].clone()) for i in (0, 2, 5))
    q = leaf(0.5 + torch.rand(N, generator=g, dtype=F64))
    w = leaf(0.2 + 0.8 * torch.rand(N, generator=g, dtype=F64))
    c = {"num_bins": M, "cutoff_wavelength": cutoff, **kw}
    if kind == "wake":
        settings = [leaf(2e6), leaf(1.5), leaf(1e5 * torch.rand(12, generator=g, dtype=F64)), leaf(1e6 * torch.rand(10, generator=g, dtype=F64))]
        build = lambda factor, wl, wt: ca.Wakefield(torch.tensor(1.5e-4, **kw), longitudinal_wake=wl, transverse_wake=wt,  # noqa: E731
                                                    factor=factor, **c)
    elif kind == "csr":
        settings = [leaf(1e15), leaf(0.5), leaf(-0.2)]
        build = lambda L, th: ca.CSRKick(L, th, **c)  # noqa: E731
    elif kind == "csr_transient":
        # x = 1.3 nodes, 4x = 5.2: a step of 1e-6 crosses no node
        d = (1.3 * h * 24 * 0.5 ** 2 / 0.2 ** 2) ** (1 / 3)
        settings = [leaf(1e15), leaf(0.5), leaf(-0.2), leaf(d)]
        build = lambda L, th, d: ca.TransientCSRKick(L, th, d, **c)  # noqa: E731
    elif kind == "csr_drift":
        settings = [leaf(1e15), leaf(0.5), leaf(0.5), leaf(0.2), leaf(0.25)]
        build = lambda L, Lb, th, d: ca.CSRDriftKick(L, Lb, th, d, **c)  # noqa: E731
    elif kind == "lsc":
        settings = [leaf(5e9), leaf(0.5), leaf(4.0)]
        build = lambda L, a: ca.LSCKick(L, a, **c)  # noqa: E731
    else:
        settings = [leaf(1e6), leaf(0.5), leaf(10.0), leaf(0.1), leaf(0.12), leaf(0.11), leaf(0.09)]
        build = lambda L, lam, sx, sy, ex, ey: ca.IBSKick(L, lam, sx, sy, ex, ey, seed=5, stream=1, **c)  # noqa: E731

    def fn(xc, yc, dc, q, w, energy, *rest):
        cols = list(base.unbind(-1))
        cols[0], cols[2], cols[5] = xc, yc, dc
        beam = ca.ParticleBeam(torch.stack(cols, dim=-1), energy, particle_charges=q, survival_probabilities=w)
        return build(*rest).track(beam).particles

    return fn, (xc, yc, dc, q, w, *settings)


@pytest.mark.parametrize("kind", KICKS)
def test_gradcheck_with_a_cutoff(kind):
    fn, leaves = _gradcheck_case(kind)
    with torch.no_grad():
        moved = (fn(*leaves)[:, 5] - leaves[2]).abs().max()
    print(f"{kind}: max |kick| {float(moved):.3e}")
    assert 1e-3 < float(moved) < 10
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-8, rtol=1e-6)


K_E = 8.9875517923e9


def _lsc_reference_row(x, q, w, energy, L, radius, M, s, mass):
    """`_reference_row` of test_gpu_lsc.py with the filter between the deposit and the node sums: one batch row, float64 on the CPU,
    the grid (and with it the filter's matrix) detached."""
    alive, lo, h, k, f = _grid(x[:, 4], w, M)
    c = torch.where(alive, q.abs() * w, torch.zeros_like(w))
    D = _smoothing_matrix(s, M) @ _deposit(k, torch.where(alive, f, torch.zeros_like(f)), c, M)
    gamma = energy / mass
    rho = radius / (gamma * h)
    j = torch.arange(-1, M + 1, dtype=F64)
    p = j / (j.abs() + torch.sqrt(j * j + rho * rho)) + torch.asinh(j / rho)
    ch = -0.5 * (p[2:] - 2 * p[1:-1] + p[:-2])
    full = torch.cat([-ch[1:].flip(0), ch])
    V = (full.unfold(0, M, 1) @ D).flip(0)
    beta = (1 - gamma.square().reciprocal()).sqrt()
    S = 2 * K_E * L / (gamma.square() * h.square() * beta * gamma * mass)
    node = S * V
    cols = list(x.unbind(-1))
    cols[5] = cols[5] + (1 - f) * node[k] + f * node[k + 1]
    return torch.stack(cols, dim=-1)


def test_tau_gradient_through_the_filtered_cotangents():
    """The gradient with respect to tau of every particle, N = 5000, M = 129, s = 17.3 (R = 70), against autograd through the
    restatement; bound 1e-9 max|reference gradient| as tests/test_gpu_binned_kick_grads.py, every reference gradient non-zero."""
    import cheetah_amd as ca

    N, M, s = 5000, 129, 17.3
    x, q, w = _pinned_beam(N, M, seed=55)
    g = torch.Generator().manual_seed(56)
    cot = torch.randn(N, 7, generator=g, dtype=F64)
    xx = x.to("cuda").requires_grad_()
    beam = ca.ParticleBeam(xx, torch.tensor(ENERGY, dtype=F64, device="cuda"), particle_charges=q.to("cuda"),
                           survival_probabilities=w[0].to("cuda"))
    _make("lsc", M, cutoff=_cutoff(s)).track(beam).particles.backward(cot.to("cuda"))
    xr = x.clone().requires_grad_()
    mass = ca.Species("electron", dtype=F64).mass_eV_float
    _lsc_reference_row(xr, q, w[0], torch.tensor(ENERGY, dtype=F64), torch.tensor(2.0, dtype=F64), torch.tensor(2.0 ** -12, dtype=F64),
                       M, _s_of(_cutoff(s), H), mass).backward(cot)
    got, ref = xx.grad.cpu()[:, 4], xr.grad[:, 4]
    through = ref - cot[:, 4]                              # what the kick adds to the cotangent that passes through
    inside = (x[:, 4] > -(M - 1) / 2 * H) & (x[:, 4] < (M - 1) / 2 * H)
    assert bool((through[inside] != 0).all()) and bool((ref != 0).all())
    scale = float(ref.abs().max())
    print(f"tau gradient: max |difference| / max |reference| {float((got - ref).abs().max()) / scale:.3e}, "
          f"max |the kick's part| / max |reference| {float(through.abs().max()) / scale:.3e}")
    assert float((got - ref).abs().max()) <= 1e-9 * scale


# ---- 6. convergence in num_bins: the point of the feature -----------------------------------------------------------------------------------
def test_the_filtered_kick_converges_as_num_bins_grows():
    """LSCKick on a drawn Gaussian beam (N = 20 000, sigma_tau = 1e-4 m, radius 2e-4 m, 1e8 eV, float64), cutoff = 8 node spacings of
    the M = 128 grid: rms(kick at M = 1024 - kick at M = 128) with the filter is at most 0.1 of the same difference without. The
    float64 restatement of this file gives 0.019 ... 0.023 for this generator's seeds 0, 1, 2 (seed 0 is used), so 0.1 is a condition
    with a 4x margin, not a measurement."""
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    N = 20_000
    g = torch.Generator().manual_seed(0)
    x = torch.zeros(N, 7, dtype=F64)
    x[:, 4] = 1e-4 * torch.randn(N, generator=g, dtype=F64)
    x[:, 6] = 1.0
    q = torch.full((N,), 1e-9 / N, dtype=F64)
    beam = ca.ParticleBeam(x.to(**kw), torch.tensor(ENERGY, **kw), particle_charges=q.to(**kw))
    h128 = float(x[:, 4].max() - x[:, 4].min()) / 127
    rms = {}
    with torch.no_grad():
        for cutoff in (None, 8 * h128):
            c = {} if cutoff is None else {"cutoff_wavelength": torch.tensor(cutoff, **kw)}
            kicks = [ca.LSCKick(torch.tensor(2.0, **kw), torch.tensor(2e-4, **kw), num_bins=M, **c, **kw).track(beam).particles[:, 5]
                     for M in (128, 1024)]
            rms[cutoff is None] = float((kicks[1] - kicks[0]).square().mean().sqrt())
    print(f"rms(kick M=1024 - kick M=128): unfiltered {rms[True]:.4e}, filtered {rms[False]:.4e}, ratio {rms[False] / rms[True]:.4f}")
    assert rms[True] > 0
    assert rms[False] <= 0.1 * rms[True]
