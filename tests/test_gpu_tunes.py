"""TurnByTurn.tunes on the GPU against its definition (include/chx.h) restated here in float64 numpy: the Hann-windowed,
mean-removed signal, the coarse grid nu_k = k / (2 P), the lowest k with the largest A, the bracket rule, the root of g by a plain
bisection of 60 steps, the amplitude 2 |F| / sum w.

Tolerances: |tune - reference| <= 2^-44 (the kernel ends its search at 2^-48; 16x for the order of its sums) and
|amplitude - reference| <= T 2^-50 amplitude. The reference itself is checked against a long-double twin: <= 2^-50.
Every test here fails without the feature: `_ops.tunes` and `TurnByTurn.tunes` do not exist."""
import functools
import itertools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_NU = 2.0 ** -44
PLANE_SETS = [c for r in (1, 2, 3) for c in itertools.combinations(("x", "y", "tau"), r)]
COLUMN = {"x": 0, "y": 2, "tau": 4}
BIT = {"x": 1, "y": 2, "tau": 4}


def grid_log2(T):
    return int(np.ceil(np.log2(T))) + 1


def spectral(v, nu, dtype=np.float64):
    """F, G of the definition for the signals v (M, T) at one frequency each, nu (M,): the phase nu n reduced in turns."""
    n = np.arange(v.shape[1]).astype(dtype)
    pi = dtype(4) * np.arctan(dtype(1))
    t = nu[:, None] * n
    t = t - np.floor(t)
    c, s = np.cos(2 * pi * t), np.sin(2 * pi * t)
    return (v * c).sum(1) - 1j * (v * s).sum(1), (n * v * c).sum(1) - 1j * (n * v * s).sum(1)


def slope(F, G):
    return F.real * G.imag - F.imag * G.real


def reference(u, dtype=np.float64, guard=True):
    """(tune, amplitude, k*) of the signals u (M, T) float64 by the definition, all arithmetic in `dtype`. The argmax over the grid
    comes from a float64 FFT and is settled among k - 2 .. k + 2 with the definition's own sums (the phases reduced in turns), so
    that the FFT's rounding decides nothing. `guard`: assert that the runner-up outside k* +- 2 is below 0.9 of the maximum."""
    M, T = u.shape
    bad = ~np.isfinite(u).all(1)
    u = np.where(bad[:, None], 0.0, u).astype(dtype)
    pi = dtype(4) * np.arctan(dtype(1))
    w = np.sin(pi * (np.arange(T).astype(dtype) + dtype(0.5)) / dtype(T)) ** 2
    sw = w.sum()
    v = w * (u - ((w * u).sum(1) / sw)[:, None])
    P = 2 ** grid_log2(T)
    A = np.abs(np.fft.fft(v.astype(np.float64), n=2 * P, axis=1)[:, :P + 1]) ** 2
    k0 = A.argmax(1)
    cand = k0[:, None] + np.arange(-2, 3)
    valid = (cand >= 0) & (cand <= P)
    Ad = np.stack([np.abs(spectral(v, np.clip(cand[:, d], 0, P).astype(dtype) / dtype(2 * P), dtype)[0]) ** 2 for d in range(5)], 1)
    Ad = np.where(valid, Ad, -1.0)
    ks = cand[np.arange(M), Ad.argmax(1)]                       # (argmax: the first, that is the lowest k, of equal values)
    zero = Ad.max(1) == 0
    if guard:
        far = np.abs(np.arange(P + 1)[None, :] - ks[:, None]) > 2
        runner_up = np.where(far, A, 0.0).max(1)
        assert (runner_up[~zero & ~bad] < 0.9 * A[np.arange(M), ks][~zero & ~bad]).all(), "the test's signals tie on the coarse grid"
    step = dtype(1) / dtype(2 * P)
    lo, hi = np.clip(ks - 1, 0, P).astype(dtype) * step, np.clip(ks + 1, 0, P).astype(dtype) * step
    refine = (ks > 0) & (ks < P) & (slope(*spectral(v, lo, dtype)) > 0) & (slope(*spectral(v, hi, dtype)) < 0)
    for _ in range(60):
        mid = (lo + hi) / 2
        up = slope(*spectral(v, mid, dtype)) > 0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    nu = np.where(refine, (lo + hi) / 2, ks.astype(dtype) * step)
    amp = 2 * np.abs(spectral(v, nu, dtype)[0]) / sw
    nu, amp = np.where(zero, np.nan, nu), np.where(zero, 0.0, amp)
    return np.where(bad, np.nan, nu), np.where(bad, np.nan, amp), ks


def two_lines(T, R, S, seed, dt):
    """(R, S, 7) records of `dt`: in columns 0, 2, 4 a line of amplitude 1e-3 at nu in [0.05, 0.45], a second one of at most a fifth
    of it, and an offset; NaN in columns 1 and 3 (never read), 1 in column 6. Below T = 64 the strong line stays in [0.15, 0.35]:
    the main lobe of a window that short is 4 / T wide, and closer to 0 or 1/2 the line's mirror image at -nu flattens the peak
    until the grid's values tie (measured on the reference at T = 8, 9, 16: up to 0.99 of the maximum over [0.05, 0.45], at most
    0.87 over [0.15, 0.35]) — the guard of `reference` would refuse those signals."""
    rng = np.random.default_rng(seed)
    n = np.arange(R)[:, None, None]
    nu1, nu2 = rng.uniform(0.05, 0.45, (2, 1, S, 3))
    if T < 64:
        nu1 = 0.15 + (nu1 - 0.05) / 2
    a2 = rng.uniform(0.0, 2e-4, (1, S, 3))
    ph1, ph2 = rng.uniform(0, 2 * np.pi, (2, 1, S, 3))
    off = rng.uniform(-1e-2, 1e-2, (1, S, 3))
    sig = off + 1e-3 * np.cos(2 * np.pi * nu1 * n + ph1) + a2 * np.cos(2 * np.pi * nu2 * n + ph2)
    x = np.full((R, S, 7), np.nan)
    x[:, :, [0, 2, 4]] = sig
    x[:, :, 5] = rng.uniform(-1e-3, 1e-3, (R, S))
    x[:, :, 6] = 1.0
    return torch.tensor(x, dtype=dt)


@functools.lru_cache(maxsize=None)
def case(T, dt):
    """The records of one (T, dtype) and their reference per first record r0: {r0: (tune (65, 3), amplitude (65, 3))}."""
    S, R = 65, T + 6
    x = two_lines(T, R, S, 1000 + T, dt)
    ref = {}
    for r0 in (0, 5):
        u = x[r0:r0 + T, :, [0, 2, 4]].to(torch.float64).numpy().transpose(1, 2, 0).reshape(S * 3, T)
        nu, amp, _ = reference(u)
        ref[r0] = (nu.reshape(S, 3), amp.reshape(S, 3))
    return x, ref


def run(x, lost, r0, T, last_turn, planes):
    import cheetah_amd._ops as ops

    nu, amp = ops.tunes(x, lost, r0, T, last_turn, sum(BIT[p] for p in planes))
    return nu.cpu().numpy(), amp.cpu().numpy()


def close(nu, amp, nu_ref, amp_ref, T):
    assert np.array_equal(np.isnan(nu), np.isnan(nu_ref)) and np.array_equal(np.isnan(amp), np.isnan(amp_ref))
    ok = ~np.isnan(nu_ref)
    err = np.abs(nu - nu_ref)[ok].max() if ok.any() else 0.0
    assert err <= TOL_NU, err
    ok = ~np.isnan(amp_ref)
    assert (np.abs(amp - amp_ref)[ok] <= T * 2.0 ** -50 * amp_ref[ok]).all(), np.abs(amp / amp_ref - 1)[ok].max()
    return err


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("T", [8, 9, 64, 100, 257, 1024, 4096])
def test_synthetic_signals_against_the_definition(T, dt):
    x, ref = case(T, dt)
    worst = 0.0
    for S in (1, 3, 65):
        xs = x[:, :S].contiguous().cuda()
        for r0 in (0, 5):
            assert xs.shape[0] > r0 + T
            for planes in PLANE_SETS:
                nu, amp = run(xs, None, r0, T, r0 + T, planes)
                cols = [("x", "y", "tau").index(p) for p in planes]
                assert nu.shape == amp.shape == (S, len(planes))
                worst = max(worst, close(nu, amp, ref[r0][0][:S, cols], ref[r0][1][:S, cols], T))
    print(f"T = {T} {dt}: largest |tune - reference| = {worst:.3e} (bound {TOL_NU:.3e})")


@pytest.mark.parametrize("T", [64, 100, 257, 1024])
def test_the_reference_against_its_long_double_twin(T):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is float64 here")
    x, _ = case(T, torch.float64)
    u = x[:T, :8, [0, 2, 4]].numpy().transpose(1, 2, 0).reshape(24, T)
    nu, amp, ks = reference(u)
    nu_l, amp_l, ks_l = reference(u, np.longdouble, guard=False)
    assert np.array_equal(ks, ks_l)
    err = np.abs(nu - nu_l).max()
    print(f"T = {T}: reference against long double {float(err):.3e}")
    assert err <= 2.0 ** -50
    assert (np.abs(amp - amp_l) <= T * 2.0 ** -52 * amp_l).all()          # T products and additions of 2^-53 each, at the worst


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("T", [64, 256, 1024])
def test_a_pure_sinusoid_against_the_truth(T, dt):
    rng = np.random.default_rng(T)
    S = 32
    nu_true = rng.uniform(0.1, 0.4, S)
    n = np.arange(T)[:, None]
    x = np.zeros((T, S, 7))
    x[:, :, 0] = 1e-3 * np.cos(2 * np.pi * nu_true * n + rng.uniform(0, 2 * np.pi, S))
    x[:, :, 2] = 2e-3 * np.sin(2 * np.pi * nu_true[::-1] * n + rng.uniform(0, 2 * np.pi, S))
    nu, amp = run(torch.tensor(x, dtype=dt).cuda(), None, 0, T, T, ("x", "y"))
    err = max(np.abs(nu[:, 0] - nu_true).max(), np.abs(nu[:, 1] - nu_true[::-1]).max())
    print(f"T = {T} {dt}: |tune - truth| = {err * T ** 3:.3f} T^-3")
    assert err <= 4.0 / T ** 3
    assert np.abs(amp[:, 0] / 1e-3 - 1).max() < 1e-3 and np.abs(amp[:, 1] / 2e-3 - 1).max() < 1e-3


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_edges(dt):
    T, S = 64, 6
    n = np.arange(T + 1)
    x = np.zeros((T + 1, S, 7))
    x[:, :, 0] = 1e-3 * np.cos(2 * np.pi * 0.21 * n)[:, None]
    x[:, :, 2] = 2e-3 * np.cos(2 * np.pi * 0.33 * n)[:, None]
    x[:, 0, 0] = (-1.0) ** n                                    # the alternating signal: exactly 1/2
    x[:, 1, 0] = 0.25                                           # a constant: NaN, 0
    x[:, 1, 2] = 0.0
    x[17, 2, 2] = np.nan                                        # one NaN sample: that row and plane only
    x[T, 3, 0] = np.inf                                         # behind the window: not read
    xt = torch.tensor(x, dtype=dt).cuda()
    lost = torch.tensor([0, 0, 0, 0, T, T + 1], dtype=torch.int32).cuda()      # the window's last turn, and one turn later
    nu, amp = run(xt, lost, 0, T, T, ("x", "y"))
    nu_ref, amp_ref, _ = reference(xt[:T, :, [0, 2]].double().cpu().numpy().transpose(1, 2, 0).reshape(2 * S, T), guard=False)
    nu_ref, amp_ref = nu_ref.reshape(S, 2), amp_ref.reshape(S, 2)
    assert nu[0, 0] == 0.5 and abs(amp[0, 0] - 2.0) < 1e-9      # (at 1/2 the line and its mirror image coincide: 2 |F| counts both)
    assert np.isnan(nu[1]).all() and (amp[1] == 0).all()
    assert np.isnan(nu[2, 1]) and np.isnan(amp[2, 1]) and abs(nu[2, 0] - 0.21) < 1e-4
    assert abs(nu[3, 0] - 0.21) < 1e-4 and abs(nu[3, 1] - 0.33) < 1e-4
    assert np.isnan(nu[4]).all() and np.isnan(amp[4]).all()
    assert not np.isnan(nu[5]).any()
    nu_ref[4], amp_ref[4] = np.nan, np.nan
    nu_ref[1], amp_ref[1] = np.nan, 0.0                         # (asserted above; the reference's own mean need not be exact)
    close(nu, amp, nu_ref, amp_ref, T)
    again = run(xt, lost, 0, T, T, ("x", "y"))                  # the same bits in every call
    assert np.array_equal(nu, again[0], equal_nan=True) and np.array_equal(amp, again[1], equal_nan=True)
    assert np.array_equal(nu.view(np.int64), again[0].view(np.int64)) and np.array_equal(amp.view(np.int64), again[1].view(np.int64))
    nu1, _ = run(xt, lost, 1, T, T + 1, ("x",))                 # the window one record on: the row lost on turn T + 1 is gone too
    assert np.isnan(nu1[4:]).all() and np.isnan(nu1[3, 0]) and nu1[0, 0] == 0.5


def sextupole_ring(dt):
    import cheetah_amd as ca

    kw = {"dtype": dt, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    dkd = {"tracking_method": "drift_kick_drift"}
    cell = lambda: [ca.Quadrupole(t(0.2), k1=t(2.0), **dkd, **kw), ca.Sextupole(t(0.1), k2=t(40.0), num_steps=2, **dkd, **kw),  # noqa: E731
                    ca.Drift(t(0.5), **dkd, **kw), ca.Quadrupole(t(0.2), k1=t(-2.0), **dkd, **kw), ca.Drift(t(0.9), **dkd, **kw)]
    return ca.Segment([e for _ in range(4) for e in cell()])


def ring_particles(dt, lead=()):
    """20 particles on amplitudes up to 2 mm; particle 5 starts far beyond the aperture of 20 mm."""
    rng = np.random.default_rng(3)
    x = np.zeros((*lead, 20, 7))
    x[..., 0] = rng.uniform(1e-4, 2e-3, (*lead, 20))
    x[..., 2] = rng.uniform(1e-4, 2e-3, (*lead, 20))
    x[..., 5] = rng.uniform(-1e-3, 1e-3, (*lead, 20))
    x[..., 5, 0] = 0.5
    x[..., 6] = 1.0
    return torch.tensor(x, dtype=dt, device="cuda")


@pytest.mark.parametrize("dt,lead,fused", [(torch.float64, (), True), (torch.float32, (2,), False)], ids=["f64-fused", "f32-general"])
def test_through_track_turns(dt, lead, fused):
    import cheetah_amd as ca

    beam = ca.ParticleBeam(ring_particles(dt, lead), torch.tensor(1e8, dtype=dt, device="cuda"))
    tbt = sextupole_ring(dt).track_turns(beam, 128, aperture=torch.tensor([2e-2, 2e-2], dtype=dt, device="cuda"), record_first=16,
                                         fused=fused)
    assert tbt.particles.shape == (128, *lead, 16, 7)
    lost = tbt.lost_turn[..., :16].cpu().numpy()
    print("particle 5 lost on turn", lost[..., 5])
    assert (lost[..., 5] > 0).all() and (lost[..., 5] <= 64).all() and (np.delete(lost, 5, axis=-1) == 0).all()
    rows = tbt.particles.to(torch.float64).cpu().numpy()
    planes = ("y", "tau", "x")                                  # not in column order: the results follow the request
    cols = [COLUMN[p] for p in planes]
    for r0, T in ((0, 128), (0, 64), (64, 64), (3, 100)):
        got = tbt.tunes(planes, r0, T)
        assert got.tune.shape == got.amplitude.shape == (*lead, 16, 3) and got.tune.dtype == torch.float64
        u = np.moveaxis(rows[r0:r0 + T][..., cols], 0, -1).reshape(-1, T)              # (..., 16, 3, T)
        nu_ref, amp_ref, _ = reference(u, guard=False)
        nu_ref, amp_ref = nu_ref.reshape(*lead, 16, 3).copy(), amp_ref.reshape(*lead, 16, 3).copy()
        gone = (lost > 0) & (lost <= r0 + T)                    # lost up to the window's last record (every turn is recorded)
        nu_ref[gone], amp_ref[gone] = np.nan, np.nan
        close(got.tune.cpu().numpy(), got.amplitude.cpu().numpy(), nu_ref, amp_ref, T)
    assert tbt.tunes(first_record=120).tune.shape == (*lead, 16, 2)                   # the last 8 records
    x_tune = tbt.tunes("x").tune.cpu().numpy()
    assert np.isnan(x_tune[..., 5, 0]).all() and ((np.delete(x_tune, 5, axis=-2) > 0.05) & (np.delete(x_tune, 5, axis=-2) < 0.45)).all()

    first, second, d = tbt.tune_diffusion()
    a, b = tbt.tunes(("x", "y"), 0, 64), tbt.tunes(("x", "y"), 64, 64)
    same = lambda p, q: torch.equal(p.view(torch.int64), q.view(torch.int64))  # noqa: E731
    assert same(first.tune, a.tune) and same(first.amplitude, a.amplitude) and same(second.tune, b.tune) and same(second.amplitude, b.amplitude)
    want = torch.log10(torch.sqrt(((b.tune - a.tune) ** 2).sum(-1)))
    assert d.shape == (*lead, 16) and same(d, want)
    assert torch.isnan(d[..., 5]).all() and (d[..., :5] < -2).all()       # regular orbits: the halves agree to 1e-2 at the very least


def test_tune_diffusion_is_minus_infinity_where_the_halves_agree():
    import cheetah_amd as ca
    from cheetah_amd.particles.turns import NUM_SUMS

    n = np.arange(32)
    x = np.zeros((32, 2, 7))
    x[:, 0, 0] = np.tile(np.cos(2 * np.pi * 0.25 * np.arange(16)), 2)       # the two halves hold the same samples
    x[:, 0, 2] = np.tile(np.sin(2 * np.pi * 0.125 * np.arange(16)), 2)
    x[:, 1, 0] = np.cos(2 * np.pi * 0.2 * n)
    x[:, 1, 2] = np.cos(2 * np.pi * (0.2 + 0.002 * n) * n)                  # a drifting line
    tbt = ca.TurnByTurn(None, torch.zeros(2, dtype=torch.int32, device="cuda"), torch.arange(1, 33, device="cuda"),
                        torch.zeros(32, NUM_SUMS, dtype=torch.float64, device="cuda"), torch.tensor(x, device="cuda"), record_every=1)
    d = tbt.tune_diffusion().d.cpu().numpy()
    assert d[0] == -np.inf and np.isfinite(d[1]) and d[1] > -3


def test_a_linear_ring_against_the_matrix_tune():
    import cheetah_amd as ca

    dt, k1, lq, ld, T = torch.float64, 4.0, 0.2, 0.8, 256
    kw = {"dtype": dt, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    ring = ca.Segment([ca.Quadrupole(t(lq), k1=t(k1), **kw), ca.Drift(t(ld), **kw), ca.Quadrupole(t(lq), k1=t(-k1), **kw), ca.Drift(t(ld), **kw)])

    def quad(k):                                                # the thick-lens 2 x 2 matrix of one plane
        if k > 0:
            r, phi = np.sqrt(k), np.sqrt(k) * lq
            return np.array([[np.cos(phi), np.sin(phi) / r], [-r * np.sin(phi), np.cos(phi)]])
        r, phi = np.sqrt(-k), np.sqrt(-k) * lq
        return np.array([[np.cosh(phi), np.sinh(phi) / r], [r * np.sinh(phi), np.cosh(phi)]])

    drift = np.array([[1.0, ld], [0.0, 1.0]])
    want = []
    for sign in (1.0, -1.0):                                    # x sees k1, y sees -k1
        M = drift @ quad(-sign * k1) @ drift @ quad(sign * k1)
        q = np.arccos(np.trace(M) / 2) / (2 * np.pi)
        want.append(min(q, 1 - q))
    assert all(0.1 <= q <= 0.4 for q in want), want
    x = np.zeros((8, 7))
    ang = 2 * np.pi * np.arange(8) / 8
    x[:, 0], x[:, 2], x[:, 6] = 1e-5, 1e-5, 1.0                 # 10 um, delta = 0, on eight phases
    x[:, 1], x[:, 3] = 2e-6 * np.sin(ang), 2e-6 * np.cos(ang)
    beam = ca.ParticleBeam(torch.tensor(x, **kw), t(1e8))
    tbt = ring.track_turns(beam, T, record_first=8)
    got = tbt.tunes().tune.cpu().numpy()
    err = np.abs(got - np.array(want)).max()
    print(f"matrix tunes {want}, |tune - matrix| = {err * T ** 3:.3f} T^-3")
    assert err <= 4.0 / T ** 3


def test_tunes_do_not_synchronise():
    """Like tests/test_gpu_track_turns_no_sync.py: torch.cuda.set_sync_debug_mode("warn"), calibrated on a call that does."""
    def sync_warnings(fn, warm=2):
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

    import cheetah_amd as ca

    dt = torch.float32
    beam = ca.ParticleBeam(ring_particles(dt), torch.tensor(1e8, dtype=dt, device="cuda"))
    ring = sextupole_ring(dt)
    assert len(sync_warnings(lambda: torch.tensor(1.0, device="cuda"), warm=0)) == 1       # the switch sees what it should see
    flows = {
        "tunes": lambda: ring.track_turns(beam, 64, record_every=2, record_first=16).tunes(("tau", "x", "y")),
        "window": lambda: ring.track_turns(beam, 64, record_first=16).tunes("y", 8, 32),
        "diffusion": lambda: ring.track_turns(beam, 64, record_first=16).tune_diffusion(),
    }
    for name, fn in flows.items():
        hits = sync_warnings(fn)
        assert not hits, (name, [(w.filename, w.lineno) for w in hits])
