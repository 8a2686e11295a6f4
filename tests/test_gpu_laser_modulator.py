"""The LaserModulator element on the GPU: the kick against a float64 torch restatement of its formulas (the phase reduced in turns
exactly as the kernel reduces it), the switches (a row of amplitude 0, non-finite coordinates), gradients against autograd through
the restatement, two physics checks (the bunching a chicane makes of the modulation, the energy spread a laser heater leaves), a
lattice with `Undulator.with_laser` and graph capture. One process, no workers.

Every floating-point bound is 4x the deviation measured on an MI355X, which stands in the comment next to it;
the statistical bound is four standard errors. Deviations are per column: max |got - ref| over max |ref|."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
ENERGY = 135e6                                 # eV: a laser heater's beam
WAVELENGTH = 8e-7                              # m
TWO_PI = 2 * math.pi
PASS_THROUGH = (0, 1, 2, 3, 4, 6)
SETTINGS = ("amplitude", "wavelength", "phase", "laser_sigma", "offset_x", "offset_y", "pulse_sigma", "pulse_center")


@functools.lru_cache(maxsize=None)
def _mass(dtype=F64):
    """The electron mass in eV as a beam of this dtype hands it to the kernels."""
    import cheetah_amd as ca

    return ca.Species("electron", dtype=dtype).mass_eV_float


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _restate(particles, energy, s, mass):
    """The formulas in float64 torch: particles (*, N, 7), energy and the settings `s` (a dict; pulse_sigma may be None) of batch
    shapes, every one taken in the dtype the kernel reads it in (the particles') -> (*batch, N, 7). The phase is reduced in turns:
    t = fl(fl(tau nu) + phi_t), f = t - rint(t) (torch rounds the product and the sum separately, and `round` is to even)."""
    dt = particles.dtype
    f64 = lambda v: v.to(dt).to(F64)  # noqa: E731
    gamma = f64(energy) / mass
    P0 = (1 - gamma.square().reciprocal()).clamp_min(0).sqrt() * gamma
    a = f64(s["amplitude"]) / (P0 * mass)
    nu = 1 / f64(s["wavelength"])
    phit = f64(s["phase"]) / TWO_PI
    g = 1 / (4 * f64(s["laser_sigma"]).square())
    h = torch.zeros((), dtype=F64, device=a.device) if s["pulse_sigma"] is None else 1 / (4 * f64(s["pulse_sigma"]).square())
    x0, y0, t0 = f64(s["offset_x"]), f64(s["offset_y"]), f64(s["pulse_center"])
    a, nu, phit, g, h, x0, y0, t0 = (v[..., None] for v in torch.broadcast_tensors(a, nu, phit, g, h, x0, y0, t0))
    x = particles.to(F64)
    x = x.expand(*torch.broadcast_shapes(a.shape[:-1], x.shape[:-2]), *x.shape[-2:])
    u, v, tau, delta = x[..., 0] - x0, x[..., 2] - y0, x[..., 4], x[..., 5]
    w = tau - t0
    t = tau * nu + phit
    f = t - torch.round(t)
    Ex = torch.exp(-g * (u * u + v * v) - h * (w * w))
    cols = list(x.unbind(-1))
    cols[5] = delta + a * Ex * torch.sin(TWO_PI * f)
    out = torch.stack(cols, dim=-1)
    return torch.where((a == 0)[..., None], x, out)            # a row that is not kicked keeps its bits


def _particles(N, dtype, seed=0, batch=(), turns=2000.0):
    """x, y ~ 1e-4, delta ~ 1e-3, tau uniform over +-`turns` wavelengths."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*batch, N, 7, generator=g, dtype=F64) * torch.tensor([1e-4, 1e-4, 1e-4, 1e-4, 0.0, 1e-3, 0.0], dtype=F64)
    x[..., 4] = (2 * torch.rand(*batch, N, generator=g, dtype=F64) - 1) * turns * WAVELENGTH
    x[..., 6] = 1.0
    return x.to(dtype).cuda()


def _beam(x, energy=ENERGY):
    import cheetah_amd as ca

    e = energy if isinstance(energy, torch.Tensor) else torch.tensor(energy, dtype=x.dtype, device="cuda")
    return ca.ParticleBeam(x, e, dtype=x.dtype, device="cuda")


def _settings(dtype, **kw):
    """The default case (a 50 keV modulation at 800 nm, sigma_r = 150 um, no envelope, laser on axis) with `kw` in its place."""
    s = {"amplitude": 50e3, "wavelength": WAVELENGTH, "phase": 0.0, "laser_sigma": 1.5e-4, "offset_x": 0.0, "offset_y": 0.0,
         "pulse_sigma": None, "pulse_center": 0.0}
    s.update(kw)
    return {k: v if v is None or isinstance(v, torch.Tensor) else torch.tensor(v, dtype=dtype, device="cuda") for k, v in s.items()}


def _kick(s, dtype):
    import cheetah_amd as ca

    return ca.LaserModulator(**s, dtype=dtype, device="cuda")


def _dev(got, ref, col=5):
    """max |got - ref| / max |ref| of a column."""
    got, ref = got.to(F64).reshape(-1, 7), ref.to(F64).reshape(-1, 7)
    return float((got[:, col] - ref[:, col]).abs().max() / ref[:, col].abs().max())


def _rel(got, ref):
    return float((got.to(F64) - ref.to(F64)).abs().max() / ref.to(F64).abs().max())


def _bit_equal(a, b):
    """Equal as bits (NaN payloads and signed zeros included)."""
    it = torch.int64 if a.dtype == F64 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------
def _forward_cases(dtype):
    """(name, batch shape of the beam, settings, shape of the result's batch): one and three batch rows, settings of shapes (), (3,)
    and (3, 1) against a (1, N, 7) and a (3, N, 7) beam, either sign of the amplitude, with and without envelope, laser off axis."""
    off = {"offset_x": 3e-5, "offset_y": -2e-5}
    pulse = {"pulse_sigma": 1e-3, "pulse_center": 2e-4}
    return [
        ("scalars, one row", (1,), _settings(dtype, phase=0.3, **off), (1,)),
        ("scalars, one row, envelope", (1,), _settings(dtype, amplitude=-50e3, phase=-2.0, **off, **pulse), (1,)),
        ("(3,) settings, shared beam", (1,), _settings(dtype, amplitude=[50e3, -20e3, 35e3], phase=[0.0, 1.0, -4.0],
                                                      pulse_sigma=[1e-3, 5e-4, 2e-3], pulse_center=2e-4, **off), (3,)),
        ("scalars, three beams", (3,), _settings(dtype, amplitude=-30e3, phase=0.5, **off, **pulse), (3,)),
        ("(3,) settings, three beams", (3,), _settings(dtype, wavelength=[8e-7, 5.32e-7, 1.03e-6], laser_sigma=[1.5e-4, 1e-4, 3e-4],
                                                      offset_x=[3e-5, 0.0, -5e-5], offset_y=-2e-5), (3,)),
        ("(3, 1) settings, shared beam", (1,), _settings(dtype, amplitude=[[50e3], [-20e3], [35e3]], wavelength=[[8e-7], [5.32e-7], [1.03e-6]],
                                                        offset_y=[[0.0], [1e-5], [-2e-5]], offset_x=3e-5, **pulse), (3, 1)),
    ]


# measured on an MI355X, largest over the cases and sizes below of each dtype: float64 2.202e-16 (two ulp of the column's largest
# value: the reduced phase is bit-equal, what differs is exp, sin(2 pi f) against sincospi(2 f) and the last sum), float32 5.196e-08
# (under one float32 ulp of the column's largest value: the arithmetic is float64, rounded once)
FORWARD_BOUND = {F64: 4 * 2.202e-16, F32: 4 * 5.196e-08}


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("N", [1, 255, 257, 511, 513, 1300])
def test_forward_against_the_restatement(N, dtype):
    worst = 0.0
    for i, (name, beam_batch, s, out_batch) in enumerate(_forward_cases(dtype)):
        x = _particles(N, dtype, seed=10 * N + i, batch=beam_batch)
        e = torch.tensor(ENERGY, dtype=dtype, device="cuda")
        out = _kick(s, dtype).track(_beam(x, e)).particles
        assert out.shape == (*out_batch, N, 7) and out.dtype == dtype, name
        ref = _restate(x, e, s, _mass(dtype))
        assert ref.shape == out.shape
        for c in PASS_THROUGH:
            assert _bit_equal(out[..., c], x[..., c].expand(*out_batch, N)), (name, c)
        assert float((out[..., 5] - x[..., 5]).abs().max()) > 0 and torch.isfinite(out).all(), name
        dev = _dev(out, ref)
        print(f"forward N={N} {dtype} {name}: {dev:.3e}")
        worst = max(worst, dev)
    print(f"forward N={N} {dtype}: worst {worst:.3e}")
    assert worst <= FORWARD_BOUND[dtype]


# ---- 2. switches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_a_row_of_amplitude_zero_keeps_every_bit(dtype):
    x = _particles(513, dtype, seed=3)
    x[4, 5] = -0.0
    x[5, 1] = -0.0
    x[7, 5] = float("nan")
    x[8, 0] = float("inf")
    beam = _beam(x)
    for pulse in (None, 1e-3):
        out = _kick(_settings(dtype, amplitude=[50e3, 0.0, -50e3], phase=0.3, pulse_sigma=pulse), dtype).track(beam).particles
        assert out.shape == (3, 513, 7)
        assert _bit_equal(out[1], x)
        assert bool(torch.signbit(out[1, 4, 5])) and bool(torch.signbit(out[1, 5, 1]))
        for b in (0, 2):
            assert not torch.equal(out[b, :4, 5], x[:4, 5])
        # -0.0 + a kick is the kick; opposite amplitudes give opposite kicks
        assert float(out[0, 4, 5]) == -float(out[2, 4, 5]) != 0.0
    # alone as well
    assert _bit_equal(_kick(_settings(dtype, amplitude=0.0), dtype).track(beam).particles, x)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_non_finite_coordinates_stay_in_their_particle(dtype):
    x = _particles(513, dtype, seed=4)
    s = _settings(dtype, phase=0.3, pulse_sigma=1e-3)
    clean = _kick(s, dtype).track(_beam(x)).particles
    x2 = x.clone()
    x2[100, 4] = float("nan")
    x2[200, 0] = float("inf")
    x2[300, 2] = float("-inf")
    x2[400, 5] = float("inf")
    out = _kick(s, dtype).track(_beam(x2)).particles
    spoiled = (100, 200, 300, 400)
    for n in spoiled:
        assert not bool(torch.isfinite(out[n, 5])), n
        assert _bit_equal(out[n, list(PASS_THROUGH)], x2[n, list(PASS_THROUGH)]), n
    others = [n for n in range(513) if n not in spoiled]
    assert _bit_equal(out[others], clean[others])
    # without an envelope h = 0 meets the NaN tau and the infinite x all the same
    out = _kick(_settings(dtype, phase=0.3), dtype).track(_beam(x2)).particles
    assert not bool(torch.isfinite(out[list(spoiled), 5]).any()) and bool(torch.isfinite(out[others]).all())


# ---- 3. gradients ----------------------------------------------------------------------------------------------------------------
# measured on an MI355X against autograd through the restatement, largest over N = 1300 and (float64) N = 65 795: float64 particles
# 3.880e-16, energy 1.099e-15, amplitude 3.522e-16, wavelength 1.043e-15, phase 2.665e-16, laser_sigma 1.235e-15, offset_x 1.997e-16,
# offset_y 1.134e-16, pulse_sigma 3.006e-16, pulse_center 5.614e-16; float32 particles 9.003e-08 (the sum over the three rows is
# formed in float32) and 0 for the energy and the eight settings: their float64 gradients agree as in the float64 case and both sides
# round them once to float32, to the same bits
GRAD_BOUND = {F64: {"particles": 4 * 3.880e-16, "energy": 4 * 1.099e-15, "amplitude": 4 * 3.522e-16, "wavelength": 4 * 1.043e-15,
                    "phase": 4 * 2.665e-16, "laser_sigma": 4 * 1.235e-15, "offset_x": 4 * 1.997e-16, "offset_y": 4 * 1.134e-16,
                    "pulse_sigma": 4 * 3.006e-16, "pulse_center": 4 * 5.614e-16},
              F32: {"particles": 4 * 9.003e-08, "energy": 0.0, "amplitude": 0.0, "wavelength": 0.0, "phase": 0.0, "laser_sigma": 0.0,
                    "offset_x": 0.0, "offset_y": 0.0, "pulse_sigma": 0.0, "pulse_center": 0.0}}


def _gradients(N, dtype, through_kernel):
    """d(sum(out * W)) / d(particles (1, N, 7), energy (), the eight settings: amplitude and phase (3,), offset_x (3,), the rest ()),
    float64 weights W (3, N, 7)."""
    import cheetah_amd as ca

    g = torch.Generator().manual_seed(N)
    W = torch.randn(3, N, 7, generator=g, dtype=F32).to(F64).cuda()     # float32 values: the same cotangent for either beam dtype
    x = _particles(N, dtype, seed=N + 1, batch=(1,)).requires_grad_(True)
    e = torch.tensor(ENERGY, dtype=dtype, device="cuda", requires_grad=True)
    s = _settings(dtype, amplitude=[50e3, -20e3, 35e3], phase=[0.3, 1.0, -4.0], offset_x=[3e-5, 0.0, -5e-5], offset_y=-2e-5,
                  pulse_sigma=1e-3, pulse_center=2e-4)
    if through_kernel:
        kick = ca.LaserModulator(**{k: torch.nn.Parameter(v) for k, v in s.items()}, dtype=dtype, device="cuda")
        out = kick.track(_beam(x, e)).particles
        assert out.shape == (3, N, 7) and out.dtype == dtype
        (out.to(F64) * W).sum().backward()
        return {"particles": x.grad, "energy": e.grad, **{k: getattr(kick, k).grad for k in SETTINGS}}
    s = {k: v.requires_grad_(True) for k, v in s.items()}
    (_restate(x, e, s, _mass(dtype)) * W).sum().backward()
    return {"particles": x.grad, "energy": e.grad, **{k: v.grad for k, v in s.items()}}


@pytest.mark.parametrize("N, dtype", [(1300, F64), (1300, F32), (65_795, F64)])
def test_gradients_against_autograd_of_the_restatement(N, dtype):
    """N = 65 795 is 257 tiles of 256 rows and 3: the strided sum of the workgroups' partials runs past one stride."""
    got, ref = _gradients(N, dtype, True), _gradients(N, dtype, False)
    again = _gradients(N, dtype, True)
    assert got["particles"].shape == (1, N, 7) and got["amplitude"].shape == (3,) and got["energy"].shape == ()
    assert got["offset_x"].shape == (3,) and got["wavelength"].shape == ()
    for name in got:
        assert got[name].dtype == dtype, name                  # a float32 beam's settings gradients come back in float32
        assert _bit_equal(got[name], again[name]), name         # two backward runs
    # the pass-through columns hand their cotangent on, summed over the three rows in the beam's dtype
    devs = {"particles": max(_rel(got["particles"][..., c], ref["particles"][..., c]) for c in range(7))}
    assert float(got["particles"][..., 6].abs().max()) > 0
    for name in ("energy",) + SETTINGS:
        devs[name] = _rel(got[name], ref[name])
    print(f"gradients N={N} {dtype}: " + ", ".join(f"{k} {v:.3e}" for k, v in devs.items()))
    for name, dev in devs.items():
        assert dev <= GRAD_BOUND[dtype][name], name


# ---- 4. physics ------------------------------------------------------------------------------------------------------------------
# measured on an MI355X, absolute: 1.388e-15, 0, 1.776e-15 and 2.355e-12 for the four arguments; the largest is the identity's own
# error on this grid (3e-12 in a float64 restatement on the CPU: 64 points per wavelength alias J1 with Bessel functions of order 63
# and 65, which only k R56 a = 3 lifts above rounding)
BUNCHING_BOUND = 4 * 2.355e-12


@pytest.mark.parametrize("arg", [0.5, 1.0, 1.8412, 3.0])
def test_a_chicane_turns_the_modulation_into_bunching(arg):
    """4096 particles on a uniform tau grid over 64 wavelengths at delta = 0, modulated with a = A / p0c = 2e-5, then
    tau <- tau + R56 delta: the bunching factor at the laser wavelength has modulus J1(k R56 a)."""
    import cheetah_amd as ca

    N, a = 4096, 2e-5
    x = torch.zeros(N, 7, dtype=F64, device="cuda")
    x[:, 4] = (torch.arange(N, dtype=F64, device="cuda") + 0.5) / N * (64 * WAVELENGTH)
    x[:, 6] = 1.0
    beam = _beam(x)
    kick = _kick(_settings(F64, amplitude=a * beam.p0c, laser_sigma=1.0), F64)
    out = kick.track(beam).particles
    top = float(out[:, 5].abs().max()) / a                       # 64 grid points per wavelength: the largest sine is sin(2 pi 15.5 / 64)
    assert abs(top / math.sin(TWO_PI * 15.5 / 64) - 1) < 1e-12
    k = TWO_PI / WAVELENGTH
    r56 = arg / (k * a)
    y = out.clone()
    y[:, 4] = out[:, 4] + r56 * out[:, 5]
    b = _beam(y).bunching_factor(WAVELENGTH)
    want = float(torch.special.bessel_j1(torch.tensor(k * r56 * a, dtype=F64)))
    dev = abs(float(b.abs().reshape(())) - abs(want))
    print(f"bunching at k R56 a = {arg}: |b| - |J1| = {dev:.3e} (J1 = {want:.6f})")
    assert dev <= BUNCHING_BOUND


def test_the_heater_leaves_the_expected_energy_spread():
    """2^16 particles, Gaussian in x (150 um) and y (100 um), a laser of sigma_r = 120 um, tau uniform over many wavelengths:
    mean(d delta^2) = a^2 / 2 / sqrt((1 + sigma_x^2 / sigma_r^2) (1 + sigma_y^2 / sigma_r^2)), within four standard errors, the
    standard error taken from the restatement's own sample of d delta^2."""
    N, sx, sy, sr = 2**16, 150e-6, 100e-6, 120e-6
    g = torch.Generator().manual_seed(1)
    x = torch.zeros(N, 7, dtype=F64)
    x[:, 0] = torch.randn(N, generator=g, dtype=F64) * sx
    x[:, 2] = torch.randn(N, generator=g, dtype=F64) * sy
    x[:, 4] = (2 * torch.rand(N, generator=g, dtype=F64) - 1) * 2000 * WAVELENGTH
    x[:, 6] = 1.0
    x = x.cuda()
    beam = _beam(x)
    s = _settings(F64, laser_sigma=sr)
    a = float(s["amplitude"] / beam.p0c)
    out = _kick(s, F64).track(beam).particles
    ref = _restate(x, beam.energy, s, _mass())
    got = float(out[:, 5].square().mean())
    sample = ref[:, 5].square()
    stderr = float(sample.std() / math.sqrt(N))
    want = a * a / 2 / math.sqrt((1 + sx**2 / sr**2) * (1 + sy**2 / sr**2))
    print(f"mean(d delta^2) = {got:.6e}, expected {want:.6e}: {(got - want) / want:+.2%}, {abs(got - want) / stderr:.2f} standard errors")
    assert abs(got - want) <= 4 * stderr


# ---- 5. in a lattice -------------------------------------------------------------------------------------------------------------
def _walk(elements, beam):
    for e in elements:
        beam = e.track(beam)
    return beam


def _heater_lattice():
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    und = ca.Undulator(t(0.5), period=t(0.05), ky=t(1.385), name="und", **kw)
    laser = und.with_laser(1.2e6, 175e-6, ENERGY, phase=0.3, offset_x=2e-5, pulse_sigma=1e-3, num_kicks=2)
    els = [ca.Drift(t(0.4), name="d1", **kw), ca.Quadrupole(t(0.1), k1=t(2.5), name="q1", **kw), *laser.elements,
           ca.Drift(t(0.3), name="d2", **kw)]
    return und, els


def _heater_beam():
    import cheetah_amd as ca

    kw = {"dtype": F64, "device": "cuda"}
    t = lambda v: torch.tensor(v, **kw)  # noqa: E731
    torch.manual_seed(5)
    return ca.ParticleBeam.from_parameters(num_particles=10_000, sigma_x=t(2e-4), sigma_y=t(1.5e-4), sigma_tau=t(3e-4), sigma_p=t(1e-5),
                                           energy=t(ENERGY), **kw)


def test_in_a_lattice_with_an_undulator(tmp_path):
    """`Segment([Drift, Quadrupole, *undulator.with_laser(num_kicks=2).elements, Drift]).track` against the walk at equal bits. The
    segment composes each run of linear elements into one map before it applies it, which rounds differently from separate
    passes, so the walk tracks every run as the segment forms it (`tests/test_gpu_synchrotron_radiation.py` does the same with its
    leading run). A lattice written to LatticeJSON and read back tracks to the same bits."""
    import cheetah_amd as ca

    und, els = _heater_lattice()
    assert [type(e).__name__ for e in els] == ["Drift", "Quadrupole", "Undulator", "LaserModulator", "Undulator", "Undulator",
                                               "LaserModulator", "Undulator", "Drift"]
    beam = _heater_beam()
    seg = ca.Segment(els, name="heater")
    with torch.no_grad():
        got = seg.track(beam)
        ref = _walk([ca.Segment(els[:3]), els[3], ca.Segment(els[4:6]), els[6], ca.Segment(els[7:])], beam)
        quiet = _walk([ca.Segment(els[:3]), ca.Segment(els[4:6]), ca.Segment(els[7:])], beam)
    assert torch.isfinite(got.particles).all()
    assert _bit_equal(got.particles, ref.particles) and torch.equal(got.s, ref.s)
    # the modulation is there: two kicks of 38.8 keV each in phase on 135 MeV, less off axis
    kick = float((got.particles[:, 5] - quiet.particles[:, 5]).abs().max())
    assert 0.5 * 77.6e3 / ENERGY < kick < 1.01 * 77.6e3 / ENERGY
    path = tmp_path / "heater.json"
    ca.latticejson.save_cheetah_model(seg, str(path))
    back = ca.latticejson.load_cheetah_model(str(path), device="cuda", dtype=F64)
    assert [type(e) for e in back.elements] == [type(e) for e in els]
    with torch.no_grad():
        again = back.track(beam)
    assert _bit_equal(again.particles, got.particles)


def test_the_undulator_pieces_compose_to_the_undulator():
    """The map of the four pieces of `with_laser(num_kicks=2)` against the undulator's own, to rounding: the entries are sines,
    cosines and a sum of four equal lengths, a few ulp of the largest entry of a row of the map."""
    import cheetah_amd as ca

    und, els = _heater_lattice()
    pieces = [e for e in els if isinstance(e, ca.Undulator)]
    assert len(pieces) == 4
    beam = _heater_beam()
    total = torch.eye(7, dtype=F64, device="cuda")
    for p in pieces:
        total = p.first_order_transfer_map(beam.energy, beam.species) @ total
    own = und.first_order_transfer_map(beam.energy, beam.species)
    dev = float(((total - own).abs().max(dim=-1).values / own.abs().max(dim=-1).values).max())
    print(f"undulator pieces against the undulator, relative to a row's largest entry: {dev:.3e}")
    assert dev <= 16 * 2.0 ** -53


# ---- 6. capture ------------------------------------------------------------------------------------------------------------------
def test_graph_capture_follows_the_phase():
    import cheetah_amd as ca

    x = _particles(1300, F32, seed=10)
    beam = _beam(x)
    kick = _kick(_settings(F32, phase=0.3, offset_x=3e-5, pulse_sigma=1e-3), F32)
    with torch.no_grad():
        first, second = kick.track(beam).particles, kick.track(beam).particles
        assert _bit_equal(first, second)                        # two eager runs
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            kick.track(beam)
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            captured = kick.track(beam).particles
        graph.replay()
        assert _bit_equal(captured, first)
        kick.phase.copy_(torch.tensor(1.7, dtype=F32, device="cuda"))
        graph.replay()
        replayed = captured.clone()
        eager = kick.track(beam).particles
        assert _bit_equal(replayed, eager)
        assert not torch.equal(replayed[:, 5], first[:, 5])
        twin = _kick(_settings(F32, phase=1.7, offset_x=3e-5, pulse_sigma=1e-3), F32)
        assert _bit_equal(twin.track(beam).particles, eager)
