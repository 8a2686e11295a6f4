"""`ParticleBeam.with_density_modulation` on the GPU: tau' against a float64 torch restatement of the kernel's solver (safeguarded
Newton, the phase reduced in turns) and the residual of the defining equation, the bits that must not change, the bunching factor
the modulation leaves on a quiet-start beam, gradients against autograd through the restatement, reproducibility, graph capture
and the absence of host synchronisation. One process, no workers.

Every floating-point bound is 4x the deviation measured on an MI355X, which stands in the comment next to it;
the bounds on the bunching factor are fixed: 0.1 / sqrt(N). Deviations of tau' and residuals are in units of the row's shortest
wavelength; deviations of gradients are max |got - ref| over max |ref|."""
import cmath
import functools
import math

import pytest
import torch

from tests.quiet_ref import modulate_tau, modulation_residual
from tests.test_gpu_no_sync import sync_warnings

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
SIGMA_TAU = 1e-4
N_BEAM = 65536
PASS_THROUGH = (0, 1, 2, 3, 5, 6)


def dev64(v):
    return torch.tensor(v, dtype=F64, device="cuda")


def _particles(N, dtype, seed=0, batch=()):
    """x, y ~ 1e-4, delta ~ 1e-3, tau ~ SIGMA_TAU: some twenty to a hundred wavelengths of the cases below along the bunch."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*batch, N, 7, generator=g, dtype=F64) * torch.tensor([1e-4, 1e-5, 1e-4, 1e-5, SIGMA_TAU, 1e-3, 0.0], dtype=F64)
    x[..., 6] = 1.0
    return x.to(dtype).cuda()


def _beam(x):
    import cheetah_amd as ca

    return ca.ParticleBeam(x, torch.tensor(1e8, dtype=x.dtype, device="cuda"), dtype=x.dtype, device="cuda")


def _restate(x, lam, A, phi):
    """The whole result in float64: tau through `modulate_tau`, every other column as it is -> (*batch, N, 7)."""
    batch = torch.broadcast_shapes(x.shape[:-2], lam.shape[:-1], A.shape[:-1], phi.shape[:-1])
    xe = x.to(F64).expand(*batch, *x.shape[-2:])
    cols = list(xe.unbind(-1))
    cols[4] = modulate_tau(cols[4], A, lam, phi)
    return torch.stack(cols, dim=-1)


def _bit_equal(a, b):
    """Equal as bits (NaN payloads and signed zeros included)."""
    it = torch.int64 if a.dtype == F64 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---- 1. forward ----------------------------------------------------------------------------------------------------------------------
def _forward_cases():
    """(name, batch shape of the beam, wavelengths, amplitudes, phases, batch shape of the result): one and three modes,
    sum |A| = 0.95, settings (K,) and (3, K) against a (1, N, 7) and a (3, N, 7) beam."""
    lam3 = [SIGMA_TAU / 20, SIGMA_TAU / 7, SIGMA_TAU / 45]
    return [
        ("one mode", (1,), dev64([SIGMA_TAU / 20]), dev64([0.02]), dev64([0.7]), (1,)),
        ("one mode, sum |A| = 0.95", (1,), dev64([SIGMA_TAU / 20]), dev64([0.95]), dev64([-2.0]), (1,)),
        ("three modes, sum |A| = 0.95", (1,), dev64(lam3), dev64([0.5, -0.3, 0.15]), dev64([0.7, -2.0, 3.0]), (1,)),
        ("three modes, three beams", (3,), dev64(lam3), dev64([0.2, 0.1, -0.05]), dev64([0.0, 1.0, -4.0]), (3,)),
        ("(3, K) settings, shared beam", (1,), dev64([lam3, lam3[::-1], [2e-6, 3e-6, 5e-6]]),
         dev64([[0.5, -0.3, 0.15], [0.02, 0.05, 0.0], [-0.3, -0.3, -0.35]]), dev64([[0.7, -2.0, 3.0], [0.0, 0.0, 0.0], [1.0, 2.0, 3.0]]),
         (3,)),
        ("(3, K) amplitudes, three beams", (3,), dev64(lam3), dev64([[0.5, -0.3, 0.15], [0.02, 0.05, 0.0], [-0.3, -0.3, -0.35]]),
         dev64([0.7, -2.0, 3.0]), (3,)),
        ("(3, 1) settings, one mode", (3,), dev64([[SIGMA_TAU / 20], [SIGMA_TAU / 50], [SIGMA_TAU / 5]]),
         dev64([[0.95], [-0.4], [0.02]]), dev64([0.3]), (3,)),
    ]


# measured on an MI355X, largest over the cases of each dtype, in units of the row's shortest wavelength: |tau' - restatement| and the
# residual of the defining equation at the tau' the kernel stored (float32: that of rounding tau' to float32, once)
# float64: deviation 3.049e-14, residual 4.879e-14; float32: deviation 7.265e-06, residual 1.274e-05
FORWARD_BOUND = {F64: 4 * 3.049e-14, F32: 4 * 7.265e-06}
RESIDUAL_BOUND = {F64: 4 * 4.879e-14, F32: 4 * 1.274e-05}


@pytest.mark.parametrize("dtype", [F64, F32])
def test_forward_against_the_restatement(dtype):
    N = 3001
    worst, worst_res = 0.0, 0.0
    for i, (name, beam_batch, lam, A, phi, out_batch) in enumerate(_forward_cases()):
        x = _particles(N, dtype, seed=i, batch=beam_batch)
        out = _beam(x).with_density_modulation(lam, A, phi).particles
        assert out.shape == (*out_batch, N, 7) and out.dtype == dtype, name
        for c in PASS_THROUGH:
            assert _bit_equal(out[..., c], x[..., c].expand(*out_batch, N)), (name, c)
        assert torch.isfinite(out).all() and float((out[..., 4] - x[..., 4]).abs().max()) > 0, name
        ref = _restate(x, lam, A, phi)
        nu_max = (1 / lam).max(dim=-1, keepdim=True).values
        dev = float(((out[..., 4].to(F64) - ref[..., 4]).abs() * nu_max).max())
        res = float(modulation_residual(out[..., 4], x[..., 4].expand(*out_batch, N), A, lam, phi).max())
        print(f"forward {dtype} {name}: deviation {dev:.3e}, residual {res:.3e}")
        worst, worst_res = max(worst, dev), max(worst_res, res)
    print(f"forward {dtype}: worst deviation {worst:.3e}, worst residual {worst_res:.3e}")
    assert worst <= FORWARD_BOUND[dtype] and worst_res <= RESIDUAL_BOUND[dtype]


@pytest.mark.parametrize("dtype", [F64, F32])
def test_bits_that_do_not_change(dtype):
    N = 3001
    x = _particles(N, dtype, seed=20, batch=(1,))
    x[0, 5, 4], x[0, 300, 4], x[0, 2999, 4] = float("nan"), float("inf"), float("-inf")
    x[0, 7, 0], x[0, 8, 5] = float("nan"), float("inf")              # other columns do not matter to tau'
    lam = dev64([SIGMA_TAU / 20, SIGMA_TAU / 7])
    A = dev64([[0.02, 0.05], [0.0, 0.0], [-0.0, 0.0], [0.6, 0.6], [0.5, 0.5], [float("nan"), 0.1]])
    out = _beam(x).with_density_modulation(lam, A, 0.3).particles
    assert out.shape == (6, N, 7)
    for c in PASS_THROUGH:
        assert _bit_equal(out[..., c], x[..., c].expand(6, N)), c
    odd = torch.zeros(N, dtype=torch.bool, device="cuda")
    odd[[5, 300, 2999]] = True
    for b in range(6):                                              # a non-finite tau stays as it is, in every row
        assert _bit_equal(out[b, odd, 4], x[0, odd, 4]), b
    assert torch.isfinite(out[0, ~odd, 4]).all() and not torch.equal(out[0, ~odd, 4], x[0, ~odd, 4])
    assert _bit_equal(out[1], x[0]) and _bit_equal(out[2], x[0])    # rows with every A = 0 keep every bit
    for b in (3, 4, 5):                                             # sum |A| >= 1, or NaN: no unique root, tau' is NaN
        assert torch.isnan(out[b, ~odd, 4]).all(), b


def test_a_negative_wavelength_on_the_device_is_its_period_with_the_phase_reversed():
    """Device tensors are used as given: nu < 0 is the same period (the step that ends the solver is measured in |nu|), and the
    equation is that of -nu with -phi, term by term with the same bits."""
    x = _particles(3001, F64, seed=21, batch=(1,))
    lam, A, phi = dev64([SIGMA_TAU / 20, SIGMA_TAU / 7]), dev64([0.5, -0.4]), dev64([0.7, -2.0])
    out = _beam(x).with_density_modulation(-lam, A, phi).particles
    twin = _beam(x).with_density_modulation(lam, A, -phi).particles
    assert torch.isfinite(out).all() and _bit_equal(out, twin)


# ---- 2. physics ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _quiet_beam():
    import cheetah_amd as ca

    return ca.ParticleBeam.from_parameters(num_particles=N_BEAM, sigma_tau=dev64(SIGMA_TAU), dtype=F64, device="cuda",
                                           quiet_start=True)


def test_one_mode_on_a_quiet_beam_gives_the_bunching_it_was_asked_for():
    """|b(k) - (A / 2) exp(i phi)| <= 0.1 / sqrt(N) = 3.9e-4; a CPU float64 run of the scheme gave 2.7e-5."""
    A, phi, lam = 0.02, 0.7, SIGMA_TAU / 20
    b = _quiet_beam().with_density_modulation(lam, A, phi).bunching_factor(lam).cpu()
    err = abs(complex(b[0]) - A / 2 * cmath.exp(1j * phi))
    print(f"one mode: b = {complex(b[0]):.6e}, |b - A/2 e^(i phi)| = {err:.3e}")
    assert err <= 0.1 / math.sqrt(N_BEAM)


def test_two_modes_on_a_quiet_beam():
    """Each mode within 0.1 / sqrt(N) of (A / 2) exp(i phi) (CPU float64 run: 1.6e-5 and 3.2e-5), a third wavelength still quiet
    (2.5e-5), and the map monotone: sorting by tau sorts tau'."""
    lam, A, phi = [SIGMA_TAU / 20, SIGMA_TAU / 7], [0.02, 0.05], [0.7, -2.0]
    beam = _quiet_beam()
    out = beam.with_density_modulation(lam, A, phi)
    b = out.bunching_factor(lam + [SIGMA_TAU / 5]).cpu()
    errs = [abs(complex(b[m]) - A[m] / 2 * cmath.exp(1j * phi[m])) for m in range(2)]
    print(f"two modes: errors {errs[0]:.3e}, {errs[1]:.3e}; |b| at sigma / 5: {abs(complex(b[2])):.3e}")
    bound = 0.1 / math.sqrt(N_BEAM)
    assert errs[0] <= bound and errs[1] <= bound and abs(complex(b[2])) <= bound
    order = torch.argsort(beam.particles[:, 4])
    assert bool((torch.diff(out.particles[order, 4]) >= 0).all())


# ---- 3. gradients ----------------------------------------------------------------------------------------------------------------------
# measured on an MI355X, largest over the cases: max |got - ref| / max |ref| of the gradient of each input: particles 5.177e-15,
# amplitudes 4.047e-14, wavelengths 7.714e-14, phases 7.846e-14 (sums over 513 particles of terms of either sign)
GRAD_BOUND = {"particles": 4 * 5.177e-15, "amplitudes": 4 * 4.047e-14, "wavelengths": 4 * 7.714e-14, "phases": 4 * 7.846e-14}


def _grad_cases():
    lam3 = [SIGMA_TAU / 20, SIGMA_TAU / 7, SIGMA_TAU / 45]
    return [
        ("one row, one mode", (1,), dev64([SIGMA_TAU / 20]), dev64([0.3]), dev64([0.7])),
        ("one row, three modes", (1,), dev64(lam3), dev64([0.5, -0.3, 0.15]), dev64([0.7, -2.0, 3.0])),
        ("three rows, shared beam", (1,), dev64([lam3, lam3[::-1], [2e-6, 3e-6, 5e-6]]),
         dev64([[0.5, -0.3, 0.15], [0.02, 0.05, 0.0], [-0.3, -0.3, -0.35]]), dev64([0.7, -2.0, 3.0])),
        ("three rows, three beams", (3,), dev64(lam3), dev64([[0.5, -0.3, 0.15], [0.02, 0.05, 0.0], [-0.3, -0.3, -0.35]]),
         dev64([[0.7, -2.0, 3.0], [0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])),
    ]


def test_gradients_against_autograd_through_the_restatement():
    N = 513                                                         # more than one tile in float64
    worst = dict.fromkeys(GRAD_BOUND, 0.0)
    for i, (name, beam_batch, lam, A, phi) in enumerate(_grad_cases()):
        x = _particles(N, F64, seed=40 + i, batch=beam_batch)
        batch = torch.broadcast_shapes(beam_batch, lam.shape[:-1], A.shape[:-1], phi.shape[:-1])
        w = torch.randn(*batch, N, 7, generator=torch.Generator().manual_seed(60 + i), dtype=F64).cuda()
        grads = []
        for fn in (lambda x, lam, A, phi: _beam(x).with_density_modulation(lam, A, phi).particles, _restate):
            leaves = [t.clone().requires_grad_(True) for t in (x, lam, A, phi)]
            (fn(*leaves) * w).sum().backward()
            grads.append([t.grad for t in leaves])
        for key, got, ref in zip(("particles", "wavelengths", "amplitudes", "phases"), *grads):
            assert got.shape == ref.shape and got.dtype == F64, (name, key)
            dev = float((got - ref).abs().max() / ref.abs().max())
            print(f"gradient {name} {key}: {dev:.3e}")
            worst[key] = max(worst[key], dev)
        # every other column hands its cotangent on, bit for bit; a shared beam's rows are summed as the same torch sum sums them
        want = w.sum(dim=0, keepdim=True) if beam_batch == (1,) else w
        for c in PASS_THROUGH:
            assert _bit_equal(grads[0][0][..., c], want[..., c]), (name, c)
    print("gradients: worst", {k: f"{v:.3e}" for k, v in worst.items()})
    for key, bound in GRAD_BOUND.items():
        assert worst[key] <= bound, key


# measured on an MI355X, max |got - ref| / max |ref| of the settings' gradients behind a float32 beam: wavelengths 1.003e-13,
# amplitudes 1.129e-14, phases 8.772e-15
F32_GRAD_BOUND = {"wavelengths": 4 * 1.003e-13, "amplitudes": 4 * 1.129e-14, "phases": 4 * 8.772e-15}


def test_gradients_of_a_float32_beam_and_of_particles_without_a_root():
    """A float32 beam (the float32 instantiation of the backward kernel: two particles per lane, tiles of 512 rows): float32
    gradients of the particles, equal to the restatement's rounded to float32, float64 gradients of the float64 settings within 4x
    the measured deviation; a non-finite tau has a gradient of exactly 0."""
    N = 513
    lam, A, phi = dev64([SIGMA_TAU / 20, SIGMA_TAU / 7]), dev64([0.3, -0.2]), dev64([0.7, -2.0])
    x_ref = _particles(N, F32, seed=50, batch=(1,))
    x = x_ref.clone()
    x[0, 3, 4] = float("nan")                                       # (the restatement gets a finite tau there, and no cotangent)
    w = torch.randn(1, N, 7, generator=torch.Generator().manual_seed(70), dtype=F32).cuda()
    grads = []
    for fn in (lambda x, lam, A, phi: _beam(x).with_density_modulation(lam, A, phi).particles, _restate):
        leaves = [t.clone().requires_grad_(True) for t in (x_ref if fn is _restate else x, lam, A, phi)]
        out = fn(*leaves)
        keep = torch.ones(N, dtype=torch.bool, device="cuda")
        keep[3] = False
        (out[:, keep] * w[:, keep]).sum().backward()
        grads.append([t.grad for t in leaves])
    got, ref = grads
    assert got[0].dtype == F32 and all(g.dtype == F64 for g in got[1:])
    assert float(got[0][0, 3, 4]) == 0.0
    assert ref[0].dtype == F32 and float(ref[0].abs().max()) > 0
    print(f"float32 gradient particles: largest difference {float((got[0] - ref[0]).abs().max()):.3e}")
    assert torch.equal(got[0], ref[0])                             # measured on an MI355X: no difference
    for key, g, r in zip(("wavelengths", "amplitudes", "phases"), got[1:], ref[1:]):
        dev = float((g - r).abs().max() / r.abs().max())
        print(f"float32 gradient {key}: {dev:.3e}")
        assert dev <= F32_GRAD_BOUND[key], key


# ---- 4. runtime behaviour --------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits():
    N = 3001
    lam = dev64([SIGMA_TAU / 20, SIGMA_TAU / 7, SIGMA_TAU / 45])
    A = dev64([[0.5, -0.3, 0.15], [0.02, 0.05, 0.0], [-0.3, -0.3, -0.35]])
    phi = dev64([0.7, -2.0, 3.0])
    for dtype in (F64, F32):
        x = _particles(N, dtype, seed=80, batch=(1,))
        w = torch.randn(3, N, 7, generator=torch.Generator().manual_seed(81), dtype=F64).to(dtype).cuda()
        runs = []
        for _ in range(2):
            leaves = [t.clone().requires_grad_(True) for t in (x, lam, A, phi)]
            out = _beam(leaves[0]).with_density_modulation(*leaves[1:]).particles
            (out * w).sum().backward()
            runs.append([out.detach()] + [t.grad for t in leaves])
        for a, b in zip(*runs):
            assert _bit_equal(a, b), dtype


def test_graph_capture_follows_an_amplitude():
    x = _particles(1300, F32, seed=90)
    beam = _beam(x)
    lam, A, phi = dev64([SIGMA_TAU / 20, SIGMA_TAU / 7]), dev64([0.02, 0.05]), dev64([0.7, -2.0])
    run = lambda: beam.with_density_modulation(lam, A, phi).particles  # noqa: E731
    with torch.no_grad():
        first = run()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            captured = run()
        graph.replay()
        assert _bit_equal(captured, first)
        A[1] = 0.3                                                  # in place: the kernel reads the setting on the device
        graph.replay()
        replayed = captured.clone()
        assert _bit_equal(replayed, run())
        assert not torch.equal(replayed[:, 4], first[:, 4])
        twin = beam.with_density_modulation(lam, dev64([0.02, 0.3]), phi).particles
        assert _bit_equal(replayed, twin)


def test_no_host_synchronisation():
    import cheetah_amd as ca

    x = _particles(3001, F32, seed=91)
    beam = _beam(x)
    lam, A, phi = dev64([SIGMA_TAU / 20, SIGMA_TAU / 7]), dev64([0.02, 0.05]), dev64([0.7, -2.0])
    assert len(sync_warnings(lambda: torch.tensor(1.0, device="cuda"), warm=0)) == 1     # the switch sees what it should see
    A_grad = A.clone().requires_grad_(True)

    def forward_backward():
        A_grad.grad = None
        beam.with_density_modulation(lam, A_grad, phi).particles[:, 4].sum().backward()

    flows = {
        "device settings": lambda: beam.with_density_modulation(lam, A, phi),
        "a number for every setting": lambda: beam.with_density_modulation(SIGMA_TAU / 20, 0.02, 0.7),
        "forward + backward": forward_backward,
        "quiet sequence": lambda: ca._ops.quiet_sequence(3001, (5, 7, 11, 13, 2, 3), offset=7, dtype=F32),
    }
    for name, fn in flows.items():
        hits = sync_warnings(fn)
        assert not hits, (name, [(w.filename, w.lineno) for w in hits])
