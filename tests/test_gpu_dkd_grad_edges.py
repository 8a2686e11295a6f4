"""chx_dkd_track_bwd (forward-mode dual numbers through the six Bmad-X maps) at the points where its closed forms change their
branch, at tile edges, under every broadcast of its operands, for float32 beams, and through a Segment — against a gradient
reference that shares no code with the kernel (tests/dkd_grad_ref.py: Richardson differences of the float64 CPU oracle for Drift,
Quadrupole, Dipole and TDC, float64 autograd through the restated maps for Sextupole and RFCavity; pinned on its own by
tests/test_dkd_grad_ref_host.py).

Acceptance: |got - ref| <= 2e-7 |ref| + 4 u + floor (u: the reference's own uncertainty, capped by the host test; floor: 1e-9 of
sum |W x_out| over the parameter's scale — the table, the scales and the steps are in tests/dkd_grad_ref.py).

MEASURED on the MI355X (float64, the table's steps: HREL, H_ENERGY, H_X of tests/dkd_grad_ref.py):
Largest |got - ref| / |ref| per kind, over the gradients that stand clear of the floor (|ref| > 100 floor), beside the largest
u / |ref| of the same gradients and the largest |got - ref| over the acceptance bound. Where the relative figure is above 1e-8 it
is the reference's own rounding (it follows u); the energy's gradient is 1e-14 of the loss per eV, the worst resolved of all:
                 parameters                    dx                            energy
  Drift          2.3e-11  u 1.5e-11  8.8e-6    3.4e-10  u 1.0e-9   1.7e-3    2.1e-5   u 1.8e-5   0.17
  Quadrupole     9.7e-10  u 8.7e-10  1.9e-3    1.2e-8   u 1.6e-8   1.7e-2    1.5e-4   u 1.2e-4   0.074
  Dipole         2.4e-5   u 2.7e-5   0.093     2.4e-6   u 2.0e-6   0.16      2.7e-5   u 1.5e-5   0.23
  TDC            4.7e-9   u 4.1e-9   0.015     2.4e-7   u 2.2e-7   7.5e-3    3.6e-5   u 2.8e-5   0.13
  Sextupole      7.6e-9   u 5.6e-9   1.1e-3    3.0e-13  u 0        2.4e-8    9.7e-8   u 0        1.4e-4
  RFCavity       1.1e-14  u 0        9.5e-9    5.1e-14  u 0        8.1e-9    9.2e-9   u 0        4.8e-5
d/dk1 at k1 = 0: 8.1e-12 (1 step), 9.9e-11 (3 steps), 1.5e-11 (tilted, misaligned); at k1 = +-1e-12: 4.6e-11, 5.9e-11.
Through the Segment: d sigma_x / d k1 of the two quadrupoles 9.2e-13 and 2.9e-12 off the chained reference.
BEFORE the val(w) == 0 branch of quad_coefficients carried its tangent the same cases gave, got against ref:
  quad_k1_0_n1               d/dk1 -1.2019e-4 against -4.1387e-4   (71 % off, 6.9e5 times the bound)
  quad_k1_0_n3               d/dk1 -3.1629e-4 against -4.1387e-4   (24 %)
  quad_k1_0_tilt_misaligned  d/dk1  5.9167e-3 against  5.1095e-3   (16 %)
  quad_k1_+-1e-12            d/dk1 3.6e-5 and 3.0e-5 off           (35 and 29 times the bound: sin(k l) / k beside 0)
  the Segment                d sigma_x / d k1 -6.0079e-5 against -6.3197e-5 (4.9 %)
and every other test of this module passed.
"""
import math

import numpy as np
import pytest
import torch

from tests import dkd_grad_ref as R

pytestmark = pytest.mark.gpu

F64 = {"dtype": torch.float64, "device": "cuda"}
KINDS = (R.DRIFT, R.QUAD, R.DIPOLE, R.TDC, R.SEXT, R.RF)


def backward(case, x, W, params=None, energy=None, dtype=torch.float64, param_shape=torch.Size(())):
    """(x_out, dx, dp, de) of the kernel for the loss (x_out * W).sum(); x (..., N, 7), params (Bp, P), energy () or (B,)."""
    import cheetah_amd  # noqa: F401
    from cheetah_amd import _ops

    t = lambda v: torch.tensor(np.asarray(v), dtype=dtype, device="cuda")  # noqa: E731
    xin = t(x).requires_grad_(True)
    p = t([case.params] if params is None else params).requires_grad_(True)
    e = t(case.energy if energy is None else energy).requires_grad_(True)
    out, _ = _ops.dkd_track(case.kind, xin, p, param_shape, e, case.mc2, case.nq, case.num_steps, case.fringe_at)
    assert out.dtype == dtype
    (out * t(W)).sum().backward()
    return out.detach(), xin.grad, p.grad, e.grad


def ratios(got, ref, u, floor):
    """(|got - ref| over the acceptance bound, |got - ref| / |ref|, u / |ref|), the largest entries; the relative figures over the
    entries that stand clear of the floor (|ref| > 100 floor: the rest is zero, or a residue that the floor is there for)."""
    got, ref, u = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(u, dtype=np.float64)
    err = np.abs(got - ref)
    bound = 2e-7 * np.abs(ref) + 4.0 * u + floor
    clear = np.abs(ref) > 100.0 * floor
    mag = np.where(clear, np.abs(ref), 1.0)
    return float(np.max(err / bound)), float(np.max(np.where(clear, err / mag, 0.0))), float(np.max(np.where(clear, u / mag, 0.0)))


def check_case(case):
    x, W = R.beam(case)
    ref = R.reference(case.name)
    out, dx, dp, de = backward(case, x, W)
    out = out.cpu().numpy()
    assert np.allclose(out, ref.out, rtol=1e-8, atol=1e-12 * np.abs(ref.out).max(axis=0)), case.name      # the same point
    dx, dp, de = dx.cpu().numpy(), dp.cpu().numpy()[0], float(de)
    assert np.all(np.isfinite(dx)) and np.all(np.isfinite(dp)) and math.isfinite(de), (case.name, dp, de)
    assert np.all(dx[:, 6] == 0.0)
    names = R.PNAMES[case.kind]
    worst = {}
    for k, key in enumerate(names):
        worst[key] = ratios(dp[k], ref.dp[k], ref.u_p[k], ref.floor_p[k])
    worst["energy"] = ratios(de, ref.de, ref.u_e, ref.floor_e)
    worst["dx"] = ratios(dx[:, :6], ref.dx, ref.u_x, ref.floor_x)
    print(f"\nGRAD {case.name} kind {case.kind}: " + " ".join(f"{k} {b:.2g}/{r:.1e}/{ur:.1e}" for k, (b, r, ur) in worst.items()))
    for key, (b, r, _) in worst.items():
        k = names.index(key) if key in names else None
        assert b <= 1.0, (case.name, key, "got", dp[k] if k is not None else (de if key == "energy" else "dx"),
                          "ref", ref.dp[k] if k is not None else (ref.de if key == "energy" else "dx"), "error over bound", b, "relative", r)


@pytest.mark.parametrize("name", [c.name for c in R.BRANCH_CASES])
def test_gradients_at_branch_points(name):
    """Parameters, energy and dx where a closed form of the map changes its branch or an operand is exactly zero. The k1 == 0 cases
    fail without the tangent of quad_coefficients' val(w) == 0 branch (d/dk1 keeps its a21 term only)."""
    check_case(R.CASES[name])


@pytest.mark.parametrize("N", R.TILE_SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_at_tile_edges(kind, N):
    """Every kind with one particle, one wave, one short of a tile, a tile, one more, and two tiles and one: the dead lanes of the
    last tile take part in the wave sum and must add nothing; `partials` is [B][ceil(N / 256)][P + 1]."""
    import cheetah_amd

    case = R.CASES[f"{R.KIND_NAME[kind]}_N{N}"]
    check_case(case)
    lib = cheetah_amd._lib.lib()
    for B in (1, 3):
        assert lib.chx_dkd_bwd_partials_count(kind, B, N) == B * ((N + 255) // 256) * (case.P + 1), (kind, B, N)


@pytest.mark.parametrize("kind", (R.QUAD, R.RF))
@pytest.mark.parametrize("Bx,Bp,Be", [(3, 1, 1), (1, 3, 1), (1, 1, 3), (3, 3, 1), (3, 1, 3), (1, 3, 3), (3, 3, 3)])
def test_broadcast_gradients_equal_separate_single_row_runs(kind, Bx, Bp, Be):
    """B = 3 with every combination of per-row and shared particles, parameters and energies: a per-row operand's gradient equals
    the single-row run's row by row, a shared one's is their sum (the row sums of DkdTrack.backward) — within 1e-13 of the summed
    magnitudes (relative to the entry for a per-row operand)."""
    case = R.CASES[f"{R.KIND_NAME[kind]}_N257"]
    rng = np.random.default_rng(7)
    xs = np.stack([R.beam(case)[0]] + [R.beam(R.Case("row", kind, case.params, N=case.N, seed=s))[0] for s in (11, 12)])
    Ws = rng.standard_normal((3, case.N, 7))
    ps = np.array(case.params)[None] * np.array([1.0, 1.1, 0.9])[:, None]
    es = case.energy * np.array([1.0, 1.2, 0.8])
    row = lambda a, B, b: a[b] if B == 3 else a[0]  # noqa: E731
    out, dx, dp, de = backward(case, xs if Bx == 3 else xs[0], Ws, ps if Bp == 3 else ps[:1], es if Be == 3 else es[0],
                               param_shape=torch.Size((3,)) if Bp == 3 else torch.Size(()))
    assert out.shape == (3, case.N, 7) and dx.shape == ((3, case.N, 7) if Bx == 3 else (case.N, 7))
    assert dp.shape == ((3, case.P) if Bp == 3 else (1, case.P)) and de.shape == ((3,) if Be == 3 else ())
    singles = []
    for b in range(3):
        o1, dx1, dp1, de1 = backward(case, row(xs, Bx, b), Ws[b], row(ps, Bp, b)[None], row(es, Be, b))
        assert torch.equal(o1, out[b])
        singles.append((dx1.cpu().numpy(), dp1.cpu().numpy()[0], float(de1)))

    def compare(got, parts, per_row, what):
        got = got.cpu().numpy()
        if per_row:
            for b in range(3):
                assert np.all(np.abs(got[b] - parts[b]) <= 1e-13 * np.abs(parts[b])), (what, b)
        else:
            got = got.reshape(np.shape(parts[0]))
            assert np.all(np.abs(got - sum(parts)) <= 1e-13 * sum(np.abs(v) for v in parts)), what

    compare(dx, [s[0] for s in singles], Bx == 3, "dx")
    compare(dp, [s[1] for s in singles], Bp == 3, "dp")
    compare(de, [np.float64(s[2]) for s in singles], Be == 3, "de")


@pytest.mark.parametrize("kind", KINDS)
def test_float32_beams_round_the_float64_gradients_once(kind):
    """The kernel evaluates in double whatever the storage dtype and rounds at the store: dx of a float32 beam is the float64 dx of
    the same (upcast) inputs within 2^-24 relative per entry, the parameter and energy gradients are the float64 sums rounded to
    float32, within 1 ulp. Derived, not measured."""
    case = R.CASES[f"{R.KIND_NAME[kind]}_N257"]
    x, W = R.beam(case)
    x32, W32 = x.astype(np.float32), W.astype(np.float32)
    p32, e32 = np.array([case.params], dtype=np.float32), np.float32(case.energy)
    out32, dx32, dp32, de32 = backward(case, x32, W32, p32, e32, dtype=torch.float32)
    out64, dx64, dp64, de64 = backward(case, x32.astype(np.float64), W32.astype(np.float64), p32.astype(np.float64), np.float64(e32))
    assert dx32.dtype == dp32.dtype == de32.dtype == torch.float32
    dx64 = dx64.cpu().numpy()
    tiny = float(np.finfo(np.float32).smallest_subnormal)
    assert np.all(np.abs(dx32.cpu().numpy().astype(np.float64) - dx64) <= 2.0 ** -24 * np.abs(dx64) + tiny)
    assert np.abs(dx64[:, :6]).max() > 0.0
    for got, want in ((dp32.cpu().numpy()[0], dp64.cpu().numpy()[0]), (de32.cpu().numpy().reshape(1), de64.cpu().numpy().reshape(1))):
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - want) <= ulp), (kind, got, want)


@pytest.mark.parametrize("kind", KINDS)
def test_backward_is_deterministic(kind):
    """include/chx.h promises a backward pass without atomics: the same inputs give the same bits."""
    case = R.CASES[f"{R.KIND_NAME[kind]}_N513"]
    x, W = R.beam(case)
    first, second = backward(case, x, W), backward(case, x, W)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_particle_leaves_the_other_rows_of_dx_alone(kind):
    case = R.CASES[f"{R.KIND_NAME[kind]}_N257"]
    x, W = R.beam(case)
    bad = x.copy()
    bad[100, :6] = np.nan
    clean, spoilt = backward(case, x, W)[1], backward(case, bad, W)[1]
    keep = torch.arange(case.N, device="cuda") != 100
    assert torch.equal(clean[keep], spoilt[keep]) and torch.isnan(spoilt[100, :6]).all()


def test_segment_whose_quadrupoles_start_at_k1_zero():
    """A drift-kick-drift lattice whose quadrupoles all stand at k1 = 0 exactly, the start of a tuning run: d sigma_x / d k1 is
    not zero and matches the reference chained element by element (the cotangent of sigma_x handed back through the elements'
    dx references; their own uncertainty, at most 1e-9 of the largest entry, is far below the 2e-7 of the acceptance)."""
    import cheetah_amd as ca

    t = lambda v: torch.tensor(v, **F64)  # noqa: E731
    lattice = [(R.DRIFT, (0.4,), 1), (R.QUAD, (0.2, 0.0, 0.0, 0.0, 0.0), 2), (R.DRIFT, (0.3,), 1),
               (R.QUAD, (0.15, 0.0, 0.0, 0.0, 0.0), 1), (R.DRIFT, (0.5,), 1)]
    x, _ = R.beam(R.Case("segment", R.DRIFT, (0.0,), seed=5))
    k1s, elements = [], []
    for kind, p, steps in lattice:
        if kind == R.DRIFT:
            elements.append(ca.Drift(length=t(p[0]), tracking_method="drift_kick_drift", **F64))
        else:
            k1s.append(torch.nn.Parameter(t(0.0)))
            elements.append(ca.Quadrupole(length=t(p[0]), k1=k1s[-1], tracking_method="drift_kick_drift", num_steps=steps, **F64))
    beam = ca.ParticleBeam(t(x), t(1e8), species=ca.Species("electron", **F64))
    sigma = ca.Segment(elements).track(beam).sigma_x
    sigma.backward()

    cases = [R.Case(f"segment_{i}", kind, p, num_steps=steps) for i, (kind, p, steps) in enumerate(lattice)]
    xs = [x]
    for c in cases:
        xs.append(R.forward(c, xs[-1], c.params, c.energy))
    xf = torch.from_numpy(xs[-1][:, 0].copy()).requires_grad_(True)
    sig_ref = torch.sqrt(((xf - xf.mean()) ** 2).sum() / (len(xf) - 1))
    sig_ref.backward()
    assert float(sigma.detach()) == pytest.approx(float(sig_ref.detach()), rel=1e-10)
    g = np.zeros_like(x)
    g[:, 0] = xf.grad.numpy()
    refs = []
    for c, xin in zip(reversed(cases), reversed(xs[:-1])):
        ref = R.reference_for(c, xin, g)
        assert ref.u_x.max() <= 1e-9 * np.abs(ref.dx).max()
        if c.kind == R.QUAD:
            refs.append((ref.dp[1], ref.u_p[1], ref.floor_p[1]))
        g = np.concatenate([ref.dx, np.zeros((len(x), 1))], axis=1)
    for k1, (want, u, floor) in zip(k1s, reversed(refs)):
        got = float(k1.grad)
        print(f"\nSEGMENT d sigma_x / d k1: got {got:.12e} ref {want:.12e} rel {abs(got - want) / abs(want):.1e}")
        assert got != 0.0 and want != 0.0
        assert abs(got - want) <= 2e-7 * abs(want) + 4.0 * u + floor, (got, want)
