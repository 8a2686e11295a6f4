"""Segment.ring_sensitivity and the `wrt` argument of one_turn_map, closed_orbit, ring_optics and chromaticity on the GPU
(chx_dkd_ring_sensitivity).

 1. every tangent against central differences of the calls WITHOUT `wrt` (the setting edited in place) at steps h and h / 2. Per
    tensor and knob the allowed error is 2 max|D(h) - D(h/2)| + 16 2^-52 max|value| / h: the differences' own truncation estimate and
    their rounding — the code under test takes no part in either. On the reference alone: the truncation estimate stays below
    1e-6 max|D|. Six (knob, field) pairs of ring A whose derivative is zero by symmetry (`ZERO_BY_SYMMETRY`) have no relative
    truncation to show: there the tangent itself is asserted to be zero to the rounding term.
    6-D (mode 2): the closed orbit carries the rounding of delta through the dispersion, not 2^-52 of the orbit as the rounding term
    assumes. Its rounding is MEASURED on the reference path alone (`reference_noise`: the largest change of each output when the
    guesses' delta moves by 1 or 2 units in the last place) and added: 2 noise / h to the rounding term, 6 noise / h to the cap.
 2. exact relations on the axis of ring A, 1e-6 of the largest entry (the bound of the corrector test of test_gpu_ring_optics.py):
    the closed-orbit response to an order-0 kick, the tune response to a thin order-1 kick.
 3. d M^T S M + M^T S d M = 0 to 1e-9 max|dM| max|M|.
 4. autograd through ring_optics(wrt=...) equals the contraction of the raw tangents through the same algebra, 1e-12 relative.
 5. Newton matching of the tunes and of the chromaticity from the tangents.
 6. bits: values with and without `wrt`, two calls, a pair alone and inside B = 9, K = 17, a captured graph after an edit.
 7. a lost seed is NaN in its own rows only.  8. no synchronisation, forward and backward.  9. a trainable ring is optimised.

Ring A: two FODO cells without bends — Quadrupole, three-step Sextupole, Drift —, thin order-0 and order-1 Multipoles at two places,
a Quadrupole of k1 = 0 and an order-3 Multipole of knl = 0, 19 items. Ring B: ring A with sector Dipoles in the drifts and an
RFCavity, taken at delta = 1e-3 with a corrector on (the sextupoles feed down); two of its knobs are a Dipole's angle and the
cavity's phase instead of two of the lengths. Ring C: one Drift, mode 0. B in {1, 9}, K in
{1, 3, 9, 17}: B K = 27 and 153 cross workgroup edges (8 pairs each) with a partly filled last wave."""
import functools
import math

import pytest
import torch

from tests.test_gpu_dkd_sextupole import S as SYMPLECTIC_S  # (the matrix diag(J2, J2, -J2) only)
from tests.test_gpu_no_sync import sync_warnings  # (helper only)
from tests.test_gpu_track_turns import same_bits  # (helper only)

pytestmark = pytest.mark.gpu

F64 = torch.float64
DKD = {"tracking_method": "drift_kick_drift"}
KW = {"dtype": F64, "device": "cuda"}
ENERGY = 1e8
TWO_PI = 2 * math.pi
EPS = 2.0 ** -52


def T(v):
    return torch.tensor(v, **KW)


class Ring:
    """A ring, its knobs [(name, tensor, index or None, step h)] and the deltas of its nine seeds."""

    # the steps of the differences per knob, ring A and ring B: the largest at which the differences' truncation estimate stays
    # under its cap — with bends the maps round at 1e-15 of a length, not of the orbit, and a smaller step only adds noise
    STEPS = {False: (1e-6, 5e-5, 5e-5, 2e-2, 2e-2, 2e-6, 2e-6, 2e-4, 5.0, 2.5e-5, 1e-4, 1e-4, 1e-6, 1e-6, 1e-5, 2.5e-5, 1e-5),
             True: (8e-6, 2e-4, 1e-4, 8e-2, 8e-2, 8e-6, 8e-6, 2e-4, 5.0, 5e-5, 4e-4, 1e-4, 4e-6, 1.6e-5, 1e-5, 5e-5, 1e-4)}

    def __init__(self, bends: bool, step_scale: float = 1.0, rf=(2e4, 8), corrector=2e-5):
        import cheetah_amd as ca

        self.kf, self.kd, self.k2f, self.k2d = T(3.0), T(-2.4), T(20.0), T(-30.0)       # (two tunes well apart)
        self.corr = [ca.Multipole(T(0.0), order=0, knl=T(corrector if bends else 0.0), ksl=T(0.0), name=f"corr{i}", **DKD, **KW) for i in range(2)]
        self.thin_quad = [ca.Multipole(T(0.0), order=1, knl=T(0.0), name=f"tq{i}", **DKD, **KW) for i in range(2)]
        self.quad0 = ca.Quadrupole(T(0.1), k1=T(0.0), name="quad0", **DKD, **KW)
        self.octu = ca.Multipole(T(0.1), order=3, knl=T(0.0), num_steps=2, name="oct", **DKD, **KW)
        self.sext, self.quads, self.drifts = [], [], []
        els = [self.corr[0]]
        for c in range(2):
            for k1, k2, tag in ((self.kf, self.k2f, "f"), (self.kd, self.k2d, "d")):
                q = ca.Quadrupole(T(0.2), k1=k1, tilt=T(0.0), misalignment=T([0.0, 0.0]), num_steps=1, name=f"q{tag}{c}", **DKD, **KW)
                s = ca.Sextupole(T(0.1), k2=k2, misalignment=T([0.0, 0.0]), num_steps=3, name=f"s{tag}{c}", **DKD, **KW)
                if bends:
                    d = ca.Dipole(T(0.9), angle=T(0.2), name=f"b{tag}{c}", **DKD, **KW)
                else:
                    d = ca.Drift(T(0.9), name=f"d{tag}{c}", **DKD, **KW)
                self.quads.append(q)
                self.sext.append(s)
                self.drifts.append(d)
                els += [q, s, d]
                if c == 0 and tag == "f":
                    els += [self.thin_quad[0], self.quad0]
                if c == 1 and tag == "f":
                    els += [self.corr[1], self.thin_quad[1], self.octu]
        self.last = ca.Drift(T(0.1), name="last", **DKD, **KW)
        els.append(self.last)
        if bends:
            # behind the first corrector: a 4-D orbit holds delta at the start, so what the cavity does to delta shows in the whole turn
            f = ca.RFCavity.harmonic_frequency(sum(float(e.length) for e in els) + 0.3, rf[1], T(ENERGY))
            self.rf = ca.RFCavity(T(0.3), voltage=T(rf[0]), phase=T(0.0), frequency=f, name="rf", **KW)
            els.insert(1, self.rf)
        self.segment = ca.Segment(els)
        self.items = els
        mis = self.sext[0].misalignment
        self.knobs = [
            ("corr0.knl (first item)", self.corr[0].knl, None, 1e-6), ("kf (shared)", self.kf, None, 2e-4), ("kd (shared)", self.kd, None, 2e-4),
            ("k2f (shared)", self.k2f, None, 2e-2), ("k2d (shared)", self.k2d, None, 2e-2), ("sf0.misalignment[0]", mis, 0, 2e-6),
            ("sf0.misalignment[1]", mis, 1, 2e-6), ("quad0.k1 = 0", self.quad0.k1, None, 2e-4), ("oct.knl = 0", self.octu.knl, None, 5.0),
            ("tq0.knl", self.thin_quad[0].knl, None, 1e-4), ("last.length (last item)", self.last.length, None, 1e-4),
            ("qf0.tilt", self.quads[0].tilt, None, 1e-4), ("corr0.ksl", self.corr[0].ksl, None, 1e-6), ("corr1.knl", self.corr[1].knl, None, 1e-6),
            ("qd0.length", self.quads[1].length, None, 1e-5), ("tq1.knl", self.thin_quad[1].knl, None, 1e-4),
            ("sd0.length", self.sext[1].length, None, 1e-5),
        ]
        if bends:                                                 # ring B: a Dipole's and the RFCavity's parameter for two of the lengths
            self.knobs[14] = ("bf0.angle", self.drifts[0].angle, None, 0.0)
            self.knobs[16] = ("rf.phase", self.rf.phase, None, 0.0)
        assert len(self.knobs) == 17
        self.knobs = [(n, t, i, h * step_scale) for (n, t, i, _), h in zip(self.knobs, self.STEPS[bends])]
        self.delta = torch.linspace(-2e-3, 2e-3, 9, **KW) + (1e-3 if bends else 0.0)

    def wrt(self, K=17):
        """The tensors of the first K knobs, each once (the two entries of a misalignment are one tensor)."""
        out = []
        for _, t, _, _ in self.knobs[:K]:
            if not any(t is u for u in out):
                out.append(t)
        return out


@functools.lru_cache(maxsize=None)
def ring(name):
    return Ring(bends=name == "B")


def knob_sets(r, K):
    """wrt for exactly K knobs: the first K of the list (K = 9 ends behind both entries of the misalignment)."""
    wrt = r.wrt(K)
    n = sum(max(t.numel(), 1) for t in wrt)
    assert n == K, (n, K)
    return wrt


def values_of(r, mode, B, ulps=0):
    """The outputs the tangents belong to, from the calls without `wrt`: a dict of tensors. `ulps`: delta moved by that many units
    in its last place (`reference_noise`)."""
    seg, delta = r.segment, r.delta[:B] if B > 1 else r.delta[4:5]
    for _ in range(abs(ulps)):
        delta = torch.nextafter(delta, torch.full_like(delta, math.copysign(1.0, ulps)))
    if mode == 0:
        x = torch.zeros(B, 6, **KW)
        x[:, 0], x[:, 2], x[:, 5] = 1e-3, -5e-4, delta
        m = seg.one_turn_map(x, T(ENERGY), along=True)
        return {"orbit": m.start[:, :6], "image": m.end[:, :6], "matrix": m.matrix, "orbit_along": m.orbit_along[..., :6], "matrix_along": m.matrix_along}
    opt = seg.ring_optics(T(ENERGY), delta=delta, longitudinal=mode == 2, num_iterations=12)
    m = seg.one_turn_map(opt.orbit, T(ENERGY), along=True)
    return {"orbit": opt.orbit[:, :6], "matrix": opt.matrix, "dispersion": opt.dispersion, "orbit_along": opt.orbit_along[..., :6],
            "matrix_along": m.matrix_along, "tunes": opt.tunes, "beta": opt.beta, "residual": opt.residual}


def tangents_of(r, mode, B, K=17):
    seg, delta = r.segment, r.delta[:B] if B > 1 else r.delta[4:5]
    wrt = knob_sets(r, K)
    if mode == 0:
        x = torch.zeros(B, 6, **KW)
        x[:, 0], x[:, 2], x[:, 5] = 1e-3, -5e-4, delta
        _, sens = seg._ring_jacobian("one_turn_map", T(ENERGY), None, x, 0, 1, True, wrt, True)
        return {"orbit": sens["d_orbit"], "image": sens["d_image"], "matrix": sens["d_matrix"], "orbit_along": sens["d_orbit_along"],
                "matrix_along": sens["d_matrix_along"]}
    s = seg.ring_sensitivity(T(ENERGY), wrt, delta=delta, longitudinal=mode == 2, num_iterations=12)
    return {"orbit": s.d_orbit, "matrix": s.d_matrix, "dispersion": s.d_dispersion, "orbit_along": s.d_orbit_along, "matrix_along": s.d_matrix_along,
            "tunes": s.d_tunes, "beta": s.d_beta, "closed": s.closed, "sens": s}


@functools.lru_cache(maxsize=None)
def differences(name, mode, B):
    """`differences_of` the shared ring `name`. Computed once, read-only."""
    return differences_of(ring(name), mode, B)


def differences_of(r, mode, B):
    """Per knob: {field: (D(h/2), D(h), max|value|, h)} from central differences of the calls without `wrt`."""
    out = []
    for _, t, index, h in r.knobs:
        entry = t if index is None else t[index]
        keep = entry.clone()
        D, size = {}, {}
        for step in (h, h / 2):
            entry.copy_(keep + step)
            plus = values_of(r, mode, B)
            entry.copy_(keep - step)
            minus = values_of(r, mode, B)
            entry.copy_(keep)
            D[step] = {f: (plus[f] - minus[f]) / (2 * step) for f in plus}
            size = {f: max(size.get(f, 0.0), float(plus[f].abs().max()), float(minus[f].abs().max())) for f in plus}
        base = values_of(r, mode, B)
        # max|value|: over the values the differences are made of (a value that is 0 on the axis is not 0 beside it)
        out.append({f: (D[h / 2][f], D[h][f], max(float(base[f].abs().max()), size[f]), h) for f in base if f != "residual"})
    return out


@functools.lru_cache(maxsize=None)
def reference_noise(name, mode, B):
    """{field: the largest change of the calls' values WITHOUT `wrt` when delta moves by 1 or 2 units in its last place, either way} —
    the rounding of the reference path measured on itself. (Such a move changes a smooth result by parts in 1e16; what is seen
    beyond that is rounding that another path through the arithmetic rearranges, as another setting does.)"""
    return noise_of(ring(name), mode, B)


def noise_of(r, mode, B):
    base = values_of(r, mode, B)
    noise = {f: 0.0 for f in base}
    for ulps in (-2, -1, 1, 2):
        moved = values_of(r, mode, B, ulps)
        noise = {f: max(noise[f], float((moved[f] - base[f]).abs().max())) for f in base}
    return noise


# Derivatives that are zero by symmetry although the values move beside the axis: (ring, mode, knob, field). The central difference of an
# even function is rounding over h and has no relative truncation to show; the tangent itself is asserted to be zero to rounding.
# Ring A's closed orbit (mode 1; the seeds of mode 0 are off the axis), a misaligned Sextupole around an orbit on the axis: its kick is k2 (x - x0)^2 / 2, even in the offset, so the orbit, its
# dispersion and the orbit along the ring move with the square of the offset (the matrices move linearly and are compared).
ZERO_BY_SYMMETRY = {("A", 1, f"sf0.misalignment[{i}]", f) for i in (0, 1) for f in ("orbit", "dispersion", "orbit_along")}


def check_against_differences(name, mode, B, K):
    r = ring(name)
    got = tangents_of(r, mode, B, K)
    ref = differences(name, mode, B)
    # (6-D: one closed orbit whatever the guess — the nine guesses, each moved four times, are 36 paths to the same fixed point)
    noise = reference_noise(name, mode, 9) if mode == 2 else {}
    worst = {}
    for k in range(K):
        for f, (fine, coarse, size, h) in ref[k].items():
            truncation = 2 * float((coarse - fine).abs().max())
            # 6-D: the measured rounding of the reference (`reference_noise`) on top of the bound's own term — D(h/2) = (v+ - v-) / h is
            # off by 2 noise / h, the truncation estimate 2 |D(h) - D(h/2)| by 2 (1 + 2) noise / h
            measured = noise.get(f, 0.0) / h
            rounding = 16 * EPS * size / h + 2 * measured
            scale = float(fine.abs().max())
            if (name, mode, r.knobs[k][0], f) in ZERO_BY_SYMMETRY:
                assert float(got[f][:, k].abs().max()) <= rounding, (name, r.knobs[k][0], f, float(got[f][:, k].abs().max()), rounding)
                continue
            assert math.isfinite(truncation) and truncation <= 1e-6 * scale + 6 * measured, \
                f"the reference of {r.knobs[k][0]} / {f} is too coarse: truncation {truncation:.3g} of {scale:.3g} (rounding {rounding:.3g})"
            err = float((got[f][:, k] - fine).abs().max())
            bound = truncation + rounding
            ratio = err / bound if bound > 0 else (0.0 if err == 0 else math.inf)
            if ratio > worst.get(f, (0.0,))[0]:
                worst[f] = (ratio, r.knobs[k][0], err, bound)
            assert err <= bound, f"ring {name} mode {mode} B {B} knob {r.knobs[k][0]} {f}: error {err:.3g} > {bound:.3g} (truncation {truncation:.3g})"
    print(f"ring {name} mode {mode} B {B} K {K}: largest error / bound per tensor", {f: (round(v[0], 4), v[1]) for f, v in worst.items()})


# ---- 1. differences ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,B,K", [("A", 1, 9, 17), ("A", 1, 1, 1), ("A", 1, 9, 3), ("A", 0, 9, 17), ("A", 0, 1, 9), ("B", 1, 9, 17),
                                           ("B", 2, 1, 17), ("B", 0, 1, 3), ("B", 2, 9, 1)])
def test_tangents_match_differences_of_the_calls_without_wrt(name, mode, B, K):
    check_against_differences(name, mode, B, K)


def test_single_drift_in_mode_0():
    import cheetah_amd as ca

    d = ca.Drift(T(0.7), **DKD, **KW)
    seg = ca.Segment([d])
    x = torch.zeros(9, 6, **KW)
    x[:, 1], x[:, 3], x[:, 5] = torch.linspace(-1e-3, 1e-3, 9, **KW), 2e-4, 1e-3
    _, sens = seg._ring_jacobian("one_turn_map", T(ENERGY), None, x, 0, 1, True, [d.length], True)
    assert sens["d_image"].shape == (9, 1, 6) and sens["d_matrix_along"].shape == (9, 1, 2, 6, 6)
    h = 1e-3

    def image(length):
        d.length.copy_(T(length))
        m = seg.one_turn_map(x, T(ENERGY))
        return m.end[:, :6], m.matrix

    (fp, Mp), (fm, Mm), (fp2, Mp2), (fm2, Mm2) = image(0.7 + h), image(0.7 - h), image(0.7 + h / 2), image(0.7 - h / 2)
    d.length.copy_(T(0.7))
    for got, fine, coarse, size in ((sens["d_image"][:, 0], (fp2 - fm2) / h, (fp - fm) / (2 * h), float(fp.abs().max())),
                                    (sens["d_matrix"][:, 0], (Mp2 - Mm2) / h, (Mp - Mm) / (2 * h), float(Mp.abs().max()))):
        truncation, rounding = 2 * float((coarse - fine).abs().max()), 16 * EPS * size / h
        assert truncation <= 1e-6 * float(fine.abs().max())
        assert float((got - fine).abs().max()) <= truncation + rounding
    # a drift is linear in its length: d x / d L = px / pz, the slope, and d M[0, 1] / d L = 1 / pz + px^2 / pz^3
    assert float((sens["d_image"][:, 0, 0] - (fp[:, 0] - x[:, 0]) / (0.7 + h)).abs().max()) <= 1e-15
    assert torch.all(sens["d_orbit"] == 0) and same_bits(sens["d_orbit_along"][:, 0, 1], sens["d_image"][:, 0])


# ---- 2. exact relations ------------------------------------------------------------------------------------------------------------------
def test_orbit_and_tune_response_formulas_on_the_axis():
    r = ring("A")
    seg = r.segment
    opt = seg.ring_optics(T(ENERGY))
    s = seg.ring_sensitivity(T(ENERGY), [r.corr[0].knl, r.corr[0].ksl, r.corr[1].knl, r.thin_quad[0].knl, r.thin_quad[1].knl])
    beta, phi = opt.beta[0], opt.phase_advance[0]                       # (E + 1, 2)
    Q = phi[-1] / TWO_PI
    worst = 0.0
    for knob, item, plane in ((0, r.items.index(r.corr[0]), 0), (1, r.items.index(r.corr[0]), 1), (2, r.items.index(r.corr[1]), 0)):
        # a thin kick sits between record `item` and `item + 1` with the same beta and phase on both sides; d px = -knl, d py = +ksl
        j = item + 1
        sign = -1.0 if plane == 0 else 1.0
        want = sign * torch.sqrt(beta[:, plane] * beta[j, plane]) * torch.cos((phi[:, plane] - phi[j, plane]).abs() - math.pi * Q[plane]) \
            / (2 * torch.sin(math.pi * Q[plane]))
        got = s.d_orbit_along[0, knob, :, 2 * plane]
        # behind the kick only: record `item` itself lies in front of the kick in the turn that starts at s = 0 but sees the kick of
        # the turn before — the formula holds at every record, the start included
        err = float((got - want).abs().max()) / float(want.abs().max())
        worst = max(worst, err)
        assert err <= 1e-6, (knob, err)
    for knob, el in ((3, r.thin_quad[0]), (4, r.thin_quad[1])):
        j = r.items.index(el) + 1
        want = torch.stack([beta[j, 0], -beta[j, 1]]) / (4 * math.pi)
        err = float((s.d_tunes[0, knob] - want).abs().max()) / float(want.abs().max())
        worst = max(worst, err)
        assert err <= 1e-6, (knob, err, s.d_tunes[0, knob], want)
    print("response formulas: largest relative error", worst)


# ---- 3. symplectic tangent ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("A", 1), ("B", 1), ("B", 2), ("A", 0)])
def test_the_tangent_of_the_matrix_is_symplectic(name, mode):
    r = ring(name)
    got = tangents_of(r, mode, 9)
    M = values_of(r, mode, 9)["matrix"]
    Sm = torch.as_tensor(SYMPLECTIC_S, **KW)
    dM = got["matrix"]
    defect = dM.transpose(-1, -2) @ Sm @ M[:, None] + M[:, None].transpose(-1, -2) @ Sm @ dM
    scale = dM.abs().amax((-2, -1)) * M.abs().amax((-2, -1))[:, None]
    ratios = (defect.abs().amax((-2, -1)) / (1e-9 * scale).clamp_min(1e-300)).amax(0)
    keep = torch.ones(17, dtype=torch.bool, device="cuda")
    if (name, mode) == ("B", 2):
        # the cavity's phase moves the 6-D orbit along tau and leaves its matrix: d M = 0, and a bound relative to max|dM| has
        # nothing to hold on to. The tangent is asserted to be zero to rounding instead (16 2^-52 of the matrix, its 20 items).
        k = [n for n, *_ in r.knobs].index("rf.phase")
        keep[k] = False
        assert float(dM[:, k].abs().max()) <= 20 * 16 * EPS * float(M.abs().max()), float(dM[:, k].abs().max())
    print(f"ring {name} mode {mode}: symplectic defect / bound per knob", [round(float(v), 9) for v in ratios])
    assert torch.all(ratios[keep] <= 1.0)
    assert float(dM.abs().max()) > 0.1


# ---- 4. autograd -------------------------------------------------------------------------------------------------------------------------
def trainable_copy(name):
    """A fresh ring whose knob tensors require grad."""
    r = Ring(bends=name != "A")
    for t in r.wrt():
        t.requires_grad_(True)
    return r


@pytest.mark.parametrize("name", ["A", "B"])
def test_autograd_equals_the_contraction_of_the_tangents(name):
    from cheetah_amd.particles.optics import ring_optics_from, ClosedOrbit

    r = trainable_copy(name)
    wrt = r.wrt()
    opt = r.segment.ring_optics(T(ENERGY), delta=r.delta, wrt=wrt)
    fields = ("orbit", "matrix", "beta", "alpha", "phase_advance", "dispersion_along", "tunes")
    g = torch.Generator().manual_seed(3)
    weights = {f: torch.randn(getattr(opt, f).shape, generator=g, dtype=F64).cuda() for f in fields}
    loss = sum((weights[f] * getattr(opt, f)).sum() for f in fields)
    grads = torch.autograd.grad(loss, wrt)
    assert all(torch.isfinite(x).all() for x in grads)
    flat = torch.cat([x.reshape(-1) for x in grads])
    s = r.segment.ring_sensitivity(T(ENERGY), wrt, delta=r.delta)
    m_along = r.segment.one_turn_map(s.closed.orbit, T(ENERGY), along=True, wrt=wrt)

    def algebra(orbit, matrix, dispersion, orbit_along, matrix_along):
        o = ring_optics_from(ClosedOrbit(orbit, opt.residual.detach(), matrix, dispersion), orbit_along, matrix_along, None)
        return torch.stack([(weights[f] * getattr(o, f)).sum() for f in fields])          # (one term of the loss per field)

    base = (s.closed.orbit, s.closed.matrix, s.closed.dispersion, m_along.orbit_along.detach(), m_along.matrix_along.detach())
    pad = lambda x: torch.cat([x, torch.zeros_like(x[..., :1])], -1)  # noqa: E731  (the seventh column is the constant 1)
    want = []
    for k in range(17):
        tang = (pad(s.d_orbit[:, k]), s.d_matrix[:, k], s.d_dispersion[:, k], pad(s.d_orbit_along[:, k]), s.d_matrix_along[:, k])
        want.append(torch.func.jvp(algebra, base, tang)[1])
    terms = torch.stack(want)                                              # (knob, field)
    want, scale = terms.sum(-1), terms.abs().sum(-1)                       # relative to the terms a gradient is the sum of
    err = float(((flat - want).abs() / scale.clamp_min(1e-300)).max())
    print(f"ring {name}: autograd against the tangents, largest relative difference", err, "gradients", flat.tolist())
    assert float(scale.max()) > 0 and torch.all((flat - want).abs() <= 1e-12 * scale)


def test_chromaticity_gradient_matches_differences():
    r = Ring(bends=True)
    r.k2f.requires_grad_(True), r.k2d.requires_grad_(True)
    xi = r.segment.chromaticity(T(ENERGY), wrt=[r.k2f, r.k2d])
    J = torch.stack([torch.stack(torch.autograd.grad(xi[p], [r.k2f, r.k2d], retain_graph=True)) for p in range(2)])     # (plane, family)
    plain = ring("B")
    for c, (t, h) in enumerate(((plain.k2f, 8e-2), (plain.k2d, 8e-2))):
        keep = t.clone()
        D = {}
        for step in (h, h / 2):
            t.copy_(keep + step)
            plus = plain.segment.chromaticity(T(ENERGY))
            t.copy_(keep - step)
            minus = plain.segment.chromaticity(T(ENERGY))
            t.copy_(keep)
            D[step] = (plus - minus) / (2 * step)
        size = float(plain.segment.chromaticity(T(ENERGY)).abs().max())
        truncation, rounding = 2 * float((D[h] - D[h / 2]).abs().max()), 16 * EPS * size / h
        assert truncation <= 1e-6 * float(D[h / 2].abs().max())
        err = float((J[:, c] - D[h / 2]).abs().max())
        print("chromaticity gradient: family", c, "error", err, "bound", truncation + rounding)
        assert err <= truncation + rounding
    assert same_bits(xi.detach(), plain.segment.chromaticity(T(ENERGY)))


# ---- 5. use ------------------------------------------------------------------------------------------------------------------------------
def test_newton_matching_of_tunes_and_chromaticity():
    r = Ring(bends=False)
    seg = r.segment
    target = seg.ring_optics(T(ENERGY)).tunes[0] + T([0.01, -0.01])
    for step in range(6):
        s = seg.ring_sensitivity(T(ENERGY), [r.kf, r.kd], along=False)
        miss = seg.ring_optics(T(ENERGY)).tunes[0] - target
        print("tune matching step", step, "miss", miss.tolist())
        if float(miss.abs().max()) <= 1e-8:
            break
        dk = torch.linalg.solve(s.d_tunes[0].T, -miss)
        r.kf += dk[0]
        r.kd += dk[1]
    assert step <= 5 and float(miss.abs().max()) <= 1e-8
    r = Ring(bends=True)
    r.k2f.requires_grad_(True), r.k2d.requires_grad_(True)
    seg = r.segment
    target = seg.chromaticity(T(ENERGY), wrt=[r.k2f, r.k2d]).detach() + T([0.01, -0.01])
    for step in range(6):
        xi = seg.chromaticity(T(ENERGY), wrt=[r.k2f, r.k2d])
        miss = xi.detach() - target
        print("chromaticity matching step", step, "miss", miss.tolist())
        if float(miss.abs().max()) <= 1e-8:
            break
        J = torch.stack([torch.stack(torch.autograd.grad(xi[p], [r.k2f, r.k2d], retain_graph=True)) for p in range(2)])
        dk = torch.linalg.solve(J, -miss)
        with torch.no_grad():
            r.k2f += dk[0]
            r.k2d += dk[1]
    assert step <= 5 and float(miss.abs().max()) <= 1e-8


# ---- 6. bits -----------------------------------------------------------------------------------------------------------------------------
OPTICS_FIELDS = ("orbit", "residual", "matrix", "dispersion", "tunes", "beta", "alpha", "phase_advance", "slip", "dispersion_along", "orbit_along")
TANGENT_FIELDS = ("d_orbit", "d_matrix", "d_dispersion", "d_orbit_along", "d_matrix_along", "d_tunes", "d_beta")


def test_values_with_wrt_are_the_values_without_and_two_calls_agree():
    plain = ring("B").segment.ring_optics(T(ENERGY), delta=ring("B").delta)
    r = trainable_copy("B")                                        # the same settings, those of the knobs trainable
    seg, wrt = r.segment, r.wrt()
    with_wrt = seg.ring_optics(T(ENERGY), delta=r.delta, wrt=wrt)
    assert with_wrt.tunes.requires_grad and with_wrt.residual.requires_grad and with_wrt.dispersion.requires_grad
    for f in OPTICS_FIELDS:
        assert same_bits(getattr(with_wrt, f).detach(), getattr(plain, f)), f
    x = torch.zeros(9, 6, **KW)
    x[:, 0] = 1e-3
    a, b = ring("B").segment.one_turn_map(x, T(ENERGY), along=True), seg.one_turn_map(x, T(ENERGY), along=True, wrt=wrt)
    assert b.end.requires_grad and same_bits(a.end, b.end.detach()) and same_bits(a.matrix_along, b.matrix_along.detach())
    co = seg.closed_orbit(T(ENERGY), delta=r.delta, wrt=wrt)
    assert co.orbit.requires_grad and same_bits(co.orbit.detach(), plain.orbit)
    s1 = seg.ring_sensitivity(T(ENERGY), wrt, delta=r.delta)
    s2 = seg.ring_sensitivity(T(ENERGY), wrt, delta=r.delta)
    for f in TANGENT_FIELDS:
        assert same_bits(getattr(s1, f), getattr(s2, f)), f
    assert same_bits(s1.closed.orbit, plain.orbit) and same_bits(s1.closed.matrix, plain.matrix)


@pytest.mark.parametrize("name", ["A", "B"])
def test_a_pair_alone_equals_the_pair_inside_the_batch(name):
    r = ring(name)
    seg = r.segment
    full = seg.ring_sensitivity(T(ENERGY), r.wrt(), delta=r.delta)
    for b, k in ((0, 0), (8, 16), (4, 5), (3, 8)):
        t = r.knobs[k][1]
        alone = seg.ring_sensitivity(T(ENERGY), [t], delta=r.delta[b:b + 1])
        col = r.knobs[k][2] or 0
        for f in TANGENT_FIELDS:
            assert same_bits(getattr(alone, f)[0, col], getattr(full, f)[b, k]), (b, k, f)


def test_more_pairs_than_one_prepare_launch_takes():
    """129 (knob, item) pairs — the tangents of the constants are prepared 128 pairs a launch, so the last pair goes in a second one:
    3 knobs (the length, the strength and the tilt all 43 Quadrupoles of a ring share; each item has a misalignment of its own, so
    the closed orbit is off the axis and moves with every knob), B = 1, the 4-D closed orbit. Every row equals, bit for bit, the
    row of the call with that knob alone (43 pairs, one launch)."""
    import cheetah_amd as ca

    length, k1, tilt = T(0.1), T(0.5), T(0.1)
    seg = ca.Segment([ca.Quadrupole(length, k1=k1, tilt=tilt, misalignment=T([1e-4 * (i % 3 - 1), 5e-5 * (i % 5 - 2)]), num_steps=1 + i % 2,
                                    name=f"q{i}", **DKD, **KW) for i in range(43)])
    fields = ("d_orbit", "d_image", "d_matrix", "d_dispersion")

    def raw(wrt):
        return seg._closed_orbit("ring_sensitivity", T(ENERGY), None, T([1e-3]), None, False, 10, False, wrt, True)[1]

    full = raw([length, k1, tilt])
    for f in fields:
        assert full[f].shape[:2] == (1, 3) and torch.isfinite(full[f]).all() and bool((full[f][0] != 0).flatten(1).any(dim=1).all()), f
    for k, t in enumerate((length, k1, tilt)):
        alone = raw([t])
        for f in fields:
            assert same_bits(alone[f][0, 0], full[f][0, k]), (k, f)


def test_a_captured_graph_replays_after_an_edit():
    import cheetah_amd as ca

    r = Ring(bends=True)
    seg, wrt, energy, delta = r.segment, r.wrt(), T(ENERGY), r.delta.clone()
    before = seg.ring_sensitivity(energy, wrt, delta=delta)
    step = ca.graph.capture(lambda: seg.ring_sensitivity(energy, wrt, delta=delta))
    first = step()
    for f in TANGENT_FIELDS:
        assert same_bits(getattr(first, f), getattr(before, f)), f
    r.kf.copy_(T(3.05))
    replayed = step()
    fresh = seg.ring_sensitivity(T(ENERGY), wrt, delta=r.delta.clone())
    assert not same_bits(fresh.d_matrix, before.d_matrix)
    for f in TANGENT_FIELDS:
        assert same_bits(getattr(replayed, f), getattr(fresh, f)), f


# ---- 7. isolation ------------------------------------------------------------------------------------------------------------------------
def test_a_lost_seed_is_nan_in_its_own_rows_only():
    r = ring("A")
    seg, wrt = r.segment, r.wrt()
    guess = torch.zeros(9, 6, **KW)
    clean = seg.ring_sensitivity(T(ENERGY), wrt, delta=r.delta, guess=guess, num_iterations=6)
    bad = guess.clone()
    bad[5, 1] = 1.5                                              # px > 1 + delta: the first drift's square root is negative
    s = seg.ring_sensitivity(T(ENERGY), wrt, delta=r.delta, guess=bad, num_iterations=6)
    keep = torch.arange(9, device="cuda") != 5
    assert torch.isnan(s.closed.orbit[5, :6]).all()
    for f in TANGENT_FIELDS:
        a, b = getattr(s, f), getattr(clean, f)
        assert same_bits(a[keep], b[keep]), f
        assert torch.isnan(a[5]).all(), f
        assert torch.isfinite(a[keep]).all(), f
    x = torch.zeros(9, 6, **KW)
    x[5, 1] = 1.5
    _, sens = seg._ring_jacobian("one_turn_map", T(ENERGY), None, x, 0, 1, True, wrt, True)
    for f, a in sens.items():
        assert torch.isnan(a[5]).all() and torch.isfinite(a[keep]).all(), f


# ---- 8. no synchronisation ---------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_do_not_synchronise():
    r = trainable_copy("B")
    seg, wrt, energy, delta = r.segment, r.wrt(), T(ENERGY), r.delta.clone()
    assert len(sync_warnings(lambda: torch.tensor(1.0, device="cuda"), warm=0)) == 1          # the switch sees what it should see
    assert sync_warnings(lambda: seg.ring_sensitivity(energy, wrt, delta=delta)) == []
    assert sync_warnings(lambda: seg.ring_optics(energy, delta=delta, wrt=wrt)) == []

    def both():
        opt = seg.ring_optics(energy, delta=delta, wrt=wrt)
        (opt.tunes.sum() + opt.beta.sum() + opt.orbit.sum()).backward()

    assert sync_warnings(both) == []
    opt = seg.ring_optics(energy, delta=delta, wrt=wrt)
    loss = opt.tunes.sum() + opt.dispersion_along.sum()
    assert sync_warnings(lambda: loss.backward(retain_graph=True)) == []


# ---- 9. a trainable ring -----------------------------------------------------------------------------------------------------------------
def test_a_trainable_ring_is_optimised_with_wrt_all():
    r = Ring(bends=False)
    r.kf.requires_grad_(True)
    r.kd.requires_grad_(True)
    seg = r.segment
    with pytest.raises(ValueError, match="requires grad"):
        seg.ring_optics(T(ENERGY))
    with pytest.raises(ValueError, match="requires grad"):
        seg.ring_optics(T(ENERGY), wrt=[r.kf])                   # kd requires grad and is not named
    opt0 = seg.ring_optics(T(ENERGY), wrt="all")
    target = opt0.tunes[0].detach() + T([0.01, -0.01])
    optimiser = torch.optim.SGD([r.kf, r.kd], lr=5.0)
    losses = []
    for _ in range(5):
        optimiser.zero_grad()
        loss = ((seg.ring_optics(T(ENERGY), wrt="all").tunes[0] - target) ** 2).sum()
        loss.backward()
        assert torch.isfinite(r.kf.grad) and torch.isfinite(r.kd.grad) and float(r.kf.grad) != 0
        optimiser.step()
        losses.append(float(loss))
    print("SGD losses", losses)
    assert losses[-1] < losses[0]
