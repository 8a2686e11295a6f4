"""The gradient reference of the drift-kick-drift edge tests (tests/dkd_grad_ref.py) checked on its own, without a GPU: it
reproduces the reference's stored autograd gradients, its own uncertainty stays under a cap for every case that
tests/test_gpu_dkd_grad_edges.py compares the kernel with, it is continuous across the branch points where that autograd returns
NaN, and the beams of the table reach the branches they are meant to reach."""
import ast
import dataclasses

import numpy as np
import pytest

from tests import dkd_grad_ref as R

GOLDEN_NAMES = ["dkd_drift", "dkd_drift_lowE", "dkd_quad", "dkd_quad_defocus", "dkd_dipole", "dkd_dipole_entrance", "dkd_tdc"]
GOLDEN_KIND = {"Drift": R.DRIFT, "Quadrupole": R.QUAD, "Dipole": R.DIPOLE, "TransverseDeflectingCavity": R.TDC}
# the stored names of the kernel's parameters, in the kernel's order
GOLDEN_KEYS = {
    R.DRIFT: ("length",),
    R.QUAD: ("length", "k1", "tilt", "misalignment", "misalignment"),
    R.DIPOLE: ("length", "angle", "dipole_e1", "dipole_e2", "tilt", "fringe_integral", "fringe_integral_exit", "gap", "gap_exit"),
    R.TDC: ("length", "voltage", "phase", "frequency", "tilt", "misalignment", "misalignment"),
}
# The Richardson value's own error falls with h^4 and with the oracle's rounding over h; u (what the cap is about) falls with h^2
# only. Where the rounding is what is left at the table's steps (the dipole's small gradients) the comparison with the stored
# values takes a larger step: the method is what is pinned here.
GOLDEN_HREL = {R.DIPOLE: (("e1", 3e-2), ("tilt", 2e-2), ("fint", 0.3), ("gap", 0.3))}


def golden_case(g, name):
    kind = GOLDEN_KIND[str(g[f"{name}__class"])]
    opts = ast.literal_eval(str(g[f"{name}__opts"]))
    stored = [str(p) for p in g[f"{name}__pnames"]]
    keys = GOLDEN_KEYS[kind]

    def entry(prefix, i):
        v = g[f"{name}__{prefix}__{keys[i]}"]
        return float(v[i - (len(keys) - 2)]) if keys[i] == "misalignment" else float(v)

    params = tuple(entry("p", i) if k in stored else 0.0 for i, k in enumerate(keys))
    grads = [entry("g", i) if k in stored else None for i, k in enumerate(keys)]
    fringe = {"neither": 0, "entrance": 1, "exit": 2, "both": 3}[opts.get("fringe_at", "both")]
    case = R.Case(name, kind, params, num_steps=opts.get("num_steps", 1), fringe_at=fringe, energy=float(g[f"{name}__energy"]),
                  N=g["x"].shape[0], hrel=GOLDEN_HREL.get(kind, ()))
    return case, grads


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_reference_reproduces_the_stored_autograd_gradients(golden, name):
    """Every parameter, the energy and dx[:, :6] of the seven drift-kick-drift cases of nonlinear_grad.npz within 1e-8 relative
    (measured: parameters <= 9.9e-10, the dipole's angle; energy <= 3.1e-9; dx <= 7.5e-10 of the column's largest entry)."""
    g = golden("nonlinear_grad.npz")
    case, grads = golden_case(g, name)
    ref = R.reference_for(case, g["x"], g["W"])
    assert np.allclose(ref.out, g[f"{name}__out"], rtol=1e-12, atol=1e-15)      # the oracle's forward pass is the stored one
    for k, want in enumerate(grads):
        if want is not None:
            print(f"{name} {R.PNAMES[case.kind][k]}: ref {ref.dp[k]:.12e} stored {want:.12e} rel {abs(ref.dp[k] - want) / max(abs(want), 1e-300):.1e}")
            assert abs(ref.dp[k] - want) <= 1e-8 * abs(want), (name, R.PNAMES[case.kind][k], ref.dp[k], want)
    # the stored loss has the term 1e-9 * ref_energy_out, whose derivative is 1e-9 (bmadx.py:49)
    ge = float(g[f"{name}__g_energy"])
    print(f"{name} energy: ref {ref.de + 1e-9:.12e} stored {ge:.12e}")
    assert abs(ref.de + 1e-9 - ge) <= 1e-8 * abs(ge), (name, ref.de, ge)
    # dx: relative to the entry, with the rounding of the difference quotient (1e-9 of the column's largest entry) beside it
    want = g[f"{name}__dx"][:, :6]
    err = np.abs(ref.dx - want)
    print(f"{name} dx: {(err / np.abs(want).max(axis=0)).max():.1e} of the column's largest entry")
    assert np.all(err <= 1e-8 * np.abs(want) + 1e-9 * np.abs(want).max(axis=0)), name


@pytest.mark.parametrize("name", list(R.CASES))
def test_uncertainty_stays_under_the_cap(name):
    """u <= 5e-8 |ref| + floor for every gradient of every case of the GPU table (largest measured: 0.42 of the cap, the angle of
    the one-particle dipole)."""
    ref = R.reference(name)
    assert np.all(np.isfinite(ref.dp)) and np.isfinite(ref.de) and np.all(np.isfinite(ref.dx))
    cap_p = 5e-8 * np.abs(ref.dp) + ref.floor_p
    cap_x = 5e-8 * np.abs(ref.dx) + ref.floor_x
    assert np.all(ref.u_p <= cap_p), (name, ref.u_p / cap_p)
    assert ref.u_e <= 5e-8 * abs(ref.de) + ref.floor_e, (name, ref.u_e, ref.de, ref.floor_e)
    assert np.all(ref.u_x <= cap_x), (name, (ref.u_x / cap_x).max(axis=0))


def _branch_neighbours(case, key, values):
    k = R.PNAMES[case.kind].index(key)
    out = []
    for v in values:
        p = list(case.params)
        p[k] = v
        c = dataclasses.replace(case, params=tuple(p))
        out.append(R.reference_for(c, *R.beam(c)))
    return k, out


@pytest.mark.parametrize("name,key", [("quad_k1_0_n1", "k1"), ("quad_k1_0_n3", "k1"), ("quad_k1_0_tilt_misaligned", "k1"),
                                      ("dipole_angle_0", "angle")])
def test_reference_is_continuous_across_the_branch_point(name, key):
    """The gradient with respect to the strength at 0 equals the one at +-1e-6 within 1e-6 relative: the closed forms change
    their branch there (the reference's autograd returns NaN at k1 == 0), the map does not."""
    case = R.CASES[name]
    at0 = R.reference(name)
    k, (minus, plus) = _branch_neighbours(case, key, (-1e-6, 1e-6))
    for other in (minus, plus):
        print(f"{name} d/d{key}: {at0.dp[k]:.12e} at 0, {other.dp[k]:.12e} beside it")
        assert at0.dp[k] != 0.0 and abs(other.dp[k] - at0.dp[k]) <= 1e-6 * abs(at0.dp[k])
    # every other gradient changes with the strength (a mixed second derivative, 2e-6 of the length's), smoothly: the mean of both
    # sides is the value at 0 up to second order
    mean = lambda a, b: 0.5 * (a + b)  # noqa: E731
    assert np.all(np.abs(mean(minus.dp, plus.dp) - at0.dp) <= 1e-7 * np.abs(at0.dp) + at0.floor_p)
    assert abs(mean(minus.de, plus.de) - at0.de) <= 1e-7 * abs(at0.de) + at0.floor_e
    assert np.all(np.abs(mean(minus.dx, plus.dx) - at0.dx) <= 1e-7 * np.abs(at0.dx) + at0.floor_x)


def test_k1_zero_gradient_is_the_one_the_issue_was_opened_with(golden):
    """x and W of nonlinear_grad.npz, L = 0.3, one step, 1e8 eV: d/dk1 at k1 = 0 is -1.7236355e-3; the a21 term alone, which is
    what the kernel kept before its val(w) == 0 branch carried a tangent, gives -1.6471e-3 (4.4 % off)."""
    g = golden("nonlinear_grad.npz")
    case = R.Case("issue", R.QUAD, (0.3, 0.0, 0.0, 0.0, 0.0), N=600)
    ref = R.reference_for(case, g["x"], g["W"])
    assert ref.dp[1] == pytest.approx(-1.7236355e-3, rel=1e-7)


def test_the_beams_reach_the_branches_they_are_meant_for():
    for name, case in R.CASES.items():
        x, W = R.beam(case)
        assert x.shape == W.shape == (case.N, 7) and np.all(x[:, 6] == 1.0)
        if case.N >= 3:
            assert not x[0, :6].any() and x[1, 5] == 0.0 and x[2, 1] == 0.0 and x[2, 3] == 0.0
    case = R.CASES["quad_protons_low_energy"]
    evaluation, threshold = R.low_energy_evaluation(case, R.beam(case)[0])
    below, above = int((evaluation < 0.5 * threshold).sum()), int((evaluation > 2.0 * threshold).sum())
    assert below >= 50 and above >= 50, (below, above)      # well inside either branch of low_energy_z_correction
    for name in ("dipole_angle_+2", "dipole_angle_-2"):
        case = R.CASES[name]
        a = np.abs(R.dipole_branch_angle(case, R.beam(case)[0]))
        assert int((a < np.pi / 2 - 0.05).sum()) == 6 and int((a > np.pi / 2 + 0.3).sum()) == case.N - 6, name
    for name, case in R.CASES.items():
        if case.kind == R.DIPOLE and abs(case.params[1]) < 1.0:
            assert np.all(np.abs(R.dipole_branch_angle(case, R.beam(case)[0])) < 1.0), name
