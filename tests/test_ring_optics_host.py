"""Segment.ring_optics without a GPU: the C-ABI entry point is exported and bound, the algebra of cheetah_amd/particles/optics.py
(`twiss_from_matrix`, `propagate_twiss`, `eigen_tunes`) on CPU tensors against matrices built from drawn Twiss values, the
host-callable parts of csrc/chx_optics_dev.h in a stand-alone program built with the address and undefined-behaviour sanitizers,
and argument errors refused before any device work.

The bounds of the algebra, 1e-12 relative, are those of a handful of float64 operations on numbers of order one to fifty."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
TWO_PI = 2 * math.pi


def twiss_matrix(beta, alpha, mu):
    """The periodic 2 x 2 matrix of (beta, alpha, mu)."""
    gamma = (1 + alpha ** 2) / beta
    c, s = math.cos(mu), math.sin(mu)
    return np.array([[c + alpha * s, beta * s], [-gamma * s, c - alpha * s]])


def transfer_matrix(b0, a0, b1, a1, phi):
    """The 2 x 2 transfer matrix from (b0, a0) to (b1, a1) with the phase advance phi."""
    c, s = math.cos(phi), math.sin(phi)
    return np.array([[math.sqrt(b1 / b0) * (c + a0 * s), math.sqrt(b0 * b1) * s],
                     [((a0 - a1) * c - (1 + a0 * a1) * s) / math.sqrt(b0 * b1), math.sqrt(b0 / b1) * (c - a1 * s)]])


def draws(n=20, seed=5):
    """n draws of beta in [0.5, 50], alpha in [-3, 3] and a fractional tune in (0.02, 0.98) outside |nu - 0.5| < 0.02."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        nu = rng.uniform(0.02, 0.98)
        if abs(nu - 0.5) < 0.02:
            continue
        out.append((rng.uniform(0.5, 50.0), rng.uniform(-3.0, 3.0), nu))
    assert any(nu > 0.5 for _, _, nu in out) and any(nu < 0.5 for _, _, nu in out)
    return out


def test_symbol_exported_and_bound():
    import cheetah_amd._lib as L
    import cheetah_amd._ops  # noqa: F401  (adds the signatures)

    lib = L.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = set(re.findall(r" T (chx_[a-z0-9_]+)", out))
    for name in ("chx_dkd_ring_jacobian", "chx_dkd_ring_jacobian_workspace_bytes"):
        assert name in exported and name in L.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == L.SIGNATURES[name][1] and fn.restype is L.SIGNATURES[name][0]
    assert lib.chx_dkd_ring_jacobian.restype is ctypes.c_int
    assert lib.chx_abi_version() == 9
    header = open(os.path.join(ROOT, "include", "chx.h")).read()
    assert int(re.search(r"#define CHX_ABI_VERSION (\d+)", header).group(1)) == 9
    assert "int chx_dkd_ring_jacobian(" in header and "size_t chx_dkd_ring_jacobian_workspace_bytes(" in header


def test_public_names():
    import cheetah_amd as ca
    from cheetah_amd.particles import optics

    for name in ("one_turn_map", "closed_orbit", "ring_optics", "chromaticity"):
        assert callable(getattr(ca.Segment, name))
    for name in ("twiss_from_matrix", "propagate_twiss", "eigen_tunes", "OneTurnMap", "ClosedOrbit", "RingOptics"):
        assert getattr(ca, name) is getattr(optics, name)
    assert ca._ops.RING_MAX_ITEMS == 192
    assert "uncoupled" in optics.RingOptics.__doc__.lower() and "coupling" in optics.RingOptics.__doc__


def test_twiss_from_matrix_recovers_drawn_values():
    from cheetah_amd.particles.optics import twiss_from_matrix

    d = draws()
    M = torch.tensor(np.stack([twiss_matrix(b, a, TWO_PI * nu) for b, a, nu in d]), dtype=F64)
    beta, alpha, mu = twiss_from_matrix(M)
    worst = 0.0
    for k, (b, a, nu) in enumerate(d):
        errs = (abs(float(beta[k]) - b) / b, abs(float(alpha[k]) - a) / max(1.0, abs(a)), abs(float(mu[k]) / TWO_PI - nu) / nu)
        worst = max(worst, *errs)
        assert max(errs) <= 1e-12, (k, b, a, nu, errs)
        assert (float(mu[k]) / TWO_PI > 0.5) == (nu > 0.5)                     # a tune above one half comes back above one half
        assert float(beta[k]) > 0
    print("twiss_from_matrix: largest relative error", worst)
    # one matrix without batch dimensions, and float32 input widened
    b1, a1, m1 = twiss_from_matrix(M[3])
    assert b1.shape == () and float(b1) == float(beta[3]) and float(a1) == float(alpha[3]) and float(m1) == float(mu[3])


def test_unstable_block_is_nan():
    from cheetah_amd.particles.optics import eigen_tunes, twiss_from_matrix

    hyper = np.array([[math.cosh(0.3), 2 * math.sinh(0.3)], [math.sinh(0.3) / 2, math.cosh(0.3)]])          # tr > 2, det 1
    beta, alpha, mu = twiss_from_matrix(torch.tensor(np.stack([hyper, -hyper, twiss_matrix(3.0, 0.5, 1.0)]), dtype=F64))
    assert torch.isnan(beta[:2]).all() and torch.isnan(alpha[:2]).all() and torch.isnan(mu[:2]).all()
    assert abs(float(beta[2]) - 3.0) <= 3e-12
    M4 = np.zeros((4, 4))
    M4[:2, :2], M4[2:, 2:] = hyper, twiss_matrix(7.0, -1.0, TWO_PI * 0.31)
    tunes, stable = eigen_tunes(torch.tensor(M4, dtype=F64))
    assert stable.tolist() == [False, True]
    assert math.isnan(float(tunes[0])) and abs(float(tunes[1]) - 0.31) <= 1e-12
    M4[:2, :2], M4[2:, 2:] = twiss_matrix(7.0, -1.0, TWO_PI * 0.31), -hyper
    tunes, stable = eigen_tunes(torch.tensor(M4, dtype=F64))
    assert stable.tolist() == [True, False]
    assert math.isnan(float(tunes[1])) and abs(float(tunes[0]) - 0.31) <= 1e-12


def test_propagate_twiss_matches_the_sigma_matrix():
    """Through a drift and a thin quadrupole: sigma_1 = A sigma_0 A^T with sigma = [[beta, -alpha], [-alpha, gamma]]."""
    from cheetah_amd.particles.optics import propagate_twiss

    rng = np.random.default_rng(11)
    for A in (np.array([[1.0, 2.7], [0.0, 1.0]]), np.array([[1.0, 0.0], [-0.8, 1.0]]),
              np.array([[1.0, 0.0], [0.45, 1.0]]) @ np.array([[1.0, 1.3], [0.0, 1.0]])):
        for _ in range(5):
            b0, a0 = rng.uniform(0.5, 50.0), rng.uniform(-3.0, 3.0)
            sigma = A @ np.array([[b0, -a0], [-a0, (1 + a0 ** 2) / b0]]) @ A.T
            beta, alpha, phase = propagate_twiss(torch.tensor(A, dtype=F64), torch.tensor(b0, dtype=F64), torch.tensor(a0, dtype=F64))
            assert abs(float(beta) - sigma[0, 0]) <= 1e-12 * sigma[0, 0]
            assert abs(float(alpha) + sigma[0, 1]) <= 1e-12 * max(1.0, abs(sigma[0, 1]))
            assert 0 <= float(phase) < TWO_PI
            # the phase: tan phi = A12 / (A11 beta0 - A12 alpha0)
            assert abs(math.tan(float(phase)) - A[0, 1] / (A[0, 0] * b0 - A[0, 1] * a0)) <= 1e-12 * max(1.0, abs(math.tan(float(phase))))


def test_phase_increments_add_up_to_the_full_tune():
    """A chain of 40 items with drawn Twiss values and phase steps: the accumulated phase is the one-turn mu plus 2 pi times the
    integer the steps were drawn with."""
    from cheetah_amd.particles.optics import _along, twiss_from_matrix

    rng = np.random.default_rng(3)
    for trial in range(4):
        n = 40
        beta = np.concatenate([rng.uniform(0.5, 50.0, n), [0.0]])
        alpha = np.concatenate([rng.uniform(-3.0, 3.0, n), [0.0]])
        beta[n], alpha[n] = beta[0], alpha[0]                                   # periodic
        steps = rng.uniform(0.0, 0.9, n)                                        # each below a turn; some of them zero (thin items)
        steps[rng.integers(0, n, 5)] = 0.0
        for k in np.nonzero(steps == 0.0)[0]:                                   # (a thin item moves alpha, never beta)
            beta[k + 1] = beta[k]
        beta[n], alpha[n] = beta[0], alpha[0]
        if steps[n - 1] == 0.0:
            steps[n - 1] = 0.4
        total = steps.sum()
        assert total > TWO_PI                                                   # an integer part to find
        cumulative, A = [np.eye(2)], np.eye(2)
        for k in range(n):
            A = transfer_matrix(beta[k], alpha[k], beta[k + 1], alpha[k + 1], steps[k]) @ A
            cumulative.append(A)
        along = np.zeros((1, n + 1, 6, 6))
        along[0, :, :2, :2] = along[0, :, 2:4, 2:4] = np.stack(cumulative)
        b0, a0, mu = twiss_from_matrix(torch.tensor(cumulative[-1], dtype=F64))
        assert abs(float(b0) - beta[0]) <= 1e-9 * beta[0]
        two = lambda v: torch.stack([v, v]).reshape(1, 2)  # noqa: E731
        betas, alphas, phases = _along(torch.tensor(along, dtype=F64), two(b0), two(a0))
        integer = math.floor(total / TWO_PI)
        assert abs(float(phases[0, -1, 0]) - (float(mu) + TWO_PI * integer)) <= 1e-9, (trial, float(phases[0, -1, 0]), total)
        assert abs(float(phases[0, -1, 0]) - total) <= 1e-9
        assert np.abs(phases[0, :, 0].numpy() - np.concatenate([[0.0], np.cumsum(steps)])).max() <= 1e-9
        assert (torch.diff(phases[0, :, 0]) >= 0).all()
        assert np.abs(betas[0, :, 1].numpy() - beta).max() <= 1e-9 * beta.max()
        assert np.abs(alphas[0, :, 0].numpy() - alpha).max() <= 1e-8


def symplectic_coupling(rng):
    """A drawn 4 x 4 symplectic matrix (S = diag(J2, J2)) that couples x and y: exp(S K) of a drawn symmetric K with off-diagonal
    blocks, by its series (norm below 1)."""
    K = rng.uniform(-0.1, 0.1, (4, 4))
    K = K + K.T
    S = np.kron(np.eye(2), np.array([[0.0, 1.0], [-1.0, 0.0]]))
    G = S @ K
    R, term = np.eye(4), np.eye(4)
    for k in range(1, 40):
        term = term @ G / k
        R = R + term
    assert np.abs(R.T @ S @ R - S).max() < 1e-14
    assert np.abs(R[:2, 2:]).max() > 0.02
    return R


def test_eigen_tunes_survive_coupling():
    from cheetah_amd.particles.optics import eigen_tunes, twiss_from_matrix

    rng = np.random.default_rng(8)
    for (bx, ax, nx), (by, ay, ny) in zip(draws(10, seed=1), draws(10, seed=2)):
        if abs(math.cos(TWO_PI * nx) - math.cos(TWO_PI * ny)) < 0.05:
            continue                                                             # (the two roots must stay apart to be told apart)
        M = np.zeros((4, 4))
        M[:2, :2], M[2:, 2:] = twiss_matrix(bx, ax, TWO_PI * nx), twiss_matrix(by, ay, TWO_PI * ny)
        tunes, stable = eigen_tunes(torch.tensor(M, dtype=F64))
        assert stable.all() and abs(float(tunes[0]) - nx) <= 1e-12 and abs(float(tunes[1]) - ny) <= 1e-12
        R = symplectic_coupling(rng)
        C = R @ M @ np.linalg.inv(R)
        tunes_c, stable_c = eigen_tunes(torch.tensor(C, dtype=F64))
        # the same two tunes, each in its plane (the coupling is weak enough for the blocks to tell the planes and the signs)
        assert stable_c.all() and abs(float(tunes_c[0]) - nx) <= 1e-12 and abs(float(tunes_c[1]) - ny) <= 1e-12, (tunes_c, nx, ny)
        want = sorted(min(t, 1 - t) for t in (nx, ny))
        # ... while the block traces no longer give them
        block = [float(twiss_from_matrix(torch.tensor(C[2 * p:2 * p + 2, 2 * p:2 * p + 2], dtype=F64))[2]) / TWO_PI for p in range(2)]
        block = sorted(min(t, 1 - t) if t == t else float("nan") for t in block)
        assert not all(abs(f - w) <= 1e-6 for f, w in zip(block, want)), (block, want)


def test_solver_and_index_logic_on_the_host_under_sanitizers(tmp_path):
    """csrc/chx_optics_dev.h (the lane layout, the solver, the Newton and dispersion systems, the singular cases) against
    long-double eliminations with complete pivoting, compiled for the host only with -fsanitize=address,undefined (no GPU, no HIP
    runtime call, nothing loaded into Python)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "optics_check"
    subprocess.run([hipcc, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cheetah_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "optics_check.hip")], check=True, capture_output=True)
    syms = subprocess.check_output(["nm", str(exe)], text=True)
    assert "__asan_init" in syms and "__ubsan_handle" in syms                   # the check did run instrumented
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    for part in ("layout", "solver", "singular", "systems", "all"):
        assert f"{part}: ok" in out.stdout, out.stdout


def test_invalid_arguments_are_refused_before_any_launch():
    import cheetah_amd._lib as L
    import cheetah_amd._ops  # noqa: F401

    lib = L.lib()
    buf = (ctypes.c_double * 64)()                 # host memory standing in for pointers that must never be dereferenced
    p = ctypes.addressof(buf)
    ws_bytes = lib.chx_dkd_ring_jacobian_workspace_bytes

    def call(E=2, kinds=None, steps=None, fringe=None, B=3, mode=1, iters=10, along=0, energy=p, start=p, orbit=p, image=p, matrix=p,
             residual=p, dispersion=p, orbit_along=None, matrix_along=None, s_along=None, ws=p, ws_size=None, dtype=1, params=True,
             null=None):
        n = max(E, 1)
        i32, vp = ctypes.c_int32 * n, ctypes.c_void_p * n
        k = i32(*(kinds or [0] * n))
        pp = vp(*([p] * n))
        if params is None:
            pp[0] = None
        arrays = {"kinds": k, "params": pp, "steps": i32(*(steps or [1] * n)), "fringe": i32(*(fringe or [3] * n))}
        if null:
            arrays[null] = None
        size = ws_bytes(min(max(E, 1), 192)) if ws_size is None else ws_size
        return lib.chx_dkd_ring_jacobian(arrays["kinds"], arrays["params"], arrays["steps"], arrays["fringe"], E, energy, 510998.95, -1.0, dtype,
                                         start, B, mode, iters, along, orbit, image, matrix, residual, dispersion, orbit_along,
                                         matrix_along, s_along, ws, size, None)

    assert ws_bytes(0) == 0 and ws_bytes(193) == 0 and ws_bytes(-1) == 0
    assert ws_bytes(1) >= 56 * 8 + 8 and ws_bytes(192) >= 192 * 57 * 8 and ws_bytes(48) % 16 == 0
    assert call(E=0) == -1
    assert call(E=193) == -1
    assert call(B=0) == -1
    assert call(B=-5) == -1
    assert call(mode=3) == -1
    assert call(mode=-1) == -1
    assert call(iters=0) == -1
    assert call(mode=2, iters=0) == -1
    assert call(kinds=[0, 3]) == -1                # the TDC is no ring element
    assert call(kinds=[0, 7]) == -1
    assert call(kinds=[0, 4]) == -1                # nor is a linear run
    assert call(steps=[1, 0]) == -1
    assert call(steps=[1, 1 << 25]) == -1
    assert call(fringe=[4, 0]) == -1
    assert call(along=2) == -1
    assert call(along=1) == -1                     # the three per-item outputs are required then
    assert call(along=1, orbit_along=p, matrix_along=p) == -1
    for name in ("energy", "start", "orbit", "image", "matrix", "residual", "dispersion", "ws"):
        assert call(**{name: None}) == -1, name
    for name in ("kinds", "params", "steps", "fringe"):
        assert call(null=name) == -1, name
    assert call(params=None) == -1                 # one item without parameters
    assert call(ws_size=ws_bytes(2) - 1) == -1
    assert call(ws=p + 8) == -1                    # not 16-byte aligned
    assert call(dtype=2) == -2


def test_python_argument_errors_come_before_the_gpu_check():
    import cheetah_amd as ca

    kw = {"dtype": F64}
    dkd = {"tracking_method": "drift_kick_drift"}
    ring = ca.Segment([ca.Drift(torch.tensor(0.3, **kw), **dkd, **kw), ca.Quadrupole(torch.tensor(0.2, **kw), k1=torch.tensor(1.0, **kw), **dkd, **kw)])
    energy = torch.tensor(1e8, **kw)
    with pytest.raises(ValueError, match="shape"):
        ring.one_turn_map(torch.zeros(3, 5, **kw), energy)
    with pytest.raises(ValueError, match="num_iterations"):
        ring.closed_orbit(energy, num_iterations=0)
    with pytest.raises(ValueError, match="requires grad"):
        ring.one_turn_map(torch.zeros(1, 6, **kw).requires_grad_(True), energy)
    with pytest.raises(ValueError, match="requires grad"):
        ring.closed_orbit(energy.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="h must be positive"):
        ring.chromaticity(energy, h=0.0)
    linear = ca.Segment([ca.Drift(torch.tensor(0.3, **kw), **kw), ring.elements[1].clone()])
    with pytest.raises(ValueError, match="run of linear elements"):
        linear.one_turn_map(torch.zeros(1, 6, **kw), energy)
    long_ring = ca.Segment([ca.Drift(torch.tensor(0.1, **kw), name=f"d{k}", **dkd, **kw) for k in range(193)])
    with pytest.raises(ValueError, match="193 drift-kick-drift elements.*1 to 192"):
        long_ring.ring_optics(energy)
    with pytest.raises(RuntimeError, match="GPU only"):
        ring.one_turn_map(torch.zeros(2, 6, **kw), energy)
