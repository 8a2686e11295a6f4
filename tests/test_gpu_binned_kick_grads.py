"""The backward passes of the four binned-beam kicks (Wakefield, CSRKick, TransientCSRKick, LSCKick) against autograd through the
float64 CPU restatements of their own test modules, at the shapes where the backward kernels leave their first loop trip: more than
one tile of 64 nodes (a second workgroup of the adjoint Toeplitz kernels, a wave's second trip, every slot of the per-workgroup
partials, dynamic LDS above 64 KiB at M = 4096), more than one workgroup of the particle passes (G = ceil(N / 2048) = 2, 3, 293 and
the cap of 1024), transient lags that straddle a tile of the b table, wakes with one table or a table shorter than the bunch, float32
beams, and particles shared by the batch rows next to a row that cannot kick. One process, no workers.

Scheme of every case (`_run`): leaves on the device for every float input, the element tracked, the output contracted with a fixed
random cotangent drawn on the CPU, `backward()`; the same on CPU copies through the restatement with the same cotangent; every
leaf's gradient compared, every reference gradient non-zero.

Bounds (`_run`). float64: 1e-9 max|reference gradient| per leaf, as the kicks' own gradient tests. float32: the kernels compute in
float64 and round at the end, so per element k ulp32(reference) + 1e-9 max|reference| with k the number of float32 roundings
between the kernel's float64 value and the leaf's gradient (`_ROUNDINGS`; a rounding moves a value v by at most 2^-24 |v| <
ulp32(v)). Where a float32 gradient is a sum over the batch rows (an input shared by B rows: `_beam_grads` sums B float32 rows), the
roundings are relative to the rows and the partial sums, not to the result, which may be small by cancellation: the ulp is then
taken at A = sum over the rows of |the row's reference gradient| (A = |reference| where the rows do not cancel), and the sum adds
B - 1 roundings of partial sums, each at most A in magnitude: (k + B - 1) ulp32(A).

Workgroups the cases produce (G of the particle passes, node workgroups ceil(M / 64) of the adjoint Toeplitz kernels):
  node tiles, N = 5000: G = 3; M = 64, 65, 129, 257, 500, 4096 -> 1, 2, 3, 5, 8, 64 node workgroups
  merge edges, M = 65 (2 node workgroups): N = 2049 -> G = 2 (chunks of 1025 and 1024); N = 600 000 -> G = 293; N = 2 100 001 ->
    G = 1024 (the cap), chunks of 2051
  transient lags, M = 257, N = 5000: G = 3, 5 node workgroups
  wake variants, M = 129, N = 5000: G = 3, 3 node workgroups
  float32, N = 5000: G = 3; M = 65, 257, 4096 -> 2, 5, 64 node workgroups
  shared particles, M = 129, N = 5000, B = 3: G = 3, 3 node workgroups per row"""
from unittest import mock

import pytest
import torch

import tests.test_gpu_csr as csr
import tests.test_gpu_csr_transient as csrt
import tests.test_gpu_lsc as lsc
import tests.test_gpu_wakefield as wake

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
ENERGY = csr.ENERGY
KICKS = ["wake", "csr", "csr_transient", "lsc"]
WAKE_SPACING = 1e-6             # 300 entries span 3e-4 m: beyond the bunch (8 sigma_tau = 1.6e-4 m) at every M; 60 entries do not
ROW_VALUES = [0.3, 0.7, 0.5]    # the per-row setting of a batch (length; the wake: its factor)

#: float32 roundings between the kernel's float64 value and a leaf's gradient
_ROUNDINGS = {
    "particles": 1,             # B4 / B5 store (T)gv[c]
    "charges": 2,               # (T)dc, then dC * w rounded (the sign is exact)
    "survival": 2,              # (T)dc, then dC * |q| rounded
}
_SETTING_ROUNDINGS = 1          # float64 per-row cotangents and chain rule, one `.to(x.dtype)` (the wake: the backward of `.to(float64)`)


def _dev(v, dtype):
    return torch.as_tensor(v, dtype=F64).to(device="cuda", dtype=dtype)


def _beam(mod, N, dtype, B, seed, shared_x=False, dead_row=None):
    """(x, q, w) of `mod._beam_tensors`: x (B, N, 7), or (N, 7) for a single row or `shared_x`; q (N,); w (N,), or (B, N) with the
    row `dead_row` all zero."""
    x, q, w = mod._beam_tensors(N, dtype, batch=() if (B is None or shared_x) else (B,), seed=seed)
    if dead_row is not None:
        w = torch.stack([torch.zeros_like(w) if b == dead_row else w for b in range(B)])
    return x, q, w


def _first_live_row(x, w):
    return (x[0] if x.dim() == 3 else x), (w[0] if w.dim() == 2 else w)


def _beam_of(x, q, w, e):
    import cheetah_amd as ca

    return ca.ParticleBeam(x, e, particle_charges=q, survival_probabilities=w)


def _row_values(B, single, dtype):
    return _dev(ROW_VALUES[:B] if B else single, dtype)


def _csr_case(N, M, dtype, B=None, seed=8, **beam):
    x, q, w = _beam(csr, N, dtype, B, seed, **beam)
    inputs = (x, q, w, _dev(ENERGY, dtype), _row_values(B, 0.4, dtype), _dev(-0.03, dtype))

    def track(x, q, w, e, L, theta):
        elem = csr._element(0.4, -0.03, M, dtype)
        elem.effect_length, elem.angle = L, theta
        return elem.track(_beam_of(x, q, w, e)).particles

    names = ["particles", "charges", "survival", "energy", "effect_length", "angle"]
    return names, inputs, track, lambda *leaves: csr._reference(*leaves, M), csr._check_against_reference


def _transient_case(N, M, dtype, B=None, seed=8, xn=None, **beam):
    """`xn`: the slippage length in node spacings (default M / 8 + 0.3: x and 4x are no integers at any M used). Rows with their own
    particles get their own distance, so that every row has x = xn; rows that share the particles share the distance too, chosen
    for the last row's length, and x goes with 1 / L^2 over the rows."""
    xn = M / 8 + 0.3 if xn is None else xn
    x, q, w = _beam(csr, N, dtype, B, seed, **beam)
    L = _row_values(B, 0.4, dtype)
    if x.dim() == 3:
        d = [csrt._distance(xn, csrt._node_spacing(x[b], w, M), float(L[b]), 0.03) for b in range(B)]
    else:
        d = csrt._distance(xn, csrt._node_spacing(*_first_live_row(x, w), M), float(L.reshape(-1)[-1]), 0.03)
    inputs = (x, q, w, _dev(ENERGY, dtype), L, _dev(-0.03, dtype), _dev(d, dtype))

    def track(x, q, w, e, L, theta, d):
        elem = csrt._element(0.4, -0.03, 0.1, M, dtype)
        elem.effect_length, elem.angle, elem.entrance_distance = L, theta, d
        return elem.track(_beam_of(x, q, w, e)).particles

    names = ["particles", "charges", "survival", "energy", "effect_length", "angle", "entrance_distance"]
    return names, inputs, track, lambda *leaves: csrt._reference(*leaves, M), csr._check_against_reference


def _lsc_case(N, M, dtype, B=None, seed=8, **beam):
    x, q, w = _beam(lsc, N, dtype, B, seed, **beam)
    radius = 1.3 * lsc._gamma(dtype) * lsc._spacing(*_first_live_row(x, w), M)               # rho about 1.3
    inputs = (x, q, w, _dev(ENERGY, dtype), _row_values(B, 1.5, dtype), _dev(radius, dtype))

    def track(x, q, w, e, L, a):
        elem = lsc._element(1.0, 1e-4, M, dtype)
        elem.effect_length, elem.beam_radius = L, a
        return elem.track(_beam_of(x, q, w, e)).particles

    def reference(*leaves):
        # the restatement takes the mass of a beam of the dtype of the particles it is handed; the float64 leaves here hold the
        # values of a beam of `dtype`, whose mass the kernels got
        mass = lsc._mass(dtype)
        with mock.patch.object(lsc, "_mass", lambda dtype=F64: mass):
            return lsc._reference(*leaves, M)

    names = ["particles", "charges", "survival", "energy", "effect_length", "beam_radius"]
    return names, inputs, track, reference, None


def _wake_case(N, M, dtype, B=None, seed=8, kind="lt", entries=300, **beam):
    x, q, w = _beam(wake, N, dtype, B, seed, **beam)
    tables = [(name, t.to(device="cuda", dtype=dtype)) for name, t in
              zip(("longitudinal_wake", "transverse_wake"), wake._tables(kind, L=entries, seed=seed)) if t is not None]
    inputs = (x, q, w, _dev(ENERGY, dtype), _row_values(B, 1.2, dtype), *(t for _, t in tables))
    h = float(_dev(WAKE_SPACING, dtype))                 # the spacing as the element holds it

    def track(x, q, w, e, factor, *tabs):
        given = dict(zip((name for name, _ in tables), tabs))
        elem = wake._element(given.get("longitudinal_wake"), given.get("transverse_wake"), M, dtype=dtype, h=WAKE_SPACING)
        elem.factor = factor
        for name, t in given.items():
            setattr(elem, name, t)
        assert float(elem.wake_spacing) == h
        return elem.track(_beam_of(x, q, w, e)).particles

    def reference(x, q, w, e, factor, *tabs):
        given = dict(zip((name for name, _ in tables), tabs))
        return wake._reference(x, q, w, e, factor, given.get("longitudinal_wake"), given.get("transverse_wake"), h, M)

    names = ["particles", "charges", "survival", "energy", "factor", *(name for name, _ in tables)]
    return names, inputs, track, reference, wake._check_against_reference


_CASES = {"wake": _wake_case, "csr": _csr_case, "csr_transient": _transient_case, "lsc": _lsc_case}


def _ulp32(v):
    v = v.to(F32)
    return (torch.nextafter(v, torch.full_like(v, float("inf"))) - v).to(F64)


def _run(case, dtype, forward=False, dead_row=None):
    """The scheme of the module docstring on one case of `_CASES`. `forward`: also assert the tracked particles against the
    restatement with the bound of the kick's own module. `dead_row`: a batch row that cannot kick: the gradients of its output alone
    are the cotangent for the particles and exactly zero for every other leaf."""
    names, inputs, track, reference, check_forward = case
    leaves = [t.clone().requires_grad_() for t in inputs]
    out = track(*leaves)
    assert out.dtype == dtype
    B = out.shape[0] if out.dim() == 3 else 1
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(3), dtype=F64)
    if dtype == F32:
        cot = cot.to(F32).to(F64)                        # the cotangent the device gets, exactly
    cot_dev = cot.to(device="cuda", dtype=dtype)

    if dead_row is not None:
        alone = torch.autograd.grad((out[dead_row] * cot_dev[dead_row]).sum(), leaves, retain_graph=True)
        for name, g in zip(names, alone):
            if name == "particles":                      # shared: the sum of the rows' gradients, the live rows' exactly zero
                assert g.shape == cot_dev.shape[1:] and torch.equal(g, cot_dev[dead_row]), name
            else:
                assert not bool(g.count_nonzero()), name

    (out * cot_dev).sum().backward()
    got = [t.grad.cpu().to(F64) for t in leaves]

    # CPU leaves: an input shared by the B rows gets a copy per row, so that the reference has the rows' gradients one by one
    shared = {name for name, t in zip(names, inputs)
              if B > 1 and ((name == "particles" and t.dim() == 2) or (name in ("charges", "survival") and t.dim() == 1))}
    rl = []
    for name, t in zip(names, inputs):
        r = t.detach().cpu().to(F64)
        rl.append((r.expand(B, *r.shape) if name in shared else r).clone().requires_grad_())
    ref = reference(*rl)
    if forward:
        check_forward(out.detach(), ref.detach(), inputs[0].expand(out.shape), dtype)
    (ref * cot).sum().backward()

    failed = []
    for name, a, r in zip(names, got, rl):
        rows = r.grad
        b, mag, adds = (rows.sum(dim=0), rows.abs().sum(dim=0), B - 1) if name in shared else (rows, rows.abs(), 0)
        scale = b.abs().max()
        assert scale > 0, name
        err = (a - b).abs()
        tol = 1e-9 * scale
        if dtype == F32:
            tol = (_ROUNDINGS.get(name, _SETTING_ROUNDINGS) + adds) * _ulp32(mag) + tol
        print(f"{name}: max error / max |gradient| {float(err.max() / scale):.3e}, max (error - bound) / max |gradient| "
              f"{float((err - tol).max() / scale):.3e}")
        if not bool((err <= tol).all()):
            failed.append((name, float(err.max() / scale), float((err - tol).max() / scale)))
    assert not failed, failed
    # the tau column gets the node coordinate's term
    assert float(got[0][..., 4].abs().max()) > 0


# ---- 1. node-tile edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [64, 65, 129, 257, 500, 4096])
@pytest.mark.parametrize("kick", KICKS)
def test_node_tile_edges(kick, M):
    """Two rows with their own particles and settings: one full tile, a second workgroup with one live lane, three tiles, wave 0's
    second trip, the lattice helpers' size, and 64 workgroups (every slot of the per-workgroup partials of both rows, dynamic LDS
    above 64 KiB in every backward kernel)."""
    _run(_CASES[kick](5000, M, F64, B=2), F64)


# ---- 2. workgroup-merge edges of the particle passes --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2049, 600_000])
@pytest.mark.parametrize("kick", KICKS)
def test_particle_workgroup_merge_edges(kick, N):
    _run(_CASES[kick](N, 65, F64, seed=N), F64)


@pytest.mark.parametrize("kick", ["csr", "wake"])
def test_capped_particle_workgroups_forward_and_backward(kick):
    """N = 2 100 001: ceil(N / 2048) = 1026 workgroups are capped at 1024, which take chunks of 2051 particles; no forward test
    reaches the cap either, so the tracked particles are asserted too. The CSR kick runs every shared particle pass, the wake with
    both tables every pass of its own."""
    _run(_CASES[kick](2_100_001, 65, F64, seed=5), F64, forward=True)


# ---- 3. transient lags across the tiles of the b table --------------------------------------------------------------------------------
@pytest.mark.parametrize("xn", [15.9, 63.55, 0.2, 70.3])
def test_transient_lags_straddle_tile_boundaries(xn):
    """x = 15.9: p4 = 63, p4 + 1 = 64. x = 63.55: p = 63, p + 1 = 64, p4 = 254, nl = 256 < M (not 63.5, whose 4x = 254 is an integer:
    the kick is not differentiable there). x = 0.2: p4 = p = 0, the combined interpolation. x = 70.3: 4x > M, so nl = M."""
    _run(_transient_case(5000, 257, F64, xn=xn), F64)


# ---- 4. wake variants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,entries", [("l", 300), ("t", 300), ("lt", 300), ("lt", 60), ("lt", 1)])
def test_wake_with_one_table_and_short_tables(kind, entries):
    """One table only (the cotangent deposit's channel slots move), a table shorter than the bunch on the grid (late lags sample
    beyond it) and a table of one entry (the self term alone); the tables' gradients are leaves like the rest."""
    _run(_wake_case(5000, 129, F64, kind=kind, entries=entries), F64)


# ---- 5. float32 beams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [65, 257, 4096])
@pytest.mark.parametrize("kick", KICKS)
def test_float32_beam(kick, M):
    _run(_CASES[kick](5000, M, F32, seed=M), F32)


# ---- 6. particles shared by the batch rows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dead_row", [None, 1])
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("kick", KICKS)
def test_shared_particles_under_a_vectorised_setting(kick, dtype, dead_row):
    """Particles (N, 7) and charges (N,) under a (3,) setting: their gradients are the sums over the rows. `dead_row`: the survival
    probabilities are (3, N) with that row all zero, a row that cannot kick between two that do."""
    _run(_CASES[kick](5000, 129, dtype, B=3, shared_x=True, dead_row=dead_row), dtype, dead_row=dead_row)
