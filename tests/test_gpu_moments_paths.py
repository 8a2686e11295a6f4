"""Every path of the beam-moment reductions (csrc/chx_moments.hip) at its edges, against the reference's two-pass weighted
statistics in np.longdouble (tests/moments_ref.py) within a derived worst-case bound — and `chx_sc_beam_geometry`, whose beam
sizes come out of a reduction of its own, against the same reference.

The host picks the kernel by shape (chx_moments_entry):
  B >= 64 and N <= 2048      moments_rows_wave_kernel: one wave per row, finalize arithmetic on lanes 0..28
  everything else            moments_onepass_kernel with nblk = min(ceil(N / tile), 512 // B) workgroups per row (tile = 512 rows
                             in float32, 256 in float64), then moments_reduce_finalize_kernel with 64, 256 or 1024 threads for
                             nblk <= 64, <= 256 and above: for B = 1 the switches sit at N = 32768 | 32769 and 131072 | 131073
                             (float32), 16384 | 16385 and 65536 | 65537 (float64)
  B > 65535 and N > 2048     row slices, cut in Python (_ops._moments_raw)
These thresholds hold with CHX_TUNE_MOMENTS_WGS unset (it overrides the 512): the module asserts that below.

Every test prints the largest error / bound it saw ("moments_paths <path> <dtype> ..."; profiles/moments_paths.md)."""
import os

import numpy as np
import pytest
import torch

from tests import moments_ref as mr
from tests.test_gpu_moments_weights import _torch_moments

assert "CHX_TUNE_MOMENTS_WGS" not in os.environ, "the shapes of this file sit at the kernel switches of the DEFAULT workgroup count"

gpu = pytest.mark.gpu
DTYPES = ["f32", "f64"]
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}
WAVE_N = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2047, 2048]
ONEPASS_N = {"f32": [1, 16, 17, 511, 512, 513, 32768, 32769, 131072, 131073, 262145],
             "f64": [255, 256, 257, 16384, 16385, 65536, 65537, 131073]}
SWITCH_N = {"f32": [32768, 32769, 131072, 131073], "f64": [16384, 16385, 65536, 65537]}
CAP = {name: (1e-3 if name == "dead_first_wave" else 1e-6) for name in mr.BEAMS}


def report(path, tag, what, worst):
    print(f"moments_paths {path} {tag} {what}: max err/bound {worst:.3g}")


def finalize_path(tag, B, N):
    """The name of the kernel path a (B, N) call takes (module docstring)."""
    if B >= 64 and N <= 2048:
        return "wave_per_row"
    nblk = min(-(-N // (512 if tag == "f32" else 256)), max(1, 512 // B))
    return f"onepass_finalize{64 if nblk <= 64 else 256 if nblk <= 256 else 1024}"


def divisor(path):
    """How the path forms W - W2 / W (`moments_ref.onepass`; it matters only where a degenerate row is compared with the formulas)."""
    return "pairs" if path == "wave_per_row" else "sums"


def stack(name, B, N, tag):
    """B rows of the named beam (seeds 0..B-1) in the dtype `tag`: x (B, N, 7), w (B, N)."""
    rows = [mr.beam(name, N, seed) for seed in range(B)]
    return np.stack([r[0] for r in rows]).astype(mr.NP_DT[tag]), np.stack([r[1] for r in rows]).astype(mr.NP_DT[tag])


def device_moments(x, w, B, entry=None):
    """chx_moments of numpy rows x (Bx, N, 7), w (Bw, N) or None through _ops._moments_raw -> numpy (B, 29); with `entry` the two
    device tensors (moments, entries) instead."""
    import cheetah_amd  # noqa: F401
    from cheetah_amd import _ops

    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    wt = None if w is None else torch.from_numpy(np.ascontiguousarray(w)).cuda()
    res = _ops._moments_raw(xt, wt, B, x.shape[1], entry)
    return res.cpu().numpy() if entry is None else res


def layouts(B):
    """(particles per row?, weights: None | 'shared' | 'rows'): weights absent, (N,) and (B, N); particles (N, 7) and (B, N, 7)."""
    return [(px, wk) for px in ((False, True) if B > 1 else (False,)) for wk in ((None, "shared", "rows") if B > 1 else (None, "shared"))]


def check_layouts(x, w, B, cap_cov, path, tag, what):
    """Run and check x (B, N, 7), w (B, N) in every layout the call takes; rows that share all their inputs share one reference."""
    worst = 0.0
    for per_row_x, wkind in layouts(B):
        xs = x if per_row_x else x[:1]
        ws = None if wkind is None else (w if wkind == "rows" else w[:1])
        got = device_moments(xs, ws, B)
        assert got.shape == (B, 29)
        R = B if (per_row_x or wkind == "rows") else 1
        xr = np.broadcast_to(xs, (R,) + xs.shape[1:])
        wr = None if ws is None else np.broadcast_to(ws, (R, ws.shape[1]))
        if R == 1:
            assert (got.view(np.int64) == got[:1].view(np.int64)).all(), (what, "rows of the same inputs differ")
            got = got[:1]
        worst = max(worst, mr.check_rows(got, xr, wr, cap_cov, f"{what} x_rows={per_row_x} w={wkind}", divisor(path)))
    report(path, tag, what, worst)


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_longdouble_reference_and_bound_on_the_cpu():
    """The reference is evaluated in an extended longdouble (otherwise its sums fall back to math.fsum), and the bound holds for a
    float64 numpy restatement of the shifted one-pass sums on shuffled rows, for the six beams, both row dtypes and an N behind every
    kernel switch — with the caps on the bound asserted on the reference alone."""
    assert np.finfo(np.longdouble).eps < 1e-18
    rng = np.random.default_rng(2024)
    worst = 0.0
    for N in (17, 257, 2049, 32769, 131073):
        for tag in DTYPES:
            for name in mr.BEAMS:
                x, w = stack(name, 1, N, tag)
                ref = mr.reference(x, w)
                bnd = mr.bounds(x, w, ref)
                mr.check_caps(ref, bnd, CAP[name], (name, N, tag))
                ratio = mr.error_over_bound(mr.onepass(x, w, rng.permutation(N)), ref, bnd)
                assert float(ratio.max()) <= 1.0, (name, N, tag, float(ratio.max()))
                worst = max(worst, float(ratio.max()))
    report("numpy_restatement", "both", "six beams, shuffled rows", worst)


# ---------------------------------------------------------------------------------------------------------------- wave per row
@gpu
@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("N", WAVE_N)
def test_wave_per_row_at_every_row_length(tag, N):
    """B = 64: rows shorter than the 16 of the provisional centre, not a multiple of the 64 lanes, of the 256 rows of a sweep, and
    the longest row the path takes. N = 1: degenerate rows.

    N = 2 is the row the divisor decides: W - W2 / W cancels when the two weights are uneven (with the divisor taken as that
    difference, covariances came out at up to 340 times their bound in rows with weights near 1 : 100), so the kernel forms it
    as 2 (sum of w_n w_m over n < m) / W; the bound of 2 u per sum leaves room for little else."""
    B = 64
    assert finalize_path(tag, B, N) == "wave_per_row"
    x, w = stack("plain_weighted", B, N, tag)
    check_layouts(x, w, B, 1e-6, "wave_per_row", tag, f"B={B} N={N} plain_weighted")


@gpu
@pytest.mark.parametrize("tag", DTYPES)
def test_wave_per_row_with_waves_past_the_last_row(tag):
    """B = 67: the last workgroup of four waves holds three rows."""
    x, w = stack("plain_weighted", 67, 33, tag)
    check_layouts(x, w, 67, 1e-6, "wave_per_row", tag, "B=67 N=33 plain_weighted")


def hard_rows(B, N, tag):
    """A different hard beam in different rows: x (B, N, 7), w (B, N), the cap of each row."""
    rows = [mr.beam(mr.HARD_BEAMS[b % 5], N, b) for b in range(B)]
    caps = np.array([CAP[mr.HARD_BEAMS[b % 5]] for b in range(B)])
    return np.stack([r[0] for r in rows]).astype(mr.NP_DT[tag]), np.stack([r[1] for r in rows]).astype(mr.NP_DT[tag]), caps


@gpu
@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("N", [300, 2048])
def test_wave_per_row_hard_beams(tag, N):
    """Dead and live outliers in slot 0, a dead first wave, an offset beam and a weighted tail, side by side in the rows of one call."""
    B = 64
    x, w, caps = hard_rows(B, N, tag)
    worst = mr.check_rows(device_moments(x, w, B), x, w, caps, f"hard beams ({B}, {N})", divisor("wave_per_row"))
    report("wave_per_row", tag, f"B={B} N={N} five hard beams", worst)


# ---------------------------------------------------------------------------------------------------------------- one pass
@gpu
@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("shape", [(63, 2048), (64, 2049)])
def test_just_off_the_wave_per_row_path(tag, shape):
    B, N = shape
    path = finalize_path(tag, B, N)
    assert path == "onepass_finalize64"
    x, w = stack("plain_weighted", B, N, tag)
    check_layouts(x, w, B, 1e-6, path, tag, f"B={B} N={N} plain_weighted")


@gpu
@pytest.mark.parametrize("tag,N", [(tag, N) for tag in DTYPES for N in ONEPASS_N[tag]])
def test_one_pass_single_row(tag, N):
    """B = 1 around the tile, on both sides of each finalize switch (there: all six beams), and with more rows per workgroup than
    one tile (N > 262144)."""
    path = finalize_path(tag, 1, N)
    for name in (mr.BEAMS if N in SWITCH_N[tag] else mr.BEAMS[:1]):
        x, w = stack(name, 1, N, tag)
        if name == "plain_weighted":
            check_layouts(x, w, 1, CAP[name], path, tag, f"B=1 N={N} {name}")
        else:                                   # (the beam is what it is with its weights)
            worst = mr.check_rows(device_moments(x, w, 1), x, w, CAP[name], f"{name} N={N}", divisor(path))
            report(path, tag, f"B=1 N={N} {name}", worst)


def test_the_single_row_shapes_sit_on_both_sides_of_each_finalize_switch():
    for tag in DTYPES:
        lo, hi, lo2, hi2 = SWITCH_N[tag]
        assert [finalize_path(tag, 1, n) for n in (lo, hi, lo2, hi2)] == ["onepass_finalize64", "onepass_finalize256",
                                                                         "onepass_finalize256", "onepass_finalize1024"]
        assert all(n in ONEPASS_N[tag] for n in SWITCH_N[tag])


@gpu
@pytest.mark.parametrize("tag", DTYPES)
def test_one_pass_at_the_workgroup_cap(tag):
    """B = 3, N = 87041: more tiles than the 512 // 3 workgroups a row gets."""
    B, N = 3, 87041
    assert -(-N // 512) > 512 // B
    x, w = stack("plain_weighted", B, N, tag)
    check_layouts(x, w, B, 1e-6, finalize_path(tag, B, N), tag, f"B={B} N={N} plain_weighted")


# ---------------------------------------------------------------------------------------------------------------- degenerate rows
@gpu
@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("shape", [(64, 33), (1, 300), (3, 2049)])
def test_rows_without_any_weight(tag, shape):
    """Rows whose weights are all zero among ordinary rows: W = W2 = 0 and NaN everywhere else (0 / 0), the other rows untouched."""
    B, N = shape
    x, w = stack("plain_weighted", B, N, tag)
    dead = sorted({0, B - 1} | ({B // 2} if B > 3 else set()))
    w[dead] = 0.0
    got = device_moments(x, w, B)
    assert (got[dead, :2] == 0.0).all() and np.isnan(got[dead, 2:]).all()
    worst = mr.check_rows(got, x, w, 1e-6, f"zero-weight rows {dead} of ({B}, {N})", divisor(finalize_path(tag, B, N)))
    report(finalize_path(tag, B, N), tag, f"B={B} N={N} rows without weight", worst)


# ---------------------------------------------------------------------------------------------------------------- entry output
@gpu
@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("shape", ["wave", 64, 256, 1024])
def test_entry_output_is_the_cast_entry_of_the_row(tag, shape):
    """chx_moments_entry (one beam property in the beam dtype from the same launches): index 8 with the square root (sigma_x), index 4
    without (mu_y), on the wave-per-row kernel and on each finalize width — the entry of the 29-vector, cast, bit for bit."""
    B, N = {"wave": (64, 257), 64: (1, 513), 256: (1, SWITCH_N[tag][1]), 1024: (1, SWITCH_N[tag][3])}[shape]
    path = finalize_path(tag, B, N)
    assert path == ("wave_per_row" if shape == "wave" else f"onepass_finalize{shape}")
    x, w = stack("plain_weighted", B, N, tag)
    plain = device_moments(x, w, B)
    worst = mr.check_rows(plain, x, w, 1e-6, f"entry ({B}, {N})", divisor(path))
    for index, take_sqrt in ((8, True), (4, False)):
        mom, picked = device_moments(x, w, B, entry=(index, take_sqrt))
        assert (mom.cpu().numpy().view(np.int64) == plain.view(np.int64)).all()
        want = (mom[:, index].sqrt() if take_sqrt else mom[:, index]).to(TORCH_DT[tag])     # (the device's own float64 sqrt)
        assert picked.dtype == TORCH_DT[tag] and picked.shape == (B,)
        view = torch.int32 if tag == "f32" else torch.int64
        off = (picked.view(view) - want.view(view)).abs()
        assert int(off.max()) == 0, (index, take_sqrt, "entries that differ", int((off != 0).sum()), "by at most (ulp)", int(off.max()))
    report(path, tag, f"B={B} N={N} entry form", worst)


# ---------------------------------------------------------------------------------------------------------------- row slicing
@gpu
def test_more_long_rows_than_one_launch_takes():
    """B = 65537 rows of N = 2049 (float32): too long for the wave-per-row kernel, too many for one grid — _ops._moments_raw cuts
    the rows into slices. A shared beam with per-row weights (0.5 GB, drawn on the device); rows 0, 65534, 65535 and 65536 carry
    the same weights and must give the same bits wherever the cut falls; they and two more rows against the reference."""
    import cheetah_amd  # noqa: F401
    from cheetah_amd import _ops

    B, N = 65537, 2049
    assert B > _ops.MAX_GRID_ROWS and N > 2048
    x, _ = stack("plain_weighted", 1, N, "f32")
    xt = torch.from_numpy(x).cuda()
    gen = torch.Generator(device="cuda").manual_seed(11)
    wt = torch.rand(B, N, device="cuda", dtype=torch.float32, generator=gen)
    same = [0, 65534, 65535, 65536]
    wt[same[1:]] = wt[0].clone()
    picks = same + [12345, 40000]
    w_host = wt[picks].cpu().numpy()
    x_host = np.broadcast_to(x, (len(picks), N, 7))
    plain = _ops._moments_raw(xt, wt, B, N)
    assert plain.shape == (B, 29)
    got = plain[picks].cpu().numpy()
    assert (got[:4].view(np.int64) == got[0].view(np.int64)).all(), "the same row gives other bits in another slice"
    worst = mr.check_rows(got, x_host, w_host, 1e-6, "row slices, plain form")
    mom, picked = _ops._moments_raw(xt, wt, B, N, entry=(8, True))
    assert mom.shape == (B, 29) and picked.shape == (B,) and picked.dtype == torch.float32
    assert torch.equal(mom.view(torch.int64), plain.view(torch.int64))
    assert torch.equal(picked.view(torch.int32), plain[:, 8].sqrt().to(torch.float32).view(torch.int32))
    del wt, plain, mom
    report("row_slices", "f32", f"B={B} N={N}", worst)


# ---------------------------------------------------------------------------------------------------------------- backward
@gpu
@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("N", [33, 2048])
def test_backward_behind_the_wave_per_row_forward(tag, N):
    """Moments (chx_moments_bwd_w) with the forward on the wave-per-row kernel, against torch autograd through the float64 tensor
    expression — inputs and tolerances of tests/test_gpu_moments_weights.py."""
    import cheetah_amd  # noqa: F401
    from cheetah_amd import _ops

    B, dt = 64, TORCH_DT[tag]
    torch.manual_seed(3)
    kw = {"dtype": dt, "device": "cuda"}
    x = (torch.randn(B, N, 7, **kw) * torch.tensor([1e-3, 1e-5, 2e-3, 1e-5, 1e-4, 1e-3, 0.0], **kw)
         + torch.tensor([2e-4, 0, -1e-3, 0, 0, 1e-3, 1.0], **kw)).requires_grad_(True)
    w = torch.rand(B, N, **kw).requires_grad_(True)
    coef = torch.randn(B, 29, dtype=torch.float64, device="cuda") * torch.tensor(
        [1e-3, 1e-3] + [1e3] * 6 + [1e6] * 21, dtype=torch.float64, device="cuda")
    out = _ops.moments(x, w)
    assert out.shape == (B, 29) and out.grad_fn is not None
    ref = _torch_moments(x, w)
    assert torch.allclose(out, ref, rtol=1e-9 if dt == torch.float64 else 1e-5, atol=1e-30)
    gx, gw = torch.autograd.grad((out * coef).sum(), (x, w))
    rx, rw = torch.autograd.grad((ref * coef).sum(), (x, w))
    tol = 1e-9 if dt == torch.float64 else 2e-4
    errs = [float((gw - rw).abs().max() / rw.abs().max())]
    errs += [float((gx[..., j] - rx[..., j]).abs().max() / rx[..., j].abs().max()) for j in range(6)]
    print(f"moments_paths backward_wave_per_row {tag} B={B} N={N}: max gradient error / tolerance {max(errs) / tol:.3g}")
    assert max(errs) < tol, errs
    assert float(gx[..., 6].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- space-charge sizes
SC_MASS, SC_POT, SC_BINS = 510998.95, 8.9875517873681764e9 * 1e-12, (32, 16, 64)


def sc_call(x, w, B, tag):
    """chx_sc_beam_geometry (raw entry point, include/chx.h) on numpy rows x (Bx, N, 7), w (Bw, N) or None, and chx_sc_geometry
    on the same rows' reference moments -> (outputs of the beam kernel, outputs from the reference row, reference, bounds)."""
    import cheetah_amd  # noqa: F401
    from cheetah_amd import _ops

    dt = TORCH_DT[tag]
    kw = {"dtype": dt, "device": "cuda"}
    N = x.shape[1]
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    wt = None if w is None else torch.from_numpy(np.ascontiguousarray(w)).cuda()
    ext, energy, length = torch.tensor([[3.0, 2.5, 4.0]], **kw), torch.tensor([1.0e8], **kw), torch.tensor([0.2], **kw)
    half, cell, scale = (torch.empty(B, 3, **kw) for _ in range(3))
    gamma, dtt = torch.empty(B, **kw), torch.empty(B, **kw)
    extent = torch.empty(B, 3, 2, **kw)
    pot = torch.empty(B, dtype=torch.float64, device="cuda")
    lib = _ops._lib.lib()
    ws_bytes = lib.chx_sc_beam_geometry_workspace_bytes(B, N)
    ws = _ops.workspace(ws_bytes, xt.device)
    _ops.check(lib.chx_sc_beam_geometry(xt.data_ptr(), _ops.ptr(wt), ext.data_ptr(), energy.data_ptr(), length.data_ptr(), SC_MASS,
                                        SC_POT, B, xt.shape[0], 1 if wt is None else wt.shape[0], 1, 1, 1, N, _ops._bins3(SC_BINS),
                                        _ops.dtype_code(dt), half.data_ptr(), cell.data_ptr(), gamma.data_ptr(), dtt.data_ptr(),
                                        scale.data_ptr(), extent.data_ptr(), pot.data_ptr(), ws.data_ptr(), ws_bytes,
                                        _ops.stream_ptr()), "chx_sc_beam_geometry")
    xr = np.broadcast_to(x, (B,) + x.shape[1:])
    wr = None if w is None else np.broadcast_to(w, (B, N))
    ref = mr.reference(xr, wr)
    bnd = mr.bounds(xr, wr, ref)
    mom = torch.from_numpy(ref.astype(np.float64)).cuda()
    want = _ops.sc_geometry(mom, ext, energy, length, SC_MASS, SC_POT, B, SC_BINS)
    got = (half, cell, gamma, dtt, scale, extent, pot)
    return [t.cpu().numpy() for t in got], [t.cpu().numpy() for t in want], ref, bnd


def check_geometry(x, w, B, tag, cap, label):
    """The seven outputs may differ only through the three variances: half, cell (and extent = -+half) within
    4 eps(T) + bound_cov_dd / (2 sigma_d^2) relative, gamma and dt the same bits, scale and pot_scale to the same relative bound
    (three times for the cell volume); non-finite entries at identical positions. -> the largest error / bound."""
    got, want, ref, bnd = sc_call(x, w, B, tag)
    mr.check_caps(ref, bnd, cap, label)
    cols = [8, 8 + 11, 8 + 18]                                    # cov_xx, cov_yy, cov_tautau
    assert cols == [mr.DIAG[0], mr.DIAG[2], mr.DIAG[4]]
    eps = float(np.finfo(mr.NP_DT[tag]).eps)
    rel = 4.0 * eps + bnd[:, cols] / (2.0 * ref[:, cols].astype(np.float64))            # (B, 3)
    names = ("half", "cell", "gamma", "dt", "scale", "extent", "pot_scale")
    for name, g, r in zip(names, got, want):
        assert g.shape == r.shape and g.dtype == r.dtype, name
        assert (np.isfinite(g) == np.isfinite(r)).all(), (label, name, g, r)
    worst = 0.0

    def within(name, g, r, tol):
        nonlocal worst
        fin = np.isfinite(r)
        ratio = np.abs(g.astype(np.float64) - r.astype(np.float64))[fin] / (np.broadcast_to(tol, r.shape)[fin] * np.abs(r.astype(np.float64))[fin])
        if ratio.size:
            worst = max(worst, float(ratio.max()))
            assert float(ratio.max()) <= 1.0, (label, name, float(ratio.max()), g, r)

    within("half", got[0], want[0], rel)
    within("cell", got[1], want[1], rel)
    within("extent", got[5], want[5], rel[:, :, None])
    within("scale", got[4], want[4], rel)
    within("pot_scale", got[6], want[6], 3.0 * rel.max(axis=1))
    for k in (2, 3):
        assert got[k].tobytes() == want[k].tobytes(), (label, names[k])
    return worst


@gpu
@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("weights", ["absent", "present"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N", [1000, 5000])
@pytest.mark.parametrize("name", mr.BEAMS)
def test_space_charge_beam_sizes(name, N, B, weights, tag):
    """The grid geometry of chx_sc_beam_geometry (its own 8-sum reduction, sc_sigma_kernel) against chx_sc_geometry on the
    reference's moments of the same rows. `dead_outlier_slot0`: a dead particle 1e8 sigma away in slot 0 — sums centred on
    particle 0 lose the variance there (negative, a NaN grid); the centre is the weighted mean of the first 16 particles."""
    x, w = stack(name, B, N, tag)
    worst = check_geometry(x, w if weights == "present" else None, B, tag, CAP[name], f"{name} ({B}, {N}) weights {weights}")
    report("sc_beam_geometry", tag, f"B={B} N={N} {name} weights {weights}", worst)


@gpu
@pytest.mark.parametrize("tag", DTYPES)
@pytest.mark.parametrize("shared", ["particles", "weights"])
def test_space_charge_beam_sizes_with_a_shared_input(shared, tag):
    """B = 3 with the particles or the weights shared by the rows: the centre is formed from the row's own copy of each."""
    B, N = 3, 1000
    x, w = stack("dead_outlier_slot0", B, N, tag)
    if shared == "particles":
        x = x[:1]
        w[:, 0] = 0.0
    else:
        w = w[:1]
    worst = check_geometry(x, w, B, tag, 1e-6, f"dead_outlier_slot0, shared {shared}")
    report("sc_beam_geometry", tag, f"B={B} N={N} dead_outlier_slot0 shared {shared}", worst)
