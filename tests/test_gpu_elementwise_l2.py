"""chx_track_elementwise on beams that fit the XCDs' L2s: passes 1..E-1 run in place with L2-allocating loads
(apply_tile_kernel MODE 3) between 14.7 MiB and 28 MiB of particles, the neighbouring sizes keep the other kernels.
Every result must equal chx_track_fused (same fma chain, one launch) and the CPU oracle bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL_BEAM_BYTES = 14 * 1024 * 1024 + 700 * 1024  # up to here: the wave-staged kernel
L2_BEAM_BYTES = 28 * 1024 * 1024  # up to here: MODE 3


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from cheetah_amd import _lib, _ops

    _lib.lib()
    return _ops


def make(B, N, E, BR, dtype, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, N, 7)) * 1e-3).astype(dtype)
    x[..., 6] = 1
    maps = np.tile(np.eye(7), (E, BR, 1, 1)).astype(dtype)
    maps[:, :, :6, :6] += (rng.standard_normal((E, BR, 6, 6)) * 0.1).astype(dtype)
    return x, maps


def run(ops, x, maps, fused):
    return ops.track_elementwise(torch.from_numpy(x).cuda(), torch.from_numpy(maps).cuda(), fused=fused).cpu().numpy()


def oracle_track(oracle, x, maps):
    y = x
    for e in range(maps.shape[0]):
        y = oracle.apply(y, maps[e], mode=1)  # the device's fma chain
    return y


ROWS_F32 = L2_BEAM_BYTES // 28


@pytest.mark.parametrize(
    "N",
    [1_000_000, 999_999, 512 * 8 * 200 - 1, 512 * 8 * 200 + 1, SMALL_BEAM_BYTES // 28, SMALL_BEAM_BYTES // 28 + 1,
     ROWS_F32, ROWS_F32 + 1],
)
@pytest.mark.parametrize("E", [1, 2, 3])
def test_f32_sizes_and_pass_counts(ops, oracle, N, E):
    x, maps = make(1, N, E, 1, np.float32, seed=N + E)
    a = run(ops, x[0], maps, fused=False)
    assert np.array_equal(a, run(ops, x[0], maps, fused=True))
    if N in (1_000_000, ROWS_F32 + 1) and E == 3:
        assert np.array_equal(a, oracle_track(oracle, x, maps)[0])


@pytest.mark.parametrize("N", [500_000, 499_999, 1_000_000])  # fp64: 28 MB and 56 MB of particles
@pytest.mark.parametrize("E", [2, 3])
def test_f64(ops, oracle, N, E):
    x, maps = make(1, N, E, 1, np.float64, seed=N + 7 * E)
    a = run(ops, x[0], maps, fused=False)
    assert np.array_equal(a, run(ops, x[0], maps, fused=True))
    assert np.array_equal(a, oracle_track(oracle, x, maps)[0])


@pytest.mark.parametrize("Bx,BR", [(3, 1), (3, 3), (1, 3)])  # (1, 3): one beam shared by the batch
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batches(ops, oracle, Bx, BR, dtype):
    B, N, E = 3, 300_001, 3  # 25 MB of fp32 rows, 50 MB of fp64 rows
    x, maps = make(Bx, N, E, BR, dtype, seed=11 + Bx + BR)
    a = run(ops, x if Bx == B else x[0], maps, fused=False)
    assert a.shape == (B, N, 7)
    assert np.array_equal(a, run(ops, x if Bx == B else x[0], maps, fused=True))
    assert np.array_equal(a, oracle_track(oracle, x, maps))


def test_back_to_back_calls(ops):
    x, maps = make(1, 1_000_000, 3, 1, np.float32, seed=5)
    xt, mt = torch.from_numpy(x[0]).cuda(), torch.from_numpy(maps).cuda()
    a = ops.track_elementwise(xt, mt)
    b = ops.track_elementwise(a, mt)
    ref = ops.track_elementwise(ops.track_elementwise(xt, mt, fused=True), mt, fused=True)
    torch.cuda.synchronize()
    assert torch.equal(b, ref)


def test_two_streams(ops):
    xa, ma = make(1, 1_000_000, 3, 1, np.float32, seed=21)
    xb, mb = make(1, 900_001, 2, 1, np.float32, seed=22)
    ta, tb = torch.from_numpy(xa[0]).cuda(), torch.from_numpy(xb[0]).cuda()
    tma, tmb = torch.from_numpy(ma).cuda(), torch.from_numpy(mb).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = ops.track_elementwise(ta, tma)
    with torch.cuda.stream(s2):
        b = ops.track_elementwise(tb, tmb)
    torch.cuda.synchronize()
    assert torch.equal(a, ops.track_elementwise(ta, tma, fused=True))
    assert torch.equal(b, ops.track_elementwise(tb, tmb, fused=True))
