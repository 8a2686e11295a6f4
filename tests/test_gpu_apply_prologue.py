"""The apply kernels' prologues — how a workgroup finds its batch row and tile, when its kernel arguments and its map reach scalar
registers (the column passes of chx_coltile.hip take their arguments preloaded with the wave) — may not change a bit of any result:
chx_track_elementwise is held to chx_track_fused and chx_apply_affine7 to the CPU oracle's fma chain, on the integer view of the
arrays, with B == 1 and B > 1 (per-row maps: both sides of the division that finds the batch row), a shared input, E = 1, 3 and 4
(pass 0 with the entering and the leaving pass right behind it), sizes around a multiple of 512 rows and on both sides of the 8 MiB,
14.7 MiB and 28 MiB thresholds, both dtypes, and rows holding NaN, inf and -0.0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ENERGY = 1e8
K = 1200  # 512 * K rows: whole tiles in both dtypes, inside the column-tiled range
MIB = 1024 * 1024
COLTILE_MIN = 8 * MIB                  # kColTileMinBytes: column tiles from this size on
SMALL_BEAM = 14 * MIB + 700 * 1024     # kSmallBeamBytes: the wave-staged kernel up to this size
L2_RESIDENT = 28 * MIB                 # kL2ResidentBytes: L2-allocating loads up to this size


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from cheetah_amd import _lib, _ops

    _lib.lib()
    return _ops


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def rows_below(nbytes, dtype):
    """the largest number of rows whose bytes do not exceed nbytes"""
    return nbytes // (7 * np.dtype(dtype).itemsize)


def threshold_sizes(dtype):
    """rows on both sides of the three size thresholds and around a multiple of 512"""
    r8, r14, r28 = rows_below(COLTILE_MIN, dtype), rows_below(SMALL_BEAM, dtype), rows_below(L2_RESIDENT, dtype)
    return [r8, r8 + 1, r14, r14 + 1, r28, r28 + 1, 512 * K - 1, 512 * K, 512 * K + 1]


_beams = {}


def beam_rows(B, N, dtype, seed=0):
    key = (np.dtype(dtype).name, seed)
    if key not in _beams or _beams[key].shape[0] < B * N:
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal((max(B * N, 1_100_000), 7)) * 1e-3).astype(dtype)
        x[:, 6] = 1
        _beams[key] = x
    return _beams[key][: B * N].reshape(B, N, 7).copy()


def fodo_maps(oracle, E, dtype, first=0):
    f = np.float32
    cell = [oracle.build_rmatrix("quadrupole", [f(0.2), f(4.2), 0, 0, 0], ENERGY), oracle.build_rmatrix("drift", [f(0.8)], ENERGY),
            oracle.build_rmatrix("quadrupole", [f(0.2), f(-4.2), 0, 0, 0], ENERGY), oracle.build_rmatrix("drift", [f(0.8)], ENERGY)]
    return np.stack([cell[(first + e) % 4].reshape(1, 7, 7) for e in range(E)]).astype(dtype)


def dense_maps(E, BR, dtype, seed):
    """every one of columns 0..5 changes in every row, the maps' seventh column is set too, every batch row has its own map"""
    rng = np.random.default_rng(seed)
    maps = np.tile(np.eye(7), (E, BR, 1, 1)).astype(dtype)
    maps[:, :, :6, :6] += (rng.standard_normal((E, BR, 6, 6)) * 0.1).astype(dtype)
    maps[:, :, :6, 6] = (rng.standard_normal((E, BR, 6)) * 1e-4).astype(dtype)
    return maps


def special_rows(N, dtype, seed=5):
    """NaN (two payloads), +inf, -inf and -0.0: first and last rows of tiles, rows in the middle of a wave, the last rows"""
    x = beam_rows(1, N, dtype, seed=seed)[0]
    u = np.uint32 if dtype == np.float32 else np.uint64
    nan_a = np.array([0x7FC00001 if dtype == np.float32 else 0x7FF8000000000001], dtype=u).view(dtype)[0]
    nan_b = np.array([0xFFC12345 if dtype == np.float32 else 0xFFF8000000012345], dtype=u).view(dtype)[0]
    vals = [nan_a, nan_b, dtype(np.inf), dtype(-np.inf), dtype(-0.0)]
    rows = [0, 1, 5, 63, 64, 255, 256, 511, 512, 1000, 4097, N // 2, N - 513, N - 2, N - 1]
    for i, r in enumerate(rows):
        for c in range(7):
            if (i + c) % 3 == 0:
                x[r, c] = vals[(i + 2 * c) % 5]
    x[7, :] = dtype(-0.0)
    x[8, 1] = nan_a
    x[9, 5] = dtype(np.inf)
    return x


def track_checked(ops, x, maps):
    """elementwise and fused results of the same device inputs; the input must come back untouched"""
    xt, mt = torch.from_numpy(x).cuda(), torch.from_numpy(maps).cuda()
    before = xt.clone()
    got = ops.track_elementwise(xt, mt, fused=False)
    torch.cuda.synchronize()
    assert same_bits(xt, before), "x_in was written"
    want = ops.track_elementwise(xt, mt, fused=True)
    torch.cuda.synchronize()
    return got, want


def oracle_chain(oracle, x, maps):
    y = x
    for e in range(maps.shape[0]):
        y = oracle.apply(y, maps[e], mode=1)  # the device's fma chain
    return y


# ---- chx_track_elementwise against chx_track_fused ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [1, 3, 4])
@pytest.mark.parametrize("i", range(9))
def test_one_beam_sizes_and_pass_counts(ops, oracle, dtype, E, i):
    """B == 1: no division. E = 3: pass 0, entering pass, leaving pass; E = 4: one column pass between them"""
    N = threshold_sizes(dtype)[i]
    x, maps = beam_rows(1, N, dtype)[0], fodo_maps(oracle, E, dtype)
    got, want = track_checked(ops, x, maps)
    assert same_bits(got, want)
    if E == 4:
        assert same_bits(got.cpu(), torch.from_numpy(oracle_chain(oracle, x[None], maps)[0]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [1, 3, 4])
@pytest.mark.parametrize("N", [100_004, 300_004, 512 * 700, 512 * 700 + 4])
@pytest.mark.parametrize("Bx,BR", [(3, 3), (3, 1), (1, 3)])  # (1, 3): one beam shared by the batch
def test_batches_take_the_division(ops, oracle, dtype, E, N, Bx, BR):
    B = 3
    x = beam_rows(Bx, N, dtype, seed=10 + Bx)
    maps = dense_maps(E, BR, dtype, 11 + BR) if BR > 1 else fodo_maps(oracle, E, dtype)
    got, want = track_checked(ops, x if Bx == B else x[0], maps)
    assert got.shape == (B, N, 7) and same_bits(got, want)
    if N == 300_004 and E == 4:
        assert same_bits(got.cpu(), torch.from_numpy(oracle_chain(oracle, x, maps)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [1, 3, 4])
@pytest.mark.parametrize("i", [1, 3, 5, 8])
def test_nan_inf_and_negative_zero_elementwise(ops, oracle, dtype, E, i):
    N = threshold_sizes(dtype)[i] + 77
    x, maps = special_rows(N, dtype), fodo_maps(oracle, E, dtype, first=1)
    got, want = track_checked(ops, x, maps)
    assert same_bits(got, want)


# ---- chx_apply_affine7 against the oracle's fma chain ------------------------------------------------------------------------

def apply_checked(ops, oracle, x, tm):
    """x: (Bx, N, 7), tm: (BR, 7, 7); the oracle broadcasts like the device"""
    xt, mt = torch.from_numpy(x).cuda(), torch.from_numpy(tm).cuda()
    before = xt.clone()
    got = ops.apply_map(xt if x.shape[0] > 1 else xt[0], mt if tm.shape[0] > 1 else mt[0])
    torch.cuda.synchronize()
    assert same_bits(xt, before), "x_in was written"
    B = max(x.shape[0], tm.shape[0])
    ref = oracle.apply(np.broadcast_to(x, (B,) + x.shape[1:]).copy(), tm, mode=1)
    return got.reshape(B, x.shape[1], 7).cpu(), torch.from_numpy(np.ascontiguousarray(ref))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", range(9))
def test_apply_one_beam(ops, oracle, dtype, i):
    N = threshold_sizes(dtype)[i]
    got, ref = apply_checked(ops, oracle, beam_rows(1, N, dtype, seed=1), dense_maps(1, 1, dtype, 21)[0])
    assert same_bits(got, ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_beam_that_streams_from_hbm(ops, oracle, dtype):
    """above 96 MiB the single-wave workgroups take the pass"""
    N = rows_below(96 * MIB, dtype) + 513
    got, ref = apply_checked(ops, oracle, beam_rows(1, N, dtype, seed=2), fodo_maps(oracle, 1, dtype)[0])
    assert same_bits(got, ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [100_004, 300_004, 300_001, 512 * 700])
@pytest.mark.parametrize("Bx,BR", [(3, 3), (3, 1), (1, 3)])
def test_apply_batches(ops, oracle, dtype, N, Bx, BR):
    got, ref = apply_checked(ops, oracle, beam_rows(Bx, N, dtype, seed=3), dense_maps(1, BR, dtype, 22 + BR)[0])
    assert same_bits(got, ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("i", [0, 3, 5])
def test_apply_nan_inf_and_negative_zero(ops, oracle, dtype, i):
    """Integer views against the oracle for every value that is not a NaN there, a NaN wherever the oracle has one, and bit for bit
    (payloads included) what chx_track_fused gives for the same single map. A NaN's payload is not compared with the oracle's: the
    CPU's fma and the GPU's do not hand on the same operand's payload, so the two sides disagree in the payload bits of some NaNs and
    in nothing else (measured on MI355X: in each of the six cases 24 values differ between
    device and oracle, all 24 NaN on both sides; the same 24 with the library of the commit before the prologues were touched)."""
    N = threshold_sizes(dtype)[i]
    x, tm = special_rows(N, dtype)[None], fodo_maps(oracle, 1, dtype, first=1)
    got, ref = apply_checked(ops, oracle, x, tm[0])
    nan = torch.isnan(ref)
    assert bool(torch.equal(torch.isnan(got), nan))
    assert bool(torch.equal(bits(got)[~nan], bits(ref)[~nan]))
    fused = ops.track_elementwise(torch.from_numpy(x[0]).cuda(), torch.from_numpy(tm).cuda(), fused=True)
    torch.cuda.synchronize()
    assert same_bits(got[0], fused.cpu())
