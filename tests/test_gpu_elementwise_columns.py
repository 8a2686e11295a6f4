"""chx_track_elementwise with E >= 3 on beams of 8 MiB and more, every batch row 16-byte aligned: passes 1..E-1 keep each full
tile of the output transposed ([7][512] fp32, [7][256] fp64) and a wave stores a column only if one of its lanes holds other
bits than it loaded (coltile_edge_kernel / coltile_pass_kernel). The output must be BIT FOR BIT what chx_track_fused computes
(same fma chain, every row computed and stored, one launch) and what the CPU oracle's chain gives, for every input: all
comparisons are made on the integer view of the arrays. Sizes below the threshold, unaligned batch rows and E < 3 take the
row passes and are held to the same results."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 1200  # 512 * K rows: 17.2 MB fp32, 34.4 MB fp64 — inside the column-tiled range, whole tiles in both dtypes
DTYPES = [np.float32, np.float64]
ENERGY = 1e8


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


_beams = {}


def beam_rows(B, N, dtype, seed=0):
    """(B, N, 7) rows of a beam-sized spread, seventh coordinate 1; one generated block per dtype and seed, cut to size"""
    key = (np.dtype(dtype).name, seed)
    if key not in _beams or _beams[key].shape[0] < B * N:
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal((max(B * N, 1_000_000), 7)) * 1e-3).astype(dtype)
        x[:, 6] = 1
        _beams[key] = x
    return _beams[key][: B * N].reshape(B, N, 7).copy()


def fodo_maps(oracle, E, dtype, first=0):
    """the benchmark's cell: Quadrupole(0.2, k1=4.2), Drift(0.8), Quadrupole(0.2, k1=-4.2), Drift(0.8), (E, 1, 7, 7)"""
    f = np.float32
    cell = [oracle.build_rmatrix("quadrupole", [f(0.2), f(4.2), 0, 0, 0], ENERGY), oracle.build_rmatrix("drift", [f(0.8)], ENERGY),
            oracle.build_rmatrix("quadrupole", [f(0.2), f(-4.2), 0, 0, 0], ENERGY), oracle.build_rmatrix("drift", [f(0.8)], ENERGY)]
    return np.stack([cell[(first + e) % 4].reshape(1, 7, 7) for e in range(E)]).astype(dtype)


def identity_maps(E, dtype):
    return np.tile(np.eye(7), (E, 1, 1, 1)).astype(dtype)


def dense_maps(E, BR, dtype, seed, affine=False):
    """every one of columns 0..5 changes in every row; affine: the maps' seventh column is set too (a corrector's kick)"""
    rng = np.random.default_rng(seed)
    maps = np.tile(np.eye(7), (E, BR, 1, 1)).astype(dtype)
    maps[:, :, :6, :6] += (rng.standard_normal((E, BR, 6, 6)) * 0.1).astype(dtype)
    if affine:
        maps[:, :, :6, 6] = (rng.standard_normal((E, BR, 6)) * 1e-4).astype(dtype)
    return maps


def corrector_maps(oracle, E, dtype):
    """drifts with a kick in column 6 of px or py: all else of a drift stays, the seventh column of the map is not zero"""
    f = np.float32
    kinds = [("hcor", 9e-5), ("drift", None), ("vcor", -1e-4), ("drift", None)]
    out = []
    for e in range(E):
        kind, angle = kinds[e % 4]
        par = [f(0.3)] if angle is None else [f(0.3), f(angle)]
        out.append(oracle.build_rmatrix(kind, par, ENERGY).reshape(1, 7, 7))
    return np.stack(out).astype(dtype)


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


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1_000_000, 512 * K, 512 * K - 1, 512 * K + 1, 300, 513])
@pytest.mark.parametrize("E", [1, 2, 3, 4, 5, 6, 24])
def test_fodo_cell_sizes_and_pass_counts(ops, oracle, dtype, N, E):
    x, maps = beam_rows(1, N, dtype)[0], fodo_maps(oracle, E, dtype)
    got, want = track_checked(ops, x, maps)
    assert same_bits(got, want)
    if N == 512 * K + 1 and E == 6:
        ref = torch.from_numpy(oracle_chain(oracle, x[None], maps)[0])
        assert same_bits(got.cpu(), ref)


@pytest.mark.parametrize("E", [4, 9])
def test_f32_beam_larger_than_the_l2s(ops, oracle, E):
    """above 28 MiB the column passes load non-temporally (fp64 reaches that size at 1e6 rows above)"""
    N = 1_300_003
    x, maps = beam_rows(1, N, np.float32, seed=3)[0], fodo_maps(oracle, E, np.float32)
    got, want = track_checked(ops, x, maps)
    assert same_bits(got, want)
    assert same_bits(got.cpu(), torch.from_numpy(oracle_chain(oracle, x[None], maps)[0]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["identity", "dense", "dense_affine", "correctors"])
def test_maps(ops, oracle, dtype, kind):
    N, E = 700_001, 7
    maps = {"identity": lambda: identity_maps(E, dtype), "dense": lambda: dense_maps(E, 1, dtype, 3),
            "dense_affine": lambda: dense_maps(E, 1, dtype, 4, affine=True), "correctors": lambda: corrector_maps(oracle, E, dtype)}[kind]()
    x = beam_rows(1, N, dtype, seed=1)[0]
    got, want = track_checked(ops, x, maps)
    assert same_bits(got, want)
    ref = torch.from_numpy(oracle_chain(oracle, x[None], maps)[0])
    assert same_bits(got.cpu(), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_different_map_per_batch_row(ops, oracle, dtype):
    B, N, E = 3, 300_004, 6
    maps = np.concatenate([fodo_maps(oracle, E, dtype), fodo_maps(oracle, E, dtype, first=1), dense_maps(E, 1, dtype, 9, affine=True)], axis=1)
    assert maps.shape == (E, B, 7, 7)
    x = beam_rows(B, N, dtype, seed=2)
    got, want = track_checked(ops, x, maps)
    assert got.shape == (B, N, 7) and same_bits(got, want)
    ref = torch.from_numpy(oracle_chain(oracle, x, maps))
    assert same_bits(got.cpu(), ref)


def special_rows(N, dtype):
    """NaN (two payloads), +inf, -inf and -0.0 in a handful of rows and columns: first and last rows of tiles, rows in the middle
    of a wave, the rows of the last (partial) tile; in columns a drift leaves alone (px, py, delta, the 1) and in ones it changes"""
    x = beam_rows(1, N, dtype, seed=5)[0]
    u = np.uint32 if dtype == np.float32 else np.uint64
    nan_a = np.array([0x7FC00001 if dtype == np.float32 else 0x7FF8000000000001], dtype=u).view(dtype)[0]
    nan_b = np.array([0xFFC12345 if dtype == np.float32 else 0xFFF8000000012345], dtype=u).view(dtype)[0]
    vals = [nan_a, nan_b, dtype(np.inf), dtype(-np.inf), dtype(-0.0)]
    rows = [0, 1, 5, 63, 64, 255, 256, 511, 512, 1000, 4097, N // 2, N - 513, N - 2, N - 1]
    for i, r in enumerate(rows):
        for c in range(7):
            if (i + c) % 3 == 0:
                x[r, c] = vals[(i + 2 * c) % 5]
    x[7, :] = dtype(-0.0)      # a row of negative zeros: 0 * x and 1 * x + (-0) keep or lose the sign exactly as in the fused chain
    x[8, 1] = nan_a            # NaN in px alone: a drift spreads it to x and leaves the other columns of the row
    x[9, 5] = dtype(np.inf)    # inf in delta alone: a drift takes it to tau
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["drifts", "fodo"])
def test_nan_inf_and_negative_zero(ops, oracle, dtype, kind):
    N, E = 512 * K + 77, 8
    maps = fodo_maps(oracle, E, dtype)
    if kind == "drifts":
        maps = np.stack([maps[1]] * E)
    x = special_rows(N, dtype)
    got, want = track_checked(ops, x, maps)
    assert same_bits(got, want)
    # rows without special values are what they are in a beam that has none
    clean = beam_rows(1, N, dtype, seed=5)[0]
    plain, _ = track_checked(ops, clean, maps)
    untouched = torch.from_numpy(np.all(bits_np(x) == bits_np(clean), axis=1)).cuda()
    assert same_bits(got[untouched], plain[untouched])


def bits_np(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["fodo", "dense_affine"])
def test_seventh_coordinate_not_one(ops, oracle, dtype, kind):
    N, E = 512 * K + 5, 5
    x = beam_rows(1, N, dtype, seed=6)[0]
    x[:, 6] = (np.random.default_rng(7).standard_normal(N) * 3).astype(dtype)
    maps = fodo_maps(oracle, E, dtype) if kind == "fodo" else dense_maps(E, 1, dtype, 8, affine=True)
    got, want = track_checked(ops, x, maps)
    assert same_bits(got, want)
    assert same_bits(got.cpu(), torch.from_numpy(oracle_chain(oracle, x[None], maps)[0]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [300_001, 300_004])  # fp32 batch rows of 300 001 x 28 bytes are not 16-byte aligned, of 300 004 are
@pytest.mark.parametrize("Bx,BR", [(3, 1), (3, 3), (1, 3)])  # (1, 3): one beam shared by the batch
def test_batches(ops, oracle, dtype, N, Bx, BR):
    B, E = 3, 5
    x = beam_rows(Bx, N, dtype, seed=10 + Bx)
    maps = dense_maps(E, BR, dtype, 11 + BR, affine=True) if BR > 1 else fodo_maps(oracle, E, dtype)
    got, want = track_checked(ops, x if Bx == B else x[0], maps)
    assert got.shape == (B, N, 7) and same_bits(got, want)
    if N == 300_004:
        assert same_bits(got.cpu(), torch.from_numpy(oracle_chain(oracle, x, maps)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_result_is_rows_again_for_the_next_kernel_on_the_stream(ops, oracle, dtype):
    """a second call and the moments reduction read the output right behind the call, no synchronisation in between"""
    import cheetah_amd as ca
    from cheetah_amd import sharding

    N, E = 1_000_000, 8
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    beam = ca.ParticleBeam.from_parameters(num_particles=N, dtype=tdt, device="cuda")
    mt = torch.from_numpy(fodo_maps(oracle, E, dtype)).cuda()
    as_beam = lambda p: ca.ParticleBeam(p, beam.energy, particle_charges=beam.particle_charges, species=beam.species)  # noqa: E731
    torch.cuda.synchronize()
    a = ops.track_elementwise(beam.particles, mt)
    mom = sharding.global_moments(as_beam(a))
    b = ops.track_elementwise(a, mt)
    torch.cuda.synchronize()
    fa = ops.track_elementwise(beam.particles, mt, fused=True)
    torch.cuda.synchronize()
    fmom = sharding.global_moments(as_beam(fa))
    fb = ops.track_elementwise(fa, mt, fused=True)
    torch.cuda.synchronize()
    assert same_bits(a, fa) and same_bits(b, fb)
    assert same_bits(mom, fmom)       # the reduction sums in a fixed order: the same rows give the same bits


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_capture_and_two_replays(ops, oracle, dtype):
    N, E = 512 * K + 3, 9
    x1, x2 = beam_rows(1, N, dtype, seed=12)[0], beam_rows(1, N, dtype, seed=13)[0]
    mt = torch.from_numpy(fodo_maps(oracle, E, dtype)).cuda()
    static_in = torch.from_numpy(x1).cuda()
    eager1 = ops.track_elementwise(static_in, mt).clone()
    eager2 = ops.track_elementwise(torch.from_numpy(x2).cuda(), mt).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            out = ops.track_elementwise(static_in, mt)
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager1)
    static_in.copy_(torch.from_numpy(x2))
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager2)
    assert same_bits(static_in.cpu(), torch.from_numpy(x2))
