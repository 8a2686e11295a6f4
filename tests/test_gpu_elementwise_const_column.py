"""chx_track_elementwise with scratch: one word per column tile says that the tile's seventh coordinate is 1 in every row, and
the column passes of such a tile do not read that column (coltile_enter_kernel writes the words, coltile_pass_flag_kernel reads
and withdraws them). Whatever the beam and the maps hold,
the output must be BIT FOR BIT what chx_track_fused computes, what the CPU oracle's chain gives and what the same call without
scratch gives (NaN payloads included: every comparison is made on the integer view), and the words left in the scratch must say
what the tiles held when the last column pass had run.

Sizes: the smallest that take the column path (8 MiB; 299 593 fp32 rows are 4 bytes short of it and take the row passes, 299 594
is the first that does not), a whole number of tiles, a partial last tile; the same above 14.7 MiB, where pass 0 in front of the
column passes is another kernel (apply_tile_kernel, not apply_wave_kernel); one beam above the 28 MiB from which the column passes
load non-temporally."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ENERGY = 1e8
TP = {np.float32: 512, np.float64: 256}            # rows per tile (tile_cfg)
MIN_BYTES = 8 * 1024 * 1024                        # kColTileMinBytes
SMALL_BEAM_BYTES = 14 * 1024 * 1024 + 700 * 1024    # kSmallBeamBytes
# rows: first size of the column path, whole tiles, a partial last tile (the issue's sizes; see the docstring for 299 593)
SMALL = {np.float32: [299_593, 299_594, 300_032, 300_069], np.float64: [149_797, 150_016, 150_053]}
# the same above kSmallBeamBytes (another pass 0), and one beam of more than 28 MiB (nt loads)
MID = {np.float32: [1076 * 512, 1076 * 512 + 37], np.float64: [1076 * 256, 1076 * 256 + 37]}
LARGE = {np.float32: 2050 * 512 + 37, np.float64: 2050 * 256 + 37}
# two batch rows: whole tiles / a partial last tile, 16-byte aligned batch rows / batch rows that are not aligned (row passes) /
# whole tiles and a partial last tile above kSmallBeamBytes
BATCH = {np.float32: [150_016, 150_020, 150_022, 275_968, 275_972], np.float64: [75_008, 75_010, 75_011, 137_984, 137_988]}


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
        x = (rng.standard_normal((max(B * N, 1_100_000), 7)) * 1e-3).astype(dtype)
        x[:, 6] = 1
        _beams[key] = x
    return _beams[key][: B * N].reshape(B, N, 7).copy()


def fodo_maps(oracle, E, dtype, first=0):
    f = np.float32
    cell = [oracle.build_rmatrix("quadrupole", [f(0.2), f(4.2), 0, 0, 0], ENERGY), oracle.build_rmatrix("drift", [f(0.8)], ENERGY),
            oracle.build_rmatrix("quadrupole", [f(0.2), f(-4.2), 0, 0, 0], ENERGY), oracle.build_rmatrix("drift", [f(0.8)], ENERGY)]
    return np.stack([cell[(first + e) % 4].reshape(1, 7, 7) for e in range(E)]).astype(dtype)


def affine_maps(E, BR, dtype, seed):
    """columns 0..5 change in every row and R[i][6] != 0: the constant enters the arithmetic; the last row stays (0,...,0,1)"""
    rng = np.random.default_rng(seed)
    maps = np.tile(np.eye(7), (E, BR, 1, 1)).astype(dtype)
    maps[:, :, :6, :6] += (rng.standard_normal((E, BR, 6, 6)) * 0.1).astype(dtype)
    maps[:, :, :6, 6] = (rng.standard_normal((E, BR, 6)) * 1e-4).astype(dtype)
    return maps


def last_row_map(BR, dtype, seed):
    """a map whose last row is not e6: the seventh coordinate of every row becomes something else"""
    rng = np.random.default_rng(seed)
    m = np.tile(np.eye(7), (BR, 1, 1)).astype(dtype)
    m[:, 6, :6] = (rng.standard_normal((BR, 6)) * 0.5).astype(dtype)
    m[:, 6, 6] = dtype(1.25)
    return m


def oracle_chain(oracle, x, maps):
    y = x
    for e in range(maps.shape[0]):
        y = oracle.apply(y, maps[e], mode=1)  # the device's fma chain
    return y


def raw_call(ops, xt, mt, B, fill):
    """chx_track_elementwise through ctypes. fill: None (scratch == NULL) or the byte the scratch is filled with before the call.
    Returns the output and the scratch as int32 words (None where the library asks for none)."""
    from cheetah_amd import _lib

    lib = _lib.lib()
    E, BR = mt.shape[0], mt.shape[1]
    Bx, N = (xt.shape[0], xt.shape[1]) if xt.dim() == 3 else (1, xt.shape[0])
    code = ops.dtype_code(xt.dtype)
    nbytes = lib.chx_track_elementwise_scratch_bytes(B, N, code)
    scratch = None
    if fill is not None and nbytes:
        assert nbytes % 4 == 0
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=xt.device)
    out = torch.empty((B, N, 7), dtype=xt.dtype, device=xt.device)
    ops.check(lib.chx_track_elementwise(ops.ptr(xt), ops.ptr(mt), ops.ptr(out), None if scratch is None else ops.ptr(scratch),
                                        E, B, Bx, BR, N, code, ops.stream_ptr()), "chx_track_elementwise")
    torch.cuda.synchronize()
    return out, (None if scratch is None else scratch.view(torch.int32).cpu().numpy())


def run_every_way(ops, oracle, x, maps, B=None, with_oracle=True):
    """x: (Bx, N, 7) or (N, 7) numpy rows. The wrapper's result against the fused chain, against the raw call without scratch and
    with scratch filled with 0x00 and with 0xFF, and against the CPU chain. Returns (result, flags [B][tiles] or None)."""
    xt, mt = torch.from_numpy(x).cuda(), torch.from_numpy(maps).cuda()
    Bx = x.shape[0] if x.ndim == 3 else 1
    B = B or max(Bx, maps.shape[1])
    N = x.shape[-2]
    before = xt.clone()
    got = ops.track_elementwise(xt, mt, fused=False)
    torch.cuda.synchronize()
    want = ops.track_elementwise(xt, mt, fused=True)
    torch.cuda.synchronize()
    got, want = got.reshape(B, N, 7), want.reshape(B, N, 7)
    assert same_bits(got, want), "wrapper (scratch from torch.empty) differs from the fused chain"
    plain, none = raw_call(ops, xt, mt, B, None)
    assert none is None and same_bits(plain, want), "scratch == NULL differs from the fused chain"
    zeros, f0 = raw_call(ops, xt, mt, B, 0x00)
    assert same_bits(zeros, want), "scratch pre-filled with 0x00 differs"
    ones, f1 = raw_call(ops, xt, mt, B, 0xFF)
    assert same_bits(ones, want), "scratch pre-filled with 0xFF differs"
    assert same_bits(xt, before), "x_in was written"
    if with_oracle:
        xb = x if x.ndim == 3 else x[None]
        ref = torch.from_numpy(oracle_chain(oracle, np.broadcast_to(xb, (B, N, 7)).copy(), maps))
        assert same_bits(got.cpu(), ref), "differs from the CPU chain"
    if f1 is None:
        return got, None
    tiles = -(-N // TP[x.dtype.type])
    assert f0.shape == (B * tiles,)
    return got, (f0.reshape(B, tiles), f1.reshape(B, tiles))


def column_path(B, N, dtype, E):
    row_bytes = N * 7 * np.dtype(dtype).itemsize
    return E >= 3 and B * row_bytes >= MIN_BYTES and (B == 1 or row_bytes % 16 == 0)


def check_flags(flags, N, dtype, expect_zero=()):
    """every full tile's word is 1 except those in expect_zero ((b, tile) pairs); the same whatever the scratch held before"""
    f0, f1 = flags
    full = N // TP[dtype]
    want = np.ones((f0.shape[0], full), dtype=np.int32)
    for b, t in expect_zero:
        want[b, t] = 0
    assert np.array_equal(f0[:, :full], want), f"flags (scratch was 0x00): tiles {np.argwhere(f0[:, :full] != want)[:8].tolist()} differ"
    assert np.array_equal(f1[:, :full], want), f"flags (scratch was 0xFF): tiles {np.argwhere(f1[:, :full] != want)[:8].tolist()} differ"


def sizes(dtype):
    return SMALL[dtype] + MID[dtype] + [LARGE[dtype]]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["fodo", "affine"])
@pytest.mark.parametrize("E", [3, 4, 7])
def test_ordinary_beam(ops, oracle, dtype, kind, E):
    """column 6 is 1 and stays 1: every full tile's word is 1 after the call, at every size and pass count"""
    assert MID[dtype][0] * 7 * np.dtype(dtype).itemsize > SMALL_BEAM_BYTES > SMALL[dtype][-1] * 7 * np.dtype(dtype).itemsize
    for N in sizes(dtype):
        x = beam_rows(1, N, dtype)[0]
        maps = fodo_maps(oracle, E, dtype) if kind == "fodo" else affine_maps(E, 1, dtype, 3)
        _, flags = run_every_way(ops, oracle, x, maps, with_oracle=(E == 7 or N == SMALL[dtype][-1]))
        if column_path(1, N, dtype, E):
            check_flags(flags, N, dtype)
        else:
            assert N == 299_593


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Bx,BR", [(2, 1), (2, 2), (1, 2)])   # (1, 2): one beam shared by the batch
@pytest.mark.parametrize("E", [3, 4])
def test_batches(ops, oracle, dtype, Bx, BR, E):
    for N in BATCH[dtype]:
        x = beam_rows(Bx, N, dtype, seed=1)
        maps = affine_maps(E, BR, dtype, 5) if BR > 1 else fodo_maps(oracle, E, dtype)
        _, flags = run_every_way(ops, oracle, x if Bx == 2 else x[0], maps, B=2)
        assert column_path(2, N, dtype, E) == (N not in (150_022, 75_011))
        if column_path(2, N, dtype, E):
            check_flags(flags, N, dtype)


def special_values(dtype):
    u = np.uint32 if dtype == np.float32 else np.uint64
    nan = np.array([0x7FC01234 if dtype == np.float32 else 0x7FF8000000012345], dtype=u).view(dtype)[0]
    return {"two": dtype(2.0), "below_one": np.nextafter(dtype(1), dtype(0)), "minus_zero": dtype(-0.0), "inf": dtype(np.inf), "nan": nan}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("value", ["two", "below_one", "minus_zero", "inf", "nan"])
def test_one_row_with_another_seventh_coordinate(ops, oracle, dtype, value):
    """one row of one tile: that tile's word is 0, every other full tile's is 1 (first, a middle and the last full tile; its first
    and its last row); below and above kSmallBeamBytes"""
    v = special_values(dtype)[value]
    if value == "below_one":
        assert v == (dtype(0.99999994) if dtype == np.float32 else 1 - 2.0 ** -53) and v != 1
    tp = TP[dtype]
    for N, E, kind in [(SMALL[dtype][-1], 4, "fodo"), (MID[dtype][1], 3, "affine")]:
        full = N // tp
        maps = fodo_maps(oracle, E, dtype) if kind == "fodo" else affine_maps(E, 1, dtype, 7)
        for tile in (0, full // 2, full - 1):
            for row in (0, tp - 1):
                x = beam_rows(1, N, dtype, seed=2)[0]
                x[tile * tp + row, 6] = v
                _, flags = run_every_way(ops, oracle, x, maps, with_oracle=(row == 0 and tile == full - 1 and value not in ("inf", "nan")))
                check_flags(flags, N, dtype, expect_zero=[(0, tile)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("at", ["first", "middle", "last"])
def test_map_whose_last_row_is_not_e6(ops, oracle, dtype, at):
    """column 6 changes in the entering pass, in a column pass (the later passes read what it stored) or in the leaving pass"""
    E = 7
    e = {"first": 0, "middle": 3, "last": E - 1}[at]
    for N in (SMALL[dtype][-1], MID[dtype][1], LARGE[dtype]):
        maps = affine_maps(E, 1, dtype, 11)
        maps[e] = last_row_map(1, dtype, 12)
        x = beam_rows(1, N, dtype, seed=3)[0]
        _, flags = run_every_way(ops, oracle, x, maps)
        full = N // TP[dtype]
        # the leaving pass does not touch the words; any earlier pass that makes the column something else leaves 0 in all of them
        check_flags(flags, N, dtype, expect_zero=[] if at == "last" else [(0, t) for t in range(full)])
    if at == "middle":   # two batch rows, the second one's maps all keep the last row: only the first row's words go
        N = 150_532 if dtype == np.float32 else 75_268
        maps = affine_maps(E, 2, dtype, 13)
        maps[e, 0] = last_row_map(1, dtype, 14)[0]
        _, flags = run_every_way(ops, oracle, beam_rows(2, N, dtype, seed=4), maps)
        assert column_path(2, N, dtype, E)
        check_flags(flags, N, dtype, expect_zero=[(0, t) for t in range(N // TP[dtype])])


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_inf_in_the_other_columns(ops, oracle, dtype):
    """0 * NaN and 0 * inf in row 6 of the map make the seventh coordinate NaN: in pass 0 where the input holds them, and in the
    middle of the run where a coordinate overflows on the way (px so large that the second drift takes x to inf: the pass after
    it turns the 1 of that row into NaN, the tile's word is withdrawn, and the passes behind it read the stored column)"""
    tp = TP[dtype]
    u = np.uint32 if dtype == np.float32 else np.uint64
    nan = np.array([0xFFC00055 if dtype == np.float32 else 0xFFF8000000000055], dtype=u).view(dtype)[0]
    drift = fodo_maps(oracle, 4, dtype)[1]
    for N in (SMALL[dtype][-1], MID[dtype][1]):
        full = N // tp
        x = beam_rows(1, N, dtype, seed=5)[0]
        x[3, 0] = nan
        x[(full // 2) * tp + 65, 5] = dtype(np.inf)
        x[(full - 1) * tp + tp - 1, 3] = dtype(-np.inf)
        x[N - 1, 2] = nan                                    # the partial tile: rows in every pass
        _, flags = run_every_way(ops, oracle, x, fodo_maps(oracle, 7, dtype), with_oracle=False)   # (a CPU's 0 * inf has the other sign)
        check_flags(flags, N, dtype, expect_zero=[(0, 0), (0, full // 2), (0, full - 1)])
        x = beam_rows(1, N, dtype, seed=5)[0]
        big = np.finfo(dtype).max * dtype(0.8)
        x[2 * tp + 130, 1] = big                             # x: 0.8 big, 1.6 big = inf behind the second or third drift
        x[(full - 2) * tp, 3] = -big
        got, flags = run_every_way(ops, oracle, x, np.stack([drift] * 7), with_oracle=False)
        assert torch.isnan(got[0, 2 * tp + 130, 6]) and torch.isnan(got[0, (full - 2) * tp, 6])
        assert float(got[0, 2 * tp + 131, 6]) == 1.0
        check_flags(flags, N, dtype, expect_zero=[(0, 2), (0, full - 2)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_consumer_on_the_stream_and_graph_replay(ops, oracle, dtype):
    """the scratch comes from the caching allocator inside the call: a second call and a copy read the output right behind it without
    a synchronisation, and one capture into a device graph replays with new inputs"""
    E = 4
    for N in (SMALL[dtype][-1], MID[dtype][1]):
        mt = torch.from_numpy(affine_maps(E, 1, dtype, 17)).cuda()
        x1, x2 = torch.from_numpy(beam_rows(1, N, dtype, seed=6)[0]).cuda(), torch.from_numpy(beam_rows(1, N, dtype, seed=7)[0]).cuda()
        want1, want2 = ops.track_elementwise(x1, mt, fused=True), ops.track_elementwise(x2, mt, fused=True)
        want11 = ops.track_elementwise(want1, mt, fused=True)
        torch.cuda.synchronize()
        a = ops.track_elementwise(x1, mt)
        b = ops.track_elementwise(a, mt)
        c = a.clone()
        torch.cuda.synchronize()
        assert same_bits(a, want1) and same_bits(c, want1) and same_bits(b, want11)
        static_in = x1.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g):
                out = ops.track_elementwise(static_in, mt)
        torch.cuda.current_stream().wait_stream(side)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want1)
        static_in.copy_(x2)
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want2)


def test_scratch_bytes(ops):
    from cheetah_amd import _lib

    lib = _lib.lib()
    for dtype, code in ((np.float32, 0), (np.float64, 1)):
        first = SMALL[dtype][1 if dtype == np.float32 else 0]
        assert lib.chx_track_elementwise_scratch_bytes(1, first - 1, code) == 0
        assert lib.chx_track_elementwise_scratch_bytes(1, first, code) == 4 * -(-first // TP[dtype])
        assert lib.chx_track_elementwise_scratch_bytes(3, 1_000_001, code) == 4 * 3 * -(-1_000_001 // TP[dtype])
    assert lib.chx_track_elementwise_scratch_bytes(1, 1_000_000, 7) == 0
