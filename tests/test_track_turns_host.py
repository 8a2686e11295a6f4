"""Host side of Segment.track_turns (no GPU): the result class for a call without records, and the planner that splits the turns
of a fused call into launches, as a pure function."""
import itertools

import pytest
import torch


def test_turn_by_turn_shapes_without_records():
    from cheetah_amd import TurnByTurn
    from cheetah_amd.particles import turns as T

    n = 5
    tbt = TurnByTurn(None, torch.zeros(n, dtype=torch.int32), T.recorded_turns(3, 4), torch.empty((0, T.NUM_SUMS), dtype=torch.float64))
    assert tbt.turns.shape == (0,) and tbt.turns.dtype == torch.int64
    assert tbt.num_alive.shape == (0,) and tbt.charge.shape == (0,)
    assert tbt.mean.shape == (0, 6) and tbt.std.shape == (0, 6)
    assert all(f.dtype == torch.float64 for f in (tbt.num_alive, tbt.charge, tbt.mean, tbt.std))
    assert tbt.particles is None and tbt.lost_turn.shape == (n,)
    with_rows = TurnByTurn(None, torch.zeros(n, dtype=torch.int32), T.recorded_turns(3, 4), torch.empty((0, 14), dtype=torch.float64),
                           torch.empty((0, 2, 7)))
    assert with_rows.particles.shape == (0, 2, 7)


def test_turn_by_turn_fields_follow_their_definitions():
    from cheetah_amd import TurnByTurn
    from cheetah_amd.particles import turns as T

    x = torch.tensor([[1.0, 2, 3, 4, 5, 6, 1], [3.0, 2, 1, 0, -1, -2, 1], [float("nan")] * 7])
    alive = torch.tensor([True, True, False])
    w = torch.tensor([1.0, 3.0, 2.0], dtype=torch.float64)
    sums = T.record_sums(x, alive, w)
    assert sums.dtype == torch.float64 and sums.shape == (14,) and torch.isfinite(sums).all()       # the NaN row is selected out
    tbt = TurnByTurn(None, torch.tensor([0, 0, 1], dtype=torch.int32), T.recorded_turns(1, 1), sums[None])
    assert tbt.num_alive.tolist() == [2.0] and tbt.charge.tolist() == [4.0]
    assert tbt.mean[0].tolist() == [2.5, 2.0, 1.5, 1.0, 0.5, 0.0]
    # population form: sqrt(sum w (x - mean)^2 / sum w), e.g. sqrt((1 * 1.5^2 + 3 * 0.5^2) / 4) for the first coordinate
    assert torch.allclose(tbt.std[0], torch.tensor([0.75 ** 0.5, 0.0, 0.75 ** 0.5, 3.0 ** 0.5, 6.75 ** 0.5, 12.0 ** 0.5], dtype=torch.float64))
    assert T.is_lost(x, None).tolist() == [False, False, True]
    assert T.is_lost(x, torch.tensor([2.5, 2.5])).tolist() == [True, True, True]                    # |y| = 3 > 2.5, |x| = 3 > 2.5


@pytest.mark.parametrize("num_turns, items, record_every, per_record, max_steps, max_bytes",
                         list(itertools.product([1, 2, 37, 1000], [1, 6, 224], [1, 5, 64], [112, 437_584], [12, 65536], [1, 64 << 20])))
def test_chunk_planner(num_turns, items, record_every, per_record, max_steps, max_bytes):
    from cheetah_amd.particles import turns as T

    chunks = T.plan_chunks(num_turns, items, record_every, per_record, max_steps, max_bytes)
    # the ranges cover 1 .. num_turns once, in order
    covered = [t for first, n in chunks for t in range(first, first + n)]
    assert covered == list(range(1, num_turns + 1))
    # the caps hold, except that a launch always does one whole turn and may hold one record
    for first, n in chunks:
        assert n >= 1
        assert n * items <= max_steps or n == 1
        assert T.chunk_records(first, n, record_every) * per_record <= max_bytes or T.chunk_records(first, n, record_every) <= 1
    # the recorded turns are those of the call without chunking
    recorded = [t for first, n in chunks for t in range(first, first + n) if t % record_every == 0]
    assert recorded == T.recorded_turns(num_turns, record_every).tolist()
    assert sum(T.chunk_records(first, n, record_every) for first, n in chunks) == num_turns // record_every


def test_entry_point_turns_invalid_arguments_away_before_any_launch():
    """chx_second_order_turns checks its arguments on the host: every case below returns before a kernel is launched, so the
    pointers only need to be distinct, aligned and non-null."""
    import ctypes

    import cheetah_amd._lib as L

    lib = L.lib()
    E, N = 3, 1000
    maps = (ctypes.c_void_p * 224)(*([0x10000] * 224))
    ws_bytes = lib.chx_second_order_turns_workspace_bytes(E, N, 4, 0)
    assert ws_bytes == E * 256 * 4 + 4 * 2 * 14 * 8                      # coefficients + 4 records x 2 tiles x 14 doubles
    assert lib.chx_second_order_turns_workspace_bytes(E, N, 4, 1) == E * 256 * 8 + 4 * 4 * 14 * 8

    def call(E=E, x_in=0x20000, N=N, dtype=0, first=1, turns=4, every=1, K=2, x_out=0x30000, lost=0x40000, sums=0x50000,
             probe=0x60000, ws=0x70000, ws_bytes=ws_bytes):
        return lib.chx_second_order_turns(maps, None, None, E, x_in, None, None, N, dtype, first, turns, every, None, K, x_out, lost,
                                          sums, probe, None, None, ws, ws_bytes, None)

    invalid, bad_dtype = -1, -2
    assert call(E=0) == invalid and call(E=225) == invalid
    assert call(turns=0) == invalid and call(every=0) == invalid and call(first=0) == invalid
    assert call(K=N + 1) == invalid and call(K=-1) == invalid
    assert call(dtype=2) == bad_dtype
    assert call(x_out=0x20000) == invalid                                # x_out aliases x_in on the first chunk
    assert call(sums=0x30000) == invalid and call(ws=0x40000) == invalid and call(probe=0x20000) == invalid
    assert call(ws_bytes=ws_bytes - 1) == invalid and call(ws=0x70008) == invalid      # too small / not 16-byte aligned
    # the last turn must stay below 2^31 - 1: the kernels count to first_turn + num_turns in int
    assert call(first=2 ** 31 - 4, turns=4, every=2 ** 31 - 1) == invalid
    assert call(first=2 ** 31 - 1, turns=1) == invalid and call(turns=2 ** 31) == invalid


def test_chunk_planner_defaults_and_errors():
    from cheetah_amd.particles import turns as T

    assert T._MAX_ITEM_STEPS == 65536 and T._MAX_PARTIAL_BYTES == 64 << 20
    assert T.plan_chunks(37, 6, 1, 112, 12, 64 << 20)[:2] == [(1, 2), (3, 2)]                     # 12 item steps: two turns of six items
    assert T.plan_chunks(1000, 100, 1, 112, 65536, 64 << 20) == [(1, 655), (656, 345)]
    for bad in ((0, 6, 1), (5, 0, 1), (5, 6, 0)):
        with pytest.raises(ValueError):
            T.plan_chunks(*bad, 112, 65536, 64 << 20)
