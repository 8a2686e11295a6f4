"""Host side of the fused drift-kick-drift ring of Segment.track_turns (no GPU): the size and layout of the workspace of
chx_dkd_turns, and its argument checks, every one of which returns before a kernel is launched (the pattern of
tests/test_track_turns_host.py: the pointers only need to be distinct, aligned and non-null)."""
import ctypes
import itertools


def _lib():
    import cheetah_amd._lib as L

    return L.lib()


def _up16(n):
    return (n + 15) // 16 * 16


def test_workspace_bytes_follow_the_documented_layout():
    """start[turns] (dtype) | block_of_turn[turns + 1] (int32) | constants[turns][E][56] (double) | partials[records][tiles][14]
    (double), tiles = ceil(N / 256) for both dtypes, the first two parts rounded up to 16 bytes (include/chx.h)."""
    lib = _lib()
    E, N, turns, records = 3, 700, 5, 4
    for dtype, esz in ((0, 4), (1, 8)):
        want = _up16(turns * esz) + _up16((turns + 1) * 4) + turns * E * 56 * 8 + records * 3 * 14 * 8
        assert lib.chx_dkd_turns_workspace_bytes(E, N, turns, records, dtype) == want
    assert lib.chx_dkd_turns_workspace_bytes(3, 700, 5, 4, 0) == 32 + 32 + 6720 + 1344
    # at the cap of 65 536 item steps per launch the constants come to 28 MiB
    assert lib.chx_dkd_turns_workspace_bytes(100, 1000, 655, 0, 0) - _up16(655 * 4) - _up16(656 * 4) == 65500 * 448 <= 28 << 20
    # out of range: 0
    for bad in ((0, N, 1, 0, 0), (193, N, 1, 0, 0), (E, 0, 1, 0, 0), (E, N, 0, 0, 0), (E, N, 1, -1, 0), (E, N, 1, 0, 2)):
        assert lib.chx_dkd_turns_workspace_bytes(*bad) == 0


def test_workspace_bytes_are_monotone_in_every_argument():
    lib = _lib()
    values = {"E": [1, 2, 7, 192], "N": [1, 256, 257, 700, 10 ** 6], "turns": [1, 2, 3, 4, 5, 37, 655], "records": [0, 1, 5, 37]}
    for dtype in (0, 1):
        size = {k: lib.chx_dkd_turns_workspace_bytes(*k, dtype) for k in itertools.product(*values.values())}
        assert all(v > 0 and v % 16 == 0 for v in size.values())
        for k, v in size.items():
            for axis, name in enumerate(values):
                for bigger in values[name]:
                    if bigger > k[axis]:
                        assert size[k[:axis] + (bigger,) + k[axis + 1:]] >= v, (k, name, bigger)
    for k in itertools.product(*values.values()):                       # a float64 beam never needs less than a float32 beam
        assert lib.chx_dkd_turns_workspace_bytes(*k, 1) >= lib.chx_dkd_turns_workspace_bytes(*k, 0)


def test_entry_point_turns_invalid_arguments_away_before_any_launch():
    lib = _lib()
    E, N = 3, 1000
    i32, vp = ctypes.c_int32 * 193, ctypes.c_void_p * 193
    ws_bytes = lib.chx_dkd_turns_workspace_bytes(E, N, 4, 4, 0)
    invalid, bad_dtype = -1, -2

    def call(kinds=(0, 1, 2), steps=(1, 3, 1), fringe=(3, 3, 0), params=0x10000, precision=2, E=E, x_in=0x20000, e_in=0x21000, e_out=0x22000,
             N=N, dtype=0, first=1, turns=4, every=1, K=2, x_out=0x30000, lost=0x40000, sums=0x50000, probe=0x60000, ws=0x70000,
             ws_bytes=ws_bytes, s_in=None, s_out=None, aperture=None, charges=None, arrays=(True, True, True, True)):
        pad = lambda v, fill: list(v) + [fill] * (193 - len(v))  # noqa: E731
        ka, pa, sa, fa = i32(*pad(kinds, 0)), vp(*([params] * 193)), i32(*pad(steps, 1)), i32(*pad(fringe, 0))
        ka, pa, sa, fa = [a if keep else None for a, keep in zip((ka, pa, sa, fa), arrays)]
        return lib.chx_dkd_turns(ka, pa, sa, fa, precision, E, x_in, e_in, e_out, 0.511e6, -1.0, charges, None, N, dtype, first, turns,
                                 every, aperture, K, x_out, lost, sums, probe, s_in, s_out, ws, ws_bytes, None)

    # E out of range, a kind other than Drift / Quadrupole / Dipole, a precision outside 0 .. 2
    assert call(E=0) == invalid and call(E=193) == invalid
    assert call(kinds=(0, 3, 2)) == invalid and call(kinds=(0, 4, 2)) == invalid and call(kinds=(-1, 1, 2)) == invalid
    assert call(precision=-1) == invalid and call(precision=3) == invalid
    # num_steps outside 1 .. 2^25 - 1, fringe_at outside 0 .. 3
    assert call(steps=(1, 0, 1)) == invalid and call(steps=(1, 1, 2 ** 25)) == invalid and call(steps=(-1, 1, 1)) == invalid
    assert call(fringe=(3, 4, 0)) == invalid and call(fringe=(-1, 3, 0)) == invalid
    # turns, records, probe rows
    assert call(turns=0) == invalid and call(every=0) == invalid and call(first=0) == invalid
    assert call(K=N + 1) == invalid and call(K=-1) == invalid
    # a last turn at or beyond 2^31 - 1: the kernels count to first_turn + num_turns in int
    assert call(first=2 ** 31 - 4, turns=4, every=2 ** 31 - 1) == invalid
    assert call(first=2 ** 31 - 1, turns=1) == invalid and call(turns=2 ** 31) == invalid
    # dtype
    assert call(dtype=2) == bad_dtype and call(dtype=-1) == bad_dtype
    # aliasing: x_out is x_in on the first chunk; two outputs, or an output and an input, at one address
    assert call(x_out=0x20000) == invalid
    assert call(sums=0x30000) == invalid and call(ws=0x40000) == invalid and call(probe=0x20000) == invalid
    assert call(e_out=0x30000) == invalid and call(e_out=0x20000) == invalid and call(lost=0x21000) == invalid
    assert call(s_in=0x80000, s_out=0x22000) == invalid and call(s_in=0x80000, s_out=0x80000) == invalid
    assert call(aperture=0x30000) == invalid and call(charges=0x22000) == invalid
    assert call(s_in=0x80000) == invalid and call(s_out=0x80000) == invalid          # both or neither
    # the workspace: too small, not 16-byte aligned
    assert call(ws_bytes=ws_bytes - 1) == invalid and call(ws=0x70008) == invalid
    assert call(turns=5, ws_bytes=ws_bytes) == invalid                               # sized for four turns
    # required pointers
    for name in ("x_in", "e_in", "e_out", "x_out", "lost", "ws", "params"):
        assert call(**{name: None}) == invalid, name
    assert call(sums=None) == invalid and call(probe=None) == invalid                # records fall into these turns, K > 0
    for k in range(4):
        assert call(arrays=tuple(i != k for i in range(4))) == invalid, k
