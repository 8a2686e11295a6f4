"""The item rule of the entry points over a list of drift-kick-drift items, without a GPU: chx_dkd_turns, chx_dkd_ring_jacobian,
chx_dkd_ring_sensitivity and chx_dkd_ring_radiation refuse the same bad items with the same code, before any launch (the pointers
address host memory, which no launch may come to read). An item is good when its kind is one of the six ring kinds (Drift 0,
Quadrupole 1, Dipole 2, Sextupole 5, RFCavity 6, Multipole 8), its parameters are there, 1 <= num_steps < 2^25 and
0 <= fringe_at <= 3; a list has 1 to 192 items."""
import ctypes

import pytest

INVALID, BAD_DTYPE = -1, -2
CAP = 193                                                               # one more than the longest list: room for the row E = 193

# one table of bad lists: what differs from the good list of three items (a Drift, a Quadrupole of three steps, a Dipole)
BAD_ITEMS = {
    "kind 3 (TransverseDeflectingCavity)": {"kinds": (0, 3, 2)},
    "kind 4 (a linear run)": {"kinds": (0, 4, 2)},
    "kind 7": {"kinds": (0, 1, 7)},
    "kind -1": {"kinds": (-1, 1, 2)},
    "num_steps 0": {"steps": (1, 0, 1)},
    "num_steps 2^25": {"steps": (1, 3, 1 << 25)},
    "fringe_at -1": {"fringe": (-1, 3, 0)},
    "fringe_at 4": {"fringe": (3, 4, 0)},
    "params[1] null": {"null_params": 1},
    "E 0": {"E": 0},
    "E 193": {"E": 193},
}


def _lib():
    import cheetah_amd._lib as L
    import cheetah_amd._ops  # noqa: F401  (adds the signatures)

    return L.lib()


class Args:
    """The arguments the four entry points share, and host buffers for the rest. Everything the call holds stays referenced here."""

    def __init__(self, kinds=(0, 1, 2), steps=(1, 3, 1), fringe=(3, 3, 0), null_params=None, E=3, dtype=1, workspace_bytes=1 << 20, K=2):
        pad = lambda v, fill: list(v) + [fill] * (CAP - len(v))  # noqa: E731
        self.par = [(ctypes.c_double * 9)(0.5, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0) for _ in range(CAP)]
        address = [ctypes.addressof(p) for p in self.par]
        if null_params is not None:
            address[null_params] = None
        self.kinds, self.steps, self.fringe = ((ctypes.c_int32 * CAP)(*pad(v, f)) for v, f in ((kinds, 0), (steps, 1), (fringe, 0)))
        self.params = (ctypes.c_void_p * CAP)(*address)
        self.E, self.dtype = E, dtype
        self.energy = ctypes.c_double(1e8)
        self.raw = ctypes.create_string_buffer((1 << 20) + 16)
        self.workspace, self.workspace_bytes, self.K = (ctypes.addressof(self.raw) + 15) // 16 * 16, workspace_bytes, K
        self.buffers = []

    def items(self):
        return self.kinds, self.params, self.steps, self.fringe

    def buf(self, n, ctype=ctypes.c_double):
        self.buffers.append((ctype * n)())
        return self.buffers[-1]

    def ring(self):
        return ctypes.addressof(self.energy), 510998.95, -1.0, self.dtype


def turns(lib, a):
    N, K, turns_ = 8, 2, 4
    e_out = ctypes.c_double(0.0)
    return lib.chx_dkd_turns(*a.items(), 2, a.E, a.buf(N * 7), ctypes.addressof(a.energy), ctypes.addressof(e_out), 510998.95, -1.0, None, None, N,
                             a.dtype, 1, turns_, 1, None, K, a.buf(N * 7), a.buf(N, ctypes.c_int32), a.buf(turns_ * 14), a.buf(turns_ * K * 7),
                             None, None, a.workspace, a.workspace_bytes, None)


def ring_jacobian(lib, a):
    B, E = 2, CAP
    return lib.chx_dkd_ring_jacobian(*a.items(), a.E, *a.ring(), a.buf(B * 6), B, 1, 4, 1, a.buf(B * 6), a.buf(B * 6), a.buf(B * 36), a.buf(B),
                                     a.buf(B * 4), a.buf(B * (E + 1) * 6), a.buf(B * (E + 1) * 36), a.buf(E + 1), a.workspace,
                                     a.workspace_bytes, None)


def ring_sensitivity(lib, a):
    B, K, E = 2, a.K, CAP
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731
    return lib.chx_dkd_ring_sensitivity(*a.items(), a.E, *a.ring(), a.buf(B * 6), B, 1, i32(0, 1), i32(1, 0), i32(1, 0), 2 if K else 0, K, 1, a.buf(B * max(K, 1) * 6),
                                        a.buf(B * max(K, 1) * 6), a.buf(B * max(K, 1) * 36), a.buf(B * max(K, 1) * 4),
                                        a.buf(B * max(K, 1) * (E + 1) * 6), a.buf(B * max(K, 1) * (E + 1) * 36), a.workspace, a.workspace_bytes, None)


def ring_radiation(lib, a):
    B, E = 2, CAP
    return lib.chx_dkd_ring_radiation(*a.items(), a.E, *a.ring(), a.buf(B * 6), a.buf(B * 2), a.buf(B * 2), a.buf(B * 4), B, a.buf(B * 7),
                                      a.buf(B * E * 7), a.workspace, a.workspace_bytes, None)


ENTRY_POINTS = {"chx_dkd_turns": turns, "chx_dkd_ring_jacobian": ring_jacobian, "chx_dkd_ring_sensitivity": ring_sensitivity,
                "chx_dkd_ring_radiation": ring_radiation}


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_every_entry_point_refuses_every_bad_item(entry):
    lib = _lib()
    for row, change in BAD_ITEMS.items():
        for dtype in (0, 1):
            assert ENTRY_POINTS[entry](lib, Args(dtype=dtype, **change)) == INVALID, (entry, row, dtype)


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_a_bad_dtype_is_told_apart_when_every_item_is_good(entry):
    lib = _lib()
    assert ENTRY_POINTS[entry](lib, Args(dtype=2)) == BAD_DTYPE
    assert ENTRY_POINTS[entry](lib, Args(dtype=2, kinds=(5, 6, 8), steps=((1 << 25) - 1, 1, 1), fringe=(0, 1, 2))) == BAD_DTYPE
    # the dtype is looked at first: a bad item does not hide it
    assert ENTRY_POINTS[entry](lib, Args(dtype=2, kinds=(0, 3, 2))) == BAD_DTYPE


# ---- controls: the -1 of the table is the item check's, not that of a check in front of it -----------------------------------------
def test_the_good_list_passes_every_check_in_front_of_the_launches():
    """chx_dkd_ring_sensitivity with K = 0 validates everything and launches nothing: the good list returns 0 through the very
    arguments the table is applied to (for float32 and float64 settings), and every bad row is still refused there."""
    lib = _lib()
    for dtype in (0, 1):
        assert ring_sensitivity(lib, Args(dtype=dtype, K=0)) == 0
        for row, change in BAD_ITEMS.items():
            assert ring_sensitivity(lib, Args(dtype=dtype, K=0, **change)) == INVALID, (row, dtype)


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_the_good_list_is_refused_only_by_the_last_check(entry):
    """The other three cannot be called to the end without a launch, and every refusal of theirs but the dtype's is -1: no
    control without a launch can tell the item check's -1 from an earlier check's. What is pinned here is the weaker half: the
    good list is refused by the check of the workspace's size, which stands behind the items in all four. The argument lists of
    this harness are those of include/chx.h, compared by hand; the control above runs one of them to its end."""
    lib = _lib()
    for dtype in (0, 1):
        assert ENTRY_POINTS[entry](lib, Args(dtype=dtype, workspace_bytes=0)) == INVALID
