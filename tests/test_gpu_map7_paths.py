"""One first-order map, one beam, every particle kernel that applies a map: the same bits.

The library has one definition of the map step (chx_map7, chx_common.h: row i is R_i0 x_0, then six fused multiply-adds in the
storage dtype) and every kernel that sends a particle through a 7x7 map uses it. This test pins that: the particles
`chx_apply_affine7` writes for ONE beam and ONE map (B = 1) are the canonical result, and the same map reached through
chx_track_fused (E = 1), chx_track_elementwise (E = 1), the shared-beam apply (one beam, B = 3 rows of the map), a one-element
lattice stretch (chx_lattice_track_diag: the element and an active monitor) and a scan of equal rows of settings over the shared
beam must be `torch.equal` to it, in float32 and float64, with one beam per row and with one beam shared by the rows.

N = 1092 rows are 16-byte aligned in both dtypes (the wave-staged kernels run: apply_wave_kernel, apply_shared_wave_kernel,
lattice_scan_wave_kernel); N = 1091 rows are not (the workgroup-staged kernels and the scalar tails run). 1091 float32 rows are two
full 512-row tiles, one partial wave and a ragged tail.

Two maps. "dense": identity plus 0.1 x standard normal draws in all 49 entries (condition number of a few units; every term
j = 0..6 of every row i = 0..6 counts, the seventh row included), for the paths that take any map: apply, fused, element by
element, shared beam. "quadrupole": the map of a quadrupole with drawn length, strength, tilt and misalignment (symplectic, its
seventh column filled by the misalignment) — the lattice paths build their maps on the device from element settings, so a map
that every path can reach is an element's; all paths run with it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3
SCAN_ROWS = 8          # the row-chunk scan kernel takes scans of at least 8 rows
ENERGY = 1e8


@pytest.fixture(scope="module")
def ca():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    import cheetah_amd

    cheetah_amd._lib.lib()
    return cheetah_amd


_cases = {}


def case(ca, dt, N, kind="quadrupole"):
    """(quadrupole settings, the map R (7, 7), the beam x (N, 7), the canonical result): drawn and computed once per dtype, N, kind"""
    key = (dt, N, kind)
    if key not in _cases:
        from cheetah_amd import _ops

        gen = torch.Generator().manual_seed(1000 + N + (0 if dt == torch.float32 else 1))
        kw = {"dtype": dt, "device": "cuda"}
        u = torch.rand(3, generator=gen, dtype=torch.float64)
        settings = {"length": float(0.1 + 0.4 * u[0]), "k1": float(-6.0 + 12.0 * u[1]), "tilt": float(0.5 * u[2]),
                    "misalignment": [float(1e-3 * (u[0] - 0.5)), float(1e-3 * (u[1] - 0.5))]}
        x = (torch.randn(N, 7, generator=gen, dtype=torch.float64) * 1e-3).to(**kw)
        x[:, 6] = 1
        quad = quadrupole(ca, settings, kw)
        energy = torch.tensor(ENERGY, **kw)
        beam = ca.ParticleBeam(x, energy, **kw)
        R = quad.first_order_transfer_map(energy, beam.species).reshape(7, 7).contiguous()
        if kind == "dense":
            R = (torch.eye(7, dtype=torch.float64) + 0.1 * torch.randn(7, 7, generator=gen, dtype=torch.float64)).to(**kw)
            assert float(torch.linalg.cond(R.double().cpu())) < 10
        with torch.no_grad():
            canonical = _ops.apply_map(x, R)
        assert canonical.shape == (N, 7) and bool(torch.isfinite(canonical).all())
        assert float((canonical[:, :4] - x[:, :4]).abs().max()) > 0          # the map does something
        assert kind == "dense" or float(R[:4, 6].abs().max()) > 0           # the misalignment fills the seventh column
        _cases[key] = (settings, R, x, canonical)
    return _cases[key]


def quadrupole(ca, settings, kw, rows=None):
    t = lambda v: torch.tensor(v, **kw) if rows is None else torch.full((rows,), v, **kw)  # noqa: E731
    return ca.Quadrupole(torch.tensor(settings["length"], **kw), k1=t(settings["k1"]), tilt=torch.tensor(settings["tilt"], **kw),
                         misalignment=torch.tensor(settings["misalignment"], **kw), **kw)


def stretch_calls(segment):
    """(list that collects one entry per chx_lattice_track* call, the host object to install as segment._HOST)"""
    calls = []
    host = segment._lib.host()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(host, name)
            return fn if name != "lattice_track" else (lambda *a: (calls.append(len(a)), fn(*a))[1])

    return calls, Spy()


DTYPES = [torch.float32, torch.float64]
SIZES = [1091, 1092]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("beams", ["shared", "per_row"])
@pytest.mark.parametrize("kind", ["dense", "quadrupole"])
def test_apply_kernels_write_the_canonical_bits(ca, dt, N, beams, kind):
    from cheetah_amd import _ops

    _, R, x, canonical = case(ca, dt, N, kind)
    want = canonical.expand(B, N, 7)
    with torch.no_grad():
        if beams == "shared":
            # one beam, B rows of the map: apply_shared_wave_kernel (N = 1092) / apply_shared_kernel (N = 1091)
            xin, maps = x, R.expand(B, 7, 7).contiguous()
        else:
            xin, maps = x.expand(B, N, 7).contiguous(), R
        out = _ops.apply_map(xin, maps)
        assert out.shape == (B, N, 7) and torch.equal(out, want)
        stack = maps.reshape(1, -1, 7, 7)                                   # (E = 1, BR, 7, 7)
        for fused in (True, False):
            out = _ops.track_elementwise(xin, stack, fused=fused)
            assert out.shape == (B, N, 7) and torch.equal(out, want), ("fused" if fused else "elementwise")
        for fused in (True, False):                                         # and B = 1 through both
            out = _ops.track_elementwise(x, R.reshape(1, 1, 7, 7), fused=fused)
            assert torch.equal(out.reshape(N, 7), canonical), ("fused" if fused else "elementwise")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("beams", ["one", "per_row"])
def test_lattice_stretch_writes_the_canonical_bits(ca, dt, N, beams):
    from cheetah_amd.accelerator import segment

    settings, _, x, canonical = case(ca, dt, N)
    kw = {"dtype": dt, "device": "cuda"}
    seg = ca.Segment([quadrupole(ca, settings, kw), ca.BPM(is_active=True, **kw)])
    xin = x if beams == "one" else x.expand(B, N, 7).contiguous()
    beam = ca.ParticleBeam(xin, torch.tensor(ENERGY, **kw), **kw)
    calls, spy = stretch_calls(segment)
    old = segment._HOST
    segment._HOST = spy
    try:
        with torch.no_grad():
            out = seg.track(beam)
    finally:
        segment._HOST = old
    assert len(calls) == 1, calls                                           # the element and its monitor: ONE stretch call
    assert torch.equal(out.particles, canonical.expand(xin.shape))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("rows", [B, SCAN_ROWS])
def test_scan_writes_the_canonical_bits(ca, dt, N, rows, monkeypatch):
    from cheetah_amd.accelerator import segment

    # rows of equal settings over ONE shared beam; with 8 rows and 16-byte aligned rows of the output: lattice_scan_wave_kernel
    monkeypatch.setenv("CHX_TUNE_SCAN_WAVE", "2")
    settings, _, x, canonical = case(ca, dt, N)
    kw = {"dtype": dt, "device": "cuda"}
    seg = ca.Segment([quadrupole(ca, settings, kw, rows=rows), ca.BPM(is_active=True, **kw)])
    beam = ca.ParticleBeam(x, torch.tensor(ENERGY, **kw), **kw)
    calls, spy = stretch_calls(segment)
    old = segment._HOST
    segment._HOST = spy
    try:
        with torch.no_grad():
            out = seg.track(beam)
    finally:
        segment._HOST = old
    assert len(calls) == 1, calls
    assert out.particles.shape == (rows, N, 7)
    assert torch.equal(out.particles, canonical.expand(rows, N, 7))
