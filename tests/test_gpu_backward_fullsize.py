"""Backward kernels of the particle passes beyond one tile, against float64 references on the host.

Loss L = sum(dY * out) with a fixed random cotangent dY (plus a term in the outgoing reference energy where there is one).
- ApplySecondOrder (chx_apply_second_order_bwd): dx and dT against float64 autograd of einsum("bijk,bnj,bnk->bni"). From 65 537
  particles on, one workgroup reduces several 256-particle tiles.
- DkdTrack (chx_dkd_track_bwd): dx, dparams and denergy against Richardson-extrapolated central differences of the float64
  oracle (oracle.dkd_track). Particles are independent, so one perturbation of column j for all particles gives every
  dL/dx_nj, and one perturbation of a setting gives every particle's term of its gradient.
- CavityTrack (chx_cavity_track_bwd with the dR path of chx_apply_affine7_bwd) through Cavity.track: dx, d(length, voltage,
  phase, frequency) and d energy against differences of oracle.build_rmatrix + cavity_coeffs + cavity_track.

A gradient that is a sum over particles (and over broadcast rows) is measured against the sum of the magnitudes of its terms;
a per-particle gradient against the largest magnitude of its column. Float32 inputs are rounded to float32 first and the
reference is evaluated on the rounded values. Float32 bounds are 4x the error measured on the MI355X;
the comment next to each quotes the largest measured value."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
MASS, NQ = 510998.95069, -1.0
COL_SCALE = np.array([1e-3, 1e-4, 1e-3, 1e-4, 1e-5, 1e-3, 1.0])
RT64 = 1e-9
# float64 drift-kick-drift gradients against finite differences: the differences themselves limit the agreement. Central
# differences of the oracle at steps h and 3h disagree by up to 5e-7 for the phase of the transverse deflecting cavity and the
# face angles of the dipole at one particle. 4x the largest error measured on the MI355X:
RT64_FD = {"dx": 8.2e-9,            # 2.04e-9, dipole with the exit fringe, N = 1
           "dparams": 2.1e-6}       # 5.19e-7, transverse deflecting cavity, N = 1
# float32: 4x the largest error measured on the MI355X over the cases (quoted after each entry)
RT32 = {
    "so": {"dx": 3.6e-7,            # 8.79e-8, N = 65 537, (Bx, BT) = (1, 3)
           "dT": 2.2e-7},           # 5.43e-8, N = 1
    "dkd": {"dx": 3.8e-7,           # 9.28e-8, quadrupole, energy (3, 1) against settings (1, 4)
            "dparams": 2.1e-6,      # 5.22e-7, transverse deflecting cavity, N = 1
            "denergy": 2.3e-7},     # 5.69e-8, drift, N = 100 003
    "cav": {"dx": 4.8e-7,           # 1.20e-7, shared settings, N = 100 003
            "dsettings": 1.9e-7,    # 4.64e-8 (voltage), shared settings, N = 257
            "denergy": 4.0e-7},     # 9.86e-8, shared beam, N = 257
}


def _dt(tag):
    return torch.float64 if tag == "f64" else torch.float32


def _rt(tag, kind, what):
    if tag == "f64":
        return RT64_FD.get(what, RT64) if kind == "dkd" else RT64
    return RT32[kind][what]


def _round(a, tag):
    return np.asarray(a, dtype=np.float64).astype(np.float32 if tag == "f32" else np.float64).astype(np.float64)


def _check(what, got, ref, scale, bound):
    got = got.detach().to(torch.float64).cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    scale = np.broadcast_to(np.asarray(scale, np.float64), ref.shape)
    scale = np.where(scale > 0, scale, scale.max())      # (a setting the element ignores: measured against the others)
    err = float(np.max(np.abs(got - ref) / scale))
    print(f"MEASURED {what}: {err:.3e} (bound {bound:.1e})")
    assert err <= bound, f"{what}: error {err:.3e} over the bound {bound:.1e}"


def _col_scale(ref):
    s = np.abs(ref).reshape(-1, ref.shape[-1]).max(axis=0)
    return np.where(s > 0, s, np.abs(ref).max())


def _particles(rng, lead, n, tag):
    x = rng.standard_normal((*lead, n, 7)) * COL_SCALE
    x[..., 6] = 1.0
    return _round(x, tag)


# The per-particle terms of the differences are formed from out - out(unperturbed): the loss itself is a sum of terms of order
# 1 (column 6 of the output is 1), whose rounding would swamp the differences. The coordinates are stepped by H_X (absolute):
# their rounding at the step (tau carries about 1e-17 m from the path length) stays below 1e-11 of the derivative.
H_X = 1e-5


def _richardson(f, h):
    """(4 D(h/2) - D(h)) / 3 of the central difference D(h) = (f(h) - f(-h)) / 2h; f returns an array."""
    d = lambda h: (f(h) - f(-h)) / (2 * h)  # noqa: E731
    return (4 * d(h / 2) - d(h)) / 3


# ---------------------------------------------------------------------------------------------------------------------------
# ApplySecondOrder

SO_CASES = ([(n, 1, 1, tag) for n in (1, 255, 256, 257, 65_537) for tag in ("f64", "f32")] + [(1_000_000, 1, 1, "f32")]
            + [(n, bx, bt, tag) for n in (257, 65_537) for bx, bt in ((1, 3), (3, 1), (3, 3)) for tag in ("f64", "f32")])


@pytest.mark.parametrize("n,bx,bt,tag", SO_CASES)
def test_apply_second_order_backward(n, bx, bt, tag):
    from cheetah_amd import _ops

    dt = _dt(tag)
    rng = np.random.default_rng(n + 10 * bx + 100 * bt)
    x = _particles(rng, (bx,), n, tag)
    T = _round(rng.standard_normal((bt, 7, 7, 7)) * 3.0, tag)
    B = max(bx, bt)
    dY = _round(rng.standard_normal((B, n, 7)), tag)
    # a row count of 1 is passed without its batch axis: the shared beam / the shared map
    xg = torch.nn.Parameter(torch.tensor(x[0] if bx == 1 else x, dtype=dt, device=DEV))
    Tg = torch.nn.Parameter(torch.tensor(T[0] if bt == 1 else T, dtype=dt, device=DEV))
    out = _ops.apply_second_order(xg, Tg)
    assert out.shape == ((n, 7) if B == 1 else (B, n, 7))
    (out * torch.tensor(dY[0] if B == 1 else dY, dtype=dt, device=DEV)).sum().backward()

    def ref_grads(x, T, dY):
        xr = torch.tensor(x, requires_grad=True)
        Tr = torch.tensor(T, requires_grad=True)
        xb, Tb = xr.expand(B, n, 7), Tr.expand(B, 7, 7, 7)
        (torch.einsum("bijk,bnj,bnk->bni", Tb, xb, xb) * torch.tensor(dY)).sum().backward()
        return xr.grad.numpy(), Tr.grad.numpy()

    dx, dT = ref_grads(x, T, dY)
    # the same contraction on magnitudes bounds every term: the scale of a sum
    _, dT_abs = ref_grads(np.abs(x), np.abs(T), np.abs(dY))
    label = f"second_order {tag} N={n} B=({bx},{bt})"
    _check(f"{label} dx", xg.grad, dx.reshape(xg.shape), _col_scale(dx), _rt(tag, "so", "dx"))
    _check(f"{label} dT", Tg.grad, dT.reshape(Tg.shape), dT_abs.reshape(Tg.shape), _rt(tag, "so", "dT"))


# ---------------------------------------------------------------------------------------------------------------------------
# DkdTrack

DKD_PARAMS = {
    "drift": [0.5],
    "quadrupole": [0.2, 3.0, 0.1, 1e-4, -2e-4],
    "dipole": [0.5, 0.1, 0.02, 0.03, 0.05, 0.4, 0.35, 0.03, 0.025],
    "tdc": [0.3, 1e6, 20.0, 2.9e9, 0.1, 1e-4, -2e-4],
}
DKD_KINDS = [("drift", 1, 3), ("quadrupole", 1, 3), ("quadrupole", 3, 3)] + [("dipole", 1, f) for f in range(4)] \
    + [("tdc", 1, 3)]
E0 = 1e8
C_E = 1e-6          # weight of the outgoing reference energy in the loss


def _dkd_reference(kind, x, p, e, dY, steps, fringe, xi, pi, ei, e_shape):
    """float64 oracle gradients of L = sum(dY * out) + C_E * sum(e_out over the energy entries). Rows b of the batch take
    particles x[xi[b]], settings p[pi[b]] and energy e[ei[b]]. Returns ((dx, dx scale), (dp, dp scale), (de, de scale))."""
    from oracle import chx_oracle as oracle

    out0 = oracle.dkd_track(kind, x[xi], p[pi], e[ei], MASS, NQ, steps, fringe)[0]

    def losses(xx, pp, ee):
        out, _ = oracle.dkd_track(kind, xx[xi], pp[pi], ee[ei], MASS, NQ, steps, fringe)
        return ((out - out0) * dY).sum(axis=-1)            # (B, N): each particle's term

    def reduce(terms, idx, rows):
        """(B, N) terms -> their sums and sums of magnitudes over the particles and the rows that share an entry."""
        tot, mag = np.zeros(rows), np.zeros(rows)
        np.add.at(tot, idx, terms.sum(axis=1))
        np.add.at(mag, idx, np.abs(terms).sum(axis=1))
        return tot, mag

    dx = np.zeros_like(x)
    for j in range(7):
        def f(h, j=j):
            xx = x.copy()
            xx[..., j] += h
            return losses(xx, p, e)
        t = _richardson(f, H_X)                            # (B, N)
        np.add.at(dx[..., j], xi, t)
    dp = np.zeros(p.shape)
    dp_mag = np.zeros(p.shape)
    for k in range(p.shape[1]):
        def f(h, k=k):
            pp = p.copy()
            pp[:, k] += h
            return losses(x, pp, e)
        dp[:, k], dp_mag[:, k] = reduce(_richardson(f, 1e-3 * abs(p[0, k])), pi, p.shape[0])

    def f(h):
        return losses(x, p, e + h)
    de, de_mag = reduce(_richardson(f, 1e-3 * E0), ei, e.shape[0])
    # the outgoing reference energy: one entry per INCOMING energy entry (bmadx.py:49)

    def g(h):
        return oracle.dkd_track(kind, x[:1], p[:1], e + h, MASS, NQ, steps, fringe)[1]
    d_eout = C_E * _richardson(g, 1e-3 * E0)
    de = de + d_eout
    de_mag = de_mag + np.abs(d_eout)
    return (dx, _col_scale(dx)), (dp, dp_mag), (de.reshape(e_shape), de_mag.reshape(e_shape))


def _dkd_case(kind, steps, fringe, n, tag, bx, bp, be, pshape=None, eshape=None):
    from cheetah_amd import _ops

    dt = _dt(tag)
    rng = np.random.default_rng(n + 7 * bx + 11 * bp + 13 * be + 17 * fringe + 19 * steps + len(kind))
    P = len(DKD_PARAMS[kind])
    x = _particles(rng, (bx,), n, tag)
    p = _round(np.array(DKD_PARAMS[kind]) * (1.0 + 0.1 * np.arange(bp)[:, None] * np.cos(np.arange(P))), tag)
    e = _round(E0 * (1.0 + 0.3 * np.arange(be)), tag)
    pshape = pshape if pshape is not None else ((bp,) if bp > 1 else ())
    eshape = eshape if eshape is not None else ((be,) if be > 1 else ())
    batch = tuple(torch.broadcast_shapes((bx,) if bx > 1 else (), pshape, eshape))
    B = int(np.prod(batch)) if batch else 1
    # rows of the flattened batch -> rows of x, p and e
    idx = lambda shape: np.broadcast_to(np.arange(int(np.prod(shape))).reshape(shape), batch).reshape(-1) \
        if shape else np.zeros(B, int)  # noqa: E731
    xi, pi, ei = idx((bx,) if bx > 1 else ()), idx(pshape), idx(eshape)
    dY = _round(rng.standard_normal((B, n, 7)), tag)

    xg = torch.nn.Parameter(torch.tensor(x if bx > 1 else x[0], dtype=dt, device=DEV))
    pg = torch.nn.Parameter(torch.tensor(p, dtype=dt, device=DEV))
    eg = torch.nn.Parameter(torch.tensor(e.reshape(eshape), dtype=dt, device=DEV))
    k = _ops.DKD_KIND[kind]
    out, e_out = _ops.dkd_track(k, xg, pg, torch.Size(pshape), eg, MASS, NQ, steps, fringe)
    assert out.shape == (*batch, n, 7) and e_out.shape == eg.shape
    loss = (out * torch.tensor(dY.reshape(*batch, n, 7), dtype=dt, device=DEV)).sum() + C_E * e_out.sum()
    loss.backward()

    (dx, sx), (dp, sp), (de, se) = _dkd_reference(kind, x, p, e, dY, steps, fringe, xi, pi, ei, eshape)
    label = f"dkd {kind} steps={steps} fringe={fringe} {tag} N={n} B=({bx},{bp},{be})"
    _check(f"{label} dx", xg.grad, dx if bx > 1 else dx[0], sx, _rt(tag, "dkd", "dx"))
    _check(f"{label} dparams", pg.grad, dp, sp, _rt(tag, "dkd", "dparams"))
    _check(f"{label} denergy", eg.grad, de, se, _rt(tag, "dkd", "denergy"))


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("n", [1, 257, 100_003])
@pytest.mark.parametrize("kind,steps,fringe", DKD_KINDS)
def test_dkd_backward(kind, steps, fringe, n, tag):
    _dkd_case(kind, steps, fringe, n, tag, 1, 1, 1)


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("bx,bp,be", [(3, 1, 1), (1, 3, 1), (1, 1, 3), (3, 3, 1), (3, 1, 3), (1, 3, 3), (3, 3, 3)])
def test_dkd_backward_broadcast(bx, bp, be, tag):
    _dkd_case("quadrupole", 1, 3, 2049, tag, bx, bp, be)


@pytest.mark.parametrize("tag", ["f64", "f32"])
def test_dkd_backward_energy_against_other_vector_dims(tag):
    """Energy (3, 1) against settings (1, 4): the outgoing energy keeps the energy's shape (the index_copy branch)."""
    _dkd_case("quadrupole", 1, 3, 2049, tag, 1, 4, 3, pshape=(1, 4), eshape=(3, 1))


# ---------------------------------------------------------------------------------------------------------------------------
# CavityTrack

CAV = np.array([[0.5, 5e6, 10.0, 1.3e9], [0.6, 8e6, 25.0, 1.3e9], [0.45, 3e6, -15.0, 1.25e9], [0.55, 6e6, 35.0, 1.35e9]])


@pytest.mark.parametrize("tag", ["f64", "f32"])
@pytest.mark.parametrize("n", [257, 100_003])
@pytest.mark.parametrize("shared", [True, False], ids=["shared_beam", "shared_settings"])
def test_cavity_backward(shared, n, tag):
    """shared_beam: one (N, 7) beam through B = 4 settings; shared_settings: a (4, N, 7) beam through one setting."""
    import cheetah_amd as ca
    from oracle import chx_oracle as oracle

    dt = _dt(tag)
    rng = np.random.default_rng(n + int(shared))
    bx, bp = (1, 4) if shared else (4, 1)
    x = _particles(rng, (bx,), n, tag)
    p = _round(CAV[:bp], tag)
    e = float(_round(1e8, tag))
    dY = _round(rng.standard_normal((4, n, 7)), tag)

    kw = {"dtype": dt, "device": DEV}
    xg = torch.nn.Parameter(torch.tensor(x[0] if shared else x, **kw))
    settings = [torch.nn.Parameter(torch.tensor(p[:, k] if shared else p[0, k], **kw)) for k in range(4)]
    eg = torch.nn.Parameter(torch.tensor(e, **kw))
    cav = ca.Cavity(length=settings[0], voltage=settings[1], phase=settings[2], frequency=settings[3], **kw)
    out = cav.track(ca.ParticleBeam(xg, eg, **kw))
    assert out.particles.shape == (4, n, 7)
    loss = (out.particles * torch.tensor(dY, **kw)).sum() + C_E * out.energy.sum()
    loss.backward()

    def track(xx, pp, ee):
        pp = np.broadcast_to(pp, (4, 4))
        R = oracle.build_rmatrix("cavity_sw", pp, ee, MASS, NQ)
        coeffs, e_out = oracle.cavity_coeffs(pp, ee, MASS, NQ)
        return oracle.cavity_track(xx, R, coeffs), e_out

    out0, e0 = track(x, p, e)

    def losses(xx, pp, ee):
        o, e_out = track(xx, pp, ee)
        terms = ((o - out0) * dY).sum(axis=-1)
        e_out = e_out - e0
        # the energy term rides on particle 0: one per row of settings, once for the shared setting
        if shared:
            terms[:, 0] += C_E * e_out
        else:
            terms[0, 0] += C_E * e_out[0]
        return terms

    rt = lambda what: _rt(tag, "cav", what)  # noqa: E731
    label = f"cavity {'shared beam' if shared else 'shared settings'} {tag} N={n}"
    dx = np.zeros((4, n, 7))
    for j in range(7):
        def f(h, j=j):
            xx = x.copy()
            xx[..., j] += h
            return losses(xx, p, e)
        dx[..., j] = _richardson(f, H_X)
    if shared:
        dx = dx.sum(axis=0)
    _check(f"{label} dx", xg.grad, dx, _col_scale(dx), rt("dx"))
    for k, name in enumerate(("length", "voltage", "phase", "frequency")):
        def f(h, k=k):
            pp = p.copy()
            pp[:, k] += h
            return losses(x, pp, e)
        t = _richardson(f, 1e-3 * abs(p[0, k]))
        ref, mag = (t.sum(axis=1), np.abs(t).sum(axis=1)) if shared else (t.sum(), np.abs(t).sum())
        _check(f"{label} d{name}", settings[k].grad, ref, mag, rt("dsettings"))
    t = _richardson(lambda h: losses(x, p, e + h), 1e-3 * e)
    _check(f"{label} denergy", eg.grad, t.sum(), np.abs(t).sum(), rt("denergy"))
