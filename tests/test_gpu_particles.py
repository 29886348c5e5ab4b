"""Lagrangian particles in the device time step (k_particle_substep, tlab_dns_particle_locate, tlab_dns_particle_sort; csrc/particles.hip) against
tests/particles_oracle.py, bit for bit: the kernel does the reference's operations in the reference's order without contraction, and so does numpy.
The oracle itself is pinned by tests/test_particles_host.py.

Shapes: (20, 12, 8) and (70, 33, 9) stretched in y, (20, 12, 1) for the bilinear branch -- the smallest a driver can have (SMALL_NZ of
tests/test_gpu_infrared.py).  Particle counts 1, 63, 64, 65, 1000: less than a wave, the wave boundaries, a partial last block.  The first particles
of every set are placed by hand (HAND below), the rest are random."""
import ctypes

import numpy as np
import pytest

from cases import grids, init_fields
from particles_oracle import Particles, locate_y, PART_TRACER, PART_INERTIA, BCS_NONE, BCS_STICK, BCS_SPECULAR

pytestmark = pytest.mark.gpu

VISC, SC = 1.0 / 800.0, (0.7,)
EINVAL, EUNSUPPORTED = -1, -2
SHAPES = [(20, 12, 8), (70, 33, 9), (20, 12, 1)]
COUNTS = [1, 63, 64, 65, 1000]
STOKES, SETTLING = 0.3, 0.05
DTE = 1e-2
PUSH = 5.0                    # a preset tendency that carries a hand-placed particle across a boundary: DTE PUSH = 0.05 against DTE |u| <= 0.012


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


_CASES = {}


def _case(shape):
    """(x, y, z, q0, s0) of a shape, made once"""
    if shape not in _CASES:
        nx, ny, nz = shape
        x, y, z = grids(nx, ny, nz, True)
        if nz == 1:
            z = np.zeros(1)
        q0, s0 = init_fields(nx, ny, nz, x, y, z, 17)
        _CASES[shape] = (x, y, z, q0, s0)
    return _CASES[shape]


_DRIVERS = {}


def _driver(shape):
    """one driver per shape for the tests that only call the particle entries (they change no field)"""
    import torch
    from tlab_amd.dns import Dns
    if shape not in _DRIVERS:
        x, y, z, q0, s0 = _case(shape)
        d = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False)
        for t, a in zip(d.q + d.s, q0 + s0):
            t.copy_(torch.from_numpy(a))
        _DRIVERS[shape] = d
    return _DRIVERS[shape]


def _particle_set(shape, n, ncol, seed=1):
    """(l_q columns, l_hq columns, names of the hand-placed particles): HAND first, then random positions inside the box"""
    x, y, z, _, _ = _case(shape)
    P = Particles(x, y, z)
    sx, sz, y0, y1 = P.sx, P.sz, y[0], y[-1]
    xm, ym, zm = 0.37 * sx, y0 + 0.41 * (y1 - y0), 0.63 * sz
    ex, ez = 0.5 * (x[-1] + sx), 0.5 * (z[-1] + sz) if len(z) > 1 else 0.0      # inside the seam cells
    # name: (x, y, z, preset tendency of x, y, z)
    HAND = [
        ("x seam", ex, ym, zm, 0, 0, 0), ("z seam", xm, ym, ez, 0, 0, 0), ("corner", ex, ym, ez, 0, 0, 0),
        ("on an x node", x[3], ym, zm, 0, 0, 0), ("on a y node", xm, y[4], zm, 0, 0, 0), ("on a z node", xm, ym, z[min(2, len(z) - 1)], 0, 0, 0),
        ("x = 0", 0.0, ym, zm, 0, 0, 0), ("y = y(1)", xm, y0, zm, 0, 0, 0), ("y = y(ny)", xm, y1, zm, 0, 0, 0),
        ("crosses x = scale", sx - 0.01, ym, zm, PUSH, 0, 0), ("crosses x = 0", 0.01, ym, zm, -PUSH, 0, 0),
        ("crosses z = scale", xm, ym, sz - 0.01, 0, 0, PUSH), ("crosses z = 0", xm, ym, 0.01, 0, 0, -PUSH),
        ("crosses y(ny)", xm, y1 - 0.01, zm, 0, PUSH, 0), ("crosses y(1)", xm, y0 + 0.01, zm, 0, -PUSH, 0),
        ("x = scale", sx, ym, zm, 0, 0, 0), ("z = scale", xm, ym, sz, 0, 0, 0),
    ]
    rng = np.random.default_rng(seed + n)
    lq = [rng.uniform(0.0, sx, n), rng.uniform(y0, y1, n), rng.uniform(0.0, sz, n)] + [rng.uniform(-0.5, 0.5, n) for _ in range(ncol - 3)]
    lh = [rng.uniform(-1.0, 1.0, n) for _ in range(ncol)]
    names = []
    for p, h in enumerate(HAND[:n]):
        names.append(h[0])
        for i in range(3):
            lq[i][p] = h[1 + i]
            lh[i][p] = h[4 + i] if h[4 + i] != 0 else lh[i][p]
        if ncol == 6:       # the particle's own velocity must not undo the push
            for i in range(3):
                lq[3 + i][p] = 0.1 * lq[3 + i][p]
    return lq, lh, names


def _upload(cols, off):
    """device copies that start on a 16-byte boundary (off = 0) or on an odd double (off = 1), and their holders"""
    import torch
    hold, views = [], []
    for a in cols:
        t = torch.zeros(len(a) + 2, dtype=torch.float64, device="cuda")
        assert t.data_ptr() % 16 == 0
        v = t[off: off + len(a)]
        assert v.data_ptr() % 16 == 8 * off
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        hold.append(t)
        views.append(v)
    return views, hold


def _ptrs(ts):
    from tlab_amd.lib import c_vp
    return (c_vp * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])


def _substep(d, dte, kco, scale, lq, lh, nodes, n=None):
    from tlab_amd.lib import load
    n = len(nodes) if n is None else n
    return load().tlab_dns_substep_particle(d._h, dte, kco, int(scale), n, d._arrays()[0], _ptrs(lq), _ptrs(lh), nodes.data_ptr())


def _equal_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got.view(np.int64) if got.dtype == np.float64 else got,
                                                      want.view(np.int64) if want.dtype == np.float64 else want)


# ---- 1: the substep bit for bit ----
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("kind", [PART_TRACER, PART_INERTIA])
@pytest.mark.parametrize("shape", SHAPES)
def test_substep_bit_for_bit(T, shape, kind, aligned):
    """one tlab_dns_substep_particle against the oracle: every column of l_q and l_hq and the nodes, all three wall conditions, scale_tendencies 0
    and 1, every particle count; arrays on a 16-byte boundary and on an odd double.  Everything bitwise, the IEEE division of the y fraction included."""
    import torch
    d = _driver(shape)
    x, y, z, q0, _ = _case(shape)
    ncol = 6 if kind == PART_INERTIA else 3
    seen = set()
    for bcs in (BCS_NONE, BCS_STICK, BCS_SPECULAR):
        d.set_particles(kind, 0, bcs, STOKES, SETTLING)
        for n in COUNTS:
            for scale in (0, 1):
                lq0, lh0, names = _particle_set(shape, n, ncol)
                O = Particles(x, y, z, type=kind, bcs=bcs, stokes=STOKES, settling=SETTLING)
                O.set(lq0, lh0)
                nodes0 = O.nodes.copy()
                O.substep(q0, DTE, -0.6, bool(scale))
                lq, hold1 = _upload(lq0, 0 if aligned else 1)
                lh, hold2 = _upload(lh0, 0 if aligned else 1)
                nodes = torch.from_numpy(nodes0).cuda()
                assert _substep(d, DTE, -0.6, scale, lq, lh, nodes) == 0
                torch.cuda.synchronize()
                for i in range(ncol):
                    assert _equal_bits(lq[i].cpu().numpy(), O.l_q[i]), (shape, kind, bcs, n, scale, "l_q", i)
                    assert _equal_bits(lh[i].cpu().numpy(), O.l_hq[i]), (shape, kind, bcs, n, scale, "l_hq", i)
                assert np.array_equal(nodes.cpu().numpy(), O.nodes), (shape, kind, bcs, n, scale)
                for t in hold1 + hold2:      # nothing outside the views was written
                    assert aligned or float(t[0]) == 0.0
                    assert float(t[-1]) == 0.0
                # the hand-placed particles did what their names say (in the oracle, which the device equals)
                nm = {k: p for p, k in enumerate(names)}
                if "crosses x = scale" in nm:
                    assert O.l_q[0][nm["crosses x = scale"]] < 0.1 and O.l_q[0][nm["crosses x = 0"]] > O.sx - 0.1
                    seen.add("x")
                if "crosses z = 0" in nm and shape[2] > 1:
                    assert O.l_q[2][nm["crosses z = scale"]] < 0.1 and O.l_q[2][nm["crosses z = 0"]] > O.sz - 0.1
                    seen.add("z")
                if "crosses y(1)" in nm:
                    up, dn = O.l_q[1][nm["crosses y(ny)"]], O.l_q[1][nm["crosses y(1)"]]
                    if bcs == BCS_NONE:
                        assert up > y[-1] and dn < y[0]
                    elif bcs == BCS_STICK:
                        assert up == y[-1] and dn == y[0]
                    else:
                        assert y[-1] - 0.1 < up < y[-1] and y[0] < dn < y[0] + 0.1
                    assert 1 <= O.nodes.min() and O.nodes.max() <= len(y) - 1
                    seen.add("y%d" % bcs)
    assert seen >= {"x", "y0", "y1", "y2"} and (shape[2] == 1 or "z" in seen)
    d.set_particles("none")


def test_zero_particles_is_a_no_op(T):
    import torch
    d = _driver(SHAPES[0])
    d.set_particles("tracer", 0)
    from tlab_amd.lib import load
    L = load()
    L.tlab_profile_reset(); L.tlab_profile_enable(1)
    try:
        assert L.tlab_dns_substep_particle(d._h, DTE, 1.0, 0, 0, None, None, None, None) == 0
        assert L.tlab_dns_particle_locate(d._h, 0, None, None) == 0
        d.locate_particles(); d.TIME_SUBSTEP_PARTICLE(DTE); d.sort_particles()
        torch.cuda.synchronize()
    finally:
        L.tlab_profile_enable(0)
    assert not _kernel_rows()                               # no launch
    L.tlab_profile_reset()
    d.set_particles("none")
    assert d.l_q is None and d.l_hq is None and d.l_nodes is None and d.l_tags is None


# ---- 2: LOCATE_Y on its own ----
@pytest.mark.parametrize("shape", SHAPES)
def test_locate_equals_the_oracles_loop(T, shape):
    import torch
    from tlab_amd.lib import load
    d = _driver(shape)
    d.set_particles("tracer", 0)
    _, y, _, _, _ = _case(shape)
    for n in COUNTS:
        lq0, _, _ = _particle_set(shape, n, 3)
        yp = lq0[1]
        if n == 1000:      # every node itself, and points outside the grid on both sides
            yp[20:20 + len(y)] = y
            yp[100:104] = [y[0] - 0.3, y[-1] + 0.3, y[0] - 1e-300, y[-1] + 1e-12]
        (dev,), _ = _upload([yp], 0)
        nodes = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        assert load().tlab_dns_particle_locate(d._h, n, dev.data_ptr(), nodes.data_ptr()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(nodes.cpu().numpy(), locate_y(yp, y)), (shape, n)
    d.set_particles("none")


# ---- 3: a linear field through the kernel ----
@pytest.mark.parametrize("shape", SHAPES)
def test_linear_field_reproduction_on_the_device(T, shape):
    """f = a + b x + c y + d z in u, v, w; l_hq = 0 and a tiny dte: l_hq after the call is the interpolated value, f at the particle within 1e-13
    for x < x(nx), z < z(nz), and the blend of the planes nx and 1 in the seam cell"""
    import torch
    from tlab_amd.dns import Dns
    x, y, z, _, _ = _case(shape)
    nx, ny, nz = shape
    d = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False)
    coefs = [(0.3, 0.7, -1.1, 0.45), (-0.2, 0.1, 0.9, -0.8), (1.0, -0.5, 0.25, 0.6)]
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    for t, (a, b, c, e) in zip(d.q, coefs):
        t.copy_(torch.from_numpy((a + b * X + c * Y + e * Z * (nz > 1)).ravel()))
    rng = np.random.default_rng(3)
    n = 5000
    P = Particles(x, y, z)
    for seam in (False, True):
        xs = rng.uniform(x[-1], x[0] + P.sx, n) if seam else rng.uniform(x[0], x[-1], n)
        pos = [xs, rng.uniform(y[0], y[-1], n), rng.uniform(z[0], z[-1], n) if nz > 1 else rng.uniform(0.1, 0.9, n)]      # (2-D: z is carried along, not used)
        d.set_particles("tracer", n, "none")
        for t, a in zip(d.l_q, pos):
            t.copy_(torch.from_numpy(a))
        d.locate_particles()
        d.TIME_SUBSTEP_PARTICLE(1e-300)
        torch.cuda.synchronize()
        xe = pos[0]
        if seam:
            tt = (xs - x[-1]) / (x[0] + P.sx - x[-1])
            xe = (1 - tt) * x[-1] + tt * x[0]
        for i, (a, b, c, e) in enumerate(coefs):
            want = a + b * xe + c * pos[1] + e * pos[2] * (nz > 1)
            err = float(np.abs(d.l_hq[i].cpu().numpy() - want).max())
            print("%s seam %s field %d: %.2e" % (shape, seam, i, err))
            assert err <= 1e-13, (shape, seam, i, err)
            assert _equal_bits(d.l_q[i].cpu().numpy(), pos[i])      # dte = 1e-300 moved nothing


# ---- 4: full steps ----
@pytest.mark.parametrize("kind", ["tracer", "inertia"])
@pytest.mark.parametrize("scheme", [3, 4])
def test_full_steps_with_particles(T, scheme, kind, monkeypatch):
    """two steps of Dns.TIME_RUNGEKUTTA on (70, 33, 9) with 1000 particles: the oracle's particles are advanced with the device's q of before every
    substep; positions, tendencies and nodes are bitwise equal at the end, and the flow and scalar fields are bit-identical to a second driver
    without particles"""
    import torch
    from tlab_amd.dns import Dns
    shape = (70, 33, 9)
    x, y, z, q0, s0 = _case(shape)
    n = 1000
    code = PART_INERTIA if kind == "inertia" else PART_TRACER
    ncol = 6 if kind == "inertia" else 3

    def make():
        m = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False, rkm_mode=scheme)
        for t, a in zip(m.q + m.s, q0 + s0):
            t.copy_(torch.from_numpy(a))
        return m
    d, plain = make(), make()
    d.set_particles(kind, n, None, STOKES, SETTLING)
    assert d.l_tags.dtype == torch.int64 and d.l_nodes.dtype == torch.int32 and len(d.l_q) == len(d.l_hq) == ncol
    assert np.array_equal(d.l_tags.cpu().numpy(), np.arange(1, n + 1))
    lq0, _, _ = _particle_set(shape, n, ncol, seed=5)
    for t, a in zip(d.l_q, lq0):
        t.copy_(torch.from_numpy(a))
    for t in d.l_hq:
        t.fill_(123.0)                                   # begin_step must zero them
    d.locate_particles()
    O = Particles(x, y, z, type=code, stokes=STOKES, settling=SETTLING)
    O.set(lq0)
    assert np.array_equal(d.l_nodes.cpu().numpy(), O.nodes)
    calls = []
    inner = d.TIME_SUBSTEP_PARTICLE

    def spy(dte, kco=1.0, scale_tendencies=False):
        torch.cuda.synchronize()
        if len(calls) % d.rkm_endstep == 0:
            O.begin_step()
        O.substep([t.cpu().numpy() for t in d.q], dte, kco, scale_tendencies)
        calls.append((dte, kco, scale_tendencies))
        inner(dte, kco, scale_tendencies)
    monkeypatch.setattr(d, "TIME_SUBSTEP_PARTICLE", spy)
    dtime = 2e-3
    for _ in range(2):
        d.TIME_RUNGEKUTTA(dtime)
        plain.TIME_RUNGEKUTTA(dtime)
    torch.cuda.synchronize()
    assert len(calls) == 2 * d.rkm_endstep
    assert [c[2] for c in calls[:d.rkm_endstep]] == [True] * (d.rkm_endstep - 1) + [False]
    for i in range(ncol):
        assert _equal_bits(d.l_q[i].cpu().numpy(), O.l_q[i]), (scheme, kind, "l_q", i)
        assert _equal_bits(d.l_hq[i].cpu().numpy(), O.l_hq[i]), (scheme, kind, "l_hq", i)
    assert np.array_equal(d.l_nodes.cpu().numpy(), O.nodes)
    moved = max(float(np.abs(O.l_q[i] - lq0[i]).max()) for i in range(3))
    assert moved > 1e-4                                   # (the particles went somewhere)
    for a, b in zip(d.q + d.s + d.hq + d.hs, plain.q + plain.s + plain.hq + plain.hs):
        assert torch.equal(a, b)


# ---- 5: nothing set changes nothing ----
def _kernel_rows():
    from tlab_amd.lib import load
    buf = ctypes.create_string_buffer(32768)
    load().tlab_profile_report(buf, len(buf))
    return {r.split("\t")[0]: int(r.split("\t")[1]) for r in buf.value.decode().splitlines() if "\t" in r}


def _profiled_step(d, q0, s0):
    import torch
    from tlab_amd.lib import load
    L = load()
    for t, a in zip(d.q + d.s, q0 + s0):
        t.copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    L.tlab_profile_reset(); L.tlab_profile_enable(1)
    try:
        d.TIME_RUNGEKUTTA(2e-3)
        torch.cuda.synchronize()
    finally:
        L.tlab_profile_enable(0)
    rows = _kernel_rows()
    L.tlab_profile_reset()
    return rows, [t.clone() for t in d.q + d.s + d.hq + d.hs]


def test_without_particles_the_step_launches_what_it_launched(T):
    """the kernel table of one step of a driver without particles has no k_particle row and is the table such a driver gave before any setter was
    called on its neighbour, after one was, and after the neighbour dropped its particles again; with particles the table grows by one
    k_particle_substep per substep and the fields keep their bits"""
    import torch
    from tlab_amd.dns import Dns
    shape = (70, 33, 9)
    x, y, z, q0, s0 = _case(shape)
    mk = lambda: Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False)      # noqa: E731
    never, other = mk(), mk()
    rows0, f0 = _profiled_step(never, q0, s0)
    assert rows0 and not [k for k in rows0 if "particle" in k]
    other.set_particles("tracer", 100)
    other.l_q[1].fill_(0.5)
    other.locate_particles()
    rows1, f1 = _profiled_step(other, q0, s0)
    assert rows1 == dict(rows0, k_particle_substep=3), (rows0, rows1)
    for a, b in zip(f0, f1):
        assert torch.equal(a, b)
    other.set_particles("none")
    rows2, f2 = _profiled_step(other, q0, s0)
    rows3, f3 = _profiled_step(never, q0, s0)
    assert rows2 == rows0 and rows3 == rows0
    for a, b, c in zip(f0, f2, f3):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---- 6: the sort ----
@pytest.mark.parametrize("kind", [PART_TRACER, PART_INERTIA])
@pytest.mark.parametrize("shape", SHAPES)
def test_sort_permutes_everything_together(T, shape, kind):
    import torch
    from tlab_amd.lib import load
    L = load()
    d = _driver(shape)
    x, y, z, q0, _ = _case(shape)
    ncol = 6 if kind == PART_INERTIA else 3
    d.set_particles(kind, 0, None, STOKES, SETTLING)
    for n in (1, 65, 1000):
        lq0, lh0, _ = _particle_set(shape, n, ncol, seed=9)
        O = Particles(x, y, z, type=kind, stokes=STOKES, settling=SETTLING)
        O.set(lq0, lh0)
        nodes0, tags0 = O.nodes.copy(), np.arange(1, n + 1, dtype=np.int64)
        lq, _ = _upload(lq0, 0)
        lh, _ = _upload(lh0, 1)
        nodes, tags = torch.from_numpy(nodes0).cuda(), torch.from_numpy(tags0).cuda()
        need = ctypes.c_longlong(-1)
        assert L.tlab_dns_particle_sort(d._h, n, None, None, None, None, None, 0, ctypes.byref(need)) == 0      # the size query
        assert need.value >= 24 * n and need.value % 256 == 0
        scratch = torch.empty(need.value + 256, dtype=torch.uint8, device="cuda")
        sp = (scratch.data_ptr() + 255) // 256 * 256
        # too small, misaligned: refused, nothing moved
        assert L.tlab_dns_particle_sort(d._h, n, _ptrs(lq), _ptrs(lh), nodes.data_ptr(), tags.data_ptr(), sp, need.value - 1, None) == EINVAL
        assert L.tlab_dns_particle_sort(d._h, n, _ptrs(lq), _ptrs(lh), nodes.data_ptr(), tags.data_ptr(), sp + 8, need.value, None) == EINVAL
        assert L.tlab_dns_particle_sort(d._h, n, _ptrs(lq), _ptrs(lh), nodes.data_ptr(), tags.data_ptr(), None, need.value, None) == EINVAL
        torch.cuda.synchronize()
        assert np.array_equal(tags.cpu().numpy(), tags0) and all(_equal_bits(t.cpu().numpy(), a) for t, a in zip(lq + lh, lq0 + lh0))
        assert L.tlab_dns_particle_sort(d._h, n, _ptrs(lq), _ptrs(lh), nodes.data_ptr(), tags.data_ptr(), sp, need.value, None) == 0
        torch.cuda.synchronize()
        tg = tags.cpu().numpy()
        assert np.array_equal(np.sort(tg), tags0)                                   # a permutation of 1..np
        perm = tg - 1
        for t, a in zip(lq + lh, lq0 + lh0):
            assert _equal_bits(t.cpu().numpy(), a[perm])                            # every column went with its tag
        assert np.array_equal(nodes.cpu().numpy(), nodes0[perm])
        S = Particles(x, y, z, type=kind, stokes=STOKES, settling=SETTLING)
        S.set([a[perm] for a in lq0], [a[perm] for a in lh0])
        S.nodes = nodes0[perm]
        keys = S.cell_keys()
        assert (np.diff(keys) >= 0).all(), (shape, n)
        if n == 1000:
            assert not (np.diff(O.cell_keys()) >= 0).all() and len(np.unique(keys)) > 50      # it was not sorted before, and there is something to sort
            same = np.flatnonzero(np.diff(keys) == 0)
            assert (np.diff(tg)[same] > 0).all()                                    # equal keys keep their order
        # one substep after the sort = the substep of the unsorted copy, tag by tag
        O.substep(q0, DTE, -0.6, True)
        assert _substep(d, DTE, -0.6, 1, lq, lh, nodes) == 0
        torch.cuda.synchronize()
        for i in range(ncol):
            assert _equal_bits(lq[i].cpu().numpy(), O.l_q[i][perm]) and _equal_bits(lh[i].cpu().numpy(), O.l_hq[i][perm])
        assert np.array_equal(nodes.cpu().numpy(), O.nodes[perm])
    d.set_particles("none")


def test_sort_particles_of_the_driver_keeps_the_state(T):
    """Dns.sort_particles, twice (the second call finds them sorted and reuses the scratch)"""
    import torch
    shape = (70, 33, 9)
    d = _driver(shape)
    n = 1000
    d.set_particles("tracer", n)
    lq0, _, _ = _particle_set(shape, n, 3, seed=2)
    for t, a in zip(d.l_q, lq0):
        t.copy_(torch.from_numpy(a))
    d.locate_particles()
    d.sort_particles()
    torch.cuda.synchronize()
    perm = d.l_tags.cpu().numpy() - 1
    assert np.array_equal(np.sort(perm), np.arange(n)) and not np.array_equal(perm, np.arange(n))
    for t, a in zip(d.l_q, lq0):
        assert _equal_bits(t.cpu().numpy(), a[perm])
    d.sort_particles()
    torch.cuda.synchronize()
    assert np.array_equal(d.l_tags.cpu().numpy() - 1, perm)
    d.set_particles("none")


# ---- 7: refusals ----
def test_refusals_leave_the_driver_as_it_was(T):
    import torch
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    L = load()
    shape = (20, 12, 8)
    x, y, z, q0, s0 = _case(shape)
    d = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False)
    for t, a in zip(d.q + d.s, q0 + s0):
        t.copy_(torch.from_numpy(a))
    n = 65
    d.set_particles("inertia", n, "stick", STOKES, SETTLING)
    lq0, lh0, _ = _particle_set(shape, n, 6)
    nodes0 = locate_y(lq0[1], y)

    def step():
        lq, _ = _upload(lq0, 0)
        lh, _ = _upload(lh0, 0)
        nodes = torch.from_numpy(nodes0).cuda()
        assert _substep(d, DTE, -0.6, 1, lq, lh, nodes) == 0
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in lq + lh] + [nodes.cpu().numpy()]
    before = step()
    nan, inf = float("nan"), float("inf")
    lq, _ = _upload(lq0, 0)
    lh, _ = _upload(lh0, 0)
    nodes = torch.from_numpy(nodes0).cuda()
    keep = [t.clone() for t in lq + lh] + [nodes.clone()]
    qp = d._arrays()[0]
    refused = [
        (lambda: L.tlab_dns_set_particles(d._h, 4, -1, STOKES, 0.0), EUNSUPPORTED),              # PART_TYPE_BIL_CLOUD_3
        (lambda: L.tlab_dns_set_particles(d._h, 5, -1, STOKES, 0.0), EUNSUPPORTED),              # PART_TYPE_BIL_CLOUD_4
        (lambda: L.tlab_dns_set_particles(d._h, 6, -1, STOKES, 0.0), EUNSUPPORTED),              # PART_TYPE_TINIA_1
        (lambda: L.tlab_dns_set_particles(d._h, 3, -1, STOKES, 0.0), EINVAL),
        (lambda: L.tlab_dns_set_particles(d._h, -1, -1, STOKES, 0.0), EINVAL),
        (lambda: L.tlab_dns_set_particles(d._h, 1, 3, STOKES, 0.0), EINVAL),                     # an unknown wall condition
        (lambda: L.tlab_dns_set_particles(d._h, 2, -1, 0.0, 0.0), EINVAL),                       # inertia with stokes <= 0
        (lambda: L.tlab_dns_set_particles(d._h, 2, -1, -1.0, 0.0), EINVAL),
        (lambda: L.tlab_dns_set_particles(d._h, 2, -1, nan, 0.0), EINVAL),
        (lambda: L.tlab_dns_set_particles(d._h, 2, -1, STOKES, inf), EINVAL),
        (lambda: L.tlab_dns_set_particles(d._h, 1, -1, 0.0, nan), EINVAL),
        (lambda: L.tlab_dns_set_particles(None, 1, -1, 0.0, 0.0), EINVAL),
        (lambda: L.tlab_dns_substep_particle(d._h, DTE, 1.0, 0, -1, qp, _ptrs(lq), _ptrs(lh), nodes.data_ptr()), EINVAL),
        (lambda: L.tlab_dns_substep_particle(d._h, DTE, 1.0, 0, 2 ** 31, qp, _ptrs(lq), _ptrs(lh), nodes.data_ptr()), EINVAL),
        (lambda: L.tlab_dns_substep_particle(d._h, DTE, 1.0, 0, n, None, _ptrs(lq), _ptrs(lh), nodes.data_ptr()), EINVAL),
        (lambda: L.tlab_dns_substep_particle(d._h, DTE, 1.0, 0, n, qp, None, _ptrs(lh), nodes.data_ptr()), EINVAL),
        (lambda: L.tlab_dns_substep_particle(d._h, DTE, 1.0, 0, n, qp, _ptrs(lq), None, nodes.data_ptr()), EINVAL),
        (lambda: L.tlab_dns_substep_particle(d._h, DTE, 1.0, 0, n, qp, _ptrs(lq), _ptrs(lh), None), EINVAL),
        (lambda: L.tlab_dns_substep_particle(d._h, DTE, 1.0, 0, n, qp, _ptrs(lq[:5] + [None]), _ptrs(lh), nodes.data_ptr()), EINVAL),
        (lambda: L.tlab_dns_substep_particle(None, DTE, 1.0, 0, n, qp, _ptrs(lq), _ptrs(lh), nodes.data_ptr()), EINVAL),
        (lambda: L.tlab_dns_particle_locate(d._h, -1, lq[1].data_ptr(), nodes.data_ptr()), EINVAL),
        (lambda: L.tlab_dns_particle_locate(d._h, n, None, nodes.data_ptr()), EINVAL),
        (lambda: L.tlab_dns_particle_locate(d._h, n, lq[1].data_ptr(), None), EINVAL),
    ]
    for i, (call, code) in enumerate(refused):
        assert call() == code, i
        assert len(L.tlab_last_error()) > 0
        torch.cuda.synchronize()
        for a, b in zip(keep, lq + lh + [nodes]):
            assert torch.equal(a, b), i                                                           # a refused call wrote nothing
        after = step()
        for a, b in zip(before, after):
            assert _equal_bits(a, b), i                                                           # type, wall condition, stokes, settling: as before
    # an anelastic driver
    d2 = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False)
    d2.set_anelastic(np.linspace(1.0, 0.8, len(y)))
    try:
        assert L.tlab_dns_set_particles(d2._h, 1, -1, 0.0, 0.0) == EUNSUPPORTED
    finally:
        d2.set_anelastic(None)
    # a driver without particles
    assert L.tlab_dns_substep_particle(d2._h, DTE, 1.0, 0, n, qp, _ptrs(lq), _ptrs(lh), nodes.data_ptr()) == EINVAL
    assert L.tlab_dns_particle_locate(d2._h, n, lq[1].data_ptr(), nodes.data_ptr()) == EINVAL
    with pytest.raises(T.TlabError):
        d2.TIME_SUBSTEP_PARTICLE(DTE)
    with pytest.raises(T.TlabError):
        d2.set_particles("bilinearcloudthree", 10)
    with pytest.raises(T.TlabError):
        d2.set_particles("inertia", 10, stokes=0.0)
    assert d2.l_q is None
    torch.cuda.synchronize()
    for a, b in zip(keep, lq + lh + [nodes]):
        assert torch.equal(a, b)
