"""The transfers between particles and fields on the device (k_particle_sample, k_particle_trajectories, k_particle_deposit; csrc/particles.hip)
against tests/particles_oracle.py and tests/transfers_oracle.py.  The sample and the trajectories are bit for bit (the reference's operations in its
order, no contraction; fp32 by round-to-nearest).  The deposit sums with atomic adds in the order of arrival: a node that receives one contribution
has the oracle's bits, a node that receives cnt of them is within 2 (cnt - 1) 2^-53 sum|contribution| of the oracle's particle-ordered sum -- the
bound on the difference between two orders (or trees) of summation of the same terms, each within (cnt - 1) 2^-53 sum|term| of the exact sum.

Shapes, particle counts and the hand-placed particles are those of tests/test_gpu_particles.py."""
import ctypes

import numpy as np
import pytest

from particles_oracle import Particles, locate_y, PART_TRACER, PART_INERTIA
from test_gpu_particles import (SHAPES, COUNTS, STOKES, SETTLING, VISC, SC, EINVAL, _case, _driver, _particle_set, _upload, _ptrs, _equal_bits,
                                _substep)
from transfers_oracle import deposit, default_tags, new_l_traj, trajectories

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GROUP = 8                     # PARTICLE_FIELDS_PER_LAUNCH of csrc/particles_host.hpp
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


_FIELDS = {}


def _fields(shape):
    """GROUP + 1 random fields of a shape, as numpy arrays and as device tensors, made once"""
    import torch
    if shape not in _FIELDS:
        rng = np.random.default_rng(41)
        f = [rng.uniform(-1.0, 1.0, shape[0] * shape[1] * shape[2]) for _ in range(GROUP + 1)]
        _FIELDS[shape] = (f, [torch.from_numpy(a).cuda() for a in f])
    return _FIELDS[shape]


def _oracle(shape, lq, kind=PART_TRACER):
    x, y, z, _, _ = _case(shape)
    P = Particles(x, y, z, type=kind, stokes=STOKES, settling=SETTLING)
    P.set(lq)
    return P


def _L():
    from tlab_amd.lib import load
    return load()


def _sample(d, fields, n, lq, nodes, out):
    return _L().tlab_dns_field_to_particle(d._h, len(fields), _ptrs(fields), n, _ptrs(lq), None if nodes is None else nodes.data_ptr(), _ptrs(out))


def _deposit(d, n, lq, nodes, prop, periodic, field):
    return _L().tlab_dns_particle_to_field(d._h, n, _ptrs(lq), None if nodes is None else nodes.data_ptr(), None if prop is None else prop.data_ptr(),
                                           int(periodic), None if field is None else field.data_ptr())


# ---- 1: the sample bit for bit ----
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_sample_bit_for_bit(T, shape, aligned):
    """tlab_dns_field_to_particle of 1, 3 and GROUP + 1 fields (two launches) onto random targets against Particles.interpolate, every particle
    count; the particle arrays on a 16-byte boundary and on an odd double"""
    import torch
    d = _driver(shape)
    d.set_particles("tracer", 0)
    fh, fd = _fields(shape)
    off = 0 if aligned else 1
    for n in COUNTS:
        lq0, _, _ = _particle_set(shape, n, 3)
        O = _oracle(shape, lq0)
        nodes = torch.from_numpy(O.nodes).cuda()
        lq, _ = _upload(lq0, off)
        for nvar in (1, 3, GROUP + 1):
            rng = np.random.default_rng(100 * n + nvar)
            tg0 = [rng.uniform(-2.0, 2.0, n) for _ in range(nvar)]
            want = [O.interpolate(fh[v], tg0[v]) for v in range(nvar)]
            out, hold = _upload(tg0, off)
            assert _sample(d, fd[:nvar], n, lq, nodes, out) == 0
            torch.cuda.synchronize()
            for v in range(nvar):
                assert _equal_bits(out[v].cpu().numpy(), want[v]), (shape, n, nvar, v)
            for t in hold:      # nothing outside the views was written
                assert (aligned or float(t[0]) == 0.0) and float(t[-1]) == 0.0
        for t, a in zip(lq, lq0):
            assert _equal_bits(t.cpu().numpy(), a)
    d.set_particles("none")


@pytest.mark.parametrize("shape", SHAPES)
def test_sample_of_q_equals_what_the_substep_interpolates(T, shape):
    """device against device: with l_hq = 0 and dte = 0 a tracer substep leaves in l_hq(1:3) the bits that the sample of q adds to zeros"""
    import torch
    d = _driver(shape)
    d.set_particles("tracer", 0)
    for n in COUNTS:
        lq0, _, _ = _particle_set(shape, n, 3)
        nodes0 = locate_y(lq0[1], _case(shape)[1])
        lq, _ = _upload(lq0, 0)
        lh, _ = _upload([np.zeros(n)] * 3, 0)
        out, _ = _upload([np.zeros(n)] * 3, 1)
        nodes = torch.from_numpy(nodes0).cuda()
        assert _sample(d, d.q, n, lq, nodes, out) == 0
        assert _substep(d, 0.0, 1.0, 0, lq, lh, nodes) == 0
        torch.cuda.synchronize()
        for i in range(3):
            assert _equal_bits(out[i].cpu().numpy(), lh[i].cpu().numpy()), (shape, n, i)
        assert float(out[0].abs().max()) > 0.0
    d.set_particles("none")


# ---- 2: the deposit where no two particles share a node ----
def _in_cells(shape, cells, seed):
    """one particle strictly inside each (i0, j0, k0), in a shuffled order"""
    x, y, z, _, _ = _case(shape)
    P = Particles(x, y, z)
    rng = np.random.default_rng(seed)
    cells = np.array(cells)[rng.permutation(len(cells))]
    fr = rng.uniform(0.1, 0.9, (3, len(cells)))
    lx = (cells[:, 0] + fr[0]) / P.dxi
    ly = y[cells[:, 1]] + fr[1] * (y[cells[:, 1] + 1] - y[cells[:, 1]])
    lz = (cells[:, 2] + fr[2]) / P.dzi if shape[2] > 1 else rng.uniform(-1.0, 1.0, len(cells))
    return [lx, ly, lz]


def _separate_sets(shape):
    """(name, positions): particle sets in which no two particles share a destination node -- at most one particle per cell with even i0, j0, k0
    below the seam cells; and one made only of seam cells: the corner cell in row j0 = 0, x-seam cells in the even rows above it and even planes,
    z-seam cells in the same rows at even i0 away from both ends"""
    nx, ny, nz = shape
    ev = lambda m: range(0, m, 2)      # noqa: E731
    ks = ev(nz - 1) if nz > 1 else [0]
    inner = [(i, j, k) for i in ev(nx - 1) for j in ev(ny - 1) for k in ks]
    seam = [(nx - 1, 0, nz - 1)]
    seam += [(nx - 1, j, k) for j in range(2, ny - 1, 2) for k in ks]
    if nz > 1:
        seam += [(i, j, nz - 1) for i in range(2, nx - 3, 2) for j in range(2, ny - 1, 2)]
    return [("inner", _in_cells(shape, inner, 21)), ("seam", _in_cells(shape, seam, 22))]


@pytest.mark.parametrize("shape", SHAPES)
def test_deposit_exact_where_every_node_gets_one_add(T, shape):
    import torch
    d = _driver(shape)
    d.set_particles("tracer", 0)
    for name, lq0 in _separate_sets(shape):
        n = len(lq0[0])
        assert n >= 6
        O = _oracle(shape, lq0)
        lq, _ = _upload(lq0, 0)
        nodes = torch.from_numpy(O.nodes).cuda()
        prop0 = np.random.default_rng(23).uniform(-1.0, 2.0, n)
        (prop,), _ = _upload([prop0], 1)
        for periodic in (1, 0):
            for ph, pd in ((prop0, prop), (None, None)):
                want, cnt, _ = deposit(O, ph, bool(periodic))
                assert cnt.max() <= 1 and cnt.sum() > 0, (shape, name)      # the set is what it claims to be
                if name == "seam":
                    assert cnt.sum() < (8 if shape[2] > 1 else 4) * n if not periodic else cnt.sum() == (8 if shape[2] > 1 else 4) * n
                field = torch.full((want.size + 2,), 7.0, dtype=torch.float64, device="cuda")      # garbage the entry must zero, and guards
                assert _deposit(d, n, lq, nodes, pd, periodic, field[1:-1]) == 0
                torch.cuda.synchronize()
                assert _equal_bits(field[1:-1].cpu().numpy(), want), (shape, name, periodic, ph is None)
                assert float(field[0]) == 7.0 and float(field[-1]) == 7.0
    d.set_particles("none")


# ---- 3: the deposit where many particles share nodes ----
def _crowded(shape, n=1000, crowd=200):
    """`crowd` particles in one cell in front of the set of test_gpu_particles (its hand-placed ones, then random positions)"""
    rest, _, _ = _particle_set(shape, n - crowd, 3, seed=31)
    cell = (shape[0] // 2, shape[1] // 2, shape[2] // 2)
    x, y, z, _, _ = _case(shape)
    P = Particles(x, y, z)
    rng = np.random.default_rng(32)
    fr = rng.uniform(0.0, 1.0, (3, crowd))
    first = [(cell[0] + fr[0]) / P.dxi, y[cell[1]] + fr[1] * (y[cell[1] + 1] - y[cell[1]]),
             (cell[2] + fr[2]) / P.dzi if shape[2] > 1 else fr[2]]
    return [np.concatenate([a, b]) for a, b in zip(first, rest)]


def _within_bound(got, want, cnt, mag):
    err = np.abs(got - want)
    bound = 2.0 * np.maximum(cnt - 1, 0) * U * mag
    worst = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max()) if (bound > 0).any() else 0.0
    return bool((err <= bound).all()), worst


@pytest.mark.parametrize("shape", SHAPES)
def test_deposit_crowded_within_the_reordering_bound(T, shape):
    """1000 particles, the first 200 in one cell (several waves' worth of equal destinations): per node within the bound of the module's header,
    before and after tlab_dns_particle_sort (another order of arrival and other runs for the in-wave sum); conservation and adjointness with the
    tolerances of tests/test_transfers_host.py"""
    import torch
    d = _driver(shape)
    n = 1000
    d.set_particles("tracer", n)
    lq0 = _crowded(shape, n)
    for t, a in zip(d.l_q, lq0):
        t.copy_(torch.from_numpy(a))
    d.locate_particles()
    O = _oracle(shape, lq0)
    rng = np.random.default_rng(33)
    prop0 = rng.uniform(-1.0, 2.0, n)
    nn = shape[0] * shape[1] * shape[2]
    fh, fd = _fields(shape)
    for sorted_ in (False, True):
        if sorted_:
            d.sort_particles()
            torch.cuda.synchronize()
        perm = d.l_tags.cpu().numpy() - 1
        prop = torch.from_numpy(prop0[perm]).cuda()
        for periodic in (True, False):
            for ph, pd in ((prop0, prop), (None, None)):
                want, cnt, mag = deposit(O, ph, periodic)
                assert cnt.max() >= 150
                got = d.PARTICLE_TO_FIELD(pd, periodic=periodic)
                torch.cuda.synchronize()
                g = got.cpu().numpy()
                ok, worst = _within_bound(g, want, cnt, mag)
                print("%s sorted %s periodic %s property %s: worst error / bound %.3f, most contributions on a node %d"
                      % (shape, sorted_, periodic, ph is not None, worst, cnt.max()))
                assert ok, (shape, sorted_, periodic, worst)
                assert np.array_equal(g[cnt == 0], np.zeros(int((cnt == 0).sum())))
                if periodic:      # conservation, and adjointness against the device's own sample
                    total = float(n) if ph is None else float(prop0.sum())
                    mass = float(n) if ph is None else float(np.abs(prop0).sum())
                    assert abs(float(g.sum()) - total) <= U * (n + nn + 16) * mass
                    smp = d.FIELD_TO_PARTICLE([fd[0]])[0].cpu().numpy()
                    p = np.ones(n) if ph is None else prop0[perm]
                    lhs, rhs = float(np.sum(g * fh[0])), float(np.sum(p * smp))
                    assert abs(lhs - rhs) <= U * (8 * n + nn) * mass * float(np.abs(fh[0]).max())
    d.set_particles("none")


# ---- 4: trajectories ----
@pytest.mark.parametrize("kind", ["tracer", "inertia"])
@pytest.mark.parametrize("shape", SHAPES)
def test_trajectories_bit_for_bit(T, shape, kind):
    """the default tag list and an unsorted hand-made one with a tag nobody carries; no field and two fields behind the prognostic columns; columns
    1, 2 and nsave; before and after a sort.  l_traj is prefilled with a sentinel: the other columns and the absent tag's row keep it."""
    import torch
    d = _driver(shape)
    n, nsave = 1000, 4
    ncol = 6 if kind == "inertia" else 3
    code = PART_INERTIA if kind == "inertia" else PART_TRACER
    d.set_particles(kind, n, None, STOKES, SETTLING)
    lq0, _, _ = _particle_set(shape, n, ncol, seed=44)
    for t, a in zip(d.l_q, lq0):
        t.copy_(torch.from_numpy(a))
    d.locate_particles()
    fh, fd = _fields(shape)
    lists = [("default", None, 7), ("hand", [900, 3, 2000, 64, 65, 1], None)]
    for sorted_ in (False, True):
        if sorted_:
            d.sort_particles()
        torch.cuda.synchronize()
        tags = d.l_tags.cpu().numpy()
        O = _oracle(shape, [t.cpu().numpy() for t in d.l_q], code)
        O.nodes = d.l_nodes.cpu().numpy()
        assert sorted_ == (not np.array_equal(tags, np.arange(1, n + 1)))
        for name, tg, number in lists:
            for nvar in (0, 2):
                d.set_trajectories(number=number, tags=tg, nsave=nsave, fields=fd[:nvar])
                tt = default_tags(n, number) if tg is None else np.array(tg, dtype=np.int64)
                assert np.array_equal(d.l_traj_tags, tt)
                assert d.l_traj.shape == (ncol + nvar, nsave, len(tt) + 1) and d.l_traj.dtype == torch.float32 and float(d.l_traj.abs().max()) == 0.0
                d.l_traj.fill_(SENTINEL)
                want = new_l_traj(len(tt), nsave, ncol + nvar, fill=SENTINEL)
                for counter in (1, 2, nsave):
                    rtime = 0.1 * counter + 1.0 / 3.0
                    d.traj_counter = counter - 1
                    d.ParticleTrajectories_Accumulate(rtime)
                    assert d.traj_counter == counter
                    trajectories(O, tags, tt, rtime, counter, want, fh[:nvar])
                torch.cuda.synchronize()
                got = d.l_traj.cpu().numpy()
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (shape, kind, sorted_, name, nvar)
                assert (got[:, 2] == SENTINEL).all()                           # a column no call named
                if name == "hand":
                    assert (got[:, :, 3] == SENTINEL).all()                    # the row of tag 2000
                assert (got[:, 0, 1:3] != SENTINEL).all()
                d.trajectories_written()
                assert d.traj_counter == 0 and float(d.l_traj.abs().max()) == 0.0
    d.set_particles("none")
    assert d.l_traj is None


# ---- 5: inside full steps ----
def test_two_steps_with_trajectories_and_a_deposit(T, monkeypatch):
    """two steps of Dns.TIME_RUNGEKUTTA (RK3) on (70, 33, 9) with 1000 tracers, ParticleTrajectories_Accumulate after each (TrajType = eulerian:
    q and s behind the positions) and PARTICLE_TO_FIELD at the end: trajectories bit for bit against the oracle driven beside it, the deposit within
    its bound, and q, s, l_q, l_hq, nodes and tags bit-identical to a twin that made none of the new calls"""
    import torch
    from tlab_amd.dns import Dns
    shape = (70, 33, 9)
    x, y, z, q0, s0 = _case(shape)
    n, nsave = 1000, 2

    def make():
        m = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False)
        for t, a in zip(m.q + m.s, q0 + s0):
            t.copy_(torch.from_numpy(a))
        m.set_particles("tracer", n)
        lq0, _, _ = _particle_set(shape, n, 3, seed=5)
        for t, a in zip(m.l_q, lq0):
            t.copy_(torch.from_numpy(a))
        m.locate_particles()
        return m, lq0
    (d, lq0), (twin, _) = make(), make()
    O = _oracle(shape, lq0)
    d.set_trajectories(number=10, nsave=nsave, fields=d.q + d.s)
    tt = default_tags(n, 10)
    want = new_l_traj(10, nsave, 3 + 4)
    calls = []
    inner = d.TIME_SUBSTEP_PARTICLE

    def spy(dte, kco=1.0, scale_tendencies=False):
        torch.cuda.synchronize()
        if len(calls) % d.rkm_endstep == 0:
            O.begin_step()
        O.substep([t.cpu().numpy() for t in d.q], dte, kco, scale_tendencies)
        calls.append(dte)
        inner(dte, kco, scale_tendencies)
    monkeypatch.setattr(d, "TIME_SUBSTEP_PARTICLE", spy)
    dtime = 2e-3
    for it in range(2):
        d.TIME_RUNGEKUTTA(dtime)
        twin.TIME_RUNGEKUTTA(dtime)
        d.ParticleTrajectories_Accumulate((it + 1) * dtime)
        torch.cuda.synchronize()
        trajectories(O, np.arange(1, n + 1), tt, (it + 1) * dtime, it + 1, want, [t.cpu().numpy() for t in d.q + d.s])
    field = d.PARTICLE_TO_FIELD()
    torch.cuda.synchronize()
    assert len(calls) == 2 * d.rkm_endstep
    got = d.l_traj.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert float(np.abs(got[:3, 1] - got[:3, 0])[:, 1:].max()) > 0.0       # (the particles went somewhere between the two columns)
    wf, cnt, mag = deposit(O, None, True)
    ok, worst = _within_bound(field.cpu().numpy(), wf, cnt, mag)
    print("deposit after two steps: worst error / bound %.3f" % worst)
    assert ok
    for a, b in zip(d.q + d.s + d.l_q + d.l_hq + [d.l_nodes, d.l_tags], twin.q + twin.s + twin.l_q + twin.l_hq + [twin.l_nodes, twin.l_tags]):
        assert torch.equal(a, b)
    for i in range(3):
        assert _equal_bits(d.l_q[i].cpu().numpy(), O.l_q[i])


# ---- 6: refusals ----
def test_refusals_write_nothing(T):
    import torch
    from tlab_amd.dns import Dns
    L = _L()
    shape = (20, 12, 8)
    x, y, z, q0, s0 = _case(shape)
    d = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False)
    bare = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False)      # a driver without particles
    n, nsave, ntraj = 65, 3, 4
    d.set_particles("inertia", n, None, STOKES, SETTLING)
    lq0, _, _ = _particle_set(shape, n, 6)
    lq, _ = _upload(lq0, 0)
    nodes = torch.from_numpy(locate_y(lq0[1], y)).cuda()
    tags = torch.arange(1, n + 1, dtype=torch.int64, device="cuda")
    _, fd = _fields(shape)
    out, _ = _upload([np.full(n, 3.0)] * 2, 0)
    field = torch.full((d.n,), 7.0, dtype=torch.float64, device="cuda")
    traj = torch.full((6 + 2, nsave, ntraj + 1), SENTINEL, dtype=torch.float32, device="cuda")
    keep = [t.clone() for t in lq + out + [field, traj, nodes, tags]]
    arr = lambda v: (ctypes.c_longlong * len(v))(*v)      # noqa: E731
    assert L.tlab_dns_set_trajectories(d._h, ntraj, arr([5, 60, 7, 1])) == 0
    nan = float("nan")
    f2 = _ptrs(fd[:2])
    samp = lambda h, nv, f, m, q, nd, o: L.tlab_dns_field_to_particle(h, nv, f, m, q, nd, o)      # noqa: E731
    dep = lambda h, m, q, nd, f: L.tlab_dns_particle_to_field(h, m, q, nd, None, 1, f)            # noqa: E731
    acc = lambda h, rt, c, ns, m, q, nd, tg, nv, f, tr: L.tlab_dns_trajectories_accumulate(h, rt, c, ns, m, q, nd, tg, nv, f, tr)      # noqa: E731
    N, TG, TR, Q, OUT = nodes.data_ptr(), tags.data_ptr(), traj.data_ptr(), _ptrs(lq), _ptrs(out)
    refused = [
        lambda: samp(bare._h, 2, f2, n, Q, N, OUT), lambda: samp(None, 2, f2, n, Q, N, OUT),
        lambda: samp(d._h, 0, f2, n, Q, N, OUT), lambda: samp(d._h, -1, f2, n, Q, N, OUT),
        lambda: samp(d._h, 2, f2, -1, Q, N, OUT), lambda: samp(d._h, 2, f2, 2 ** 31, Q, N, OUT),
        lambda: samp(d._h, 2, None, n, Q, N, OUT), lambda: samp(d._h, 2, f2, n, None, N, OUT),
        lambda: samp(d._h, 2, f2, n, Q, None, OUT), lambda: samp(d._h, 2, f2, n, Q, N, None),
        lambda: samp(d._h, 2, _ptrs([fd[0], None]), n, Q, N, OUT), lambda: samp(d._h, 2, f2, n, Q, N, _ptrs([out[0], None])),
        lambda: dep(bare._h, n, Q, N, field.data_ptr()), lambda: dep(None, n, Q, N, field.data_ptr()),
        lambda: dep(d._h, -1, Q, N, field.data_ptr()), lambda: dep(d._h, 2 ** 31, Q, N, field.data_ptr()),
        lambda: dep(d._h, n, None, N, field.data_ptr()), lambda: dep(d._h, n, Q, None, field.data_ptr()),
        lambda: dep(d._h, n, Q, N, None), lambda: dep(d._h, 0, Q, N, None),
        lambda: L.tlab_dns_set_trajectories(bare._h, 2, arr([1, 2])), lambda: L.tlab_dns_set_trajectories(None, 2, arr([1, 2])),
        lambda: L.tlab_dns_set_trajectories(d._h, -1, arr([1, 2])), lambda: L.tlab_dns_set_trajectories(d._h, 2, None),
        lambda: L.tlab_dns_set_trajectories(d._h, 3, arr([4, 9, 4])), lambda: L.tlab_dns_set_trajectories(d._h, 2, arr([4, 0])),
        lambda: L.tlab_dns_set_trajectories(d._h, 2, arr([-3, 4])),
        lambda: acc(bare._h, 0.5, 1, nsave, n, Q, N, TG, 2, f2, TR), lambda: acc(None, 0.5, 1, nsave, n, Q, N, TG, 2, f2, TR),
        lambda: acc(d._h, nan, 1, nsave, n, Q, N, TG, 2, f2, TR), lambda: acc(d._h, 0.5, 0, nsave, n, Q, N, TG, 2, f2, TR),
        lambda: acc(d._h, 0.5, nsave + 1, nsave, n, Q, N, TG, 2, f2, TR), lambda: acc(d._h, 0.5, 1, 0, n, Q, N, TG, 2, f2, TR),
        lambda: acc(d._h, 0.5, 1, nsave, -1, Q, N, TG, 2, f2, TR), lambda: acc(d._h, 0.5, 1, nsave, 2 ** 31, Q, N, TG, 2, f2, TR),
        lambda: acc(d._h, 0.5, 1, nsave, n, Q, N, TG, -1, f2, TR), lambda: acc(d._h, 0.5, 1, nsave, n, None, N, TG, 2, f2, TR),
        lambda: acc(d._h, 0.5, 1, nsave, n, Q, None, TG, 2, f2, TR), lambda: acc(d._h, 0.5, 1, nsave, n, Q, N, None, 2, f2, TR),
        lambda: acc(d._h, 0.5, 1, nsave, n, Q, N, TG, 2, None, TR), lambda: acc(d._h, 0.5, 1, nsave, n, Q, N, TG, 2, f2, None),
        lambda: acc(d._h, 0.5, 1, nsave, n, _ptrs(lq[:5] + [None]), N, TG, 2, f2, TR),
    ]
    for i, call in enumerate(refused):
        assert call() == EINVAL, i
        assert len(L.tlab_last_error()) > 0
        torch.cuda.synchronize()
        for a, b in zip(keep, lq + out + [field, traj, nodes, tags]):
            assert torch.equal(a, b), i
    # the refused set_trajectories calls kept the table of (5, 60, 7, 1): the accumulate still fills those rows
    assert acc(d._h, 0.5, 2, nsave, n, Q, N, TG, 2, f2, TR) == 0
    torch.cuda.synchronize()
    got = traj.cpu().numpy()
    O = _oracle(shape, lq0, PART_INERTIA)
    want = trajectories(O, np.arange(1, n + 1), np.array([5, 60, 7, 1]), 0.5, 2, new_l_traj(ntraj, nsave, 8, fill=SENTINEL),
                        [t.cpu().numpy() for t in fd[:2]])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # np = 0: no-ops, except that the deposit zeroes its field
    traj.fill_(SENTINEL)
    assert samp(d._h, 2, None, 0, None, None, None) == 0 and acc(d._h, 0.5, 1, nsave, 0, None, None, None, 2, None, None) == 0
    assert acc(d._h, 0.5, 1, nsave, 0, Q, N, TG, 2, f2, TR) == 0
    assert dep(d._h, 0, None, None, field.data_ptr()) == 0
    torch.cuda.synchronize()
    assert float(field.abs().max()) == 0.0 and (traj == SENTINEL).all()
    for a, b in zip(keep[:8], lq + out):
        assert torch.equal(a, b)
    # without a table, and after the particles were taken off (the table goes with them)
    assert L.tlab_dns_set_trajectories(d._h, 0, None) == 0
    assert acc(d._h, 0.5, 1, nsave, n, Q, N, TG, 2, f2, TR) == EINVAL
    assert L.tlab_dns_set_trajectories(d._h, ntraj, arr([5, 60, 7, 1])) == 0
    d.set_particles("none")
    d.set_particles("inertia", n, None, STOKES, SETTLING)
    assert acc(d._h, 0.5, 1, nsave, n, Q, N, TG, 2, f2, TR) == EINVAL
    torch.cuda.synchronize()
    assert (traj == SENTINEL).all()
    with pytest.raises(T.TlabError):
        bare.FIELD_TO_PARTICLE(bare.q)
    with pytest.raises(T.TlabError):
        bare.PARTICLE_TO_FIELD()
    with pytest.raises(T.TlabError):
        d.ParticleTrajectories_Accumulate(0.0)
    with pytest.raises(T.TlabError):
        d.set_trajectories(number=n + 1)


# ---- 7: behind a recorded substep ----
def test_sample_behind_a_deferred_tail_sees_the_updated_fields(T):
    """RHS and the DAXPYs of the velocities recorded (csrc/deferred.cpp), a sample of u, then the rest of the tail (the operator-in-between case of
    tests/test_gpu_deferred.py): what was recorded runs before the sample, so the values and the fields are those of the same calls executed one
    by one with the layer off -- and the sample is not that of u before the update"""
    import torch
    from tlab_amd.lib import check
    from test_gpu_deferred import _dns, _fields as _flow_fields, _ptrs as _flow_ptrs
    L = _L()
    d = _dns(1)
    f0 = _flow_fields(d, 9)
    n = 1000
    d.set_particles("tracer", n)
    rng = np.random.default_rng(3)
    for t, lo, hi in zip(d.l_q, (0.0, 0.05, 0.0), (1.0, 0.95, 1.0)):
        t.copy_(torch.from_numpy(rng.uniform(lo, hi, n)))
    d.locate_particles()
    q, s, hq, hs, txc = _flow_ptrs(d)
    dte = 1e-3

    def run(on, update=True):
        for t, a in zip(d.q + d.s, f0):
            t.copy_(a)
        for t in d.hq + d.hs:
            t.zero_()
        out = torch.zeros(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        check(L.tlab_deferred_enable(1 if on else 0), "enable")
        try:
            H, F = d.hq + d.hs, d.q + d.s
            if update:
                check(L.tlab_deferred_rhs(d._h, dte, q, s, hq, hs, txc), "rhs")
                for h, u in list(zip(H, F))[:3]:
                    check(L.tlab_deferred_axpy(d.n, dte, h.data_ptr(), u.data_ptr()), "axpy")
            check(L.tlab_dns_field_to_particle(d._h, 1, _ptrs([d.q[0]]), n, d._particle_arrays()[0], d.l_nodes.data_ptr(), _ptrs([out])), "sample")
            if update:      # (the rest of the tail: the sample in its middle makes the whole sequence run literally, with the layer on or off)
                check(L.tlab_deferred_axpy(d.n, dte, H[3].data_ptr(), F[3].data_ptr()), "axpy")
                for h in H:
                    check(L.tlab_deferred_scal(d.n, -0.5, h.data_ptr()), "scal")
            check(L.tlab_sync(), "sync")
        finally:
            check(L.tlab_deferred_enable(0), "disable")
        return [out] + [t.clone() for t in d.q + d.s]
    a, b, before = run(True), run(False), run(False, update=False)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i
    assert not torch.equal(a[0], before[0])
    d.set_particles("none")
