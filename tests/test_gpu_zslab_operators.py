"""GPU parity tests of the z-slab derivative kernels (tlab_amd/csrc/zslab.hip: k_zslab P1 / Burgers, phase A / B, z_solve and z_solve2), operator by
operator, through the public C ABI only (tlab_zslab_*), against the numpy oracle on the whole periodic z-line.  Tolerance: fp64 relative error
<= 1e-12 (BASELINE.json north_star, as tests/test_gpu_derivs.py); accumulation and the nf-field grid mapping bit for bit.

The ring of P slabs is simulated on one device.  Every field lives in one array of nz + 6 planes (the first 3 hold the global planes nz-3 .. nz-1,
the last 3 the planes 0 .. 2), so that slab r's operand pointer base + (3 + r kmax) nx ny has its halo planes in place, for P = 1 as well.  Phase 1
of every slab writes head[r] / tail[r]; phase 2 of slab r reads tail[(r-1) % P] and head[(r+1) % P] directly.  Results, head and tail sit between
guard planes holding a sentinel, overwritten results start as NaN.

Not reachable through the public ABI, and therefore not covered here:
 - the in-place scalar finish of the Burgers phase B (ffin) and halo planes in buffers of their own exist only on tlab_internal_*: they stay with
   tests/test_gpu_slab_native.py.
On a uniform periodic z the separator row of a slab equals its right neighbour's (aS == aSn, binv == binvn) and koffset does not change the
tables: a kernel that swapped them, or a plan built for the wrong koffset, would pass those cases.  The `varying` cases (VARYING, tables of
tests/periodic_tables.py whose rows all differ, device plan and oracle from the same arrays) close that: each slab's plan is built for its own
koffset from rows no other slab has, and each separator row differs from its neighbour's; tests/test_periodic_tables_host.py holds the negative
control (the oracle with slab 0's rows exchanged with slab 1's differs by more than 1e-3).
The experiment switches TLAB_ZSLAB_DUAL / _EARLY / _M are read once per process and are left alone."""
import ctypes

import numpy as np
import pytest
from conftest import rel_err
from guarded import Guarded, SENT, bits_equal      # noqa: F401
import periodic_tables as PT

pytestmark = pytest.mark.gpu
TOL = 1e-12
DTE, KCO = 2.0e-3, -5.0 / 9.0
NU = (1.0 / 500.0, 1.0 / 350.0, 1.0 / 900.0, 1.0 / 120.0)

# kmax, chunk, P (nz = P kmax): the smallest slabs that reach each sub-chunk form M x C
SLABS = {"k64_16x4_P3": (64, 0, 3), "k64_32x2_P2": (64, 32, 2), "k80_16x5_P2": (80, 0, 2), "k96_32x3_P2": (96, 0, 2), "k128_32x4_P1": (128, 0, 1),
         "k128_16x8_P2": (128, 16, 2), "k256_32x8_P2": (256, 0, 2)}
# nx, ny: 35 lines (less than a tile) / 100 (a tile + 36 lanes, 6 padding workgroups in the Burgers octet) / 512 (one octet) / 576 (9 tiles)
PLANES = {"7x5": (7, 5), "20x5": (20, 5), "64x8": (64, 8), "64x9": (64, 9)}
SHAPES = [(s, "20x5") for s in SLABS] + [(s, p) for p in ("7x5", "64x8", "64x9") for s in ("k64_16x4_P3", "k96_32x3_P2")]
GRAD_SHAPES = [(s, "20x5") for s in SLABS] + [(s, "7x5") for s in ("k64_16x4_P3", "k96_32x3_P2")]
# tables whose rows all differ (tests/periodic_tables.py): 3 slabs of 64 planes, 2 of 96, 128 (16-row sub-chunks) and 256
VARYING = [(s, p) for s in ("k64_16x4_P3", "k96_32x3_P2", "k128_16x8_P2", "k256_32x8_P2") for p in ("20x5", "7x5")]
SCHEMES = [(4, 4), (6, 6)]         # beside the default (6, 7); (5, 7) is pentadiagonal and refused


def _ids(shapes):
    return ["%s-%s" % sp for sp in shapes]


@pytest.fixture(scope="module")
def L():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tlab_amd.lib import load, check
    lib = load()
    check(lib.tlab_init(0), "tlab_init")
    check(lib.tlab_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "tlab_set_stream")
    yield lib
    for h in _GZ.values():
        lib.tlab_fdm_plan_destroy(h)
    _GZ.clear()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs and references: made once per key, shared, never modified (the arrays are read-only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
_GZ, _OG, _FIELD, _REF = {}, {}, {}, {}


def znodes(nz, periodic=True):
    return np.arange(nz) / nz * 2.0 if periodic else np.arange(nz) / (nz - 1) * 2.0


def oracle_plan(nz, m1=6, m2=7, kind=None):
    """kind = None: the plan of the uniform grid; else the tables of tests/periodic_tables.py of that kind"""
    from oracle import tlab_oracle as O
    if kind is not None:
        return PT.oracle_plan(nz, kind, (m1, m2))
    if (nz, m1, m2) not in _OG:
        _OG[nz, m1, m2] = O.FdmPlan(znodes(nz), True, True, m1, m2)
    return _OG[nz, m1, m2]


def device_plan(L, nz, m1=6, m2=7, periodic=True, kind=None):
    """kind = None: tlab_fdm_plan_create; else tlab_fdm_plan_create_from_arrays on the arrays of oracle_plan(nz, m1, m2, kind)"""
    from tlab_amd.lib import check, c_vp
    key = (nz, m1, m2, periodic, kind)
    if key not in _GZ:
        h, z = c_vp(0), znodes(nz, periodic)
        if kind is None:
            check(L.tlab_fdm_plan_create(ctypes.byref(h), nz, z.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(periodic), 1, m1, m2, 0.1),
                  "tlab_fdm_plan_create")
        else:
            assert periodic
            dp = ctypes.POINTER(ctypes.c_double)
            tab = [np.asfortranarray(a, dtype=np.float64) for a in PT.host_tables(oracle_plan(nz, m1, m2, kind))]
            tab[0], tab[2] = np.asfortranarray(tab[0][:, :3]), np.asfortranarray(tab[2][:, :3])
            check(L.tlab_fdm_plan_create_from_arrays(ctypes.byref(h), nz, 1, 0, 3, tab[1].shape[1], tab[0].ctypes.data_as(dp), tab[1].ctypes.data_as(dp),
                                                     3, tab[3].shape[1] - 3, tab[2].ctypes.data_as(dp), tab[3].ctypes.data_as(dp)),
                  "tlab_fdm_plan_create_from_arrays")
        _GZ[key] = h
    return _GZ[key]


def field(nx, ny, nz, seed):
    """0.1 uniform(-1, 1) + a smooth product of sines, flat x-fastest; neighbouring planes differ everywhere (a wrong halo row shows)."""
    key = (nx, ny, nz, seed)
    if key not in _FIELD:
        rng = np.random.default_rng(1000 * seed + nz + nx)
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        u = np.sin(0.37 * i + 0.3 * seed) * np.cos(0.61 * j + 0.2) * np.sin(2.0 * np.pi * (1 + seed % 3) * k / nz + 0.1 * seed)
        u = (u + 0.1 * rng.uniform(-1, 1, u.shape)).ravel()
        u.setflags(write=False)
        _FIELD[key] = u
    return _FIELD[key]


def ref_partial(nx, ny, nz, u, key, m=(6, 7), kind=None):
    from oracle import tlab_oracle as O
    key = ("p1", nx, ny, nz, m, kind) + key
    if key not in _REF:
        r = O.opr_partial(3, O.OPR_P1, nx, ny, nz, 0, oracle_plan(nz, *m, kind=kind), u)[0]
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def ref_burgers(nx, ny, nz, nu, s, vel, key, m=(6, 7), kind=None):
    from oracle import tlab_oracle as O
    key = ("burgers", nx, ny, nz, m, kind, nu) + key
    if key not in _REF:
        r = O.opr_burgers(3, nx, ny, nz, 0, oracle_plan(nz, *m, kind=kind), nu, s, vel)[0]
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the ring of slabs on one device
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Ring:
    def __init__(self, L, slab, plane, m=(6, 7), kind=None):
        """kind: the tables of the z direction (None: the uniform grid's; "varying": rows that all differ), for the device plan and the oracle alike"""
        from tlab_amd.lib import check, c_vp
        self.L, self.kind = L, kind
        self.kmax, self.chunk, self.P = SLABS[slab]
        self.nx, self.ny = PLANES[plane]
        self.nz, self.nl, self.m = self.kmax * self.P, self.nx * self.ny, m
        self.plans = []
        gz = device_plan(L, self.nz, *m, kind=kind)
        for r in range(self.P):
            h = c_vp(0)
            # M x C accepted; with `varying` tables the separator coupling stays below the plan's 1e-19 limit at the full amplitude for every slab used
            # here (worked out in numpy from the tables: 2.5e-27 and 8.4e-24 for the two systems at kmax = 64, the thinnest; every plan was accepted):
            # no slab needed a lower amplitude
            check(L.tlab_zslab_plan_create(ctypes.byref(h), gz, self.kmax, r * self.kmax, self.chunk), "tlab_zslab_plan_create")
            self.plans.append(h)

    def close(self):
        for h in self.plans:
            self.L.tlab_zslab_plan_destroy(h)
        self.plans = []

    def field(self, seed):
        return field(self.nx, self.ny, self.nz, seed)

    def operand(self, u):
        """nz + 6 planes with the periodic wrap in place; .slab(r) is the pointer of slab r's first plane"""
        import torch
        a = np.asarray(u).reshape(self.nz, self.nl)
        t = torch.from_numpy(np.concatenate([a[-3:], a, a[:3]]).ravel()).cuda()
        return Operand(t, self)

    def result(self, fill):
        """nz planes between two guard planes"""
        return Guarded(self.nz * self.nl, 2 * self.nl, fill)

    def out(self, res, r):
        return res.ptr(r * self.kmax * self.nl)

    def messages(self, rows):
        """head[r], tail[r]: [rows][nl] each, NaN, between guard rows of at least one tile"""
        g = max(self.nl, 64)
        return [Guarded(rows * self.nl, g, float("nan")) for _ in range(self.P)], [Guarded(rows * self.nl, g, float("nan")) for _ in range(self.P)]

    def check_messages(self, head, tail, what, written=None):
        """After phase 1 (written = None): every row written, the guard rows not; returns the messages.  After phase 2: equal to `written`."""
        now = []
        for r in range(self.P):
            for name, msg in (("head", head[r]), ("tail", tail[r])):
                assert msg.guards_intact(), (what, name, r, "guard rows written")
                now.append(msg.host())
                assert not np.isnan(now[-1]).any(), (what, name, r, "message rows left unwritten")
                assert written is None or bits_equal(now[-1], written[len(now) - 1]), (what, name, r, "phase 2 wrote into the messages")
        return now


class Operand:
    def __init__(self, t, ring):
        self.t, self.ring, self.snapshot = t, ring, t.clone()

    def slab(self, r):
        from tlab_amd.lib import c_vp
        return c_vp(self.t.data_ptr() + 8 * (3 + r * self.ring.kmax) * self.ring.nl)

    def unchanged(self):
        import torch
        return bool(torch.equal(self.t, self.snapshot))


@pytest.fixture
def ring(L, request):
    made = []

    def make(slab, plane, m=(6, 7), kind=None):
        made.append(Ring(L, slab, plane, m, kind))
        return made[-1]
    yield make
    for r in made:
        r.close()


def nan_result_untouched(res):
    return res.guards_intact() and bool(np.isnan(res.host()).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the operators
# ---------------------------------------------------------------------------------------------------------------------------------------------
def run_partial(R, u, ub, scale, prior, what):
    """Phase 1 + phase 2 of tlab_zslab_partial_z on every slab; returns (overwrite result, accumulated result) as host arrays."""
    from tlab_amd.lib import check
    L = R.L
    du, dub = R.operand(u), (R.operand(ub) if ub is not None else None)
    head, tail = R.messages(1)
    res = R.result(float("nan"))
    for r in range(R.P):            # phase 1 writes nothing but head and tail (the result pointer is ignored)
        check(L.tlab_zslab_partial_z(R.plans[r], 1, R.nx, R.ny, du.slab(r), dub.slab(r) if dub else None, scale, head[r].ptr(), tail[r].ptr(), None, None,
                                     R.out(res, r), 0), "tlab_zslab_partial_z phase 1")
    sent = R.check_messages(head, tail, what)
    assert nan_result_untouched(res), (what, "phase 1 wrote into the result")
    acc = R.result(prior)
    for a, dst in ((0, res), (1, acc)):
        for r in range(R.P):
            check(L.tlab_zslab_partial_z(R.plans[r], 2, R.nx, R.ny, du.slab(r), dub.slab(r) if dub else None, scale, None, None,
                                         tail[(r - 1) % R.P].ptr(), head[(r + 1) % R.P].ptr(), R.out(dst, r), a), "tlab_zslab_partial_z phase 2")
        assert dst.guards_intact(), (what, "acc=%d" % a, "guard planes of the result written")
    assert du.unchanged() and (dub is None or dub.unchanged()), (what, "operand modified")
    R.check_messages(head, tail, what, sent)
    return res.host(), acc.host()


def check_overwrite_and_accumulate(got, got_acc, ref, prior, what):
    assert not np.isnan(got).any(), (what, "result planes left unwritten")
    err = rel_err(got, ref)
    print("%s: rel_err %.3e" % (what, err))
    assert err <= TOL, (what, err)
    assert bits_equal(got_acc, prior + got), (what, "acc = 1 is not prior + (acc = 0 result) to the bit", float(np.abs(got_acc - (prior + got)).max()))


def partial_cases(R, m=(6, 7)):
    nx, ny, nz = R.nx, R.ny, R.nz
    u, ub, prior = R.field(1), R.field(2), R.field(9)
    tag = "partial_z %dx%d kmax=%d chunk=%d P=%d scheme=%s%s" % (nx, ny, R.kmax, R.chunk, R.P, m, " %s tables" % R.kind if R.kind else "")
    got, acc = run_partial(R, u, None, 0.0, prior, tag)
    check_overwrite_and_accumulate(got, acc, ref_partial(nx, ny, nz, u, (1,), m, R.kind), prior, tag)
    scale = 1.0 / DTE
    comb = u + scale * ub
    got, acc = run_partial(R, u, ub, scale, prior, tag + " ub")
    check_overwrite_and_accumulate(got, acc, ref_partial(nx, ny, nz, comb, (1, 2, scale), m, R.kind), prior, tag + " ub")


@pytest.mark.parametrize("slab,plane", SHAPES, ids=_ids(SHAPES))
def test_partial_z(ring, slab, plane):
    """tlab_zslab_partial_z, ub = NULL and u + ub / dte; overwrite against the oracle, accumulation bit for bit."""
    partial_cases(ring(slab, plane))


def run_burgers(R, nu, s, vel, prior, what):
    """tlab_zslab_burgers_z (one field); returns (overwrite result, accumulated result, heads, tails) as host arrays."""
    from tlab_amd.lib import check
    L = R.L
    ds, dv = R.operand(s), R.operand(vel)
    head, tail = R.messages(2)
    res = R.result(float("nan"))
    for r in range(R.P):
        check(L.tlab_zslab_burgers_z(R.plans[r], 1, R.nx, R.ny, nu, ds.slab(r), dv.slab(r), head[r].ptr(), tail[r].ptr(), None, None, R.out(res, r), 0),
              "tlab_zslab_burgers_z phase 1")
    sent = R.check_messages(head, tail, what)
    assert nan_result_untouched(res), (what, "phase 1 wrote into the result")
    acc = R.result(prior)
    for a, dst in ((0, res), (1, acc)):
        for r in range(R.P):
            check(L.tlab_zslab_burgers_z(R.plans[r], 2, R.nx, R.ny, nu, ds.slab(r), dv.slab(r), None, None, tail[(r - 1) % R.P].ptr(),
                                         head[(r + 1) % R.P].ptr(), R.out(dst, r), a), "tlab_zslab_burgers_z phase 2")
        assert dst.guards_intact(), (what, "acc=%d" % a, "guard planes of the result written")
    assert ds.unchanged() and dv.unchanged(), (what, "operand modified")
    R.check_messages(head, tail, what, sent)
    return res.host(), acc.host(), [h.host() for h in head], [t.host() for t in tail]


def burgers_cases(R, m=(6, 7)):
    nx, ny, nz = R.nx, R.ny, R.nz
    s, vel, prior = R.field(3), R.field(4), R.field(9)
    tag = "burgers_z %dx%d kmax=%d chunk=%d P=%d scheme=%s%s" % (nx, ny, R.kmax, R.chunk, R.P, m, " %s tables" % R.kind if R.kind else "")
    got, acc, _, _ = run_burgers(R, NU[0], s, vel, prior, tag)
    check_overwrite_and_accumulate(got, acc, ref_burgers(nx, ny, nz, NU[0], s, vel, (3, 4), m, R.kind), prior, tag)


@pytest.mark.parametrize("slab,plane", SHAPES, ids=_ids(SHAPES))
def test_burgers_z(ring, slab, plane):
    """tlab_zslab_burgers_z with distinct s and vel; overwrite against the oracle, accumulation bit for bit."""
    burgers_cases(ring(slab, plane))


@pytest.mark.parametrize("slab,plane", VARYING, ids=_ids(VARYING))
def test_partial_z_varying_tables(ring, slab, plane):
    """test_partial_z on tables whose rows all differ: every slab's plan from rows of its own, every separator row unlike its neighbour's."""
    partial_cases(ring(slab, plane, kind="varying"))


@pytest.mark.parametrize("slab,plane", VARYING, ids=_ids(VARYING))
def test_burgers_z_varying_tables(ring, slab, plane):
    """test_burgers_z on tables whose rows all differ (both systems, each with its own rows)."""
    burgers_cases(ring(slab, plane, kind="varying"))


@pytest.mark.parametrize("slab,plane", SHAPES, ids=_ids(SHAPES))
def test_burgers_z_n(ring, slab, plane):
    """tlab_zslab_burgers_z_n, nf = 1 .. 4: every field with its own nu, operand and result, the velocity being the last operand (the w equation:
    s[f] == vel).  Each field against the oracle, and results and messages [nf][2][nlines] bit-identical to the one-field call on the same data."""
    from tlab_amd.lib import check, c_vp
    R = ring(slab, plane)
    L, nx, ny, nz, nl = R.L, R.nx, R.ny, R.nz, R.nl
    fields, prior = [R.field(10 + f) for f in range(4)], [R.field(20 + f) for f in range(4)]
    for nf in (1, 2, 3, 4):
        tag = "burgers_z_n nf=%d %dx%d kmax=%d chunk=%d P=%d" % (nf, nx, ny, R.kmax, R.chunk, R.P)
        vel = fields[nf - 1]
        ops = [R.operand(fields[f]) for f in range(nf)]
        nus = (ctypes.c_double * nf)(*NU[:nf])
        head, tail = R.messages(2 * nf)
        res = [R.result(float("nan")) for _ in range(nf)]
        acc = [R.result(prior[f]) for f in range(nf)]
        sp = lambda r: (c_vp * nf)(*[o.slab(r).value for o in ops])                              # noqa: E731
        rp = lambda dst, r: (c_vp * nf)(*[R.out(d, r).value for d in dst])                       # noqa: E731
        for r in range(R.P):
            check(L.tlab_zslab_burgers_z_n(R.plans[r], 1, nx, ny, nf, nus, sp(r), ops[nf - 1].slab(r), head[r].ptr(), tail[r].ptr(), None, None, rp(res, r), 0),
                  "tlab_zslab_burgers_z_n phase 1")
        sent = R.check_messages(head, tail, tag)
        assert all(nan_result_untouched(d) for d in res), (tag, "phase 1 wrote into a result")
        for a, dst in ((0, res), (1, acc)):
            for r in range(R.P):
                check(L.tlab_zslab_burgers_z_n(R.plans[r], 2, nx, ny, nf, nus, sp(r), ops[nf - 1].slab(r), None, None, tail[(r - 1) % R.P].ptr(),
                                               head[(r + 1) % R.P].ptr(), rp(dst, r), a), "tlab_zslab_burgers_z_n phase 2")
            assert all(d.guards_intact() for d in dst), (tag, "acc=%d" % a, "guard planes of a result written")
        assert all(o.unchanged() for o in ops), (tag, "operand modified")
        R.check_messages(head, tail, tag, sent)
        for f in range(nf):
            ftag = tag + " field %d" % f
            got, gacc = res[f].host(), acc[f].host()
            check_overwrite_and_accumulate(got, gacc, ref_burgers(nx, ny, nz, NU[f], fields[f], vel, (10 + f, 10 + nf - 1)), prior[f], ftag)
            one, one_acc, h1, t1 = run_burgers(R, NU[f], fields[f], vel, prior[f], ftag + " (one-field call)")
            assert bits_equal(got, one) and bits_equal(gacc, one_acc), (ftag, "differs from the one-field call", float(np.abs(got - one).max()))
            for r in range(R.P):
                assert bits_equal(head[r].host()[2 * f * nl:(2 * f + 2) * nl], h1[r]), (ftag, "head rows differ from the one-field call", r)
                assert bits_equal(tail[r].host()[2 * f * nl:(2 * f + 2) * nl], t1[r]), (ftag, "tail rows differ from the one-field call", r)


@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("slab,plane", GRAD_SHAPES, ids=_ids(GRAD_SHAPES))
def test_gradient_final_z(ring, slab, plane, scale):
    """tlab_zslab_gradient_final_z after phase 1 of tlab_zslab_partial_z: hv = h - dp/dz, hv = 0 on the planes j = 0 and j = ny - 1, q += dte hv,
    h = scale ? kco hv : hv, restated in numpy from the oracle's dp/dz."""
    from tlab_amd.lib import check
    R = ring(slab, plane)
    L, nx, ny, nz, nl = R.L, R.nx, R.ny, R.nz, R.nl
    tag = "gradient_final_z scale=%d %dx%d kmax=%d chunk=%d P=%d" % (scale, nx, ny, R.kmax, R.chunk, R.P)
    p, q0, h0 = R.field(5), R.field(6), R.field(7)
    dp = R.operand(p)
    head, tail = R.messages(1)
    q, h = R.result(q0), R.result(h0)
    for r in range(R.P):
        check(L.tlab_zslab_partial_z(R.plans[r], 1, nx, ny, dp.slab(r), None, 0.0, head[r].ptr(), tail[r].ptr(), None, None, None, 0), "tlab_zslab_partial_z phase 1")
    sent = R.check_messages(head, tail, tag)
    assert bits_equal(q.host(), q0) and bits_equal(h.host(), h0), (tag, "phase 1 wrote into q or h")
    for r in range(R.P):
        check(L.tlab_zslab_gradient_final_z(R.plans[r], nx, ny, dp.slab(r), tail[(r - 1) % R.P].ptr(), head[(r + 1) % R.P].ptr(), R.out(q, r), R.out(h, r),
                                            DTE, KCO, scale), "tlab_zslab_gradient_final_z")
    assert q.guards_intact() and h.guards_intact(), (tag, "guard planes written")
    assert dp.unchanged(), (tag, "operand modified")
    R.check_messages(head, tail, tag, sent)
    wall = np.zeros((nz, ny, nx), dtype=bool)
    wall[:, 0, :] = wall[:, ny - 1, :] = True
    wall = wall.ravel()
    hv = np.where(wall, 0.0, h0 - ref_partial(nx, ny, nz, p, (5,)))
    q_ref, h_ref = q0 + DTE * hv, (KCO * hv if scale else hv)
    gq, gh = q.host(), h.host()
    eq, eh = rel_err(gq, q_ref), rel_err(gh, h_ref)
    print("%s: rel_err q %.3e h %.3e" % (tag, eq, eh))
    assert eq <= TOL and eh <= TOL, (tag, eq, eh)
    assert np.all(gh[wall] == 0.0), (tag, "wall rows of h are not exactly zero")
    assert bits_equal(gq[wall], q0[wall]), (tag, "q changed on the wall rows")
    assert np.all(gh[~wall] != 0.0), (tag, "h vanishes off the walls: wall row misplaced")


@pytest.mark.parametrize("m1,m2", SCHEMES)
def test_other_schemes(ring, m1, m2):
    """CompactJacobian4 and CompactJacobian6 (3- and 5-diagonal right-hand sides: c2_1 = 0, c3_2 = 0) at kmax = 64, P = 3, 20 x 5: a scheme that
    plan_create accepts must meet the same 1e-12."""
    R = ring("k64_16x4_P3", "20x5", (m1, m2))
    partial_cases(R, (m1, m2))
    burgers_cases(R, (m1, m2))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# refusals: TlabError, no kernel runs
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_pentadiagonal_scheme_is_refused(L):
    from tlab_amd.lib import check, c_vp, TlabError
    h = c_vp(0)
    with pytest.raises(TlabError):
        check(L.tlab_zslab_plan_create(ctypes.byref(h), device_plan(L, 192, 5, 7), 64, 0, 0), "tlab_zslab_plan_create")
    assert not h.value


@pytest.mark.parametrize("what,nz,periodic,kmax,koffset,chunk", [
    ("accepted", 128, True, 64, 64, 0),                     # the control: the same call with nothing wrong
    ("non_periodic_plan", 128, False, 64, 0, 0),
    ("nz_not_a_multiple_of_kmax", 192, True, 128, 0, 0),
    ("koffset_not_a_multiple_of_kmax", 128, True, 64, 32, 0),
    ("koffset_beyond_nz", 128, True, 64, 128, 0),
    ("koffset_negative", 128, True, 64, -64, 0),
    ("kmax_48_too_thin", 96, True, 48, 0, 0),
    ("kmax_144_nine_sub_chunks", 288, True, 144, 0, 0),
    ("kmax_288_nine_sub_chunks", 576, True, 288, 0, 0),
    ("chunk_32_with_kmax_80", 160, True, 80, 0, 32),
    ("chunk_24", 192, True, 96, 0, 24)], ids=lambda v: v if isinstance(v, str) else "")
def test_plan_refusals(L, what, nz, periodic, kmax, koffset, chunk):
    from tlab_amd.lib import check, c_vp, TlabError
    gz, h = device_plan(L, nz, periodic=periodic), c_vp(0)
    if what == "accepted":
        check(L.tlab_zslab_plan_create(ctypes.byref(h), gz, kmax, koffset, chunk), what)
        assert h.value
        L.tlab_zslab_plan_destroy(h)
        return
    with pytest.raises(TlabError):
        check(L.tlab_zslab_plan_create(ctypes.byref(h), gz, kmax, koffset, chunk), what)
    assert not h.value, (what, "a refused creation left a plan behind")


def test_launch_refusals(ring):
    """Aliased results and a field count out of range are refused before any launch: the results keep their NaN."""
    from tlab_amd.lib import check, c_vp, TlabError
    R = ring("k64_32x2_P2", "7x5")
    L, nx, ny = R.L, R.nx, R.ny
    u, ub, vel = R.operand(R.field(1)), R.operand(R.field(2)), R.operand(R.field(4))
    head, tail = R.messages(10)
    for m in head + tail:
        m.body.fill_(0.5)          # valid interface values for the launches that must not happen
    res = [R.result(float("nan")) for _ in range(5)]
    pl, tl, hr = R.plans[0], tail[1].ptr(), head[1].ptr()

    def refused(rc, what):
        with pytest.raises(TlabError):
            check(rc, what)
    refused(L.tlab_zslab_partial_z(pl, 2, nx, ny, u.slab(0), None, 0.0, None, None, tl, hr, u.slab(0), 0), "partial_z: result == u")
    refused(L.tlab_zslab_partial_z(pl, 2, nx, ny, u.slab(0), ub.slab(0), 1.0, None, None, tl, hr, ub.slab(0), 0), "partial_z: result == ub")
    refused(L.tlab_zslab_partial_z(pl, 3, nx, ny, u.slab(0), None, 0.0, head[0].ptr(), tail[0].ptr(), tl, hr, R.out(res[0], 0), 0), "partial_z: phase 3")
    refused(L.tlab_zslab_burgers_z(pl, 2, nx, ny, NU[0], u.slab(0), vel.slab(0), None, None, tl, hr, u.slab(0), 0), "burgers_z: result == s")
    refused(L.tlab_zslab_burgers_z(pl, 2, nx, ny, NU[0], u.slab(0), vel.slab(0), None, None, tl, hr, vel.slab(0), 0), "burgers_z: result == vel")
    refused(L.tlab_zslab_gradient_final_z(pl, nx, ny, u.slab(0), tl, hr, R.out(res[0], 0), R.out(res[0], 0), DTE, KCO, 1), "gradient_final_z: q == h")
    nus = (ctypes.c_double * 5)(*(NU + (1e-3,)))
    sp = (c_vp * 5)(*[o.slab(0).value for o in (u, ub, vel, u, ub)])
    rp = (c_vp * 5)(*[R.out(d, 0).value for d in res])
    for phase in (1, 2):
        for nf in (0, 5):
            refused(L.tlab_zslab_burgers_z_n(pl, phase, nx, ny, nf, nus, sp, vel.slab(0), head[0].ptr(), tail[0].ptr(), tl, hr, rp, 0), "burgers_z_n: nf = %d" % nf)
    for f in range(3):              # result f aliases its own operand / the velocity
        for alias in (sp[f], vel.slab(0).value):
            bad = (c_vp * 3)(*[alias if g == f else rp[g] for g in range(3)])
            refused(L.tlab_zslab_burgers_z_n(pl, 2, nx, ny, 3, nus, sp, vel.slab(0), None, None, tl, hr, bad, 0), "burgers_z_n: aliased result %d" % f)
    assert all(nan_result_untouched(d) for d in res), "a refused call wrote into a result"
    assert u.unchanged() and ub.unchanged() and vel.unchanged(), "a refused call wrote into an operand"
    for m in head + tail:
        assert m.guards_intact() and bool((m.body == 0.5).all()), "a refused call wrote into head / tail"
