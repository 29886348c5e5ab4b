"""GPU parity tests of the single-domain derivative kernels along a PERIODIC direction -- k_xline along x; k_rtile, k_htile and k_ptile along z --
on tables whose rows differ (tests/periodic_tables.py), through the public C ABI only: tlab_fdm_plan_create_from_arrays, tlab_opr_partial,
tlab_opr_burgers, tlab_opr_partial_add, tlab_opr_burgers_add_n, against the numpy oracle working from the same arrays.  Tolerance: fp64 relative
error <= 1e-12 (BASELINE.json north_star).

With the tables of a uniform grid the cyclic system is circulant, and a kernel that reads another chunk's rows, transposes the dense separator
inverse or reverses the lane order of its per-lane tables computes the same numbers; on `varying` tables it is wrong by 1e-1 (tests/
test_periodic_tables_host.py).  The table content also decides which kernel variant runs, so every case asserts the variant it reached, the
expectation read off the dispatch rules (operators.cpp xline_chunks / xline_wide_ok, fdm_plan.cpp tlab_fdm_plan::system, kernels.hip launch_xline, htile.hip
ptile_ok), not off the run:

 x lines   n     equal                                wander                               varying
           256   64 chunks, rows equal: scalar loads  64 chunks, per-lane tables in LDS    64 chunks, per-lane tables in LDS
           512   64 chunks, rows equal (the kernel    64 chunks, per-lane tables in LDS    64 chunks, per-lane tables in LDS
                 keeps per-chunk tables in LDS all the same: launch_xline has no scalar-load form at 512 points)
           1024  128 chunks (2 waves), rows equal     128 chunks, doubles in LDS           64 chunks: ONE wave, 16 rows per lane (the float-difference
                                                                                           form of the wide kernels is not exact: xline_wide_ok)
           2048  256 chunks (4 waves), scalar loads   256 chunks, float differences        0 chunks: the generic kernel (path 1) -- a check of that
                 in the two-system modes                                                   kernel, not coverage of a fast one
 z lines   every length and kind on the tile kernels (path 3).  tlab_set_tuning(2, 1): k_rtile for everything (two launches for OPR_P2_P1 and
           Burgers); (2, 2): k_htile<P1 / P2 / P2_P1 / BURGERS>, and k_ptile<BURGERS> where ptile_ok says so: 512 / 1024 points, a line count
           that is a multiple of the tile (288 = 9 x 32 = 18 x 16; 200 is not) and interior chunks equal to the bit, i.e. `equal` tables only --
           on `wander` and `varying` tables the same shape stays on k_htile<BURGERS>.

Every result, tmp1, tmp2 and accumulated tendency lives between guard zones of two planes (at least one tile of 64 lines) holding a sentinel;
after every call the guards are intact, overwritten outputs (NaN before) hold no NaN, and every operand equals its snapshot to the bit.  200 lines
= 6 tiles of 32 + 8 lines = 3 tiles of 64 + 8; 15 x lines = 3 workgroups of 4 + 3."""
import ctypes

import numpy as np
import pytest
from conftest import rel_err
from guarded import Guarded
import periodic_tables as PT

pytestmark = pytest.mark.gpu
TOL = 1e-12
NU = (1.0 / 500.0, 1.0 / 350.0, 1.0 / 900.0)
SCALE = 0.75
DEFAULT = (6, 7)
SCHEMES = [(4, 4), (6, 6)]

# d, (nx, ny, nz), kind, scheme
X_CASES = ([(n, 5, 3, kind, DEFAULT) for n in (256, 512, 1024, 2048) for kind in PT.KINDS] +
           [(512, 16, 5, "varying", DEFAULT)] +                       # 80 lines: more than a wave of lines, 20 workgroups
           [(512, 5, 3, "varying", m) for m in SCHEMES])
# 40 x 5 = 200 lines: a partial last tile for 32- and 64-line tiles (and for the 16-line tiles of 1024 points); 96 x 3 = 288: the shape k_ptile accepts
Z_CASES = ([(40, 5, n, kind, DEFAULT) for n in (64, 256, 512, 1024) for kind in PT.KINDS] +
           [(96, 3, n, kind, DEFAULT) for n in (512, 1024) for kind in PT.KINDS] +
           [(40, 5, 256, "varying", m) for m in SCHEMES] +            # k_rtile (policy 1) / k_htile (policy 2)
           [(96, 3, 512, "equal", m) for m in SCHEMES])               # k_ptile (policy 2)


def _id(c):
    return "%dx%dx%d-%s-%d%d" % (c[0], c[1], c[2], c[3], c[4][0], c[4][1])


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    from tlab_amd.lib import load, check
    T.init(0)
    check(load().tlab_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "tlab_set_stream")
    yield T
    _DEV.clear()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs and references: made once per key, shared, never modified (the arrays are read-only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
_FIELD, _REF, _DEV = {}, {}, {}


def field(nx, ny, nz, seed):
    """a smooth product of sines + 0.1 uniform(-1, 1), flat x-fastest: neighbouring rows and lines differ everywhere"""
    key = (nx, ny, nz, seed)
    if key not in _FIELD:
        rng = np.random.default_rng([nx, ny, nz, seed])
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        u = np.sin(2.0 * np.pi * (1 + seed % 3) * i / nx + 0.3 * seed) * np.cos(0.61 * j + 0.2) * np.sin(2.0 * np.pi * (1 + seed % 2) * k / nz + 0.1 * seed + 0.5)
        u = (u + 0.1 * rng.uniform(-1, 1, u.shape)).ravel()
        u.setflags(write=False)
        _FIELD[key] = u
    return _FIELD[key]


def references(d, nx, ny, nz, kind, m):
    """The oracle's results of every operator of a case (shared by the two tile policies)."""
    from oracle import tlab_oracle as O
    key = (d, nx, ny, nz, kind, m)
    if key not in _REF:
        og = PT.oracle_plan((nx, ny, nz)[d - 1], kind, m)
        f = [field(nx, ny, nz, s) for s in range(7)]
        p2, p1 = O.opr_partial(d, O.OPR_P2_P1, nx, ny, nz, 0, og, f[0])
        r = {"p1": p1, "p2": p2,
             "b_self": O.opr_burgers(d, nx, ny, nz, 0, og, NU[0], f[0], f[0])[0],
             "p_add": f[4] + O.opr_partial(d, O.OPR_P1, nx, ny, nz, 0, og, f[0] + SCALE * f[2])[0],
             "b_n": [O.opr_burgers(d, nx, ny, nz, 0, og, NU[i], f[i], f[1])[0] for i in range(3)]}
        r["b_uin"] = r["b_n"][0]                 # field 0 advected by field 1 with NU[0]
        for a in [r["p1"], r["p2"], r["b_self"], r["p_add"]] + r["b_n"]:
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def device_plan(T, n, kind, m):
    key = (n, kind, m)
    if key not in _DEV:
        _DEV[key] = PT.device_plan(T, PT.oracle_plan(n, kind, m))
    return _DEV[key]


def profiled(L, fn):
    """fn() with every launch timed by the library; returns the set of kernel names it launched"""
    import torch
    L.tlab_profile_filter(None); L.tlab_profile_reset(); L.tlab_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.tlab_profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 14)
    L.tlab_profile_report(buf, len(buf))
    L.tlab_profile_reset()
    return {ln.split("\t")[0] for ln in buf.value.decode().split("\n") if ln}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# what the dispatch rules say
# ---------------------------------------------------------------------------------------------------------------------------------------------
def x_expectation(n, kind):
    """(chunks = tlab_fdm_plan_info 8, lane-invariant = info 9, kernel path) of periodic x lines (operators.cpp xline_chunks): 256 / 512 points: one wave
    per line whatever the tables; 1024 / 2048: 2 / 4 waves while the tables can be kept as chunk 0 + float differences -- rows equal to the bit or
    apart by rounding (1e-13: the difference has about 10 significant bits), not rows 5 % apart --, else one wave at 1024 points and the generic
    kernel at 2048.  Lane-invariant: every row bit-identical (info 9 answers 0 where there are no chunks)."""
    chunks = {256: 64, 512: 64, 1024: 64 if kind == "varying" else 128, 2048: 0 if kind == "varying" else 256}[n]
    return chunks, 1 if (kind == "equal" and chunks) else 0, 2 if chunks else 1


def z_expectation(op, n, lines, kind, policy):
    """kernel names a z-line operator must launch under tlab_set_tuning(2, policy) (operators.cpp tlab_opr_partial / tlab_opr_burgers / run_p1_tile,
    htile.hip launch_htile_m / ptile_ok)"""
    tile = 16 if n == 1024 else 32                   # Burgers tiles: 16 lines at 1024 points (32 chunks of 32 rows)
    ptile = policy == 2 and kind == "equal" and n in (512, 1024) and lines % tile == 0
    burgers = {"k_ptile<BURGERS>"} if ptile else {"k_htile<BURGERS>"}
    if policy == 1:
        return {"p1": {"k_rtile<P1>"}, "p2": {"k_rtile<P2>"}, "p2_p1": {"k_rtile<P1>", "k_rtile<P2>"}, "burgers": {"k_rtile<P1>", "k_rtile<BURGERS_D1IN>"},
                "p_add": {"k_rtile<P1>"}, "b_n": {"k_rtile<P1>", "k_rtile<BURGERS_D1IN>"}}[op]
    # the accumulating first derivative keeps the 64-line tiles up to 512 points; at 1024 their 64-row chunks spill and it takes the 32-line ones
    return {"p1": {"k_htile<P1>"}, "p2": {"k_htile<P2>"}, "p2_p1": {"k_htile<P2_P1>"}, "burgers": burgers,
            "p_add": {"k_htile<P1>"} if n == 1024 else {"k_rtile<P1>"}, "b_n": burgers}[op]


FAMILIES = ("k_xline", "k_rtile", "k_htile", "k_ptile", "k_generic")


def check_names(names, must, tag):
    """the launches include `must`, and no derivative kernel of a family that `must` does not name"""
    assert must <= names, (tag, "expected", sorted(must), "launched", sorted(names))
    allowed = {f for f in FAMILIES if any(k.startswith(f) for k in must)}
    stray = {k for k in names if k.startswith(FAMILIES) and not k.startswith(tuple(allowed))}
    assert not stray, (tag, "expected", sorted(must), "also launched", sorted(stray))
    if "k_htile<BURGERS>" in must:
        assert "k_ptile<BURGERS>" not in names, (tag, "the persistent kernel ran on tables it must not take")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# one case: every operator, guarded
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, T, d, nx, ny, nz, kind, m):
        import torch
        from tlab_amd.lib import load
        self.T, self.L, self.d, self.shape, self.kind, self.m = T, load(), d, (nx, ny, nz), kind, m
        self.n, self.N = (nx, ny, nz)[d - 1], nx * ny * nz
        self.guard = max(2 * nx * ny, 64)            # two planes, at least one tile of 64 lines x 8 B (even: 16-byte accesses stay aligned)
        self.g = device_plan(T, self.n, kind, m)
        self.f = [field(nx, ny, nz, s) for s in range(7)]
        self.dev = [torch.from_numpy(np.array(a)).cuda() for a in self.f]
        self.snap = [t.clone() for t in self.dev]
        self.ref = references(d, nx, ny, nz, kind, m)
        self.tag = "dir %d %dx%dx%d %s scheme %s" % (d, nx, ny, nz, kind, m)

    def new(self, fill):
        return Guarded(self.N, self.guard, fill)

    def call(self, what, fn, arrays, written):
        """fn() -> return code; then: guards of all `arrays` intact, `written` without NaN, operands untouched.  Returns the kernel names launched."""
        import torch
        from tlab_amd.lib import check
        names = profiled(self.L, lambda: check(fn(), what))
        for k, a in enumerate(arrays):
            assert a.guards_intact(), (self.tag, what, "guard zone of array %d written" % k)
        for k, a in enumerate(written):
            assert not np.isnan(a.host()).any(), (self.tag, what, "output %d left unwritten in places" % k)
        for k, (t, s) in enumerate(zip(self.dev, self.snap)):
            assert torch.equal(t, s), (self.tag, what, "operand %d modified" % k)
        return names

    def close_to(self, what, got, ref):
        err = rel_err(got.host(), ref)
        print("%s %s: rel_err %.3e" % (self.tag, what, err))
        assert err <= TOL, (self.tag, what, err)

    def run(self, path, names_of):
        """Every operator; path: the expected tlab_last_kernel_path; names_of(op): kernel names the launch must include (None: not checked)."""
        L, d, g = self.L, self.d, self.g._h
        nx, ny, nz = self.shape
        from tlab_amd.lib import c_vp
        nan = float("nan")
        p = lambda t: c_vp(t.data_ptr())       # noqa: E731
        u, v, ub = self.dev[0], self.dev[1], self.dev[2]

        def done(op, what, names):
            assert L.tlab_last_kernel_path() == path, (self.tag, what, "kernel path", L.tlab_last_kernel_path(), "expected", path)
            if names_of(op) is not None:
                check_names(names, names_of(op), (self.tag, what))

        for typ, op, key in ((1, "p1", "p1"), (2, "p2", "p2"), (3, "p2_p1", "p2")):
            res, tmp = self.new(nan), self.new(nan)
            names = self.call("OPR_P%s" % op[1:], lambda: L.tlab_opr_partial(d, g, typ, nx, ny, nz, 0, p(u), res.ptr(), tmp.ptr()), [res, tmp],
                              [res, tmp] if typ == 3 else [res])
            done(op, "tlab_opr_partial %d" % typ, names)
            self.close_to("tlab_opr_partial %d" % typ, res, self.ref[key])
            if typ == 3:
                self.close_to("tlab_opr_partial 3 tmp1", tmp, self.ref["p1"])
        for ivel, vel, key in ((self.T.OPR_B_U_IN, v, "b_uin"), (self.T.OPR_B_SELF, u, "b_self")):
            res, tmp = self.new(nan), self.new(nan)
            names = self.call("tlab_opr_burgers " + key, lambda: L.tlab_opr_burgers(d, g, ivel, nx, ny, nz, 0, NU[0], p(u), p(vel), res.ptr(), tmp.ptr(), 0),
                              [res, tmp], [res])
            done("burgers", "tlab_opr_burgers " + key, names)
            self.close_to("tlab_opr_burgers " + key, res, self.ref[key])
        # result += d (u + SCALE ub)
        res, t1, t2 = self.new(self.f[4]), self.new(nan), self.new(nan)
        names = self.call("tlab_opr_partial_add", lambda: L.tlab_opr_partial_add(d, g, nx, ny, nz, 0, p(u), p(ub), SCALE, res.ptr(), 1, t1.ptr(), t2.ptr()),
                          [res, t1, t2], [res])
        done("p_add", "tlab_opr_partial_add", names)
        self.close_to("tlab_opr_partial_add", res, self.ref["p_add"])
        # three fields advected by the second of them: accumulating, then overwriting NaN
        nu = (ctypes.c_double * 3)(*NU)
        sp = (c_vp * 3)(*[self.dev[i].data_ptr() for i in range(3)])
        for overwrite in (0, 1):
            out = [self.new(nan if overwrite else self.f[4 + i]) for i in range(3)]
            t1, t2 = self.new(nan), self.new(nan)
            hp = (c_vp * 3)(*[o.ptr().value for o in out])
            what = "tlab_opr_burgers_add_n overwrite=%d" % overwrite
            names = self.call(what, lambda: L.tlab_opr_burgers_add_n(d, g, nx, ny, nz, 0, 3, nu, sp, p(v), hp, t1.ptr(), t2.ptr(), overwrite), out + [t1, t2], out)
            done("b_n", what, names)
            for i in range(3):
                self.close_to("%s field %d" % (what, i), out[i], self.ref["b_n"][i] if overwrite else self.f[4 + i] + self.ref["b_n"][i])


@pytest.mark.parametrize("nx,ny,nz,kind,m", X_CASES, ids=[_id(c) for c in X_CASES])
def test_x_lines(T, nx, ny, nz, kind, m):
    """k_xline in the form the tables select, or the generic kernel where they select none (2048 points, varying)."""
    c = Case(T, 1, nx, ny, nz, kind, m)
    chunks, invariant, path = x_expectation(nx, kind)
    assert c.L.tlab_fdm_plan_info(c.g._h, 8) == chunks, (c.tag, "chunks", c.L.tlab_fdm_plan_info(c.g._h, 8), "expected", chunks)
    assert c.L.tlab_fdm_plan_info(c.g._h, 9) == invariant, (c.tag, "lane-invariant", c.L.tlab_fdm_plan_info(c.g._h, 9), "expected", invariant)
    xline = {"p1": "k_xline<P1>", "p2": "k_xline<P2>", "p2_p1": "k_xline<P2_P1>", "burgers": "k_xline<BURGERS>", "p_add": "k_xline<P1>", "b_n": "k_xline<BURGERS>"}
    c.run(path, lambda op: {xline[op]} if path == 2 else {"k_generic"})


_SUBSTEPS = {}


@pytest.mark.parametrize("fuse", [True, False])
def test_substep_on_varying_tables(T, fuse):
    """The fused epilogues of the x-line kernel -- the x term of the pressure forcing, the finishing update, the scalar finish -- are reachable only
    through a driver: two Runge-Kutta substeps of Dns on 256 x 16 x 64 whose x and z plans come from `varying` tables (carrying the uniform plans'
    modified wavenumbers for the Poisson solver), y the ordinary stretched plan, against DnsOracle on the same tables, each field within
    bound(scatter) as tests/test_gpu_rhs.py::test_substep_vs_oracle.  The operators are no derivatives any more and the new velocity is not
    solenoidal; both sides evaluate the same formulas."""
    import torch
    from tlab_amd.dns import Dns
    from oracle import tlab_oracle as O
    from oracle.tlab_oracle_rhs import DnsOracle
    from cases import grids, init_fields
    from scatter import substep_scatter, bound
    nx, ny, nz = 256, 16, 64
    x, y, z = PT.nodes(nx), grids(8, ny, 8, True)[1], PT.nodes(nz)
    visc, sc = 1.0 / 800.0, (0.7,)
    q0, s0 = init_fields(nx, ny, nz, x, y, z, 29)
    ogx, ogz = PT.oracle_plan(nx, "varying"), PT.oracle_plan(nz, "varying")
    gp = [PT.device_plan_for_driver(T, ogx), T.FdmPlan(y, False, False, hyper_bc1_ext=0.1), PT.device_plan_for_driver(T, ogz)]
    d = Dns(x, y, z, nscal=1, visc=visc, schmidt=sc, yuniform=False, plans=gp, hyper_bc1_ext=0.1)
    d.set_fusion(fuse)
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(q0[i]))
    d.s[0].copy_(torch.from_numpy(s0[0]))
    sched = [(2e-3 * d.kdt[k], d.kco[k], True) for k in range(2)]
    if "BS" not in _SUBSTEPS:
        _SUBSTEPS["BS"] = substep_scatter(lambda: DnsOracle(x, y, z, nscal=1, visc=visc, schmidt=sc, yuniform=False, plans=[ogx, O.FdmPlan(y, False, False), ogz]),
                                          q0, s0, sched, nsamples=2)
    B, S = _SUBSTEPS["BS"]
    for k, (dte, kco, scale) in enumerate(sched):
        d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dte, kco, scale)
        for name in ("q", "hq", "s", "hs"):
            for i, (b, scat) in enumerate(zip(B[k][name], S[k][name])):
                e = rel_err(getattr(d, name)[i].cpu().numpy(), b)
                print("substep %d fuse %s %s[%d]: err %.2e, oracle scatter %.2e" % (k, fuse, name, i, e, scat))
                assert e <= bound(scat, 2.0, "oracle one-ulp scatter"), (k, name, i, "err %.2e" % e, "oracle scatter %.2e" % scat)


@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("nx,ny,nz,kind,m", Z_CASES, ids=[_id(c) for c in Z_CASES])
def test_z_lines(T, nx, ny, nz, kind, m, policy):
    """k_rtile (policy 1) and k_htile / k_ptile (policy 2) along z."""
    c = Case(T, 3, nx, ny, nz, kind, m)
    c.L.tlab_set_tuning(2, policy)
    try:
        c.run(3, lambda op: z_expectation(op, nz, nx * ny, kind, policy))
    finally:
        c.L.tlab_set_tuning(2, 0)
