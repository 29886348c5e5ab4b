"""Body forces ([Rotation], [BodyForce]; TLab_Sources_Flow, src/physics/tlab_sources.f90:36-92) in the device substep: the stand-alone routine against
the numpy restatement bit for bit, full Runge-Kutta steps on every route of the driver against tests/sources_oracle.py (the oracle that adds the forces
before its RHS, as time.f90:610-612 does), the kernels launched with forces on and off, the RHS-only entry, the refusals, the deferred tail and the
decomposed drivers.

The forces of the full steps -- normalized Coriolis f2 = 1.5, p = (0.3, 1.0); linear buoyancy c = (1.0, -0.4), c0 = 0.1, bbackground = 0.2 y,
g = (0.3, -2.0, 0.2) -- move every component of q by >= 6e-4 and of hq by >= 1.9e-3 (relative, one RK3 step of 2e-3 at 64 x 24 x 8) while the oracle's
one-ulp scatter stays <= 4.2e-12: the term stands eight orders above the bound it is held to."""
import ctypes

import numpy as np
import pytest
from conftest import rel_err
from scatter import substep_scatter, bound
from cases import grids, init_fields

pytestmark = pytest.mark.gpu

VISC, SC = 1.0 / 800.0, (0.7, 1.0, 1.3)
DP = ctypes.POINTER(ctypes.c_double)
EINVAL, EUNSUPPORTED = -1, -2
COR = (12, (0.0, 1.5, 0.0), (0.3, 1.0))                                    # EQNS_COR_NORMALIZED


def BOD(y, nscal=2):                                                       # EQNS_BOD_LINEAR on two scalars; c0 = parameters[inb_scal_array]
    return (6, (0.3, -2.0, 0.2), 2, (1.0, -0.4, 0.1)[:nscal] + (0.1,), nscal, 0.2 * np.asarray(y))


def _dev(cor, bod):
    """the dicts Dns.set_body_forces takes, from the tuples of the oracle"""
    c = None if cor is None else {"type": cor[0], "vector": cor[1], "parameters": cor[2]}
    b = None if bod is None else {"type": bod[0], "vector": bod[1], "scalars": bod[2], "parameters": bod[3], "inb_scal_array": bod[4], "bbackground": bod[5]}
    return c, b


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def _case(nx=256, ny=32, nz=16, nscal=2):
    x, y, z = grids(nx, ny, nz, True)
    if nz == 1:
        z = np.zeros(1)
    q0, s0 = init_fields(nx, ny, nz, x, y, z, 41)
    s = s0[0]
    return x, y, z, q0, [s, 0.5 * s + 0.3, -0.6 * s * s + 0.1][:nscal]


def _load(d, q0, s0):
    import torch
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(q0[i]))
    for i, a in enumerate(s0):
        d.s[i].copy_(torch.from_numpy(a))


def _schedule(d, dtime):
    n = d.rkm_endstep
    return [(dtime * d.kdt[k], d.kco[k] if k < n - 1 else 1.0, k < n - 1, k == 0) for k in range(n)]


def _fields(d):
    return [t.clone() for t in d.q + d.s + d.hq + d.hs]


# ---- 1, 2: the routine on its own ----
def _standalone_cases():
    g_all = [(0.0, -2.0, 0.0), (0.7, 0.0, 0.0), (0.0, 0.0, -0.3), (0.3, -2.0, 0.2)]
    cases = [("cor_explicit", (4, (0.7, -1.3, 0.4), (0.0, 0.0)), None), ("cor_explicit_f2", (4, (0.0, -1.3, 0.0), (0.0, 0.0)), None),
             ("cor_normalized", (12, (0.0, 1.5, 0.0), (0.3, 1.0)), None)]
    par = (1.1, -0.4, 0.3, 0.17)
    for ig, g in enumerate(g_all):
        cases.append(("homogeneous_g%d" % ig, None, (5, g, 0, (0.8,), 3, None)))
        for ns in (1, 2, 3):
            cases.append(("linear%d_g%d" % (ns, ig), None, (6, g, ns, par, 3, "ref")))
        cases.append(("bilinear_g%d" % ig, None, (7, g, 2, par[:3], 3, "ref")))
        cases.append(("quadratic_g%d" % ig, None, (8, g, 1, (0.9, 1.6), 3, "ref")))
    cases.append(("linear_general0", None, (6, g_all[3], 0, par, 3, "ref")))                                   # gravity.f90:279-291 with no scalar
    cases.append(("linear_no_profile", None, (6, g_all[3], 2, par, 3, None)))                                  # bbackground NULL: zeros
    cases.append(("both", (4, (0.7, -1.3, 0.4), (0.0, 0.0)), (6, g_all[3], 3, par, 3, "ref")))
    cases.append(("both_normalized", (12, (0.0, 1.5, 0.0), (0.3, 1.0)), (7, g_all[0], 2, par[:3], 3, "ref")))
    return cases


def _standalone(T, nx, ny, nz, aligned=True):
    import torch
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load, check, c_vp
    from sources_oracle import sources_flow
    x, y, z, q0, s0 = _case(nx, ny, nz, 3)
    n = nx * ny * nz
    d = Dns(x, y, z, nscal=3, visc=VISC, schmidt=SC, yuniform=False)
    rng = np.random.default_rng(3)
    h0 = [rng.uniform(-1, 1, n) for _ in range(3)]
    ref = 0.2 * y + 0.05
    off = 0 if aligned else 1
    hold = [torch.zeros(n + off, dtype=torch.float64, device="cuda") for _ in range(9)]
    arrs = [t[off:] for t in hold]
    assert all(t.data_ptr() % 16 == 8 * off for t in arrs)
    arr = lambda ts: (c_vp * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
    worst = 0.0
    for name, cor, bod in _standalone_cases():
        if bod is not None and isinstance(bod[5], str):
            bod = bod[:5] + (ref,)
        for t, a in zip(arrs, q0 + s0 + h0):
            t.copy_(torch.from_numpy(a))
        d.set_body_forces(*_dev(cor, bod))
        check(load().tlab_dns_sources_flow(d._h, arr(arrs[0:3]), arr(arrs[3:6]), arr(arrs[6:9])), "tlab_dns_sources_flow")
        torch.cuda.synchronize()
        want = [a.copy() for a in h0]
        sources_flow(cor, bod, q0, s0, want, nx, ny, nz)
        got = [t.cpu().numpy() for t in arrs]
        for a, b in zip(got[:6], q0 + s0):
            assert np.array_equal(a, b), name                                         # q and s are only read
        touched = [False] * 3
        if cor is not None:
            f = cor[1]
            touched = [bool(f[2] or f[1]), bool(f[0] or f[2]), bool(f[1] or f[0])] if cor[0] == 4 else [True, False, True]
        if bod is not None:
            touched = [t or g != 0.0 for t, g in zip(touched, bod[1])]
        for i in range(3):
            if not touched[i]:
                assert np.array_equal(got[6 + i], h0[i]), (name, i)                   # a component no force touches keeps its bits
                continue
            assert not np.array_equal(want[i], h0[i]), (name, i)
            if cor is not None and cor[0] == 12 and i != 1:                          # cos / sin pass through the host's libm
                e = float(np.abs(got[6 + i] - want[i]).max() / np.abs(want[i]).max())
                worst = max(worst, e)
                assert e <= 1e-15, (name, i, e)
            else:
                assert np.array_equal(got[6 + i], want[i]), (name, i, float(np.abs(got[6 + i] - want[i]).max()))
    print("normalized Coriolis: worst rel. difference %.2e" % worst)
    if not aligned:
        assert all(float(t[0]) == 0.0 for t in hold)


@pytest.mark.parametrize("shape", [(64, 16, 8), (16, 12, 1)])
def test_standalone_routine_against_numpy(T, shape):
    _standalone(T, *shape)


def test_unaligned_arrays_take_the_scalar_form(T):
    """The 16-byte form needs 16-byte aligned arrays; arrays that start on an odd double -- columns of a host's two-dimensional block may -- take the
    scalar instance of the kernel."""
    _standalone(T, 64, 16, 8, aligned=False)


# ---- 3: full Runge-Kutta steps ----
ROUTES = ["fused_dirichlet", "freeslip_neumann", "literal", "zones_and_bounds"]
PJMIN, PJMAX, PU, PS = 4, 6, (150.0, 2.0), (120.0, 2.0)
LO, HI = (-0.55, -0.1), (0.6, 0.75)


def _route(T, route):
    """(driver, oracle factory with forces, oracle factory without, q0, s0)"""
    from tlab_amd.dns import Dns, scalar_bcs, velocity_bcs
    from sources_oracle import SourcesOracle
    x, y, z, q0, s0 = _case(64, 24, 8) if route == "literal" else _case()
    if route == "zones_and_bounds":      # (fields as a run under bounds holds them: inside the bounds)
        s0 = [np.minimum(np.maximum(a, lo), hi) for a, lo, hi in zip(s0, LO, HI)]
    d = Dns(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False)
    setup = []
    cls = SourcesOracle
    if route == "freeslip_neumann":
        d.set_bcs("freeslip", "freeslip", "neumann", "dirichlet")
        setup.append(lambda o: (setattr(o, "flow_jmin", velocity_bcs("freeslip")), setattr(o, "flow_jmax", velocity_bcs("freeslip")),
                                setattr(o, "scal_jmin", [scalar_bcs("neumann")] * 2)))
    elif route == "literal":
        d.set_fusion(False)
    elif route == "zones_and_bounds":
        _load(d, q0, s0)
        d.set_buffer_zones(PJMIN, PJMAX, PU, PS)
        d.set_scalar_bounds(LO, HI)

        class Bounded(SourcesOracle):
            """... + DNS_BOUNDS_LIMIT after the update (dns_local.f90:67-90)"""

            def time_substep(self, dte, kco=1.0, scale=False):
                self.sources_flow()
                self.rhs_global_incompressible_1(dte)
                self.buffer_relax_scal()
                for i in range(3):
                    self.q[i] = self.q[i] + dte * self.hq[i]
                for i in range(self.nscal):
                    self.s[i] = np.minimum(np.maximum(self.s[i] + dte * self.hs[i], LO[i]), HI[i])
                if scale:
                    self.hq = [kco * h for h in self.hq]
                    self.hs = [kco * h for h in self.hs]
        cls = Bounded

        def zones(o):
            o.q, o.s = [a.copy() for a in q0], [a.copy() for a in s0]      # the zones' reference comes from the unperturbed fields, like the device's
            o.set_buffer_zones(PJMIN, PJMAX, PU, PS)
        setup.append(zones)

    def factory(forces):
        def make():
            o = cls(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False, hyper_bc1_ext=0.0)
            for f in setup:
                f(o)
            if forces:
                o.set_body_forces(COR, BOD(y))
            return o
        return make
    return d, factory(True), factory(False), q0, s0


@pytest.mark.parametrize("route", ROUTES)
def test_rk_step_with_forces_against_the_oracle(T, route):
    d, make_on, make_off, q0, s0 = _route(T, route)
    _load(d, q0, s0)
    d.set_body_forces(*_dev(COR, BOD(d.y)))
    sched = _schedule(d, 2e-3)
    B, S = substep_scatter(make_on, q0, s0, sched, nsamples=1)
    Boff, _ = substep_scatter(make_off, q0, s0, sched, nsamples=0)
    # CPU side: the term must not be lost in the bound -- with and without forces the oracle differs by >= 1e-4 in every velocity component
    for k in range(len(sched)):
        for name in ("q", "hq"):
            for i in range(3):
                diff = rel_err(Boff[k][name][i], B[k][name][i])
                print("%s substep %d %s[%d]: forces move the oracle by %.2e (scatter %.2e)" % (route, k, name, i, diff, S[k][name][i]))
                assert diff >= 1e-4, (route, k, name, i, diff)
    d.begin_step()
    for k, (dte, kco, scale, _) in enumerate(sched):
        d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dte, kco, scale)
        for name in ("q", "s", "hq", "hs"):
            for i, (b, scat) in enumerate(zip(B[k][name], S[k][name])):
                e = rel_err(getattr(d, name)[i].cpu().numpy(), b)
                print("%s substep %d %s[%d]: err %.2e scatter %.2e" % (route, k, name, i, e, scat))
                assert e <= bound(scat), (route, k, name, i, "err %.2e" % e)


# ---- 4: forces off change nothing; on, one launch per substep ----
def _kernel_rows():
    from tlab_amd.lib import load
    buf = ctypes.create_string_buffer(32768)
    load().tlab_profile_report(buf, len(buf))
    return {r.split("\t")[0]: int(r.split("\t")[1]) for r in buf.value.decode().splitlines() if "\t" in r}


def _profiled_step(d, q0, s0):
    import torch
    from tlab_amd.lib import load
    L = load()
    _load(d, q0, s0)
    L.tlab_profile_reset(); L.tlab_profile_enable(1)
    try:
        d.TIME_RUNGEKUTTA(2e-3)
        torch.cuda.synchronize()
    finally:
        L.tlab_profile_enable(0)
    rows = _kernel_rows()
    L.tlab_profile_reset()
    return rows, _fields(d)


@pytest.mark.parametrize("route", ["fused_dirichlet", "freeslip_neumann", "literal"])
def test_forces_off_change_nothing(T, route):
    import torch
    from tlab_amd.dns import Dns
    x, y, z, q0, s0 = _case(64, 24, 8) if route == "literal" else _case()
    mk = lambda: Dns(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False)      # noqa: E731
    never, off, zero = mk(), mk(), mk()
    for m in (never, off, zero):
        if route == "freeslip_neumann":
            m.set_bcs("freeslip", "freeslip", "neumann", "dirichlet")
        if route == "literal":
            m.set_fusion(False)
    rows0, f0 = _profiled_step(never, q0, s0)
    assert "k_body_force" not in rows0
    off.set_body_forces(*_dev(COR, BOD(y)))
    rows_on, f_on = _profiled_step(off, q0, s0)
    # with forces: the kernels of the run without, as often, plus exactly one k_body_force per substep
    assert rows_on == dict(rows0, k_body_force=3), (rows0, rows_on)
    assert not any(torch.equal(a, b) for a, b in zip(f0[:3], f_on[:3]))
    off.set_body_forces(None, None)                                                    # type 0
    cz, bz = _dev((12, (0.0, 0.0, 0.0), (0.3, 1.0)), BOD(y)[:1] + ((0.0, 0.0, 0.0),) + BOD(y)[2:])
    zero.set_body_forces(cz, bz)                                                       # both set, every vector zero
    for m in (off, zero):
        rows1, f1 = _profiled_step(m, q0, s0)
        assert rows1 == rows0, (rows0, rows1)
        for a, b in zip(f0, f1):
            assert torch.equal(a, b)
    zero.set_body_forces({"type": "explicit", "vector": (0.0, 0.0, 0.0)}, None)
    rows1, f1 = _profiled_step(zero, q0, s0)
    assert rows1 == rows0 and all(torch.equal(a, b) for a, b in zip(f0, f1))


# ---- 5: the RHS entry on its own ----
def test_rhs_alone_applies_no_force(T):
    import torch
    from tlab_amd.dns import Dns
    x, y, z, q0, s0 = _case()
    mk = lambda: Dns(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False)      # noqa: E731
    a, b = mk(), mk()
    b.set_body_forces(*_dev(COR, BOD(y)))
    for m in (a, b):
        _load(m, q0, s0)
        m.begin_step()
        m.RHS_GLOBAL_INCOMPRESSIBLE_1(2e-3 / 3.0)
        m.RHS_GLOBAL_INCOMPRESSIBLE_1(2e-3 / 3.0)                                      # (accumulating onto the first)
    torch.cuda.synchronize()
    for u, v in zip(_fields(a), _fields(b)):
        assert torch.equal(u, v)


# ---- 6: refusals on a live driver ----
def test_refusals_leave_the_driver_as_it_was(T):
    import torch
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    x, y, z, q0, s0 = _case(64, 16, 8)
    ny = len(y)
    d = Dns(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False)
    d0 = Dns(x, y, z, nscal=0, visc=VISC, schmidt=(), yuniform=False)
    L = load()
    d.set_body_forces(*_dev(COR, BOD(y)))

    def step():
        _load(d, q0, s0)
        d.TIME_RUNGEKUTTA(2e-3)
        torch.cuda.synchronize()
        return _fields(d)
    before = step()
    v = (ctypes.c_double * 3)(0.3, -2.0, 0.2)
    vy = (ctypes.c_double * 3)(0.0, 1.5, 0.0)
    p2 = (ctypes.c_double * 2)(0.3, 1.0)
    par = (ctypes.c_double * 4)(1.0, -0.4, 0.1, 0.2)
    nan = float("nan")
    bb = (ctypes.c_double * ny)(*([0.1] * ny))
    bbnan = (ctypes.c_double * ny)(*([0.1] * (ny - 1) + [nan]))
    refused = [
        (lambda: L.tlab_dns_set_buoyancy(d._h, 4, v, 2, par, 4, 2, bb), EUNSUPPORTED),                # EQNS_BOD_EXPLICIT
        (lambda: L.tlab_dns_set_buoyancy(d._h, 9, v, 2, par, 4, 2, bb), EUNSUPPORTED),                # NORMALIZEDMEAN
        (lambda: L.tlab_dns_set_buoyancy(d._h, 10, v, 2, par, 4, 2, bb), EUNSUPPORTED),               # SUBTRACTMEAN
        (lambda: L.tlab_dns_set_buoyancy(d._h, 6, v, 3, par, 4, 3, bb), EUNSUPPORTED),                # buoyancy%scalar(1) > nscal
        (lambda: L.tlab_dns_set_buoyancy(d._h, 3, v, 2, par, 4, 2, bb), EINVAL),                      # unknown types
        (lambda: L.tlab_dns_set_buoyancy(d._h, 11, v, 2, par, 4, 2, bb), EINVAL),
        (lambda: L.tlab_dns_set_coriolis(d._h, 5, vy, p2), EINVAL),
        (lambda: L.tlab_dns_set_coriolis(d._h, 12, (ctypes.c_double * 3)(0.1, 1.5, 0.0), p2), EINVAL),    # an active y equation
        (lambda: L.tlab_dns_set_coriolis(d._h, 12, (ctypes.c_double * 3)(0.0, 1.5, 0.2), p2), EINVAL),
        (lambda: L.tlab_dns_set_coriolis(d._h, 4, (ctypes.c_double * 3)(0.0, nan, 0.0), p2), EINVAL),
        (lambda: L.tlab_dns_set_coriolis(d._h, 12, vy, (ctypes.c_double * 2)(float("inf"), 1.0)), EINVAL),
        (lambda: L.tlab_dns_set_buoyancy(d._h, 6, (ctypes.c_double * 3)(nan, 0.0, 0.0), 2, par, 4, 2, bb), EINVAL),
        (lambda: L.tlab_dns_set_buoyancy(d._h, 6, v, 2, (ctypes.c_double * 4)(1.0, nan, 0.0, 0.0), 4, 2, bb), EINVAL),
        (lambda: L.tlab_dns_set_buoyancy(d._h, 6, v, 2, par, 4, 2, bbnan), EINVAL),
        (lambda: L.tlab_dns_set_buoyancy(d._h, 8, v, 1, (ctypes.c_double * 2)(1.0, 0.0), 2, 2, bb), EINVAL),   # c0 = -p1 / (p2/2)^2 is infinite
        (lambda: L.tlab_dns_set_buoyancy(None, 6, v, 2, par, 4, 2, bb), EINVAL),                      # a profile and no driver
    ]
    for i, (call, code) in enumerate(refused):
        assert call() == code, i
        assert len(L.tlab_last_error()) > 0
        after = step()
        for a, b in zip(before, after):
            assert torch.equal(a, b), i
    # a type that needs scalars on a driver without them
    for t in (6, 7, 8):
        assert L.tlab_dns_set_buoyancy(d0._h, t, v, 1, par, 4, 1, None) == EINVAL, t
    assert L.tlab_dns_set_buoyancy(d0._h, 5, v, 0, par, 1, 0, None) == 0                              # homogeneous reads none
    d1 = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC[:1], yuniform=False)
    assert L.tlab_dns_set_buoyancy(d1._h, 7, v, 2, par, 4, 1, None) == EINVAL                         # bilinear reads two
    with pytest.raises(T.TlabError):
        d.set_body_forces(None, {"type": "subtractmean", "vector": (0.0, -1.0, 0.0)})
    with pytest.raises(T.TlabError):
        d.set_body_forces({"type": "sideways"}, None)


# ---- 7: the deferred tail: time.f90's calls of an unchanged host, TLab_Sources_Flow before the RHS ----
def _deferred_step(d, order, dtime=2e-3, other=None, substeps=3, daxpy=True):
    """One RK3 step through the deferred entry points.  order: "time.f90" (zero fills, then per substep sources, RHS, DAXPYs, DSCALs), "none" (no
    sources call), "after" (sources after the RHS), "other" (sources on other tendency arrays), "twice".  Returns the differences of (deferred stats,
    sources stats)."""
    import torch
    from tlab_amd.lib import load, check, c_vp
    L = load()
    mk = lambda ts: (c_vp * max(1, len(ts)))(*[t.data_ptr() for t in ts])      # noqa: E731
    q, s, hq, hs, txc = mk(d.q), mk(d.s), mk(d.hq), mk(d.hs), mk(d.txc)
    ohq = mk(other) if other is not None else None
    st0, ss0 = (ctypes.c_longlong * 6)(), (ctypes.c_longlong * 2)()
    check(L.tlab_deferred_stats(st0), "stats"); check(L.tlab_deferred_sources_stats(ss0), "sources stats")
    N = d.n
    check(L.tlab_deferred_enable(1), "enable")
    try:
        for t in d.hq + d.hs:
            check(L.tlab_deferred_zero(t.data_ptr(), N), "zero")
        for k in range(substeps):
            dte = dtime * d.kdt[k]
            if order in ("time.f90", "twice"):
                check(L.tlab_deferred_sources_flow(d._h, q, s, hq), "sources")
            if order == "twice":
                check(L.tlab_deferred_sources_flow(d._h, q, s, hq), "sources")
            if order == "other":
                check(L.tlab_deferred_sources_flow(d._h, q, s, ohq), "sources")
            check(L.tlab_deferred_rhs(d._h, dte, q, s, hq, hs, txc), "rhs")
            if order == "after":
                check(L.tlab_deferred_sources_flow(d._h, q, s, hq), "sources")
            if not daxpy:
                continue
            for h, u in zip(d.hq + d.hs, d.q + d.s):
                check(L.tlab_deferred_axpy(N, dte, h.data_ptr(), u.data_ptr()), "axpy")
            if k < 2:
                for h in d.hq + d.hs:
                    check(L.tlab_deferred_scal(N, d.kco[k], h.data_ptr()), "scal")
        check(L.tlab_deferred_flush(), "flush")
    finally:
        check(L.tlab_deferred_enable(0), "disable")
    torch.cuda.synchronize()
    st1, ss1 = (ctypes.c_longlong * 6)(), (ctypes.c_longlong * 2)()
    check(L.tlab_deferred_stats(st1), "stats"); check(L.tlab_deferred_sources_stats(ss1), "sources stats")
    return [b - a for a, b in zip(st0, st1)], [b - a for a, b in zip(ss0, ss1)]


def _forced_driver(forces=True, shape=(256, 32, 16)):
    from tlab_amd.dns import Dns
    x, y, z, q0, s0 = _case(*shape)
    d = Dns(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False)
    _load(d, q0, s0)
    if forces:
        d.set_body_forces(*_dev(COR, BOD(y)))
    return d, (x, y, z, q0, s0)


def test_deferred_tail_with_the_marker_is_the_fused_substep(T):
    import torch
    a, _ = _forced_driver()
    b, _ = _forced_driver()
    a.TIME_RUNGEKUTTA(2e-3)
    st, ss = _deferred_step(b, "time.f90")
    assert st[0] == 3 and st[1] == 0 and st[2] == 1 and ss == [3, 0], (st, ss)       # three fused substeps, each carrying the marker; nothing literal
    for u, v in zip(_fields(a), _fields(b)):
        assert torch.equal(u, v)


def test_deferred_record_without_the_marker_adds_no_force(T):
    import torch
    a, _ = _forced_driver(forces=False)
    b, _ = _forced_driver()
    a.TIME_RUNGEKUTTA(2e-3)
    st, ss = _deferred_step(b, "none")
    assert st[0] == 3 and st[1] == 0 and ss == [0, 0], (st, ss)
    for u, v in zip(_fields(a), _fields(b)):
        assert torch.equal(u, v)
    a.TIME_RUNGEKUTTA(2e-3)
    b.TIME_RUNGEKUTTA(2e-3)                                                           # the driver's own substep applies the forces again afterwards
    assert not torch.equal(a.q[0], b.q[0])


@pytest.mark.parametrize("order", ["after", "other", "twice"])
def test_deferred_tail_out_of_order_runs_the_marker_literally(T, order):
    """The marker after the RHS, on other arrays, or twice: it runs literally, in call order, and the fields are those of an oracle that makes the
    same calls in the same order."""
    import torch
    from buffer_oracle import BufferOracle
    from sources_oracle import SourcesOracle
    d, (x, y, z, q0, s0) = _forced_driver(shape=(64, 24, 8))
    rng = np.random.default_rng(8)
    o0 = [rng.uniform(-1, 1, d.n) for _ in range(3)]
    other = [torch.from_numpy(a).cuda() for a in o0] if order == "other" else None
    st, ss = _deferred_step(d, order, other=other)
    if order == "twice":
        assert st[0] == 3 and ss == [3, 3], (st, ss)            # the first call of each pair on its own, the second in the fused substep
    else:
        assert ss == [0, 3] and st[0] == (3 if order == "other" else 0), (st, ss)

    class Ordered(SourcesOracle):
        def time_substep(self, dte, kco=1.0, scale=False):
            if order == "twice":                                # sources, then the substep with its own sources call
                self.sources_flow()
                return SourcesOracle.time_substep(self, dte, kco, scale)
            if order == "other":                                # the forces never reach hq
                return BufferOracle.time_substep(self, dte, kco, scale)
            self.rhs_global_incompressible_1(dte)               # "after": RHS, sources (outside the projection), update, scaling
            self.sources_flow()
            for i in range(3):
                self.q[i] = self.q[i] + dte * self.hq[i]
            for i in range(self.nscal):
                self.s[i] = self.s[i] + dte * self.hs[i]
            if scale:
                self.hq = [kco * h for h in self.hq]
                self.hs = [kco * h for h in self.hs]

    def make():
        o = Ordered(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False, hyper_bc1_ext=0.0)
        o.set_body_forces(COR, BOD(y))
        return o
    sched = _schedule(d, 2e-3)
    B, S = substep_scatter(make, q0, s0, sched, nsamples=1)
    for name in ("q", "s", "hq", "hs"):
        for i, (b, scat) in enumerate(zip(B[2][name], S[2][name])):
            e = rel_err(getattr(d, name)[i].cpu().numpy(), b)
            assert e <= bound(scat), (order, name, i, "err %.2e" % e)
    if order == "other":      # the other arrays took the three calls instead
        assert not any(np.array_equal(t.cpu().numpy(), a) for t, a in zip(other, o0))


def test_literal_first_substep_after_recorded_zero_fills_starts_from_zero(T):
    """Zero fills, marker, RHS and then a flush: the record runs literally.  The routine on its own ADDS to hq, so the recorded zero fills must be
    executed, not taken as tlab_dns_begin_step: whatever hq held before must not reach the result."""
    import torch
    from sources_oracle import SourcesOracle
    d, (x, y, z, q0, s0) = _forced_driver(shape=(64, 24, 8))
    outs = []
    for fill in (7.0, -3.0e5):
        _load(d, q0, s0)
        for t in d.hq + d.hs:
            t.fill_(fill)
        st, ss = _deferred_step(d, "time.f90", substeps=1, daxpy=False)
        assert st[0] == 0 and st[1] == 1 and st[2] == 0 and ss == [0, 1], (st, ss)
        outs.append([t.clone() for t in d.hq + d.hs])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    o = SourcesOracle(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False, hyper_bc1_ext=0.0)
    o.q, o.s = [a.copy() for a in q0], [a.copy() for a in s0]
    o.set_body_forces(COR, BOD(y))
    o.sources_flow()
    o.rhs_global_incompressible_1(2e-3 * d.kdt[0])
    sched = [(2e-3 * d.kdt[0], 1.0, False, True)]

    def make():
        m = SourcesOracle(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False, hyper_bc1_ext=0.0)
        m.set_body_forces(COR, BOD(y))
        return m
    _, S = substep_scatter(make, q0, s0, sched, nsamples=1)
    for i in range(3):
        assert rel_err(outs[0][i].cpu().numpy(), o.hq[i]) <= bound(S[0]["hq"][i]), i


# ---- 8: the decomposed drivers on loopback ranks of one GPU ----
@pytest.fixture(scope="module")
def single_domain(T):
    """The single-domain RK3 step with forces at the shape of the slab and pencil cases, and the one-ulp scatter of its oracle: made once"""
    from tlab_amd.dns import Dns
    from sources_oracle import SourcesOracle
    nx, ny, nz = 128, 24, 256
    x, y, z, q0, s0 = _case(nx, ny, nz)
    kw = dict(nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False)
    d = Dns(x, y, z, **kw)
    _load(d, q0, s0)
    d.set_body_forces(*_dev(COR, BOD(y)))
    d.TIME_RUNGEKUTTA(2e-3)
    one = {"q": [t.clone() for t in d.q], "s": [t.clone() for t in d.s]}
    sched = _schedule(d, 2e-3)

    def make():
        o = SourcesOracle(x, y, z, hyper_bc1_ext=0.0, **kw)
        o.set_body_forces(COR, BOD(y))
        return o
    B, S = substep_scatter(make, q0, s0, sched, nsamples=1)
    for name in ("q", "s"):
        for i, rf in enumerate(one[name]):
            assert rel_err(rf.cpu().numpy(), B[2][name][i]) <= bound(S[2][name][i]), (name, i)
    del d
    return (x, y, z, q0, s0, kw), one, S[2]


def _decomposed_errors(m, one, gather):
    import torch
    for k in range(m.rkm_endstep):
        m.substep_of_cycle(k, 2e-3)
    torch.cuda.synchronize()
    errs = {}
    for name in ("q", "s"):
        for i, rf in enumerate(one[name]):
            errs[(name, i)] = float((gather(name, i) - rf).abs().max() / rf.abs().max())
    return errs


def test_slab_driver_with_forces_equals_the_single_domain(T, single_domain):
    import torch
    from tlab_amd.slab import NativeSlabDns
    (x, y, z, q0, s0, kw), one, S = single_domain
    m = NativeSlabDns("loopback", x, y, z, size=4, **kw)
    for i in range(3):
        m.scatter("q", i, torch.from_numpy(q0[i]).cuda())
    for i in range(2):
        m.scatter("s", i, torch.from_numpy(s0[i]).cuda())
    m.set_body_forces(*_dev(COR, BOD(y)))
    errs = _decomposed_errors(m, one, lambda name, i: torch.cat([m.st[r][name][i] for r in m.local_ranks]))
    m.close()
    for (name, i), e in errs.items():
        assert e <= bound(S[name][i]), (name, i, e)


def test_pencil_driver_with_forces_equals_the_single_domain(T, single_domain):
    import torch
    from tlab_amd.pencil import NativePencilDns
    (x, y, z, q0, s0, kw), one, S = single_domain
    nx, ny, nz = len(x), len(y), len(z)
    m = NativePencilDns("loopback", 2, 2, x, y, z, **kw)
    for i in range(3):
        m.scatter("q", i, torch.from_numpy(q0[i]).cuda())
    for i in range(2):
        m.scatter("s", i, torch.from_numpy(s0[i]).cuda())
    m.set_body_forces(*_dev(COR, BOD(y)))

    def gather(name, i):
        out = torch.empty(nz, ny, nx, dtype=torch.float64, device="cuda")
        for r, t in m.gather_local(name, i).items():
            pi, pk = m.pro(r)
            out[pk * m.kmax:(pk + 1) * m.kmax, :, pi * m.imax:(pi + 1) * m.imax] = t.view(m.kmax, ny, m.imax)
        return out.reshape(-1)
    errs = _decomposed_errors(m, one, gather)
    m.close()
    for (name, i), e in errs.items():
        assert e <= bound(S[name][i]), (name, i, e)
