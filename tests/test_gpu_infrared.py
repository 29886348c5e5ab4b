"""Cloud-top physics in the device substep: the diagnostic liquid (FI_DIAGNOSTIC / THERMO_AIRWATER_LINEAR, k_airwater_linear), a buoyancy that
reads it, and the gray-liquid infrared heating (TLab_Sources_Scal / Radiation_Infrared_Y, k_infrared_y), against tests/infrared_oracle.py.

What pins the oracle: its first-order integral is the restatement oracle/tlab_oracle_poisson.py::int1_solve, held to the reference's own compiled
FDM_Int1_Solve through tests/golden/infrared_tau.npz (tests/test_infrared_host.py).  THERMO_AIRWATER_LINEAR and the exp / product lines of
IR_RTE1_OnlyLiquid are not reachable through oracle/ref_lib.py: they are pinned by restatement only.

The terms of the full steps (CLOUD below) move the oracle by far more than the bound they are held to: the asserts in
test_rk_step_with_cloud_physics_against_the_oracle print the figures."""
import ctypes

import numpy as np
import pytest
from conftest import rel_err
from scatter import substep_scatter, bound
from cases import grids, init_fields

pytestmark = pytest.mark.gpu

VISC, SC = 1.0 / 800.0, (0.7, 1.0)
# SMALL_NZ: a periodic direction of a plan has 1 or >= 8 points (tlab_fdm_plan_create), so no driver exists for nz = 3 or 5; the small shapes below keep
# nx and ny of (20, 12, 3) and (70, 33, 5) and take nz = 8 and 9, and (20, 12, 1) keeps "fewer columns than one wave", which no 3-D driver can have
DP = ctypes.POINTER(ctypes.c_double)
EINVAL, EUNSUPPORTED = -1, -2
SMOOTH = 0.005625                                   # thermo_param(inb_scal + 1) of examples/Case16-21
# the full steps: AirWaterLinear xi = 1 - 2.5 s1 + 0.8 s2, sharp (max) branch; linear buoyancy on s1, s2 and the liquid; infrared on scalar 2
CLOUD = dict(mixture=(-2.5, 0.8, 0.0), buoyancy=(6, (0.0, -2.0, 0.0), 3, (1.0, -0.4, 0.9, 0.1), 3, None), infrared=(1, 2, 3.0, -4.0, 1.5))


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def _grid(nx, ny, nz, stretch=True):
    x, y, z = grids(nx, ny, nz, stretch)
    if nz == 1:
        z = np.zeros(1)
    return x, y, z


def _case(nx=256, ny=32, nz=16):
    x, y, z = _grid(nx, ny, nz)
    q0, s0 = init_fields(nx, ny, nz, x, y, z, 41)
    s = s0[0]
    return x, y, z, q0, [s, 0.5 * s + 0.3]


def _smooth_liquid(nx, ny, nz, y):
    """a product of smooth functions of x, y, z, clipped at 0 (white noise would make the compact integral itself ill-conditioned on coarse
    stretched grids); flat (nz ny nx)"""
    X = (np.arange(nx) / nx)[None, None, :]
    Y = ((y - y[0]) / (y[-1] - y[0]))[None, :, None]
    Z = (np.arange(nz) / nz)[:, None, None]
    return np.maximum(0.0, (1.0 + 0.5 * np.sin(2 * np.pi * X)) * np.sin(1.3 * np.pi * Y) * (1.0 + 0.3 * np.cos(2 * np.pi * Z)) - 0.2).reshape(-1)


def _load(d, q0, s0):
    import torch
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(q0[i]))
    for i, a in enumerate(s0):
        d.s[i].copy_(torch.from_numpy(a))
    if d.liquid is not None:
        d.FI_DIAGNOSTIC()


def _schedule_rk3(dtime):
    from cases import KDT, KCO
    return [(dtime * KDT[k], KCO[k] if k < 2 else 1.0, k < 2, k == 0) for k in range(3)]


def _fields(d):
    return [t.clone() for t in d.q + d.s + d.hq + d.hs]


def _bod_dev(bod):
    return {"type": bod[0], "vector": bod[1], "scalars": bod[2], "parameters": bod[3], "inb_scal_array": bod[4], "bbackground": bod[5]}


# ---- 1: the liquid ----
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("shape", [(20, 12, 8), (70, 33, 9)])
def test_liquid_against_the_restatement(T, shape, aligned):
    """k_airwater_linear: the max branch bit for bit, the smoothed branch within 1e-13 of the field maximum (device and host exp / log may differ
    in the last place), one and two scalars, 16-byte aligned arrays (vector form) and arrays that start on an odd double (scalar form).
    (SMALL_NZ: the shapes are the smallest 3-D ones a driver can have next to (20, 12, 3) and (70, 33, 5).)"""
    import torch
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load, check, c_vp
    from infrared_oracle import airwater_linear
    nx, ny, nz = shape
    x, y, z = _grid(nx, ny, nz)
    n = nx * ny * nz
    rng = np.random.default_rng(9)
    s0 = [rng.uniform(-1, 1, n) for _ in range(2)]
    off = 0 if aligned else 1
    hold = [torch.zeros(n + off, dtype=torch.float64, device="cuda") for _ in range(3)]
    arrs = [t[off:] for t in hold]
    assert all(t.data_ptr() % 16 == 8 * off for t in arrs)
    worst = 0.0
    for ns in (1, 2):
        d = Dns(x, y, z, nscal=ns, visc=VISC, schmidt=SC[:ns], yuniform=False)
        sa = arrs[:ns] + [arrs[2]]                                              # the scalars, then the liquid
        ptr = (c_vp * len(sa))(*[t.data_ptr() for t in sa])
        for pd in (0.0, SMOOTH):
            par = (1.5, -0.5)[:ns] + (pd,)
            assert pd == 0.0 or (1.0 + 1.5 + 0.5) / pd < 700.0     # |xi / d| < 700: exp stays finite
            d.set_mixture("airwaterlinear", par)
            for t, a in zip(arrs, s0):
                t.copy_(torch.from_numpy(a))
            arrs[2].fill_(-7.0)
            check(load().tlab_dns_diagnostic(d._h, ptr), "tlab_dns_diagnostic")
            torch.cuda.synchronize()
            want = airwater_linear(par, s0[:ns])
            got = arrs[2].cpu().numpy()
            for t, a in zip(arrs[:ns], s0):
                assert np.array_equal(t.cpu().numpy(), a)                       # the scalars are only read
            if pd == 0.0:
                assert (want == 0.0).any() and (want > 0.0).any()
                assert np.array_equal(got, want), (ns, float(np.abs(got - want).max()))
            else:
                e = float(np.abs(got - want).max() / np.abs(want).max())
                worst = max(worst, e)
                assert e <= 1e-13, (ns, e)
    print("smoothed liquid: worst difference %.2e of the field maximum" % worst)
    if not aligned:
        assert all(float(t[0]) == 0.0 for t in hold)


# ---- 2: the source on its own ----
@pytest.mark.parametrize("stretch", [False, True])
@pytest.mark.parametrize("shape", [(20, 12, 1), (20, 12, 8), (70, 33, 9), (256, 32, 16), (64, 24, 1)])
def test_source_against_the_restatement(T, shape, stretch):
    """tlab_dns_sources_scal, downward only and with both fluxes: hs[scalar-1] += source within the per-operator 1e-13 of max |source| (the one-ulp
    scatter of the restatement is <= 1.4e-15); s, the liquid and the other tendency keep their bits.  (20, 12, 1): a short ny that is no multiple
    of the unroll, 20 columns: under one wave; (20, 12, 8): the same lines in three dimensions, a partial last wave; (70, 33, 9): odd sizes, a
    partial last wave; (64, 24, 1): a 2-D run.  (SMALL_NZ: a box of (20, 12, 3) or (70, 33, 5) points cannot be a driver's.)"""
    import torch
    from tlab_amd.dns import Dns
    from infrared_oracle import infrared_gray_liquid
    from oracle import tlab_oracle as O
    nx, ny, nz = shape
    x, y, z = _grid(nx, ny, nz, stretch)
    n = nx * ny * nz
    d = Dns(x, y, z, nscal=2, visc=VISC, schmidt=SC, yuniform=not stretch)
    gy = O.FdmPlan(y, False, not stretch, hyper_bc1_ext=0.0)
    d.set_mixture("airwaterlinear", (-1.2, 0.8, 0.0))
    rng = np.random.default_rng(4)
    s0 = [rng.uniform(-1, 1, n) for _ in range(2)]
    h0 = [rng.uniform(-1, 1, n) for _ in range(2)]
    liq = _smooth_liquid(nx, ny, nz, y)
    assert (liq == 0.0).any() and liq.max() > 1.0
    for scalar, (kappa, ft, fb) in ((2, (3.0, -4.0, 0.0)), (1, (3.0, -4.0, 1.5))):
        for t, a in zip(d.s + d.hs, s0 + h0):
            t.copy_(torch.from_numpy(a))
        d.liquid.copy_(torch.from_numpy(liq))
        d.set_infrared("grayliquid", scalar, kappa, ft, fb)
        d.sources_scal()
        torch.cuda.synchronize()
        src = infrared_gray_liquid(gy, kappa, ft, fb, liq, nx, ny, nz)
        want = h0[scalar - 1] + src
        e = float(np.abs(d.hs[scalar - 1].cpu().numpy() - want).max() / np.abs(src).max())
        print("%s stretch %s flux_bottom %g: err %.2e of max |source| = %.3e" % (shape, stretch, fb, e, np.abs(src).max()))
        assert e <= 1e-13, (shape, stretch, fb, e)
        assert np.array_equal(d.hs[2 - scalar].cpu().numpy(), h0[2 - scalar])          # the other tendency
        assert np.array_equal(d.liquid.cpu().numpy(), liq)
        for t, a in zip(d.s, s0):
            assert np.array_equal(t.cpu().numpy(), a)


# ---- 3: full Runge-Kutta steps ----
ROUTES = ["fused_dirichlet", "freeslip_neumann", "literal"]


def _route(route, source=True, liquid_coefficient=True):
    """(driver, oracle factory, q0, s0): the mixture, linear buoyancy with a coefficient for the liquid, infrared on scalar 2"""
    from tlab_amd.dns import Dns, scalar_bcs, velocity_bcs
    from infrared_oracle import CloudOracle
    x, y, z, q0, s0 = _case(64, 24, 8) if route == "literal" else _case()
    bod = CLOUD["buoyancy"]
    if not liquid_coefficient:
        bod = bod[:3] + (bod[3][:2] + (0.0,) + bod[3][3:],) + bod[4:]

    def make():
        o = CloudOracle(x, y, z, nscal=2, visc=VISC, schmidt=SC, yuniform=False, hyper_bc1_ext=0.0)
        if route == "freeslip_neumann":
            o.flow_jmin, o.flow_jmax = velocity_bcs("freeslip"), velocity_bcs("freeslip")
            o.scal_jmin = [scalar_bcs("neumann")] * 2
        o.set_mixture(CLOUD["mixture"])
        o.set_body_forces(None, bod)
        if source:
            o.set_infrared(*CLOUD["infrared"])
        return o

    def device():
        d = Dns(x, y, z, nscal=2, visc=VISC, schmidt=SC, yuniform=False)
        if route == "freeslip_neumann":
            d.set_bcs("freeslip", "freeslip", "neumann", "dirichlet")
        if route == "literal":
            d.set_fusion(False)
        d.set_mixture("airwaterlinear", CLOUD["mixture"])
        d.set_body_forces(None, _bod_dev(bod))
        if source:
            d.set_infrared(*CLOUD["infrared"])
        return d
    return device, make, q0, s0


@pytest.mark.parametrize("route", ROUTES)
def test_rk_step_with_cloud_physics_against_the_oracle(T, route):
    """One RK3 step against CloudOracle within the project's bound(scatter).  The scatter is the maximum over THREE one-ulp perturbations (tests/scatter.py:
    "a few"): from one sample to the next the oracle's own scatter of hq[0] in the last substep ranges over 2.7e-12 .. 3.5e-12 here (six seeds on the
    CPU; the projection amplifies rounding), and the seed the helper starts from gives the smallest of them.  With that single sample the device's
    5.82e-12 in hq[0] of the last substep on the fused Dirichlet route stood 7 % above 2 x 2.73e-12; every other figure was inside either way."""
    device, make_on, q0, s0 = _route(route)
    sched = _schedule_rk3(2e-3)
    B, S = substep_scatter(make_on, q0, s0, sched, nsamples=3)
    Bsrc, _ = substep_scatter(_route(route, source=False)[1], q0, s0, sched, nsamples=0)
    Bliq, _ = substep_scatter(_route(route, liquid_coefficient=False)[1], q0, s0, sched, nsamples=0)
    # CPU side: the bound must not swallow the terms
    for k in range(len(sched)):
        for name in ("s", "hs"):
            diff = rel_err(Bsrc[k][name][1], B[k][name][1])
            print("%s substep %d %s[1]: the source moves the oracle by %.2e (scatter %.2e)" % (route, k, name, diff, S[k][name][1]))
            assert diff >= 1e-4, (route, k, name, diff)
        diff = rel_err(Bliq[k]["hq"][1], B[k]["hq"][1])
        print("%s substep %d hq[1]: the liquid coefficient moves the oracle by %.2e (scatter %.2e)" % (route, k, diff, S[k]["hq"][1]))
        assert diff >= 1e-4, (route, k, diff)
    d = device()
    _load(d, q0, s0)
    d.begin_step()
    for k, (dte, kco, scale, _) in enumerate(sched):
        d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dte, kco, scale)
        for name in ("q", "s", "hq", "hs"):
            for i, (b, scat) in enumerate(zip(B[k][name], S[k][name])):
                e = rel_err(getattr(d, name)[i].cpu().numpy(), b)
                print("%s substep %d %s[%d]: err %.2e scatter %.2e" % (route, k, name, i, e, scat))
                assert e <= bound(scat), (route, k, name, i, "err %.2e" % e)


# ---- 4: off changes nothing; on, the launches that belong to it and no other ----
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
    torch.cuda.synchronize()
    L.tlab_profile_reset(); L.tlab_profile_enable(1)
    try:
        d.TIME_RUNGEKUTTA(2e-3)
        torch.cuda.synchronize()
    finally:
        L.tlab_profile_enable(0)
    rows = _kernel_rows()
    L.tlab_profile_reset()
    return rows, _fields(d)


@pytest.mark.parametrize("route", ROUTES)
def test_cloud_physics_off_changes_nothing(T, route):
    import torch
    from tlab_amd.dns import Dns
    x, y, z, q0, s0 = _case(64, 24, 8) if route == "literal" else _case()
    bod2 = _bod_dev((6, (0.0, -2.0, 0.0), 2, (1.0, -0.4, 0.1), 2, None))           # no coefficient for the liquid

    def mk():
        m = Dns(x, y, z, nscal=2, visc=VISC, schmidt=SC, yuniform=False)
        if route == "freeslip_neumann":
            m.set_bcs("freeslip", "freeslip", "neumann", "dirichlet")
        if route == "literal":
            m.set_fusion(False)
        m.set_body_forces(None, bod2)
        return m
    never, mixed = mk(), mk()
    rows0, f0 = _profiled_step(never, q0, s0)
    assert "k_airwater_linear" not in rows0 and "k_infrared_y" not in rows0
    mixed.set_mixture("airwaterlinear", CLOUD["mixture"])
    mixed.set_infrared("none")
    mixed.set_body_forces(None, bod2)
    rows1, f1 = _profiled_step(mixed, q0, s0)
    assert rows1 == dict(rows0, k_airwater_linear=3), (rows0, rows1)             # one refresh of the liquid per substep, nothing else
    for a, b in zip(f0, f1):
        assert torch.equal(a, b)                                                 # velocities, prognostic scalars, tendencies: today's bits
    mixed.set_infrared(*CLOUD["infrared"])
    rows2, f2 = _profiled_step(mixed, q0, s0)
    assert rows2 == dict(rows0, k_airwater_linear=3, k_infrared_y=3), (rows0, rows2)
    assert not torch.equal(f0[4], f2[4])                                         # scalar 2 moved
    mixed.set_infrared("none")
    rows3, f3 = _profiled_step(mixed, q0, s0)
    assert rows3 == rows1 and all(torch.equal(a, b) for a, b in zip(f0, f3))


# ---- 5: the RHS entry on its own ----
def test_rhs_alone_applies_no_source_and_keeps_the_liquid(T):
    import torch
    device, _, q0, s0 = _route("fused_dirichlet")
    plain = _route("fused_dirichlet", source=False)[0]()
    b = device()
    outs = []
    for m in (plain, b):
        _load(m, q0, s0)
        m.liquid.fill_(0.25)                                                     # (not what FI_DIAGNOSTIC would give: a refresh would show)
        m.begin_step()
        m.RHS_GLOBAL_INCOMPRESSIBLE_1(2e-3 / 3.0)
        m.RHS_GLOBAL_INCOMPRESSIBLE_1(2e-3 / 3.0)                                # (accumulating onto the first)
        torch.cuda.synchronize()
        assert bool((m.liquid == 0.25).all())
        outs.append(_fields(m))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


# ---- 6: refusals on a live driver ----
def test_refusals_leave_the_driver_as_it_was(T):
    import torch
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    from tlab_amd.operators import FdmPlan
    L = load()
    device, _, q0, s0 = _route("literal")
    d = device()
    x, y, z = _grid(64, 24, 8)

    def step():
        _load(d, q0, s0)
        d.TIME_RUNGEKUTTA(2e-3)
        torch.cuda.synchronize()
        return _fields(d) + [d.liquid.clone()]
    before = step()
    nan, inf = float("nan"), float("inf")
    par = (ctypes.c_double * 3)(-1.2, 0.8, 0.0)
    v = (ctypes.c_double * 3)(0.0, -2.0, 0.0)
    bpar = (ctypes.c_double * 5)(1.0, -0.4, 0.9, 0.3, 0.1)
    refused = [
        (lambda: L.tlab_dns_set_mixture(d._h, 11, par, 3), EUNSUPPORTED),                             # MIXT_TYPE_AIRWATER
        (lambda: L.tlab_dns_set_mixture(d._h, 1, par, 3), EUNSUPPORTED),
        (lambda: L.tlab_dns_set_mixture(d._h, 12, par, 2), EINVAL),                                   # nparam < nscal + 1
        (lambda: L.tlab_dns_set_mixture(d._h, 12, None, 3), EINVAL),
        (lambda: L.tlab_dns_set_mixture(d._h, 12, (ctypes.c_double * 3)(-1.2, nan, 0.0), 3), EINVAL),
        (lambda: L.tlab_dns_set_mixture(d._h, 12, (ctypes.c_double * 3)(-1.2, 0.8, inf), 3), EINVAL),
        (lambda: L.tlab_dns_set_mixture(d._h, 0, None, 0), EINVAL),                                   # the buoyancy set on d reads the liquid
        (lambda: L.tlab_dns_set_infrared(d._h, 2, 2, 3.0, -4.0, 1.5), EUNSUPPORTED),                  # gray
        (lambda: L.tlab_dns_set_infrared(d._h, 3, 2, 3.0, -4.0, 1.5), EUNSUPPORTED),                  # band
        (lambda: L.tlab_dns_set_infrared(d._h, 4, 2, 3.0, -4.0, 1.5), EINVAL),
        (lambda: L.tlab_dns_set_infrared(d._h, 1, 0, 3.0, -4.0, 1.5), EINVAL),                        # scalar outside 1..nscal
        (lambda: L.tlab_dns_set_infrared(d._h, 1, 3, 3.0, -4.0, 1.5), EINVAL),
        (lambda: L.tlab_dns_set_infrared(d._h, 1, 2, nan, -4.0, 1.5), EINVAL),
        (lambda: L.tlab_dns_set_infrared(d._h, 1, 2, 3.0, inf, 1.5), EINVAL),
        (lambda: L.tlab_dns_set_infrared(d._h, 1, 2, 3.0, -4.0, nan), EINVAL),
        (lambda: L.tlab_dns_set_infrared(None, 1, 2, 3.0, -4.0, 1.5), EINVAL),
        (lambda: L.tlab_dns_set_buoyancy(d._h, 6, v, 4, bpar, 5, 4, None), EUNSUPPORTED),             # buoyancy%scalar(1) beyond the liquid
    ]
    for i, (call, code) in enumerate(refused):
        assert call() == code, i
        assert len(L.tlab_last_error()) > 0
        after = step()
        for a, b in zip(before, after):
            assert torch.equal(a, b), i
    # drivers the setters refuse outright
    kw = dict(visc=VISC, yuniform=False)
    d0 = Dns(x, y, z, nscal=0, schmidt=(), **kw)
    assert L.tlab_dns_set_mixture(d0._h, 12, par, 3) == EINVAL                                        # a mixture and no scalar
    assert L.tlab_dns_info(d0._h, 5) == 0
    d2 = Dns(x, y, z, nscal=2, schmidt=SC, **kw)
    assert L.tlab_dns_info(d2._h, 5) == 2
    assert L.tlab_dns_set_infrared(d2._h, 1, 2, 3.0, -4.0, 0.0) == EINVAL                             # no mixture: the reference stops there
    assert L.tlab_dns_set_buoyancy(d2._h, 6, v, 3, bpar, 5, 3, None) == EUNSUPPORTED                  # (as before: no diagnostic array without one)
    d2.set_mixture("airwaterlinear", CLOUD["mixture"])
    assert L.tlab_dns_info(d2._h, 5) == 3
    assert L.tlab_dns_set_infrared(d2._h, 0, 0, 0.0, 0.0, 0.0) == 0                                    # type 0 reads nothing else
    d2.set_anelastic(np.linspace(1.0, 0.8, len(y)))
    try:
        assert L.tlab_dns_set_infrared(d2._h, 1, 2, 3.0, -4.0, 0.0) == EUNSUPPORTED                   # an anelastic driver
    finally:
        d2.set_anelastic(None)
    gy4 = FdmPlan(y, False, False, scheme1=4)                                                         # CompactJacobian4: a tridiagonal integral system
    d4 = Dns(x, y, z, nscal=2, schmidt=SC, plans=(FdmPlan(x, True, True), gy4, FdmPlan(z, True, True)), **kw)
    d4.set_mixture("airwaterlinear", CLOUD["mixture"])
    assert L.tlab_dns_set_infrared(d4._h, 1, 2, 3.0, -4.0, 0.0) == EUNSUPPORTED
    # the substep refuses a mixture together with active scalar bounds (FI_DIAGNOSTIC would see clipped scalars)
    d2.set_scalar_bounds((-0.5, -0.1), (0.6, 0.75))
    _load(d2, q0, s0)
    keep = _fields(d2)
    with pytest.raises(T.TlabError):
        d2.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(1e-3, 1.0, False)
    torch.cuda.synchronize()
    for a, b in zip(keep, _fields(d2)):
        assert torch.equal(a, b)
    d2.set_scalar_bounds(None, None)
    d2.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(1e-3, 1.0, False)
    with pytest.raises(T.TlabError):
        d2.set_mixture("airwater", CLOUD["mixture"])
    with pytest.raises(T.TlabError):
        d2.set_infrared("gray", 2, 3.0, -4.0, 0.0)
