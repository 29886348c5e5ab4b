"""Relaxation buffer zones ([BufferZone] Type = relaxation, tools/dns/boundary_buffer.f90) in the single-domain device substep: the stand-alone
operators against numpy, full Runge-Kutta steps on every route of the driver against tests/buffer_oracle.py (the oracle with the two relaxation calls
in the reference's places), the kernels launched with zones on and off, the RHS-only entry, and the refusals."""
import ctypes

import numpy as np
import pytest
from conftest import rel_err, golden_files
from scatter import substep_scatter, bound
from cases import grids, init_fields

pytestmark = pytest.mark.gpu

VISC, SC = 1.0 / 800.0, (0.7, 1.0, 1.3)
PJMIN, PJMAX = 5, 8
PU, PS = (150.0, 2.0), (120.0, 0.0, 200.0, 1.5)          # strengths large enough to stand far above the parity bound; scalar 2 is inactive
DP = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def _case(nx=256, ny=32, nz=16):
    x, y, z = grids(nx, ny, nz, True)
    q0, s0 = init_fields(nx, ny, nz, x, y, z, 41)
    s = s0[0]
    return x, y, z, q0, [s, 0.5 * s + 0.3, -0.6 * s]


def _load(d, q0, s0):
    import torch
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(q0[i]))
    for i, a in enumerate(s0):
        d.s[i].copy_(torch.from_numpy(a))


def _schedule(d, dtime):
    n = d.rkm_endstep
    return [(dtime * d.kdt[k], d.kco[k] if k < n - 1 else 1.0, k < n - 1, k == 0) for k in range(n)]


def _zone_planes(ny):
    return np.r_[0:PJMIN, ny - PJMAX:ny]


def _oracle_factory(x, y, z, q0, s0, zones, setup=(), **kw):
    """() -> BufferOracle whose zones (tau, ref) come from the UNPERTURBED fields q0, s0, like the device's"""
    from buffer_oracle import BufferOracle

    def make():
        o = BufferOracle(x, y, z, nscal=len(s0), visc=VISC, schmidt=SC[:len(s0)], yuniform=False, **({"hyper_bc1_ext": 0.0} if "plans" not in kw else {}), **kw)
        for f in setup:
            f(o)
        if zones:
            o.q = [a.copy() for a in q0]
            o.s = [a.copy() for a in s0]
            o.set_buffer_zones(PJMIN, PJMAX, PU, PS if len(s0) == 3 else (PS[0], PS[3]))
        return o
    return make


def test_standalone_operators_against_numpy(T):
    import torch
    from tlab_amd.dns import Dns
    from buffer_oracle import relax_block
    nx, ny, nz = 256, 32, 16
    x, y, z, q0, s0 = _case(nx, ny, nz)
    d = Dns(x, y, z, nscal=3, visc=VISC, schmidt=SC, yuniform=False)
    _load(d, q0, s0)
    d.set_buffer_zones(PJMIN, PJMAX, PU, PS)
    o = _oracle_factory(x, y, z, q0, s0, True)()
    rng = np.random.default_rng(3)
    h0 = [rng.uniform(-1, 1, nx * ny * nz) for _ in range(6)]
    for t, a in zip(d.hq + d.hs, h0):
        t.copy_(torch.from_numpy(a))
    d.buffer_relax_flow()
    d.buffer_relax_scal()
    torch.cuda.synchronize()
    want = [a.copy() for a in h0]
    for blk in o.buff_flow:
        relax_block(blk, q0, want[:3], nx, ny, nz)
    for blk in o.buff_scal:
        relax_block(blk, s0, want[3:], nx, ny, nz)
    zone = _zone_planes(ny)
    outside = np.setdiff1d(np.arange(ny), zone)
    for i, (t, w, a) in enumerate(zip(d.hq + d.hs, want, h0)):
        got = t.cpu().numpy().reshape(nz, ny, nx)
        w3, a3 = w.reshape(nz, ny, nx), a.reshape(nz, ny, nx)
        assert np.array_equal(got[:, outside, :], a3[:, outside, :]), i                      # nothing outside the zones is written
        e = np.abs(got[:, zone, :] - w3[:, zone, :]).max() / np.abs(w3[:, zone, :]).max()
        print("field %d: zone rel-err %.2e" % (i, e))
        assert e <= 1e-13, (i, e)
        if i != 4:
            assert np.abs(w3[:, zone, :] - a3[:, zone, :]).max() > 1.0                       # the term is there ...
    assert np.array_equal(d.hs[1].cpu().numpy(), h0[4])                                      # ... and strength 0 changes nothing at all
    for t, a in zip(d.q + d.s, q0 + s0):
        assert np.array_equal(t.cpu().numpy(), a)


def test_unaligned_arrays_take_the_scalar_form(T):
    """The 16-byte form needs 16-byte aligned arrays (nx is even in every driver: the FFT demands it); arrays that start on an odd double
    -- columns of a host's two-dimensional block may -- take the scalar instance of the kernel."""
    import torch
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load, check, c_vp
    from buffer_oracle import BufferOracle, relax_block
    nx, ny, nz = 64, 16, 8
    x, y, z, q0, s0 = _case(nx, ny, nz)
    d = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC[:1], yuniform=False)
    _load(d, q0, s0[:1])
    d.set_buffer_zones(3, 4, (7.0, 2.0), (9.0, 2.0))
    o = BufferOracle(x, y, z, nscal=1, visc=VISC, schmidt=SC[:1], yuniform=False)
    o.q, o.s = [a.copy() for a in q0], [s0[0].copy()]
    o.set_buffer_zones(3, 4, (7.0, 2.0), (9.0, 2.0))
    rng = np.random.default_rng(4)
    n = nx * ny * nz
    h0 = [rng.uniform(-1, 1, n) for _ in range(4)]
    hold = [torch.zeros(n + 1, dtype=torch.float64, device="cuda") for _ in range(8)]
    fld, ten = [t[1:] for t in hold[:4]], [t[1:] for t in hold[4:]]
    for t, a in zip(fld, q0 + s0[:1]):
        t.copy_(torch.from_numpy(a))
    for t, a in zip(ten, h0):
        t.copy_(torch.from_numpy(a))
    assert all(t.data_ptr() % 16 == 8 for t in fld + ten)
    arr = lambda ts: (c_vp * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
    check(load().tlab_dns_buffer_relax_flow(d._h, arr(fld[:3]), arr(ten[:3])), "tlab_dns_buffer_relax_flow")
    check(load().tlab_dns_buffer_relax_scal(d._h, arr(fld[3:]), arr(ten[3:])), "tlab_dns_buffer_relax_scal")
    torch.cuda.synchronize()
    want = [a.copy() for a in h0]
    for blk in o.buff_flow:
        relax_block(blk, q0, want[:3], nx, ny, nz)
    for blk in o.buff_scal:
        relax_block(blk, s0[:1], want[3:], nx, ny, nz)
    for t, w, a in zip(ten, want, h0):
        assert rel_err(t.cpu().numpy(), w) <= 1e-13 and not np.array_equal(w, a)
    assert all(float(t[0]) == 0.0 for t in hold)


FUSED_GRID = (256, 64, 64)
ROUTES = ["fused_dirichlet", "fused_neumann", "surface", "freeslip", "literal", "direct", "pfilter"]


def _route(T, route, mode):
    """(driver, oracle factory with zones, oracle factory without, q0, s0) of one route"""
    from tlab_amd.dns import Dns, RKM_EXP3, RKM_EXP4, scalar_bcs, velocity_bcs
    rkm = RKM_EXP3 if mode == "exp3" else RKM_EXP4
    setup, okw = [], {}
    if route == "direct":      # SpaceOrder2 = EllipticOrder = CompactDirect6, the combination of the CompactDirect6 example cases
        from oracle import tlab_oracle as O
        nx, ny, nz = 64, 64, 16
        g = np.load(golden_files("direct_y")[0])
        tab = {k[len("ny%d_" % ny):]: g[k] for k in g.files if k.startswith("ny%d_" % ny)}
        y = np.array(tab["nodes"])
        x, z = np.arange(nx) / nx * 2.0, np.arange(nz) / nz * 1.0
        q0, s0 = init_fields(nx, ny, nz, x, y, z, 43)
        s0 = [s0[0], 0.5 * s0[0] + 0.3, -0.6 * s0[0]]
        gy = T.FdmPlan.from_tables(tab, scheme1=6, scheme2=16)
        d = Dns(x, y, z, nscal=3, visc=VISC, schmidt=SC, yuniform=False, rkm_mode=rkm, plans=[T.FdmPlan(x, True, True), gy, T.FdmPlan(z, True, True)],
                gy_elliptic=gy)
        go = lambda: [O.FdmPlan(x, True, True), O.FdmPlan.from_tables(tab, mode2=O.FDM_COM6_DIRECT), O.FdmPlan(z, True, True)]      # noqa: E731
        okw = {"plans_factory": go}
    else:      # 256 x 64 x 64 is on the fully fused route of the driver (five Burgers launches carrying the pressure forcing; test_gpu_rhs.py)
        x, y, z, q0, s0 = _case() if route == "literal" else _case(*FUSED_GRID)
        d = Dns(x, y, z, nscal=3, visc=VISC, schmidt=SC, yuniform=False, rkm_mode=rkm)
    if route == "fused_neumann":
        d.set_bcs("noslip", "noslip", "neumann", "neumann")
        setup.append(lambda o: (setattr(o, "scal_jmin", [scalar_bcs("neumann")] * 3), setattr(o, "scal_jmax", [scalar_bcs("neumann")] * 3)))
    elif route == "surface":
        d.set_surface_bcs(["linear"] * 3, ["static"] * 3, [0.35] * 3, [0.0] * 3)
        setup.append(lambda o: (setattr(o, "sfc_jmin", [1] * 3), setattr(o, "cpl_jmin", [0.35] * 3)))
    elif route == "freeslip":
        d.set_bcs("freeslip", "freeslip", "neumann", "dirichlet")
        setup.append(lambda o: (setattr(o, "flow_jmin", velocity_bcs("freeslip")), setattr(o, "flow_jmax", velocity_bcs("freeslip")),
                                setattr(o, "scal_jmin", [scalar_bcs("neumann")] * 3)))
    elif route == "literal":
        d.set_fusion(False)
    elif route == "pfilter":      # [PressureFilter] along y: p and dp/dy are filtered, the scalars never see it and stay in the x Burgers epilogue
        from test_gpu_filter import device_filter, filter_of
        fdev, _ = device_filter(T, "n64_t1_p0_b66")
        forc, _ = filter_of("n64_t1_p0_b66")
        d.set_pressure_filter(None, fdev, None)
        setup.append(lambda o: setattr(o, "pressure_filter", [None, forc, None]))

    def factory(zones):
        if "plans_factory" in okw:
            def make():
                go = okw["plans_factory"]()
                return _oracle_factory(x, y, z, q0, s0, zones, setup, plans=go, gy_elliptic=go[1])()
            return make
        return _oracle_factory(x, y, z, q0, s0, zones, setup)
    return d, factory(True), factory(False), q0, s0


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mode", ["exp3", "exp4"])
def test_rk_step_with_zones_against_the_oracle(T, route, mode):
    d, make_on, make_off, q0, s0 = _route(T, route, mode)
    nx, ny, nz = d.nx, d.ny, d.nz
    _load(d, q0, s0)
    d.set_buffer_zones(PJMIN, PJMAX, PU, PS)
    sched = _schedule(d, 2e-3)
    B, S = substep_scatter(make_on, q0, s0, sched, nsamples=1 if (nx, ny, nz) == FUSED_GRID else 2)
    Boff, _ = substep_scatter(make_off, q0, s0, sched, nsamples=0)
    k = len(sched) - 1
    zone = _zone_planes(ny)
    # CPU side: the term must not be lost in the bound -- with and without zones the oracle differs by more than 100 x the bound inside the zone
    for name, idx in (("hq", (0, 1, 2)), ("hs", (0, 2))):
        for i in idx:
            on3, off3 = B[k][name][i].reshape(nz, ny, nx), Boff[k][name][i].reshape(nz, ny, nx)
            diff = np.abs(on3[:, zone, :] - off3[:, zone, :]).max() / np.abs(on3).max()
            assert diff > 100.0 * float(bound(S[k][name][i])), (route, mode, name, i, diff, S[k][name][i])
    d.TIME_RUNGEKUTTA(2e-3)
    for name in ("q", "s", "hq", "hs"):
        for i, (b, scat) in enumerate(zip(B[k][name], S[k][name])):
            e = rel_err(getattr(d, name)[i].cpu().numpy(), b)
            print("%s %s %s[%d]: err %.2e scatter %.2e" % (route, mode, name, i, e, scat))
            assert e <= bound(scat), (route, mode, name, i, "err %.2e" % e)
    # the wall plane of hs under the Jmax zone (Dirichlet there on every route but fused_neumann): the BC value minus tau_max (s - ref), on its own
    for i in (0, 2):
        got = d.hs[i].cpu().numpy().reshape(nz, ny, nx)[:, ny - 1, :]
        want = B[k]["hs"][i].reshape(nz, ny, nx)[:, ny - 1, :]
        assert np.abs(want).max() > 0.0
        e = float(np.abs(got - want).max() / np.abs(B[k]["hs"][i]).max())
        assert e <= bound(S[k]["hs"][i]), (route, mode, "wall plane of hs", i, e)
        if route != "fused_neumann":
            assert np.abs(want).max() / np.abs(B[k]["hs"][i]).max() > 100.0 * float(bound(S[k]["hs"][i]))


def _kernel_rows():
    from tlab_amd.lib import load
    L = load()
    buf = ctypes.create_string_buffer(32768)
    L.tlab_profile_report(buf, len(buf))
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
    return rows, [t.clone() for t in d.q + d.s + d.hq + d.hs]


@pytest.mark.parametrize("route", ["fused_dirichlet", "fused_neumann", "literal"])
def test_zones_switched_off_again_change_nothing(T, route):
    import torch
    from tlab_amd.dns import Dns
    x, y, z, q0, s0 = _case() if route == "literal" else _case(*FUSED_GRID)
    mk = lambda: Dns(x, y, z, nscal=3, visc=VISC, schmidt=SC, yuniform=False)      # noqa: E731
    never, d = mk(), mk()
    for m in (never, d):
        if route == "fused_neumann":
            m.set_bcs("noslip", "noslip", "neumann", "neumann")
        if route == "literal":
            m.set_fusion(False)
    rows0, f0 = _profiled_step(never, q0, s0)
    assert route == "literal" or rows0.get("k_htile<BURGERS+div>") == 6, rows0          # the fused routes are the fused routes
    _load(d, q0, s0)
    d.set_buffer_zones(PJMIN, PJMAX, PU, PS)
    rows_on, f_on = _profiled_step(d, q0, s0)
    assert rows_on.get("k_buffer_relax", 0) > 0 and not torch.equal(f_on[0], f0[0])
    d.set_buffer_zones(0, 0)
    rows1, f1 = _profiled_step(d, q0, s0)
    assert rows1 == rows0, (rows0, rows1)                      # the same kernel names and call counts as a driver that never had zones
    for a, b in zip(f0, f1):
        assert torch.equal(a, b)
    d.set_buffer_zones(PJMIN, PJMAX, PU, PS)
    d.set_buffer_zones(type="none")                            # [BufferZone] Type = none
    rows2, f2 = _profiled_step(d, q0, s0)
    assert rows2 == rows0
    for a, b in zip(f0, f2):
        assert torch.equal(a, b)


def test_fused_route_stays_fused_with_zones(T):
    """Fused Dirichlet route: every kernel of the run without zones is still launched as often -- the fused Burgers launches with the pressure
    forcing riding on them, the Poisson solver that finishes v, the gradient kernels that finish u and w -- plus the zone kernel (per substep: one
    launch per end for the flow, one per end for the scalars, all between the second and the third Burgers launch) and its wall-plane form (one
    launch per end): the Dirichlet scalars stay in the epilogue of the x Burgers launch, no update pass over them appears."""
    from tlab_amd.dns import Dns
    x, y, z, q0, s0 = _case(*FUSED_GRID)
    d = Dns(x, y, z, nscal=3, visc=VISC, schmidt=SC, yuniform=False)
    rows0, _ = _profiled_step(d, q0, s0)
    print(rows0)
    assert rows0.get("k_htile<BURGERS+div>") == 6 and "k_final_update" not in rows0 and "k_rk_update" not in rows0, rows0
    _load(d, q0, s0)
    d.set_buffer_zones(PJMIN, PJMAX, PU, PS)
    rows, _ = _profiled_step(d, q0, s0)
    for name, calls in rows0.items():
        assert rows.get(name) == calls, (name, calls, rows)
    assert set(rows) - set(rows0) == {"k_buffer_relax", "k_buffer_relax<wall plane>"}, rows
    assert rows["k_buffer_relax"] == 3 * 4 and rows["k_buffer_relax<wall plane>"] == 3 * 2, rows
    # flow zones only: the scalars stay in the epilogue
    d.set_buffer_zones(type="none")
    import numpy as _np
    from tlab_amd.lib import load
    tau = _np.full((3, PJMAX), 5.0)
    ref = _np.zeros((3, d.nz, PJMAX, d.nx))
    assert load().tlab_dns_set_buffer_zone(d._h, 4, 0, PJMAX, 3, tau.ctypes.data_as(DP), ref.ctypes.data_as(DP)) == 0
    rows, _ = _profiled_step(d, q0, s0)
    assert set(rows) - set(rows0) == {"k_buffer_relax"} and rows["k_buffer_relax"] == 3, rows


def test_rhs_alone_applies_the_flow_blocks_only(T):
    import torch
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load, check
    x, y, z, q0, s0 = _case(*FUSED_GRID)
    nx, ny, nz = len(x), len(y), len(z)
    mk = lambda: Dns(x, y, z, nscal=3, visc=VISC, schmidt=SC, yuniform=False)      # noqa: E731
    a, b = mk(), mk()
    for m in (a, b):
        _load(m, q0, s0)
        m.set_buffer_zones(PJMIN, PJMAX, PU, PS)
    dte, kco = 2e-3 / 3.0, -5.0 / 9.0
    sched = [(dte, kco, True, True)]
    B, S = substep_scatter(_oracle_factory(x, y, z, q0, s0, True), q0, s0, sched, nsamples=2)
    # the oracle's RHS alone: flow blocks in, scalar blocks not
    o = _oracle_factory(x, y, z, q0, s0, True)()
    o.q, o.s = [v.copy() for v in q0], [v.copy() for v in s0]
    o.rhs_global_incompressible_1(dte)
    a.begin_step()
    a.RHS_GLOBAL_INCOMPRESSIBLE_1(dte)
    for i in range(3):
        assert rel_err(a.hq[i].cpu().numpy(), o.hq[i]) <= bound(S[0]["hq"][i]), i
        assert rel_err(a.hs[i].cpu().numpy(), o.hs[i]) <= bound(S[0]["hs"][i]), i
        assert not a.hs[i].view(nz, ny, nx)[:, ny - 1, :].any()                  # Dirichlet wall plane: no scalar zone term yet
    a.buffer_relax_scal()
    L = load()
    for u, h in zip(a.q + a.s, a.hq + a.hs):
        check(L.tlab_pw_rk_update(u.data_ptr(), h.data_ptr(), dte, kco, 1, a.n), "tlab_pw_rk_update")
    b.begin_step()
    b.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dte, kco, True)
    torch.cuda.synchronize()
    for name in ("q", "s", "hq", "hs"):
        for i in range(3):
            got, fused = getattr(a, name)[i].cpu().numpy(), getattr(b, name)[i].cpu().numpy()
            assert rel_err(got, fused) <= bound(S[0][name][i]), (name, i)
            assert rel_err(fused, B[0][name][i]) <= bound(S[0][name][i]), (name, i)


def test_refusals(T):
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    x, y, z, q0, s0 = _case(64, 16, 8)
    d = Dns(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False)
    L = load()
    EINVAL, EUNSUPPORTED = -1, -2
    tau = np.ones(3 * 16)
    ref = np.zeros(64 * 16 * 8 * 3)
    t, r = tau.ctypes.data_as(DP), ref.ctypes.data_as(DP)
    JMIN, JMAX, FLOW, SCAL = 3, 4, 0, 1
    assert L.tlab_dns_set_buffer_zone(d._h, JMAX, FLOW, 1, 3, t, r) == EINVAL              # size == 1
    assert L.tlab_dns_set_buffer_zone(d._h, JMAX, FLOW, 4, 2, t, r) == EINVAL              # nfields: 3 for the flow
    assert L.tlab_dns_set_buffer_zone(d._h, JMIN, SCAL, 4, 3, t, r) == EINVAL              # ... nscal for the scalars
    assert L.tlab_dns_set_buffer_zone(d._h, JMIN, FLOW, 17, 3, t, r) == EINVAL             # size > ny
    assert L.tlab_dns_set_buffer_zone(d._h, JMIN, FLOW, 4, 3, t, None) == EINVAL
    bad = tau.copy(); bad[5] = np.nan
    assert L.tlab_dns_set_buffer_zone(d._h, JMIN, FLOW, 4, 3, bad.ctypes.data_as(DP), r) == EINVAL
    for end in (1, 2):                                                                     # Imin, Imax
        assert L.tlab_dns_set_buffer_zone(d._h, end, FLOW, 4, 3, t, r) == EUNSUPPORTED
    assert L.tlab_dns_set_buffer_zone(d._h, 7, FLOW, 4, 3, t, r) == EINVAL
    for code in (2, 3):                                                                    # filter, both
        assert L.tlab_dns_set_buffer_type(d._h, code) == EUNSUPPORTED
    assert L.tlab_dns_set_buffer_type(d._h, 9) == EINVAL
    for kw in (dict(points_jmax=1), dict(points_jmin=4, type="filter"), dict(points_jmin=4, type="both"), dict(points_imin=4), dict(points_imax=4),
               dict(points_jmin=4, params_s=(1.0, 2.0, 3.0, 4.0))):
        with pytest.raises(T.TlabError):
            d.set_buffer_zones(**kw)
    # none of the refused calls left a zone behind
    assert L.tlab_dns_set_buffer_zone(d._h, JMIN, FLOW, 4, 3, t, r) == 0 and L.tlab_dns_set_buffer_zone(d._h, JMIN, FLOW, 0, 3, None, None) == 0


def test_zone_that_spans_the_height_relaxes_both_wall_planes(T):
    """size == ny with sigma = 0: tau is the strength on every plane, the opposite wall included; the epilogue route redoes both wall planes."""
    from tlab_amd.dns import Dns
    from buffer_oracle import BufferOracle
    nx, ny, nz = FUSED_GRID
    x, y, z, q0, s0 = _case(nx, ny, nz)
    d = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC[:1], yuniform=False)
    _load(d, q0, s0[:1])
    args = (0, ny, (30.0, 0.0), (40.0, 0.0))
    d.set_buffer_zones(*args)

    def make():
        o = BufferOracle(x, y, z, nscal=1, visc=VISC, schmidt=SC[:1], yuniform=False, hyper_bc1_ext=0.0)
        o.q, o.s = [a.copy() for a in q0], [s0[0].copy()]
        o.set_buffer_zones(*args)
        return o
    sched = _schedule(d, 2e-3)
    B, S = substep_scatter(make, q0, s0[:1], sched, nsamples=1)
    d.TIME_RUNGEKUTTA(2e-3)
    k = len(sched) - 1
    for name in ("q", "s", "hq", "hs"):
        for i, (b, scat) in enumerate(zip(B[k][name], S[k][name])):
            assert rel_err(getattr(d, name)[i].cpu().numpy(), b) <= bound(scat), (name, i)
    got, want = d.hs[0].cpu().numpy().reshape(nz, ny, nx), B[k]["hs"][0].reshape(nz, ny, nx)
    for j in (0, ny - 1):
        assert np.abs(want[:, j, :]).max() / np.abs(want).max() > 100.0 * float(bound(S[k]["hs"][0]))
        assert float(np.abs(got[:, j, :] - want[:, j, :]).max() / np.abs(want).max()) <= bound(S[k]["hs"][0]), j


# ---- the deferred tail: time.f90's calls of an unchanged host, with BOUNDARY_BUFFER_RELAX_SCAL between the RHS and the DAXPYs ----
def _deferred_step(d, order, dtime=2e-3):
    """One RK3 step through the deferred entry points.  order: "time.f90" (RHS, relax, DAXPYs, DSCALs), "none" (no relaxation call), "late" (relax
    after the DAXPYs), "twice" (two relaxations after the RHS).  Returns (deferred stats, relax stats) differences."""
    import torch
    from tlab_amd.lib import load, check, c_vp
    L = load()
    mk = lambda ts: (c_vp * max(1, len(ts)))(*[t.data_ptr() for t in ts])      # noqa: E731
    q, s, hq, hs, txc = mk(d.q), mk(d.s), mk(d.hq), mk(d.hs), mk(d.txc)
    st0, rs0 = (ctypes.c_longlong * 6)(), (ctypes.c_longlong * 2)()
    check(L.tlab_deferred_stats(st0), "stats"); check(L.tlab_deferred_relax_stats(rs0), "relax stats")
    N = d.n
    check(L.tlab_deferred_enable(1), "enable")
    try:
        for t in d.hq + d.hs:
            check(L.tlab_deferred_zero(t.data_ptr(), N), "zero")
        for k in range(3):
            dte = dtime * d.kdt[k]
            check(L.tlab_deferred_rhs(d._h, dte, q, s, hq, hs, txc), "rhs")
            if order in ("time.f90", "twice"):
                check(L.tlab_deferred_relax_scal(d._h), "relax")
            if order == "twice":
                check(L.tlab_deferred_relax_scal(d._h), "relax")
            for h, u in zip(d.hq + d.hs, d.q + d.s):
                check(L.tlab_deferred_axpy(N, dte, h.data_ptr(), u.data_ptr()), "axpy")
            if order == "late":
                check(L.tlab_deferred_relax_scal(d._h), "relax")
            if k < 2:
                for h in d.hq + d.hs:
                    check(L.tlab_deferred_scal(N, d.kco[k], h.data_ptr()), "scal")
        check(L.tlab_deferred_flush(), "flush")
    finally:
        check(L.tlab_deferred_enable(0), "disable")
    torch.cuda.synchronize()
    st1, rs1 = (ctypes.c_longlong * 6)(), (ctypes.c_longlong * 2)()
    check(L.tlab_deferred_stats(st1), "stats"); check(L.tlab_deferred_relax_stats(rs1), "relax stats")
    return [b - a for a, b in zip(st0, st1)], [b - a for a, b in zip(rs0, rs1)]


def _zoned_driver(zones=True, scal_zones=True):
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    x, y, z, q0, s0 = _case(*FUSED_GRID)
    d = Dns(x, y, z, nscal=3, visc=VISC, schmidt=SC, yuniform=False)
    _load(d, q0, s0)
    if zones:
        d.set_buffer_zones(PJMIN, PJMAX, PU, PS)
        if not scal_zones:
            for end in (3, 4):
                assert load().tlab_dns_set_buffer_zone(d._h, end, 1, 0, 3, None, None) == 0
    return d, (x, y, z, q0, s0)


def test_deferred_tail_with_the_relaxation_is_the_fused_substep(T):
    import torch
    a, _ = _zoned_driver()
    b, _ = _zoned_driver()
    a.TIME_RUNGEKUTTA(2e-3)
    st, rs = _deferred_step(b, "time.f90")
    assert st[0] == 3 and st[1] == 0 and rs == [3, 0], (st, rs)            # three fused substeps, each carrying the relaxation; nothing literal
    for u, v in zip(a.q + a.s + a.hq + a.hs, b.q + b.s + b.hq + b.hs):
        assert torch.equal(u, v)


@pytest.mark.parametrize("order", ["late", "twice", "no_scalar_zones"])
def test_deferred_tail_out_of_order_runs_literally(T, order):
    """A relaxation after the DAXPYs, a second relaxation, a relaxation on a driver without scalar zones: the record runs literally, in call order,
    and the fields are those of an oracle that makes the same calls in the same order."""
    from buffer_oracle import BufferOracle
    d, (x, y, z, q0, s0) = _zoned_driver(scal_zones=order != "no_scalar_zones")
    st, rs = _deferred_step(d, "time.f90" if order == "no_scalar_zones" else order)
    assert st[0] == 0 and st[1] == 3 and rs[0] == 0 and rs[1] == (6 if order == "twice" else 3), (st, rs)

    class Ordered(BufferOracle):
        def time_substep(self, dte, kco=1.0, scale=False):
            self.rhs_global_incompressible_1(dte)
            if order == "twice":
                self.buffer_relax_scal(); self.buffer_relax_scal()
            elif order == "no_scalar_zones":
                self.buffer_relax_scal()                                   # (no blocks: nothing happens)
            for i in range(3):
                self.q[i] = self.q[i] + dte * self.hq[i]
            for i in range(self.nscal):
                self.s[i] = self.s[i] + dte * self.hs[i]
            if order == "late":
                self.buffer_relax_scal()                                   # with the UPDATED s, into the tendency the next substep continues from
            if scale:
                self.hq = [kco * h for h in self.hq]
                self.hs = [kco * h for h in self.hs]

    def make():
        o = Ordered(x, y, z, nscal=3, visc=VISC, schmidt=SC, yuniform=False, hyper_bc1_ext=0.0)
        o.q, o.s = [v.copy() for v in q0], [v.copy() for v in s0]
        o.set_buffer_zones(PJMIN, PJMAX, PU, PS)
        if order == "no_scalar_zones":
            o.buff_scal = [None, None]
        return o
    sched = _schedule(d, 2e-3)
    B, S = substep_scatter(make, q0, s0, sched, nsamples=1)
    for name in ("q", "s", "hq", "hs"):
        for i, (b, scat) in enumerate(zip(B[2][name], S[2][name])):
            e = rel_err(getattr(d, name)[i].cpu().numpy(), b)
            assert e <= bound(scat), (order, name, i, "err %.2e" % e)


def test_deferred_record_without_the_relaxation_leaves_the_scalars_alone(T):
    """RHS + DAXPY + DSCAL with scalar zones set and NO relaxation call: the fused replay must give what the literal replay gives -- the flow blocks
    (they belong to the RHS), no scalar blocks.  Equal to a driver that holds the flow blocks only, bit for bit."""
    import torch
    a, _ = _zoned_driver(scal_zones=False)
    b, _ = _zoned_driver()
    a.TIME_RUNGEKUTTA(2e-3)
    st, rs = _deferred_step(b, "none")
    assert st[0] == 3 and st[1] == 0 and rs == [0, 0], (st, rs)
    for u, v in zip(a.q + a.s + a.hq + a.hs, b.q + b.s + b.hq + b.hs):
        assert torch.equal(u, v)
    b.TIME_RUNGEKUTTA(2e-3)                                                # the driver's own substep applies the scalar blocks again afterwards
    a.TIME_RUNGEKUTTA(2e-3)
    assert not torch.equal(a.s[0], b.s[0])


@pytest.mark.parametrize("bcs", ["dirichlet", "neumann"])
def test_slab_driver_with_zones_equals_the_single_domain(T, bcs):
    """Loopback z-slabs, 4 ranks, with zones against the single-domain result, within the bound the slab driver's own tests use against it (the
    one-ulp scatter of the oracle, here the zoned oracle); and the zones must matter: without them the slabs miss the same bound by far."""
    import torch
    from tlab_amd.dns import Dns, scalar_bcs
    from tlab_amd.slab import NativeSlabDns
    nx, ny, nz = 128, 24, 256
    x, y, z, q0, s0 = _case(nx, ny, nz)
    kw = dict(nscal=3, visc=VISC, schmidt=SC, yuniform=False)
    d = Dns(x, y, z, **kw)
    d.set_bcs("noslip", "noslip", bcs, bcs)
    _load(d, q0, s0)
    d.set_buffer_zones(PJMIN, PJMAX, PU, PS)
    d.TIME_RUNGEKUTTA(2e-3)
    one = {"q": [t.clone() for t in d.q], "s": [t.clone() for t in d.s]}
    setup = [lambda o: (setattr(o, "scal_jmin", [scalar_bcs(bcs)] * 3), setattr(o, "scal_jmax", [scalar_bcs(bcs)] * 3))]
    sched = _schedule(d, 2e-3)
    _, S = substep_scatter(_oracle_factory(x, y, z, q0, s0, True, setup), q0, s0, sched, nsamples=1)
    del d
    errs = {}
    for zones in (True, False):
        m = NativeSlabDns("loopback", x, y, z, size=4, **kw)
        m.set_bcs("noslip", "noslip", bcs, bcs)
        for i in range(3):
            m.scatter("q", i, torch.from_numpy(q0[i]).cuda())
            m.scatter("s", i, torch.from_numpy(s0[i]).cuda())
        if zones:
            m.set_buffer_zones(PJMIN, PJMAX, PU, PS)
        for k in range(m.rkm_endstep):
            m.substep_of_cycle(k, 2e-3)
        torch.cuda.synchronize()
        for name in ("q", "s"):
            for i, rf in enumerate(one[name]):
                got = torch.cat([m.st[r][name][i] for r in m.local_ranks])
                errs[(zones, name, i)] = float((got - rf).abs().max() / rf.abs().max())
        m.close()
    for name in ("q", "s"):
        for i in range(3):
            assert errs[(True, name, i)] <= bound(S[2][name][i]), (name, i, errs[(True, name, i)])
            if (name, i) != ("s", 1):
                assert errs[(False, name, i)] > 100.0 * float(bound(S[2][name][i])), (name, i, errs[(False, name, i)])


def test_pencil_driver_with_zones_equals_the_single_domain(T):
    """2 x 2 loopback pencils with zones against the single-domain result, within the one-ulp scatter bound of the zoned oracle (the bound the pencil
    driver's tests use against the single domain); without zones the pencils miss it by far."""
    import torch
    from tlab_amd.dns import Dns
    from tlab_amd.pencil import NativePencilDns
    nx, ny, nz = 128, 24, 256
    x, y, z, q0, s0 = _case(nx, ny, nz)
    kw = dict(nscal=3, visc=VISC, schmidt=SC, yuniform=False)
    d = Dns(x, y, z, **kw)
    _load(d, q0, s0)
    d.set_buffer_zones(PJMIN, PJMAX, PU, PS)
    d.TIME_RUNGEKUTTA(2e-3)
    one = {"q": [t.clone() for t in d.q], "s": [t.clone() for t in d.s]}
    sched = _schedule(d, 2e-3)
    _, S = substep_scatter(_oracle_factory(x, y, z, q0, s0, True), q0, s0, sched, nsamples=1)
    del d
    errs = {}
    for zones in (True, False):
        m = NativePencilDns("loopback", 2, 2, x, y, z, **kw)
        for i in range(3):
            m.scatter("q", i, torch.from_numpy(q0[i]).cuda())
            m.scatter("s", i, torch.from_numpy(s0[i]).cuda())
        if zones:
            m.set_buffer_zones(PJMIN, PJMAX, PU, PS)
        for k in range(m.rkm_endstep):
            m.substep_of_cycle(k, 2e-3)
        torch.cuda.synchronize()
        for name in ("q", "s"):
            for i, rf in enumerate(one[name]):
                out = torch.empty(nz, ny, nx, dtype=torch.float64, device="cuda")
                for r, t in m.gather_local(name, i).items():
                    pi, pk = m.pro(r)
                    out[pk * m.kmax:(pk + 1) * m.kmax, :, pi * m.imax:(pi + 1) * m.imax] = t.view(m.kmax, ny, m.imax)
                errs[(zones, name, i)] = float((out.reshape(-1) - rf).abs().max() / rf.abs().max())
        m.close()
    for name in ("q", "s"):
        for i in range(3):
            assert errs[(True, name, i)] <= bound(S[2][name][i]), (name, i, errs[(True, name, i)])
            if (name, i) != ("s", 1):
                assert errs[(False, name, i)] > 100.0 * float(bound(S[2][name][i])), (name, i, errs[(False, name, i)])
