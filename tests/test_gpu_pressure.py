"""tlab_dns_pressure (FI_PRESSURE_BOUSSINESQ on the device: a route through the stages of the substep, csrc/rhs.cpp) against the numpy restatement
tests/pressure_oracle.py, which tests/test_pressure_host.py holds to the reference's own compiled routines.

Every case is device p against the restatement with err <= bound(scatter): max(1e-12, 2 x the restatement's own one-ulp scatter) relative to max|p|
(tests/scatter.py), on the fields of tests/cases.py.  A restatement is computed once per configuration and shared (read-only).  The shapes are those
of tests/launch_census.py: 256 x 64 x 64 takes the five-launch Burgers route -- which the test ASSERTS from the library's own profile, so that a case
meant for a fused route cannot pass through the literal one unnoticed --, 32 x 40 x 16 no fast kernel, 256 x 64 x 1 and 1024 x 64 x 16 the
per-equation sums of the census' nz1 and nx1024."""
import ctypes
import functools

import numpy as np
import pytest

import cases as C
import pressure_oracle as P
from conftest import rel_err
from launch_census import FAST, FORCES, FREESLIP, REF_HYPER, SMALL
from scatter import bound, scatter_of

pytestmark = pytest.mark.gpu

VISC, SC = 1.0 / 800.0, (0.7,)
COR, BOD = P.GOLDEN_COR, P.GOLDEN_BOD                    # launch_census.FORCES as the tuples of tests/sources_oracle.py
ALL = ("total", "advection", "advdiff", "diffusion", "coriolis", "buoyancy")
FILTER = "n64_t1_p0_b66"                                 # [PressureFilter] along y on the 64-point stretched grid (tests/golden/filters.npz)


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def background(y):
    rb = 1.0 + 0.6 * np.exp(-2.5 * (y - y[0]) / (y[-1] - y[0]))
    return rb, 1.0 / rb


@functools.lru_cache(maxsize=None)
def _fields(shape, freeslip):
    nx, ny, nz = shape
    x, y, z = C.grids(nx, ny, nz, True)
    q0, s0 = C.neumann_fields(x, y, z, 21) if freeslip else C.init_fields(nx, ny, nz, x, y, z, 3)
    for a in q0 + s0:
        a.setflags(write=False)
    return x, y, z, tuple(q0), tuple(s0)


@functools.lru_cache(maxsize=None)
def _reference(shape, decomposition, nscal=1, forces=True, freeslip=False, anelastic=False, stagger=False, pfilter=False):
    """(p, one-ulp scatter) of the restatement, computed once and shared"""
    from oracle.tlab_oracle_rhs import DnsOracle
    x, y, z, q0, s0 = _fields(shape, freeslip)
    cor, bod = (COR if forces else None), (BOD if forces and nscal else None)

    def run(*f):
        o = DnsOracle(x, y, z, nscal=nscal, visc=VISC, schmidt=SC[:nscal], yuniform=False, anelastic=background(y) if anelastic else None, stagger=stagger)
        if pfilter:
            from test_gpu_filter import filter_of
            o.pressure_filter = [None, filter_of(FILTER)[0], None]
        o.q, o.s = [np.array(a) for a in f[:3]], [np.array(a) for a in f[3:]]
        return (P.fi_pressure_boussinesq(o, decomposition, cor, bod),)
    (p,), (sc,) = scatter_of(run, list(q0) + list(s0[:nscal]), nsamples=1)
    p.setflags(write=False)
    return p, sc


class Driver:
    """a Dns with the fields of the configuration loaded; leaves the operator state as it found it"""

    def __init__(self, T, shape, nscal=1, forces=True, freeslip=False, anelastic=False, stagger=False, pfilter=False, fuse=True):
        import torch
        from tlab_amd.dns import Dns
        x, y, z, q0, s0 = _fields(shape, freeslip)
        self.anelastic, self.keep = anelastic, []
        self.d = d = Dns(x, y, z, nscal=nscal, visc=VISC, schmidt=SC[:nscal] if nscal else (1.0,), yuniform=False, hyper_bc1_ext=REF_HYPER, stagger=stagger)
        d.set_fusion(fuse)
        if freeslip:
            d.set_bcs(*FREESLIP)
        if anelastic:
            d.set_anelastic(background(y)[0])
        if pfilter:
            from test_gpu_filter import device_filter
            self.keep.append(device_filter(T, FILTER)[0])
            d.set_pressure_filter(None, self.keep[-1], None)
        if forces:
            d.set_body_forces(FORCES["coriolis"], FORCES["buoyancy"] if nscal else None)
        for i in range(3):
            d.q[i].copy_(torch.from_numpy(np.array(q0[i])))
        for i in range(nscal):
            d.s[i].copy_(torch.from_numpy(np.array(s0[i])))

    def __enter__(self):
        return self.d

    def __exit__(self, *exc):
        if self.anelastic:
            self.d.set_anelastic(None)


def _check(d, decomposition, ref, tag):
    p, sc = ref
    got = d.FI_PRESSURE_BOUSSINESQ(decomposition=decomposition)[: d.n].cpu().numpy()
    err = rel_err(got, p)
    print("%s %-10s err %.3e scatter %.3e" % (tag, decomposition, err, sc))
    assert err <= bound(sc), (tag, decomposition, err, sc)
    return got


def _profiled(fn):
    """{tag: (calls, bytes)} of the library's profile over fn()"""
    import torch
    from tlab_amd.lib import load
    L = load()
    torch.cuda.synchronize()
    L.tlab_profile_reset(); L.tlab_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 16)
        L.tlab_profile_report(buf, len(buf))
    finally:
        L.tlab_profile_enable(0)
        L.tlab_profile_reset()
    rows = [r.split("\t") for r in buf.value.decode().splitlines() if "\t" in r]
    return {r[0]: (int(r[1]), float(r[3])) for r in rows}


# ---- the fused default: five Burgers launches, the forcing on them, no scalar equation ---------------------------------------------------------------
def test_total_on_the_five_launch_route_and_on_the_literal_one(T):
    ref = _reference(FAST, "total")
    with Driver(T, FAST) as d:
        rows = _profiled(lambda: _check(d, "total", ref, "fused"))
        calls = {k: v[0] for k, v in rows.items()}
        # z (u, v), y (u, w), x (u, v, w: finishes u, writes the x term), y (v: the y term), z (w: the z term); the forces after the second
        assert calls.get("k_htile<BURGERS>") == 2 and calls.get("k_xline<BURGERS>") == 1 and calls.get("k_htile<BURGERS+div>") == 2, calls
        assert calls.get("k_body_force") == 1, calls
        for tag in ("k_add3", "k_sum3", "k_axpy3", "k_sub3", "k_final_update", "k_rk_update", "k_generic", "k_burgers_epilogue", "k_htile<P1>", "k_xline<P1>",
                    "k_rtile<P1>", "k_axpy1"):      # no literal sum, no forcing pass, no gradient, no update
            assert tag not in calls, (tag, calls)
        # no scalar equation: the x launch of a substep of the same driver carries the scalar as a fourth field and moves more bytes
        d.begin_step()
        sub = _profiled(lambda: d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(2e-3 / 3.0, -5.0 / 9.0, True))
        assert sub["k_xline<BURGERS>"][0] == 1 and rows["k_xline<BURGERS>"][1] < sub["k_xline<BURGERS>"][1], (rows, sub)
    with Driver(T, FAST, fuse=False) as d:
        rows = _profiled(lambda: _check(d, "total", ref, "literal"))
        assert "k_htile<BURGERS+div>" not in rows and rows.get("k_sum3", (0,))[0] == 1, rows


# ---- no fast kernel: every decomposition -----------------------------------------------------------------------------------------------------------
def test_every_decomposition_where_no_fast_kernel_applies(T):
    with Driver(T, SMALL) as d:
        got = {dc: _check(d, dc, _reference(SMALL, dc), "small") for dc in ALL}
        ref, sc = _reference(SMALL, "advdiff")
        err = rel_err(got["advection"] + got["diffusion"], ref)
        assert err <= bound(max(sc, _reference(SMALL, "advection")[1], _reference(SMALL, "diffusion")[1])), err
        for a, b in (("total", "advdiff"), ("advdiff", "advection"), ("coriolis", "buoyancy"), ("diffusion", "advection")):
            assert rel_err(got[a], got[b]) > 1e-3, (a, b)      # (no decomposition passes as another)
        with pytest.raises(T.TlabError):
            d.FI_PRESSURE_BOUSSINESQ(decomposition=1)           # DCMP_RESOLVED is not a case of the routine
        with pytest.raises(T.TlabError):
            d.FI_PRESSURE_BOUSSINESQ(decomposition="resolved")


def test_every_decomposition_on_the_fused_routes(T):
    """advdiff: the five launches; diffusion: the three-launch form with a zero velocity and the fused forcing launches; advection: two passes of that
    form; coriolis and buoyancy: one k_body_force and the fused forcing launches"""
    with Driver(T, FAST) as d:
        for dc in ALL[1:]:
            rows = _profiled(lambda dc=dc: _check(d, dc, _reference(FAST, dc), "fast"))
            calls = {k: v[0] for k, v in rows.items()}
            assert "k_add3" not in calls and "k_sum3" not in calls and "k_generic" not in calls, (dc, calls)
            if dc == "advection":
                assert calls.get("k_htile<BURGERS>") == 4 and calls.get("k_xline<BURGERS>") == 2 and calls.get("k_sub3") == 1, calls
            elif dc == "diffusion":
                assert calls.get("k_htile<BURGERS>") == 2 and calls.get("k_xline<BURGERS>") == 1 and "k_htile<BURGERS+div>" not in calls, calls
            elif dc == "advdiff":
                assert calls.get("k_htile<BURGERS+div>") == 2 and calls.get("k_xline<BURGERS>") == 1, calls
            else:
                assert calls.get("k_body_force") == 1 and not any("BURGERS" in k for k in calls), (dc, calls)


# ---- the census' other routes, walls, the pressure filter, no scalar ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 64, 1), (1024, 64, 16)])
def test_total_on_the_per_equation_routes(T, shape):
    with Driver(T, shape) as d:
        _check(d, "total", _reference(shape, "total"), "x".join(map(str, shape)))


def test_total_with_free_slip_walls(T):
    """the routine knows no wall type: the walls only change what decide_route finds"""
    with Driver(T, FAST, freeslip=True) as d:
        _check(d, "total", _reference(FAST, "total", freeslip=True), "freeslip")


def test_total_with_a_pressure_filter(T):
    ref = _reference(FAST, "total", pfilter=True)
    assert rel_err(ref[0], _reference(FAST, "total")[0]) > 1e-6          # (the filter does something)
    with Driver(T, FAST, pfilter=True) as d:
        _check(d, "total", ref, "pfilter")


def test_total_without_scalars(T):
    with Driver(T, FAST, nscal=0) as d:
        _check(d, "total", _reference(FAST, "total", nscal=0), "nscal0")
        _check(d, "coriolis", _reference(FAST, "coriolis", nscal=0), "nscal0")


@pytest.mark.gpu_extra
def test_total_anelastic(T):
    shape = (64, 40, 32)
    ref = _reference(shape, "total", anelastic=True)
    assert rel_err(ref[0], _reference(shape, "total")[0]) > 1e-6
    for fuse in (True, False):
        with Driver(T, shape, anelastic=True, fuse=fuse) as d:
            _check(d, "total", ref, "anelastic fuse=%s" % fuse)


@pytest.mark.gpu_extra
def test_total_on_the_staggered_pressure_grid(T):
    shape = (64, 40, 32)
    ref = _reference(shape, "total", stagger=True)
    assert rel_err(ref[0], _reference(shape, "total")[0]) > 1e-6
    with Driver(T, shape, stagger=True) as d:
        _check(d, "total", ref, "stagger")
        _check(d, "advection", _reference(shape, "advection", stagger=True), "stagger")


# ---- the state of the driver ------------------------------------------------------------------------------------------------------------------
def test_the_call_changes_no_state(T):
    import torch
    with Driver(T, FAST) as a, Driver(T, FAST) as b:
        g = torch.Generator(device="cuda").manual_seed(5)
        for m in (a, b):                                            # whatever the tendencies hold from the last step must neither be read nor changed
            for t, src in zip(m.hq + m.hs, a.hq + a.hs):
                t.copy_(torch.rand(t.shape, generator=g, device="cuda", dtype=torch.float64) if m is a else src)
        before = [t.clone() for t in a.q + a.s + a.hq + a.hs]
        a.begin_step()
        p1 = a.FI_PRESSURE_BOUSSINESQ().clone()
        p2 = a.FI_PRESSURE_BOUSSINESQ(decomposition="advection").clone()      # (the calls share self.txc[2])
        p3 = a.FI_PRESSURE_BOUSSINESQ()
        assert torch.equal(p1[: a.n], p3[: a.n]) and not torch.equal(p1[: a.n], p2[: a.n])      # two calls give the same bits
        for t, t0 in zip(a.q + a.s + a.hq + a.hs, before):
            assert torch.equal(t, t0)
        b.begin_step()
        for m in (a, b):                                            # the one-shot flag of begin_step is still there: the substep overwrites hq, hs
            m.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(2e-3 / 3.0, -5.0 / 9.0, True)
        for t, u in zip(a.q + a.s + a.hq + a.hs, b.q + b.s + b.hq + b.hs):
            assert torch.equal(t, u)
        assert not torch.equal(a.hq[0], before[3 + a.nscal])


def test_refusals_on_the_device(T):
    from tlab_amd.lib import load
    with Driver(T, SMALL, forces=False) as d:
        y = _fields(SMALL, False)[1]
        tilted = {"type": "linear", "vector": (0.4, -2.0, 0.0), "parameters": (1.0, 0.1), "bbackground": 0.3 * np.asarray(y)}
        d.set_body_forces(None, tilted)
        d.FI_PRESSURE_BOUSSINESQ(decomposition="total")                                   # TLab_Sources_Flow's form is served ...
        with pytest.raises(T.TlabError):
            d.FI_PRESSURE_BOUSSINESQ(decomposition="buoyancy")                            # ... the decomposition's is refused, not approximated
        assert b"bbackground" in load().tlab_last_error()
        d.set_body_forces(None, dict(tilted, bbackground=None))
        d.FI_PRESSURE_BOUSSINESQ(decomposition="buoyancy")
        with pytest.raises(T.TlabError):
            d.FI_PRESSURE_BOUSSINESQ(p=d.txc[3], decomposition="advection")               # p taken from the sums: six work arrays are left
