"""The monitors of the main loop on the device (dns_main.f90:268, :273): TIME_COURANT and DNS_BOUNDS_CONTROL's dilatation check with the location of
its failure branch, on the single domain, on z-slabs and on x/z pencils (tlab_amd/csrc/monitor.hip), the MINMAX guard and the Fortran monitors."""
import ctypes
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_HYPER = 0.1
NX, NY, NZ = 32, 24, 128
KW = dict(nscal=1, visc=1.0 / 700.0, schmidt=(0.5,), yuniform=False, hyper_bc1_ext=REF_HYPER)
PENCILS = [(2, 2), (2, 4), (1, 8)]      # (1, 8): npro_i = 1 over slabs of 16 planes, too thin for the slab driver


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def grids(nx=NX, ny=NY, nz=NZ):
    x = np.arange(nx) / nx * 2 * np.pi
    z = np.arange(nz) / nz * np.pi
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    return x, y, z


def smooth_fields(x, y, z, seed, amp=1.0):
    rng = np.random.default_rng(seed)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wall = np.sin(np.pi * (Y - y[0]) / (y[-1] - y[0]))
    return [(amp * (np.sin(X + k) * np.cos(2 * Z + k) + 0.1 * rng.uniform(-1, 1, X.shape)) * wall).ravel() for k in range(4)]


def spiked_fields(x, y, z):
    """a unique dilatation maximum and minimum next to a spike of u at (i, j, k) = (16, 11, 64) (1-based): the x derivative of the spike is largest on
    its two x neighbours, one of them across the x boundary of the pencils, the spike on the last plane of a slab / pencil"""
    f = smooth_fields(x, y, z, 3, amp=0.1)
    u = f[0].reshape(len(z), len(y), len(x))
    u[63, 10, 15] += 50.0
    return f


def tie_fields(x, y, z):
    """u = w = 0, v = y^2: div = dv/dy, the same on every (i, k) -- the maximum on the whole plane j = ny, the minimum on j = 1"""
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return [np.zeros(X.size), (Y ** 2).ravel().copy(), np.zeros(X.size), np.zeros(X.size)]


def make_dns(x, y, z, fields):
    import torch
    from tlab_amd.dns import Dns
    d = Dns(x, y, z, **KW)
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(fields[i]))
    d.s[0].copy_(torch.from_numpy(fields[3]))
    return d


def make_slab(x, y, z, fields, P=2):
    import torch
    from tlab_amd.slab import NativeSlabDns
    d = NativeSlabDns("loopback", x, y, z, size=P, **KW)
    for i in range(4):
        d.scatter("q" if i < 3 else "s", i if i < 3 else 0, torch.from_numpy(fields[i]).cuda())
    return d


def make_pencil(x, y, z, fields, npi, npk):
    import torch
    from tlab_amd.pencil import NativePencilDns
    d = NativePencilDns("loopback", npi, npk, x, y, z, **KW)
    for i in range(4):
        d.scatter("q" if i < 3 else "s", i if i < 3 else 0, torch.from_numpy(fields[i]).cuda())
    return d


def oracle_div(x, y, z, fields):
    from oracle.tlab_oracle_rhs import DnsOracle
    o = DnsOracle(x, y, z, nscal=1, visc=KW["visc"], schmidt=KW["schmidt"], yuniform=False)
    for i in range(3):
        o.q[i] = fields[i].copy()
    return -o.fi_invariant_p()


def first_loc(flat, nx, ny, fn):
    """numpy's first occurrence in Fortran order (x fastest = the flat order here), 1-based (i, j, k)"""
    e = int(fn(flat))
    return (e % nx + 1, (e // nx) % ny + 1, e // (nx * ny) + 1)


@pytest.mark.parametrize("npi,npk", PENCILS)
def test_pencil_monitors_match_the_single_domain_and_the_oracle(T, npi, npk):
    x, y, z = grids()
    f = smooth_fields(x, y, z, 11)
    single = make_dns(x, y, z, f)
    pen = make_pencil(x, y, z, f, npi, npk)
    (p1, p2), dt = single.TIME_COURANT(1.2, 0.25)
    (r1, r2), rdt = pen.TIME_COURANT(1.2, 0.25)
    assert (r1, r2, rdt) == (p1, p2, dt)                  # bit for bit: the global one_ov_ds1 entries at i + ims_offset_i, k + ims_offset_k
    from tlab_amd.lib import load, check
    pm = (ctypes.c_double * 2)()
    check(load().tlab_pencil_dns_courant_local(pen._h, pm), "tlab_pencil_dns_courant_local")
    assert (pm[0], pm[1]) == (p1, p2)                     # (loopback: every rank is local)
    ref = oracle_div(x, y, z, f)
    scale = np.abs(ref).max()
    smin, smax = single.dilatation_bounds()
    for dmin, dmax in (pen.dilatation_bounds(), pen.dilatation_extremes(locations=False), single.dilatation_extremes(locations=False)):
        assert abs(dmin - ref.min()) <= 1e-12 * scale and abs(dmax - ref.max()) <= 1e-12 * scale, (dmin, dmax, ref.min(), ref.max())
        assert abs(dmin - smin) <= 1e-12 * scale and abs(dmax - smax) <= 1e-12 * scale
    pen.close()


@pytest.mark.parametrize("kind", ["spike", "tie", "zero"])
def test_extremes_with_location_agree_on_every_driver(T, kind):
    x, y, z = grids()
    f = {"spike": spiked_fields, "tie": tie_fields, "zero": lambda *a: [np.zeros(NX * NY * NZ) for _ in range(4)]}[kind](x, y, z)
    ref = oracle_div(x, y, z, f)
    want = (first_loc(ref, NX, NY, np.argmin), first_loc(ref, NX, NY, np.argmax))
    if kind == "spike":
        assert all(w[1] == 11 and w[2] == 64 and 14 <= w[0] <= 18 for w in want), want      # next to the planted spike
    elif kind == "tie":
        assert want == ((1, 1, 1), (1, NY, 1)), want
    else:
        assert want == ((1, 1, 1), (1, 1, 1))
    scale = max(np.abs(ref).max(), 1e-300)
    drivers = [("single", make_dns(x, y, z, f)), ("slab2", make_slab(x, y, z, f))]
    drivers += [("pencil%dx%d" % pk, make_pencil(x, y, z, f, *pk)) for pk in PENCILS]
    for name, d in drivers:
        dmin, dmax, lmin, lmax = d.dilatation_extremes()
        assert (lmin, lmax) == want, (name, lmin, lmax, want)
        assert abs(dmin - ref.min()) <= 1e-12 * scale and abs(dmax - ref.max()) <= 1e-12 * scale, (name, dmin, dmax)
        if hasattr(d, "close"):
            d.close()


def test_monitors_run_the_recorded_substep_first(T):
    """the deferred tail: a recorded RHS + DAXPYs (time.f90's last substep) is still pending when a monitor is called; the monitor must see the
    updated q (single domain and a one-rank pencil driver, whose arrays the deferred layer knows)"""
    import torch
    from tlab_amd.lib import load, check
    from tlab_amd.dns import device_minmax
    L = load()
    x, y, z = grids(32, 24, 32)
    f = smooth_fields(x, y, z, 5)
    dte = 2e-3

    def run(d, record, q, h, monitors):
        for t, a in zip(q, f):
            t.copy_(torch.from_numpy(a).cuda())
        for t in h:
            t.zero_()
        torch.cuda.synchronize()
        before = monitors()
        check(L.tlab_deferred_enable(1), "enable")
        try:
            record()
            for hh, u in zip(h, q):
                check(L.tlab_deferred_axpy(u.numel(), dte, hh.data_ptr(), u.data_ptr()), "axpy")
            after = monitors()               # nothing synchronised in between: the monitors flush the recorded substep themselves
        finally:
            check(L.tlab_deferred_enable(0), "disable")
        return before, after

    d = make_dns(x, y, z, f)
    arrs = d._arrays()
    mon = lambda: (d.TIME_COURANT(1.0, 0.2)[0][0], d.dilatation_extremes(), device_minmax(d.q[0]))      # noqa: E731
    b1, a1 = run(d, lambda: check(L.tlab_deferred_rhs(d._h, dte, *arrs), "rhs"), d.q + d.s, d.hq + d.hs, mon)
    # the literal substep on the same start gives the monitors' values
    for t, a in zip(d.q + d.s, f):
        t.copy_(torch.from_numpy(a).cuda())
    for t in d.hq + d.hs:
        t.zero_()
    d.RHS_GLOBAL_INCOMPRESSIBLE_1(dte)
    for u, h in zip(d.q + d.s, d.hq + d.hs):
        u.add_(dte * h)
    ref = mon()
    assert a1[1][0] != b1[1][0] and a1[0] != b1[0]
    assert abs(a1[0] - ref[0]) <= 1e-12 * abs(ref[0])
    assert abs(a1[1][0] - ref[1][0]) <= 1e-9 * abs(b1[1][0]) and abs(a1[1][1] - ref[1][1]) <= 1e-9 * abs(b1[1][1])
    assert abs(a1[2][0] - ref[2][0]) <= 1e-12 and abs(a1[2][1] - ref[2][1]) <= 1e-12

    p = make_pencil(x, y, z, f, 1, 1)
    S = p.st[0]
    pmon = lambda: (p.TIME_COURANT(1.0, 0.2)[0][0], p.dilatation_extremes())      # noqa: E731
    b2, a2 = run(p, lambda: check(L.tlab_deferred_pencil_rhs(p._h, dte), "pencil rhs"), S["q"] + S["s"], S["hq"] + S["hs"], pmon)
    assert a2[0] != b2[0] and a2[1][0] != b2[1][0]
    assert abs(a2[0] - ref[0]) <= 1e-12 * abs(ref[0])
    assert abs(a2[1][0] - ref[1][0]) <= 1e-9 * abs(b1[1][0]) and abs(a2[1][1] - ref[1][1]) <= 1e-9 * abs(b1[1][1])
    p.close()


def test_minmax_guard_sends_only_device_arrays_to_the_kernel(T):
    import torch
    from tlab_amd.lib import load, check
    L = load()
    rng = np.random.default_rng(2)
    a = rng.uniform(-3, 2, 1_000_001)          # odd: the scalar-load instance
    dev = torch.from_numpy(a).cuda()
    mn, mx = ctypes.c_double(), ctypes.c_double()

    def calls():
        buf = ctypes.create_string_buffer(1 << 14)
        assert L.tlab_profile_report(buf, len(buf)) >= 0
        return sum(int(line.split("\t")[1]) for line in buf.value.decode().splitlines() if line.startswith("k_extremes_partial"))
    check(L.tlab_profile_enable(1), "profile")
    check(L.tlab_profile_filter(b""), "filter")
    try:
        check(L.tlab_profile_reset(), "reset")
        check(L.tlab_minmax_any(ctypes.c_void_p(dev.data_ptr()), dev.numel(), ctypes.byref(mn), ctypes.byref(mx)), "device")
        assert (mn.value, mx.value) == (a.min(), a.max())
        assert calls() == 1
        host = np.ascontiguousarray(a[:-1])     # even
        check(L.tlab_minmax_any(host.ctypes.data_as(ctypes.c_void_p), host.size, ctypes.byref(mn), ctypes.byref(mx)), "host")
        assert (mn.value, mx.value) == (host.min(), host.max())
        assert calls() == 1                      # the host array took the host loop
        check(L.tlab_device_minmax(ctypes.c_void_p(dev.data_ptr()), dev.numel() - 1, ctypes.byref(mn), ctypes.byref(mx)), "device even")
        assert (mn.value, mx.value) == (host.min(), host.max())
        assert calls() == 2
    finally:
        check(L.tlab_profile_enable(0), "profile off")


RK_EXE = os.path.join(ROOT, "tlab_amd", "fortran", "_build_rk", "test_rk_driver")


def _driver_has_monitors():
    """the driver is built from the reference's files, so where the reference is absent build() puts back a prebuilt one (oracle/_ref/fortran): that
    one may predate TLab_AMD_Monitors, and then it has no TLAB_AMD_MONITORS switch to run"""
    with open(RK_EXE, "rb") as f:
        return b"TLAB_AMD_MONITORS" in f.read()


@pytest.mark.parametrize("route", [None, "TLAB_AMD_FORCE_SLAB", "TLAB_AMD_FORCE_PENCIL"])
def test_fortran_monitors_equal_the_python_drivers(T, tmp_path, route):
    """test_rk_driver with TLAB_AMD_MONITORS=1 (TLab_AMD_Courant, TLab_AMD_Dilatation, MINMAX after every iteration) on the three routes of the
    Fortran host; the printed CFL# / D# / DilMin / DilMax of the last iteration against the Python driver on the fields the run wrote"""
    import torch
    from tlab_amd import io as tio
    if not os.path.exists(RK_EXE):
        pytest.skip("tlab_amd/fortran/_build_rk/test_rk_driver not built (needs oracle/_ref, i.e. the build container)")
    if not _driver_has_monitors():
        pytest.skip("tlab_amd/fortran/_build_rk/test_rk_driver is a prebuilt driver from before TLab_AMD_Monitors: rebuild it where the reference is")
    from test_gpu_fortran_dropin import run_rk_driver
    nx, ny, nz = 64, 32, 64
    x = np.arange(nx) / nx * 2.0
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    rng = np.random.default_rng(7)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wall = np.sin(np.pi * Y)
    q0 = [((np.sin(np.pi * X + k) * np.cos(2 * np.pi * Z) + 0.1 * rng.uniform(-1, 1, X.shape)) * wall).ravel() for k in range(3)]
    s0 = [(np.cos(np.pi * X) * Y + 0.1 * rng.uniform(-1, 1, X.shape)).ravel()]
    re_, sc, dt = 1000.0, 0.7, 1e-3
    bcs = ["VelocityJmin=noslip", "VelocityJmax=noslip", "Scalar1Jmin=dirichlet", "Scalar1Jmax=dirichlet"]
    env = {"TLAB_AMD_MONITORS": "1"}
    if route:
        env[route] = "1"
    q1, s1, log = run_rk_driver(str(tmp_path), x, y, z, q0, s0, re_, sc, dt, 2, bcs, env=env)
    log = open(os.path.join(str(tmp_path), "tlab.log")).read()
    lines = [l for l in log.splitlines() if "MONITORS: itime" in l]
    assert len(lines) == 2, log
    num = r"([-+0-9.Ee]+)"
    m = re.search(r"itime 2 CFL#\s+%s D#\s+%s DilMin\s+%s DilMax\s+%s at\s+(.*)$" % (num, num, num, num), lines[-1])
    assert m, lines[-1]
    cfl, dnum, dmin, dmax = (float(m.group(i)) for i in range(1, 5))
    loc = [int(v) for v in m.group(5).split()]
    mm = [float(v) for v in re.search(r"MINMAX: device host\s+(.*)$", log, re.M).group(1).split()]
    assert mm[:2] == mm[2:] == [q1[0].min(), q1[0].max()]
    from tlab_amd.dns import Dns
    d = Dns(x, y, z, nscal=1, visc=1.0 / re_, schmidt=(sc,), yuniform=False, hyper_bc1_ext=REF_HYPER)
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(q1[i]))
    (p1, p2), _ = d.TIME_COURANT(0.0, 0.0)
    assert abs(cfl - dt * p1) <= 1e-12 * abs(dt * p1) and abs(dnum - dt * p2) <= 1e-12 * abs(dt * p2), (cfl, dt * p1, dnum, dt * p2)
    rmin, rmax, lmin, lmax = d.dilatation_extremes()
    scale = max(abs(rmin), abs(rmax))
    assert abs(dmin - rmin) <= 1e-10 * scale and abs(dmax - rmax) <= 1e-10 * scale, (dmin, rmin, dmax, rmax)
    assert tuple(loc[:3]) == lmin and tuple(loc[3:]) == lmax, (loc, lmin, lmax)
