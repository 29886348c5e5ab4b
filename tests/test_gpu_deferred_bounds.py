"""The deferred tail with the host's DNS_BOUNDS_LIMIT (tlab_deferred_clip; time.f90:248-250 through tlab_amd/fortran/dns_local_device.sed): the
sequence RHS, DAXPY x (3 + ns), clips, DSCAL x (3 + ns) is ONE fused substep with those bounds; other orders run literally.  And the BLAS guard of
tlab_deferred_axpy / tlab_deferred_scal (host arrays never reach a kernel)."""
import ctypes
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KDT, KCO = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0]
LO, HI, ACTIVE = [0.1, -1.0], [0.5, 1.0], [1, 0]


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def _dns(ns=2):
    from tlab_amd.dns import Dns
    nx, ny, nz = 256, 64, 32
    x = np.arange(nx) / nx
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    return Dns(x, y, z, nscal=ns, visc=1.0 / 500.0, schmidt=(0.7, 1.3)[:ns], yuniform=False, hyper_bc1_ext=0.1)


def _fields(d, seed):
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    Y = torch.linspace(0, 1, d.ny, dtype=torch.float64, device="cuda").view(1, d.ny, 1)
    wall = torch.sin(np.pi * Y)
    return [((2 * torch.rand(d.nz, d.ny, d.nx, dtype=torch.float64, device="cuda", generator=g) - 1) * wall).reshape(-1) for _ in range(3 + d.nscal)]


def _ptrs(d):
    from tlab_amd.lib import c_vp
    mk = lambda ts: (c_vp * max(1, len(ts)))(*[t.data_ptr() for t in ts])      # noqa: E731
    return mk(d.q), mk(d.s), mk(d.hq), mk(d.hs), mk(d.txc)


def _stats(L):
    c, b = (ctypes.c_longlong * 6)(), (ctypes.c_longlong * 2)()
    assert L.tlab_deferred_stats(c) == 0 and L.tlab_deferred_clip_stats(b) == 0
    return list(c) + list(b)


def _load(d, f0):
    import torch
    for t, a in zip(d.q + d.s, f0):
        t.copy_(a)
    torch.cuda.synchronize()


def _driver_step(d, f0, dt):
    """The fused driver with its own bounds: the yardstick of the recorded sequence."""
    import torch
    _load(d, f0)
    d.set_scalar_bounds(LO, HI, ACTIVE)
    d.begin_step()
    for k in range(3):
        d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dt * KDT[k], KCO[k] if k < 2 else 1.0, k < 2)
    torch.cuda.synchronize()
    d.set_scalar_bounds(None)
    return [t.clone() for t in d.q + d.s + d.hq + d.hs]


def test_recorded_time_loop_with_clips_is_one_fused_substep_each(T):
    """time.f90 with ScalLimit = yes: zero fills, then per substep RHS, DAXPY x 5, clip of s(1), DSCAL x 5 (none after the last): three fused
    substeps that carried the bounds, nothing literal, no clip on its own, and the fields equal the driver's own bounded substeps to the bit."""
    import torch
    from tlab_amd.lib import load, check
    L = load()
    d = _dns()
    f0 = _fields(d, 5)
    ref = _driver_step(d, f0, 2e-3)
    _load(d, f0)
    q, s, hq, hs, txc = _ptrs(d)
    n = d.n
    before = _stats(L)
    check(L.tlab_deferred_enable(1), "enable")
    try:
        for t in d.hq + d.hs:
            check(L.tlab_deferred_zero(t.data_ptr(), n), "zero")
        for k in range(3):
            dte = 2e-3 * KDT[k]
            check(L.tlab_deferred_rhs(d._h, dte, q, s, hq, hs, txc), "rhs")
            for h, u in zip(d.hq + d.hs, d.q + d.s):
                check(L.tlab_deferred_axpy(n, dte, h.data_ptr(), u.data_ptr()), "axpy")
            for i, a in enumerate(ACTIVE):
                if a:
                    check(L.tlab_deferred_clip(n, LO[i], HI[i], d.s[i].data_ptr()), "clip")
            if k < 2:
                for h in d.hq + d.hs:
                    check(L.tlab_deferred_scal(n, KCO[k], h.data_ptr()), "scal")
        check(L.tlab_sync(), "sync")
    finally:
        check(L.tlab_deferred_enable(0), "disable")
    after = _stats(L)
    assert [a - b for a, b in zip(after, before)] == [3, 0, 1, 0, 0, 0, 3, 0]
    for a, b in zip(d.q + d.s + d.hq + d.hs, ref):
        assert torch.equal(a, b)
    assert float(d.s[0].min()) >= LO[0] and float(d.s[0].max()) <= HI[0] and bool((d.s[0] == HI[0]).any())


@pytest.mark.parametrize("variant", ["other array", "before its axpy", "twice", "driver bounds"])
def test_clips_that_do_not_match_run_literally_in_order(T, variant):
    """A clip of an array that is not a recorded s, a clip before the DAXPY of its field, two clips of one field, a driver with bounds of its own:
    the fields equal the same calls executed one by one with the layer off."""
    import torch
    from tlab_amd.lib import load, check
    L = load()
    d = _dns()
    f0 = _fields(d, 9)
    q, s, hq, hs, txc = _ptrs(d)
    n, dte = d.n, 1e-3
    other = torch.empty(n, dtype=torch.float64, device="cuda")

    def run(on):
        _load(d, f0)
        other.copy_(f0[0])
        for t in d.hq + d.hs:
            t.zero_()
        if variant == "driver bounds":
            d.set_scalar_bounds([-0.3, -0.2], [0.3, 0.2])
        torch.cuda.synchronize()
        check(L.tlab_deferred_enable(1 if on else 0), "enable")
        try:
            if variant == "driver bounds" and not on:       # off: the RHS entry does not clip; the driver's bounds belong to its own substep only
                d.set_scalar_bounds(None)
            check(L.tlab_deferred_rhs(d._h, dte, q, s, hq, hs, txc), "rhs")
            H, U = d.hq + d.hs, d.q + d.s
            if variant == "before its axpy":
                for h, u in list(zip(H, U))[:3]:
                    check(L.tlab_deferred_axpy(n, dte, h.data_ptr(), u.data_ptr()), "axpy")
                check(L.tlab_deferred_clip(n, 0.1, 0.5, U[3].data_ptr()), "clip")
                for h, u in list(zip(H, U))[3:]:
                    check(L.tlab_deferred_axpy(n, dte, h.data_ptr(), u.data_ptr()), "axpy")
            else:
                for h, u in zip(H, U):
                    check(L.tlab_deferred_axpy(n, dte, h.data_ptr(), u.data_ptr()), "axpy")
                if variant == "other array":
                    check(L.tlab_deferred_clip(n, 0.1, 0.5, other.data_ptr()), "clip")
                else:
                    check(L.tlab_deferred_clip(n, 0.1, 0.5, U[3].data_ptr()), "clip")
                    check(L.tlab_deferred_clip(n, 0.0, 0.2, U[4 if variant == "driver bounds" else 3].data_ptr()), "clip")
            for h in H:
                check(L.tlab_deferred_scal(n, -0.5, h.data_ptr()), "scal")
            check(L.tlab_sync(), "sync")
        finally:
            check(L.tlab_deferred_enable(0), "disable")
            d.set_scalar_bounds(None)
        return [t.clone() for t in d.q + d.s + d.hq + d.hs] + [other.clone()]
    eager = run(False)
    before = _stats(L)
    rec = run(True)
    after = _stats(L)
    assert after[7] > before[7]                     # a clip ran on its own
    if variant != "twice":                          # (twice: the record up to the first clip is complete and carries it; the second runs on its own)
        assert after[6] == before[6]
    for a, b in zip(rec, eager):
        if variant == "before its axpy":            # incomplete record: the RHS entry and the BLAS kernels themselves, to the bit
            assert torch.equal(a, b)
        else:                                       # complete up to the clip: the fused substep ran, the eager calls sum in another order
            assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)


def test_blas_guard(T):
    """Host arrays never reach a kernel: host + host DAXPY / DSCAL run on the host (even with a substep recorded), mixed pointers are refused."""
    from tlab_amd.lib import load
    L = load()
    assert hasattr(L, "tlab_pointer_on_device")          # first: on a library without the guard the host arrays below would go to a kernel
    import torch
    n = 1000
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    xd = torch.from_numpy(x).cuda()
    dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)        # noqa: E731
    assert L.tlab_pointer_on_device(dp(x)) == 0 and L.tlab_pointer_on_device(xd.data_ptr()) == 1
    assert L.tlab_pointer_on_device(xd.data_ptr() + 8 * 10) == 1        # inside a known allocation (the cached range)
    y0 = y.copy()
    assert L.tlab_deferred_axpy(n, 0.25, dp(x), dp(y)) == 0
    np.testing.assert_array_equal(y, y0 + 0.25 * x)
    assert L.tlab_deferred_scal(n, -3.0, dp(y)) == 0
    np.testing.assert_array_equal(y, (y0 + 0.25 * x) * -3.0)
    y1 = y.copy()
    assert L.tlab_deferred_axpy(n, 0.25, xd.data_ptr(), dp(y)) != 0          # mixed: refused, nothing written
    assert L.tlab_deferred_axpy(n, 0.25, dp(x), xd.data_ptr()) != 0
    np.testing.assert_array_equal(y, y1)
    # with the layer on and a substep recorded, a host BLAS call runs at once and leaves the record alone
    from tlab_amd.lib import check
    d = _dns(1)
    _load(d, _fields(d, 2))
    q, s, hq, hs, txc = _ptrs(d)
    before = _stats(L)
    check(L.tlab_deferred_enable(1), "enable")
    try:
        check(L.tlab_deferred_rhs(d._h, 1e-3, q, s, hq, hs, txc), "rhs")
        for h, u in zip(d.hq + d.hs, d.q + d.s):
            check(L.tlab_deferred_axpy(d.n, 1e-3, h.data_ptr(), u.data_ptr()), "axpy")
        assert L.tlab_deferred_axpy(n, 2.0, dp(x), dp(y)) == 0
        np.testing.assert_array_equal(y, y1 + 2.0 * x)
        check(L.tlab_sync(), "sync")
    finally:
        check(L.tlab_deferred_enable(0), "disable")
    after = _stats(L)
    assert [a - b for a, b in zip(after, before)][:2] == [1, 0]
