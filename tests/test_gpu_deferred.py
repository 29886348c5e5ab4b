"""csrc/deferred.cpp through the C ABI: the recorded tail of a Runge-Kutta substep (tlab_deferred_*; include/tlab_amd.h) -- sequences that match
time.f90's become one fused substep, everything else runs literally in the order it came, and nothing is left behind when another entry point of
the library is called."""
import ctypes
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def _dns(ns=1):
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
    c = (ctypes.c_longlong * 6)()
    assert L.tlab_deferred_stats(c) == 0
    return list(c)


KDT, KCO = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0]


def _reference_step(d, f0, dt):
    import torch
    for t, a in zip(d.q + d.s, f0):
        t.copy_(a)
    d.begin_step()
    for k in range(3):
        d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dt * KDT[k], KCO[k] if k < 2 else 1.0, k < 2)
    torch.cuda.synchronize()
    return [t.clone() for t in d.q + d.s + d.hq + d.hs]


@pytest.mark.parametrize("ns", [1, 2])
def test_recorded_time_loop_equals_the_fused_substeps_bitwise(T, ns):
    """time.f90's own sequence -- zero fills, then per substep RHS, DAXPY x (3 + ns), DSCAL x (3 + ns) (none after the last) -- recorded, then a
    tlab_sync: three fused substeps ran, no BLAS pass, the zero fills were the begin_step; state AND tendencies equal the fused driver's."""
    import torch
    from tlab_amd.lib import load, check
    L = load()
    d = _dns(ns)
    f0 = _fields(d, 5)
    ref = _reference_step(d, f0, 2e-3)
    for t, a in zip(d.q + d.s, f0):
        t.copy_(a)
    for t in d.hq + d.hs:
        t.fill_(7.0)                       # garbage the zero fills must take care of
    torch.cuda.synchronize()
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
            if k < 2:
                for h in d.hq + d.hs:
                    check(L.tlab_deferred_scal(n, KCO[k], h.data_ptr()), "scal")
        check(L.tlab_sync(), "sync")
    finally:
        check(L.tlab_deferred_enable(0), "disable")
    after = _stats(L)
    assert [a - b for a, b in zip(after, before)] == [3, 0, 1, 0, 0, 0]
    for a, b in zip(d.q + d.s + d.hq + d.hs, ref):
        assert torch.equal(a, b)


def test_sequences_that_do_not_match_run_literally_in_order(T):
    """(a) another factor in one DAXPY, (b) a DSCAL before every field was updated, (c) an operator call in the middle of the tail: each time the
    fields equal those of the same calls executed one by one with the layer off."""
    import torch
    from tlab_amd.lib import load, check
    L = load()
    d = _dns(1)
    f0 = _fields(d, 9)
    q, s, hq, hs, txc = _ptrs(d)
    n, dte = d.n, 1e-3

    def run(variant, on):
        for t, a in zip(d.q + d.s, f0):
            t.copy_(a)
        for t in d.hq + d.hs:
            t.zero_()
        torch.cuda.synchronize()
        check(L.tlab_deferred_enable(1 if on else 0), "enable")
        try:
            check(L.tlab_deferred_rhs(d._h, dte, q, s, hq, hs, txc), "rhs")
            H, U = d.hq + d.hs, d.q + d.s
            if variant == "factor":
                for i, (h, u) in enumerate(zip(H, U)):
                    check(L.tlab_deferred_axpy(n, dte * (2.0 if i == 2 else 1.0), h.data_ptr(), u.data_ptr()), "axpy")
                for h in H:
                    check(L.tlab_deferred_scal(n, -0.5, h.data_ptr()), "scal")
            elif variant == "early scal":
                for h, u in list(zip(H, U))[:2]:
                    check(L.tlab_deferred_axpy(n, dte, h.data_ptr(), u.data_ptr()), "axpy")
                check(L.tlab_deferred_scal(n, -0.5, H[0].data_ptr()), "scal")
                for h, u in list(zip(H, U))[2:]:
                    check(L.tlab_deferred_axpy(n, dte, h.data_ptr(), u.data_ptr()), "axpy")
            else:
                for h, u in list(zip(H, U))[:3]:
                    check(L.tlab_deferred_axpy(n, dte, h.data_ptr(), u.data_ptr()), "axpy")
                T.OPR_Partial_X(T.OPR_P1, d.nx, d.ny, d.nz, 0, d.g[0], d.q[0], d.txc[5][: d.n], None)       # reads u: must see it updated
                check(L.tlab_deferred_axpy(n, dte, H[3].data_ptr(), U[3].data_ptr()), "axpy")
                for h in H:
                    check(L.tlab_deferred_scal(n, -0.5, h.data_ptr()), "scal")
            check(L.tlab_sync(), "sync")
        finally:
            check(L.tlab_deferred_enable(0), "disable")
        return [t.clone() for t in d.q + d.s + d.hq + d.hs + [d.txc[5][: d.n]]]

    for variant in ("factor", "early scal", "operator in between"):
        a, b = run(variant, True), run(variant, False)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (variant, i)


def test_the_last_substep_of_a_step_waits_for_nothing(T):
    """After the last substep no DSCAL follows (time.f90:272): the description is completed by whatever comes next -- here a device-to-host copy of
    the field, which must already see the update."""
    import torch
    from tlab_amd.lib import load, check
    L = load()
    d = _dns(1)
    f0 = _fields(d, 13)
    for t, a in zip(d.q + d.s, f0):
        t.copy_(a)
    d.begin_step()
    d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(1e-3, 1.0, False)
    torch.cuda.synchronize()
    ref = d.q[1].cpu().numpy().copy()
    for t, a in zip(d.q + d.s, f0):
        t.copy_(a)
    torch.cuda.synchronize()
    q, s, hq, hs, txc = _ptrs(d)
    check(L.tlab_deferred_enable(1), "enable")
    try:
        for t in d.hq + d.hs:
            check(L.tlab_deferred_zero(t.data_ptr(), d.n), "zero")
        check(L.tlab_deferred_rhs(d._h, 1e-3, q, s, hq, hs, txc), "rhs")
        for h, u in zip(d.hq + d.hs, d.q + d.s):
            check(L.tlab_deferred_axpy(d.n, 1e-3, h.data_ptr(), u.data_ptr()), "axpy")
        out = np.empty(d.n)
        check(L.tlab_memcpy_d2h(out.ctypes.data, d.q[1].data_ptr(), d.n * 8), "d2h")
    finally:
        check(L.tlab_deferred_enable(0), "disable")
    assert np.array_equal(out, ref)


def _zone_ref(q0, s0, nx, ny, nz, pjmin, pjmax):
    """Reference fields for Dns.set_buffer_zones(ref=...), plane means of the INITIAL fields: a driver that sets its zones after a substep gets the
    tables of one that set them before it."""
    ref = {}
    for gkey, fields in (("flow", q0), ("scal", s0)):
        for key, size, offset in (("jmin", pjmin, 0), ("jmax", pjmax, ny - pjmax)):
            r = np.empty((len(fields), nz, size, nx))
            for i, a in enumerate(fields):
                r[i] = a.reshape(nz, ny, nx)[:, offset:offset + size, :].mean(axis=(0, 2))[None, :, None]
            ref[(gkey, key)] = r
    return ref


def test_replay_leaves_the_drivers_own_settings_alone(T):
    """A driver with bounds, flow and scalar zones and both body forces of its own.  Substep 1 recorded as RHS + DAXPYs + DSCALs (no sources marker, no
    relaxation; clips are not recorded for a driver with bounds): the replay is the substep WITHOUT bounds, scalar zones and forces.  Substep 2 called
    directly is the driver's own substep with all three again: fields and kernel table equal a twin's that ran substep 1 directly with the three off
    and then had them switched on -- and differ from a run of substep 2 without the forces."""
    import torch
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load, check
    from test_gpu_sources import _case, _load, _dev, _kernel_rows, COR, BOD, PJMIN, PJMAX, PU, PS, LO, HI, VISC, SC
    L = load()
    nx, ny, nz = 256, 64, 64
    x, y, z, q0, s0 = _case(nx, ny, nz)
    s0 = [np.minimum(np.maximum(a, lo), hi) for a, lo, hi in zip(s0, LO, HI)]      # (fields as a run under bounds holds them)
    ref = _zone_ref(q0, s0, nx, ny, nz, PJMIN, PJMAX)
    forces = _dev(COR, BOD(y))
    mk = lambda: Dns(x, y, z, nscal=2, visc=VISC, schmidt=SC[:2], yuniform=False)      # noqa: E731
    a, b = mk(), mk()
    for d in (a, b):
        _load(d, q0, s0)
        for t in d.hq + d.hs:
            t.fill_(7.0)                   # garbage the start of the step must take care of
    (dte1, kco1), (dte2, kco2) = [(2e-3 * a.kdt[k], a.kco[k]) for k in range(2)]

    def settings(d, bounds, scal_zones, forced):
        d.set_buffer_zones(PJMIN, PJMAX, PU, PS, ref=ref)
        if not scal_zones:
            for end in (3, 4):
                check(L.tlab_dns_set_buffer_zone(d._h, end, 1, 0, 2, None, None), "scalar zones off")
        d.set_scalar_bounds(*((LO, HI) if bounds else (None,)))
        d.set_body_forces(*(forces if forced else (None, None)))

    def profiled_substep2(d):
        L.tlab_profile_reset(); L.tlab_profile_enable(1)
        try:
            d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dte2, kco2, True)
            torch.cuda.synchronize()
        finally:
            L.tlab_profile_enable(0)
        rows = _kernel_rows()
        L.tlab_profile_reset()
        return rows, [t.clone() for t in d.q + d.s + d.hq + d.hs]

    # A: everything on; substep 1 through the record
    settings(a, True, True, True)
    q, s, hq, hs, txc = _ptrs(a)
    stats = lambda: [_stats(L)] + [list(_two(f)) for f in (L.tlab_deferred_clip_stats, L.tlab_deferred_relax_stats, L.tlab_deferred_sources_stats)]      # noqa: E731
    before = stats()
    check(L.tlab_deferred_enable(1), "enable")
    try:
        for t in a.hq + a.hs:
            check(L.tlab_deferred_zero(t.data_ptr(), a.n), "zero")
        check(L.tlab_deferred_rhs(a._h, dte1, q, s, hq, hs, txc), "rhs")
        for h, u in zip(a.hq + a.hs, a.q + a.s):
            check(L.tlab_deferred_axpy(a.n, dte1, h.data_ptr(), u.data_ptr()), "axpy")
        for h in a.hq + a.hs:
            check(L.tlab_deferred_scal(a.n, kco1, h.data_ptr()), "scal")
        check(L.tlab_sync(), "sync")
    finally:
        check(L.tlab_deferred_enable(0), "disable")
    after = stats()
    assert [v - w for v, w in zip(after[0], before[0])] == [1, 0, 1, 0, 0, 0]      # one fused substep, the zero fills its begin_step
    assert after[1:] == before[1:]                                                  # ... that carried no clip, no relaxation, no marker
    rows_a, fa = profiled_substep2(a)
    # B: substep 1 directly with the three off, then on
    settings(b, False, False, False)
    b.begin_step()
    b.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dte1, kco1, True)
    torch.cuda.synchronize()
    mid = [t.clone() for t in b.q + b.s + b.hq + b.hs]
    settings(b, True, True, True)
    rows_b, fb = profiled_substep2(b)
    for i, (u, v) in enumerate(zip(fa, fb)):
        assert torch.equal(u, v), i
    assert rows_a == rows_b, (rows_a, rows_b)
    assert rows_a.get("k_body_force") == 1 and any(k.startswith("k_buffer_relax") for k in rows_a), rows_a
    # the guard: the same substep 2 without the forces is another result
    for t, m in zip(b.q + b.s + b.hq + b.hs, mid):
        t.copy_(m)
    settings(b, True, True, False)
    rows_c, fc = profiled_substep2(b)
    assert "k_body_force" not in rows_c
    assert not any(torch.equal(u, v) for u, v in zip(fa[:3], fc[:3]))


def _two(entry):
    c = (ctypes.c_longlong * 2)()
    assert entry(c) == 0
    return c


# (the slab driver refuses slabs of 32 planes -- too thin for its partitioned z systems: its one-rank case takes a shape it runs at)
@pytest.mark.parametrize("driver,shape", [("pencil", (32, 24, 32)), ("slab", (128, 32, 64))])
def test_decomposed_replay_applies_the_recorded_clip_and_no_force(T, driver, shape):
    """One local rank of a decomposed driver with body forces and no bounds of its own: RHS + DAXPYs + one clip of the scalar + DSCALs recorded through
    tlab_deferred_pencil_rhs / _slab_rhs.  No sources marker can be recorded for these drivers, so the replay adds no force; the clip becomes the
    bounds of the one fused call: the fields equal, to the bit, the direct substep of a twin without forces whose own bounds are the clip's."""
    import torch
    from tlab_amd.lib import load, check
    L = load()
    nx, ny, nz = shape
    x = np.arange(nx) / nx * 2 * np.pi
    z = np.arange(nz) / nz * np.pi
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    rng = np.random.default_rng(5)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    f0 = [torch.from_numpy(((np.sin(X + k) * np.cos(2 * Z + k) + 0.1 * rng.uniform(-1, 1, X.shape)) * np.sin(np.pi * Y)).ravel()).cuda() for k in range(4)]
    lo, hi, dte, kco = -0.2, 0.3, 2e-3 / 3.0, -5.0 / 9.0
    assert float(f0[3].min()) < lo and float(f0[3].max()) > hi
    kw = dict(nscal=1, visc=1.0 / 700.0, schmidt=(0.5,), yuniform=False)
    cor = {"type": "normalized", "vector": (0.0, 1.5, 0.0), "parameters": (0.3, 1.0)}
    bod = {"type": "linear", "vector": (0.3, -2.0, 0.2), "scalars": 1, "parameters": (1.0, 0.1), "inb_scal_array": 1, "bbackground": 0.2 * y}

    def make():
        if driver == "pencil":
            from tlab_amd.pencil import NativePencilDns
            return NativePencilDns("loopback", 1, 1, x, y, z, **kw)
        from tlab_amd.slab import NativeSlabDns
        return NativeSlabDns("loopback", x, y, z, size=1, **kw)

    def start(m):
        S = m.st[0]
        for t, a in zip(S["q"] + S["s"], f0):
            t.copy_(a)
        for t in S["hq"] + S["hs"]:
            t.zero_()
        torch.cuda.synchronize()
        return S["q"] + S["s"], S["hq"] + S["hs"]

    a, b = make(), make()
    a.set_body_forces(cor, bod)
    b.set_scalar_bounds([lo], [hi])
    U, H = start(a)
    record = L.tlab_deferred_pencil_rhs if driver == "pencil" else L.tlab_deferred_slab_rhs
    before = _stats(L) + list(_two(L.tlab_deferred_clip_stats))
    check(L.tlab_deferred_enable(1), "enable")
    try:
        check(record(a._h, dte), "rhs")
        for h, u in zip(H, U):
            check(L.tlab_deferred_axpy(a.n, dte, h.data_ptr(), u.data_ptr()), "axpy")
        check(L.tlab_deferred_clip(a.n, lo, hi, U[3].data_ptr()), "clip")
        for h in H:
            check(L.tlab_deferred_scal(a.n, kco, h.data_ptr()), "scal")
        check(L.tlab_sync(), "sync")
    finally:
        check(L.tlab_deferred_enable(0), "disable")
    after = _stats(L) + list(_two(L.tlab_deferred_clip_stats))
    assert [v - w for v, w in zip(after, before)] == [1, 0, 0, 0, 0, 0, 1, 0]      # one fused substep that carried the clip; nothing literal
    fa = [t.clone() for t in U + H]
    V, G = start(b)
    b.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dte, kco, True)
    torch.cuda.synchronize()
    for i, (u, v) in enumerate(zip(fa, V + G)):
        assert torch.equal(u, v), i
    assert float(fa[3].min()) == lo and float(fa[3].max()) == hi                   # the clip acted
    # the guard: the forces of A are live -- its own substep from the same start is another result
    start(a)
    a.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dte, kco, True)
    torch.cuda.synchronize()
    assert not any(torch.equal(u, v) for u, v in zip(fa[:3], U[:3]))
    a.close(); b.close()
