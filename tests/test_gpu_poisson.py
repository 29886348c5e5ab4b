"""GPU parity tests of OPR_Poisson (rocFFT + per-mode ODE kernels, through the C ABI) against the numpy oracle
(itself pinned against the reference's Fortran at the per-mode level) and through the discrete identity
div(grad p) = f at BASELINE size.  Tolerance 1e-12 relative (north_star)."""
import numpy as np
import pytest
from conftest import rel_err
from scatter import scatter_of, bound, ref_build_bound, ref_build_diff

pytestmark = pytest.mark.gpu
TOL = 1e-12


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def setup(nx, ny, nz, stretch=True):
    x = np.arange(nx) / nx * 2 * np.pi
    z = np.arange(nz) / max(nz, 1) * 2 * np.pi if nz > 1 else np.zeros(1)
    if stretch:
        y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5)) * 2.0
    else:
        y = np.arange(ny) / (ny - 1.0) * 2.0
    return x, y, z


@pytest.mark.parametrize("nx,ny,nz,stretch", [(32, 40, 16, True), (16, 24, 1, True), (64, 33, 8, False), (128, 64, 32, True), (8, 9, 8, False),
                                              (32, 512, 8, True), (16, 256, 8, False), (24, 1024, 8, True), (40, 16, 8, True)])
def test_poisson_vs_oracle(T, nx, ny, nz, stretch):
    import torch
    from oracle import tlab_oracle as O, tlab_oracle_poisson as OP
    x, y, z = setup(nx, ny, nz, stretch)
    go = [O.FdmPlan(x, True, True), O.FdmPlan(y, False, not stretch), O.FdmPlan(z, True, True)]
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, not stretch), T.FdmPlan(z, True, True)]
    rng = np.random.default_rng(nx + ny + nz)
    N = nx * ny * nz
    i = np.arange(N)
    f = np.sin(0.3 * (i % nx)) * np.cos(0.07 * (i // nx)) + 0.2 * rng.uniform(-1, 1, N)
    hb = rng.uniform(-1, 1, nx * nz)
    ht = rng.uniform(-1, 1, nx * nz)
    # make the mean mode compatible (the singular problem assumes it, opr_odes.f90:176): int f dy = ht - hb for the mean
    plan_o = OP.PoissonPlan(go[0], go[1], go[2], nx, ny, nz)
    p_ref, d_ref = OP.opr_poisson_fxz(plan_o, f, hb.reshape(nz, nx), ht.reshape(nz, nx))
    plan = T.PoissonPlan(gp[0], gp[1], gp[2], nx, ny, nz)
    p = dev(f)
    t1 = torch.empty(plan.isize_txc_field, dtype=torch.float64, device="cuda")
    t2 = torch.empty_like(t1)
    dpdy = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
    T.OPR_Poisson(plan, nx, ny, nz, T.BCS_NN, p, t1, t2, dev(hb), dev(ht), dpdy)
    assert rel_err(p.cpu().numpy(), p_ref) <= TOL
    assert rel_err(dpdy.cpu().numpy(), d_ref) <= TOL
    # second call on the same plan (module state must be reusable), without dpdy
    p2 = dev(f)
    T.OPR_Poisson(plan, nx, ny, nz, T.BCS_NN, p2, t1, t2, dev(hb), dev(ht), None)
    assert rel_err(p2.cpu().numpy(), p_ref) <= TOL
    with pytest.raises(T.TlabError):        # the factorized solver has BCS_NN and BCS_DD only, like the reference (opr_elliptic.f90:312-331)
        T.OPR_Poisson(plan, nx, ny, nz, T.BCS_ND, p2, t1, t2, dev(hb), dev(ht), None)


ROUTES = {"default": {}, "fused 2-D": {"TLAB_FFTZ": "0"}, "rocFFT 1-D z": {"TLAB_FFTZ": "0", "TLAB_FFT2D": "0"}, "rocFFT forward x": {"TLAB_FFTX": "0"}}
_ROUTE_REFS = {}


def _route_case(T, op, nx, ny, nz, stretch):
    """Inputs, device-side plan arguments and the oracle's answer of one (operator, shape) of test_transform_routes_vs_oracle: computed once, shared
    by the four routes, never modified.  Returns (plans, kwargs, f, hb, ht, refs, bounds)."""
    key = (op, nx, ny, nz)
    if key in _ROUTE_REFS:
        return _ROUTE_REFS[key]
    from oracle import tlab_oracle as O, tlab_oracle_poisson as OP
    if op == "direct":      # built like tests/test_gpu_poisson_direct.py builds it
        import test_gpu_poisson_direct as D
        (ogx, ogy, ogz), gp, f, hb, ht = D._setup(T, nx, ny, nz, ny + 3)
        oplan = OP.PoissonDirectPlan(ogx, ogy, ogz, nx, ny, nz)
        (p_ref, d_ref), (_, sc_d) = scatter_of(lambda f_, hb_, ht_: OP.opr_poisson_fxz_direct(oplan, f_, hb_, ht_, 3), [f, hb, ht], nsamples=2)
        # p: the bound of the chunked kernel in test_marching_and_chunked_direct_solvers_agree; dp/dy = OPR_Partial_Y(p): max(1e-12, 2 x oracle scatter)
        out = (gp, {"gy_elliptic": gp[1]}, f, hb.ravel(), ht.ravel(), (p_ref, d_ref), (1e-12, sc_d))
    else:
        x, y, z = setup(nx, ny, nz, stretch)
        go = [O.FdmPlan(x, True, True), O.FdmPlan(y, False, not stretch), O.FdmPlan(z, True, True)]
        gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, not stretch), T.FdmPlan(z, True, True)]
        rng = np.random.default_rng(nx + ny + nz + len(op))
        N = nx * ny * nz
        i = np.arange(N)
        f = np.sin(0.3 * (i % nx)) * np.cos(0.07 * (i // nx)) + 0.2 * rng.uniform(-1, 1, N)
        hb, ht = rng.uniform(-1, 1, nx * nz), rng.uniform(-1, 1, nx * nz)
        plan_o = OP.PoissonPlan(go[0], go[1], go[2], nx, ny, nz)
        if op == "helmholtz":
            refs = (OP.opr_helmholtz_fxz_factorize(plan_o, f, hb.reshape(nz, nx), ht.reshape(nz, nx), O.BCS_NN, -7.5), None)
        else:
            refs = OP.opr_poisson_fxz(plan_o, f, hb.reshape(nz, nx), ht.reshape(nz, nx), ibc=O.BCS_NN if op == "NN" else O.BCS_DD)
        out = (gp, {}, f, hb, ht, refs, (TOL, None))
    _ROUTE_REFS[key] = out
    return out


@pytest.mark.parametrize("nx,ny,nz,stretch", [(32, 40, 16, True), (16, 33, 8, False)])      # chunked with low and four singular modes; marching
@pytest.mark.parametrize("op", ["NN", "DD", "helmholtz", "direct"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_transform_routes_vs_oracle(T, route, op, nx, ny, nz, stretch, monkeypatch):
    """Every transform route a plan can take (read at plan creation: the own z transform, the fused 2-D rocFFT plans where it is off, rocFFT's 1-D z
    transform where both are off, rocFFT's forward x) under OPR_Poisson BCS_NN / BCS_DD with dp/dy, OPR_Helmholtz BCS_NN (alpha = -7.5) and a direct
    plan's OPR_Poisson (ibc = 3, dp/dy), against the numpy oracle with the bounds of the neighbouring tests.  The other tests' nz all take the own z
    transform.  Errors of the commit before the solver's source was split: profiles/r12/poisson_split.txt."""
    import torch
    for k in ("TLAB_FFTZ", "TLAB_FFT2D", "TLAB_FFTX"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    gp, kw, f, hb, ht, (p_ref, d_ref), (tol_p, sc_d) = _route_case(T, op, nx, ny, nz, stretch)
    plan = T.PoissonPlan(gp[0], gp[1], gp[2], nx, ny, nz, **kw)
    assert bool(plan.direct) == (op == "direct")
    p = dev(f)
    t1 = torch.empty(plan.isize_txc_field, dtype=torch.float64, device="cuda")
    t2 = torch.empty_like(t1)
    dpdy = torch.full((nx * ny * nz,), float("nan"), dtype=torch.float64, device="cuda")
    if op == "helmholtz":
        T.OPR_Helmholtz(plan, nx, ny, nz, T.BCS_NN, -7.5, p, t1, t2, dev(hb), dev(ht))
    else:
        T.OPR_Poisson(plan, nx, ny, nz, {"NN": T.BCS_NN, "DD": T.BCS_DD, "direct": 3}[op], p, t1, t2, dev(hb), dev(ht), dpdy)
    ep = rel_err(p.cpu().numpy(), p_ref)
    ed = rel_err(dpdy.cpu().numpy(), d_ref) if d_ref is not None else 0.0
    print("route %-16s %-9s %2dx%2dx%2d  p %.2e  dpdy %.2e" % (route, op, nx, ny, nz, ep, ed))
    assert ep <= tol_p, ep
    assert ed <= (TOL if sc_d is None else bound(sc_d)), (ed, sc_d)


def test_chunked_and_marching_ode_kernels_agree(T, monkeypatch):
    """ny % 8 == 0 runs the register-chunked k_ode_nn; TLAB_ODE_CHUNKED=0 (read at plan creation) keeps the marching k_int1 kernels.
    Same discrete equations, same pivots: the two must agree to round-off on a large-lambda-range case."""
    import torch
    nx, ny, nz = 128, 128, 64
    x, y, z = setup(nx, ny, nz, True)
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, False), T.FdmPlan(z, True, True)]
    rng = np.random.default_rng(5)
    N = nx * ny * nz
    f, hb, ht = rng.uniform(-1, 1, N), rng.uniform(-1, 1, nx * nz), rng.uniform(-1, 1, nx * nz)
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("TLAB_ODE_CHUNKED", flag)
        plan = T.PoissonPlan(gp[0], gp[1], gp[2], nx, ny, nz)
        p = dev(f)
        t1 = torch.empty(plan.isize_txc_field, dtype=torch.float64, device="cuda"); t2 = torch.empty_like(t1)
        dpdy = torch.empty(N, dtype=torch.float64, device="cuda")
        T.OPR_Poisson(plan, nx, ny, nz, T.BCS_NN, p, t1, t2, dev(hb), dev(ht), dpdy)
        outs.append((p.cpu().numpy(), dpdy.cpu().numpy()))
    assert rel_err(outs[0][0], outs[1][0]) <= 1e-13
    assert rel_err(outs[0][1], outs[1][1]) <= 1e-13


@pytest.mark.parametrize("nx,ny,nz", [(128, 128, 64), (32, 64, 8), (48, 512, 12), (16, 24, 16)])
def test_mirror_pair_and_single_mode_ode_kernels_agree(T, nx, ny, nz, monkeypatch):
    """k_ode_nn carries the modes (kx, kz) and (kx, nz - kz) -- same lambda to the bit, hence same pivots, constants and homogeneous solutions --
    through one thread (default); TLAB_ODE_PAIR=0 at plan creation keeps one mode per thread.  Same operations per line, so the two agree to the
    last bits (the compiler may contract the two instantiations differently); BCS_NN and BCS_DD; kz = 0 and nz/2 are their own mirrors."""
    import torch
    x, y, z = setup(nx, ny, nz, True)
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, False), T.FdmPlan(z, True, True)]
    rng = np.random.default_rng(nx + nz)
    N = nx * ny * nz
    f, hb, ht = rng.uniform(-1, 1, N), rng.uniform(-1, 1, nx * nz), rng.uniform(-1, 1, nx * nz)
    outs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("TLAB_ODE_PAIR", flag)
        plan = T.PoissonPlan(gp[0], gp[1], gp[2], nx, ny, nz)
        t1 = torch.empty(plan.isize_txc_field, dtype=torch.float64, device="cuda"); t2 = torch.empty_like(t1)
        for ibc in (T.BCS_NN, T.BCS_DD):
            p = dev(f)
            dpdy = torch.empty(N, dtype=torch.float64, device="cuda")
            T.OPR_Poisson(plan, nx, ny, nz, ibc, p, t1, t2, dev(hb), dev(ht), dpdy)
            outs[flag, ibc] = (p.cpu().numpy(), dpdy.cpu().numpy())
    for ibc in (T.BCS_NN, T.BCS_DD):
        for k in range(2):
            assert np.isfinite(outs["1", ibc][k]).all() and np.abs(outs["1", ibc][k]).max() > 0.0
            assert rel_err(outs["1", ibc][k], outs["0", ibc][k]) <= 1e-14, (ibc, k)


@pytest.mark.parametrize("nz", [16, 32, 64, 128, 256, 512, 1024, 2048])
def test_own_z_fft_matches_numpy(T, nz):
    """k_fftz (strided Stockham, fftz.hip) against numpy on the kx-pencil layout (nxl, ny, nz); lengths 8^a * {1,2,4}."""
    import ctypes
    import torch
    from tlab_amd.lib import load, check, c_vp
    nx, ny, kmax, nxl, ioff = 16, 16, nz // 2, 5, 2
    x, y, z = np.arange(nx) / nx, np.arange(ny) / (ny - 1.0), np.arange(nz) / nz
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, True), T.FdmPlan(z, True, True)]
    h = c_vp(0)
    L = load()
    check(L.tlab_poisson_plan_create_pencil(ctypes.byref(h), gp[0]._h, gp[1]._h, gp[2]._h, nx, ny, kmax, nz, ioff, nxl), "pencil plan")
    rng = np.random.default_rng(nz)
    a = rng.uniform(-1, 1, (nz, ny, nxl)) + 1j * rng.uniform(-1, 1, (nz, ny, nxl))
    da = torch.from_numpy(np.ascontiguousarray(a).view(np.float64).reshape(-1)).cuda()
    db = torch.empty_like(da)
    check(L.tlab_poisson_fft_z(h, 1, da.data_ptr(), db.data_ptr()), "fft_z")
    fwd = db.cpu().numpy().view(np.complex128).reshape(nz, ny, nxl)
    ref = np.fft.fft(a, axis=0)
    assert np.abs(fwd - ref).max() <= 1e-13 * np.abs(ref).max()
    check(L.tlab_poisson_fft_z(h, -1, db.data_ptr(), da.data_ptr()), "fft_z")           # unnormalised inverse, like FFTW / rocFFT
    back = da.cpu().numpy().view(np.complex128).reshape(nz, ny, nxl)
    assert np.abs(back - nz * a).max() <= 1e-13 * nz * np.abs(a).max()
    check(L.tlab_poisson_plan_destroy(h), "destroy")


@pytest.mark.parametrize("nx", [64, 128, 256, 512, 1024, 2048])
def test_x_fft_matches_numpy(T, nx):
    """OPR_Fourier_X_Forward / _Backward through the C ABI against numpy.fft.rfft: the one-pass k_fftx_r2c (fftz.hip; nx/2 = 8^a * {1,2,4} from 128
    points on) and rocFFT for the other lengths (64 here) and for the inverse; 11 lines (a 2-D box) leave the last workgroup partly empty."""
    import torch
    from tlab_amd.lib import load, check
    ny, nz = 11, 1
    x, y, z = np.arange(nx) / nx, np.arange(ny) / (ny - 1.0), np.zeros(1)
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, True), T.FdmPlan(z, True, True)]
    plan = T.PoissonPlan(gp[0], gp[1], gp[2], nx, ny, nz)
    rng = np.random.default_rng(nx)
    a = rng.uniform(-1, 1, (nz, ny, nx))
    da = torch.from_numpy(a.reshape(-1)).cuda()
    db = torch.full((nz * ny * (nx // 2 + 1) * 2 + 8,), np.nan, dtype=torch.float64, device="cuda")
    L = load()
    check(L.tlab_poisson_fft_x(plan._h, 1, da.data_ptr(), db.data_ptr()), "fft_x")
    out = db.cpu().numpy()
    assert np.isnan(out[-8:]).all()            # nothing written past the last line
    fwd = out[:-8].view(np.complex128).reshape(nz, ny, nx // 2 + 1)
    ref = np.fft.rfft(a, axis=2)
    assert np.abs(fwd - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.abs(fwd[..., 0].imag).max() == 0.0 and np.abs(fwd[..., -1].imag).max() == 0.0      # the two real modes, like FFTW's r2c
    dc = torch.empty_like(da)
    check(L.tlab_poisson_fft_x(plan._h, -1, db.data_ptr(), dc.data_ptr()), "fft_x")
    assert np.abs(dc.cpu().numpy().reshape(a.shape) - nx * a).max() <= 1e-13 * nx
    if nx >= 128:      # the library's own inverse (k_fftx_c2r: the kernel that finishes the v equation inside OPR_Poisson), on a spectrum of its own
        spec = rng.uniform(-1, 1, (nz, ny, nx // 2 + 1)) + 1j * rng.uniform(-1, 1, (nz, ny, nx // 2 + 1))
        dsp = torch.from_numpy(np.ascontiguousarray(spec).view(np.float64).reshape(-1)).cuda()
        dd = torch.full((nz * ny * nx + 8,), np.nan, dtype=torch.float64, device="cuda")
        check(L.tlab_poisson_fft_x(plan._h, -2, dsp.data_ptr(), dd.data_ptr()), "fft_x own inverse")
        got = dd.cpu().numpy()
        assert np.isnan(got[-8:]).all()
        ref = np.fft.irfft(spec, n=nx, axis=2) * nx           # imaginary parts of the two real modes ignored, like FFTW's c2r
        assert np.abs(got[:-8].reshape(ref.shape) - ref).max() <= 1e-13 * np.abs(ref).max()


@pytest.mark.parametrize("nx,P", [(128, 2), (256, 3), (512, 8)])
def test_packed_x_transforms_equal_transform_plus_repack(T, nx, P):
    """tlab_poisson_fft_x_packed / _packed_final (the repack of the slab <-> kx-pencil exchange folded into the own x-transforms, the native slab
    driver's default route) through the C ABI: the forward transform into the pack buffer is BIT-identical to tlab_poisson_fft_x followed by
    tlab_pencil_repack_blocks (same kernel arithmetic, other store addresses); the inverse from the pack buffer is bit-identical to the own inverse
    (dir = -2) of the unpacked spectrum; the final form equals k_final_update's arithmetic on that inverse.  Two halves per rank, uneven kx ranges."""
    import ctypes
    import torch
    from tlab_amd.lib import load, check
    from tlab_amd.parallel import pencil_stage_layout
    ny, kmax = 9, 4
    nzt = kmax * P
    nxh = nx // 2 + 1
    x, y, z = np.arange(nx) / nx, np.arange(ny) / (ny - 1.0), np.arange(nzt) / nzt
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, True), T.FdmPlan(z, True, True)]
    L = load()
    h = ctypes.c_void_p(0)
    base_, rem = nxh // P, nxh % P
    nxl = [base_ + (1 if r < rem else 0) for r in range(P)]
    ioff = [r * base_ + min(r, rem) for r in range(P)]
    check(L.tlab_poisson_plan_create_pencil(ctypes.byref(h), gp[0]._h, gp[1]._h, gp[2]._h, nx, ny, kmax, nzt, ioff[0], nxl[0]), "pencil plan")
    start, base, split, nxa, nxb = pencil_stage_layout(ioff, nxl, ny, kmax)
    nb = len(start)
    st = (ctypes.c_int * nb)(*start)
    bs = (ctypes.c_longlong * nb)(*base)
    rng = np.random.default_rng(nx + P)
    a = torch.from_numpy(rng.uniform(-1, 1, kmax * ny * nx)).cuda()
    nc = 2 * nxh * ny * kmax
    spec = torch.full((nc,), np.nan, dtype=torch.float64, device="cuda")
    pack_ref = torch.full((nc,), np.nan, dtype=torch.float64, device="cuda")
    pack = torch.full((nc + 8,), np.nan, dtype=torch.float64, device="cuda")
    check(L.tlab_poisson_fft_x(h, 1, a.data_ptr(), spec.data_ptr()), "fft_x")
    check(L.tlab_pencil_repack_blocks(spec.data_ptr(), pack_ref.data_ptr(), nxh, ny, kmax, nb, st, bs, 1), "repack")
    check(L.tlab_poisson_fft_x_packed(h, 1, a.data_ptr(), pack.data_ptr(), nb, st, bs), "fft_x_packed")
    assert bool(torch.isnan(pack[-8:]).all()) and torch.equal(pack[:-8], pack_ref) and not bool(torch.isnan(pack_ref).any())
    # inverse: a spectrum of its own in the pack layout
    sp = torch.from_numpy(rng.uniform(-1, 1, nc)).cuda()
    unp = torch.empty_like(sp)
    check(L.tlab_pencil_repack_blocks(unp.data_ptr(), sp.data_ptr(), nxh, ny, kmax, nb, st, bs, -1), "repack back")
    r_ref = torch.empty(kmax * ny * nx, dtype=torch.float64, device="cuda")
    r_got = torch.full((kmax * ny * nx + 8,), np.nan, dtype=torch.float64, device="cuda")
    check(L.tlab_poisson_fft_x(h, -2, unp.data_ptr(), r_ref.data_ptr()), "own inverse")
    check(L.tlab_poisson_fft_x_packed(h, -1, sp.data_ptr(), r_got.data_ptr(), nb, st, bs), "packed inverse")
    assert bool(torch.isnan(r_got[-8:]).all()) and torch.equal(r_got[:-8], r_ref)
    # final form: h = h - g, wall planes zero, q += dte h, h *= kco
    q = torch.from_numpy(rng.uniform(-1, 1, kmax * ny * nx)).cuda()
    hh = torch.from_numpy(rng.uniform(-1, 1, kmax * ny * nx)).cuda()
    q2, h2 = q.clone(), hh.clone()
    dte, kco = 3e-3, -0.6
    check(L.tlab_pw_final_update(q2.data_ptr(), h2.data_ptr(), r_ref.data_ptr(), None, None, dte, kco, 1, nx, ny, kmax), "final_update")
    check(L.tlab_poisson_fft_x_packed_final(h, sp.data_ptr(), q.data_ptr(), hh.data_ptr(), dte, kco, 1, nb, st, bs), "packed final")
    assert float((q - q2).abs().max()) <= 1e-15 * float(q2.abs().max()) and float((hh - h2).abs().max()) <= 1e-15 * float(h2.abs().max())
    assert float(hh.view(kmax, ny, nx)[:, 0].abs().max()) == 0.0 and float(hh.view(kmax, ny, nx)[:, -1].abs().max()) == 0.0
    # refusals: a block map that does not start at kx = 0, in place
    bad = (ctypes.c_int * nb)(*([1] + list(start[1:])))
    assert L.tlab_poisson_fft_x_packed(h, 1, a.data_ptr(), pack.data_ptr(), nb, bad, bs) != 0
    assert L.tlab_poisson_fft_x_packed(h, 1, a.data_ptr(), a.data_ptr(), nb, st, bs) != 0
    check(L.tlab_poisson_plan_destroy(h), "destroy")


@pytest.mark.parametrize("n", [256])
def test_poisson_full_size_identity(T, n):
    """256^3: div(grad p) = f with the device operators (vpoisson.f90 / SURVEY 4.4 construction), dpdy = d/dy of phi."""
    import torch
    nx = ny = nz = n
    x, y, z = setup(nx, ny, nz, True)
    gx, gy, gz = T.FdmPlan(x, True, True), T.FdmPlan(y, False, False), T.FdmPlan(z, True, True)
    N = n ** 3
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    X = torch.from_numpy(x).cuda().view(1, 1, nx); Y = torch.from_numpy(y).cuda().view(1, ny, 1); Z = torch.from_numpy(z).cuda().view(nz, 1, 1)
    phi = (torch.sin(X) * torch.cos(2 * Z) * torch.exp(0.5 * Y) + torch.cos(3 * X + 1) * Y ** 2 + 0.3 * torch.sin(2 * Z) * torch.cos(2 * Y)).contiguous().view(-1)
    phi = phi + 0.01 * (torch.rand(N, dtype=torch.float64, device="cuda", generator=gen) - 0.5)
    a, b, dphidy, f = (torch.empty_like(phi) for _ in range(4))
    T.OPR_Partial_Y(T.OPR_P1, nx, ny, nz, 0, gy, phi, dphidy)
    T.OPR_Partial_Y(T.OPR_P1, nx, ny, nz, 0, gy, dphidy, f)
    T.OPR_Partial_X(T.OPR_P1, nx, ny, nz, 0, gx, phi, a); T.OPR_Partial_X(T.OPR_P1, nx, ny, nz, 0, gx, a, b); f += b
    T.OPR_Partial_Z(T.OPR_P1, nx, ny, nz, 0, gz, phi, a); T.OPR_Partial_Z(T.OPR_P1, nx, ny, nz, 0, gz, a, b); f += b
    d3 = dphidy.view(nz, ny, nx)
    hb, ht = d3[:, 0, :].contiguous().view(-1), d3[:, ny - 1, :].contiguous().view(-1)
    plan = T.PoissonPlan(gx, gy, gz, nx, ny, nz)
    t1 = torch.empty(plan.isize_txc_field, dtype=torch.float64, device="cuda"); t2 = torch.empty_like(t1)
    p = f.clone(); dpdy = torch.empty_like(p)
    T.OPR_Poisson(plan, nx, ny, nz, T.BCS_NN, p, t1, t2, hb, ht, dpdy)
    assert float((dpdy - dphidy).abs().max() / dphidy.abs().max()) <= 1e-11
    res = torch.empty_like(p)
    T.OPR_Partial_Y(T.OPR_P1, nx, ny, nz, 0, gy, dpdy, res)
    T.OPR_Partial_X(T.OPR_P1, nx, ny, nz, 0, gx, p, a); T.OPR_Partial_X(T.OPR_P1, nx, ny, nz, 0, gx, a, b); res += b
    T.OPR_Partial_Z(T.OPR_P1, nx, ny, nz, 0, gz, p, a); T.OPR_Partial_Z(T.OPR_P1, nx, ny, nz, 0, gz, a, b); res += b
    assert float((res - f).abs().max() / f.abs().max()) <= 1e-11


def test_projection_forcing_within_the_oracles_own_scatter(T):
    """The forcing of the pressure equation in the first substep of a non-solenoidal field, div(hq + q/dte) ~ 3e4 for a pressure of 4e2 on
    512-point lines: the solve amplifies rounding.  How much is MEASURED here on the oracle (OPR_ODE2_Factorize_NN per mode, pinned bitwise
    against oracle/_ref): the forcing and the wall data are moved by one ulp of white noise and the oracle's own p and dp/dy scatter is
    recorded (tests/scatter.py).  The default solver (k_ode_nn + the modes with lambda h^2 << 1 through the marching sub-plan) and the exact
    mode (tlab_poisson_set_exact: marching kernels, the reference's operations one by one) must stay within max(1e-12, 2 x scatter) of the
    oracle.  The chunked kernel alone (TLAB_POISSON_LOW_MODES=0, a diagnostic switch, not a product path and not a parity claim) is printed; it
    sits at what two builds of the reference differ by (with / without fused multiply-adds, ~9 x the scatter) and is only sanity-checked."""
    import os
    import torch
    import test_gpu_rhs as M
    from oracle import tlab_oracle as O, tlab_oracle_poisson as OP
    from oracle.tlab_oracle_rhs import DnsOracle
    import oracle.tlab_oracle_rhs as R
    nx, ny, nz = 64, 512, 16
    x, y, z = M.grids(nx, ny, nz, False)
    q0, s0 = M.init_fields(nx, ny, nz, x, y, z, 23, noise=1e-3)
    o = DnsOracle(x, y, z, nscal=1, visc=1.0 / 5000.0, schmidt=(0.7,), yuniform=True)
    for i in range(3):
        o.q[i] = q0[i].copy()
    o.s[0] = s0[0].copy()
    cap = {}
    orig = R.OP.opr_poisson_fxz

    def spy(plan, f, hb, ht, *a, **k):
        cap["f"], cap["hb"], cap["ht"] = f.copy(), hb.copy(), ht.copy()
        return orig(plan, f, hb, ht, *a, **k)
    R.OP.opr_poisson_fxz = spy
    try:
        o.rhs_global_incompressible_1(1e-3 / 3)
    finally:
        R.OP.opr_poisson_fxz = orig
    (p_ref, dp_ref), (sc_p, sc_dp) = scatter_of(lambda f, hb, ht: orig(o.poisson, f, hb, ht), [cap["f"], cap["hb"], cap["ht"]], nsamples=3)
    print("oracle one-ulp scatter: p %.1e dpdy %.1e (forcing %.1e, pressure %.1e)" % (sc_p, sc_dp, np.abs(cap["f"]).max(), np.abs(p_ref).max()))
    assert sc_p < 1e-10 and sc_dp < 1e-10              # the oracle itself is healthy
    g = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, True), T.FdmPlan(z, True, True)]
    err = {}
    for mode in ("default", "chunked only", "exact"):
        T.poisson_set_exact(mode == "exact")
        if mode == "chunked only":
            os.environ["TLAB_POISSON_LOW_MODES"] = "0"
        try:
            plan = T.PoissonPlan(g[0], g[1], g[2], nx, ny, nz)
        finally:
            T.poisson_set_exact(False)
            os.environ.pop("TLAB_POISSON_LOW_MODES", None)
        p = torch.from_numpy(cap["f"].copy()).cuda()
        t1 = torch.zeros(plan.isize_txc_field, dtype=torch.float64, device="cuda"); t2 = torch.zeros_like(t1); dp = torch.zeros_like(p)
        T.OPR_Poisson(plan, nx, ny, nz, T.BCS_NN, p, t1, t2, torch.from_numpy(cap["hb"].ravel().copy()).cuda(),
                      torch.from_numpy(cap["ht"].ravel().copy()).cuda(), dp)
        err[mode] = (rel_err(p.cpu().numpy(), p_ref), rel_err(dp.cpu().numpy(), dp_ref))
    print("projection forcing: " + " | ".join("%s p %.1e dpdy %.1e" % ((m,) + e) for m, e in err.items()))
    # The exact mode repeats the reference's operations one by one, but its transforms are rocFFT's, not numpy's: measured 1.5 x the 3-sample scatter
    # in dp/dy (3.08e-12 against 2.04e-12; p at the floor) -- 1 x does not hold for it, the table of profiles/r03/parity_table.json carries the numbers.
    rp = (ref_build_diff("poisson_first_p"), "ref_fma_scatter.npz:poisson_first_p")          # the reference against itself on this very forcing, recorded next to
    rd = (ref_build_diff("poisson_first_dpdy"), "ref_fma_scatter.npz:poisson_first_dpdy")    # every comparison below (and asserted as a bound further down)
    for mode, factor in (("default", 2.0), ("exact", 1.6)):
        assert float(err[mode][0]) <= bound(sc_p, factor, ref=rp) and float(err[mode][1]) <= bound(sc_dp, factor, ref=rd), (mode, err, sc_p, sc_dp)
    assert float(err["chunked only"][0]) <= bound(sc_p, 16.0, ref=rp) and float(err["chunked only"][1]) <= bound(sc_dp, 16.0, ref=rd), (err, sc_p, sc_dp)     # sanity only
    # ... and against a yardstick that does not come from this repository's oracle: the SAME per-mode stage in two builds of the reference itself (amdflang
    # -O2 with and without fused multiply-adds; tests/golden/ref_fma_scatter.npz, case poisson_first = this very forcing).  Both product modes must differ
    # from the oracle by no more than the reference differs from itself (p 1.1e-12, dp/dy 4.4e-12).
    for mode in ("default", "exact"):
        assert float(err[mode][0]) <= ref_build_bound("poisson_first_p") and float(err[mode][1]) <= ref_build_bound("poisson_first_dpdy"), (mode, err)


@pytest.mark.parametrize("nx,ny,nz,stretch", [(32, 40, 16, True), (16, 24, 1, True), (64, 33, 8, False), (128, 64, 32, True),
                                              (32, 512, 8, True), (16, 256, 8, False)])
def test_poisson_dirichlet_vs_oracle(T, nx, ny, nz, stretch):
    """ibc = BCS_DD of the factorized solver (OPR_ODE2_Factorize_DD / _DD_Sing per mode, opr_elliptic.f90:322-329): bcs_hb, bcs_ht are the
    wall VALUES of p.  Chunked plans (ny % 8 == 0) take k_ode_nn<DD> with the singular and the lowest modes marched beside it, the marching plan
    (ny = 33) the marching kernels for every mode; test_poisson_dirichlet_marching_route_on_chunked_plans keeps the old route of chunked plans covered."""
    import torch
    from oracle import tlab_oracle as O, tlab_oracle_poisson as OP
    x, y, z = setup(nx, ny, nz, stretch)
    go = [O.FdmPlan(x, True, True), O.FdmPlan(y, False, not stretch), O.FdmPlan(z, True, True)]
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, not stretch), T.FdmPlan(z, True, True)]
    rng = np.random.default_rng(nx + ny + nz + 1)
    N = nx * ny * nz
    i = np.arange(N)
    f = np.sin(0.3 * (i % nx)) * np.cos(0.07 * (i // nx)) + 0.2 * rng.uniform(-1, 1, N)
    hb = rng.uniform(-1, 1, nx * nz)
    ht = rng.uniform(-1, 1, nx * nz)
    plan_o = OP.PoissonPlan(go[0], go[1], go[2], nx, ny, nz)
    (p_ref, d_ref), (sc_p, sc_d) = scatter_of(lambda f_, hb_, ht_: OP.opr_poisson_fxz(plan_o, f_, hb_, ht_, ibc=O.BCS_DD),
                                              [f, hb.reshape(nz, nx), ht.reshape(nz, nx)], nsamples=2)
    plan = T.PoissonPlan(gp[0], gp[1], gp[2], nx, ny, nz)
    t1 = torch.empty(plan.isize_txc_field, dtype=torch.float64, device="cuda")
    t2 = torch.empty_like(t1)
    for rep in range(2):          # twice: the second call finds the lazily built pieces in place; and an NN solve in between still works
        p = dev(f)
        dpdy = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        T.OPR_Poisson(plan, nx, ny, nz, T.BCS_DD, p, t1, t2, dev(hb), dev(ht), dpdy)
        assert rel_err(p.cpu().numpy(), p_ref) <= bound(sc_p), (rel_err(p.cpu().numpy(), p_ref), sc_p)
        assert rel_err(dpdy.cpu().numpy(), d_ref) <= bound(sc_d), (rel_err(dpdy.cpu().numpy(), d_ref), sc_d)      # max(1e-12, 2 x oracle scatter)
        p3 = p.view(nz, ny, nx)
        assert float((p3[:, 0, :].reshape(-1) - dev(hb)).abs().max()) <= 1e-13 and float((p3[:, ny - 1, :].reshape(-1) - dev(ht)).abs().max()) <= 1e-13
        if rep == 0:
            q = dev(f)
            T.OPR_Poisson(plan, nx, ny, nz, T.BCS_NN, q, t1, t2, dev(hb), dev(ht), dpdy)
            qn, _ = OP.opr_poisson_fxz(plan_o, f, hb.reshape(nz, nx), ht.reshape(nz, nx))
            assert rel_err(q.cpu().numpy(), qn) <= TOL


@pytest.mark.parametrize("n", [40, 129])
@pytest.mark.parametrize("scheme1", [5, 4])
def test_device_int1_solve_with_3_and_7_diagonals_is_bitwise_the_oracle(T, scheme1, n):
    """One FDM_Int1_Solve per mode on the device (k_int1g: MatMul_3d / MatMul_5d, TRIDSS / HEPTADSS on host-made factors, free-end value and
    derivative at the given end) against the oracle, which is bitwise the reference for these widths: equal to the last bit, 305 constants."""
    import ctypes
    from tlab_amd.lib import load, check
    from oracle import tlab_oracle as O, tlab_oracle_poisson as OP
    L = load()
    dp = ctypes.POINTER(ctypes.c_double)
    y = 0.5 * (1 + np.tanh(2 * (2 * np.arange(n) / (n - 1) - 1)) / np.tanh(2))
    gp, op = T.FdmPlan(y, False, False, scheme1, 7), O.FdmPlan(y, False, False, scheme1, 7)
    lam = np.concatenate([[0.0, 1.2246467991473532e-16, 0.5, 6.28, 97.0, 1500.0], np.linspace(0.1, 900, 299)])
    nm = len(lam)
    rng = np.random.default_rng(n + scheme1)
    def solve(ibc, variant, ls, f, bv):
        res, du = np.zeros((2, n, nm)), np.zeros((2, nm))
        check(L.tlab_debug_int1_solve(gp._h, ibc, variant, nm, ls.ctypes.data_as(dp), f.ctypes.data_as(dp), bv.ctypes.data_as(dp),
                                      res.ctypes.data_as(dp), du.ctypes.data_as(dp)), "tlab_debug_int1_solve")
        return res.transpose(1, 0, 2), du

    for ibc, sgn in ((1, 1.0), (2, -1.0)):
        ls = np.ascontiguousarray(sgn * lam)
        p = OP.int1_initialize(op.der1, ls, ibc)
        # variant 0: two given lines with given boundary values
        f, bv = rng.uniform(-1, 1, (2, n, nm)), rng.uniform(-1, 1, (2, nm))
        res, du = solve(ibc, 0, ls, f, bv)
        ro = np.zeros((n, 2, nm))
        ro[0 if ibc == 1 else n - 1] = bv
        duo = OP.int1_solve(p, p.rhs, f.transpose(1, 0, 2).copy(), ro, want_du=True)
        assert np.array_equal(res, ro) and np.array_equal(du, duo), (scheme1, n, ibc, "given lines")
        # variant 1: the unit forcings of the homogeneous solutions (opr_odes.f90:308-318)
        res, du = solve(ibc, 1, ls, f, bv)
        fo, ro = np.zeros((n, 2, nm)), np.zeros((n, 2, nm))
        fo[n - 1 if ibc == 1 else 0, 0] = 1.0
        ro[0 if ibc == 1 else n - 1, 1] = 1.0
        duo = OP.int1_solve(p, p.rhs, fo, ro, want_du=True)
        assert np.array_equal(res, ro) and np.array_equal(du, duo), (scheme1, n, ibc, "unit forcing")
        if ibc == 2:      # variant 2: three lines (u1, s+, e+ of OPR_ODE2_Factorize_NN: two forced lines and the free one with value 1 at the top)
            res, du = solve(2, 2, ls, f, bv)
            fo, ro = np.zeros((n, 3, nm)), np.zeros((n, 3, nm))
            fo[:, 0:2] = f.transpose(1, 0, 2)
            ro[n - 1, 2] = 1.0
            duo = OP.int1_solve(p, p.rhs, fo, ro, want_du=True)
            assert np.array_equal(res, ro[:, 1:3]) and np.array_equal(du, duo[1:3]), (scheme1, n, "three lines")


@pytest.mark.parametrize("ibc", ["NN", "DD"])
@pytest.mark.parametrize("scheme1,nx,ny,nz", [(5, 32, 40, 16), (5, 16, 128, 8), (4, 32, 36, 16), (4, 16, 24, 1)])
def test_poisson_with_3_and_7_diagonal_integral_systems(T, scheme1, nx, ny, nz, ibc):
    """The factorized solver on a y plan whose first derivative is CompactJacobian6Penta (5: heptadiagonal integral systems, HEPTADFS / HEPTADSS,
    MatMul_5d) or CompactJacobian4 (4: tridiagonal ones, TRIDFS / TRIDSS) -- fdm_integral.f90:75-83, 249-263.  The systems are factorized on the
    host (tlab_amd/csrc/int1_generic.cpp; bitwise equal to the oracle's, tests/test_capi_host.py), k_int1g substitutes; against the oracle, whose
    FDM_Int1 for these widths is bitwise equal to the reference's (tests/golden/poisson_modes_penta_*, _jacobian4_*)."""
    import torch
    from oracle import tlab_oracle as O, tlab_oracle_poisson as OP
    x, y, z = setup(nx, ny, nz, True)
    go = [O.FdmPlan(x, True, True), O.FdmPlan(y, False, False, scheme1, 7), O.FdmPlan(z, True, True)]
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, False, scheme1, 7), T.FdmPlan(z, True, True)]
    rng = np.random.default_rng(nx + ny + nz + scheme1)
    N = nx * ny * nz
    i = np.arange(N)
    f = np.sin(0.3 * (i % nx)) * np.cos(0.07 * (i // nx)) + 0.2 * rng.uniform(-1, 1, N)
    hb, ht = rng.uniform(-1, 1, nx * nz), rng.uniform(-1, 1, nx * nz)
    code = O.BCS_NN if ibc == "NN" else O.BCS_DD
    plan_o = OP.PoissonPlan(go[0], go[1], go[2], nx, ny, nz)
    (p_ref, d_ref), (sc_p, sc_d) = scatter_of(lambda f_, hb_, ht_: OP.opr_poisson_fxz(plan_o, f_, hb_, ht_, ibc=code),
                                              [f, hb.reshape(nz, nx), ht.reshape(nz, nx)], nsamples=2)
    plan = T.PoissonPlan(gp[0], gp[1], gp[2], nx, ny, nz)
    t1 = torch.empty(plan.isize_txc_field, dtype=torch.float64, device="cuda")
    t2 = torch.empty_like(t1)
    for rep in range(2):
        p = dev(f)
        dpdy = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        T.OPR_Poisson(plan, nx, ny, nz, T.BCS_NN if ibc == "NN" else T.BCS_DD, p, t1, t2, dev(hb), dev(ht), dpdy)
        ep, ed = rel_err(p.cpu().numpy(), p_ref), rel_err(dpdy.cpu().numpy(), d_ref)
        assert ep <= bound(sc_p) and ed <= bound(sc_d), (scheme1, ibc, ep, sc_p, ed, sc_d)


def test_poisson_dirichlet_marching_route_on_chunked_plans(T):
    """TLAB_ODE_DD_CHUNKED=0: a chunked plan marches every mode for BCS_DD (the route before k_ode_nn<DD>); both routes of the same plan agree
    with each other far inside the oracle's scatter."""
    import os
    import torch
    nx, ny, nz = 32, 64, 16
    x, y, z = setup(nx, ny, nz, True)
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, False), T.FdmPlan(z, True, True)]
    plan = T.PoissonPlan(gp[0], gp[1], gp[2], nx, ny, nz)
    rng = np.random.default_rng(5)
    f, hb, ht = rng.uniform(-1, 1, nx * ny * nz), rng.uniform(-1, 1, nx * nz), rng.uniform(-1, 1, nx * nz)
    t1 = torch.empty(plan.isize_txc_field, dtype=torch.float64, device="cuda"); t2 = torch.empty_like(t1)
    out = {}
    try:
        for route in ("1", "0"):
            os.environ["TLAB_ODE_DD_CHUNKED"] = route
            p, dpdy = dev(f), torch.empty(nx * ny * nz, dtype=torch.float64, device="cuda")
            T.OPR_Poisson(plan, nx, ny, nz, T.BCS_DD, p, t1, t2, dev(hb), dev(ht), dpdy)
            out[route] = (p.cpu().numpy(), dpdy.cpu().numpy())
    finally:
        os.environ.pop("TLAB_ODE_DD_CHUNKED", None)
    assert rel_err(out["1"][0], out["0"][0]) <= 1e-12 and rel_err(out["1"][1], out["0"][1]) <= 1e-12
    assert not np.array_equal(out["1"][0], out["0"][0])          # (two different kernels did run)


@pytest.mark.parametrize("nx,ny,nz,stretch,ibc,alphas", [
    (32, 40, 16, True, 3, (-7.5,)), (16, 24, 1, True, 0, (-120.0,)), (64, 33, 8, False, 3, (-2.0e3,)), (128, 64, 32, True, 0, (-0.5, -40.0)),
    (32, 512, 8, True, 3, (-1.0e4, -3.0)), (16, 256, 8, False, 3, (-1.0, -2.0, -3.0, -4.0, -5.0, -1.0))])
@pytest.mark.gpu
def test_factorized_helmholtz_vs_oracle(T, nx, ny, nz, stretch, ibc, alphas):
    """OPR_Helmholtz_FourierXZ_Factorize (opr_elliptic.f90:466-557) on the plan of OPR_Poisson: per mode OPR_ODE2_Factorize_NN / _DD with
    sqrt(lambda - alpha).  Chunked (ny % 8 == 0) and marching (ny = 33) plans; the last case walks through more alphas than the plan keeps
    tables for and comes back to the first; a Poisson solve on the same plan afterwards is untouched."""
    import torch
    from oracle import tlab_oracle as O, tlab_oracle_poisson as OP
    x, y, z = setup(nx, ny, nz, stretch)
    go = [O.FdmPlan(x, True, True), O.FdmPlan(y, False, not stretch), O.FdmPlan(z, True, True)]
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, not stretch), T.FdmPlan(z, True, True)]
    rng = np.random.default_rng(nx + ny + nz + ibc)
    N = nx * ny * nz
    i = np.arange(N)
    f = np.sin(0.3 * (i % nx)) * np.cos(0.07 * (i // nx)) + 0.2 * rng.uniform(-1, 1, N)
    hb = rng.uniform(-1, 1, nx * nz)
    ht = rng.uniform(-1, 1, nx * nz)
    plan_o = OP.PoissonPlan(go[0], go[1], go[2], nx, ny, nz)
    plan = T.PoissonPlan(gp[0], gp[1], gp[2], nx, ny, nz)
    t1 = torch.empty(plan.isize_txc_field, dtype=torch.float64, device="cuda")
    t2 = torch.empty_like(t1)
    refs = {}
    for alpha in alphas:
        if alpha not in refs:
            refs[alpha] = OP.opr_helmholtz_fxz_factorize(plan_o, f, hb.reshape(nz, nx), ht.reshape(nz, nx), ibc, alpha)
        a = dev(f)
        T.OPR_Helmholtz(plan, nx, ny, nz, ibc, alpha, a, t1, t2, dev(hb), dev(ht))
        assert rel_err(a.cpu().numpy(), refs[alpha]) <= TOL, (alpha, rel_err(a.cpu().numpy(), refs[alpha]))
    p = dev(f)
    dpdy = torch.empty(N, dtype=torch.float64, device="cuda")
    T.OPR_Poisson(plan, nx, ny, nz, T.BCS_NN, p, t1, t2, dev(hb), dev(ht), dpdy)
    p_ref, _ = OP.opr_poisson_fxz(plan_o, f, hb.reshape(nz, nx), ht.reshape(nz, nx))
    assert rel_err(p.cpu().numpy(), p_ref) <= TOL
