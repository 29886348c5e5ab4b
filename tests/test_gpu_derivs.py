"""GPU parity tests (run on the MI355X with -m gpu): the HIP path, called through the C ABI, against
 (1) the golden vectors generated from the reference itself, and (2) the numpy oracle on seeded inputs, for every
kernel family (wave-per-line x kernel, register-tile y/z kernel, generic kernel), every OPR_P* type on the path,
every boundary variant, Burgers SELF / U_IN, and the bit-exact transposes.
Tolerance: fp64 relative error <= 1e-12 (BASELINE.json north_star); index work (transposes) bit-exact."""
import numpy as np
import pytest
from conftest import golden_files, rel_err

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


def host(t):
    return t.cpu().numpy()


def grids(nx, ny, nz, ystretch=True, xper=True):
    x = np.arange(nx) / nx if xper else 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(nx) / (nx - 1) - 1)) / np.tanh(1.5))
    z = np.arange(nz) / nz * 2.0
    y = 0.5 * (1 + np.tanh(2 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(2)) if ystretch else np.arange(ny) / (ny - 1) * 1.5
    return x, y, z


def fields(nx, ny, nz, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(nx * ny * nz)
    u = np.sin(0.37 * (i % nx)) * np.cos(0.11 * (i // nx)) + 0.1 * rng.uniform(-1, 1, nx * ny * nz)
    v = np.cos(0.23 * (i % nx)) + 0.1 * rng.uniform(-1, 1, nx * ny * nz)
    return u, v


def run_all_ops(T, O, d, gp, op, nx, ny, nz, ibcs, u, v, visc, expect=None, tag=""):
    """Runs P1, P2, P2_P1, Burgers SELF and U_IN along direction d and checks against oracle (or `expect`)."""
    import torch
    part = (T.OPR_Partial_X, T.OPR_Partial_Y, T.OPR_Partial_Z)[d - 1]
    burg = (T.OPR_Burgers_X, T.OPR_Burgers_Y, T.OPR_Burgers_Z)[d - 1]
    du, dv = dev(u), dev(v)
    res, tmp = torch.empty_like(du), torch.empty_like(du)
    for ibc in ibcs:
        for t in (T.OPR_P1, T.OPR_P2, T.OPR_P2_P1):
            res.fill_(float("nan")); tmp.fill_(float("nan"))
            part(t, nx, ny, nz, ibc, gp, du, res, tmp)
            if expect is None:
                r, t1 = O.opr_partial(d, t, nx, ny, nz, ibc, op, u)
            else:
                r = expect["partial_d%d_t%d_bc%d" % (d, t, ibc)]
                t1 = expect["partial_d%d_t%d_bc%d_tmp1" % (d, t, ibc)] if t == 3 else None
            assert rel_err(host(res), r) <= TOL, (tag, d, ibc, t)
            if t == T.OPR_P2_P1:
                assert rel_err(host(tmp), t1) <= TOL, (tag, d, ibc, t, "tmp1")
        # Burgers: U_IN with velocity v, SELF with velocity = s
        res.fill_(float("nan"))
        burg(T.OPR_B_U_IN, visc, nx, ny, nz, ibc, gp, du, dv, res, tmp)
        r = O.opr_burgers(d, nx, ny, nz, ibc, op, visc, u, v)[0] if expect is None else expect["burgers_d%d_bc%d" % (d, ibc)]
        assert rel_err(host(res), r) <= TOL, (tag, d, ibc, "burgers u_in")
        res.fill_(float("nan")); tmp.fill_(float("nan"))
        burg(T.OPR_B_SELF, visc, nx, ny, nz, ibc, gp, du, du, res, tmp, write_transposed=True)
        r, st = O.opr_burgers(d, nx, ny, nz, ibc, op, visc, u, u)
        assert rel_err(host(res), r) <= TOL, (tag, d, ibc, "burgers self")
        if d == 1 or (d == 2 and nz > 1):
            assert np.array_equal(host(tmp), st), (tag, d, "transposed operand must be bit-exact")


@pytest.mark.parametrize("path", golden_files("derivs_"))
def test_golden_vectors(T, path):
    """Reference-generated fixtures (small sizes -> generic kernel family)."""
    from oracle import tlab_oracle as O
    g = np.load(path)
    nx, ny, nz = int(g["nx"]), int(g["ny"]), int(g["nz"])
    spec = {1: (g["x"], True, True), 2: (g["y"], False, bool(g["yuniform"])), 3: (g["z"], True, True)}
    for d, (nodes, per, uni) in spec.items():
        gp = T.FdmPlan(nodes, per, uni, int(g["mode1"]), int(g["mode2"]))
        op = O.FdmPlan(nodes, per, uni, int(g["mode1"]), int(g["mode2"]))
        # golden burgers used velocity v for U_IN; SELF checked against the oracle inside run_all_ops
        run_all_ops(T, O, d, gp, op, nx, ny, nz, (0, 1, 2, 3) if d == 2 else (0,), g["u"], g["v"], float(g["visc"]), expect=g, tag=path)


@pytest.mark.parametrize("nx,ny,nz", [(96, 64, 40), (256, 130, 12), (512, 128, 64)])
def test_penta_first_derivative(T, nx, ny, nz):
    """SpaceOrder1 = CompactJacobian6Penta (fdm_com1_jacobian.f90:136-192; k_pentatile on lines of 64 .. 512 points in 32-row chunks -- 96, 64, 256, 512,
    128 here --, k_penta1, one line per thread, on the others) in the three directions, all
    operator types and the Burgers operator, against the oracle (itself bitwise equal to the reference for this scheme, tests/golden/
    derivs_penta_*.npz); the plan also built from the host's tables (tlab_fdm_plan_create_from_arrays, ndl1 = 5).
    Uniform periodic grids, whole tiles, 2 / 3 / 4 / 8 / 16 chunks only: tables whose rows differ, odd chunk counts, partial tiles, non-periodic
    x and z lines, k_penta1 along x, guard zones and the forms behind environment switches are in tests/test_gpu_penta_lines.py."""
    from oracle import tlab_oracle as O
    x, y, z = grids(nx, ny, nz, ystretch=True)
    u, v = fields(nx, ny, nz, 5 * nx + ny)
    for d, (nodes, per) in {1: (x, True), 2: (y, False), 3: (z, True)}.items():
        gp, op = T.FdmPlan(nodes, per, per, 5, 7), O.FdmPlan(nodes, per, per, 5, 7)
        run_all_ops(T, O, d, gp, op, nx, ny, nz, (0,) if per else (0, 1, 2, 3), u, v, 1.0 / 500.0, tag="penta")
    nd2 = op.der2
    hp = T.FdmPlan.from_arrays(nz, True, 0, op.der1.lhs, op.der1.rhs[:, :7], nd2.lhs, nd2.rhs[:, :nd2.nb_diag[1] + 3], ndl1=5)
    run_all_ops(T, O, 3, hp, op, nx, ny, nz, (0,), u, v, 1.0 / 500.0, tag="penta from_arrays")


@pytest.mark.parametrize("nx,ny,nz,xper", [(256, 5, 3, True), (512, 3, 5, True), (1024, 2, 3, True), (256, 4, 3, False), (512, 3, 2, False)])
def test_x_wave_per_line_kernel(T, nx, ny, nz, xper):
    from oracle import tlab_oracle as O
    from tlab_amd.lib import load
    x, _, _ = grids(nx, 8, 8, xper=xper)
    gp, op = T.FdmPlan(x, xper, xper), O.FdmPlan(x, xper, xper)
    u, v = fields(nx, ny, nz, nx + ny)
    run_all_ops(T, O, 1, gp, op, nx, ny, nz, (0,) if xper else (0, 1, 2, 3), u, v, 1.0 / 300.0, tag="xline")
    expected_path = 2 if (xper or True) else 1
    if xper:
        assert load().tlab_last_kernel_path() == 2
    else:
        # stretched x needs the Jacobian correction for the second derivative -> generic family for Burgers
        assert load().tlab_last_kernel_path() in (1, 2)


@pytest.mark.parametrize("m", [0, 16, 32, 64])
@pytest.mark.parametrize("nx,ny,nz", [(64, 32, 3), (80, 48, 2), (128, 96, 2), (64, 128, 2), (64, 512, 1), (96, 192, 2)])
def test_y_register_tile_kernel(T, nx, ny, nz, m):
    from oracle import tlab_oracle as O
    from tlab_amd.lib import load
    load().tlab_set_tuning(1, m)
    try:
        for stretch in (True, False):
            _, y, _ = grids(8, ny, 8, ystretch=stretch)
            gp, op = T.FdmPlan(y, False, not stretch), O.FdmPlan(y, False, not stretch)
            u, v = fields(nx, ny, nz, ny + nz)
            run_all_ops(T, O, 2, gp, op, nx, ny, nz, (0, 1, 2, 3), u, v, 1.0 / 700.0, tag="rtile-y m=%d" % m)
            assert load().tlab_last_kernel_path() == 3
    finally:
        load().tlab_set_tuning(1, 0)


@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("nx,ny,nz,d", [(64, 64, 3, 2), (48, 128, 2, 2), (32, 512, 2, 2), (40, 1024, 1, 2), (64, 2, 256, 3), (16, 4, 1024, 3), (96, 192, 1, 2)])
def test_half_wave_tile_kernel_policies(T, nx, ny, nz, d, policy):
    """k_htile (32-line tiles, fused two-derivative modes) forced on (2) and off (1): both must match the oracle."""
    from oracle import tlab_oracle as O
    from tlab_amd.lib import load
    load().tlab_set_tuning(2, policy)
    try:
        n = (nx, ny, nz)[d - 1]
        for stretch in ((True, False) if d == 2 else (False,)):
            if d == 2:
                _, nodes, _ = grids(8, n, 8, ystretch=stretch)
                per, uni = False, not stretch
            else:
                nodes, per, uni = np.arange(n) / n * 2.0, True, True
            gp, op = T.FdmPlan(nodes, per, uni), O.FdmPlan(nodes, per, uni)
            u, v = fields(nx, ny, nz, n + policy)
            run_all_ops(T, O, d, gp, op, nx, ny, nz, (0, 1, 2, 3) if d == 2 else (0,), u, v, 1.0 / 400.0, tag="htile policy %d" % policy)
            assert load().tlab_last_kernel_path() == 3
    finally:
        load().tlab_set_tuning(2, 0)


@pytest.mark.parametrize("m", [0, 64])
@pytest.mark.parametrize("nx,ny,nz", [(64, 3, 32), (40, 5, 64), (64, 2, 256), (32, 6, 512), (16, 4, 1024)])
def test_z_register_tile_kernel(T, nx, ny, nz, m):
    from oracle import tlab_oracle as O
    from tlab_amd.lib import load
    load().tlab_set_tuning(1, m)
    try:
        _, _, z = grids(8, 8, nz)
        gp, op = T.FdmPlan(z, True, True), O.FdmPlan(z, True, True)
        u, v = fields(nx, ny, nz, nz)
        run_all_ops(T, O, 3, gp, op, nx, ny, nz, (0,), u, v, 1.0 / 500.0, tag="rtile-z m=%d" % m)
        assert load().tlab_last_kernel_path() == 3
    finally:
        load().tlab_set_tuning(1, 0)


@pytest.mark.parametrize("nx,ny,nz", [(24, 10, 9), (50, 13, 11), (8, 8, 8)])
def test_generic_kernel_odd_sizes(T, nx, ny, nz):
    from oracle import tlab_oracle as O
    x, y, z = grids(nx, ny, nz)
    u, v = fields(nx, ny, nz, 5)
    for d, (nodes, per, uni) in {1: (x, True, True), 2: (y, False, False), 3: (z, True, True)}.items():
        gp, op = T.FdmPlan(nodes, per, uni), O.FdmPlan(nodes, per, uni)
        run_all_ops(T, O, d, gp, op, nx, ny, nz, (0, 1, 2, 3) if d == 2 else (0,), u, v, 1e-2, tag="generic")


@pytest.mark.parametrize("m1,m2", [(4, 4), (6, 6), (4, 7)])
def test_other_schemes_on_fast_kernels(T, m1, m2):
    """CompactJacobian4 (3-diagonal RHS) and CompactJacobian6 (5-diagonal second-derivative RHS) through the same fast kernels."""
    from oracle import tlab_oracle as O
    from tlab_amd.lib import load
    nx, ny, nz = 256, 64, 32
    x, y, z = grids(nx, ny, nz)
    u, v = fields(nx, ny, nz, m1 * 10 + m2)
    for d, (nodes, per, uni) in {1: (x, True, True), 2: (y, False, False), 3: (z, True, True)}.items():
        gp, op = T.FdmPlan(nodes, per, uni, m1, m2), O.FdmPlan(nodes, per, uni, m1, m2)
        run_all_ops(T, O, d, gp, op, nx, ny, nz, (0, 1, 2, 3) if d == 2 else (0,), u, v, 1e-2, tag="schemes %d/%d" % (m1, m2))
        assert load().tlab_last_kernel_path() in (2, 3)


@pytest.mark.parametrize("nx,ny,nz,stretch,m1", [(16, 12, 8, True, 6), (64, 128, 4, True, 6), (64, 512, 2, False, 6), (40, 33, 3, True, 4), (32, 64, 1, True, 4)])
def test_boundary_bcs_neumann_y(T, nx, ny, nz, stretch, m1):
    """BOUNDARY_BCS_NEUMANN_Y vs the oracle (C1N6) or, for C1N4, through the property it exists for: du/dy = 0 at the wall."""
    import torch
    from oracle import tlab_oracle as O
    x, y, z = grids(nx, ny, nz, stretch)
    gp = T.FdmPlan(y, False, not stretch, m1, 7 if m1 == 6 else 4)
    op = O.FdmPlan(y, False, not stretch, m1, 7 if m1 == 6 else 4)
    u, _ = fields(nx, ny, nz, 21)
    du = dev(u)
    tmp = torch.empty_like(du)
    for ibc in (1, 2, 3):
        hb = torch.full((nx * nz,), float("nan"), dtype=torch.float64, device="cuda")
        ht = hb.clone()
        T.BOUNDARY_BCS_NEUMANN_Y(ibc, nx, ny, nz, gp, du, hb, ht, tmp)
        assert bool(torch.isnan(hb).all()) == (ibc == 2) and bool(torch.isnan(ht).all()) == (ibc == 1)    # untouched when not selected
        if m1 == 6:
            ob, ot = O.boundary_bcs_neumann_y(ibc, nx, ny, nz, op, u)
            if ibc & 1:
                assert rel_err(host(hb), ob.ravel()) <= TOL
            if ibc & 2:
                assert rel_err(host(ht), ot.ravel()) <= TOL
        a = u.reshape(nz, ny, nx).copy()
        if ibc & 1:
            a[:, 0, :] = host(hb).reshape(nz, nx)
        if ibc & 2:
            a[:, -1, :] = host(ht).reshape(nz, nx)
        d = O.opr_partial(2, O.OPR_P1, nx, ny, nz, 0, op, a.ravel())[0].reshape(nz, ny, nx)
        if ibc & 1:
            assert np.abs(d[:, 0, :]).max() <= 1e-10 * np.abs(d).max()
        if ibc & 2:
            assert np.abs(d[:, -1, :]).max() <= 1e-10 * np.abs(d).max()
    with pytest.raises(T.TlabError):
        T.BOUNDARY_BCS_NEUMANN_Y(0, nx, ny, nz, gp, du, hb, ht, tmp)


def test_two_dimensional_guard_and_errors(T):
    """opr_partial.f90:175-177: a direction of size 1 returns zeros; bad calls are refused, not computed."""
    import torch
    from tlab_amd.lib import load
    nx, ny, nz = 256, 16, 1
    gz = T.FdmPlan(np.zeros(1), True, True)
    u = dev(np.ones(nx * ny * nz)); r = torch.full_like(u, 7.0); t = torch.full_like(u, 7.0)
    T.OPR_Partial_Z(T.OPR_P2_P1, nx, ny, nz, 0, gz, u, r, t)
    assert float(r.abs().max()) == 0.0 and float(t.abs().max()) == 0.0
    gx = T.FdmPlan(np.arange(nx) / nx, True, True)
    with pytest.raises(T.TlabError):
        T.OPR_Partial_X(5, nx, ny, nz, 0, gx, u, r, t)          # OPR_P1_INT_VP: not built on the device
    with pytest.raises(T.TlabError):
        T.OPR_Partial_X(T.OPR_P1, nx, ny, nz, 0, gx, u, u, t)   # aliasing
    with pytest.raises(T.TlabError):
        T.OPR_Partial_Y(T.OPR_P1, nx, ny, nz, 0, gx, u, r, t)   # plan of the wrong size


def test_transpose_bit_exact(T):
    import torch
    rng = np.random.default_rng(11)
    for nra, nca in ((130, 70), (64, 64), (1, 257), (300, 3)):
        a = rng.uniform(-1, 1, nra * nca)
        b = torch.empty(nra * nca, dtype=torch.float64, device="cuda")
        T.TLab_Transpose(dev(a), nra, nca, b)
        assert np.array_equal(host(b).reshape(nra, nca), a.reshape(nca, nra).T)


@pytest.mark.parametrize("n", [256, 512])
def test_full_size_properties(T, n):
    """BASELINE sizes (256^3, 512^3): size-independent properties instead of an oracle run.
    (a) spectral exactness target: d/dx of a resolved sine is within the scheme's truncation error;
    (b) linearity; (c) fast kernels == generic kernel on the same data (two independent device algorithms);
    (d) d/dx of a constant is exactly representable: |result| <= 1e-12."""
    import torch
    from tlab_amd.lib import load
    nx = ny = nz = n
    x = np.arange(n) / n
    gp = T.FdmPlan(x, True, True)
    gy = T.FdmPlan(np.arange(n) / (n - 1.0), False, True)
    N = n ** 3
    gen = torch.Generator(device="cuda"); gen.manual_seed(20250509)
    a = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    b = torch.rand(N, dtype=torch.float64, device="cuda", generator=gen) - 0.5
    ra, rb, rc, tmp = (torch.empty_like(a) for _ in range(4))
    for d, plan, part in ((1, gp, T.OPR_Partial_X), (2, gy, T.OPR_Partial_Y), (3, gp, T.OPR_Partial_Z)):
        part(T.OPR_P1, nx, ny, nz, 0, plan, a, ra)
        part(T.OPR_P1, nx, ny, nz, 0, plan, b, rb)
        c = 2.0 * a - 3.0 * b
        part(T.OPR_P1, nx, ny, nz, 0, plan, c, rc)
        scale = float(rc.abs().max())
        assert float((rc - (2.0 * ra - 3.0 * rb)).abs().max()) / scale <= TOL, ("linearity", d)
        fast_path = load().tlab_last_kernel_path()
        assert fast_path in (2, 3)
        load().tlab_force_kernel_path(1)
        try:
            part(T.OPR_P1, nx, ny, nz, 0, plan, a, rb)
        finally:
            load().tlab_force_kernel_path(0)
        assert float((ra - rb).abs().max()) / float(ra.abs().max()) <= TOL, ("fast vs generic", d)
        part(T.OPR_P2_P1, nx, ny, nz, 0, plan, a, rc, tmp)
        assert float((tmp - ra).abs().max()) / float(ra.abs().max()) <= TOL, ("P2_P1 tmp1 == P1", d)
    # analytic: sin(2 pi k x) along x, k = 4
    i = torch.arange(nx, dtype=torch.float64, device="cuda")
    line = torch.sin(2 * np.pi * 4 * i / nx)
    a.view(nz * ny, nx)[:] = line
    T.OPR_Partial_X(T.OPR_P1, nx, ny, nz, 0, gp, a, ra)
    exact = (2 * np.pi * 4) * torch.cos(2 * np.pi * 4 * i / nx)
    assert float((ra.view(nz * ny, nx) - exact).abs().max()) / (2 * np.pi * 4) <= 1e-9
    a.fill_(3.25)
    T.OPR_Partial_X(T.OPR_P1, nx, ny, nz, 0, gp, a, ra)
    assert float(ra.abs().max()) <= 1e-12 * n


def test_x_lines_of_2048_take_the_wave_per_line_kernel(T):
    """BASELINE configs[4]: x lines of 2048 points.  32 rows per lane; the lane-variant tables (164 KB as doubles for the two systems) are
    kept as chunk 0's value + a float difference, which the plan verifies to be exact on the host (operators.cpp xline_wide_ok).  All operator
    types against the oracle; a non-periodic x of 2048 points (not compressible) still takes the generic kernel."""
    import torch
    from oracle import tlab_oracle as O
    nx, ny, nz = 2048, 16, 8
    x = np.arange(nx) / nx * 3.0
    g, og = T.FdmPlan(x, True, True), O.FdmPlan(x, True, True)
    rng = np.random.default_rng(2048)
    u = rng.uniform(-1, 1, nx * ny * nz); v = rng.uniform(-1, 1, nx * ny * nz)
    du, dv = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    r = torch.zeros_like(du); t = torch.zeros_like(du)
    for typ in (1, 2, 3):
        T.OPR_Partial_X(typ, nx, ny, nz, 0, g, du, r, t)
        assert T.load().tlab_last_kernel_path() == 2                      # wave-per-line
        ro, to = O.opr_partial(1, typ, nx, ny, nz, 0, og, u)
        assert rel_err(r.cpu().numpy(), ro) <= 1e-12, typ
        if typ == 3:
            assert rel_err(t.cpu().numpy(), to) <= 1e-12
    T.OPR_Burgers_X(T.OPR_B_U_IN, 2e-4, nx, ny, nz, 0, g, du, dv, r, t)
    assert T.load().tlab_last_kernel_path() == 2
    assert rel_err(r.cpu().numpy(), O.opr_burgers(1, nx, ny, nz, 0, og, 2e-4, u, v)[0]) <= 1e-12
    xs = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(nx) / (nx - 1) - 1)) / np.tanh(1.5))
    gs, ogs = T.FdmPlan(xs, False, False), O.FdmPlan(xs, False, False)
    T.OPR_Partial_X(1, nx, ny, nz, 0, gs, du, r, t)
    assert T.load().tlab_last_kernel_path() == 1                          # generic
    assert rel_err(r.cpu().numpy(), O.opr_partial(1, 1, nx, ny, nz, 0, ogs, u)[0]) <= 1e-12


@pytest.mark.parametrize("nx", [1024, 2048])
@pytest.mark.parametrize("wander", [False, True])
def test_x_lines_on_several_waves_both_table_forms(T, nx, wander):
    """x lines of 1024 / 2048 points on 2 / 4 waves (8 rows per lane); the two-system forms keep the per-lane constants of the separator reduction
    in LDS.  wander = False: tables whose rows are all the same (2048 points, two systems: scalar loads of chunk 0's rows, no table in LDS);
    True: rows that differ by ~1e-13 like the reference's own tables of a "uniform" grid (per-chunk tables in LDS: doubles, or chunk 0 + float
    differences).  All operator types and the 4-field Burgers launch against the oracle working from the same tables."""
    import ctypes
    import torch
    from oracle import tlab_oracle as O
    from tlab_amd.lib import load, check, c_vp
    L = load()
    ny, nz = 6, 5
    x = np.arange(nx) / nx * 2.0
    og = O.FdmPlan(x, True, True)
    rng = np.random.default_rng(nx)
    w = 1.0 + 1e-13 * rng.uniform(-1, 1, nx) if wander else np.ones(nx)
    mid = nx // 2           # every row = the middle row (exactly uniform), times what a per-row Jacobian does to the tables
    for dp, ww in ((og.der1, w), (og.der2, w * w)):
        dp.lhs = np.tile(dp.lhs[mid], (nx, 1)) * ww[:, None]
        dp.rhs = np.tile(dp.rhs[mid], (nx, 1)) * ww[:, None]
        ndl = dp.nb_diag[0]
        cols = [dp.lhs[:, k].copy() if k < ndl else np.zeros(nx) for k in range(ndl + 2)]
        O.tridpfs(*cols)
        dp.lu = np.stack(cols, axis=1)
    g = T.FdmPlan.from_arrays(nx, True, 0, og.der1.lhs, og.der1.rhs[:, :og.der1.nb_diag[1]], og.der2.lhs, og.der2.rhs[:, :og.der2.nb_diag[1] + 3])
    assert L.tlab_fdm_plan_info(g._h, 8) == nx // 8 and L.tlab_fdm_plan_info(g._h, 9) == (0 if wander else 1)
    rng = np.random.default_rng(nx + 1)
    N = nx * ny * nz
    f = [rng.uniform(-1, 1, N) for _ in range(4)]
    d = [torch.from_numpy(a).cuda() for a in f]
    r = torch.zeros(N, dtype=torch.float64, device="cuda"); t = torch.zeros_like(r)
    for typ in (1, 2, 3):
        T.OPR_Partial_X(typ, nx, ny, nz, 0, g, d[0], r, t)
        assert L.tlab_last_kernel_path() == 2
        ro, to = O.opr_partial(1, typ, nx, ny, nz, 0, og, f[0])
        assert rel_err(r.cpu().numpy(), ro) <= 1e-12, typ
        if typ == 3:
            assert rel_err(t.cpu().numpy(), to) <= 1e-12
    h = [torch.from_numpy(rng.uniform(-1, 1, N)).cuda() for _ in range(4)]
    h0 = [a.cpu().numpy().copy() for a in h]
    nu = (ctypes.c_double * 4)(2e-4, 3e-4, 4e-4, 5e-4)
    sp = (c_vp * 4)(*[a.data_ptr() for a in d])
    hp = (c_vp * 4)(*[a.data_ptr() for a in h])
    check(L.tlab_opr_burgers_add_n(1, g._h, nx, ny, nz, 0, 4, nu, sp, d[0].data_ptr(), hp, r.data_ptr(), t.data_ptr(), 0), "burgers_add_n")
    for i in range(4):
        ref = h0[i] + O.opr_burgers(1, nx, ny, nz, 0, og, nu[i], f[i], f[0])[0]
        assert rel_err(h[i].cpu().numpy(), ref) <= 1e-12, i


@pytest.mark.parametrize("d", [2, 3])
def test_lines_of_1024_points_fused_on_16_line_tiles(T, d):
    """BASELINE configs[3]/[4]: y / z lines of 1024 points.  OPR_P2_P1 and OPR_Burgers keep two line-sets in registers on 16-line tiles
    (32 chunks of 32 rows, 512 threads) instead of taking two launches; stretched grid along y (Jacobian correction in-kernel)."""
    import torch
    from oracle import tlab_oracle as O
    n = 1024
    nx, ny, nz = (32, n, 8) if d == 2 else (32, 8, n)
    stretched = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(n) / (n - 1) - 1)) / np.tanh(1.5))
    nodes = stretched if d == 2 else np.arange(n) / n
    g = T.FdmPlan(nodes, d == 3, d == 3)
    og = O.FdmPlan(nodes, d == 3, d == 3)
    rng = np.random.default_rng(d)
    u = rng.uniform(-1, 1, nx * ny * nz); v = rng.uniform(-1, 1, nx * ny * nz)
    du, dv = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    r = torch.zeros_like(du); t = torch.zeros_like(du)
    part, burg = (T.OPR_Partial_Y, T.OPR_Burgers_Y) if d == 2 else (T.OPR_Partial_Z, T.OPR_Burgers_Z)
    part(T.OPR_P2_P1, nx, ny, nz, 0, g, du, r, t)
    ro, to = O.opr_partial(d, 3, nx, ny, nz, 0, og, u)
    assert rel_err(r.cpu().numpy(), ro) <= 1e-12 and rel_err(t.cpu().numpy(), to) <= 1e-12
    burg(T.OPR_B_U_IN, 3e-4, nx, ny, nz, 0, g, du, dv, r, t)
    assert rel_err(r.cpu().numpy(), O.opr_burgers(d, nx, ny, nz, 0, og, 3e-4, u, v)[0]) <= 1e-12


@pytest.mark.parametrize("grid", [0, 5, 3, 13])
def test_persistent_z_burgers_with_padding_items_and_any_grid(T, grid):
    """k_ptile (persistent workgroups, operand tile of the next item by LDS-DMA): 96 x 3 lines of 512 points = 9 tiles, three fields -> 48 items of
    which every (item & 7) >= tile count of its octet is padding.  With a grid that is not a multiple of 8 (partitioned parts: 38 / 228 CUs) a
    workgroup meets a padding item and then a valid one: the skip path must still bring the next operand tile in.  The grid is
    forced through tlab_set_tuning(4, n); 0 = the default (CUs rounded down to a multiple of 8)."""
    import ctypes
    import torch
    from oracle import tlab_oracle as O
    from tlab_amd.lib import load, check
    L = load()
    c_vp = ctypes.c_void_p
    nx, ny, nz = 96, 3, 512
    z = np.arange(nz) / nz
    g, og = T.FdmPlan(z, True, True), O.FdmPlan(z, True, True)
    rng = np.random.default_rng(40 + grid)
    N = nx * ny * nz
    f = [rng.uniform(-1, 1, N) for _ in range(3)]
    d = [torch.from_numpy(a).cuda() for a in f]
    h0 = [rng.uniform(-1, 1, N) for _ in range(3)]
    h = [torch.from_numpy(a).cuda() for a in h0]
    r = torch.zeros(N, dtype=torch.float64, device="cuda"); t = torch.zeros_like(r)
    nu = (ctypes.c_double * 3)(2e-4, 3e-4, 4e-4)
    sp = (c_vp * 3)(*[a.data_ptr() for a in d])
    hp = (c_vp * 3)(*[a.data_ptr() for a in h])
    check(L.tlab_set_tuning(4, grid), "set_tuning")
    try:
        L.tlab_profile_reset(); L.tlab_profile_enable(1)
        check(L.tlab_opr_burgers_add_n(3, g._h, nx, ny, nz, 0, 3, nu, sp, d[2].data_ptr(), hp, r.data_ptr(), t.data_ptr(), 0), "burgers_add_n")
        torch.cuda.synchronize()
        L.tlab_profile_enable(0)
        buf = ctypes.create_string_buffer(1 << 14); L.tlab_profile_report(buf, len(buf))
        assert "k_ptile<BURGERS>" in buf.value.decode(), buf.value.decode()
    finally:
        L.tlab_set_tuning(4, 0)
    for i in range(3):
        ref = h0[i] + O.opr_burgers(3, nx, ny, nz, 0, og, nu[i], f[i], f[2])[0]
        assert rel_err(h[i].cpu().numpy(), ref) <= 1e-12, (grid, i)
