"""GPU test of the Fortran side of the boundary: tlab_amd/fortran/test_dropin.f90 calls the drop-in modules
(OPR_Partial / OPR_Burgers signatures of the reference, ISO_C_BINDING underneath) on device memory and compares with the
reference's own CPU modules (oracle/_ref objects) in the same executable."""
import os
import subprocess
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "tlab_amd", "fortran", "_build", "test_dropin")


def test_fortran_dropin_side_by_side():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not os.path.exists(EXE):
        pytest.skip("tlab_amd/fortran/_build/test_dropin not built (needs oracle/_ref, i.e. the build container)")
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dropin ok" in r.stdout


# ---- the Runge-Kutta mini-driver: start-up sequence of dns_main.f90 and the loop of time.f90 on device memory -------------------------------
RK_EXE = os.path.join(ROOT, "tlab_amd", "fortran", "_build_rk", "test_rk_driver")
INI = """[Main]
Scalars={nscal}
SpaceOrder1=CompactJacobian6
SpaceOrder2=CompactJacobian6Hyper
{elliptic}
[Grid]
Imax={nx}
Jmax={ny}
Kmax={nz}
XUniform=yes
YUniform=no
ZUniform=yes
XPeriodic=yes
YPeriodic=no
ZPeriodic=yes

[Parameters]
Reynolds={reynolds}
Schmidt={schmidt}

[Time]
Scheme=RungeKuttaExplicit3
TimeStep={dtime}
Start=0
End={steps}

[BoundaryConditions]
{bcs}
"""


RK_EXE_FUSED = os.path.join(ROOT, "tlab_amd", "fortran", "_build_rk_fused", "test_rk_driver")


def run_rk_driver(tmp_path, x, y, z, q0, s0, reynolds, schmidt, dtime, steps, bcs_lines, elliptic="", ini=None, exe=None, env=None):
    """Writes tlab.ini, grid, flow.0.*, scal.0.* in the reference's formats, runs the Fortran mini-driver there, reads flow.<steps>.*, scal.<steps>.*"""
    import numpy as np
    from tlab_amd import io as tio
    nx, ny, nz = len(x), len(y), len(z)
    with open(os.path.join(tmp_path, "tlab.ini"), "w") as f:
        f.write((ini or INI).format(nscal=len(s0), nx=nx, ny=ny, nz=nz, reynolds=repr(float(reynolds)), schmidt=repr(float(schmidt)), dtime=repr(float(dtime)),
                           steps=steps, bcs="\n".join(bcs_lines), elliptic=elliptic))
    tio.grid_write(os.path.join(tmp_path, "grid"), x, y, z, scales=[x[-1] - x[0] + (x[1] - x[0]), y[-1] - y[0], z[-1] - z[0] + (z[1] - z[0])])
    tio.io_write_fields(os.path.join(tmp_path, "flow.0"), nx, ny, nz, 0, q0, params=(0.0, 1.0 / reynolds))
    tio.io_write_fields(os.path.join(tmp_path, "scal.0"), nx, ny, nz, 0, s0, params=(0.0,))
    r = subprocess.run([exe or RK_EXE], cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    log = ""
    for name in ("tlab.err", "tlab.log"):
        p = os.path.join(tmp_path, name)
        if os.path.exists(p):
            log += "\n--- %s ---\n" % name + open(p).read()[-3000:]
    assert r.returncode == 0, r.stdout + r.stderr + log
    assert not os.path.exists(os.path.join(tmp_path, "tlab.err")), r.stdout + r.stderr + log      # TLab_Stop after an error exits with code 0 in the serial build
    q1, _, _ = tio.io_read_fields(os.path.join(tmp_path, "flow.%d" % steps), nx, ny, nz, 3)
    s1, _, _ = tio.io_read_fields(os.path.join(tmp_path, "scal.%d" % steps), nx, ny, nz, len(s0))
    return q1, s1, log


def _need_rk():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not os.path.exists(RK_EXE):
        pytest.skip("tlab_amd/fortran/_build_rk/test_rk_driver not built (needs oracle/_ref, i.e. the build container)")


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("case", ["noslip", "freeslip"])
def test_fortran_rk_driver_against_golden_step(case, fused, tmp_path):
    """The unchanged-host sequence TLab_Start, TLab_Grid_Read, FDM_Initialize (all three the reference's own code), TLab_Initialize_Memory (hook),
    OPR_Burgers_Initialize(ifile), OPR_Elliptic_Initialize(ifile), OPR_Fourier_Initialize(), IO_Read_Fields, TIME_RUNGEKUTTA x 2 with the external
    RHS_GLOBAL_INCOMPRESSIBLE_1 and DAXPY / DSCAL on device arrays, IO_Write_Fields -- against the committed oracle fixture of the same two steps
    (tests/golden/make_golden_rk.py)."""
    import numpy as np
    from conftest import rel_err
    _need_rk()
    g = np.load(os.path.join(ROOT, "tests", "golden", "rk_step_%s.npz" % case))
    # fused: the same driver built with -DTLAB_AMD_FUSED_SUBSTEP -- the six-line patch of time.f90 that hands RHS + update loops + tendency scaling
    # of a substep to tlab_time_substep_incompressible_explicit in one call (TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT_AMD)
    if fused and not os.path.exists(RK_EXE_FUSED):
        pytest.skip("tlab_amd/fortran/_build_rk_fused/test_rk_driver not built")
    q1, s1, log = run_rk_driver(str(tmp_path), g["x"], g["y"], g["z"], list(g["q0"]), list(g["s0"]), float(g["reynolds"]), float(g["schmidt"]),
                                float(g["dtime"]), int(g["steps"]), [str(v) for v in g["ini"]], exe=RK_EXE_FUSED if fused else None)
    assert "HBM (tlab_malloc)" in log                         # the allocation hook was the allocator
    for i in range(3):
        assert rel_err(q1[i], g["q1"][i]) <= 1e-12, (case, "q", i, rel_err(q1[i], g["q1"][i]))
    assert rel_err(s1[0], g["s1"][0]) <= 1e-12, (case, "s")


@pytest.mark.parametrize("fused", [False, True])
def test_fortran_rk_driver_fast_kernels(tmp_path, fused):
    """The same driver at a size that takes the fused kernels (256-point x lines, 64-point y lines), against the numpy oracle run here; the log
    carries the transposition round trip of the same-named TLabMPI_Trp_Exec* procedures (one rank, RCCL communicator)."""
    import numpy as np
    from conftest import rel_err
    from scatter import substep_scatter, bound
    from oracle.tlab_oracle_rhs import DnsOracle
    _need_rk()
    nx, ny, nz = 256, 64, 32
    x = np.arange(nx) / nx * 2.0
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    rng = np.random.default_rng(77)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wall = np.sin(np.pi * Y)
    q0 = [((np.sin(np.pi * X + k) * np.cos(2 * np.pi * Z) + 0.1 * rng.uniform(-1, 1, X.shape)) * wall).ravel() for k in range(3)]
    s0 = [(np.cos(np.pi * X) * Y + 0.1 * rng.uniform(-1, 1, X.shape)).ravel()]
    re, sc, dt = 1000.0, 0.7, 1e-3
    bcs = ["VelocityJmin=noslip", "VelocityJmax=noslip", "Scalar1Jmin=dirichlet", "Scalar1Jmax=dirichlet"]
    if fused and not os.path.exists(RK_EXE_FUSED):
        pytest.skip("tlab_amd/fortran/_build_rk_fused/test_rk_driver not built")
    q1, s1, log = run_rk_driver(str(tmp_path), x, y, z, q0, s0, re, sc, dt, 1, bcs, exe=RK_EXE_FUSED if fused else None)
    assert "Checking transposition round trip: residual  0.000E+00" in log, log[-1500:]
    kdt, kco = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0]
    sched = [(dt * kdt[k], kco[k] if k < 2 else 1.0, k < 2) for k in range(3)]
    B, S = substep_scatter(lambda: DnsOracle(x, y, z, nscal=1, visc=1.0 / re, schmidt=(sc,), yuniform=False), q0, s0, sched, nsamples=1)
    for i in range(3):
        assert rel_err(q1[i], B[2]["q"][i]) <= bound(S[2]["q"][i]), ("q", i, rel_err(q1[i], B[2]["q"][i]), S[2]["q"][i])
    assert rel_err(s1[0], B[2]["s"][0]) <= bound(S[2]["s"][0])


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("nx,walls", [(64, "freeslip"), (128, "noslip")])
def test_fortran_rk_driver_through_the_slab_driver(tmp_path, fused, nx, walls):
    """The decomposed route of the Fortran host: RHS_GLOBAL_INCOMPRESSIBLE_1 (and TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT_AMD) hand the substep to the
    native z-slab driver -- tlab_slab_dns_create over the RCCL communicator of module TLabMPI_Transpose, the module arrays q(:, 1:3), s, hq, hs,
    txc bound as they are (columns back to back: the halo planes live in the driver's buffers).  One GPU here, so TLAB_AMD_FORCE_SLAB=1 takes that
    route with ims_npro_k = 1: the rank is its own ring neighbour and all-to-all peer, through ncclSend / ncclRecv.  Against the oracle.
    nx = 128, no-slip walls: the library's own x-transforms apply, so the driver folds the repack into them and finishes v and the scalar in the
    kernels that complete their tendencies (its default route)."""
    import numpy as np
    from conftest import rel_err
    from scatter import substep_scatter, bound
    from oracle.tlab_oracle_rhs import DnsOracle
    _need_rk()
    if fused and not os.path.exists(RK_EXE_FUSED):
        pytest.skip("tlab_amd/fortran/_build_rk_fused/test_rk_driver not built")
    ny, nz = 32, 64
    x = np.arange(nx) / nx * 2.0
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    rng = np.random.default_rng(64)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wall = np.sin(np.pi * Y)
    q0 = [((np.sin(np.pi * X + k) * np.cos(2 * np.pi * Z) + 0.1 * rng.uniform(-1, 1, X.shape)) * wall).ravel() for k in range(3)]
    s0 = [(np.cos(np.pi * X) * Y + 0.1 * rng.uniform(-1, 1, X.shape)).ravel()]
    re, sc, dt = 1000.0, 0.7, 1e-3
    bcs = ["VelocityJmin=freeslip", "VelocityJmax=freeslip", "Scalar1Jmin=neumann", "Scalar1Jmax=dirichlet"] if walls == "freeslip" else \
        ["VelocityJmin=noslip", "VelocityJmax=noslip", "Scalar1Jmin=dirichlet", "Scalar1Jmax=dirichlet"]
    q1, s1, log = run_rk_driver(str(tmp_path), x, y, z, q0, s0, re, sc, dt, 2, bcs, exe=RK_EXE_FUSED if fused else None, env={"TLAB_AMD_FORCE_SLAB": "1"})
    kdt, kco = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0]
    sched = [(dt * kdt[k % 3], kco[k % 3] if k % 3 < 2 else 1.0, k % 3 < 2, k % 3 == 0) for k in range(6)]

    def make_oracle():
        from tlab_amd.dns import velocity_bcs
        o = DnsOracle(x, y, z, nscal=1, visc=1.0 / re, schmidt=(sc,), yuniform=False)
        o.flow_jmin = o.flow_jmax = velocity_bcs(walls)
        if walls == "freeslip":
            o.scal_jmin, o.scal_jmax = [4], [3]
        return o
    B, S = substep_scatter(make_oracle, q0, s0, sched, nsamples=1)
    for i in range(3):
        assert rel_err(q1[i], B[5]["q"][i]) <= bound(S[5]["q"][i]), ("q", i, rel_err(q1[i], B[5]["q"][i]), S[5]["q"][i])
    assert rel_err(s1[0], B[5]["s"][0]) <= bound(S[5]["s"][0])
    # and it did take the slab route: the single-domain driver state was never created (its Poisson plan logs nothing; the slab one is silent too),
    # so ask the run itself: a second run without the switch differs in the last bits (another operator order), not in substance
    q2, _, _ = run_rk_driver(str(tmp_path), x, y, z, q0, s0, re, sc, dt, 2, bcs, exe=RK_EXE_FUSED if fused else None)
    d = max(rel_err(q1[i], q2[i]) for i in range(3))
    assert 0.0 < d <= 1e-10, d


@pytest.mark.parametrize("route", ["TLAB_AMD_FORCE_PENCIL", "TLAB_AMD_FORCE_SLAB"])
@pytest.mark.parametrize("fused", [False, True])
def test_fortran_rk_driver_through_the_pencil_driver(tmp_path, fused, route):
    """TLAB_AMD_FORCE_SLAB on this box of 32 planes: the z-slab route with slabs too THIN for the partitioned z systems (tlab_zslab_plan_create refuses
    them) -- the Fortran host then takes the reference's own scheme, K-transpositions around the z operators, through the pencil driver with npro_i = 1
    instead of stopping.
    The x/z pencil route of the Fortran host (ims_npro_i > 1): RHS_GLOBAL_INCOMPRESSIBLE_1 / TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT_AMD hand the substep
    to tlab_pencil_dns_* with the module arrays bound as they are.  One GPU here: TLAB_AMD_FORCE_PENCIL=1 takes that route on 1 x 1 ranks (loopback
    transport: the marshalling, the binding of q / s / hq / hs / txc and the step-start zeroing are what is exercised; the transpositions themselves are
    covered on 2 x 2 .. 4 x 4 ranks in tests/test_gpu_pencil.py).  Two Runge-Kutta steps against the oracle."""
    import numpy as np
    from conftest import rel_err
    from scatter import substep_scatter, bound
    from oracle.tlab_oracle_rhs import DnsOracle
    _need_rk()
    if fused and not os.path.exists(RK_EXE_FUSED):
        pytest.skip("tlab_amd/fortran/_build_rk_fused/test_rk_driver not built")
    nx, ny, nz = 64, 32, 32
    x = np.arange(nx) / nx * 2.0
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    rng = np.random.default_rng(65)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wall = np.sin(np.pi * Y)
    q0 = [((np.sin(np.pi * X + k) * np.cos(2 * np.pi * Z) + 0.1 * rng.uniform(-1, 1, X.shape)) * wall).ravel() for k in range(3)]
    s0 = [(np.cos(np.pi * X) * Y + 0.1 * rng.uniform(-1, 1, X.shape)).ravel()]
    re, sc, dt = 1000.0, 0.7, 1e-3
    bcs = ["VelocityJmin=freeslip", "VelocityJmax=freeslip", "Scalar1Jmin=neumann", "Scalar1Jmax=dirichlet"]
    q1, s1, log = run_rk_driver(str(tmp_path), x, y, z, q0, s0, re, sc, dt, 2, bcs, exe=RK_EXE_FUSED if fused else None, env={route: "1"})
    kdt, kco = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0]
    sched = [(dt * kdt[k % 3], kco[k % 3] if k % 3 < 2 else 1.0, k % 3 < 2, k % 3 == 0) for k in range(6)]

    def make_oracle():
        from tlab_amd.dns import velocity_bcs
        o = DnsOracle(x, y, z, nscal=1, visc=1.0 / re, schmidt=(sc,), yuniform=False)
        o.flow_jmin = o.flow_jmax = velocity_bcs("freeslip")
        o.scal_jmin, o.scal_jmax = [4], [3]
        return o
    B, S = substep_scatter(make_oracle, q0, s0, sched, nsamples=1)
    for i in range(3):
        assert rel_err(q1[i], B[5]["q"][i]) <= bound(S[5]["q"][i]), ("q", i, rel_err(q1[i], B[5]["q"][i]), S[5]["q"][i])
    assert rel_err(s1[0], B[5]["s"][0]) <= bound(S[5]["s"][0])
    q2, _, _ = run_rk_driver(str(tmp_path), x, y, z, q0, s0, re, sc, dt, 2, bcs, exe=RK_EXE_FUSED if fused else None)
    d = max(rel_err(q1[i], q2[i]) for i in range(3))
    assert 0.0 < d <= 1e-10, d       # another operator order than the single-domain driver, not another result


def test_case01_own_tlab_ini_through_the_fortran_driver(tmp_path):
    """BASELINE configs[0] = examples/Case01 on ITS OWN tlab.ini (tests/golden/case01/tlab.ini: the example's input file as the reference ships it,
    a data fixture; only `End=10` is shortened to 2 iterations): 512 x 256 x 1, SpaceOrder = CompactJacobian6 (the backwards-compatible key, read by
    the reference's own FDM_Initialize), TimeOrder = RungeKuttaExplicit4, TimeCFL = 1.2 with TimeStep < 0 (the step comes from TIME_COURANT every
    iteration), free-slip walls, Neumann scalar -- all read by the Fortran mini-driver through the reference's key names.  The case's initial fields come
    from the reference's initialisation tools (out of scope), so synthetic shear-layer fields of the case's shape are written in the reference's restart
    format.  Against the oracle stepping the same way (time_courant + 5 RK4 substeps per iteration)."""
    import numpy as np
    from conftest import rel_err
    from tlab_amd import io as tio
    from tlab_amd.dns import rk_coefficients, RKM_EXP4, velocity_bcs
    from oracle.tlab_oracle_rhs import DnsOracle
    _need_rk()
    ini = open(os.path.join(ROOT, "tests", "golden", "case01", "tlab.ini")).read()
    assert "Imax=512" in ini and "TimeOrder=RungeKuttaExplicit4" in ini and "TimeCFL=1.20000" in ini and "VelocityJmin=freeslip" in ini
    iters = 2
    ini = ini.replace("End=10", "End=%d" % iters)
    nx, ny, nz = 512, 256, 1
    x = np.arange(nx) / nx * 2.0                 # [IniGridOx]: 513 points on 2.0, periodic -> 512 nodes
    y = np.arange(ny) / (ny - 1.0)               # [IniGridOy]: 256 points on 1.0
    z = np.zeros(1)
    rng = np.random.default_rng(101)
    Y, X = np.meshgrid(y, x, indexing="ij")
    thick = 0.005859375 * 8
    u0 = 0.5 * np.tanh((Y - 0.5) / (2 * thick)) + 0.02 * rng.uniform(-1, 1, X.shape) * np.exp(-((Y - 0.5) / 0.1) ** 2)
    v0 = 0.02 * rng.uniform(-1, 1, X.shape) * np.exp(-((Y - 0.5) / 0.1) ** 2) * np.sin(np.pi * Y)
    s0 = 0.5 - 0.5 * np.tanh((Y - 0.5) / (2 * thick))
    q0, sc0 = [u0.ravel(), v0.ravel(), np.zeros(nx * ny)], [s0.ravel()]
    tmp = str(tmp_path)
    open(os.path.join(tmp, "tlab.ini"), "w").write(ini)
    tio.grid_write(os.path.join(tmp, "grid"), x, y, z, scales=[2.0, 1.0, 1.0])
    tio.io_write_fields(os.path.join(tmp, "flow.0"), nx, ny, nz, 0, q0, params=(0.0, 1.0 / 5000.0))
    tio.io_write_fields(os.path.join(tmp, "scal.0"), nx, ny, nz, 0, sc0, params=(0.0,))
    r = subprocess.run([RK_EXE], cwd=tmp, capture_output=True, text=True, timeout=600)
    log = "".join(open(os.path.join(tmp, f)).read()[-3000:] for f in ("tlab.err", "tlab.log") if os.path.exists(os.path.join(tmp, f)))
    assert r.returncode == 0 and not os.path.exists(os.path.join(tmp, "tlab.err")), r.stdout + r.stderr + log
    q1, _, _ = tio.io_read_fields(os.path.join(tmp, "flow.%d" % iters), nx, ny, nz, 3)
    s1, _, _ = tio.io_read_fields(os.path.join(tmp, "scal.%d" % iters), nx, ny, nz, 1)
    o = DnsOracle(x, y, z, nscal=1, visc=1.0 / 5000.0, schmidt=(1.0,), yuniform=True)
    o.flow_jmin = o.flow_jmax = velocity_bcs("freeslip"); o.scal_jmin = o.scal_jmax = [4]
    for i in range(3):
        o.q[i] = q0[i].copy()
    o.s[0] = sc0[0].copy()
    kdt, kco = rk_coefficients(RKM_EXP4)
    steps = []
    for it in range(iters):
        _, dt = o.time_courant(1.2, 0.3)         # TimeDiffusiveCFL defaults to 0.25 TimeCFL (dns_read_local.f90:72-73)
        steps.append(dt)
        o.hq = [np.zeros_like(a) for a in o.hq]; o.hs = [np.zeros_like(a) for a in o.hs]
        for k in range(5):
            o.time_substep(dt * kdt[k], 1.0 if k == 4 else kco[k], k < 4)
    logged = [float(line.split("=")[1]) for line in log.splitlines() if "TIME_COURANT: dtime" in line]
    assert len(logged) == iters and all(abs(a - b) <= 1e-13 * b for a, b in zip(logged, steps)), (logged, steps)
    for i in range(2):
        assert rel_err(q1[i], o.q[i]) <= 1e-12, ("q", i, rel_err(q1[i], o.q[i]))
    assert np.abs(q1[2]).max() == 0.0 and rel_err(s1[0], o.s[0]) <= 1e-12


def test_fortran_rk_driver_direct_schemes_from_the_ini_file(tmp_path):
    """[Main] SpaceOrder2 = CompactDirect6, EllipticOrder = CompactDirect6 (the scheme set of examples/Case81-93) read by the reference's own
    FDM_Initialize and by the drop-in OPR_Elliptic_Initialize(inifile), which builds fdm_loc with the reference's FDM_CreatePlan
    (opr_elliptic.f90:107-124) -- against the oracle on the tables the reference generated for the same nodes (tests/golden/direct_y.npz)."""
    import numpy as np
    from conftest import rel_err
    from scatter import substep_scatter, bound
    from oracle import tlab_oracle as O
    from oracle.tlab_oracle_rhs import DnsOracle
    _need_rk()
    G = np.load(os.path.join(ROOT, "tests", "golden", "direct_y.npz"))
    nx, ny, nz = 256, 64, 32
    tab = {k[len("ny%d_" % ny):]: G[k] for k in G.files if k.startswith("ny%d_" % ny)}
    x, y, z = np.arange(nx) / nx * 2.0, tab["nodes"], np.arange(nz) / nz
    rng = np.random.default_rng(81)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wall = np.sin(np.pi * (Y - y[0]) / (y[-1] - y[0]))
    q0 = [((np.sin(np.pi * X + k) * np.cos(2 * np.pi * Z) + 0.1 * rng.uniform(-1, 1, X.shape)) * wall).ravel() for k in range(3)]
    s0 = [(np.cos(np.pi * X) * Y + 0.1 * rng.uniform(-1, 1, X.shape)).ravel()]
    re, sc, dt = 800.0, 0.7, 2e-3
    bcs = ["VelocityJmin=noslip", "VelocityJmax=noslip", "Scalar1Jmin=dirichlet", "Scalar1Jmax=dirichlet"]
    ini = INI.replace("SpaceOrder2=CompactJacobian6Hyper", "SpaceOrder2=CompactDirect6")
    q1, s1, _ = run_rk_driver(str(tmp_path), x, y, z, q0, s0, re, sc, dt, 1, bcs, elliptic="EllipticOrder=CompactDirect6", ini=ini)

    def make_oracle():
        go = [O.FdmPlan(x, True, True), O.FdmPlan.from_tables(tab, mode2=O.FDM_COM6_DIRECT), O.FdmPlan(z, True, True)]
        return DnsOracle(x, y, z, nscal=1, visc=1.0 / re, schmidt=(sc,), yuniform=False, plans=go, gy_elliptic=go[1])
    kdt, kco = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0]
    sched = [(dt * kdt[k], kco[k] if k < 2 else 1.0, k < 2) for k in range(3)]
    B, S = substep_scatter(make_oracle, q0, s0, sched, nsamples=1)
    for i in range(3):
        assert rel_err(q1[i], B[2]["q"][i]) <= bound(S[2]["q"][i]), ("q", i, rel_err(q1[i], B[2]["q"][i]), S[2]["q"][i])
    assert rel_err(s1[0], B[2]["s"][0]) <= bound(S[2]["s"][0])


@pytest.mark.gpu_extra
@pytest.mark.parametrize("divergence", ["remove", "none"])
def test_fortran_rk_driver_staggered_pressure(tmp_path, divergence):
    """[Staggering] StaggerHorizontalPressure = yes (examples/Case92-93) and [Main] TermDivergence read from tlab.ini: the reference's own
    FDM_Initialize builds g%intl and the interpolatory wavenumbers, the drop-in OPR_Partial_AMD_Plan hands them on (tlab_fdm_plan_set_stagger),
    and the device RHS takes the staggered branch -- against the oracle's restatement of rhs_global_incompressible_1.f90."""
    import numpy as np
    from conftest import rel_err
    from scatter import substep_scatter, bound
    from oracle.tlab_oracle_rhs import DnsOracle
    _need_rk()
    nx, ny, nz = 64, 40, 32
    x = np.arange(nx) / nx * 2.0
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    rng = np.random.default_rng(92)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wall = np.sin(np.pi * Y)
    q0 = [((np.sin(np.pi * X + k) * np.cos(2 * np.pi * Z) + 0.1 * rng.uniform(-1, 1, X.shape)) * wall).ravel() for k in range(3)]
    s0 = [(np.cos(np.pi * X) * Y + 0.1 * rng.uniform(-1, 1, X.shape)).ravel()]
    re, sc, dt = 800.0, 0.7, 2e-3
    bcs = ["VelocityJmin=noslip", "VelocityJmax=noslip", "Scalar1Jmin=dirichlet", "Scalar1Jmax=dirichlet"]
    ini = INI.replace("{elliptic}", "TermDivergence=%s\n{elliptic}" % divergence) + "\n[Staggering]\nStaggerHorizontalPressure=yes\n"
    q1, s1, _ = run_rk_driver(str(tmp_path), x, y, z, q0, s0, re, sc, dt, 1, bcs, ini=ini)

    def make_oracle():
        o = DnsOracle(x, y, z, nscal=1, visc=1.0 / re, schmidt=(sc,), yuniform=False, stagger=True)
        o.remove_divergence = divergence == "remove"
        return o
    kdt, kco = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0]
    sched = [(dt * kdt[k], kco[k] if k < 2 else 1.0, k < 2) for k in range(3)]
    B, S = substep_scatter(make_oracle, q0, s0, sched, nsamples=1)
    for i in range(3):
        assert rel_err(q1[i], B[2]["q"][i]) <= bound(S[2]["q"][i]), ("q", i, rel_err(q1[i], B[2]["q"][i]), S[2]["q"][i])
    assert rel_err(s1[0], B[2]["s"][0]) <= bound(S[2]["s"][0])
    # and the staggered run is not the collocated one
    C, _ = substep_scatter(lambda: DnsOracle(x, y, z, nscal=1, visc=1.0 / re, schmidt=(sc,), yuniform=False), q0, s0, sched, nsamples=0)
    assert rel_err(q1[0], C[2]["q"][0]) > 1e-9


def test_unchanged_time_loop_runs_the_fused_substep_bit_for_bit(tmp_path):
    """The UNPATCHED time loop (RHS_GLOBAL_INCOMPRESSIBLE_1, then DAXPY per field, then DSCAL per field: time.f90:612-664, :272-297; `hq = 0` through
    TLab_AMD_Zero) with the library's deferred tail (csrc/deferred.cpp, the Fortran host's default): every substep ran as ONE
    tlab_time_substep_incompressible_explicit -- the fields equal those of the patched host (-DTLAB_AMD_FUSED_SUBSTEP) to the bit, none of the BLAS
    calls was executed as a pass of its own, and the zero fills of the second step became tlab_dns_begin_step.  TLAB_AMD_DEFER=0 = the literal
    sequence: same fields to round-off (another summation order in the tail), 8 + 8 BLAS passes per full step executed."""
    import re
    import numpy as np
    from conftest import rel_err
    _need_rk()
    if not os.path.exists(RK_EXE_FUSED):
        pytest.skip("tlab_amd/fortran/_build_rk_fused/test_rk_driver not built")
    nx, ny, nz = 256, 64, 32
    x = np.arange(nx) / nx * 2.0
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    rng = np.random.default_rng(78)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wall = np.sin(np.pi * Y)
    q0 = [((np.sin(np.pi * X + k) * np.cos(2 * np.pi * Z) + 0.1 * rng.uniform(-1, 1, X.shape)) * wall).ravel() for k in range(3)]
    s0 = [(np.cos(np.pi * X) * Y + 0.1 * rng.uniform(-1, 1, X.shape)).ravel()]
    bcs = ["VelocityJmin=noslip", "VelocityJmax=noslip", "Scalar1Jmin=dirichlet", "Scalar1Jmax=dirichlet"]
    res = {}
    logs = {}
    for tag, exe, env in (("fused", RK_EXE_FUSED, {}), ("deferred", RK_EXE, {}), ("literal", RK_EXE, {"TLAB_AMD_DEFER": "0"}),
                          ("deferred, arrays where the allocator put them", RK_EXE, {"TLAB_AMD_PLACE": "0"})):
        d = tmp_path / tag
        d.mkdir()
        q1, s1, log = run_rk_driver(str(d), x, y, z, q0, s0, 1000.0, 0.7, 1e-3, 2, bcs, exe=exe, env=dict(env, TLAB_AMD_TIMING="0"))
        m = re.search(r"DEFERRED: [a-z_ ]+?((?:\s+\d+){6})\s*$", log, re.M)
        assert m, log[-1500:]
        res[tag] = (q1 + s1, [int(v) for v in m.group(1).split()])
        logs[tag] = log
    f_fused, f_def, f_lit = res["fused"][0], res["deferred"][0], res["literal"][0]
    assert all(np.array_equal(a, b) for a, b in zip(f_def, f_fused))
    # 2 steps x 3 substeps, both steps' zero fills became begin_step (the placement search of the start-up created the driver handle, so the layer is on
    # from the first statement of the loop)
    assert res["deferred"][1] == [6, 0, 2, 0, 0, 0], res["deferred"][1]
    # TLab_AMD_Place_Arrays ran (six candidates per block by default) and changed nothing but the addresses; without it the first step's fills come
    # before the driver handle exists and are executed as fills (hq and hs)
    assert "PLACEMENT: candidates 6" in logs["deferred"] and "PLACEMENT" not in logs["deferred, arrays where the allocator put them"]
    assert all(np.array_equal(a, b) for a, b in zip(res["deferred, arrays where the allocator put them"][0], f_fused))
    assert res["deferred, arrays where the allocator put them"][1] == [6, 0, 1, 0, 0, 2]
    assert res["literal"][1] == [0, 0, 0, 24, 16, 4], res["literal"][1]
    d = max(rel_err(a, b) for a, b in zip(f_lit, f_fused))
    assert 0.0 < d <= 1e-11, d


def test_operator_call_after_the_time_step_sees_the_recorded_substep_executed(tmp_path):
    """TLAB_AMD_PROBE_OPERATOR=1: after every TIME_RUNGEKUTTA() the host calls OPR_Partial_X(OPR_P1) on u through the drop-in module, with no sync
    in front -- what DNS_BOUNDS_CONTROL -> FI_INVARIANT_P does (dns_main.f90:269).  With the deferred tail the last substep of the step is only
    recorded at that point (no DSCAL follows it): the operator must make it run first.  Box and fields of the test above, 2 steps.  The PROBE lines
    (sum and maximum of |du/dx|, 17 digits) of the unpatched host equal those of the patched one character for character, and the counters are
    still those of six whole fused substeps: the probe made the record run as it was, neither early in pieces nor not at all.  The literal
    sequence (TLAB_AMD_DEFER=0) has nothing pending; its lines are printed."""
    import re
    import numpy as np
    _need_rk()
    if not os.path.exists(RK_EXE_FUSED):
        pytest.skip("tlab_amd/fortran/_build_rk_fused/test_rk_driver not built")
    # the drivers are built from the reference's files: where the reference is absent build() puts back prebuilt ones (oracle/_ref/fortran), and
    # those may predate the switch (as tests/test_gpu_monitors.py finds for TLAB_AMD_MONITORS): such drivers are not the ones this test is about
    for exe in (RK_EXE, RK_EXE_FUSED):
        with open(exe, "rb") as f:
            if b"TLAB_AMD_PROBE_OPERATOR" not in f.read():
                pytest.skip("%s is a prebuilt driver from before TLAB_AMD_PROBE_OPERATOR: rebuild it where the reference is" % os.path.relpath(exe, ROOT))
    nx, ny, nz = 256, 64, 32
    x = np.arange(nx) / nx * 2.0
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    rng = np.random.default_rng(78)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wall = np.sin(np.pi * Y)
    q0 = [((np.sin(np.pi * X + k) * np.cos(2 * np.pi * Z) + 0.1 * rng.uniform(-1, 1, X.shape)) * wall).ravel() for k in range(3)]
    s0 = [(np.cos(np.pi * X) * Y + 0.1 * rng.uniform(-1, 1, X.shape)).ravel()]
    bcs = ["VelocityJmin=noslip", "VelocityJmax=noslip", "Scalar1Jmin=dirichlet", "Scalar1Jmax=dirichlet"]
    fields, probes, counters = {}, {}, {}
    for tag, exe, env in (("fused", RK_EXE_FUSED, {}), ("deferred", RK_EXE, {}), ("literal", RK_EXE, {"TLAB_AMD_DEFER": "0"})):
        d = tmp_path / tag
        d.mkdir()
        q1, s1, _ = run_rk_driver(str(d), x, y, z, q0, s0, 1000.0, 0.7, 1e-3, 2, bcs, exe=exe,
                                  env=dict(env, TLAB_AMD_TIMING="0", TLAB_AMD_PROBE_OPERATOR="1"))
        log = open(os.path.join(str(d), "tlab.log")).read()
        probes[tag] = re.findall(r"PROBE: itime\s+\d+\s+sum\s+\S+\s+max\s+\S+", log)
        m = re.search(r"DEFERRED: [a-z_ ]+?((?:\s+\d+){6})\s*$", log, re.M)
        assert m, log[-1500:]
        fields[tag], counters[tag] = q1 + s1, [int(v) for v in m.group(1).split()]
        print(tag, counters[tag], probes[tag])
    assert len(probes["fused"]) == 2 and probes["fused"][0] != probes["fused"][1], probes["fused"]      # one line per step, and u moves
    assert probes["deferred"] == probes["fused"], (probes["deferred"], probes["fused"])
    assert counters["deferred"] == [6, 0, 2, 0, 0, 0], counters["deferred"]
    assert all(np.array_equal(a, b) for a, b in zip(fields["deferred"], fields["fused"]))
    # nothing is ever pending in the literal sequence: its lines are those of fields that differ by rounding (no bound is set on a derivative here)
    assert len(probes["literal"]) == 2 and counters["literal"] == [0, 0, 0, 24, 16, 4], (probes["literal"], counters["literal"])


@pytest.mark.parametrize("route,nx,ny,nz", [("TLAB_AMD_FORCE_SLAB", 128, 32, 64), ("TLAB_AMD_FORCE_PENCIL", 64, 32, 32)])
def test_unchanged_time_loop_behind_the_decomposed_drivers(tmp_path, route, nx, ny, nz):
    """The deferred tail behind tlab_slab_dns / tlab_pencil_dns (tlab_deferred_slab_rhs / _pencil_rhs): the unpatched loop's RHS + DAXPY + DSCAL calls
    become tlab_slab_dns_substep / tlab_pencil_dns_substep -- the fields equal those of the patched host to the bit, no BLAS pass runs on its own."""
    import re
    import numpy as np
    _need_rk()
    if not os.path.exists(RK_EXE_FUSED):
        pytest.skip("tlab_amd/fortran/_build_rk_fused/test_rk_driver not built")
    x = np.arange(nx) / nx * 2.0
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    rng = np.random.default_rng(79)
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    wall = np.sin(np.pi * Y)
    q0 = [((np.sin(np.pi * X + k) * np.cos(2 * np.pi * Z) + 0.1 * rng.uniform(-1, 1, X.shape)) * wall).ravel() for k in range(3)]
    s0 = [(np.cos(np.pi * X) * Y + 0.1 * rng.uniform(-1, 1, X.shape)).ravel()]
    bcs = ["VelocityJmin=noslip", "VelocityJmax=noslip", "Scalar1Jmin=dirichlet", "Scalar1Jmax=dirichlet"]
    res = {}
    for tag, exe in (("fused", RK_EXE_FUSED), ("deferred", RK_EXE)):
        d = tmp_path / tag
        d.mkdir()
        q1, s1, log = run_rk_driver(str(d), x, y, z, q0, s0, 1000.0, 0.7, 1e-3, 2, bcs, exe=exe, env={route: "1", "TLAB_AMD_TIMING": "0"})
        m = re.search(r"DEFERRED: [a-z_ ]+?((?:\s+\d+){6})\s*$", log, re.M)
        assert m, log[-1500:]
        res[tag] = (q1 + s1, [int(v) for v in m.group(1).split()])
    assert all(np.array_equal(a, b) for a, b in zip(res["deferred"][0], res["fused"][0]))
    fused_n, literal_n, begins, eaxpy, escal, ezero = res["deferred"][1]
    # the first step's zero fills come before the driver handle exists and run as fills; everything else rides
    assert (fused_n, literal_n, eaxpy, escal) == (6, 0, 0, 0) and begins == 1 and ezero == 2, res["deferred"][1]
    assert res["fused"][1] == [0, 0, 0, 0, 0, 0]
