"""tests/particles_oracle.py pinned by properties that do not depend on the restatement being right (no GPU): FIELD_TO_PARTICLE and LOCATE_Y cannot
be reached through oracle/ref_lib.py, so the oracle the device kernel is held to bit for bit is itself held to what trilinear weights, a bisection,
a uniform flow and a linear relaxation must give."""
import numpy as np
import pytest

from cases import KDT, KCO, grids
from particles_oracle import Particles, locate_y, PART_TRACER, PART_INERTIA, BCS_NONE


def _rk(name):
    if name == "rk3":
        return KDT, KCO, 3
    from tlab_amd.dns import rk_coefficients, RKM_EXP4
    kdt, kco = rk_coefficients(RKM_EXP4)
    return kdt, kco, 4


def _stretched(nx=20, ny=12, nz=8):
    x, y, z = grids(nx, ny, nz, True)
    return x, y, z


def _linear(x, y, z, coef):
    a, b, c, d = coef
    Z, Y, X = np.meshgrid(z, y, x, indexing="ij")
    return (a + b * X + c * Y + d * Z).ravel()


def test_trilinear_weights_reproduce_a_linear_field():
    """f = a + b x + c y + d z on the nodes of a stretched 20 x 12 x 8 grid: the interpolated value is f at the particle within 1e-13 (eight products
    and seven adds of O(1) numbers; measured 1.3e-15) for x < x(nx), z < z(nz); in the seam cell it is the linear blend of the planes nx and 1."""
    x, y, z = _stretched()
    coef = (0.3, 0.7, -1.1, 0.45)
    f = _linear(x, y, z, coef)
    rng = np.random.default_rng(5)
    n = 5000
    P = Particles(x, y, z)
    P.set([rng.uniform(x[0], x[-1], n), rng.uniform(y[0], y[-1], n), rng.uniform(z[0], z[-1], n)])
    assert (P.l_q[0] < x[-1]).all() and (P.l_q[2] < z[-1]).all()
    got = P.interpolate(f, np.zeros(n))
    want = coef[0] + coef[1] * P.l_q[0] + coef[2] * P.l_q[1] + coef[3] * P.l_q[2]
    e = float(np.abs(got - want).max())
    print("interior: %.2e" % e)
    assert e <= 1e-13
    # the x seam: x(nx) <= x < scale blends plane nx with plane 1
    xs = rng.uniform(x[-1], x[0] + P.sx, n)
    xs[0] = x[-1]
    P.set([xs, P.l_q[1], P.l_q[2]])
    got = P.interpolate(f, np.zeros(n))
    t = (xs - x[-1]) / (x[0] + P.sx - x[-1])
    want = coef[0] + coef[1] * ((1 - t) * x[-1] + t * x[0]) + coef[2] * P.l_q[1] + coef[3] * P.l_q[2]
    e = float(np.abs(got - want).max())
    print("x seam: %.2e" % e)
    assert e <= 1e-13
    # ... and the z seam
    zs = rng.uniform(z[-1], z[0] + P.sz, n)
    P.set([rng.uniform(x[0], x[-1], n), P.l_q[1], zs])
    got = P.interpolate(f, np.zeros(n))
    t = (zs - z[-1]) / (z[0] + P.sz - z[-1])
    want = coef[0] + coef[1] * P.l_q[0] + coef[2] * P.l_q[1] + coef[3] * ((1 - t) * z[-1] + t * z[0])
    e = float(np.abs(got - want).max())
    print("z seam: %.2e" % e)
    assert e <= 1e-13
    # the interpolation ADDS onto its target
    assert float(np.abs(P.interpolate(f, np.full(n, 2.0)) - (got + 2.0)).max()) <= 1e-13


def test_bilinear_branch_ignores_z():
    x, y, _ = _stretched()
    f = _linear(x, y, np.zeros(1), (0.3, 0.7, -1.1, 0.0))
    rng = np.random.default_rng(6)
    n = 2000
    P = Particles(x, y, np.zeros(1))
    P.set([rng.uniform(x[0], x[-1], n), rng.uniform(y[0], y[-1], n), rng.uniform(-5.0, 5.0, n)])
    want = 0.3 + 0.7 * P.l_q[0] - 1.1 * P.l_q[1]
    assert float(np.abs(P.interpolate(f, np.zeros(n)) - want).max()) <= 1e-13


def test_locate_y_against_searchsorted():
    """strictly inside cells the loop is clip(searchsorted(y, yp, 'right'), 1, ny - 1); the ends go to the first and the last cell"""
    _, y, _ = _stretched()
    ny = len(y)
    rng = np.random.default_rng(7)
    yp = rng.uniform(y[0], y[-1], 5000)
    yp = yp[~np.isin(yp, y)]
    assert np.array_equal(locate_y(yp, y), np.clip(np.searchsorted(y, yp, "right"), 1, ny - 1))
    assert locate_y([y[0]], y)[0] == 1 and locate_y([y[-1]], y)[0] == ny - 1
    out = locate_y(np.concatenate([y, [y[0] - 1.0, y[-1] + 1.0, np.nan]]), y)
    assert out.min() >= 1 and out.max() <= ny - 1                      # every path of the bisection ends inside


@pytest.mark.parametrize("scheme", ["rk3", "rk4"])
def test_uniform_flow_moves_tracers_by_dtime_times_velocity(scheme):
    """one full step of each scheme in q = (U, V, W): every tracer moves by dtime (U, V, W) modulo the wraps, within 1e-14 of the box size -- dte,
    the scaling of l_hq and the wraps together"""
    kdt, kco, _ = _rk(scheme)
    x, y, z = _stretched()
    n = len(x) * len(y) * len(z)
    U = (0.83, -0.21, -1.37)
    q = [np.full(n, v) for v in U]
    rng = np.random.default_rng(8)
    m = 3000
    P = Particles(x, y, z, bcs=BCS_NONE)
    p0 = [rng.uniform(x[0], x[0] + P.sx, m), rng.uniform(y[0] + 0.2, y[-1] - 0.2, m), rng.uniform(z[0], z[0] + P.sz, m)]
    P.set(p0)
    dtime = 0.11
    P.step(lambda k: q, dtime, kdt, kco)
    wrapped = 0
    for i, (s, lo) in enumerate(((P.sx, x[0]), (None, None), (P.sz, z[0]))):
        want = p0[i] + dtime * U[i]
        if s is not None:
            w = np.where(want > lo + s, want - s, np.where(want < lo, want + s, want))
            wrapped += int((w != want).sum())
            want = w
        box = (P.sx, P.sy, P.sz)[i]
        e = float(np.abs(P.l_q[i] - want).max() / box)
        print("%s direction %d: %.2e of the box" % (scheme, i, e))
        assert e <= 1e-14, (scheme, i, e)
    assert wrapped > 100                                                # both wraps were exercised
    assert np.array_equal(P.nodes, locate_y(P.l_q[1], y))


@pytest.mark.parametrize("scheme", ["rk3", "rk4"])
def test_inertial_particle_relaxes_exponentially(scheme):
    """fluid at rest, settling = 0: v_p(t) = v_p(0) exp(-t / stokes) to the scheme's order -- halving dtime reduces the error by at least
    2^(order - 0.5)"""
    kdt, kco, order = _rk(scheme)
    x, y, z = _stretched()
    n = len(x) * len(y) * len(z)
    q = [np.zeros(n)] * 3
    stokes, T = 0.5, 0.4
    v0 = np.array([0.3, -0.2, 0.25])
    errs = []
    for steps in (4, 8):
        P = Particles(x, y, z, type=PART_INERTIA, stokes=stokes, settling=0.0)
        P.set([np.array([0.9]), np.array([0.5]), np.array([0.4])] + [np.array([v]) for v in v0])
        for _ in range(steps):
            P.step(lambda k: q, T / steps, kdt, kco)
        got = np.array([P.l_q[3 + i][0] for i in range(3)])
        errs.append(float(np.abs(got - v0 * np.exp(-T / stokes)).max()))
        # the position integrates the velocity: x(T) = x0 + v0 stokes (1 - exp(-T / stokes))
        assert abs(P.l_q[0][0] - (0.9 + v0[0] * stokes * (1 - np.exp(-T / stokes)))) <= 10 * max(errs[-1], 1e-15)
    print("%s: errors %.3e -> %.3e, ratio %.1f" % (scheme, errs[0], errs[1], errs[0] / errs[1]))
    assert errs[0] > 1e-12                                               # (not already at rounding level: the ratio means something)
    assert errs[0] / errs[1] >= 2.0 ** (order - 0.5), (scheme, errs)


def test_particles_module_compiles_against_the_c_interfaces(tmp_path):
    """tlab_amd/fortran/tlab_amd_particles.f90 depends on TLab_AMD_C alone, and a caller shaped like the patched TIME_SUBSTEP_PARTICLE (module arrays
    of rank 2, l_g%nodes, a logical for the scaling) compiles against it"""
    import os
    import re
    import shutil
    import subprocess
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    fortran = os.path.join(root, "tlab_amd", "fortran")
    fc = shutil.which("amdflang")
    mod = os.path.join(root, "oracle", "_ref", "mod")                   # TLab_AMD_Check of tlab_amd_c.f90 writes through the reference's TLab_WorkFlow
    if fc is None or not os.path.isdir(mod):
        pytest.skip("amdflang or the reference's module files (oracle/_ref/mod) are not here")
    run = lambda *a: subprocess.run([fc, "-cpp", "-O2", "-I", mod, "-module-dir", str(tmp_path), "-c", *a], cwd=tmp_path,      # noqa: E731
                                    capture_output=True, text=True)
    r = run(os.path.join(fortran, "tlab_amd_c.f90"), "-o", str(tmp_path / "c.o"))
    assert r.returncode == 0, r.stderr
    r = run("-I", str(tmp_path), os.path.join(fortran, "tlab_amd_particles.f90"), "-o", str(tmp_path / "p.o"))
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(fortran, "tlab_amd_particles.f90")).read()
    assert re.findall(r"^\s*use\s+(\w+)", src, flags=re.M | re.I) == ["TLab_AMD_C"]
    assert max(len(l) for l in src.splitlines()) <= 160
    (tmp_path / "caller.f90").write_text(
        "subroutine caller(dns, q, l_q, l_hq, nodes, tags, n, isize_part, np)\n"
        "    use TLab_AMD_C\n"
        "    use TLab_AMD_Particles\n"
        "    type(c_ptr) :: dns\n"
        "    integer :: n, isize_part, np, part_type, part_bcs, rkm_substep, rkm_endstep, inb_part\n"
        "    real(c_double) :: q(n, 3), l_q(isize_part, *), l_hq(isize_part, *), stokes, settling, dte, kco(5)\n"
        "    integer(c_int) :: nodes(isize_part)\n"
        "    integer(c_long_long) :: tags(isize_part)\n"
        "    call TLab_AMD_Locate_Particles(dns, part_type, part_bcs, stokes, settling, np, isize_part, l_q, nodes)\n"
        "    call TLab_AMD_Substep_Particle(dns, part_type, part_bcs, stokes, settling, dte, kco(rkm_substep), rkm_substep < rkm_endstep, &\n"
        "                                   np, isize_part, inb_part, q, l_q, l_hq, nodes)\n"
        "    call TLab_AMD_Sort_Particles(dns, np, isize_part, inb_part, l_q, l_hq, nodes, tags)\n"
        "end subroutine caller\n")
    r = run("-I", str(tmp_path), str(tmp_path / "caller.f90"), "-o", str(tmp_path / "caller.o"))
    assert r.returncode == 0, r.stderr


def test_settling_adds_a_terminal_velocity():
    """fluid at rest: dv/dt = -(v + settling) / stokes, so v -> -settling"""
    x, y, z = _stretched()
    n = len(x) * len(y) * len(z)
    q = [np.zeros(n)] * 3
    P = Particles(x, y, z, type=PART_INERTIA, bcs=BCS_NONE, stokes=0.05, settling=0.01)
    P.set([np.array([0.9]), np.array([0.5]), np.array([0.4])] + [np.zeros(1)] * 3)
    for _ in range(200):
        P.step(lambda k: q, 0.01, KDT, KCO)
    assert abs(P.l_q[4][0] + 0.01) <= 1e-12 and P.l_q[3][0] == 0.0 and P.l_q[5][0] == 0.0
