"""The plane statistics without a GPU: properties that pin the numpy restatement (tests/averages_oracle.py), the host branch of the four entry
points against it bit for bit (tlab_init is never called here: every array is host memory, as in tests/test_monitors_host.py), the argument
checks, and the Fortran module against the C interfaces."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import averages_oracle as A

SHAPES = [(20, 12, 8), (70, 33, 9), (20, 12, 1)]
EINVAL = -1
vp = ctypes.c_void_p


def _fields(shape, n, seed):
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    off = 10.0 * np.cos(np.arange(ny))[None, :, None]
    return [np.ascontiguousarray(rng.uniform(-1, 1, (nz, ny, nx)) + (i + 1) * off) for i in range(n)]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_constant_planes_return_their_constants():
    nx, ny, nz = 20, 12, 8
    c = 0.25 * np.arange(ny) - 1.0                                       # dyadic: every partial sum is exact
    a = np.broadcast_to(c[None, :, None], (nz, ny, nx)).copy()
    assert np.array_equal(A.avg_ik_v(a), c)
    for imom in (1, 2, 3, 4):
        assert np.array_equal(A.avg1v2d_v(a, imom), c ** imom)
    assert np.array_equal(A.exact_mean(a), c)


def test_sine_line_gives_the_moments_of_a_sine():
    nx, ny, nz, m, amp = 20, 5, 3, 3, 0.7
    U = 1.0 + 0.5 * np.arange(ny)
    u = U[None, :, None] + amp * np.sin(2 * np.pi * m * np.arange(nx) / nx)[None, None, :] + np.zeros((nz, ny, nx))
    z = np.zeros(ny)
    t = A.flow_terms(u, np.zeros_like(u), np.zeros_like(u), None, U, z, z, None)
    Rxx, rU3, rU4 = (A.avg_ik_v(t[k]) for k in ("Rxx", "rU3", "rU4"))
    assert np.abs(Rxx - amp ** 2 / 2).max() <= 1e-14 * amp ** 2 / 2
    assert np.abs(rU3).max() <= 1e-14 * amp ** 3
    assert np.abs(rU4 - 3 * amp ** 4 / 8).max() <= 1e-14 * 3 * amp ** 4 / 8


def test_scal_with_s_equal_u_reproduces_flow():
    u, v, w = _fields((20, 12, 8), 3, 1)
    fU, fV, fW = (A.avg_ik_v(a) for a in (u, v, w))
    F = A.flow_terms(u, v, w, None, fU, fV, fW, None)
    S = A.scal_terms(u, u, v, w, None, fU, fU, fV, fW, None)
    for s, f in (("rS2", "Rxx"), ("rS3", "rU3"), ("rS4", "rU4"), ("Rsv", "Rxy")):
        assert np.array_equal(A.avg_ik_v(S[s]), A.avg_ik_v(F[f])), (s, f)


# ---- the host branch of the entry points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_host_branch_equals_the_restatement_bit_for_bit(shape):
    import tlab_amd.operators as T
    nx, ny, nz = shape
    s, u, v, w, p = _fields(shape, 5, 2)
    nine = _fields(shape, 9, 3)
    got = T.avg_ik_v(nx, ny, nz, nine)                                   # nine fields: two groups
    assert got.shape == (9, ny)
    for f in range(9):
        assert np.array_equal(got[f], A.avg_ik_v(nine[f])), f
    for imom in (1, 2, 3, 4):
        assert np.array_equal(T.avg1v2d_v(nx, ny, nz, imom, u), A.avg1v2d_v(u, imom)), imom
    fS, fU, fV, fW, rP = (A.avg_ik_v(a) for a in (s, u, v, w, p))
    for pp, pm in ((None, None), (p, rP)):
        got = T.avg_moments_flow(nx, ny, nz, u, v, w, fU, fV, fW, pp, pm)
        terms = A.flow_terms(u, v, w, pp, fU, fV, fW, pm)
        assert tuple(terms) == A.FLOW_NAMES + (A.FLOW_NAMES_P if pp is not None else ()) == T.FLOW_MOMENTS + (T.FLOW_MOMENTS_P if pp is not None else ())
        ref = A.averages(terms)
        assert got.shape == ref.shape
        for name, g, r in zip(terms, got, ref):
            assert np.array_equal(g, r), ("flow", name, float(np.abs(g - r).max()))
        got = T.avg_moments_scal(nx, ny, nz, s, u, v, w, fS, fU, fV, fW, pp, pm)
        terms = A.scal_terms(s, u, v, w, pp, fS, fU, fV, fW, pm)
        assert tuple(terms) == A.SCAL_NAMES + (A.SCAL_NAMES_P if pp is not None else ()) == T.SCAL_MOMENTS + (T.SCAL_MOMENTS_P if pp is not None else ())
        ref = A.averages(terms)
        assert got.shape == ref.shape
        for name, g, r in zip(terms, got, ref):
            assert np.array_equal(g, r), ("scal", name, float(np.abs(g - r).max()))


def test_profiles_go_to_columns_ld_apart():
    """column f of avg starts at avg + f*ldavg (mean2d(1, k) of the host): what lies between the columns is not touched"""
    import tlab_amd
    L = tlab_amd.load()
    nx, ny, nz, ld = 20, 12, 8, 17
    u, v = _fields((nx, ny, nz), 2, 4)
    out = np.full((2, ld), -7.0)
    ptrs = (vp * 2)(u.ctypes.data, v.ctypes.data)
    assert L.tlab_avg_ik_v(nx, ny, nz, 2, ptrs, vp(out.ctypes.data), ld) == 0
    assert np.array_equal(out[0, :ny], A.avg_ik_v(u)) and np.array_equal(out[1, :ny], A.avg_ik_v(v))
    assert np.all(out[:, ny:] == -7.0)


def test_argument_errors_are_refused():
    import tlab_amd
    L = tlab_amd.load()
    nx, ny, nz = 6, 4, 3
    a = np.ones((nz, ny, nx))
    prof = np.zeros(ny)
    out = np.zeros((22, ny))
    A_, P_, O_ = vp(a.ctypes.data), vp(prof.ctypes.data), vp(out.ctypes.data)
    one = (vp * 1)(a.ctypes.data)
    assert L.tlab_avg_ik_v(nx, ny, nz, 1, one, O_, ny) == 0
    for bad in ((0, ny, nz), (nx, 0, nz), (nx, ny, 0), (-1, ny, nz)):
        assert L.tlab_avg_ik_v(*bad, 1, one, O_, ny) == EINVAL
        assert L.tlab_avg1v2d_v(*bad, 1, A_, O_) == EINVAL
        assert L.tlab_avg_moments_flow(*bad, A_, A_, A_, None, P_, P_, P_, None, O_, ny) == EINVAL
        assert L.tlab_avg_moments_scal(*bad, A_, A_, A_, A_, None, P_, P_, P_, P_, None, O_, ny) == EINVAL
    assert L.tlab_avg_ik_v(nx, ny, nz, 0, one, O_, ny) == EINVAL              # nf < 1
    assert L.tlab_avg_ik_v(nx, ny, nz, 1, None, O_, ny) == EINVAL
    assert L.tlab_avg_ik_v(nx, ny, nz, 1, one, None, ny) == EINVAL
    assert L.tlab_avg_ik_v(nx, ny, nz, 1, (vp * 1)(None), O_, ny) == EINVAL
    assert L.tlab_avg_ik_v(nx, ny, nz, 1, one, O_, ny - 1) == EINVAL          # columns that overlap
    for imom in (0, 5, -1):
        assert L.tlab_avg1v2d_v(nx, ny, nz, imom, A_, O_) == EINVAL
    assert L.tlab_avg1v2d_v(nx, ny, nz, 2, None, O_) == EINVAL
    assert L.tlab_avg1v2d_v(nx, ny, nz, 2, A_, None) == EINVAL
    good = [A_, A_, A_, None, P_, P_, P_, None, O_]
    assert L.tlab_avg_moments_flow(nx, ny, nz, *good, ny) == 0
    for i in (0, 1, 2, 4, 5, 6, 8):
        args = list(good)
        args[i] = None
        assert L.tlab_avg_moments_flow(nx, ny, nz, *args, ny) == EINVAL, i
    assert L.tlab_avg_moments_flow(nx, ny, nz, A_, A_, A_, A_, P_, P_, P_, None, O_, ny) == EINVAL      # p without rP
    assert L.tlab_avg_moments_flow(nx, ny, nz, A_, A_, A_, None, P_, P_, P_, P_, O_, ny) == EINVAL      # rP without p
    good = [A_, A_, A_, A_, None, P_, P_, P_, P_, None, O_]
    assert L.tlab_avg_moments_scal(nx, ny, nz, *good, ny) == 0
    for i in (0, 1, 2, 3, 5, 6, 7, 8, 10):
        args = list(good)
        args[i] = None
        assert L.tlab_avg_moments_scal(nx, ny, nz, *args, ny) == EINVAL, i
    assert L.tlab_avg_moments_scal(nx, ny, nz, A_, A_, A_, A_, A_, P_, P_, P_, P_, None, O_, ny) == EINVAL
    assert b"tlab_avg_moments_scal" in L.tlab_last_error()


# ---- the Fortran module ---------------------------------------------------------------------------------------------------------------------
def test_averages_module_compiles_against_the_c_interfaces(tmp_path):
    """tlab_amd/fortran/tlab_amd_averages.f90 depends on TLab_AMD_C alone (outside its USE_MPI blocks, which use what the reference's module
    Averages uses there), and a caller shaped like AVG_FLOW_XZ's call sites (fields of rank 3 behind pointers, the profiles as macros over mean2d(jmax, nv), wrk1d of rank 2)
    compiles against it"""
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
    r = run("-I", str(tmp_path), os.path.join(fortran, "tlab_amd_averages.f90"), "-o", str(tmp_path / "a.o"))
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(fortran, "tlab_amd_averages.f90")).read()
    serial = re.sub(r"^#ifdef USE_MPI\n.*?^#endif\n", "", src, flags=re.M | re.S)
    assert re.findall(r"^\s*use\s+(\w+)", serial, flags=re.M | re.I) == ["TLab_AMD_C"]
    assert max(len(l) for l in src.splitlines()) <= 160
    (tmp_path / "caller.f90").write_text(
        "subroutine caller(q, s, dudz, mean2d, wrk1d, imax, jmax, kmax, nv)\n"
        "    use TLab_AMD_C\n"
        "    use TLab_AMD_Averages\n"
        "    integer :: imax, jmax, kmax, nv, ig(16)\n"
        "    real(c_double), target :: q(imax, jmax, kmax, 3), s(imax, jmax, kmax), dudz(imax, jmax, kmax), mean2d(jmax, nv), wrk1d(jmax, 2)\n"
        "    real(c_double), pointer :: u(:, :, :), v(:, :, :), w(:, :, :), p_loc(:, :, :)\n"
        "#define rU(j) mean2d(j,ig(1)+1)\n"
        "#define rV(j) mean2d(j,ig(1)+2)\n"
        "#define rW(j) mean2d(j,ig(1)+3)\n"
        "#define rP(j) mean2d(j,ig(1)+4)\n"
        "#define rS(j) mean2d(j,ig(1)+5)\n"
        "#define Rxx(j) mean2d(j,ig(2))\n"
        "#define rS2(j) mean2d(j,ig(3))\n"
        "    u => q(:, :, :, 1); v => q(:, :, :, 2); w => q(:, :, :, 3); p_loc => dudz\n"
        "    call TLab_AMD_AVG_IK_V(imax, jmax, kmax, u, rU(1), wrk1d)\n"
        "    call TLab_AMD_AVG_IK_V(imax, jmax, kmax, v, rV(1), wrk1d)\n"
        "    call TLab_AMD_AVG_IK_V(imax, jmax, kmax, w, rW(1), wrk1d)\n"
        "    call TLab_AMD_AVG_IK_V(imax, jmax, kmax, p_loc, rP(1), wrk1d)\n"
        "    call TLab_AMD_AVG1V2D_V(imax, jmax, kmax, 2, s, rS(1), wrk1d)\n"
        "    call TLab_AMD_Avg_Moments_Flow(imax, jmax, kmax, u, v, w, rU(1), rV(1), rW(1), Rxx(1), p_loc, rP(1))\n"
        "    call TLab_AMD_Avg_Moments_Flow(imax, jmax, kmax, u, v, w, rU(:), rV(:), rW(:), Rxx(1))\n"
        "    call TLab_AMD_Avg_Moments_Scal(imax, jmax, kmax, s, u, v, w, rS(1), rU(1), rV(1), rW(1), rS2(1), p_loc, rP(1))\n"
        "end subroutine caller\n")
    r = run("-I", str(tmp_path), str(tmp_path / "caller.f90"), "-o", str(tmp_path / "caller.o"))
    assert r.returncode == 0, r.stderr
