"""The gradient statistics without a GPU: properties that pin the numpy restatement (tests/gradient_stats_oracle.py), the host branch of
tlab_avg_gradients_flow, tlab_avg_ugradp and tlab_avg_gradients_scal against it bit for bit (tlab_init is never called here: every array is host
memory), the column layout, the argument checks, and the Fortran module against the C interfaces."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gradient_stats_oracle as G

SHAPES = [(20, 12, 8), (70, 33, 9), (20, 12, 1)]
EINVAL = -1
vp = ctypes.c_void_p


def _fields(shape, n, seed):
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    off = 2.0 * np.cos(np.arange(ny))[None, :, None]
    return [np.ascontiguousarray(rng.uniform(-1, 1, (nz, ny, nx)) + (0.2 * i + 1) * off) for i in range(n)]


def _profiles(ny, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, ny) for _ in range(n)]


def _const(shape, c):
    nx, ny, nz = shape
    return np.full((nz, ny, nx), float(c))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_solid_body_rotation_has_vorticity_and_no_dissipation():
    """u = -Omega z, w = Omega x (derivatives handed in): dudz = -Omega, dwdx = Omega, everything else 0.  The magnitude is 2 Omega exactly; with
    the reference's vorty = dudz - dwdx (:998) the sign is -2 Omega for this sense of rotation and +2 Omega for the opposite one (both are run).
    No variance, no dissipation, no stress"""
    shape = (20, 12, 8)
    z = np.zeros(shape[1])
    for om in (0.75, -0.75):
        g = [_const(shape, 0.0) for _ in range(9)]
        g[2], g[6] = _const(shape, -om), _const(shape, om)
        vel = [_const(shape, 0.0)] * 3
        r = G.flow_averages(g, *vel, None, z, z, z, None, z, z, z)
        assert np.array_equal(r["vorty"], np.full(shape[1], -2.0 * om)) and np.all(r["vortx"] == 0) and np.all(r["vortz"] == 0)
        for k in ("vortx2", "vorty2", "vortz2", "Phi", "Exx", "Eyy", "Ezz", "Exy", "Exz", "Eyz", "U_ii2", "Tau_yy", "Tau_xy", "Tau_yz"):
            assert np.all(r[k] == 0.0), k
        assert np.array_equal(r["U_z2"], np.full(shape[1], om * om)) and np.array_equal(r["W_x4"], np.full(shape[1], om ** 4))


def test_pure_strain_gives_its_dissipation():
    shape, a = (20, 12, 8), 0.5
    z = np.zeros(shape[1])
    g = [_const(shape, 0.0) for _ in range(9)]
    g[0], g[4] = _const(shape, a), _const(shape, -a)
    vel = [_const(shape, 0.0)] * 3
    r = G.flow_averages(g, *vel, None, z, z, z, None, z, z, z)
    one = np.ones(shape[1])
    assert np.array_equal(r["Phi"], 2 * a * a * one) and np.array_equal(r["U_x2"], a * a * one) and np.array_equal(r["V_y2"], a * a * one)
    assert np.array_equal(r["Exx"], 2 * a * a * one) and np.array_equal(r["Eyy"], 2 * a * a * one) and np.all(r["Ezz"] == 0) and np.all(r["Exy"] == 0)
    assert np.array_equal(r["Tau_yy"], -3 * a * one) and np.all(r["U_ii2"] == 0) and np.all(r["vortz"] == 0)


def test_scal_with_s_equal_u_reproduces_the_flow_chains():
    shape = (20, 12, 8)
    g = _fields(shape, 9, 1)
    rU_y, rV_y, rW_y = _profiles(shape[1], 3, 2)
    z = np.zeros(shape[1])
    F = G.flow_terms2(g, rU_y, rV_y, rW_y, z, z, z)
    S = G.scal_terms1(g[:3], rU_y)
    for d, fd in (("x", "U_x"), ("y", "U_y"), ("z", "U_z")):
        for k in (2, 3, 4):
            assert np.array_equal(G.avg_ik_v(S["S_%s%d" % (d, k)]), G.avg_ik_v(F["%s%d" % (fd, k)])), (d, k)


def test_fourth_power_is_a_chain():
    a = np.array([[[1.0 + 2.0 ** -30, 3.1, -0.7]]])
    p2, p3, p4 = G._chain(a)
    assert np.array_equal(p4, ((a * a) * a) * a)


# ---- the host branch of the entry points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_host_branch_equals_the_restatement_bit_for_bit(shape):
    import tlab_amd.operators as T
    nx, ny, nz = shape
    g = _fields(shape, 9, 3)
    s, u, v, w, p = _fields(shape, 5, 4)
    fS, fU, fV, fW, rP, rU_y, rV_y, rW_y, rS_y, fS_y = _profiles(ny, 10, 5)
    assert T.FLOW_GRADIENTS == G.FLOW_GRAD_NAMES and T.FLOW_GRADIENTS_P == G.FLOW_GRAD_NAMES_P
    assert T.SCAL_GRADIENTS == G.SCAL_GRAD_NAMES and T.SCAL_GRADIENTS_P == G.SCAL_GRAD_NAMES_P
    assert len(T.FLOW_GRADIENTS) == 50 and len(T.SCAL_GRADIENTS) == 15
    for pp, pm in ((None, None), (p, rP)):
        got = T.avg_gradients_flow(nx, ny, nz, g, u, v, w, fU, fV, fW, rU_y, rV_y, rW_y, pp, pm)
        ref = G.flow_averages(g, u, v, w, pp, fU, fV, fW, pm, rU_y, rV_y, rW_y)
        assert tuple(ref) == T.FLOW_GRADIENTS + (T.FLOW_GRADIENTS_P if pp is not None else ())
        assert got.shape == (len(ref), ny)
        for (name, r), a in zip(ref.items(), got):
            assert np.array_equal(a, r), ("flow", name, float(np.abs(a - r).max()))
        got = T.avg_gradients_scal(nx, ny, nz, g[:3], s, u, v, w, fS, fU, fV, fW, rS_y, pp, pm, fS_y if pp is not None else None)
        ref = G.scal_averages(g[:3], s, u, v, w, pp, fS, fU, fV, fW, pm, rS_y, fS_y)
        assert tuple(ref) == T.SCAL_GRADIENTS + (T.SCAL_GRADIENTS_P if pp is not None else ())
        assert got.shape == (len(ref), ny)
        for (name, r), a in zip(ref.items(), got):
            assert np.array_equal(a, r), ("scal", name, float(np.abs(a - r).max()))
    got = T.avg_ugradp(nx, ny, nz, u, v, w, g[0], g[1], g[2])
    assert np.array_equal(got, G.avg_ik_v(G.ugradp_term(u, v, w, g[0], g[1], g[2])))


def _flow_args(g, f, P, O, with_p):
    return [(vp * 9)(*[a.ctypes.data for a in g])] + [f] * 3 + [f if with_p else None] + [P] * 3 + [P if with_p else None] + [P] * 3 + [O]


def _scal_args(g, f, P, O, with_p):
    return ([(vp * 3)(*[a.ctypes.data for a in g[:3]])] + [f] * 4 + [f if with_p else None] + [P] * 4 + [P if with_p else None] + [P]
            + [P if with_p else None] + [O])


def test_columns_go_ldout_apart_and_nothing_between_them_is_touched():
    import tlab_amd
    L = tlab_amd.load()
    shape = (20, 12, 8)
    nx, ny, nz = shape
    ld = 17
    g = _fields(shape, 9, 6)
    s, u, v, w, p = _fields(shape, 5, 7)
    fS, fU, fV, fW, rP, rU_y, rV_y, rW_y, rS_y, fS_y = _profiles(ny, 10, 8)
    P_ = lambda a: vp(a.ctypes.data)      # noqa: E731
    out = np.full((56, ld), -7.0)
    assert L.tlab_avg_gradients_flow(nx, ny, nz, (vp * 9)(*[a.ctypes.data for a in g]), P_(u), P_(v), P_(w), P_(p), P_(fU), P_(fV), P_(fW), P_(rP),
                                     P_(rU_y), P_(rV_y), P_(rW_y), P_(out), ld) == 0
    ref = G.flow_averages(g, u, v, w, p, fU, fV, fW, rP, rU_y, rV_y, rW_y)
    for c, r in enumerate(ref.values()):
        assert np.array_equal(out[c, :ny], r), c
    assert np.all(out[:, ny:] == -7.0)
    out = np.full((18, ld), -7.0)
    assert L.tlab_avg_gradients_scal(nx, ny, nz, (vp * 3)(*[a.ctypes.data for a in g[:3]]), P_(s), P_(u), P_(v), P_(w), P_(p), P_(fS), P_(fU),
                                     P_(fV), P_(fW), P_(rP), P_(rS_y), P_(fS_y), P_(out), ld) == 0
    ref = G.scal_averages(g[:3], s, u, v, w, p, fS, fU, fV, fW, rP, rS_y, fS_y)
    for c, r in enumerate(ref.values()):
        assert np.array_equal(out[c, :ny], r), c
    assert np.all(out[:, ny:] == -7.0)
    out = np.full((50 + 2, ld), -7.0)                                   # without p: 50 columns and not one more
    assert L.tlab_avg_gradients_flow(nx, ny, nz, (vp * 9)(*[a.ctypes.data for a in g]), P_(u), P_(v), P_(w), None, P_(fU), P_(fV), P_(fW), None,
                                     P_(rU_y), P_(rV_y), P_(rW_y), P_(out), ld) == 0
    assert np.all(out[50:] == -7.0) and np.all(out[:50, :ny] != -7.0)


def test_single_passes_equal_the_columns_of_the_whole_call():
    """tlab_avg_gradients_pass: a pass handed the profiles of the pass before it gives the bits of the whole call (what the Fortran module does
    between its MPI reductions)"""
    import tlab_amd
    import tlab_amd.operators as T
    L = tlab_amd.load()
    shape = (70, 33, 9)
    nx, ny, nz = shape
    g = _fields(shape, 9, 9)
    s, u, v, w, p = _fields(shape, 5, 10)
    fS, fU, fV, fW, rP, rU_y, rV_y, rW_y, rS_y, fS_y = _profiles(ny, 10, 11)
    arr = lambda xs: (vp * len(xs))(*[a.ctypes.data for a in xs])      # noqa: E731
    whole = T.avg_gradients_flow(nx, ny, nz, g, u, v, w, fU, fV, fW, rU_y, rV_y, rW_y, p, rP)
    out = np.zeros((56, ny))
    col = lambda c: vp(out[c].ctypes.data)      # noqa: E731
    assert L.tlab_avg_gradients_pass(1, 0, nx, ny, nz, arr(g), None, col(0), ny) == 0
    assert L.tlab_avg_gradients_pass(2, 0, nx, ny, nz, arr(g), arr([rU_y, rV_y, rW_y, out[0], out[1], out[2]]), col(6), ny) == 0
    assert L.tlab_avg_gradients_pass(3, 1, nx, ny, nz, arr(g + [u, v, w, p]), arr([out[3], out[4], out[5], fU, fV, fW, rP]), col(44), ny) == 0
    assert np.array_equal(out, whole)
    whole = T.avg_gradients_scal(nx, ny, nz, g[:3], s, u, v, w, fS, fU, fV, fW, rS_y, p, rP, fS_y)
    out = np.zeros((18, ny))
    assert L.tlab_avg_gradients_pass(4, 0, nx, ny, nz, arr(g[:3]), arr([rS_y]), col(0), ny) == 0
    assert L.tlab_avg_gradients_pass(5, 1, nx, ny, nz, arr([g[1], s, u, v, w, p, g[0], g[2]]), arr([out[0], fS, fU, fV, fW, rP, fS_y]), col(11), ny) == 0
    assert np.array_equal(out, whole)
    for bad in (0, 6):
        assert L.tlab_avg_gradients_pass(bad, 0, nx, ny, nz, arr(g), None, col(0), ny) == EINVAL
    assert L.tlab_avg_gradients_pass(2, 0, nx, ny, nz, arr(g), None, col(0), ny) == EINVAL                  # a pass with means, none given
    assert L.tlab_avg_gradients_pass(1, 0, nx, ny, nz, None, None, col(0), ny) == EINVAL
    assert L.tlab_avg_gradients_pass(1, 0, nx, ny, nz, arr(g), None, None, ny) == EINVAL
    assert L.tlab_avg_gradients_pass(1, 0, nx, ny, nz, arr(g), None, col(0), ny - 1) == EINVAL


def test_argument_errors_are_refused():
    import tlab_amd
    L = tlab_amd.load()
    nx, ny, nz = 6, 4, 3
    a = np.ones((nz, ny, nx))
    g = [a] * 9
    prof = np.zeros(ny)
    out = np.zeros((56, ny))
    A_, P_, O_ = vp(a.ctypes.data), vp(prof.ctypes.data), vp(out.ctypes.data)
    for with_p in (False, True):
        assert L.tlab_avg_gradients_flow(nx, ny, nz, *_flow_args(g, A_, P_, O_, with_p), ny) == 0
        assert L.tlab_avg_gradients_scal(nx, ny, nz, *_scal_args(g, A_, P_, O_, with_p), ny) == 0
    assert L.tlab_avg_ugradp(nx, ny, nz, A_, A_, A_, A_, A_, A_, O_) == 0
    for bad in ((0, ny, nz), (nx, 0, nz), (nx, ny, 0), (-1, ny, nz)):
        assert L.tlab_avg_gradients_flow(*bad, *_flow_args(g, A_, P_, O_, False), ny) == EINVAL
        assert L.tlab_avg_gradients_scal(*bad, *_scal_args(g, A_, P_, O_, False), ny) == EINVAL
        assert L.tlab_avg_ugradp(*bad, A_, A_, A_, A_, A_, A_, O_) == EINVAL
    assert L.tlab_avg_gradients_flow(nx, ny, nz, *_flow_args(g, A_, P_, O_, True), ny - 1) == EINVAL      # columns that overlap
    assert L.tlab_avg_gradients_scal(nx, ny, nz, *_scal_args(g, A_, P_, O_, True), ny - 1) == EINVAL
    good = _flow_args(g, A_, P_, O_, False)                              # grad u v w p fU fV fW rP rU_y rV_y rW_y out
    for i in (0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12):
        args = list(good)
        args[i] = None
        assert L.tlab_avg_gradients_flow(nx, ny, nz, *args, ny) == EINVAL, i
    for i in range(9):                                                   # a null pointer inside the list of gradients
        ptrs = (vp * 9)(*[a.ctypes.data] * 9)
        ptrs[i] = None
        assert L.tlab_avg_gradients_flow(nx, ny, nz, ptrs, *good[1:], ny) == EINVAL, i
    args = list(good); args[4] = A_                                      # p without rP     # noqa: E702
    assert L.tlab_avg_gradients_flow(nx, ny, nz, *args, ny) == EINVAL
    args = list(good); args[8] = P_                                      # rP without p     # noqa: E702
    assert L.tlab_avg_gradients_flow(nx, ny, nz, *args, ny) == EINVAL
    assert b"tlab_avg_gradients_flow" in L.tlab_last_error()
    good = [A_] * 6 + [O_]
    for i in range(7):
        args = list(good)
        args[i] = None
        assert L.tlab_avg_ugradp(nx, ny, nz, *args) == EINVAL, i
    good = _scal_args(g, A_, P_, O_, False)                              # grads s u v w p fS fU fV fW rP rS_y fS_y out
    for i in (0, 1, 2, 3, 4, 6, 7, 8, 9, 11, 13):
        args = list(good)
        args[i] = None
        assert L.tlab_avg_gradients_scal(nx, ny, nz, *args, ny) == EINVAL, i
    for i in range(3):
        ptrs = (vp * 3)(*[a.ctypes.data] * 3)
        ptrs[i] = None
        assert L.tlab_avg_gradients_scal(nx, ny, nz, ptrs, *good[1:], ny) == EINVAL, i
    args = list(good); args[5] = A_; args[12] = P_                       # p without rP     # noqa: E702
    assert L.tlab_avg_gradients_scal(nx, ny, nz, *args, ny) == EINVAL
    args = list(good); args[10] = P_                                     # rP without p     # noqa: E702
    assert L.tlab_avg_gradients_scal(nx, ny, nz, *args, ny) == EINVAL
    args = list(good); args[5] = A_; args[10] = P_                       # p without fS_y   # noqa: E702
    assert L.tlab_avg_gradients_scal(nx, ny, nz, *args, ny) == EINVAL
    assert b"tlab_avg_gradients_scal" in L.tlab_last_error()
    # the driver's entry points check their arguments before they touch the handle
    assert L.tlab_dns_avg_gradients_flow(None, None, None, None, P_, P_, P_, None, P_, P_, P_, O_, ny) == EINVAL
    assert L.tlab_dns_avg_gradients_scal(None, A_, None, None, None, P_, P_, P_, P_, None, P_, None, O_, ny) == EINVAL


# ---- the Fortran module ---------------------------------------------------------------------------------------------------------------------
def test_averages_module_and_a_caller_shaped_like_section_3_compile(tmp_path):
    """TLab_AMD_Avg_Gradients_Flow, TLab_AMD_Avg_UGradP and TLab_AMD_Avg_Gradients_Scal take AVG_FLOW_XZ's own arrays (the nine gradient arrays
    of rank 3, the velocity pointers) and its mean2d macros unchanged; the module still depends on TLab_AMD_C alone"""
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    fortran = os.path.join(root, "tlab_amd", "fortran")
    fc = shutil.which("amdflang")
    mod = os.path.join(root, "oracle", "_ref", "mod")
    if fc is None or not os.path.isdir(mod):
        pytest.skip("amdflang or the reference's module files (oracle/_ref/mod) are not here")
    run = lambda *a: subprocess.run([fc, "-cpp", "-O2", "-I", mod, "-module-dir", str(tmp_path), "-c", *a], cwd=tmp_path,      # noqa: E731
                                    capture_output=True, text=True)
    r = run(os.path.join(fortran, "tlab_amd_c.f90"), "-o", str(tmp_path / "c.o"))
    assert r.returncode == 0, r.stderr
    r = run("-I", str(tmp_path), os.path.join(fortran, "tlab_amd_averages.f90"), "-o", str(tmp_path / "a.o"))
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(fortran, "tlab_amd_averages.f90")).read()
    for name in ("TLab_AMD_Avg_Gradients_Flow", "TLab_AMD_Avg_UGradP", "TLab_AMD_Avg_Gradients_Scal"):
        assert re.search(r"subroutine\s+%s\b" % name, src), name
    serial = re.sub(r"^#ifdef USE_MPI\n.*?^#endif\n", "", src, flags=re.M | re.S)
    assert re.findall(r"^\s*use\s+(\w+)", serial, flags=re.M | re.I) == ["TLab_AMD_C"]
    assert "MPI_ALLREDUCE" in src and max(len(l) for l in src.splitlines()) <= 160
    (tmp_path / "caller.f90").write_text(
        "subroutine caller(q, s, dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz, mean2d, wrk1d, imax, jmax, kmax, nv)\n"
        "    use TLab_AMD_C\n"
        "    use TLab_AMD_Averages\n"
        "    integer :: imax, jmax, kmax, nv, ig(16)\n"
        "    real(c_double), target :: q(imax, jmax, kmax, 3), s(imax, jmax, kmax), mean2d(jmax, nv), wrk1d(jmax, 60)\n"
        "    real(c_double), target, dimension(imax, jmax, kmax) :: dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz\n"
        "    real(c_double), pointer :: u(:, :, :), v(:, :, :), w(:, :, :), p_loc(:, :, :)\n"
        "#define rU(j) mean2d(j,ig(1)+1)\n"
        "#define rV(j) mean2d(j,ig(1)+2)\n"
        "#define rW(j) mean2d(j,ig(1)+3)\n"
        "#define rP(j) mean2d(j,ig(1)+4)\n"
        "#define rS(j) mean2d(j,ig(1)+5)\n"
        "#define rU_y(j) mean2d(j,ig(2)+1)\n"
        "#define rV_y(j) mean2d(j,ig(2)+2)\n"
        "#define rW_y(j) mean2d(j,ig(2)+3)\n"
        "#define rS_y(j) mean2d(j,ig(2)+4)\n"
        "#define ugradp(j) mean2d(j,ig(3))\n"
        "    u => q(:, :, :, 1); v => q(:, :, :, 2); w => q(:, :, :, 3); p_loc => dudz\n"
        "    call TLab_AMD_Avg_UGradP(imax, jmax, kmax, u, v, w, dwdx, dwdy, dwdz, ugradp(1), wrk1d)\n"
        "    call TLab_AMD_Avg_Gradients_Flow(imax, jmax, kmax, dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz, u, v, w, &\n"
        "                                     rU(1), rV(1), rW(1), rU_y(1), rV_y(1), rW_y(1), wrk1d, wrk1d(1, 58), p_loc, rP(1))\n"
        "    call TLab_AMD_Avg_Gradients_Flow(imax, jmax, kmax, dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz, u, v, w, &\n"
        "                                     rU(:), rV(:), rW(:), rU_y(:), rV_y(:), rW_y(:), wrk1d, wrk1d(1, 58))\n"
        "    call TLab_AMD_Avg_Gradients_Scal(imax, jmax, kmax, dudx, dudy, dudz, s, u, v, w, rS(1), rU(1), rV(1), rW(1), rS_y(1), &\n"
        "                                     wrk1d, wrk1d(1, 58), p_loc, rP(1), rS_y(1))\n"
        "end subroutine caller\n")
    r = run("-I", str(tmp_path), str(tmp_path / "caller.f90"), "-o", str(tmp_path / "caller.o"))
    assert r.returncode == 0, r.stderr
