"""The head of DNS_STATISTICS_TEMPORAL (FI_PRESSURE_BOUSSINESQ, FI_VORTICITY, INTER_N_XZ) without a GPU: the numpy restatement
(tests/pressure_oracle.py) against what the reference's own compiled routines gave (tests/golden/pressure_ref.npz, recorded by
tests/golden/make_golden_pressure.py), the host branches of the handle-free entry points against the restatement bit for bit (tlab_init is never
called here: every array is host memory), the argument checks, and the Fortran modules against the C interfaces.

Bounds.  Intermittency: np.array_equal (a count is exact).  Vorticity: the record holds the result, not the six derivative arrays, so the
comparison is <= 1e-13 of the maximum.  Pressure: max(1e-12, 2 x the restatement's own one-ulp scatter) relative to max|p| (tests/scatter.py).
The record holds every GOLDEN_STRIDE-th point of a field and its maximum.  Nothing here needs oracle/_ref."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pressure_oracle as P
from scatter import bound, scatter_of

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL = -1
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "pressure_ref.npz"))


@pytest.fixture(scope="module", params=sorted(P.GOLDEN_BOXES))
def restated(request):
    """(box, case, {decomposition: (p, scatter)}) of one golden box: the restatement runs once per decomposition, plus two perturbed runs"""
    box = request.param
    case = P.golden_case(box)
    out = {}
    for name in P.GOLDEN_CASES:
        forces = (P.GOLDEN_COR, P.GOLDEN_BOD) if name == "total" else (None, None)

        def run(u, v, w, s, name=name, forces=forces):
            o = P.golden_oracle(dict(case, q=[u, v, w], s=[s]))
            return (P.fi_pressure_boussinesq(o, name, *forces),)
        (p,), (sc,) = scatter_of(run, case["q"] + case["s"], nsamples=2)
        out[name] = (p, sc)
    return box, case, out


def _err(got, ref_strided, ref_max):
    return float(np.abs(got[::P.GOLDEN_STRIDE] - ref_strided).max() / ref_max)


# ---- the restatement against the reference's compiled routines ------------------------------------------------------------------------------------
def test_pressure_restatement_equals_the_reference(golden, restated):
    box, _, out = restated
    assert int(golden["stride"]) == P.GOLDEN_STRIDE
    for name, (p, sc) in out.items():
        err = _err(p, golden["%s_p_%s" % (box, name)], float(golden["%s_p_%s_max" % (box, name)]))
        print("%s %-10s err %.3e scatter %.3e" % (box, name, err, sc))
        assert err <= bound(sc), (box, name, err, sc)


def test_the_decompositions_differ_and_the_forces_act(restated):
    """the records are four different fields: no case can pass as another"""
    _, case, out = restated
    names = list(out)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert np.abs(out[a][0] - out[b][0]).max() > 1e-3 * np.abs(out[a][0]).max(), (a, b)
    o = P.golden_oracle(case)
    assert np.abs(P.fi_pressure_boussinesq(o, "total") - out["advdiff"][0]).max() <= 1e-13 * np.abs(out["advdiff"][0]).max()      # total without forces


def test_advection_plus_diffusion_is_advdiff(restated):
    box, _, out = restated
    ref = out["advdiff"][0]
    err = float(np.abs(out["advection"][0] + out["diffusion"][0] - ref).max() / np.abs(ref).max())
    sc = max(out[k][1] for k in ("advdiff", "advection", "diffusion"))
    print("%s advection + diffusion - advdiff: %.3e (scatter %.3e)" % (box, err, sc))
    assert err <= bound(sc)


def test_coriolis_and_buoyancy_decompositions_add_up_to_the_sources(restated):
    """total = advdiff + coriolis + buoyancy (the routine is linear in its three sums)"""
    _, case, out = restated
    o = P.golden_oracle(case)
    pc = P.fi_pressure_boussinesq(o, "coriolis", P.GOLDEN_COR, P.GOLDEN_BOD)
    pb = P.fi_pressure_boussinesq(o, "buoyancy", P.GOLDEN_COR, P.GOLDEN_BOD)
    ref = out["total"][0]
    assert np.abs(pc).max() > 1e-3 and np.abs(pb).max() > 1e-3
    err = float(np.abs(out["advdiff"][0] + pc + pb - ref).max() / np.abs(ref).max())
    assert err <= bound(max(out["total"][1], out["advdiff"][1]))


def test_buoyancy_decomposition_subtracts_bbackground_for_y_only():
    """fi_pressure_boussinesq.f90:171-177 against tlab_sources.f90:68: with a horizontal gravity component the x sums of the two differ by
    g_x bbackground(y), which has no x derivative -- the pressures agree to rounding.  (The device refuses that combination instead of deciding
    which rounding to return: tests/test_gpu_pressure.py.)"""
    case = P.golden_case("a")
    o = P.golden_oracle(case)
    bb = 0.3 * np.asarray(case["y"])
    tilted = (6, (0.4, -2.0, 0.0), 1, (1.0, 0.1), 1, bb)
    p_dcmp = P.fi_pressure_boussinesq(o, "buoyancy", None, tilted)
    p_src = P.fi_pressure_boussinesq(o, "total", None, tilted) - P.fi_pressure_boussinesq(o, "advdiff")
    upright = (6, (0.0, -2.0, 0.0), 1, (1.0, 0.1), 1, bb)
    q_dcmp = P.fi_pressure_boussinesq(o, "buoyancy", None, upright)
    q_src = P.fi_pressure_boussinesq(o, "total", None, upright) - P.fi_pressure_boussinesq(o, "advdiff")
    assert np.abs(q_dcmp - q_src).max() <= 1e-9 * np.abs(q_src).max()              # (a difference of two pressures: rounding of the larger ones)
    assert np.abs(p_dcmp - p_src).max() <= 1e-9 * np.abs(p_src).max()
    assert np.abs(p_dcmp - q_dcmp).max() > 1e-3 * np.abs(q_dcmp).max()             # (the horizontal component itself does act)


def test_resolved_is_not_a_case():
    with pytest.raises(ValueError):
        P.fi_pressure_boussinesq(P.golden_oracle(P.golden_case("a")), P.DCMP_RESOLVED)


def test_vorticity_and_intermittency_restatements_equal_the_reference(golden):
    for box in P.GOLDEN_BOXES:
        case = P.golden_case(box)
        vort, six = P.fi_vorticity(P.golden_oracle(case))
        err = _err(vort, golden[box + "_vorticity"], float(golden[box + "_vorticity_max"]))
        print("%s vorticity err %.3e" % (box, err))
        assert err <= 1e-13
        gate = case["gate"]
        ref = golden[box + "_inter"]
        assert ref.shape == (3, gate.shape[1])
        assert np.array_equal(P.inter_n_xz(gate, 3), ref)
        assert not ref[:, 1].any() and (ref[:, 0] > 0).all()                           # the empty plane; levels 1..3 elsewhere
        assert np.all(ref.sum(axis=0) < 1.0)                                           # level 0 is not counted


def test_intermittency_block_uses_the_threshold_of_the_code():
    """dns_statistics.f90:105: (1e-3 * 1e-3) * amax, not the 0.1 % of its comment"""
    nx, ny, nz = 8, 5, 4
    vort = np.full((nz, ny, nx), 1.0)
    vort[:, 0, :] = 0.5e-6            # below 1e-6 of the maximum 1.0
    vort[:, 1, :] = 1.0e-4            # above it, yet below 0.1 %
    out, gate = P.intermittency(vort.ravel(), nx, ny, nz)
    assert np.array_equal(out["Vorticity"], [0.0, 1.0, 1.0, 1.0, 1.0])
    assert gate.dtype == np.int8 and gate.shape == (nz, ny, nx)


# ---- the host branches of the handle-free entry points ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(20, 12, 8), (33, 5, 33), (16, 1, 1), (1, 3, 2)])
@pytest.mark.parametrize("np_", [1, 4])
def test_inter_n_xz_host_branch_equals_the_restatement_bit_for_bit(shape, np_):
    import tlab_amd.operators as T
    nx, ny, nz = shape
    gate = np.random.default_rng(nx + np_).integers(0, 6, (nz, ny, nx)).astype(np.int8)
    gate[:, 0, :] = 0                                                                   # an empty plane
    if ny > 1:
        gate[:, ny - 1, :] = 1                                                          # a full plane
    got = T.inter_n_xz(nx, ny, nz, np_, gate)
    assert got.shape == (np_, ny)
    assert np.array_equal(got, P.inter_n_xz(gate, np_))
    whole = np.frombuffer(bytes(bytearray(1) + bytearray(gate.tobytes())), dtype=np.int8)[1:]      # the same gate one byte off its alignment
    assert np.array_equal(T.inter_n_xz(nx, ny, nz, np_, np.ascontiguousarray(whole)), got)
    gate[gate == 0] = -3                                                                # negative values are not levels either
    assert np.array_equal(T.inter_n_xz(nx, ny, nz, np_, gate), got)


@pytest.mark.parametrize("n", [1, 255, 257])
def test_vorticity_from_gradients_host_branch_is_the_formula(n):
    import tlab_amd.operators as T
    six = [np.random.default_rng(10 * n + i).uniform(-2, 2, n) for i in range(6)]
    got = T.vorticity_from_gradients(*six)
    assert np.array_equal(got, P.vorticity_from_gradients(*six))
    assert np.array_equal(got, ((six[0] - six[1]) ** 2 + (six[2] - six[3]) ** 2) + (six[4] - six[5]) ** 2)


def test_argument_errors_are_refused():
    import tlab_amd
    L = tlab_amd.load()
    nx, ny, nz = 6, 4, 3
    gate = np.ones((nz, ny, nx), dtype=np.int8)
    inter = np.zeros((127, ny))
    G_, I_ = vp(gate.ctypes.data), vp(inter.ctypes.data)
    assert L.tlab_inter_n_xz(nx, ny, nz, 1, G_, I_) == 0
    assert L.tlab_inter_n_xz(nx, ny, nz, 127, G_, I_) == 0                                # the limit itself
    for np_ in (0, -1, 128):
        assert L.tlab_inter_n_xz(nx, ny, nz, np_, G_, I_) == EINVAL
    assert b"127" in L.tlab_last_error()
    for bad in ((0, ny, nz), (nx, 0, nz), (nx, ny, 0), (-1, ny, nz)):
        assert L.tlab_inter_n_xz(*bad, 1, G_, I_) == EINVAL
    assert L.tlab_inter_n_xz(nx, ny, nz, 1, None, I_) == EINVAL
    assert L.tlab_inter_n_xz(nx, ny, nz, 1, G_, None) == EINVAL
    a = np.ones(8)
    A_ = vp(a.ctypes.data)
    out = np.zeros(8)
    O_ = vp(out.ctypes.data)
    assert L.tlab_vorticity_from_gradients(8, A_, A_, A_, A_, A_, A_, O_) == 0
    for n in (0, -5, 2 ** 31):
        assert L.tlab_vorticity_from_gradients(n, A_, A_, A_, A_, A_, A_, O_) == EINVAL
    for k in range(7):
        args = [A_] * 6 + [O_]
        args[k] = None
        assert L.tlab_vorticity_from_gradients(8, *args) == EINVAL, k
    six = (vp * 6)(*[a.ctypes.data] * 6)
    assert L.tlab_fi_vorticity(None, A_, A_, A_, O_, six) == EINVAL                       # no driver
    # tlab_dns_pressure: the arguments are checked before the device is asked for
    three, seven = (vp * 3)(*[a.ctypes.data] * 3), (vp * 7)(*[a.ctypes.data] * 7)
    for dc in (1, -1, 7, 100):                                                            # DCMP_RESOLVED and anything else
        assert L.tlab_dns_pressure(None, dc, three, three, A_, A_, A_, seven, 7) == EINVAL
        assert b"decomposition" in L.tlab_last_error()
    for dc, ntmp in ((0, 2), (3, 0), (5, 2), (6, 2), (2, 6), (4, 3)):                     # three sums; seven for advection and diffusion
        assert L.tlab_dns_pressure(None, dc, three, three, A_, A_, A_, seven, ntmp) == EINVAL
        assert b"work arrays" in L.tlab_last_error(), (dc, ntmp)
    assert L.tlab_dns_pressure(None, 0, three, three, A_, A_, A_, three, 3) == EINVAL     # a null handle
    assert b"null" in L.tlab_last_error()


def test_new_symbols_are_exported_and_bound():
    import tlab_amd
    from tlab_amd import lib as tl
    lib = ctypes.CDLL(tlab_amd.lib_path())
    names = ["tlab_dns_pressure", "tlab_fi_vorticity", "tlab_vorticity_from_gradients", "tlab_inter_n_xz"]
    hdr = open(os.path.join(ROOT, "include", "tlab_amd.h")).read()
    iface = open(os.path.join(ROOT, "tlab_amd", "fortran", "tlab_amd_c.f90")).read()
    for n in names:
        assert hasattr(lib, n) and n in tl.SIGNATURES and re.search(r"\b%s\s*\(" % n, hdr), n
    for n in ("tlab_dns_pressure", "tlab_fi_vorticity", "tlab_inter_n_xz"):
        assert "bind(C, name='%s')" % n in iface, n
    for dc, code in P.DECOMPOSITIONS.items():
        assert re.search(r"#define TLAB_DCMP_%s %d\b" % (dc.upper(), code), hdr), dc
    from tlab_amd.dns import Dns, PRESSURE_DECOMPOSITIONS
    assert PRESSURE_DECOMPOSITIONS == P.DECOMPOSITIONS
    assert callable(Dns.FI_PRESSURE_BOUSSINESQ) and callable(Dns.FI_VORTICITY) and callable(Dns.intermittency)
    assert callable(tlab_amd.fi_vorticity) and callable(tlab_amd.inter_n_xz)


# ---- the Fortran modules ------------------------------------------------------------------------------------------------------------------------
def test_fortran_modules_compile_and_link_against_a_caller(tmp_path):
    """tlab_amd/fortran/tlab_amd_pressure.f90 and the intermittency routines of tlab_amd_averages.f90 depend on TLab_AMD_C alone (outside the
    USE_MPI blocks, which are not compiled here), and a caller shaped like the head of DNS_STATISTICS_TEMPORAL (dns_statistics.f90:93-117) compiles
    against them and links with the library"""
    fortran = os.path.join(ROOT, "tlab_amd", "fortran")
    fc = shutil.which("amdflang")
    mod = os.path.join(ROOT, "oracle", "_ref", "mod")                   # TLab_AMD_Check of tlab_amd_c.f90 writes through the reference's TLab_WorkFlow
    if fc is None or not os.path.isdir(mod):
        pytest.skip("amdflang or the reference's module files (oracle/_ref/mod) are not here")
    run = lambda *a: subprocess.run([fc, "-cpp", "-O2", "-fPIC", "-I", mod, "-module-dir", str(tmp_path), "-c", *a], cwd=tmp_path,      # noqa: E731
                                    capture_output=True, text=True)
    r = run(os.path.join(fortran, "tlab_amd_c.f90"), "-o", str(tmp_path / "c.o"))
    assert r.returncode == 0, r.stderr
    for f, o in (("tlab_amd_pressure.f90", "p.o"), ("tlab_amd_averages.f90", "a.o")):
        r = run("-I", str(tmp_path), os.path.join(fortran, f), "-o", str(tmp_path / o))
        assert r.returncode == 0, r.stderr
        src = open(os.path.join(fortran, f)).read()
        serial = re.sub(r"^#ifdef USE_MPI\n.*?^#e(?:lse|ndif)\n", "", src, flags=re.M | re.S)
        assert re.findall(r"^\s*use\s+(\w+)", serial, flags=re.M | re.I) == ["TLab_AMD_C"]
        assert max(len(l) for l in src.splitlines()) <= 160
    (tmp_path / "caller.f90").write_text(
        "subroutine caller(dns, q, s, txc, mean, imax, jmax, kmax, isize_field, isize_txc_field, inb_txc)\n"
        "    use TLab_AMD_C\n"
        "    use TLab_AMD_Pressure\n"
        "    use TLab_AMD_Averages\n"
        "    type(c_ptr) :: dns, txc6(6)\n"
        "    integer :: imax, jmax, kmax, isize_field, isize_txc_field, inb_txc, i\n"
        "    real(c_double), target :: q(isize_field, 3), s(isize_field, *), txc(isize_txc_field, inb_txc), mean(jmax, 2)\n"
        "    real(c_double) :: amin(1), amax(1)\n"
        "    integer(1), allocatable, target :: gate(:)\n"
        "    call TLab_AMD_FI_Pressure_Boussinesq(dns, q, s, txc(1, 3), txc(1, 1), txc(1, 2), txc(1, 4), 0, isize_txc_field, inb_txc - 3)\n"
        "    allocate (gate(isize_field))\n"
        "    do i = 1, 6\n"
        "        txc6(i) = c_loc(txc(1, 3 + i))\n"
        "    end do\n"
        "    call TLab_AMD_FI_Vorticity(dns, imax, jmax, kmax, q(:, 1), q(:, 2), q(:, 3), txc(:, 1), txc6)\n"
        "    call TLab_AMD_Check(tlab_minmax_any(c_loc(txc(1, 1)), int(isize_field, c_long_long), amin(1), amax(1)), 'MINMAX')\n"
        "    amin(1) = 1.0e-3_c_double*1.0e-3_c_double*amax(1)\n"
        "    call TLab_AMD_Check(tlab_gate_threshold(c_loc(txc(1, 1)), int(isize_field, c_long_long), amin(1), c_loc(gate)), 'gate')\n"
        "    call TLab_AMD_Inter_N_XZ(imax, jmax, kmax, 1, gate, mean(:, 1:1), mean(:, 2:2))\n"
        "end subroutine caller\n")
    r = run("-I", str(tmp_path), str(tmp_path / "caller.f90"), "-o", str(tmp_path / "caller.o"))
    assert r.returncode == 0, r.stderr
    import tlab_amd
    r = subprocess.run([fc, "-shared", "-o", str(tmp_path / "libcaller.so"), str(tmp_path / "caller.o"), str(tmp_path / "p.o"), str(tmp_path / "a.o"),
                        str(tmp_path / "c.o"), "-Wl,--unresolved-symbols=ignore-all", "-L", os.path.dirname(tlab_amd.lib_path()), "-ltlab_amd"],
                       cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nm = subprocess.run(["nm", "-D", "--undefined-only", str(tmp_path / "libcaller.so")], capture_output=True, text=True).stdout
    assert "tlab_dns_pressure" in nm and "tlab_fi_vorticity" in nm and "tlab_inter_n_xz" in nm
