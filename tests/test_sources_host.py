"""The host side of the body forces ([Rotation], [BodyForce]; TLab_Sources_Flow, src/physics/tlab_sources.f90:36-92), no GPU: pins on
tests/sources_oracle.py, the oracle the GPU tests compare against, the refusals that need no device, the sed recipe for an unchanged host, the Fortran
module and the exported symbols."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from cases import grids, init_fields
from tlab_amd import lib as L

DP = ctypes.POINTER(ctypes.c_double)
TLAB_EINVAL, TLAB_EUNSUPPORTED = -1, -2
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KDT, KCO = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0, 1.0]


def _small():
    nx, ny, nz = 16, 20, 8
    x, y, z = grids(nx, ny, nz, True)
    q0, s0 = init_fields(nx, ny, nz, x, y, z, 5)
    return nx, ny, nz, x, y, z, q0, [s0[0], 0.5 * s0[0] + 0.2, 0.25 * s0[0] ** 2 - 0.1]


def _load(o, q0, s0):
    for i in range(3):
        o.q[i] = q0[i].copy()
    for i in range(o.nscal):
        o.s[i] = s0[i].copy()


def test_oracle_without_forces_is_the_buffer_oracle_bit_for_bit():
    from buffer_oracle import BufferOracle
    from sources_oracle import SourcesOracle
    nx, ny, nz, x, y, z, q0, s0 = _small()
    kw = dict(nscal=2, visc=1.0 / 400.0, schmidt=(0.7, 1.0), yuniform=False, hyper_bc1_ext=0.0)
    a, b, c = BufferOracle(x, y, z, **kw), SourcesOracle(x, y, z, **kw), SourcesOracle(x, y, z, **kw)
    c.set_body_forces((0, (1.0, 2.0, 3.0), (0.0, 1.0)), (0, (0.0, -1.0, 0.0), 1, (1.0,), 2, None))      # type none, whatever the vectors hold
    for o in (a, b, c):
        _load(o, q0, s0)
        for k in range(3):
            o.time_substep(2e-3 * KDT[k], KCO[k], k < 2)
    for o in (b, c):
        for name in ("q", "s", "hq", "hs"):
            for u, v in zip(getattr(a, name), getattr(o, name)):
                assert np.array_equal(u, v), name


POINTS = [(3, 7, 2), (0, 0, 0), (15, 19, 7)]      # (i, j, k): an interior point, the first and the last of the box


def test_coriolis_three_points_by_hand():
    from sources_oracle import coriolis
    nx, ny, nz, x, y, z, q0, s0 = _small()
    rng = np.random.default_rng(3)
    h0 = [rng.uniform(-1, 1, nx * ny * nz) for _ in range(3)]
    f1, f2, f3 = 0.7, -1.3, 0.4
    hq = [a.copy() for a in h0]
    coriolis(4, (f1, f2, f3), (0.0, 0.0), q0, hq)                              # EQNS_COR_EXPLICIT
    for i, j, k in POINTS:
        p = i + nx * (j + ny * k)
        u, v, w = (float(a[p]) for a in q0)
        assert hq[0][p] == (h0[0][p] + f3 * v) - f2 * w
        assert hq[1][p] == (h0[1][p] + f1 * w) - f3 * u
        assert hq[2][p] == (h0[2][p] + f2 * u) - f1 * v
    hq = [a.copy() for a in h0]
    p1, p2 = 0.3, 1.1
    coriolis(12, (0.0, f2, 0.0), (p1, p2), q0, hq)                             # EQNS_COR_NORMALIZED
    geo_u, geo_w = math.cos(p1) * p2, -math.sin(p1) * p2
    for i, j, k in POINTS:
        p = i + nx * (j + ny * k)
        u, v, w = (float(a[p]) for a in q0)
        assert hq[0][p] == h0[0][p] + f2 * (geo_w - w)
        assert hq[2][p] == h0[2][p] + f2 * (u - geo_u)
    assert np.array_equal(hq[1], h0[1])


def test_buoyancy_three_points_by_hand():
    from sources_oracle import buoyancy, sources_flow
    nx, ny, nz, x, y, z, q0, s0 = _small()
    ref = 0.2 * y + 0.05
    c = (1.1, -0.4, 0.3, 0.17, 0.9)      # parameters; with inb_scal_array = 3 the independent term of LINEAR is c[3]

    def at(b, i, j, k):
        return float(b[i + nx * (j + ny * k)])
    for i, j, k in POINTS:
        p = i + nx * (j + ny * k)
        s1, s2, s3 = (float(a[p]) for a in s0)
        r = float(ref[j])
        assert at(buoyancy(5, 0, c, 3, s0, ref, nx, ny, nz), i, j, k) == c[0]                                                # HOMOGENEOUS
        assert at(buoyancy(6, 1, c, 3, s0, ref, nx, ny, nz), i, j, k) == c[0] * s1 - (r - c[3])                              # LINEAR
        assert at(buoyancy(6, 2, c, 3, s0, ref, nx, ny, nz), i, j, k) == (c[0] * s1 + c[1] * s2) - (r - c[3])
        assert at(buoyancy(6, 3, c, 3, s0, ref, nx, ny, nz), i, j, k) == ((c[0] * s1 + c[1] * s2) + c[2] * s3) - (r - c[3])
        assert at(buoyancy(6, 0, c, 3, s0, ref, nx, ny, nz), i, j, k) == c[3] - r                                            # general branch, no scalar
        assert at(buoyancy(7, 2, c, 3, s0, ref, nx, ny, nz), i, j, k) == ((c[0] * s1 + c[1] * s2) + (c[2] * s1) * s2) - r    # BILINEAR
        c0 = -c[0] / (c[1] / 2.0) ** 2
        assert at(buoyancy(8, 1, c, 3, s0, ref, nx, ny, nz), i, j, k) == (c0 * s1) * (s1 - c[1]) - r                         # QUADRATIC
    # hq_i = hq_i + g_i b for the g_i that are not zero, the others untouched
    rng = np.random.default_rng(4)
    h0 = [rng.uniform(-1, 1, nx * ny * nz) for _ in range(3)]
    hq = [a.copy() for a in h0]
    g = (0.3, 0.0, -2.0)
    sources_flow(None, (6, g, 2, c, 3, ref), q0, s0, hq, nx, ny, nz)
    b = buoyancy(6, 2, c, 3, s0, ref, nx, ny, nz)
    for i, j, k in POINTS:
        p = i + nx * (j + ny * k)
        assert hq[0][p] == h0[0][p] + g[0] * b[p] and hq[2][p] == h0[2][p] + g[2] * b[p]
    assert np.array_equal(hq[1], h0[1])


@pytest.mark.parametrize("g2", [-2.0, 3.5])
def test_dirichlet_wall_planes_of_hq2_stay_zero(g2):
    """The wall planes of hq2 feed the Neumann data of the Poisson solver and are zeroed by the BCs afterwards: whatever g2 is, v keeps its walls."""
    from sources_oracle import SourcesOracle
    nx, ny, nz, x, y, z, q0, s0 = _small()
    o = SourcesOracle(x, y, z, nscal=2, visc=1.0 / 400.0, schmidt=(0.7, 1.0), yuniform=False, hyper_bc1_ext=0.0)
    _load(o, q0, s0)
    o.set_body_forces(None, (6, (0.0, g2, 0.0), 2, (1.0, -0.4, 0.1), 2, 0.2 * y))
    o.time_substep(1e-3)
    h2 = o.hq[1].reshape(nz, ny, nx)
    assert not h2[:, 0, :].any() and not h2[:, ny - 1, :].any()
    assert np.abs(h2).max() > 0.0


def test_refusals_without_a_device():
    lib = L.load()
    v = (ctypes.c_double * 3)(0.0, 1.5, 0.0)
    p2 = (ctypes.c_double * 2)(0.3, 1.0)
    par = (ctypes.c_double * 3)(1.0, -0.4, 0.1)
    nan3 = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    inf3 = (ctypes.c_double * 3)(float("inf"), 0.0, 0.0)
    bb = (ctypes.c_double * 8)(*([0.1] * 8))
    # null handle, with arguments that are valid otherwise
    assert lib.tlab_dns_set_coriolis(None, 4, v, p2) == TLAB_EINVAL
    assert b"null handle" in lib.tlab_last_error()
    assert lib.tlab_dns_set_coriolis(None, 0, None, None) == TLAB_EINVAL
    assert lib.tlab_dns_set_buoyancy(None, 6, v, 1, par, 3, 1, None) == TLAB_EINVAL
    assert lib.tlab_dns_set_buoyancy(None, 6, v, 1, par, 3, 1, bb) == TLAB_EINVAL          # a profile and no driver
    assert lib.tlab_dns_set_buoyancy(None, 0, None, 0, None, 0, 0, None) == TLAB_EINVAL
    assert lib.tlab_slab_dns_set_coriolis(None, 4, v, p2) == TLAB_EINVAL
    assert lib.tlab_slab_dns_set_buoyancy(None, 6, v, 1, par, 3, 1, None) == TLAB_EINVAL
    assert lib.tlab_pencil_dns_set_coriolis(None, 4, v, p2) == TLAB_EINVAL
    assert lib.tlab_pencil_dns_set_buoyancy(None, 6, v, 1, par, 3, 1, None) == TLAB_EINVAL
    assert lib.tlab_dns_sources_flow(None, None, None, None) != 0
    assert lib.tlab_deferred_sources_flow(None, None, None, None) != 0
    assert lib.tlab_deferred_sources_stats(None) == TLAB_EINVAL
    assert lib.tlab_dns_info(None, 4) == -1
    # unknown types
    for t in (1, 3, 5, 11, 13, -1):
        assert lib.tlab_dns_set_coriolis(None, t, v, p2) == TLAB_EINVAL, t
    assert b"unknown type" in lib.tlab_last_error()
    for t in (1, 2, 3, 11, -4):
        assert lib.tlab_dns_set_buoyancy(None, t, v, 1, par, 3, 1, None) == TLAB_EINVAL, t
    assert b"unknown type" in lib.tlab_last_error()
    # the three buoyancy types that are not built
    for t, word in ((4, b"Thermo_Anelastic_BUOYANCY"), (9, b"plane means"), (10, b"plane means")):
        for setter in (lib.tlab_dns_set_buoyancy, lib.tlab_slab_dns_set_buoyancy, lib.tlab_pencil_dns_set_buoyancy):
            assert setter(None, t, v, 1, par, 3, 1, None) == TLAB_EUNSUPPORTED, t
            assert word in lib.tlab_last_error()
    # normalized Coriolis with an active y equation (f1 or f3), as the reference stops
    for vec in ((0.5, 1.5, 0.0), (0.0, 1.5, -0.1)):
        assert lib.tlab_dns_set_coriolis(None, 12, (ctypes.c_double * 3)(*vec), p2) == TLAB_EINVAL
        assert b"normalized" in lib.tlab_last_error()
    # NaN and infinite values
    assert lib.tlab_dns_set_coriolis(None, 4, nan3, p2) == TLAB_EINVAL and b"NaN" in lib.tlab_last_error()
    assert lib.tlab_dns_set_coriolis(None, 4, inf3, p2) == TLAB_EINVAL
    assert lib.tlab_dns_set_coriolis(None, 12, v, (ctypes.c_double * 2)(float("nan"), 1.0)) == TLAB_EINVAL and b"NaN" in lib.tlab_last_error()
    assert lib.tlab_dns_set_buoyancy(None, 6, nan3, 1, par, 3, 1, None) == TLAB_EINVAL and b"NaN" in lib.tlab_last_error()
    assert lib.tlab_dns_set_buoyancy(None, 6, v, 1, (ctypes.c_double * 3)(1.0, float("nan"), 0.0), 3, 1, None) == TLAB_EINVAL and b"NaN" in lib.tlab_last_error()
    assert lib.tlab_dns_set_buoyancy(None, 6, v, -1, par, 3, 1, None) == TLAB_EINVAL


def _routine(t, name):
    m = re.search(r"^ *subroutine %s\b.*?^ *end subroutine %s\b" % (name, name), t, flags=re.S | re.M)
    assert m, name
    return m.group(0)


def test_sed_recipe_moves_the_sources_to_the_device():
    import subprocess
    src = os.path.join(os.environ.get("TLAB_REFERENCE", "/root/reference"), "src", "physics", "tlab_sources.f90")
    if not os.path.isfile(src):
        pytest.skip("the reference's tlab_sources.f90 is not on this machine")
    out = subprocess.run(["sed", "-f", os.path.join(ROOT, "tlab_amd", "fortran", "tlab_sources_device.sed"), src], capture_output=True, text=True,
                         check=True).stdout
    text = open(src).read()
    f0, f1 = _routine(text, "TLab_Sources_Flow"), _routine(out, "TLab_Sources_Flow")
    assert f0 != f1
    assert out.replace(f1, "") == text.replace(f0, "")                          # nothing outside TLab_Sources_Flow changes
    assert _routine(out, "TLab_Sources_Scal") == _routine(text, "TLab_Sources_Scal")
    call = ("call TLab_AMD_Sources_Flow(TLab_AMD_DNS_Handle(), coriolis%type, coriolis%vector, coriolis%parameters, &\n"
            "                                   buoyancy%type, buoyancy%vector, buoyancy%scalar(1), buoyancy%parameters, &\n"
            "                                   inb_scal_array, bbackground, q, s, hq)")
    assert f1.count("call TLab_AMD_Sources_Flow(") == 1 and f1.count(call) == 1
    assert out.count("TLab_AMD_Sources_Flow(") == 1
    assert "Rotation_Coriolis(" not in f1 and "Gravity_Buoyancy(" not in f1 and "Thermo_Anelastic_BUOYANCY(" not in f1
    assert "buoyancy%active" not in f1 and "buoyancy%vector(iq)" not in f1
    # the guard stands before the call: subsidence and the special forcing are host loops over device memory
    guard = "if (any(subsidenceProps%active) .or. any(forcingProps%active)) &\n            call TLab_AMD_Check("
    assert f1.count(guard) == 1 and f1.index(guard) < f1.index(call)
    for use in ("use TLab_AMD_C, only: TLab_AMD_Check", "use TLab_AMD_Sources, only: TLab_AMD_Sources_Flow", "use TLab_AMD_DNS, only: TLab_AMD_DNS_Handle"):
        assert f1.count(use) == 1
    # the blocks that stay are untouched, and if / end if still pair up
    for keep in ("LargeScaleForcing_Subsidence(", "SpecialForcing_Source("):
        assert f1.count(keep) == f0.count(keep) == 1
    assert max(len(l) for l in f1.splitlines()) <= 132                          # (the free-form line limit of strict compilers)
    opens = len(re.findall(r"^ *if \(.*\) then *$", f1, flags=re.M))
    assert opens == len(re.findall(r"^ *end if *$", f1, flags=re.M)) == 2
    assert len(re.findall(r"^ *do iq = 1, 3", f1, flags=re.M)) == 1 and len(re.findall(r"^ *end do *$", f1, flags=re.M)) == f0.count("end do") - 1


def test_sources_module_compiles_against_the_c_interfaces(tmp_path):
    import shutil
    import subprocess
    fortran = os.path.join(ROOT, "tlab_amd", "fortran")
    fc = shutil.which("amdflang")
    mod = os.path.join(ROOT, "oracle", "_ref", "mod")
    if fc is None or not os.path.isdir(mod):
        pytest.skip("amdflang or the reference's module files (oracle/_ref/mod) are not here")
    run = lambda *a: subprocess.run([fc, "-cpp", "-O2", "-I", mod, "-module-dir", str(tmp_path), "-c", *a], cwd=tmp_path,      # noqa: E731
                                    capture_output=True, text=True)
    r = run(os.path.join(fortran, "tlab_amd_c.f90"), "-o", str(tmp_path / "c.o"))
    assert r.returncode == 0, r.stderr
    r = run("-I", str(tmp_path), os.path.join(fortran, "tlab_amd_sources.f90"), "-o", str(tmp_path / "s.o"))
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(fortran, "tlab_amd_sources.f90")).read()
    assert re.findall(r"^\s*use\s+(\w+)", src, flags=re.M | re.I) == ["TLab_AMD_C"]          # depends on the C interfaces alone
    # a caller shaped like the patched TLab_Sources_Flow (an allocatable profile, assumed-size fields) compiles against the module
    (tmp_path / "caller.f90").write_text(
        "subroutine caller(dns, q, s, hq, n)\n"
        "    use TLab_AMD_C\n"
        "    use TLab_AMD_Sources, only: TLab_AMD_Sources_Flow\n"
        "    type(c_ptr) :: dns\n"
        "    integer :: n, scal(10), itype\n"
        "    real(c_double) :: q(n, *), s(n, *), hq(n, *), vector(3), parameters(10)\n"
        "    real(c_double), allocatable :: bbackground(:)\n"
        "    call TLab_AMD_Sources_Flow(dns, itype, vector, parameters, itype, vector, scal(1), parameters, n, bbackground, q, s, hq)\n"
        "end subroutine caller\n")
    r = run("-I", str(tmp_path), str(tmp_path / "caller.f90"), "-o", str(tmp_path / "caller.o"))
    assert r.returncode == 0, r.stderr


def test_new_symbols_are_exported_and_bound():
    import tlab_amd
    lib = ctypes.CDLL(tlab_amd.lib_path())
    names = ["tlab_dns_set_coriolis", "tlab_dns_set_buoyancy", "tlab_dns_sources_flow", "tlab_dns_info", "tlab_deferred_sources_flow",
             "tlab_deferred_sources_stats", "tlab_slab_dns_set_coriolis", "tlab_slab_dns_set_buoyancy", "tlab_pencil_dns_set_coriolis",
             "tlab_pencil_dns_set_buoyancy"]
    for n in names:
        assert hasattr(lib, n), n
        assert n in L.SIGNATURES, n
    hdr = open(os.path.join(ROOT, "include", "tlab_amd.h")).read()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    iface = open(os.path.join(ROOT, "tlab_amd", "fortran", "tlab_amd_c.f90")).read()
    for n in names[:6]:
        assert "bind(C, name='%s')" % n in iface, n
    from tlab_amd.dns import Dns
    from tlab_amd.pencil import NativePencilDns
    from tlab_amd.slab import NativeSlabDns
    for cls in (Dns, NativeSlabDns, NativePencilDns):
        assert callable(getattr(cls, "set_body_forces"))
    assert callable(Dns.sources_flow)
