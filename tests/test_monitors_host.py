"""The host side of the device monitors (no GPU): time_courant_device.sed and dns_bounds_control_device.sed turn the array statements of the reference's
TIME_COURANT and DNS_BOUNDS_CONTROL into calls of TLab_AMD_Courant / TLab_AMD_Dilatation (tlab_amd/fortran/tlab_amd_monitors.f90) and change nothing
else; the host branch of the drop-in MINMAX (tlab_minmax_any on host memory) against numpy."""
import ctypes
import difflib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FORTRAN = os.path.join(ROOT, "tlab_amd", "fortran")
REF = os.environ.get("TLAB_REFERENCE", "/root/reference")
TIME = os.path.join(REF, "src", "tools", "dns", "time.f90")
DNS_LOCAL = os.path.join(REF, "src", "tools", "dns", "dns_local.f90")


def _sed(recipe, text):
    return subprocess.run(["sed", "-f", os.path.join(FORTRAN, recipe)], input=text, capture_output=True, text=True, check=True).stdout


def _changes(before, after):
    """the removed and the added lines (stripped)"""
    rem, add = [], []
    for line in difflib.ndiff(before.splitlines(), after.splitlines()):
        if line.startswith("- "):
            rem.append(line[2:].strip())
        elif line.startswith("+ "):
            add.append(line[2:].strip())
    return rem, add


def _routine(text, name):
    m = re.search(r"^\s*subroutine %s\b.*?^\s*end subroutine %s\b" % (name, name), text, flags=re.S | re.M | re.I)
    assert m, name
    return m.group(0)


def test_time_courant_recipe_replaces_only_the_incompressible_maximum():
    if not os.path.isfile(TIME):
        pytest.skip("the reference's time.f90 is not on this machine")
    src = open(TIME).read()
    out = _sed("time_courant_device.sed", src)
    before, after = _routine(src, "TIME_COURANT"), _routine(out, "TIME_COURANT")
    assert out.replace(after, "") == src.replace(before, "")          # nothing outside TIME_COURANT changes
    rem, add = _changes(before, after)
    assert add == ["use TLab_AMD_Monitors, only: TLab_AMD_Courant", "call TLab_AMD_Courant(pmax(1:2))",
                   "if (nse_eqns == DNS_EQNS_INTERNAL .or. nse_eqns == DNS_EQNS_TOTAL) pmax(1) = maxval(p_wrk3d)"]
    # removed: the two incompressible loop nests over u, v, w into p_wrk3d, and the unconditional maxval
    assert rem.count("pmax(1) = maxval(p_wrk3d)") == 1
    body = [r for r in rem if r != "pmax(1) = maxval(p_wrk3d)"]
    assert body[0] == "if (z%size > 1) then" and body[-1] == "end if"
    assert all(not re.search(r"\bp\(|\brho\(|gama0|one_ov_ds2", r) for r in body)      # the compressible branches are untouched
    assert sum("abs(u(i, j, k))*ds(1)%one_ov_ds1(i + idsp)" in r for r in body) == 2
    # what stays the reference's own: the all-reduce, the choice of dtime, the logged Courant numbers, the diffusion maximum
    for keep in ("call MPI_ALLREDUCE(pmax, pmax_aux, ipmax, MPI_REAL8, MPI_MAX, MPI_COMM_WORLD, ims_err)", "logs_data(2) = dtime*pmax(1)",
                 "logs_data(3) = dtime*pmax(2)", "pmax(2) = schmidtfactor*dx2i", "dt_loc = min(dtc, dtd)"):
        assert keep in after


def test_bounds_control_recipe_replaces_only_the_dilatation_statements():
    if not os.path.isfile(DNS_LOCAL):
        pytest.skip("the reference's dns_local.f90 is not on this machine")
    src = _sed("dns_local_device.sed", open(DNS_LOCAL).read())      # the two recipes apply one after the other
    out = _sed("dns_bounds_control_device.sed", src)
    before, after = _routine(src, "DNS_BOUNDS_CONTROL"), _routine(out, "DNS_BOUNDS_CONTROL")
    assert out.replace(after, "") == src.replace(before, "")
    rem, add = _changes(before, after)
    assert add == ["use TLab_AMD_Monitors, only: TLab_AMD_Dilatation", "integer dil_imn(3), dil_imx(3)",
                   "call TLab_AMD_Dilatation(d_min_loc, d_max_loc, dil_imn, dil_imx, imode_ibm)",
                   "dummy = d_max_loc", "idummy = dil_imx", "dummy = d_min_loc", "idummy = dil_imn"]
    allowed = re.compile(r"^(call (FI_INVARIANT_P|FI_INVARIANT_P_STAG|Thermo_Anelastic_WEIGHT_OUTPLACE|IBM_BCS_FIELD|IBM_BCS_FIELD_STAGGER)\(|"
                         r"if \(nse_eqns == DNS_EQNS_ANELASTIC\) then|if \(stagger_on\) then|if \(imode_ibm == 1\) then|else|end if|"
                         r"call MINMAX\(imax, jmax, kmax, txc\(1, 1\), d_max_loc, d_min_loc\)|d_min_loc = -d_min_loc; d_max_loc = -d_max_loc|"
                         r"wrk3d = -txc\(:, 1\)|loc_max\(1:imax, 1:jmax, 1:kmax\) => wrk3d|dummy = (max|min)val\(wrk3d\)|idummy = (max|min)loc\(loc_max\)|"
                         r"idummy\(1\) = idummy\(1\) \+ ims_offset_i|idummy\(3\) = idummy\(3\) \+ ims_offset_k)")
    assert all(allowed.match(r) for r in rem), [r for r in rem if not allowed.match(r)]
    # the bound test as the reference wrote it (abs(d_min_loc) twice) and the log lines stay
    for keep in ("if (max(abs(d_min_loc), abs(d_min_loc)) > bound_d%max) then", "call TLab_Write_ASCII(efile, 'DNS_CONTROL. Dilatation out of bounds.')",
                 "line = 'Maximum dilatation '//trim(adjustl(str))", "line = 'Minimum dilatation '//trim(adjustl(str))",
                 "line = trim(adjustl(line))//' at grid node '//trim(adjustl(str))"):
        assert keep in after
    for stmt in ("minval(wrk3d)", "maxval(wrk3d)", "maxloc(", "minloc(", "call MINMAX(imax, jmax, kmax, txc(1, 1)", "call FI_INVARIANT_P("):
        assert stmt not in after


def test_minmax_host_branch_against_numpy():
    """without tlab_init no array is the library's: tlab_minmax_any (the drop-in MINMAX) takes the host loop"""
    import tlab_amd
    L = tlab_amd.load()
    rng = np.random.default_rng(4)
    for n in (1, 2, 7, 1000):
        a = rng.uniform(-5, 5, n)
        mn, mx = ctypes.c_double(), ctypes.c_double()
        assert L.tlab_minmax_any(a.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(mn), ctypes.byref(mx)) == 0
        assert (mn.value, mx.value) == (a.min(), a.max())
    a = np.ones(3)
    assert L.tlab_minmax_any(a.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(mn), ctypes.byref(mx)) != 0        # empty: refused
