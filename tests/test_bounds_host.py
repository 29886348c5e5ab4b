"""The host side of scalar bounds limiting (no GPU): dns_local_device.sed turns the scalar loop of the reference's DNS_BOUNDS_LIMIT into one call of
TLab_AMD_Bounds_Limit (tlab_amd/fortran/tlab_amd_bounds.f90), and that module compiles against the interfaces of tlab_amd_c.f90."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FORTRAN = os.path.join(ROOT, "tlab_amd", "fortran")
REF = os.environ.get("TLAB_REFERENCE", "/root/reference")
DNS_LOCAL = os.path.join(REF, "src", "tools", "dns", "dns_local.f90")


def _routine(text, name):
    m = re.search(r"^\s*subroutine %s\b.*?^\s*end subroutine %s\b" % (name, name), text, flags=re.S | re.M | re.I)
    assert m, name
    return m.group(0)


def test_sed_recipe_moves_the_scalar_loop_to_the_device():
    if not os.path.isfile(DNS_LOCAL):
        pytest.skip("the reference's dns_local.f90 is not on this machine")
    out = subprocess.run(["sed", "-f", os.path.join(FORTRAN, "dns_local_device.sed"), DNS_LOCAL], capture_output=True, text=True, check=True).stdout
    before, after = _routine(open(DNS_LOCAL).read(), "DNS_BOUNDS_LIMIT"), _routine(out, "DNS_BOUNDS_LIMIT")
    assert "s(:, is) = min(max(s(:, is)" in before
    assert "s(:, is)" not in after and not re.search(r"do\s+is\s*=", after, flags=re.I)          # the host loop over device memory is gone
    assert re.search(r"call TLab_AMD_Bounds_Limit\(s, size\(s, 1\), inb_scal, bound_s\(1:inb_scal\)%active", after)
    assert "use TLab_AMD_Bounds, only: TLab_AMD_Bounds_Limit" in after
    for line in before.splitlines():                      # bound_r / bound_p (compressible) untouched
        if "bound_r" in line or "bound_p" in line:
            assert line in after.splitlines()
    # nothing outside the routine changes
    assert out.replace(after, "") == open(DNS_LOCAL).read().replace(before, "")


def test_bounds_module_compiles_against_the_c_interfaces(tmp_path):
    fc = shutil.which("amdflang")
    mod = os.path.join(ROOT, "oracle", "_ref", "mod")
    if fc is None or not os.path.isdir(mod):
        pytest.skip("amdflang or the reference's module files (oracle/_ref/mod) are not here")
    run = lambda *a: subprocess.run([fc, "-cpp", "-O2", "-I", mod, "-module-dir", str(tmp_path), "-c", *a], cwd=tmp_path,      # noqa: E731
                                    capture_output=True, text=True)
    r = run(os.path.join(FORTRAN, "tlab_amd_c.f90"), "-o", str(tmp_path / "c.o"))
    assert r.returncode == 0, r.stderr
    r = run("-I", str(tmp_path), os.path.join(FORTRAN, "tlab_amd_bounds.f90"), "-o", str(tmp_path / "b.o"))
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(FORTRAN, "tlab_amd_bounds.f90")).read()
    assert re.findall(r"^\s*use\s+(\w+)", src, flags=re.M | re.I) == ["TLab_AMD_C"]          # depends on the C interfaces alone
