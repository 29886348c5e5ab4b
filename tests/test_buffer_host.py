"""The host side of the relaxation buffer zones ([BufferZone] Type = relaxation, tools/dns/boundary_buffer.f90), no GPU: tlab_buffer_tau against
INI_BLOCK's formula, the refusals that need no device, and pins on tests/buffer_oracle.py, the oracle the GPU tests compare against."""
import ctypes

import numpy as np
import pytest

from cases import grids, init_fields
from tlab_amd import lib as L

DP = ctypes.POINTER(ctypes.c_double)
TLAB_EINVAL, TLAB_EUNSUPPORTED = -1, -2


def _tau(y, offset, size, strength, sigma, form):
    y = np.ascontiguousarray(y, dtype=np.float64)
    out = np.full(max(size, 1), np.nan)
    rc = L.load().tlab_buffer_tau(len(y), y.ctypes.data_as(DP), offset, size, strength, sigma, form, out.ctypes.data_as(DP))
    return rc, out


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("sigma", [2.0, 1.5])
@pytest.mark.parametrize("size", [2, 8])
def test_buffer_tau_is_ini_blocks_formula(form, sigma, size):
    ny = 40
    y = grids(16, ny, 8, True)[1]
    offset = 0 if form == 1 else ny - size
    rc, tau = _tau(y, offset, size, 1.57, sigma, form)
    assert rc == 0
    inv = 1.0 / (y[offset + size - 1] - y[offset])                      # "dummy", boundary_buffer.f90:362
    j = offset + np.arange(size)
    d = (y[j] - y[offset]) if form == 2 else (y[offset + size - 1] - y[j])
    want = 1.57 * np.array([float(v) ** sigma for v in d * inv])
    assert (_ulps(tau, want) <= 2.0).all(), (tau, want)
    far, near = (0, -1) if form == 1 else (-1, 0)                       # the strength itself on the wall plane, zero at the inner edge
    assert tau[far] == 1.57 and tau[near] == 0.0
    from buffer_oracle import buffer_tau
    assert (_ulps(tau, buffer_tau(y, offset, size, [1.57], [sigma], form)[:, 0]) <= 2.0).all()


def test_refusals_without_a_device():
    y = grids(16, 24, 8, True)[1]
    lib = L.load()
    assert _tau(y, 0, 1, 1.0, 2.0, 1)[0] == TLAB_EINVAL                 # one plane: no length (the reference never sets tau there)
    assert b"one plane" in lib.tlab_last_error()
    assert _tau(y, 0, 4, 1.0, 2.0, 0)[0] == TLAB_EINVAL                 # form
    assert _tau(y, 21, 4, 1.0, 2.0, 2)[0] == TLAB_EINVAL                # beyond the grid
    assert _tau(y, -1, 4, 1.0, 2.0, 2)[0] == TLAB_EINVAL
    assert lib.tlab_buffer_tau(24, None, 0, 4, 1.0, 2.0, 1, None) == TLAB_EINVAL
    t = np.ones(4)
    assert lib.tlab_dns_set_buffer_zone(None, 3, 0, 4, 3, t.ctypes.data_as(DP), t.ctypes.data_as(DP)) == TLAB_EINVAL      # no driver
    assert lib.tlab_dns_set_buffer_type(None, 1) == TLAB_EINVAL
    assert lib.tlab_dns_buffer_relax_flow(None, None, None) != 0
    assert lib.tlab_dns_buffer_relax_scal(None, None, None) != 0


def _small():
    nx, ny, nz = 16, 20, 8
    x, y, z = grids(nx, ny, nz, True)
    q0, s0 = init_fields(nx, ny, nz, x, y, z, 5)
    return nx, ny, nz, x, y, z, q0, [s0[0], 0.5 * s0[0] + 0.2]


def _load(o, q0, s0):
    for i in range(3):
        o.q[i] = q0[i].copy()
    for i in range(len(s0)):
        o.s[i] = s0[i].copy()


def test_oracle_without_zones_is_the_plain_oracle_bit_for_bit():
    from oracle.tlab_oracle_rhs import DnsOracle
    from buffer_oracle import BufferOracle
    nx, ny, nz, x, y, z, q0, s0 = _small()
    kw = dict(nscal=2, visc=1.0 / 400.0, schmidt=(0.7, 1.0), yuniform=False, hyper_bc1_ext=0.0)
    a, b = DnsOracle(x, y, z, **kw), BufferOracle(x, y, z, **kw)
    b.set_buffer_zones(0, 0)
    kdt, kco = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0, 1.0]
    for o in (a, b):
        _load(o, q0, s0)
        for k in range(3):
            o.time_substep(2e-3 * kdt[k], kco[k], k < 2)
    for name in ("q", "s", "hq", "hs"):
        for u, v in zip(getattr(a, name), getattr(b, name)):
            assert np.array_equal(u, v), name


def test_oracle_with_zones_on_three_planes_by_hand():
    """One substep from zero tendencies.  The scalars feel neither the pressure nor the flow relaxation within a substep, so hs of the zoned oracle is
    the plain oracle's hs, BCs included, minus tau (s - ref) on the zone's planes, with s the field BEFORE the update."""
    from oracle.tlab_oracle_rhs import DnsOracle
    from buffer_oracle import BufferOracle, plane_mean
    nx, ny, nz, x, y, z, q0, s0 = _small()
    kw = dict(nscal=2, visc=1.0 / 400.0, schmidt=(0.7, 1.0), yuniform=False, hyper_bc1_ext=0.0)
    a, b = DnsOracle(x, y, z, **kw), BufferOracle(x, y, z, **kw)
    _load(a, q0, s0); _load(b, q0, s0)
    size, strength, sigma = 5, 40.0, 2.0
    b.set_buffer_zones(0, size, params_u=(strength, sigma), params_s=(strength, sigma))
    assert b.buff_flow[0] is None and b.buff_scal[0] is None and b.buff_scal[1].offset == ny - size
    a.time_substep(1e-3)
    b.time_substep(1e-3)
    blk = b.buff_scal[1]
    assert blk.tau[-1, 0] == strength and blk.tau[0, 0] == 0.0
    for i in range(2):
        s3 = s0[i].reshape(nz, ny, nx)
        ha, hb = a.hs[i].reshape(nz, ny, nx), b.hs[i].reshape(nz, ny, nx)
        jloc = 2
        j = ny - size + jloc                                                     # an interior plane of the zone
        ref = plane_mean(s3, j)
        assert np.array_equal(blk.ref[i, :, jloc, :], np.full((nz, nx), ref))
        assert np.array_equal(hb[:, j, :], ha[:, j, :] - blk.tau[jloc, i] * (s3[:, j, :] - ref))
        assert np.abs(hb[:, j, :] - ha[:, j, :]).max() > 0.0
        ref = plane_mean(s3, ny - 1)                                             # the Dirichlet wall plane: BC value 0, then the zone term at its maximum
        assert np.array_equal(hb[:, ny - 1, :], -strength * (s3[:, ny - 1, :] - ref))
        assert np.abs(hb[:, ny - 1, :]).max() > 0.0 and not ha[:, ny - 1, :].any()
        assert np.array_equal(hb[:, ny - size - 1, :], ha[:, ny - size - 1, :])  # just outside the zone
        assert np.array_equal(b.s[i], s0[i] + 1e-3 * b.hs[i])
    # the flow part is inside the projection: hq differs beyond the zone too, v keeps its Dirichlet wall planes
    assert np.abs(b.hq[0] - a.hq[0]).max() > 0.0
    assert not b.hq[1].reshape(nz, ny, nx)[:, ny - 1, :].any()


def test_sed_recipe_moves_the_zones_to_the_device():
    import os
    import re
    import subprocess
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    src = os.path.join(os.environ.get("TLAB_REFERENCE", "/root/reference"), "src", "tools", "dns", "boundary_buffer.f90")
    if not os.path.isfile(src):
        pytest.skip("the reference's boundary_buffer.f90 is not on this machine")
    out = subprocess.run(["sed", "-f", os.path.join(root, "tlab_amd", "fortran", "boundary_buffer_device.sed"), src], capture_output=True, text=True,
                         check=True).stdout
    text = open(src).read()

    def routine(t, name):
        m = re.search(r"^ *subroutine %s\b.*?^ *end subroutine %s\b" % (name, name), t, flags=re.S | re.M)
        assert m, name
        return m.group(0)
    ini0, ini1 = routine(text, "BOUNDARY_BUFFER_INITIALIZE"), routine(out, "BOUNDARY_BUFFER_INITIALIZE")
    rs0, rs1 = routine(text, "BOUNDARY_BUFFER_RELAX_SCAL"), routine(out, "BOUNDARY_BUFFER_RELAX_SCAL")
    # nothing outside the two routines changes
    assert out.replace(ini1, "").replace(rs1, "") == text.replace(ini0, "").replace(rs0, "")
    # the four J blocks are pushed at the end of the initialisation, after every INI_BLOCK
    for blk, end, group in (("BuffFlowJmin", 3, 0), ("BuffFlowJmax", 4, 0), ("BuffScalJmin", 3, 1), ("BuffScalJmax", 4, 1)):
        call = "call TLab_AMD_Buffer_Push(TLab_AMD_DNS_Handle(), %d, %d, %s%%size, %s%%nfields, %s%%tau, %s%%ref)" % (end, group, blk, blk, blk, blk)
        assert ini1.count(call) == 1 and ini1.index(call) > ini1.rindex("call INI_BLOCK("), blk
    assert "use TLab_AMD_Buffer, only: TLab_AMD_Buffer_Push" in ini1
    kept = [l for l in ini0.splitlines()]
    assert [l for l in ini1.splitlines() if "TLab_AMD" not in l] == kept          # only lines were added
    # the host statement over hs is gone from the DEFAULT branch; the compressible branch stays
    default = rs1[rs1.index("case DEFAULT"):]
    assert "RELAX_BLOCK(" not in default and default.count("call TLab_AMD_Buffer_Relax_Scal(TLab_AMD_DNS_Handle())") == 1
    assert rs1.count("RELAX_BLOCK_RHO(") == rs0.count("RELAX_BLOCK_RHO(") == 4
    assert routine(out, "RELAX_BLOCK") == routine(text, "RELAX_BLOCK")


def test_buffer_module_compiles_against_the_c_interfaces(tmp_path):
    import os
    import re
    import shutil
    import subprocess
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
    r = run("-I", str(tmp_path), os.path.join(fortran, "tlab_amd_buffer.f90"), "-o", str(tmp_path / "b.o"))
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(fortran, "tlab_amd_buffer.f90")).read()
    assert re.findall(r"^\s*use\s+(\w+)", src, flags=re.M | re.I) == ["TLab_AMD_C"]          # depends on the C interfaces alone
