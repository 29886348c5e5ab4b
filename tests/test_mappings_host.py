"""The field mappings without a GPU: the numpy restatement (tests/mappings_oracle.py) on the stand-in operators against what the reference's own
compiled routines gave on the same stand-ins (tests/golden/mappings_ref.npz, recorded by tests/golden/make_golden_mappings.py), the host branch of
tlab_gradient_maps against the restatement (tlab_init is never called here: every array is host memory), its refusals, and the Fortran wrappers
against the C interfaces.

Every comparison is np.array_equal on the whole output: the records hold the reference's compiled pointwise arithmetic and call order, the
restatement rounds where they round, and the host loop keeps every operation as written.  The refusal of a mix of host and device arrays needs
a device array: it is in tests/test_gpu_mappings.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mappings_oracle as M
import tlab_amd as T
from tlab_amd import lib as tl

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL = -1
vp = ctypes.c_void_p
BOXES = ("a", "b")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "mappings_ref.npz"))


def _fields(g, box):
    return {k: np.ascontiguousarray(g["in_%s_%s" % (box, k)]).reshape(-1) for k in "uvwps"}


def _gradients(g, box):
    """the stand-in gradients of the fixture's fields: du9, ds3"""
    nx, ny, nz = (int(v) for v in g["box_%s" % box])
    p1, _ = M.standin_operators(nx, ny, nz)
    F = _fields(g, box)
    return [p1(d, F[c]) for c in "uvw" for d in (1, 2, 3)], [p1(d, F["s"]) for d in (1, 2, 3)]


# ---- the restatement against the reference's compiled routines ----------------------------------------------------------------------------------
@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("name", M.MAPS)
def test_restated_maps_equal_the_reference_bit_for_bit(golden, box, name):
    nx, ny, nz = (int(v) for v in golden["box_%s" % box])
    p1, _ = M.standin_operators(nx, ny, nz)
    F = _fields(golden, box)
    got = M.fi_map(name, p1, F["u"], F["v"], F["w"], F["s"])
    ref = golden["out_%s_%s" % (box, name)]
    assert len(got) == ref.shape[0] == M.NOUT[name]
    for k, a in enumerate(got):
        assert np.array_equal(a, ref[k]), (name, k)


@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("kind", sorted(M.FI_DIFFUSION))
def test_restated_diffusion_and_pressure_terms_equal_the_reference_bit_for_bit(golden, box, kind):
    nx, ny, nz = (int(v) for v in golden["box_%s" % box])
    p1, p2 = M.standin_operators(nx, ny, nz)
    F = _fields(golden, box)
    f = F["p"] if kind == "STRAIN_PRESSURE" else F["s"]
    got = M.FI_DIFFUSION[kind](p1, p2, (F["u"], F["v"], F["w"]), f)
    assert np.array_equal(got, golden["out_%s_%s" % (box, kind)][0])


def test_the_fixture_takes_both_branches_of_strain_a(golden):
    for box in BOXES:
        gg = golden["out_%s_STRAIN_A" % box][2]
        assert (gg == 0.0).any() and (gg > 0.0).any()


def test_the_restatement_from_gradients_is_the_restatement_on_operators(golden):
    """from_gradients() hands the routines the derivatives the operators would give: nothing else differs"""
    du9, ds3 = _gradients(golden, "b")
    nx, ny, nz = (int(v) for v in golden["box_b"])
    p1, _ = M.standin_operators(nx, ny, nz)
    F = _fields(golden, "b")
    want = {m: M.fi_map(m, p1, F["u"], F["v"], F["w"], F["s"]) for m in M.MAPS}
    got = M.gradient_maps(du9, ds3, M.MAPS)
    for m in M.MAPS:
        for a, b in zip(got[m], want[m]):
            assert np.array_equal(a, b), m


# ---- the host branch of tlab_gradient_maps ------------------------------------------------------------------------------------------------------
def _as_tuple(x):
    return x if isinstance(x, tuple) else (x,)


@pytest.mark.parametrize("box", BOXES)
def test_host_branch_equals_the_records_for_every_map_alone_and_all_together(golden, box):
    du9, ds3 = _gradients(golden, box)
    alone = {m: T.gradient_maps(du9, ds3 if m in M.SCALAR_MAPS else None, m)[m] for m in M.MAPS}
    together = T.gradient_maps(du9, ds3, list(M.MAPS))
    for m in M.MAPS:
        ref = golden["out_%s_%s" % (box, m)]
        for got in (alone[m], together[m]):
            got = _as_tuple(got)
            assert len(got) == ref.shape[0]
            for k, a in enumerate(got):
                assert np.array_equal(a, ref[k]), (m, k)


def test_host_branch_reads_no_gradient_a_map_does_not_need(golden):
    """P reads the diagonal, VORTICITY and CURL the six off-diagonal gradients: the others may be missing"""
    du9, ds3 = _gradients(golden, "b")
    diag = [a if i in (0, 4, 8) else None for i, a in enumerate(du9)]
    off = [None if i in (0, 4, 8) else a for i, a in enumerate(du9)]
    assert np.array_equal(T.gradient_maps(diag, None, "P")["P"], golden["out_b_P"][0])
    got = T.gradient_maps(off, None, ["CURL", "VORTICITY"])
    assert np.array_equal(got["VORTICITY"], golden["out_b_VORTICITY"][0])
    assert np.array_equal(np.stack(got["CURL"]), golden["out_b_CURL"])
    assert np.array_equal(T.gradient_maps([None] * 9, ds3, "GRADIENT")["GRADIENT"], golden["out_b_GRADIENT"][0])
    with pytest.raises(T.TlabError):
        T.gradient_maps(diag, None, "Q")


def test_map_tables_agree():
    assert tuple(T.MAPS) == M.MAPS
    assert {m: v[1] for m, v in T.MAPS.items()} == M.NOUT
    assert tuple(m for m, v in T.MAPS.items() if v[2]) == M.SCALAR_MAPS
    hdr = open(os.path.join(ROOT, "tlab_amd", "csrc", "tlab_amd_mappings.h")).read()
    for m, (code, _, _) in T.MAPS.items():
        assert re.search(r"#define TLAB_MAP_%s %d\b" % (m, code), hdr), m
    for k, code in T.FI_DIFFUSION_KINDS.items():
        assert re.search(r"#define TLAB_FI_%s %d\b" % (k, code), hdr), k


def test_refusals():
    L = tl.load()
    n = 16
    a = [np.linspace(0.0, 1.0, n) + i for i in range(12)]
    o = [np.zeros(n) for _ in range(22)]
    P = lambda arrs: (vp * len(arrs))(*[x.ctypes.data if x is not None else None for x in arrs])      # noqa: E731
    codes = lambda *c: (ctypes.c_int * len(c))(*c)      # noqa: E731
    du, ds = P(a[:9]), P(a[9:])
    call = lambda n_, du_, ds_, c, out: L.tlab_gradient_maps(n_, du_, ds_, c, len(c), out)      # noqa: E731
    assert call(n, du, ds, codes(*range(12)), P(o)) == 0
    assert call(n, du, None, codes(0, 1, 2), P(o[:3])) == 0
    for bad_n in (0, -1, 2 ** 31):
        assert call(bad_n, du, ds, codes(0), P(o[:1])) == EINVAL, bad_n
    assert L.tlab_gradient_maps(n, du, ds, codes(0), 0, P(o[:1])) == EINVAL                       # no map
    assert call(n, du, ds, codes(12), P(o[:1])) == EINVAL                                        # not a code
    assert call(n, du, ds, codes(0, 0), P(o[:2])) == EINVAL                                      # named twice
    for m in (9, 10, 11):
        assert call(n, du, None, codes(m), P(o[:3])) == EINVAL, m                                # a missing ds3
    assert call(n, du, P([a[9], None, a[11]]), codes(9), P(o[:1])) == EINVAL                     # a needed gradient is null
    assert call(n, du, ds, codes(0), P([None])) == EINVAL                                        # a null output
    assert call(n, du, ds, codes(0), P([a[3]])) == EINVAL                                        # an output is an input, even one P does not read
    assert call(n, du, ds, codes(0, 1), P([o[0], o[0]])) == EINVAL                               # two outputs are one array
    big = np.zeros(2 * n)
    assert call(n, du, ds, codes(0, 1), P([big[: n], big[n - 1: 2 * n - 1]])) == EINVAL          # ... or overlap by one point
    assert call(n, du, ds, codes(0, 1), P([big[: n], big[n:]])) == 0
    with pytest.raises(T.TlabError):
        T.gradient_maps(a[:9], None, "NOT_A_MAP")
    with pytest.raises(T.TlabError):
        T.gradient_maps(a[:9], a[9:], ["P", "Q"], out=o[:1])


# ---- the Fortran wrappers --------------------------------------------------------------------------------------------------------------------
def test_fortran_wrappers_compile_against_tlab_amd_c_alone(tmp_path):
    """tlab_amd_mappings.f90 depends on TLab_AMD_C alone, and a caller shaped like the enstrophy block of tools/statistics/averages.f90 compiles
    against it and links with the library"""
    fortran = os.path.join(ROOT, "tlab_amd", "fortran")
    fc = shutil.which("amdflang")
    mod = os.path.join(ROOT, "oracle", "_ref", "mod")                   # TLab_AMD_Check of tlab_amd_c.f90 writes through the reference's TLab_WorkFlow
    if fc is None or not os.path.isdir(mod):
        pytest.skip("amdflang or the reference's module files (oracle/_ref/mod) are not here")
    run = lambda *a: subprocess.run([fc, "-cpp", "-O2", "-fPIC", "-I", mod, "-module-dir", str(tmp_path), "-c", *a], cwd=tmp_path,      # noqa: E731
                                    capture_output=True, text=True)
    r = run(os.path.join(fortran, "tlab_amd_c.f90"), "-o", str(tmp_path / "c.o"))
    assert r.returncode == 0, r.stderr
    r = run("-I", str(tmp_path), os.path.join(fortran, "tlab_amd_mappings.f90"), "-o", str(tmp_path / "m.o"))
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(fortran, "tlab_amd_mappings.f90")).read()
    assert re.findall(r"^\s*use\s+(\w+)", src, flags=re.M | re.I) == ["TLab_AMD_C"]
    assert max(len(l) for l in src.splitlines()) <= 160
    names = ["Strain", "Strain_Tensor", "Curl", "Invariant_Q", "Invariant_R", "Vorticity_Production", "Vorticity_Diffusion", "Strain_Production",
             "Strain_Diffusion", "Strain_Pressure", "Gradient_Production", "Gradient_Diffusion", "Strain_A"]
    for nme in names:
        assert re.search(r"subroutine TLab_AMD_FI_%s\(" % nme, src), nme
    (tmp_path / "caller.f90").write_text(
        "subroutine caller(dns, imax, jmax, kmax, u, v, w, s, txc)\n"
        "    use TLab_AMD_C\n"
        "    use TLab_AMD_Mappings\n"
        "    type(c_ptr) :: dns\n"
        "    integer :: imax, jmax, kmax\n"
        "    real(c_double) :: u(imax*jmax*kmax), v(imax*jmax*kmax), w(imax*jmax*kmax), s(imax*jmax*kmax), txc(imax*jmax*kmax, 9)\n"
        "    call TLab_AMD_FI_Curl(dns, imax, jmax, kmax, u, v, w, txc(1, 1), txc(1, 2), txc(1, 3), txc(1, 7))\n"
        "    call TLab_AMD_FI_Vorticity_Production(dns, imax, jmax, kmax, u, v, w, txc(1, 1), txc(1, 2), txc(1, 3), txc(1, 4), txc(1, 5), txc(1, 6))\n"
        "    call TLab_AMD_FI_Vorticity_Diffusion(dns, imax, jmax, kmax, u, v, w, txc(1, 2), txc(1, 3), txc(1, 4), txc(1, 5), txc(1, 6), txc(1, 7))\n"
        "    call TLab_AMD_FI_Strain_A(dns, imax, jmax, kmax, s, u, v, w, txc(1, 1), txc(1, 2), txc(1, 3), txc(1, 4), txc(1, 5), txc(1, 6))\n"
        "    call TLab_AMD_FI_Invariant_R(dns, imax, jmax, kmax, u, v, w, txc(1, 1), txc(1, 2), txc(1, 3), txc(1, 4), txc(1, 5), txc(1, 6))\n"
        "end subroutine\n")
    r = run("-I", str(tmp_path), str(tmp_path / "caller.f90"), "-o", str(tmp_path / "caller.o"))
    assert r.returncode == 0, r.stderr
    r = subprocess.run([fc, "-shared", "-o", str(tmp_path / "libcaller.so"), str(tmp_path / "caller.o"), str(tmp_path / "m.o"), str(tmp_path / "c.o"),
                        "-Wl,--unresolved-symbols=ignore-all", "-L", os.path.join(ROOT, "tlab_amd"), "-ltlab_amd"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
