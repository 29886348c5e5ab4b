"""The plane spectra and correlations without a GPU: the numpy restatement tests/spectra_oracle.py and the host branch of the C entry points
(tlab_spectrum_reduce, tlab_correlation_reduce, tlab_radial_samplesize with host arrays: the reference's loops in csrc/spectra.cpp) against
tests/golden/spectra_ref.npz, which tests/golden/make_golden_spectra.py recorded from the reference's own compiled module SpectraMod.

Every comparison is np.array_equal, on the exact-data records and on the rounding-data records alike: both restatements keep the reference's
order in every floating-point sum, so they give its bits."""
import functools
import json
import os

import numpy as np
import pytest

import spectra_oracle as S

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xz", "x", "z", "r", "variance")


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(HERE, "golden", "spectra_ref.npz"))
    return g, json.loads(str(g["index"]))


def records(kind):
    return [(n, r) for n, r in enumerate(golden()[1]) if r["kind"] == kind]


def ids(kind):
    return ["%s-nblock%d%s" % (r["box"], r.get("nblock", 0), "-cross" if r.get("cross") else "") for _, r in records(kind)]


def box(r):
    return tuple(int(v) for v in r["box"].split("x"))


def test_the_fixture_holds_every_case():
    g, index = golden()
    boxes = {r["box"] for r in index}
    assert boxes == {"16x5x8", "32x7x16", "8x4x32", "256x2x16", "20x6x12", "12x3x9", "130x3x4"}
    assert {r["nblock"] for r in index if r["box"] == "32x7x16" and r["kind"] == "spectrum"} == {1, 2, 3}
    assert any(r["exact"] for r in index) and any(not r["exact"] for r in index if r["kind"] != "samplesize")
    assert os.path.getsize(os.path.join(HERE, "golden", "spectra_ref.npz")) < 512 * 1024


@pytest.mark.parametrize("n,r", records("spectrum"), ids=ids("spectrum"))
def test_restatement_of_reduce_and_integrate_spectrum(n, r):
    g, _ = golden()
    nx, ny, nz = box(r)
    o = S.spectrum(nx, ny, nz, r["nblock"], r["kr_total"], g["ah_" + r["box"]], g["bh_" + r["box"]] if r["cross"] else None)
    for k in KEYS:
        assert np.array_equal(o[k], g["%s_%d" % (k, n)]), k


@pytest.mark.parametrize("n,r", records("correlation"), ids=ids("correlation"))
def test_restatement_of_reduce_correlation(n, r):
    g, _ = golden()
    nx, ny, nz = box(r)
    o = S.correlation(nx, ny, nz, r["nblock"], r["nr_total"], g["field_" + r["box"]], g["var1_" + r["box"]], g["var2_" + r["box"]])
    for k in KEYS:
        assert np.array_equal(o[k], g["%s_%d" % (k, n)]), k


@pytest.mark.parametrize("n,r", records("samplesize"), ids=ids("samplesize"))
def test_radial_samplesize(n, r):
    import tlab_amd.operators as O
    g, _ = golden()
    nx, _, nz = box(r)
    assert np.array_equal(S.radial_samplesize(nx, nz, r["nr_total"]), g["samplesize_%d" % n])
    assert np.array_equal(O.radial_samplesize(nx, nz, r["nr_total"]), g["samplesize_%d" % n])


@pytest.mark.parametrize("n,r", records("spectrum"), ids=ids("spectrum"))
def test_host_branch_of_tlab_spectrum_reduce(n, r):
    import tlab_amd.operators as O
    g, _ = golden()
    nx, ny, nz = box(r)
    ah = np.ascontiguousarray(g["ah_" + r["box"]])
    bh = np.ascontiguousarray(g["bh_" + r["box"]]) if r["cross"] else None
    o = O.spectrum_reduce(nx, ny, nz, r["nblock"], r["kr_total"], ah, bh, out2d=True)
    for k in KEYS:
        assert np.array_equal(o[k], g["%s_%d" % (k, n)]), k
    # the outputs are accumulated into, the variance is written
    o2 = O.spectrum_reduce(nx, ny, nz, r["nblock"], r["kr_total"], ah, bh, out={k: o[k] for k in ("x", "z", "r")})
    assert np.array_equal(o2["variance"], g["variance_%d" % n])
    if r["exact"]:
        assert np.array_equal(o2["x"], 2.0 * g["x_%d" % n]) and np.array_equal(o2["r"], 2.0 * g["r_%d" % n])


@pytest.mark.parametrize("n,r", records("correlation"), ids=ids("correlation"))
def test_host_branch_of_tlab_correlation_reduce(n, r):
    import tlab_amd.operators as O
    g, _ = golden()
    nx, ny, nz = box(r)
    f = np.ascontiguousarray(g["field_" + r["box"]])
    o = O.correlation_reduce(nx, ny, nz, r["nblock"], r["nr_total"], f, g["var1_" + r["box"]], g["var2_" + r["box"]], out2d=True)
    for k in KEYS:
        assert np.array_equal(o[k], g["%s_%d" % (k, n)]), k
    o = O.correlation_reduce(nx, ny, nz, r["nblock"], r["nr_total"], f, g["var1_" + r["box"]], g["var2_" + r["box"]], icalc_radial=0)
    assert "r" not in o and np.array_equal(o["x"], g["x_%d" % n]) and np.array_equal(o["z"], g["z_%d" % n])


def test_host_cross_product_and_fluctuation_and_covariances():
    import tlab_amd.operators as O
    g, _ = golden()
    ah, bh = np.ascontiguousarray(g["ah_20x6x12"]), np.ascontiguousarray(g["bh_20x6x12"])
    c = O.cross_product(ah, bh, np.zeros_like(ah))
    assert np.array_equal(c.real, S.product(ah, bh)) and np.array_equal(c.imag, bh.imag * ah.real - bh.real * ah.imag)
    c = O.cross_product(ah.copy())
    assert np.array_equal(c.real, S.product(ah)) and not c.imag.any()
    f = np.ascontiguousarray(g["field_20x6x12"]) + np.cos(np.arange(6))[None, :, None]
    nz, ny, nx = f.shape
    fl = O.fluctuation(nx, ny, nz, f, O.avg_ik_v(nx, ny, nz, [f])[0], np.zeros_like(f))
    assert np.array_equal(fl, S.fluctuation(f))
    h = np.ascontiguousarray(g["field_20x6x12"][::-1])
    cov = O.avg_cov2v(nx, ny, nz, fl, h)
    assert np.array_equal(cov, np.stack([S.cov2v2d(fl, h), S.cov2v2d(fl, fl), S.cov2v2d(h, h)]))


def test_index_maps_against_the_fft_shift():
    """the kz shuffle is numpy's fftshift for even nz, and the fold puts every position on |kz| with the Nyquist mode on its neighbour"""
    for nz in (4, 8, 12, 32):
        assert np.array_equal(S.shuffle(nz), np.fft.fftshift(np.arange(nz)))
        kz = np.abs(np.fft.fftshift(np.fft.fftfreq(nz, 1.0 / nz))).astype(int)
        want = np.where(kz == nz // 2, max(nz // 2 - 1, 0), kz)
        assert [S.fold(ks, nz)[0] - 1 for ks in range(nz)] == list(want)


def test_refusals_on_host_arrays():
    import tlab_amd as T
    L = T.load()
    a = np.zeros((4, 3, 5), dtype=np.complex128)
    o = [np.zeros(64) for _ in range(5)]
    p = lambda x: x.ctypes.data      # noqa: E731
    call = lambda nx, ny, nz, nb, kr: L.tlab_spectrum_reduce(nx, ny, nz, nb, kr, p(a), None, None, p(o[0]), p(o[1]), p(o[2]), p(o[3]))      # noqa: E731
    assert call(8, 3, 4, 1, 2) == 0
    assert call(7, 3, 4, 1, 2) == -1                 # odd nx: TLAB_EINVAL
    assert call(8, 3, 4, 0, 2) == -1                 # nblock = 0
    assert call(8, 3, 1, 1, 1) == -2                 # nz = 1: TLAB_EUNSUPPORTED
    f = np.zeros((4, 3, 8))
    corr = lambda nx, nz, nb: L.tlab_correlation_reduce(nx, 3, nz, nb, 2, p(f), p(o[4]), p(o[4]), None, p(o[0]), p(o[1]), p(o[2]), p(o[3]), 1)      # noqa: E731
    assert corr(8, 4, 1) == 0 and corr(7, 4, 1) == -1 and corr(8, 4, 0) == -1 and corr(8, 1, 1) == -2


def test_the_new_symbols_are_exported_and_bound():
    import ctypes
    import tlab_amd
    from tlab_amd import lib as tl
    L = ctypes.CDLL(tlab_amd.lib_path())
    hdr = open(os.path.join(HERE, "..", "include", "tlab_amd.h")).read()
    for name in ("tlab_spectrum_reduce", "tlab_correlation_reduce", "tlab_radial_samplesize", "tlab_cross_product", "tlab_fluctuation",
                 "tlab_avg_cov2v", "tlab_spectra_pair", "tlab_dns_spectra"):
        assert hasattr(L, name) and name in tl.SIGNATURES and ("int %s(" % name) in hdr, name


def test_spectra_module_compiles_and_links_against_a_caller(tmp_path):
    """tlab_amd/fortran/tlab_amd_spectra.f90 depends on TLab_AMD_C alone, is part of the Fortran build, and a caller shaped like the loop body of
    tools/statistics/spectra.f90:640-659 compiles against it and links with the library"""
    import re
    import shutil
    import subprocess
    root = os.path.abspath(os.path.join(HERE, ".."))
    fortran = os.path.join(root, "tlab_amd", "fortran")
    assert "tlab_amd_spectra.f90" in open(os.path.join(fortran, "Makefile")).read()
    fc = shutil.which("amdflang")
    mod = os.path.join(root, "oracle", "_ref", "mod")                   # TLab_AMD_Check of tlab_amd_c.f90 writes through the reference's TLab_WorkFlow
    if fc is None or not os.path.isdir(mod):
        pytest.skip("amdflang or the reference's module files (oracle/_ref/mod) are not here")
    run = lambda *a: subprocess.run([fc, "-cpp", "-O2", "-fPIC", "-I", mod, "-module-dir", str(tmp_path), "-c", *a], cwd=tmp_path,      # noqa: E731
                                    capture_output=True, text=True)
    r = run(os.path.join(fortran, "tlab_amd_c.f90"), "-o", str(tmp_path / "c.o"))
    assert r.returncode == 0, r.stderr
    r = run("-I", str(tmp_path), os.path.join(fortran, "tlab_amd_spectra.f90"), "-o", str(tmp_path / "s.o"))
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(fortran, "tlab_amd_spectra.f90")).read()
    assert re.findall(r"^\s*use\s+(\w+)", src, flags=re.M | re.I) == ["TLab_AMD_C"]
    assert max(len(l) for l in src.splitlines()) <= 160
    (tmp_path / "caller.f90").write_text(
        "subroutine caller(plan, flag_mode, a, b, txc, outx, outz, outr, out2d, wrk1d, samplesize, imax, jmax, kmax, opt_block, kr_total)\n"
        "    use TLab_AMD_C\n"
        "    use TLab_AMD_Spectra\n"
        "    type(c_ptr) :: plan\n"
        "    integer :: flag_mode, imax, jmax, kmax, opt_block, kr_total\n"
        "    real(c_double), target :: a(imax*jmax*kmax), b(imax*jmax*kmax), txc((imax + 2)*jmax*kmax, 4)\n"
        "    real(c_double), target :: outx(*), outz(*), outr(*), out2d(*)\n"
        "    real(c_double) :: wrk1d(jmax, 4), samplesize(kr_total)\n"
        "    if (flag_mode == 1) then\n"
        "        call TLab_AMD_Reduce_Spectrum(imax, jmax, kmax, opt_block, kr_total, txc(:, 1), outx, outz, outr, wrk1d(:, 4), b_hat=txc(:, 2))\n"
        "        call TLab_AMD_Integrate_Spectrum(imax, jmax, kmax, opt_block, kr_total, txc(:, 1), outx, outz, outr, wrk1d(:, 4), out2d=out2d)\n"
        "    else\n"
        "        call TLab_AMD_Reduce_Correlation(imax, jmax, kmax, opt_block, kr_total, txc(:, 2), out2d, outx, outz, outr, wrk1d(:, 2:3), &\n"
        "                                         wrk1d(:, 4), 1)\n"
        "        call TLab_AMD_Radial_Samplesize(imax, kmax, kr_total, samplesize)\n"
        "    end if\n"
        "    call TLab_AMD_Spectra_Pair(plan, flag_mode, opt_block, kr_total, a, txc(:, 1), txc(:, 2), txc(:, 3), outx, outz, outr, wrk1d(:, 1:3), &\n"
        "                               wrk1d(:, 4), b=b, out2d=out2d)\n"
        "end subroutine caller\n")
    r = run("-I", str(tmp_path), str(tmp_path / "caller.f90"), "-o", str(tmp_path / "caller.o"))
    assert r.returncode == 0, r.stderr
    import tlab_amd
    r = subprocess.run([fc, "-shared", "-o", str(tmp_path / "libcaller.so"), str(tmp_path / "caller.o"), str(tmp_path / "s.o"), str(tmp_path / "c.o"),
                        "-Wl,--unresolved-symbols=ignore-all", "-L", os.path.dirname(tlab_amd.lib_path()), "-ltlab_amd"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nm = subprocess.run(["nm", "-D", "--undefined-only", str(tmp_path / "libcaller.so")], capture_output=True, text=True).stdout
    for name in ("tlab_spectrum_reduce", "tlab_correlation_reduce", "tlab_radial_samplesize", "tlab_spectra_pair"):
        assert name in nm, name
