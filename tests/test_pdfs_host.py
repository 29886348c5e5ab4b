"""The plane PDFs without a GPU: the numpy restatement (tests/pdfs_oracle.py) against what the reference's own module PDFS gave
(tests/golden/pdfs_ref.npz, recorded by tests/golden/make_golden_pdfs.py), the composition of PDF1V_N from the restatement's parts, the host branch
of every entry point against the restatement bit for bit (tlab_init is never called here: every array is host memory), the argument checks, and the
Fortran module against the C interfaces.

Every comparison is np.array_equal on the whole output, bounds included; no tolerance exists in this feature.  equal_nan is set because PDF_ANALIZE
divides by nbins - 1: with nbins = 1 its interval is NaN in the reference too (the fixture holds those NaN), and a NaN must meet a NaN.
The refusal of mixed host and device arrays needs a device array: it is in tests/test_gpu_pdfs.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pdfs_oracle as P

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHAPES = [(20, 12, 8), (70, 33, 9), (20, 12, 1), (6, 1, 4)]
EINVAL = -1
vp = ctypes.c_void_p


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "pdfs_ref.npz"))
    return g, json.loads(str(g["index"]))


def _planes(a):
    nz, ny, nx = a.shape
    return [a[:, j, :] for j in range(ny)] + ([a] if ny > 1 else [])


def _fields(shape, n, seed):
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    off = np.cos(np.arange(ny))[None, :, None]
    return [np.ascontiguousarray(rng.uniform(-1, 1, (nz, ny, nx)) + off) for _ in range(n)]


def _gate(shape, seed):
    """about half of the points, plane 1 empty and plane 2 with one point (where the box has them)"""
    nx, ny, nz = shape
    g = (np.random.default_rng(seed).uniform(size=(nz, ny, nx)) > 0.5).astype(np.int8)
    if ny > 2:
        g[:, 1:3, :] = 0
        g[nz // 2, 2, nx // 2] = 1
    return g


# ---- the restatement against the reference's own module -------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_bit_for_bit(golden):
    g, index = golden
    kinds = {"pdf1v": 0, "analize": 0, "pdf2v": 0}
    for n, m in enumerate(index):
        ref = g["out_%d" % n]
        kinds[m["kind"]] += 1
        if m["kind"] == "pdf1v":
            a = g["in_%s_%s" % (m["box"], m["field"])]
            masks = _planes(g["in_%s_gate" % m["box"]] == 1) if m["igate"] else None
            for j, pts in enumerate(_planes(a)):
                got = P.pdf1v2d(m["ilim"], pts, m["umin"], m["umax"], m["nbins"], None if masks is None else masks[j])
                assert same(got, ref[j]), (m, j)
        elif m["kind"] == "analize":
            pdfs = g["out_%d" % m["of"]]
            for j in range(len(_planes(g["in_%s_u" % m["box"]]))):
                got = P.pdf_analize(m["ibc"], m["nbins"], pdfs[j], m["plim"])
                assert same(np.array(got, dtype=np.float64), ref[j]), (m, j)
        else:
            got = P.pdf2v(g["in_%s_%s" % (m["box"], m["u"])], g["in_%s_%s" % (m["box"], m["v"])], m["nbins"])
            assert same(got, ref), m
    assert min(kinds.values()) > 0, kinds


def test_the_reference_counts_below_umin_and_drops_umax(golden):
    """the two quirks of int(): in the fixture itself, field e on the external interval [0.25, 0.75] with 8 bins of 1/16"""
    g, index = golden
    n = next(n for n, m in enumerate(index) if m["kind"] == "pdf1v" and m["box"] == "b" and m["field"] == "e" and not m["igate"])
    e, vol = g["in_b_e"].ravel(), g["out_%d" % n][-1]
    assert e[1] == 0.75 and e[2] == 0.25 - 1.0 / 256 and e[3] == 0.25 - 1.0 / 64
    inside = np.count_nonzero((e >= 0.25) & (e < 0.75))
    below = np.count_nonzero((e > 0.25 - 1.0 / 16) & (e < 0.25))
    assert below >= 2 and vol[:8].sum() == inside + below            # q in (-1, 0) is counted (in bin 1), umax itself is not
    assert vol[0] == np.count_nonzero((e > 0.25 - 1.0 / 16) & (e < 0.25 + 1.0 / 16))


# ---- PDF1V_N from the restatement's parts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ibc", range(6))
def test_pdf1v_n_is_the_composition_of_its_parts(ibc):
    shape, nbins = (20, 12, 8), 32
    nx, ny, nz = shape
    a, = _fields(shape, 1, 3)
    got = P.pdf1v_n([a], nbins, [ibc], [-0.5], [0.8])[0]
    assert got.shape == (ny + 1, nbins + 2)
    for j, pts in enumerate(_planes(a)):
        if ibc == 0:
            ref = P.pdf1v2d(0, pts, -0.5, 0.8, nbins)
            q = (pts - (-0.5)) / ((0.8 - (-0.5)) / 32.0)
            assert ref[:nbins].sum() == np.count_nonzero((q > -1.0) & (q < 32)) < pts.size      # (the interval cuts some points off)
        else:
            ref = P.pdf1v2d(1, pts, 0.0, 0.0, nbins)
            assert ref[:nbins].sum() == pts.size                                 # a local interval loses no point
            step = (pts.max() - pts.min()) / nbins
            assert ref[nbins] == pts.min() + 0.5 * step and ref[nbins + 1] == pts.max() - 0.5 * step
            if ibc > 1:
                lo, hi, nplim = P.pdf_analize(ibc - 2, nbins, ref, 1.0e-4)
                assert 0 < nplim <= nbins and pts.min() - 1e-12 <= lo < hi <= pts.max() + 1e-12
                ref = P.pdf1v2d(0, pts, lo, hi, nbins)
        assert same(got[j], ref), j


# ---- the host branch of the entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_host_branch_equals_the_restatement_bit_for_bit(shape):
    import tlab_amd.operators as T
    nx, ny, nz = shape
    f = _fields(shape, 3, 5)
    f[2][:, ny // 2, :] = 0.75                                                    # a constant plane
    gate = _gate(shape, 6)
    ibcs = [0, 1, 2, 3, 4, 5]
    for nbins in (1, 2, 32, 100):
        for g, ig in ((None, 0), (gate, 1)):
            for ibc in ibcs:
                got = T.pdf1v_n(nx, ny, nz, f, nbins, ibc, -0.5, 0.8, g, ig)
                assert got.shape == (3, ny + 1, nbins + 2)
                assert same(got, P.pdf1v_n(f, nbins, [ibc] * 3, [-0.5] * 3, [0.8] * 3, g, ig)), (nbins, ig, ibc)
            got = T.pdf1v_n(nx, ny, nz, f, nbins, [0, 1, 4], [-0.5, 0.0, 0.0], [0.8, 0.0, 0.0], g, ig)      # the fields of one call may differ
            assert same(got, P.pdf1v_n(f, nbins, [0, 1, 4], [-0.5, 0, 0], [0.8, 0, 0], g, ig)), (nbins, ig)
    for nb2 in ((8, 8), (32, 5), (1, 3)):
        assert same(T.pdf2v(nx, ny, nz, nb2, f[0], f[1]), P.pdf2v(f[0], f[1], nb2)), nb2
    assert np.array_equal(T.gate_threshold(f[0].reshape(-1), 0.25), P.gate_threshold(f[0].reshape(-1), 0.25))
    pdf = P.pdf1v2d(1, f[0], 0.0, 0.0, 32)
    for ibc in range(4):
        assert same(np.array(T.pdf_analize(ibc, 32, pdf), dtype=np.float64), np.array(P.pdf_analize(ibc, 32, pdf, 1.0e-4), dtype=np.float64))


@pytest.mark.parametrize("shape", SHAPES)
def test_the_two_passes_on_their_own_equal_the_composed_call(shape):
    import tlab_amd.operators as T
    nx, ny, nz = shape
    f = _fields(shape, 2, 7)
    for g, ig in ((None, 0), (_gate(shape, 8), 1)):
        lo, hi = T.pdf_minmax_planes(nx, ny, nz, f, g, ig)
        assert lo.shape == hi.shape == (2, ny + 1)
        for v in range(2):
            m = None if g is None else (g == ig)
            for j in range(ny):
                assert (lo[v, j], hi[v, j]) == P.minmax(f[v][:, j, :], None if m is None else m[:, j, :])
            assert (lo[v, ny], hi[v, ny]) == P.minmax(f[v], m)
        got = T.pdf_histogram_planes(nx, ny, nz, f, 32, 1, lo, hi, g, ig)
        assert same(got, T.pdf1v_n(nx, ny, nz, f, 32, 1, None, None, g, ig))
        # ... and the third pass: the analysed intervals handed in as external ones
        alo, ahi = lo.copy(), hi.copy()
        for v in range(2):
            for j in range(ny + 1 if ny > 1 else 1):
                alo[v, j], ahi[v, j], _ = T.pdf_analize(0, 32, got[v, j])
        assert same(T.pdf_histogram_planes(nx, ny, nz, f, 32, 0, alo, ahi, g, ig), T.pdf1v_n(nx, ny, nz, f, 32, 2, None, None, g, ig))


def test_argument_errors_are_refused():
    import tlab_amd
    L = tlab_amd.load()
    nx, ny, nz, nb = 6, 4, 3, 8
    a = np.ones((nz, ny, nx))
    gate = np.ones((nz, ny, nx), dtype=np.int8)
    ibc = np.zeros(1, dtype=np.int32)
    lo, hi = np.zeros(ny + 1), np.ones(ny + 1)
    out = np.zeros((ny + 1) * (4096 + 2 + 2 * 4096))
    A_, G_, I_, LO, HI, O_ = (vp(x.ctypes.data) for x in (a, gate, ibc, lo, hi, out))
    one, null = (vp * 1)(a.ctypes.data), (vp * 1)(None)
    assert L.tlab_pdf1v_n(nx, ny, nz, 1, nb, I_, LO, HI, one, 0, None, O_) == 0
    assert L.tlab_pdf1v_n(nx, ny, nz, 1, 4096, I_, LO, HI, one, 1, G_, O_) == 0           # the compiled limit itself
    assert L.tlab_pdf_minmax_planes(nx, ny, nz, 1, one, 0, None, LO, HI) == 0
    lo[:], hi[:] = 0.0, 2.0
    assert L.tlab_pdf_histogram_planes(nx, ny, nz, 1, nb, I_, LO, HI, one, 0, None, O_) == 0
    for bad in ((0, ny, nz), (nx, 0, nz), (nx, ny, 0), (-1, ny, nz)):
        assert L.tlab_pdf1v_n(*bad, 1, nb, I_, LO, HI, one, 0, None, O_) == EINVAL
        assert L.tlab_pdf_minmax_planes(*bad, 1, one, 0, None, LO, HI) == EINVAL
        assert L.tlab_pdf_histogram_planes(*bad, 1, nb, I_, LO, HI, one, 0, None, O_) == EINVAL
        assert L.tlab_pdf2v(*bad, (ctypes.c_int * 2)(4, 4), A_, A_, O_) == EINVAL
    for nbins in (0, -3, 4097):                                                          # nbins < 1, nbins above the limit
        assert L.tlab_pdf1v_n(nx, ny, nz, 1, nbins, I_, LO, HI, one, 0, None, O_) == EINVAL
        assert L.tlab_pdf_histogram_planes(nx, ny, nz, 1, nbins, I_, LO, HI, one, 0, None, O_) == EINVAL
    assert b"4096" in L.tlab_last_error()
    assert L.tlab_pdf1v_n(nx, ny, nz, 0, nb, I_, LO, HI, one, 0, None, O_) == EINVAL      # nv < 1
    assert L.tlab_pdf1v_n(nx, ny, nz, 1, nb, I_, LO, HI, null, 0, None, O_) == EINVAL     # a null field
    assert L.tlab_pdf1v_n(nx, ny, nz, 1, nb, I_, LO, HI, None, 0, None, O_) == EINVAL
    assert L.tlab_pdf1v_n(nx, ny, nz, 1, nb, I_, LO, HI, one, 1, None, O_) == EINVAL      # igate != 0 with a null gate
    assert L.tlab_pdf_minmax_planes(nx, ny, nz, 1, one, 1, None, LO, HI) == EINVAL
    assert L.tlab_pdf_histogram_planes(nx, ny, nz, 1, nb, I_, LO, HI, one, 1, None, O_) == EINVAL
    assert L.tlab_pdf1v_n(nx, ny, nz, 1, nb, None, LO, HI, one, 0, None, O_) == EINVAL
    assert L.tlab_pdf1v_n(nx, ny, nz, 1, nb, I_, None, HI, one, 0, None, O_) == EINVAL    # ibc = 0 without its interval
    assert L.tlab_pdf1v_n(nx, ny, nz, 1, nb, I_, LO, HI, one, 0, None, None) == EINVAL
    for bad_ibc in (-1, 6):
        assert L.tlab_pdf1v_n(nx, ny, nz, 1, nb, vp(np.array([bad_ibc], dtype=np.int32).ctypes.data), LO, HI, one, 0, None, O_) == EINVAL
    assert L.tlab_pdf2v(nx, ny, nz, (ctypes.c_int * 2)(64, 64), A_, A_, O_) == 0
    for nb2 in ((0, 4), (4, 0), (65, 64), (2048, 2)):                                     # the product above 4096; nbins(1) above 1024
        assert L.tlab_pdf2v(nx, ny, nz, (ctypes.c_int * 2)(*nb2), A_, A_, O_) == EINVAL, nb2
    assert L.tlab_pdf2v(nx, ny, nz, (ctypes.c_int * 2)(4, 4), None, A_, O_) == EINVAL
    assert L.tlab_pdf2v(nx, ny, nz, None, A_, A_, O_) == EINVAL
    d = ctypes.c_double(0.0)
    n = ctypes.c_int(0)
    assert L.tlab_pdf_analize(0, 0, O_, ctypes.byref(d), ctypes.byref(d), 1e-4, ctypes.byref(n)) == EINVAL
    assert L.tlab_pdf_analize(0, 8, None, ctypes.byref(d), ctypes.byref(d), 1e-4, ctypes.byref(n)) == EINVAL
    assert L.tlab_gate_threshold(A_, 0, 0.5, G_) == EINVAL
    assert L.tlab_gate_threshold(None, a.size, 0.5, G_) == EINVAL
    assert L.tlab_gate_threshold(A_, a.size, 0.5, None) == EINVAL
    assert b"tlab_gate_threshold" in L.tlab_last_error()


# ---- the Fortran module ---------------------------------------------------------------------------------------------------------------------
def test_pdfs_module_compiles_and_links_against_a_caller(tmp_path):
    """tlab_amd/fortran/tlab_amd_pdfs.f90 depends on TLab_AMD_C alone (outside its USE_MPI blocks, which are not compiled here), and a caller shaped
    like the block stats_pdfs of DNS_STATISTICS (dns_statistics.f90:122-148) compiles against it and links with the library"""
    fortran = os.path.join(ROOT, "tlab_amd", "fortran")
    fc = shutil.which("amdflang")
    mod = os.path.join(ROOT, "oracle", "_ref", "mod")                   # TLab_AMD_Check of tlab_amd_c.f90 writes through the reference's TLab_WorkFlow
    if fc is None or not os.path.isdir(mod):
        pytest.skip("amdflang or the reference's module files (oracle/_ref/mod) are not here")
    run = lambda *a: subprocess.run([fc, "-cpp", "-O2", "-fPIC", "-I", mod, "-module-dir", str(tmp_path), "-c", *a], cwd=tmp_path,      # noqa: E731
                                    capture_output=True, text=True)
    r = run(os.path.join(fortran, "tlab_amd_c.f90"), "-o", str(tmp_path / "c.o"))
    assert r.returncode == 0, r.stderr
    r = run("-I", str(tmp_path), os.path.join(fortran, "tlab_amd_pdfs.f90"), "-o", str(tmp_path / "p.o"))
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(fortran, "tlab_amd_pdfs.f90")).read()
    serial = re.sub(r"^#ifdef USE_MPI\n.*?^#e(?:lse|ndif)\n", "", src, flags=re.M | re.S)
    assert re.findall(r"^\s*use\s+(\w+)", serial, flags=re.M | re.I) == ["TLab_AMD_C"]
    assert max(len(l) for l in src.splitlines()) <= 160
    (tmp_path / "caller.f90").write_text(
        "subroutine caller(q, s, p, gate, pdf, pdf2, imax, jmax, kmax, inb_scal)\n"
        "    use TLab_AMD_C\n"
        "    use TLab_AMD_PDFs\n"
        "    integer :: imax, jmax, kmax, inb_scal, nfield, is, ibc(16), nbins(2)\n"
        "    real(c_double), target :: q(imax*jmax*kmax, 3), s(imax*jmax*kmax, inb_scal), p(imax*jmax*kmax)\n"
        "    real(c_double) :: pdf(34, jmax + 1, 4 + inb_scal), pdf2(8*8 + 2 + 2*8, jmax + 1), vmin(16), vmax(16)\n"
        "    integer(1) :: gate(*), igate\n"
        "    type(c_ptr) :: vars(16)\n"
        "    nfield = 0\n"
        "    nfield = nfield + 1; vars(nfield) = c_loc(q(:, 1))\n"
        "    nfield = nfield + 1; vars(nfield) = c_loc(q(:, 2))\n"
        "    nfield = nfield + 1; vars(nfield) = c_loc(q(:, 3))\n"
        "    nfield = nfield + 1; vars(nfield) = c_loc(p)\n"
        "    do is = 1, inb_scal\n"
        "        nfield = nfield + 1; vars(nfield) = c_loc(s(:, is))\n"
        "    end do\n"
        "    ibc(1:nfield) = 2; igate = 0_1; nbins = 8\n"
        "    call TLab_AMD_PDF1V_N(imax, jmax, kmax, nfield, 32, ibc, vmin, vmax, vars, igate, gate, pdf)\n"
        "    call TLab_AMD_PDF2V(imax, jmax, kmax, nbins, q(:, 1), s(:, 1), pdf2)\n"
        "end subroutine caller\n")
    r = run("-I", str(tmp_path), str(tmp_path / "caller.f90"), "-o", str(tmp_path / "caller.o"))
    assert r.returncode == 0, r.stderr
    import tlab_amd
    r = subprocess.run([fc, "-shared", "-o", str(tmp_path / "libcaller.so"), str(tmp_path / "caller.o"), str(tmp_path / "p.o"), str(tmp_path / "c.o"),
                        "-Wl,--unresolved-symbols=ignore-all", "-L", os.path.dirname(tlab_amd.lib_path()), "-ltlab_amd"], cwd=tmp_path,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nm = subprocess.run(["nm", "-D", "--undefined-only", str(tmp_path / "libcaller.so")], capture_output=True, text=True).stdout
    assert "tlab_pdf1v_n" in nm and "tlab_pdf2v" in nm
