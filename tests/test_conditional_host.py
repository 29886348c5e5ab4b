"""The conditional statistics without a GPU: the numpy restatement (tests/conditional_oracle.py) against what the reference's own compiled routines
gave (tests/golden/conditional_ref.npz, recorded by tests/golden/make_golden_conditional.py: AVG1V2D, AVG1V2D1G, PDF1V2D / PDF1V2D1G / PDF2V2D with
a and avg, RAW_TO_CENTRAL), the host branch of every new entry point against the same records (tlab_init is never called here: every array is host
memory), the reference's quirks, the argument checks, and the Fortran wrappers against the C interfaces.

Every comparison is np.array_equal on the whole output, rounding data included: the host branch keeps the reference's order and its integer power.
The refusal of mixed host and device arrays needs a device array: it is in tests/test_gpu_conditional.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import conditional_oracle as C
import pdfs_oracle as P

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EUNSUPPORTED = -1, -2
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "conditional_ref.npz"))
    return g, json.loads(str(g["index"]))


def _field(g, box, name):
    """a field of a record: stored, or one of the two derived ones (make_golden_conditional.py)"""
    if name == "c":
        c = g["in_%s_u" % box].copy()
        c[:, c.shape[1] // 2, :] = 0.75
        return c
    if name == "uv":
        return g["in_%s_u" % box] * g["in_%s_v" % box]
    return np.ascontiguousarray(g["in_%s_%s" % (box, name)])


def _records(golden, kind):
    g, index = golden
    recs = [(m, g["out_%d" % n]) for n, m in enumerate(index) if m["kind"] == kind]
    assert recs
    return g, recs


# ---- the restatement against the reference's compiled routines ----------------------------------------------------------------------------------
def test_restated_moments_equal_the_reference_bit_for_bit(golden):
    g, recs = _records(golden, "moments")
    for m, ref in recs:
        a, gate = _field(g, m["box"], m["field"]), g["in_%s_gate" % m["box"]]
        for j in range(a.shape[1]):
            for mom in range(1, 11):
                assert C.avg1v2d(a, j, mom) == ref[0, mom - 1, j], (m, j, mom)
                for lev in (1, 2, 3):
                    assert C.avg1v2d1g(a, j, lev, mom, gate) == ref[lev, mom - 1, j], (m, j, mom, lev)


def test_a_naive_power_is_not_the_reference(golden):
    """why the restatement spells the power out: x**m of numpy differs from the reference's for some m >= 3 on rounding data"""
    g, recs = _records(golden, "moments")
    m, ref = next(r for r in recs if r[0]["box"] == "a" and r[0]["field"] == "u")
    a = _field(g, "a", "u")
    naive = np.array([[C.seqsum(a[:, j, :].ravel() ** mom) / a[:, j, :].size for j in range(a.shape[1])] for mom in range(1, 11)])
    assert np.array_equal(naive[:2], ref[0, :2]) and not np.array_equal(naive[2:], ref[0, 2:])


def test_restated_conditional_averages_equal_the_reference_bit_for_bit(golden):
    g, recs = _records(golden, "cavg1v")
    seen = set()
    for m, ref in recs:
        u, a, gate, nb = _field(g, m["box"], m["field"]), _field(g, m["box"], m["a"]), g["in_%s_gate" % m["box"]], m["nbins"]
        masks = P._planes(gate == m["igate"]) if m["igate"] else None
        for j, (pu, pa) in enumerate(zip(P._planes(u), P._planes(a))):
            pdf, s, _ = C.cavg1v2d(m["ilim"], pu, pa, m["umin"], m["umax"], nb, None if masks is None else masks[j])
            assert np.array_equal(pdf, ref[j, :, 0]), (m, j)
            assert np.array_equal(C.divide(s, pdf[:nb]), ref[j, :nb, 1]), (m, j)
        seen.add((m["ilim"], nb))
    assert seen >= {(il, nb) for il in (0, 1) for nb in (1, 2, 32, 100)}
    g, recs = _records(golden, "cavg2v")
    for m, ref in recs:
        got, _ = C.cavg2v(_field(g, m["box"], "u"), _field(g, m["box"], "v"), _field(g, m["box"], m["a"]), m["nbins"])
        nb = m["nbins"][0] * m["nbins"][1]
        assert np.array_equal(got[:, nb:], ref[:, nb:, 0]) and np.array_equal(got[:, :nb], ref[:, :nb, 1]), m
        assert np.array_equal(P.pdf2v(_field(g, m["box"], "u"), _field(g, m["box"], "v"), m["nbins"]), ref[:, :, 0]), m


def test_restated_raw_to_central_equals_the_reference_bit_for_bit(golden):
    g, recs = _records(golden, "central")
    assert sorted(m["nm"] for m, _ in recs) == list(range(2, 11))
    for m, ref in recs:
        assert np.array_equal(C.raw_to_central(g["central_in"][:m["nm"]]), ref[:m["nm"]]), m


# ---- the host branch of the entry points against the same records -------------------------------------------------------------------------------
def test_host_moments_equal_the_reference_bit_for_bit(golden):
    import tlab_amd.operators as T
    g, recs = _records(golden, "moments")
    for m, ref in recs:
        a, gate = _field(g, m["box"], m["field"]), np.ascontiguousarray(g["in_%s_gate" % m["box"]])
        nz, ny, nx = a.shape
        for np_, rows in ((0, ref[:1]), (3, ref[1:])):
            avg, sums, ns = T.avg_n_xz(nx, ny, nz, [a, a], 10, np_, gate if np_ else None, raw=True)
            assert avg.shape == sums.shape == (max(np_, 1), 2, 10, ny) and ns.shape == (max(np_, 1), ny)
            mask = [np.ones_like(gate, dtype=bool)] if np_ == 0 else [gate == l for l in (1, 2, 3)]
            assert np.array_equal(ns, np.array([k.sum(axis=(0, 2)) for k in mask]))
            raw = np.divide(sums, ns[:, None, None, :], out=sums.copy(), where=ns[:, None, None, :] > 0)
            assert np.array_equal(raw[:, 0], rows) and np.array_equal(raw[:, 1], rows), (m, np_)
            # avg is RAW_TO_CENTRAL of the reference's raw moments, for every nm
            for nm in (1, 2, 4, 10):
                got = T.avg_n_xz(nx, ny, nz, [a], nm, np_, gate if np_ else None)
                for l in range(max(np_, 1)):
                    for j in range(ny):
                        want = T.raw_to_central(rows[l, :nm, j]) if nm > 1 else rows[l, :1, j]
                        assert np.array_equal(got[l, 0, :, j], want), (m, np_, nm, l, j)
            assert np.array_equal(avg, C.central_of(sums, ns))


def test_host_raw_to_central_equals_the_reference_bit_for_bit(golden):
    import tlab_amd.operators as T
    g, recs = _records(golden, "central")
    for m, ref in recs:
        assert np.array_equal(T.raw_to_central(g["central_in"][:m["nm"]]), ref[:m["nm"]]), m
    assert np.array_equal(T.raw_to_central([0.375]), [0.375])


def test_host_conditional_averages_equal_the_reference_bit_for_bit(golden):
    import tlab_amd.operators as T
    g, recs = _records(golden, "cavg1v")
    for m, ref in recs:
        u, a, gate, nb = _field(g, m["box"], m["field"]), _field(g, m["box"], m["a"]), np.ascontiguousarray(g["in_%s_gate" % m["box"]]), m["nbins"]
        nz, ny, nx = u.shape
        avg, s, pdf = T.cavg1v_n(nx, ny, nz, [u, u], a, nb, m["ilim"], m["umin"], m["umax"], gate if m["igate"] else None, m["igate"], raw=True)
        for v in (0, 1):
            assert np.array_equal(pdf[v], ref[:, :, 0]), m
            assert np.array_equal(avg[v, :, :nb], ref[:, :nb, 1]) and np.array_equal(avg[v, :, nb:], ref[:, nb:, 0]), m      # the two coordinates stay
            assert np.array_equal(C.divide(s[v, :, :nb], pdf[v, :, :nb]), ref[:, :nb, 1]) and np.array_equal(s[v, :, nb:], ref[:, nb:, 0]), m
        assert np.array_equal(T.cavg1v_n(nx, ny, nz, [u], a, nb, m["ilim"], m["umin"], m["umax"], gate if m["igate"] else None, m["igate"])[0], avg[0])
    g, recs = _records(golden, "cavg2v")
    for m, ref in recs:
        u, v, a = (_field(g, m["box"], k) for k in ("u", "v", m["a"]))
        nz, ny, nx = u.shape
        nb = m["nbins"][0] * m["nbins"][1]
        got = T.cavg2v(nx, ny, nz, m["nbins"], u, v, a)
        assert np.array_equal(got[:, :nb], ref[:, :nb, 1]) and np.array_equal(got[:, nb:], ref[:, nb:, 0]), m


def test_host_gates_equal_the_restatement():
    import tlab_amd.operators as T
    rng = np.random.default_rng(3)
    a = rng.integers(-4, 5, 4001).astype(np.float64) / 2.0
    v = rng.integers(-2, 3, 4001).astype(np.float64)
    for thr in ([], [0.5], [-1.0, -0.5, 0.5, 1.5], list(np.linspace(-2.0, 2.0, 126))):      # igate_size 1, 2, 5, 127; thresholds ON data values
        got = T.gate_levels(a, thr)
        assert got.dtype == np.int8 and np.array_equal(got, C.gate_levels(a, thr)), len(thr)
    got = T.gate_levels(a, [-1.0, -0.5, 0.5, 1.5])
    assert np.all(got[a == 0.5] == 4) and np.all(got[a == 0.0] == 3) and np.all(got[a == 2.0] == 5) and np.all(got[a == -2.0] == 1)      # a < thr, not <=
    assert np.array_equal(T.gate_flux(a, v), C.gate_flux(a, v))
    q = T.gate_flux(np.array([0.0, 0.0, 0.0, 1.0, 1.0, -1.0, -1.0, -1.0]), np.array([0.0, 1.0, -1.0, 0.0, -1.0, 0.0, 1.0, -1.0]))
    assert list(q) == [4, 2, 4, 1, 4, 3, 2, 3]                                                  # exactly the reference's >, >=, <=, <


# ---- the reference's quirks ----------------------------------------------------------------------------------------------------------------
def test_reference_quirks(golden):
    import tlab_amd.operators as T
    g, _ = golden
    u, v, gate = _field(g, "a", "u"), _field(g, "a", "v"), np.ascontiguousarray(g["in_a_gate"])
    nz, ny, nx = u.shape
    # an empty level gives 0: plane 1 has no point of level 2; plane 2 has one point of level 3: its moments are the powers, its central moments 0
    avg, sums, ns = T.avg_n_xz(nx, ny, nz, [u], 4, 3, gate, raw=True)
    assert ns[1, 1] == 0 and np.all(avg[1, 0, :, 1] == 0.0) and np.all(sums[1, 0, :, 1] == 0.0)
    one = u[nz // 2, 2, nx // 2]
    assert ns[2, 2] == 1 and avg[2, 0, 0, 2] == one and sums[2, 0, 1, 2] == one * one
    # ustep == 0 puts everything into bin 1: the constant plane of field c with a local interval
    c = _field(g, "a", "c")
    avg, s, pdf = T.cavg1v_n(nx, ny, nz, [c], v, 32, 1, raw=True)
    j = ny // 2
    assert pdf[0, j, 0] == nx * nz and pdf[0, j, 1:32].sum() == 0 and s[0, j, 0] == C.seqsum(v[:, j, :]) and pdf[0, j, 32] == pdf[0, j, 33] == 0.75
    # ilim = 0 drops outside points from sum and count alike
    avg, s, pdf = T.cavg1v_n(nx, ny, nz, [u], v, 8, 0, -0.5, 0.8, raw=True)
    q = (u - (-0.5)) / ((0.8 - (-0.5)) / 8.0)
    inside = (q > -1.0) & (q < 8)
    assert 0 < inside.sum() < u.size and pdf[0, ny, :8].sum() == inside.sum()
    ok, b = P.bins(u.ravel(), -0.5, P.step(-0.5, 0.8, 8)[0], 8, True)
    assert np.array_equal(ok, inside.ravel())
    for up in range(8):                                              # the volume's sums: the points of a bin in their order, nothing from outside
        assert s[0, ny, up] == C.seqsum(v.ravel()[ok & (b == up)]), up
    # CAVG1V_N keeps the two coordinates, and the volume plane is zero when ny == 1
    assert avg[0, 0, 8] == -0.5 + 0.5 * (1.3 / 8.0) and avg[0, 0, 9] == 0.8 - 0.5 * (1.3 / 8.0)
    uc, vc = _field(g, "c", "u"), _field(g, "c", "v")
    assert np.all(T.cavg1v_n(6, 1, 4, [uc], vc, 8, 1)[0, 1] == 0.0) and np.all(T.cavg2v(6, 1, 4, (4, 2), uc, vc, vc)[1] == 0.0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_refused():
    import tlab_amd
    L = tlab_amd.load()
    nx, ny, nz = 6, 4, 3
    a = np.ones((nz, ny, nx))
    gate = np.ones((nz, ny, nx), dtype=np.int8)
    out = np.zeros(127 * 10 * ny * 2 + (ny + 1) * (1024 + 2 + 2 * 1024))
    ns = np.zeros(127 * ny, dtype=np.int64)
    ibc = np.ones(1, dtype=np.int32)
    thr = np.linspace(0.0, 1.0, 126)
    A_, G_, O_, N_, I_, T_ = (vp(x.ctypes.data) for x in (a, gate, out, ns, ibc, thr))
    one, null = (vp * 1)(a.ctypes.data), (vp * 1)(None)
    assert L.tlab_avg_n_xz(nx, ny, nz, 1, 10, one, 127, G_, O_, O_, N_) == 0                     # the limits themselves
    assert L.tlab_avg_n_xz(nx, ny, nz, 1, 11, one, 0, None, O_, None, None) == EINVAL             # nm = 11
    assert L.tlab_avg_n_xz(nx, ny, nz, 1, 0, one, 0, None, O_, None, None) == EINVAL
    assert L.tlab_avg_n_xz(nx, ny, nz, 1, 4, one, 128, G_, O_, None, None) == EINVAL              # np = 128
    assert b"127" in L.tlab_last_error()
    assert L.tlab_avg_n_xz(nx, ny, nz, 1, 4, one, -1, G_, O_, None, None) == EINVAL
    assert L.tlab_avg_n_xz(nx, ny, nz, 1, 4, one, 2, None, O_, None, None) == EINVAL              # levels without a gate
    assert L.tlab_avg_n_xz(nx, ny, nz, 1, 4, one, 0, None, None, None, None) == EINVAL            # no output at all
    assert L.tlab_avg_n_xz(nx, ny, nz, 1, 4, one, 0, None, None, None, N_) == 0                   # any one will do
    assert L.tlab_avg_n_xz(nx, ny, nz, 0, 4, one, 0, None, O_, None, None) == EINVAL
    assert L.tlab_avg_n_xz(nx, ny, nz, 1, 4, null, 0, None, O_, None, None) == EINVAL
    for bad in ((0, ny, nz), (nx, 0, nz), (nx, ny, 0)):
        assert L.tlab_avg_n_xz(*bad, 1, 4, one, 0, None, O_, None, None) == EINVAL
        assert L.tlab_cavg1v_n(*bad, 1, 8, I_, None, None, one, 0, None, A_, O_, None, None) == EINVAL
        assert L.tlab_cavg2v(*bad, (ctypes.c_int * 2)(4, 4), A_, A_, A_, O_) == EINVAL
    assert L.tlab_raw_to_central(11, O_) == EINVAL and L.tlab_raw_to_central(0, O_) == EINVAL and L.tlab_raw_to_central(4, None) == EINVAL
    assert L.tlab_gate_levels(A_, a.size, 127, T_, G_) == 0
    assert L.tlab_gate_levels(A_, a.size, 0, T_, G_) == EINVAL                                    # igate_size = 0
    assert L.tlab_gate_levels(A_, a.size, 128, T_, G_) == EINVAL
    assert L.tlab_gate_levels(A_, a.size, 3, None, G_) == EINVAL
    assert L.tlab_gate_levels(A_, a.size, 1, None, G_) == 0                                       # one level needs no threshold
    assert L.tlab_gate_levels(A_, 0, 3, T_, G_) == EINVAL and L.tlab_gate_levels(None, a.size, 3, T_, G_) == EINVAL
    assert L.tlab_gate_flux(A_, None, a.size, G_) == EINVAL and L.tlab_gate_flux(A_, A_, 0, G_) == EINVAL
    assert b"tlab_gate_flux" in L.tlab_last_error()
    assert L.tlab_cavg1v_n(nx, ny, nz, 1, 1024, I_, None, None, one, 1, G_, A_, O_, O_, O_) == 0  # the compiled limit itself
    for nbins in (0, -3, 1025):                                                                   # bins above the limit
        assert L.tlab_cavg1v_n(nx, ny, nz, 1, nbins, I_, None, None, one, 0, None, A_, O_, None, None) == EINVAL
    assert b"CAVG_MAX_BINS" in L.tlab_last_error() and b"1024" in L.tlab_last_error()
    assert L.tlab_cavg1v_n(nx, ny, nz, 1, 8, I_, None, None, one, 1, None, A_, O_, None, None) == EINVAL      # igate != 0 with a null gate
    assert L.tlab_cavg1v_n(nx, ny, nz, 1, 8, I_, None, None, one, 0, None, None, O_, None, None) == EINVAL
    assert L.tlab_cavg1v_n(nx, ny, nz, 1, 8, I_, None, None, one, 0, None, A_, None, None, None) == EINVAL
    assert L.tlab_cavg1v_n(nx, ny, nz, 1, 8, I_, None, None, null, 0, None, A_, O_, None, None) == EINVAL
    zero = np.zeros(1, dtype=np.int32)
    assert L.tlab_cavg1v_n(nx, ny, nz, 1, 8, vp(zero.ctypes.data), None, None, one, 0, None, A_, O_, None, None) == EINVAL      # ibc = 0 without its interval
    assert L.tlab_cavg2v(nx, ny, nz, (ctypes.c_int * 2)(32, 32), A_, A_, A_, O_) == 0
    for nb2 in ((0, 4), (4, 0), (33, 32), (1025, 1)):
        assert L.tlab_cavg2v(nx, ny, nz, (ctypes.c_int * 2)(*nb2), A_, A_, A_, O_) == EINVAL, nb2
    assert L.tlab_cavg2v(nx, ny, nz, (ctypes.c_int * 2)(4, 4), A_, None, A_, O_) == EINVAL
    assert L.tlab_cavg2v(nx, ny, nz, None, A_, A_, A_, O_) == EINVAL
    # FI_GATE: a gate read from a file is the host's, the potential vorticity is not built; both are said before anything else is looked at
    three = (vp * 3)(a.ctypes.data, a.ctypes.data, a.ctypes.data)
    assert L.tlab_dns_gate(None, 1, 0, 1, 2, T_, three, three, three, G_) == EINVAL
    assert L.tlab_dns_gate(None, 8, 0, 1, 2, T_, three, three, three, G_) == EUNSUPPORTED
    assert b"FI_CURL" in L.tlab_last_error()
    assert L.tlab_dns_gate(None, 9, 0, 1, 2, T_, three, three, three, G_) == EINVAL
    assert L.tlab_dns_gate(None, 2, 0, 1, 2, T_, three, three, three, G_) == EINVAL               # no driver


def test_the_compiled_limits_are_what_the_documents_say():
    src = open(os.path.join(ROOT, "tlab_amd", "csrc", "conditional_host.hpp")).read()
    assert int(re.search(r"CAVG_MAX_BINS\s*=\s*(\d+)", src).group(1)) >= 1024
    assert int(re.search(r"COND_MAX_MOMENTS\s*=\s*(\d+)", src).group(1)) == C.NMOMS_MAX


# ---- the Fortran wrappers --------------------------------------------------------------------------------------------------------------------
def test_fortran_wrappers_compile_and_link_against_a_caller(tmp_path):
    """the new wrappers of tlab_amd_averages.f90 and tlab_amd_pdfs.f90 depend on TLab_AMD_C alone, and a caller shaped like the conditional block of
    tools/statistics/averages.f90 and pdfs.f90 compiles against them and links with the library"""
    fortran = os.path.join(ROOT, "tlab_amd", "fortran")
    fc = shutil.which("amdflang")
    mod = os.path.join(ROOT, "oracle", "_ref", "mod")                   # TLab_AMD_Check of tlab_amd_c.f90 writes through the reference's TLab_WorkFlow
    if fc is None or not os.path.isdir(mod):
        pytest.skip("amdflang or the reference's module files (oracle/_ref/mod) are not here")
    run = lambda *a: subprocess.run([fc, "-cpp", "-O2", "-fPIC", "-I", mod, "-module-dir", str(tmp_path), "-c", *a], cwd=tmp_path,      # noqa: E731
                                    capture_output=True, text=True)
    r = run(os.path.join(fortran, "tlab_amd_c.f90"), "-o", str(tmp_path / "c.o"))
    assert r.returncode == 0, r.stderr
    for name in ("tlab_amd_averages", "tlab_amd_pdfs"):
        r = run("-I", str(tmp_path), os.path.join(fortran, name + ".f90"), "-o", str(tmp_path / (name + ".o")))
        assert r.returncode == 0, r.stderr
        src = open(os.path.join(fortran, name + ".f90")).read()
        serial = re.sub(r"^#ifdef USE_MPI\n.*?^#e(?:lse|ndif)\n", "", src, flags=re.M | re.S)
        assert re.findall(r"^\s*use\s+(\w+)", serial, flags=re.M | re.I) == ["TLab_AMD_C"]
        assert max(len(l) for l in src.splitlines()) <= 160
    (tmp_path / "caller.f90").write_text(
        "subroutine caller(dns, q, s, txc, a, gate, avg, cavg, cavg2, imax, jmax, kmax, inb_scal)\n"
        "    use TLab_AMD_C\n"
        "    use TLab_AMD_Averages\n"
        "    use TLab_AMD_PDFs\n"
        "    type(c_ptr) :: dns, vars(16), pq(3), ps(8), ptxc(7)\n"
        "    integer :: imax, jmax, kmax, inb_scal, nfield, is, ibc(16), nbins(2)\n"
        "    real(c_double), target :: q(imax*jmax*kmax, 3), s(imax*jmax*kmax, inb_scal), txc(imax*jmax*kmax, 7), a(imax*jmax*kmax)\n"
        "    real(c_double) :: avg(jmax, 4, 3 + inb_scal), cavg(34, jmax + 1, 3 + inb_scal), cavg2(8*8 + 2 + 2*8, jmax + 1)\n"
        "    real(c_double) :: avgs(jmax, 4, 3 + inb_scal, 3)\n"
        "    real(c_double) :: vmin(16), vmax(16), gate_threshold(3)\n"
        "    integer(1) :: gate(imax*jmax*kmax), igate\n"
        "    nfield = 0\n"
        "    do is = 1, 3\n"
        "        nfield = nfield + 1; vars(nfield) = c_loc(q(:, is)); pq(is) = c_loc(q(:, is))\n"
        "    end do\n"
        "    do is = 1, inb_scal\n"
        "        nfield = nfield + 1; vars(nfield) = c_loc(s(:, is)); ps(is) = c_loc(s(:, is))\n"
        "    end do\n"
        "    do is = 1, 7\n"
        "        ptxc(is) = c_loc(txc(:, is))\n"
        "    end do\n"
        "    gate_threshold = [0.1_c_double, 0.5_c_double, 0.0_c_double]\n"
        "    call TLab_AMD_FI_Gate(dns, 3, 1, 1, imax, jmax, kmax, 3, gate_threshold, pq, ps, ptxc, gate)\n"
        "    call TLab_AMD_AVG_N_XZ_Levels(imax, jmax, kmax, nfield, 4, vars, 3, gate, avgs)\n"
        "    igate = 0_1\n"
        "    call TLab_AMD_AVG_N_XZ(imax, jmax, kmax, nfield, 4, vars, igate, gate, avg)\n"
        "    ibc(1:nfield) = 1; igate = 0_1; nbins = 8\n"
        "    call TLab_AMD_CAVG1V_N(imax, jmax, kmax, nfield, 32, ibc, vmin, vmax, vars, igate, gate, a, cavg)\n"
        "    call TLab_AMD_CAVG2V(imax, jmax, kmax, nbins, q(:, 1), s(:, 1), a, cavg2)\n"
        "end subroutine caller\n")
    r = run("-I", str(tmp_path), str(tmp_path / "caller.f90"), "-o", str(tmp_path / "caller.o"))
    assert r.returncode == 0, r.stderr
    import tlab_amd
    r = subprocess.run([fc, "-shared", "-o", str(tmp_path / "libcaller.so"), str(tmp_path / "caller.o"), str(tmp_path / "tlab_amd_averages.o"),
                        str(tmp_path / "tlab_amd_pdfs.o"), str(tmp_path / "c.o"), "-Wl,--unresolved-symbols=ignore-all", "-L",
                        os.path.dirname(tlab_amd.lib_path()), "-ltlab_amd"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nm = subprocess.run(["nm", "-D", "--undefined-only", str(tmp_path / "libcaller.so")], capture_output=True, text=True).stdout
    for sym in ("tlab_dns_gate", "tlab_avg_n_xz", "tlab_cavg1v_n", "tlab_cavg2v"):
        assert sym in nm, sym
