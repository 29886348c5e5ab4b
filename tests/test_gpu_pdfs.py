"""The plane PDFs on the device (csrc/pdfs.hip behind tlab_pdf1v_n, tlab_pdf_minmax_planes, tlab_pdf_histogram_planes, tlab_pdf2v,
tlab_gate_threshold) against the numpy restatement tests/pdfs_oracle.py, which tests/test_pdfs_host.py holds to the reference's own module.

Every comparison is np.array_equal on the whole output, bounds included: a histogram is integer counts, exact in any order, and its interval bounds
are a handful of fp64 expressions evaluated on the host on both sides.  No tolerance exists in this feature.  (equal_nan: with nbins = 1 PDF_ANALIZE
divides by nbins - 1 = 0 and the analysed interval is NaN in the reference too; a NaN must meet a NaN, and no point is counted.)

Shapes: those of tests/test_gpu_averages.py with R the kernels' own rows-per-group constant -- an odd tail behind a full pass of a wave, three chunks
of rows with the last partial, nz = 1, lines shorter than a wave -- and one box with odd nx; each with the fields at offset 0 (16-byte loads where nx
is even) and at offset 1 double from a 16-byte boundary (8-byte loads).  The inputs hold neither -0.0 nor NaN."""
import functools
import os
import re

import numpy as np
import pytest

import pdfs_oracle as P

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
R = int(re.search(r"PDF_ROWS_PER_GROUP\s*=\s*(\d+)", open(os.path.join(ROOT, "tlab_amd", "csrc", "pdfs_host.hpp")).read()).group(1))
SHAPES = [(20, 12, 8), (70, 33, 9), (20, 12, 1), (130, 3, 2 * R + 1), (7, 5, 3)]
NBINS = (1, 2, 32, 100)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def _dev(a3, offset):
    """a device copy of a field that starts `offset` doubles behind a 16-byte boundary (offset 1: the 8-byte loads)"""
    import torch
    buf = torch.empty(a3.size + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:offset + a3.size]
    t.copy_(torch.from_numpy(np.array(a3, dtype=np.float64).reshape(-1)))      # (a copy: the shared fields are read-only)
    return t


def _dev_gate(g):
    import torch
    return torch.from_numpy(np.array(g, dtype=np.int8).reshape(-1)).cuda()


@functools.lru_cache(maxsize=None)
def _fields(shape):
    """uniform(-1, 1) + cos(j); the third field with a constant plane; read-only, shared by the tests"""
    nx, ny, nz = shape
    rng = np.random.default_rng(100 + nx)
    off = np.cos(np.arange(ny))[None, :, None]
    f = [np.ascontiguousarray(rng.uniform(-1, 1, (nz, ny, nx)) + off) for _ in range(3)]
    f[2][:, ny // 2, :] = 0.75
    for a in f:
        a.setflags(write=False)
    return tuple(f)


@functools.lru_cache(maxsize=None)
def _gate(shape):
    """about half of the points; plane 1 empty and plane 2 with one point (where the box has them)"""
    nx, ny, nz = shape
    g = (np.random.default_rng(200 + nx).uniform(size=(nz, ny, nx)) > 0.5).astype(np.int8)
    if ny > 2:
        g[:, 1:3, :] = 0
        g[nz // 2, 2, nx // 2] = 1
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _ref(shape, nbins, ibc, gated):
    f = _fields(shape)
    return P.pdf1v_n(f, nbins, [ibc] * 3, [-0.5] * 3, [0.8] * 3, _gate(shape) if gated else None, 1 if gated else 0)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_ibc_and_bin_count(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    d = [_dev(a, offset) for a in _fields(shape)]
    for nbins in NBINS:
        for ibc in range(6):
            got = O.pdf1v_n(nx, ny, nz, d, nbins, ibc, -0.5, 0.8)
            assert got.shape == (3, ny + 1, nbins + 2)
            assert same(got, _ref(shape, nbins, ibc, False)), (nbins, ibc)
    # the fields of one call may differ in ibc, and nine fields go in two groups of launches
    ibcs = [0, 1, 2, 3, 4, 5, 2, 0, 1]
    got = O.pdf1v_n(nx, ny, nz, [d[i % 3] for i in range(9)], 32, ibcs, -0.5, 0.8)
    for i, ibc in enumerate(ibcs):
        assert same(got[i], _ref(shape, 32, ibc, False)[i % 3]), (i, ibc)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_gated_with_an_empty_and_a_one_point_plane(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    d = [_dev(a, offset) for a in _fields(shape)]
    g = _gate(shape)
    dg = _dev_gate(g)
    for ibc in range(6):
        got = O.pdf1v_n(nx, ny, nz, d, 32, ibc, -0.5, 0.8, dg, 1)
        assert same(got, _ref(shape, 32, ibc, True)), ibc
    got = O.pdf1v_n(nx, ny, nz, d, 32, 1, None, None, dg, 1)
    if ny > 2:
        assert got[0, 1, :32].sum() == 0 and got[0, 1, 32] == 1e20 + 0.5 * (-2e20 / 32)      # the empty plane: big_wp through the same expressions
        assert got[0, 2, :32].sum() == 1 and got[0, 2, 0] == 1                                # one point: a zero step, everything in bin 1
    # conservation with a gate: the counts are the gated points of the plane, of the volume
    for v in range(3):
        assert np.array_equal(got[v, :ny, :32].sum(axis=1), (g == 1).sum(axis=(0, 2)))
        if ny > 1:
            assert got[v, ny, :32].sum() == (g == 1).sum()
    got0 = O.pdf1v_n(nx, ny, nz, d, 32, 1, None, None, _dev_gate(1 - g), 0)                   # igate = 0: the gate is not read
    assert same(got0, _ref(shape, 32, 1, False))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_conservation_with_a_local_interval(T, shape, offset):
    """each plane's counts sum to nx*nz and the volume's to nx*ny*nz: a lost or doubled element at a tail or a seam shows on its own"""
    import tlab_amd.operators as O
    nx, ny, nz = shape
    d = [_dev(a, offset) for a in _fields(shape)]
    for nbins in NBINS:
        got = O.pdf1v_n(nx, ny, nz, d, nbins, 1)
        assert np.all(got[:, :ny, :nbins].sum(axis=2) == nx * nz), nbins
        assert np.all(got[:, ny, :nbins].sum(axis=1) == (nx * ny * nz if ny > 1 else 0)), nbins


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_bin_edges_umax_umin_and_the_quotients_between_minus_one_and_zero(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    rng = np.random.default_rng(300 + nx)
    # integers in [-8, 8] on the external interval [-8, 8] with 16 bins: every quotient is an exact integer -- points on bin edges, at umin, at umax
    w = rng.integers(-8, 9, (nz, ny, nx)).astype(np.float64)
    got = O.pdf1v_n(nx, ny, nz, [_dev(w, offset)], 16, 0, -8.0, 8.0)
    assert same(got, P.pdf1v_n([w], 16, [0], [-8.0], [8.0]))
    pl = got[0, :ny, :16]
    assert np.array_equal(pl, np.stack([(w == k).sum(axis=(0, 2)) for k in range(-8, 8)], axis=1))      # 8 = umax is dropped
    for ibc in (1, 2):
        assert same(O.pdf1v_n(nx, ny, nz, [_dev(w, offset)], 16, ibc), P.pdf1v_n([w], 16, [ibc]))
    # dyadic values in [0, 1) on [0.25, 0.75] with 8 bins of 1/16: q in (-1, 0) for [0.1875, 0.25) is counted in bin 1
    e = rng.integers(0, 256, (nz, ny, nx)).astype(np.float64) / 256.0
    e.reshape(-1)[:4] = [0.25, 0.75, 0.25 - 1.0 / 256, 0.1875]
    got = O.pdf1v_n(nx, ny, nz, [_dev(e, offset)], 8, 0, 0.25, 0.75)
    assert same(got, P.pdf1v_n([e], 8, [0], [0.25], [0.75]))
    assert np.array_equal(got[0, :ny, 0], ((e > 0.1875) & (e < 0.3125)).sum(axis=(0, 2)))
    assert np.array_equal(got[0, :ny, :8].sum(axis=1), ((e > 0.1875) & (e < 0.75)).sum(axis=(0, 2)))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_constant_planes_and_a_constant_field(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    c = _fields(shape)[2]
    k = np.full((nz, ny, nx), 0.75)
    d = [_dev(c, offset), _dev(k, offset)]
    for ibc in (0, 1, 2, 5):
        got = O.pdf1v_n(nx, ny, nz, d, 32, ibc, 0.75, 0.75)                  # (ibc 0: a degenerate external interval)
        assert same(got, P.pdf1v_n([c, k], 32, [ibc] * 2, [0.75] * 2, [0.75] * 2)), ibc
    got = O.pdf1v_n(nx, ny, nz, d, 32, 1)
    assert got[0, ny // 2, 0] == nx * nz and got[0, ny // 2, 32] == 0.75 and got[0, ny // 2, 33] == 0.75
    assert np.all(got[1, :ny, 0] == nx * nz)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_two_passes_on_their_own_equal_the_composed_call(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    f = _fields(shape)
    d = [_dev(a, offset) for a in f]
    g = _gate(shape)
    for dg, ig, m in ((None, 0, None), (_dev_gate(g), 1, g == 1)):
        lo, hi = O.pdf_minmax_planes(nx, ny, nz, d, dg, ig)
        for v in range(3):
            for j in range(ny):
                assert (lo[v, j], hi[v, j]) == P.minmax(f[v][:, j, :], None if m is None else m[:, j, :]), (v, j)
            assert (lo[v, ny], hi[v, ny]) == P.minmax(f[v], m), v
        got = O.pdf_histogram_planes(nx, ny, nz, d, 32, 1, lo, hi, dg, ig)
        assert same(got, _ref(shape, 32, 1, ig == 1))
        alo, ahi = lo.copy(), hi.copy()
        for v in range(3):
            for j in range(ny + 1 if ny > 1 else 1):
                alo[v, j], ahi[v, j], _ = O.pdf_analize(0, 32, got[v, j])
        assert same(O.pdf_histogram_planes(nx, ny, nz, d, 32, 0, alo, ahi, dg, ig), _ref(shape, 32, 2, ig == 1))


@pytest.mark.parametrize("nbins", [128, 256, 1024, 4096])
@pytest.mark.parametrize("shape", [(70, 33, 9), (130, 3, 2 * R + 1)])
def test_bin_counts_at_which_the_number_of_replicas_changes(T, shape, nbins):
    """32 replicas of the tables up to 128 bins, 16 at 256, 4 at 1024, 1 at the compiled limit"""
    import tlab_amd.operators as O
    nx, ny, nz = shape
    f = _fields(shape)[:2]
    for offset in (0, 1):
        d = [_dev(a, offset) for a in f]
        for ibc in (0, 2):
            assert same(O.pdf1v_n(nx, ny, nz, d, nbins, ibc, -0.5, 0.8), P.pdf1v_n(f, nbins, [ibc] * 2, [-0.5] * 2, [0.8] * 2)), (offset, ibc)


@functools.lru_cache(maxsize=None)
def _joint_fields(shape):
    u, _, c = _fields(shape)
    v = np.ascontiguousarray(0.5 * u + np.random.default_rng(400 + shape[0]).uniform(-1, 1, u.shape))
    v.setflags(write=False)
    return u, v, c


@functools.lru_cache(maxsize=None)
def _ref2(shape, nb, pair):
    u, v, c = _joint_fields(shape)
    return P.pdf2v(*((u, v), (c, v), (u, c))[pair], nb)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_joint_pdf(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    u, v, c = _joint_fields(shape)
    du, dv, dc = _dev(u, offset), _dev(v, offset), _dev(c, offset)
    for nb in ((8, 8), (32, 5), (1, 3), (64, 64), (1024, 4)):                                # the last two: the compiled limits
        got = O.pdf2v(nx, ny, nz, nb, du, dv)
        assert got.shape == (ny + 1, nb[0] * nb[1] + 2 + 2 * nb[0])
        assert same(got, _ref2(shape, nb, 0)), nb
        assert np.all(got[:ny, :nb[0] * nb[1]].sum(axis=1) == nx * nz)
    assert same(O.pdf2v(nx, ny, nz, (8, 8), dc, dv), _ref2(shape, (8, 8), 1))                # a constant plane of u: one u-bin
    assert same(O.pdf2v(nx, ny, nz, (8, 8), du, dc), _ref2(shape, (8, 8), 2))                # ... of v: zero v-steps


def test_gate_threshold_against_numpy(T):
    import torch
    import tlab_amd.operators as O
    a = np.random.default_rng(5).uniform(-1, 1, 100003)
    a[:3] = 0.25                                                                              # equal to the threshold: not above it
    for offset in (0, 1):
        g = O.gate_threshold(_dev(a, offset), 0.25)
        assert g.dtype == torch.int8 and np.array_equal(g.cpu().numpy(), P.gate_threshold(a, 0.25))
    assert np.array_equal(O.gate_threshold(a, 0.25), P.gate_threshold(a, 0.25))              # a host array after tlab_init: the host loop


def test_the_same_call_twice_gives_identical_bits_and_mixed_arrays_are_refused(T):
    import tlab_amd.operators as O
    shape = (70, 33, 9)
    nx, ny, nz = shape
    f = _fields(shape)
    d = [_dev(a, 0) for a in f]
    g = _gate(shape)
    a1 = O.pdf1v_n(nx, ny, nz, d, 32, 2)
    _ = O.pdf2v(nx, ny, nz, (8, 8), d[0], d[1])                                               # (another call uses the scratch in between)
    assert np.array_equal(a1, O.pdf1v_n(nx, ny, nz, d, 32, 2))
    with pytest.raises(T.TlabError, match="host and device"):
        O.pdf1v_n(nx, ny, nz, [d[0], f[1]], 32, 2)
    with pytest.raises(T.TlabError, match="host and device"):
        O.pdf1v_n(nx, ny, nz, d, 32, 2, None, None, g, 1)                                     # device fields, host gate
    with pytest.raises(T.TlabError, match="host and device"):
        O.pdf_minmax_planes(nx, ny, nz, [f[0], d[1]])
    with pytest.raises(T.TlabError, match="host and device"):
        O.pdf2v(nx, ny, nz, (8, 8), d[0], f[1])
    with pytest.raises(T.TlabError, match="host and device"):
        O.gate_threshold(d[0], 0.0, np.zeros(d[0].numel(), dtype=np.int8))
    assert same(O.pdf1v_n(nx, ny, nz, f, 32, 2, None, None, g, 1), _ref(shape, 32, 2, True))  # all host after tlab_init: the host loop


# ---- on a driver ----------------------------------------------------------------------------------------------------------------------------
KDT, KCO = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0]


def _dns():
    from tlab_amd.dns import Dns
    nx, ny, nz = 256, 64, 32
    x = np.arange(nx) / nx
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    return Dns(x, y, z, nscal=1, visc=1.0 / 500.0, schmidt=(0.7,), yuniform=False, hyper_bc1_ext=0.1)


def _set(d, fields):
    import torch
    for t, a in zip(d.q + d.s, fields):
        t.copy_(torch.from_numpy(a.reshape(-1)))
    for t in d.hq + d.hs:
        t.zero_()
    torch.cuda.synchronize()


def test_driver_method_against_the_restatement_and_nothing_else_changes(T):
    """Dns.plane_pdfs with one scalar and with p equals the restatement field by field; a substep after it gives the bits of a driver on which no
    PDF was taken"""
    import torch
    a, b = _dns(), _dns()
    rng = np.random.default_rng(51)
    wall = np.sin(np.pi * np.linspace(0, 1, a.ny))[None, :, None]
    f0 = [(rng.uniform(-1, 1, (a.nz, a.ny, a.nx)) + 0.3 * (i + 1)) * wall + 0.0 for i in range(4)]      # (the wall plane j = 0 is constant; + 0.0: no -0.0)
    _set(a, f0)
    _set(b, f0)
    hp = rng.uniform(-1, 1, (a.nz, a.ny, a.nx)) + 3.0
    p = torch.from_numpy(hp.reshape(-1)).cuda()
    u, v, w, s = f0
    res = a.plane_pdfs()
    assert list(res) == ["u", "v", "w", "s1"]
    ref = P.pdf1v_n([u, v, w, s], 32, [2] * 4)
    for i, k in enumerate(res):
        assert res[k].shape == (a.ny + 1, 34) and same(res[k], ref[i]), k
    res = a.plane_pdfs(p)
    assert list(res) == ["u", "v", "w", "p", "s1"]
    refp = P.pdf1v_n([hp], 32, [2])[0]
    for k, r in zip(res, (ref[0], ref[1], ref[2], refp, ref[3])):
        assert same(res[k], r), k
    gate = T.gate_threshold(a.q[0], 0.1)
    res = a.plane_pdfs(nbins=16, ibc=1, gate=gate, igate=1)
    refg = P.pdf1v_n([u, v, w, s], 16, [1] * 4, None, None, P.gate_threshold(u, 0.1), 1)
    for i, k in enumerate(res):
        assert same(res[k], refg[i]), k
    for d in (a, b):
        d.begin_step()
        d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(2e-3 * KDT[0], KCO[0], True)
    torch.cuda.synchronize()
    for x, y in zip(a.q + a.s + a.hq + a.hs, b.q + b.s + b.hq + b.hs):
        assert torch.equal(x, y)


def test_a_recorded_substep_completes_before_the_fields_are_read(T):
    """with the deferred tail on, tlab_pdf1v_n right behind a recorded substep equals the call made after tlab_deferred_flush on a second driver"""
    from tlab_amd.lib import load, check, c_vp
    L = load()
    rng = np.random.default_rng(61)
    f0, got = None, []
    for flush in (False, True):
        d = _dns()
        if f0 is None:
            wall = np.sin(np.pi * np.linspace(0, 1, d.ny))[None, :, None]
            f0 = [(rng.uniform(-1, 1, (d.nz, d.ny, d.nx)) + 0.3 * (i + 1)) * wall + 0.0 for i in range(4)]
        _set(d, f0)
        mk = lambda ts: (c_vp * max(1, len(ts)))(*[t.data_ptr() for t in ts])      # noqa: E731
        q, s, hq, hs, txc = mk(d.q), mk(d.s), mk(d.hq), mk(d.hs), mk(d.txc)
        dte = 2e-3 * KDT[0]
        ibc = np.full(3, 2, dtype=np.int32)
        check(L.tlab_deferred_enable(1), "enable")
        try:
            check(L.tlab_deferred_rhs(d._h, dte, q, s, hq, hs, txc), "rhs")
            for h, u in zip(d.hq + d.hs, d.q + d.s):
                check(L.tlab_deferred_axpy(d.n, dte, h.data_ptr(), u.data_ptr()), "axpy")
            for h in d.hq + d.hs:
                check(L.tlab_deferred_scal(d.n, KCO[0], h.data_ptr()), "scal")
            if flush:
                check(L.tlab_deferred_flush(), "flush")
            out = np.zeros((3, d.ny + 1, 34))      # the entry point itself, with no other call of the library in front of it
            check(L.tlab_pdf1v_n(d.nx, d.ny, d.nz, 3, 32, c_vp(ibc.ctypes.data), None, None, q, 0, None, c_vp(out.ctypes.data)), "tlab_pdf1v_n")
            got.append(out)
        finally:
            check(L.tlab_deferred_enable(0), "disable")
    assert np.array_equal(got[0], got[1])
    assert not same(got[0], P.pdf1v_n(f0[:3], 32, [2] * 3))                # (the substep moved the fields: the call did not read the old ones)
