"""The conditional statistics on the device (csrc/conditional.hip behind tlab_gate_levels, tlab_gate_flux, tlab_dns_gate, tlab_avg_n_xz,
tlab_cavg1v_n, tlab_cavg2v) against the numpy restatement tests/conditional_oracle.py and the records of the reference's own compiled routines
(tests/golden/conditional_ref.npz), both of which tests/test_conditional_host.py holds together.

What must be equal is compared with np.array_equal: every gate byte, every count and nsample, every bin coordinate, and every sum on exactly
summable data (multiples of 1/4 in [-2, 2] for nm <= 4, integers in [-2, 2] for nm = 10: every power and every partial sum is exact, so the order
of a sum cannot show).  On rounding data a device sum differs from the reference's by its order alone, and is held to the bound of two summation
orders of n terms, |got - ref| <= 2 (n - 1) u sum|t| / n + 2 u |ref| with u = 2^-53, per (plane, level, moment) and per bin; the largest fraction of
it that is used is printed (profiles/r25/conditional.txt holds a record).  Nothing here is tuned: the bound is derived.
Fractions seen on the MI355X: raw moments at most 0.37, CAVG1V_N at most 0.50, CAVG2V at most 0.59 of the bound.

Shapes: those of tests/test_gpu_pdfs.py, for the same launch shape, with R the kernels' rows-per-group constant -- lines shorter than a wave, a
partial second pass of a wave, nz = 1, three chunks of rows with the last partial, odd nx -- each with the fields at offset 0 (16-byte loads where
nx is even) and at offset 1 double from a 16-byte boundary (8-byte loads).  Bin counts: every count at which k_cavg_sum takes another number of
columns (64 down to 1: nbins 8 | 9, 16 | 17, .., 256 | 257) or leaves the volume's table to a launch of its own (512 | 513), and the limit 1024."""
import functools
import json
import os
import re

import numpy as np
import pytest

import conditional_oracle as C
import pdfs_oracle as P

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
R = int(re.search(r"PDF_ROWS_PER_GROUP\s*=\s*(\d+)", open(os.path.join(ROOT, "tlab_amd", "csrc", "pdfs_host.hpp")).read()).group(1))
SHAPES = [(20, 12, 8), (70, 33, 9), (20, 12, 1), (130, 3, 2 * R + 1), (7, 5, 3)]
EVERY_PATH = (1, 2, 8, 9, 16, 17, 32, 33, 64, 65, 100, 128, 129, 256, 257, 512, 513, 1024)


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "conditional_ref.npz"))
    return g, json.loads(str(g["index"]))


def _dev(a3, offset=0):
    """a device copy of a field that starts `offset` doubles behind a 16-byte boundary (offset 1: the 8-byte loads)"""
    import torch
    buf = torch.empty(a3.size + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:offset + a3.size]
    t.copy_(torch.from_numpy(np.array(a3, dtype=np.float64).reshape(-1)))
    return t


def _dev_gate(g, offset=0):
    """... of a gate, `offset` bytes behind a 16-byte boundary"""
    import torch
    buf = torch.empty(g.size + 16, dtype=torch.int8, device="cuda")
    t = buf[offset:offset + g.size]
    t.copy_(torch.from_numpy(np.array(g, dtype=np.int8).reshape(-1)))
    return t


@functools.lru_cache(maxsize=None)
def _fields(shape):
    """rounding data u, v, a: uniform(-1, 1) + cos(j), u with a constant plane; exact data q4 (multiples of 1/4 in [-2, 2]) and i2 (integers
    in [-2, 2]); read-only, shared by the tests"""
    nx, ny, nz = shape
    rng = np.random.default_rng(400 + nx)
    off = np.cos(np.arange(ny))[None, :, None]
    f = {k: np.ascontiguousarray(rng.uniform(-1, 1, (nz, ny, nx)) + off) for k in ("u", "v", "a")}
    f["u"][:, ny // 2, :] = 0.75
    f["q4"] = rng.integers(-8, 9, (nz, ny, nx)).astype(np.float64) / 4.0
    f["i2"] = rng.integers(-2, 3, (nz, ny, nx)).astype(np.float64)
    for a in f.values():
        a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _gate(shape):
    """levels 0 .. 3; plane 1 without a point of level 2 and plane 2 with one point of level 3 (where the box has them)"""
    nx, ny, nz = shape
    g = np.random.default_rng(500 + nx).integers(0, 4, (nz, ny, nx)).astype(np.int8)
    if ny > 2:
        g[:, 1, :][g[:, 1, :] == 2] = 1
        g[:, 2, :][g[:, 2, :] == 3] = 0
        g[nz // 2, 2, nx // 2] = 3
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _ref_moments(shape, names, nm, np_):
    f = _fields(shape)
    return C.avg_n_xz([f[k] for k in names], nm, np_, _gate(shape) if np_ else None)


@functools.lru_cache(maxsize=None)
def _ref_cavg(shape, names, aname, nbins, ibc, igate):
    f = _fields(shape)
    return C.cavg1v_n([f[k] for k in names], f[aname], nbins, [ibc] * len(names), [-0.5] * len(names), [0.8] * len(names), _gate(shape), igate)


# ---- the partition ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 256 * 4 + 5, 256 * 65536 + 77])
def test_gate_levels_and_quadrants_equal_the_restatement_in_every_byte(T, n):
    import torch
    import tlab_amd.operators as O
    rng = np.random.default_rng(n % 1000)
    a = rng.integers(-4, 5, n).astype(np.float64) / 2.0                  # data ON the thresholds below, on both sides of <
    v = rng.integers(-2, 3, n).astype(np.float64)                        # zeros in both: every branch of the quadrants
    big = n > 10 ** 6                                                    # more points than one pass of the grid: one form, one set of thresholds
    for off in ((0,) if big else (0, 1)):
        da, dv = _dev(a, off), _dev(v, 1 - off)
        for thr in ([[-1.0, -0.5, 0.5, 1.5]] if big else [[], [0.5], [-1.0, -0.5, 0.5, 1.5], list(np.linspace(-2.0, 2.0, 126))]):      # igate_size 1, 2, 5, 127
            out = _dev_gate(np.full(n, -7, dtype=np.int8), off)
            got = O.gate_levels(da, thr, out)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), C.gate_levels(a, thr)), (off, len(thr))
        assert np.array_equal(O.gate_flux(da, dv).cpu().numpy(), C.gate_flux(a, v)), off
    if n == 257:
        with pytest.raises(T.TlabError):
            O.gate_levels(da, [0.5], np.zeros(n, dtype=np.int8))        # a device field and a host gate
        with pytest.raises(T.TlabError):
            O.gate_flux(da, v)


def test_dns_gate_classifies_its_own_indicator(T):
    """FI_GATE for opt_cond 2 .. 7: the device's own indicator (the field, or what the call left in txc[0]) classified by the restatement must give
    the gate in every byte -- no tolerance, so that no point next to a threshold may change its level"""
    import torch
    import cases
    from launch_census import REF_HYPER, SMALL
    from tlab_amd.dns import Dns
    nx, ny, nz = SMALL
    x, y, z = cases.grids(nx, ny, nz, True)
    q0, s0 = cases.init_fields(nx, ny, nz, x, y, z, 3)
    d = Dns(x, y, z, nscal=1, visc=1.0 / 800.0, schmidt=(0.7,), yuniform=False, hyper_bc1_ext=REF_HYPER)
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(q0[i]))
    d.s[0].copy_(torch.from_numpy(s0[0]))
    before = [t.clone() for t in d.q + d.s + d.hq + d.hs]
    n = d.n
    for opt in (2, 3, 4, 5, 6):
        d.txc[0].fill_(-77.0)
        g0 = d.FI_GATE(opt, [0.25, 0.5, 0.75], relative=True).cpu().numpy()
        if opt in (2, 5):
            assert bool((d.txc[0] == -77.0).all()), "opt_cond 2 and 5 read their field in place"
            ind = (d.s[0] if opt == 2 else d.q[1])[:n].cpu().numpy()
        else:
            ind = d.txc[0][:n].cpu().numpy()
        assert np.array_equal(g0, C.gate_levels(ind, C.relative_thresholds([0.25, 0.5, 0.75], ind))), opt
        assert len(np.unique(g0)) >= 2, opt
        # absolute thresholds that ARE values of the indicator: equality at a threshold goes to the level above it
        thr = np.sort(ind[:: max(n // 5, 1)][:4])
        thr = thr[np.concatenate(([True], np.diff(thr) > 0))]
        g1 = d.FI_GATE(opt, thr).cpu().numpy()
        again = (d.s[0] if opt == 2 else d.q[1] if opt == 5 else d.txc[0])[:n].cpu().numpy()
        assert np.array_equal(again, ind) and np.array_equal(g1, C.gate_levels(ind, thr)), opt
        assert np.all(g1[ind == thr[0]] == 2)
    g7 = d.FI_GATE(7, None).cpu().numpy()
    fluct = d.txc[0][:n].cpu().numpy()
    s3 = s0[0].reshape(nz, ny, nx)
    assert np.allclose(fluct.reshape(nz, ny, nx), s3 - s3.mean(axis=(0, 2))[None, :, None], rtol=0, atol=1e-13)      # (the indicator has tests of its own)
    assert np.array_equal(g7, C.gate_flux(fluct, d.q[1][:n].cpu().numpy())) and set(np.unique(g7)) == {1, 2, 3, 4}
    assert all(torch.equal(a, b) for a, b in zip(before, d.q + d.s + d.hq + d.hs))
    with pytest.raises(T.TlabError, match="FI_CURL"):
        d.FI_GATE(8, [0.5])
    with pytest.raises(T.TlabError):
        d.FI_GATE(1, [0.5])
    # ... and the two statistics on the driver's own fields
    cm = d.conditional_moments(d.FI_GATE(2, [0.5], relative=True), 2)
    assert sorted(cm) == ["Scalar1", "U", "V", "W", "nsample"] and cm["U"].shape == (2, 4, ny) and np.all(cm["nsample"].sum(axis=0) == nx * nz)
    ca = d.conditional_averages(d.s[0])
    assert sorted(ca) == ["s1", "u", "v", "w"] and ca["u"].shape == (ny + 1, 34)
    own = ca["s1"]                                                           # <s | s> lies inside the bin it is taken over
    step = (own[:, 33] - own[:, 32]) / 31.0
    lo = own[:, 32:33] - 0.5 * step[:, None] + step[:, None] * np.arange(32)[None, :]
    filled = own[:, :32] != 0.0
    assert np.all((own[:, :32] >= lo - 1e-12)[filled]) and np.all((own[:, :32] <= lo + step[:, None] + 1e-12)[filled])


# ---- gated moments -------------------------------------------------------------------------------------------------------------------------
def test_moments_of_the_fixture_on_exact_data_are_the_reference_bit_for_bit(T, golden):
    import tlab_amd.operators as O
    g, index = golden
    seen = 0
    for n, m in enumerate(index):
        if m["kind"] != "moments" or m["field"] == "u":
            continue
        ref, a, gate = g["out_%d" % n], g["in_%s_%s" % (m["box"], m["field"])], g["in_%s_gate" % m["box"]]
        nz, ny, nx = a.shape
        nm = 4 if m["field"] == "q4" else 10
        for np_, rows in ((0, ref[:1]), (3, ref[1:])):
            avg, sums, ns = O.avg_n_xz(nx, ny, nz, [_dev(a)], nm, np_, _dev_gate(gate) if np_ else None, raw=True)
            raw = np.divide(sums, ns[:, None, None, :], out=sums.copy(), where=ns[:, None, None, :] > 0)
            assert np.array_equal(raw[:, 0], rows[:, :nm]), (m, np_)
            assert np.array_equal(avg, C.central_of(sums, ns))
        seen += 1
    assert seen == 6


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_moments_exact_data_bit_for_bit_rounding_data_within_the_bound(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    f = _fields(shape)
    dg = _dev_gate(_gate(shape), offset)
    worst = 0.0
    for names, nm in ((("q4",), 2), (("q4", "q4"), 4), (("i2",), 10)):
        d = [_dev(f[k], offset) for k in names]
        for np_ in (0, 3):
            want = _ref_moments(shape, names, nm, np_)
            got = O.avg_n_xz(nx, ny, nz, d, nm, np_, dg if np_ else None, raw=True)
            for a, b, what in zip(got, want, ("avg", "sums", "nsample")):
                assert a.dtype == b.dtype and np.array_equal(a, b), (names, nm, np_, what)
    for names, nm in ((("u", "v"), 4), (("a",), 10)):
        d = [_dev(f[k], offset) for k in names]
        for np_ in (0, 3):
            avg_r, sums_r, ns_r = _ref_moments(shape, names, nm, np_)
            avg, sums, ns = O.avg_n_xz(nx, ny, nz, d, nm, np_, dg if np_ else None, raw=True)
            assert np.array_equal(ns, ns_r)
            assert np.array_equal(avg, C.central_of(sums, ns)), "avg is tlab_raw_to_central of its own sums / nsample"
            again = O.avg_n_xz(nx, ny, nz, d, nm, np_, dg if np_ else None, raw=True)
            assert all(np.array_equal(a, b) for a, b in zip(again, (avg, sums, ns))), "the same call twice"
            assert np.array_equal(O.avg_n_xz(nx, ny, nz, d, nm, np_, dg if np_ else None), avg)
            for v, k in enumerate(names):
                for m in range(1, nm + 1):
                    absum = np.zeros_like(ns, dtype=np.float64)
                    for l in range(max(np_, 1)):
                        for j in range(ny):
                            mask = None if np_ == 0 else (_gate(shape)[:, j, :] == l + 1)
                            absum[l, j] = C.raw_moment(np.abs(f[k][:, j, :]), m, mask)[0]
                    nn = np.maximum(ns, 1)
                    worst = max(worst, C.within_bound(sums[:, v, m - 1] / nn, sums_r[:, v, m - 1] / nn, absum, ns, "raw moment %s**%d np=%d" % (k, m, np_)))
    print("%s offset %d: raw moments use at most %.3f of the bound" % (shape, offset, worst))


def test_moments_of_many_levels_and_many_fields(T):
    """127 levels take 32 launches over groups of levels, nine fields two groups of fields: every group lands in its own place"""
    import tlab_amd.operators as O
    shape = (20, 12, 8)
    nx, ny, nz = shape
    f = _fields(shape)
    gate = np.random.default_rng(9).integers(-1, 128, (nz, ny, nx)).astype(np.int8)      # -1 and 0 belong to no level
    got = O.avg_n_xz(nx, ny, nz, [_dev(f["q4"])], 4, 127, _dev_gate(gate), raw=True)
    want = C.avg_n_xz([f["q4"]], 4, 127, gate)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert got[2].sum() == np.count_nonzero(gate >= 1)
    names = ["q4", "i2"] * 4 + ["q4"]
    got = O.avg_n_xz(nx, ny, nz, [_dev(f[k]) for k in names], 2, 3, _dev_gate(_gate(shape)), raw=True)
    want = C.avg_n_xz([f[k] for k in names], 2, 3, _gate(shape))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- conditional averages ----------------------------------------------------------------------------------------------------------------------
def test_conditional_averages_of_the_fixture_on_exact_data_are_the_reference_bit_for_bit(T, golden):
    import tlab_amd.operators as O
    g, index = golden
    seen = 0
    for n, m in enumerate(index):
        exact = m.get("a") in ("q4", "i2")
        if m["kind"] == "cavg1v":
            ref, nb = g["out_%d" % n], m["nbins"]
            if m["field"] == "c":
                u = g["in_%s_u" % m["box"]].copy()
                u[:, u.shape[1] // 2, :] = 0.75
            else:
                u = g["in_%s_%s" % (m["box"], m["field"])]
            a = g["in_%s_%s" % (m["box"], m["a"])]
            nz, ny, nx = u.shape
            avg, s, pdf = O.cavg1v_n(nx, ny, nz, [_dev(u)], _dev(a), nb, m["ilim"], m["umin"], m["umax"],
                                     _dev_gate(g["in_%s_gate" % m["box"]]) if m["igate"] else None, m["igate"], raw=True)
            assert np.array_equal(pdf[0], ref[:, :, 0]) and np.array_equal(avg[0, :, nb:], ref[:, nb:, 0]), m      # counts and coordinates: always
            if exact:
                assert np.array_equal(avg[0, :, :nb], ref[:, :nb, 1]), m
                seen += 1
        elif m["kind"] == "cavg2v" and exact:
            ref = g["out_%d" % n]
            u, v, a = (g["in_%s_%s" % (m["box"], k)] for k in ("u", "v", m["a"]))
            nz, ny, nx = u.shape
            nb = m["nbins"][0] * m["nbins"][1]
            got = O.cavg2v(nx, ny, nz, m["nbins"], _dev(u), _dev(v), _dev(a))
            assert np.array_equal(got[:, :nb], ref[:, :nb, 1]) and np.array_equal(got[:, nb:], ref[:, nb:, 0]), m
            seen += 1
    assert seen >= 3 * 6 + 3


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_conditional_averages_exact_data_bit_for_bit_rounding_data_within_the_bound(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    f = _fields(shape)
    names = ("u", "v", "q4")
    d = [_dev(f[k], offset) for k in names]
    dg = _dev_gate(_gate(shape), offset)
    worst = 0.0
    for aname in ("q4", "a"):
        da = _dev(f[aname], offset)
        for nbins, ibc, igate in [(nb, ibc, 0) for nb in (1, 2, 32, 100) for ibc in (0, 1)] + [(32, 0, 2), (32, 1, 2), (32, 1, 3)]:
            avg_r, s_r, pdf_r, sa_r = _ref_cavg(shape, names, aname, nbins, ibc, igate)
            avg, s, pdf = O.cavg1v_n(nx, ny, nz, d, da, nbins, ibc, -0.5, 0.8, dg if igate else None, igate, raw=True)
            assert np.array_equal(pdf, pdf_r), (aname, nbins, ibc, igate)                                  # counts and coordinates
            assert np.array_equal(avg[:, :, nbins:], avg_r[:, :, nbins:]) and np.array_equal(s[:, :, nbins:], s_r[:, :, nbins:])
            assert np.array_equal(avg[:, :, :nbins], C.divide(s[:, :, :nbins], pdf[:, :, :nbins])), "one division per bin"
            if aname == "q4":
                assert np.array_equal(s, s_r) and np.array_equal(avg, avg_r), (nbins, ibc, igate)
            else:
                worst = max(worst, C.within_bound(avg[:, :, :nbins], avg_r[:, :, :nbins], sa_r[:, :, :nbins], pdf_r[:, :, :nbins],
                                                  "<a|.> nbins=%d ibc=%d igate=%d" % (nbins, ibc, igate)))
                again = O.cavg1v_n(nx, ny, nz, d, da, nbins, ibc, -0.5, 0.8, dg if igate else None, igate, raw=True)
                assert all(np.array_equal(x, y) for x, y in zip(again, (avg, s, pdf))), "the same call twice"
    if ny > 2:
        avg, s, pdf = O.cavg1v_n(nx, ny, nz, d[:1], d[1], 32, 1, None, None, dg, 2, raw=True)
        assert pdf[0, 1, :32].sum() == 0 and np.all(avg[0, 1, :32] == 0.0) and pdf[0, 1, 32] == 1e20 + 0.5 * (-2e20 / 32)      # the empty plane
        avg, s, pdf = O.cavg1v_n(nx, ny, nz, d[:1], d[1], 32, 1, None, None, dg, 3, raw=True)
        assert pdf[0, 2, 0] == 1 and avg[0, 2, 0] == f["v"][nz // 2, 2, nx // 2]                             # one point: a zero step, bin 1
    print("%s offset %d: conditional averages use at most %.3f of the bound" % (shape, offset, worst))


def test_every_number_of_columns_and_the_split_of_the_tables(T, shape=(130, 3, 2 * R + 1)):
    """on the box with three chunks of rows: every nbins at which k_cavg_sum takes another COLS (64 .. 1), hands the volume's table to a second launch (above 512), and the limit"""
    import tlab_amd.operators as O
    nx, ny, nz = shape
    f = _fields(shape)
    d, dq, da = [_dev(f["v"])], _dev(f["q4"]), _dev(f["a"])
    worst = 0.0
    for nbins in EVERY_PATH:
        avg_r, s_r, pdf_r, sa_r = _ref_cavg(shape, ("v",), "q4", nbins, 1, 0)
        avg, s, pdf = O.cavg1v_n(nx, ny, nz, d, dq, nbins, 1, raw=True)
        assert np.array_equal(pdf, pdf_r) and np.array_equal(s, s_r) and np.array_equal(avg, avg_r), nbins
        assert np.all(pdf[0, :ny, :nbins].sum(axis=1) == nx * nz) and pdf[0, ny, :nbins].sum() == nx * ny * nz, nbins
        avg_r, s_r, pdf_r, sa_r = _ref_cavg(shape, ("v",), "a", nbins, 1, 0)
        avg = O.cavg1v_n(nx, ny, nz, d, da, nbins, 1)
        worst = max(worst, C.within_bound(avg[:, :, :nbins], avg_r[:, :, :nbins], sa_r[:, :, :nbins], pdf_r[:, :, :nbins], "<a|v> nbins=%d" % nbins))
    print("%s: every path uses at most %.3f of the bound" % (shape, worst))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_cavg2v(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    f = _fields(shape)
    du, dv = _dev(f["a"], offset), _dev(f["v"], offset)      # (a as the first variable: no constant plane)
    worst = 0.0
    for nb2 in ((8, 8), (32, 5), (1, 3), (32, 32), (256, 4)):
        nb = nb2[0] * nb2[1]
        counts = P.pdf2v(f["a"], f["v"], nb2)
        avg_r, sa_r = C.cavg2v(f["a"], f["v"], f["q4"], nb2)
        got = O.cavg2v(nx, ny, nz, nb2, du, dv, _dev(f["q4"], offset))
        assert np.array_equal(got, avg_r), nb2                                                         # exact data, and the 2 + 2 nb1 coordinates
        avg_r, sa_r = C.cavg2v(f["a"], f["v"], f["u"], nb2)
        got = O.cavg2v(nx, ny, nz, nb2, du, dv, _dev(f["u"], offset))
        assert np.array_equal(got[:, nb:], avg_r[:, nb:]) and np.array_equal(got[:, nb:], counts[:, nb:]), nb2
        assert np.array_equal(got[:, :nb] != 0.0, (avg_r[:, :nb] != 0.0))
        worst = max(worst, C.within_bound(got[:, :nb], avg_r[:, :nb], sa_r, counts[:, :nb], "<a|u,v> %s" % (nb2,)))
        assert np.array_equal(O.cavg2v(nx, ny, nz, nb2, du, dv, _dev(f["u"], offset)), got), "the same call twice"
    print("%s offset %d: CAVG2V uses at most %.3f of the bound" % (shape, offset, worst))


def test_a_mix_of_host_and_device_arrays_is_refused(T):
    import tlab_amd.operators as O
    shape = (20, 12, 8)
    nx, ny, nz = shape
    f = _fields(shape)
    du, g = _dev(f["u"]), np.array(_gate(shape))
    with pytest.raises(T.TlabError, match="host and device"):
        O.avg_n_xz(nx, ny, nz, [du, np.array(f["v"])], 2)
    with pytest.raises(T.TlabError, match="host and device"):
        O.avg_n_xz(nx, ny, nz, [du], 2, 3, g)
    with pytest.raises(T.TlabError, match="host and device"):
        O.cavg1v_n(nx, ny, nz, [du], np.array(f["a"]), 8)
    with pytest.raises(T.TlabError, match="host and device"):
        O.cavg1v_n(nx, ny, nz, [du], du, 8, 1, None, None, g, 1)
    with pytest.raises(T.TlabError, match="host and device"):
        O.cavg2v(nx, ny, nz, (4, 4), du, du, np.array(f["a"]))
    # host arrays after tlab_init take the host loops: the reference's bits
    want = C.avg_n_xz([f["u"]], 4, 3, _gate(shape))
    got = O.avg_n_xz(nx, ny, nz, [np.array(f["u"])], 4, 3, g, raw=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- a pending record of the deferred tail runs first ----------------------------------------------------------------------------------------
def _entry(name):
    def deco(fn):
        fn.entry = name
        fn.opts = dict(pre=None, post=None, before=None, zeros=True, marker=False, relax=False, liquid=False, reset=None, probe=None)
        return fn
    return deco


def _pending_cases():
    """one raw ctypes call per new stream entry point, as tests/test_gpu_deferred_entry_points.py shapes its cases: it reads state the pending
    substep changes (q[0], q[1], s[0]) and names what it wrote"""
    import ctypes
    import torch
    from test_gpu_deferred_entry_points import NX, NY, NZ, N, P as A, PA, host, ok
    thr = np.array([-0.1, 0.0, 0.1])
    nb2 = (ctypes.c_int * 2)(8, 4)
    one = np.ones(1, dtype=np.int32)

    @_entry("tlab_gate_levels")
    def levels(L, d, out):
        ok(L.tlab_gate_levels(A(d.q[0]), N, 4, thr.ctypes.data, A(d.gate)), "tlab_gate_levels")
        out["dev"] += [d.gate]

    @_entry("tlab_gate_flux")
    def flux(L, d, out):
        ok(L.tlab_gate_flux(A(d.s[0]), A(d.q[1]), N, A(d.gate)), "tlab_gate_flux")
        out["dev"] += [d.gate]

    @_entry("tlab_dns_gate")
    def dns_gate(L, d, out):
        ok(L.tlab_dns_gate(d._h, 6, 1, 1, 4, thr.ctypes.data, PA(d.q), PA(d.s), PA(d.W[:7]), A(d.gate)), "tlab_dns_gate")
        out["dev"] += [d.gate, d.W[0][:N]]

    @_entry("tlab_avg_n_xz")
    def moments(L, d, out):
        avg, ns = host(out, NY * 4 * 2 * 2), np.zeros(NY * 2, dtype=np.int64)
        out["host"].append(ns)
        ok(L.tlab_avg_n_xz(NX, NY, NZ, 2, 4, PA([d.q[0], d.s[0]]), 2, A(d.fixed_gate), avg.ctypes.data, None, ns.ctypes.data), "tlab_avg_n_xz")

    @_entry("tlab_cavg1v_n")
    def cavg1(L, d, out):
        avg = host(out, 34 * (NY + 1))
        ok(L.tlab_cavg1v_n(NX, NY, NZ, 1, 32, one.ctypes.data, None, None, PA([d.q[0]]), 0, None, A(d.s[0]), avg.ctypes.data, None, None), "tlab_cavg1v_n")

    @_entry("tlab_cavg2v")
    def cavg2(L, d, out):
        avg = host(out, (32 + 2 + 16) * (NY + 1))
        ok(L.tlab_cavg2v(NX, NY, NZ, nb2, A(d.q[0]), A(d.q[1]), A(d.s[0]), avg.ctypes.data), "tlab_cavg2v")

    return [levels, flux, dns_gate, moments, cavg1, cavg2]


def test_a_pending_record_runs_first(T):
    """every new stream entry point called through raw ctypes while the last substep of a step is only recorded: the record runs first, whole, as
    one fused substep -- what the call wrote and the fields equal, to the bit, the run with tlab_deferred_flush() in front, and differ from a call
    that ran ahead of the substep (the runs of tests/test_gpu_deferred_entry_points.py; tests/conditional_entry_points.py names this test)"""
    import torch
    from conditional_entry_points import ENTRY_POINTS, PENDING_TEST
    from deferred_entry_points import STREAM
    from test_gpu_deferred import _dns, _fields as _state
    from test_gpu_deferred_entry_points import Run, _same
    from tlab_amd.lib import load
    L = load()
    d = _dns(1)
    d.f0 = _state(d, 21)
    d.W = [torch.zeros(d.isize_txc_field, dtype=torch.float64, device="cuda") for _ in range(8)]
    d.liq = torch.zeros(d.n, dtype=torch.float64, device="cuda")
    d.gate = torch.zeros(d.n, dtype=torch.int8, device="cuda")
    d.fixed_gate = (torch.arange(d.n, device="cuda") % 3).to(torch.int8)
    whole = [1, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    try:
        cases = _pending_cases()
        assert PENDING_TEST == "test_a_pending_record_runs_first"
        assert sorted(fn.entry for fn in cases) == sorted(n for n, c in ENTRY_POINTS.items() if c == STREAM)
        for fn in cases:
            run = Run(L, d, fn)
            wrote_on, fields_on, counters_on = run.layer_on(False)
            wrote_fl, fields_fl, counters_fl = run.layer_on(True)
            right, ahead = run.layer_off(["sequence", "call"]), run.layer_off(["call", "sequence"])
            assert not _same(right[0], ahead[0]), (fn.entry, "the case cannot see a call that ran ahead of the record")
            assert counters_fl == whole and counters_on == whole, (fn.entry, counters_on, counters_fl)
            assert _same(wrote_on, wrote_fl), (fn.entry, "the call did not see the recorded substep executed")
            assert _same(fields_on, fields_fl), fn.entry
    finally:
        L.tlab_deferred_enable(0)
