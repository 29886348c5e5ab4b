"""The plane statistics on the device (csrc/averages.hip behind tlab_avg_ik_v, tlab_avg1v2d_v, tlab_avg_moments_flow, tlab_avg_moments_scal) against
the numpy restatement tests/averages_oracle.py.

Two kinds of data.  EXACT: integer fields in [-8, 8] and means that are multiples of 1/4 -- a fluctuation is at most 10 with 2 fractional bits, its
fourth power is below 2^17 with 8 fractional bits, a plane has at most 8645 terms, so every term and every partial sum in any order is exact in
fp64: the device must equal the restatement bit for bit, and a missed or doubled element at a tail or a chunk seam shows.  ROUNDING: uniform(-1, 1)
plus a y-dependent offset of order 10 with the same means handed to both sides -- the terms are the same doubles, only the order of summation
differs, so an output may differ by at most
    2 (n - 1) 2^-53 sum|term| / n + 2 2^-53 |value|,   n = nx nz
(two orders of summing the same n terms, each within (n - 1) 2^-53 sum|term| of the exact sum, and the rounding of the division on either side):
derived, not measured; the bound tests/test_gpu_transfers.py uses for the deposit.  The means are also held to half of it against math.fsum."""
import os
import re

import numpy as np
import pytest

import averages_oracle as A

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
R = int(re.search(r"AVG_ROWS_PER_GROUP\s*=\s*(\d+)", open(os.path.join(ROOT, "tlab_amd", "csrc", "averages_host.hpp")).read()).group(1))
# the last one: an odd tail behind a 128-double pass of a wave, three chunks of rows, the last of them partial
SHAPES = [(20, 12, 8), (70, 33, 9), (20, 12, 1), (130, 3, 2 * R + 1)]
U53 = 2.0 ** -53


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
    t.copy_(torch.from_numpy(a3.reshape(-1)))
    return t


def _exact_fields(shape, n, seed):
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    return [rng.integers(-8, 9, (nz, ny, nx)).astype(np.float64) for _ in range(n)]


def _rounding_fields(shape, n, seed):
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    off = 10.0 * np.cos(1.0 + np.arange(ny))[None, :, None]
    return [np.ascontiguousarray(rng.uniform(-1, 1, (nz, ny, nx)) + (1.0 + 0.1 * i) * off) for i in range(n)]


def _within_bound(got, terms, what, scale=1.0):
    """every output within scale x the bound of the docstring of the restatement's value; returns the largest fraction of the bound used"""
    worst = 0.0
    for (name, t), g in zip(terms.items(), got):
        nz, ny, nx = t.shape
        n = nx * nz
        ref = A.avg_ik_v(t)
        bound = scale * (2.0 * (n - 1) * U53 * A.plane_sums(np.abs(t)) / n + 2.0 * U53 * np.abs(ref))
        err = np.abs(g - ref)
        frac = float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())      # (a plane of zeros: bound 0, error 0)
        print("%s %s: largest error / bound = %.3f" % (what, name, frac))
        assert np.all(err <= bound), (what, name, frac)
        worst = max(worst, frac)
    return worst


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_data_equal_the_restatement_bit_for_bit(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    h = _exact_fields(shape, 9, 11)
    d = [_dev(a, offset) for a in h]
    rng = np.random.default_rng(12)
    fS, fU, fV, fW, rP = (rng.integers(-8, 9, ny) / 4.0 for _ in range(5))
    for nf in (1, 4, 9):                                                 # 9: two launches
        got = O.avg_ik_v(nx, ny, nz, d[:nf])
        for f in range(nf):
            assert np.array_equal(got[f], A.avg_ik_v(h[f])), ("MEANS", nf, f)
    for imom in (1, 2, 3, 4):
        assert np.array_equal(O.avg1v2d_v(nx, ny, nz, imom, d[0]), A.avg1v2d_v(h[0], imom)), ("POWER", imom)
    s, u, v, w, p = h[:5]
    ds, du, dv, dw, dp = d[:5]
    for hp, gp, pm in ((None, None, None), (p, dp, rP)):
        got = O.avg_moments_flow(nx, ny, nz, du, dv, dw, fU, fV, fW, gp, pm)
        ref = A.flow_terms(u, v, w, hp, fU, fV, fW, pm)
        assert got.shape == (len(ref), ny)
        for (name, t), g in zip(ref.items(), got):
            assert np.array_equal(g, A.avg_ik_v(t)), ("FLOW", name, hp is not None)
        got = O.avg_moments_scal(nx, ny, nz, ds, du, dv, dw, fS, fU, fV, fW, gp, pm)
        ref = A.scal_terms(s, u, v, w, hp, fS, fU, fV, fW, pm)
        assert got.shape == (len(ref), ny)
        for (name, t), g in zip(ref.items(), got):
            assert np.array_equal(g, A.avg_ik_v(t)), ("SCAL", name, hp is not None)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_rounding_data_within_the_summation_bound(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    h = _rounding_fields(shape, 5, 21)
    d = [_dev(a, offset) for a in h]
    s, u, v, w, p = h
    ds, du, dv, dw, dp = d
    means = O.avg_ik_v(nx, ny, nz, d)
    worst = _within_bound(means, {"mean%d" % i: a for i, a in enumerate(h)}, "MEANS")
    n = nx * nz
    for i, a in enumerate(h):                                            # against the correctly rounded sums: half the bound
        bound = 0.5 * (2.0 * (n - 1) * U53 * A.plane_sums(np.abs(a)) / n + 2.0 * U53 * np.abs(means[i]))
        err = np.abs(means[i] - A.exact_mean(a))
        assert np.all(err <= bound), ("exact mean", i, float((err / bound).max()))
        worst = max(worst, 0.5 * float((err / bound).max()))
    for imom in (1, 2, 3, 4):
        worst = max(worst, _within_bound([O.avg1v2d_v(nx, ny, nz, imom, du)], {"a**%d" % imom: A.power(u, imom)}, "POWER"))
    fS, fU, fV, fW, rP = means                                           # the same means on both sides
    for hp, gp, pm in ((None, None, None), (p, dp, rP)):
        worst = max(worst, _within_bound(O.avg_moments_flow(nx, ny, nz, du, dv, dw, fU, fV, fW, gp, pm), A.flow_terms(u, v, w, hp, fU, fV, fW, pm), "FLOW"))
        worst = max(worst, _within_bound(O.avg_moments_scal(nx, ny, nz, ds, du, dv, dw, fS, fU, fV, fW, gp, pm),
                                         A.scal_terms(s, u, v, w, hp, fS, fU, fV, fW, pm), "SCAL"))
    print("plane statistics %s offset %d: largest fraction of the summation bound %.3f" % (shape, offset, worst))


@pytest.mark.parametrize("shape", [(70, 33, 9), (130, 3, 2 * R + 1)])
def test_the_same_call_twice_gives_identical_bits(T, shape):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    h = _rounding_fields(shape, 5, 31)
    d = [_dev(a, 0) for a in h]
    m1, m2 = O.avg_ik_v(nx, ny, nz, d), O.avg_ik_v(nx, ny, nz, d)
    assert np.array_equal(m1, m2)
    f1 = O.avg_moments_flow(nx, ny, nz, d[1], d[2], d[3], m1[1], m1[2], m1[3], d[4], m1[4])
    _ = O.avg_moments_scal(nx, ny, nz, d[0], d[1], d[2], d[3], m1[0], m1[1], m1[2], m1[3])      # (another program uses the scratch in between)
    f2 = O.avg_moments_flow(nx, ny, nz, d[1], d[2], d[3], m1[1], m1[2], m1[3], d[4], m1[4])
    assert np.array_equal(f1, f2)


def test_mixed_host_and_device_arrays_are_refused(T):
    import tlab_amd.operators as O
    nx, ny, nz = 20, 12, 8
    h = _rounding_fields((nx, ny, nz), 3, 41)
    d = [_dev(a, 0) for a in h]
    z = np.zeros(ny)
    with pytest.raises(T.TlabError, match="host and device"):
        O.avg_ik_v(nx, ny, nz, [d[0], h[1]])
    with pytest.raises(T.TlabError, match="host and device"):           # ... also when the odd one out belongs to the second launch
        O.avg_ik_v(nx, ny, nz, [d[0]] * 8 + [h[1]])
    with pytest.raises(T.TlabError, match="host and device"):
        O.avg_moments_flow(nx, ny, nz, d[0], h[1], d[2], z, z, z)
    with pytest.raises(T.TlabError, match="host and device"):
        O.avg_moments_scal(nx, ny, nz, h[0], d[0], d[1], d[2], z, z, z, z)
    # all host after tlab_init: the host loop, bit for bit the restatement
    assert np.array_equal(O.avg_ik_v(nx, ny, nz, h[:1])[0], A.avg_ik_v(h[0]))


# ---- on a driver ----------------------------------------------------------------------------------------------------------------------------
KDT, KCO = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0]


def _dns():
    from tlab_amd.dns import Dns
    nx, ny, nz = 256, 64, 32
    x = np.arange(nx) / nx
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    return Dns(x, y, z, nscal=1, visc=1.0 / 500.0, schmidt=(0.7,), yuniform=False, hyper_bc1_ext=0.1)


def _dns_fields(d, seed):
    rng = np.random.default_rng(seed)
    wall = np.sin(np.pi * np.linspace(0, 1, d.ny))[None, :, None]
    return [(rng.uniform(-1, 1, (d.nz, d.ny, d.nx)) + 0.3 * (i + 1)) * wall for i in range(4)]


def _set(d, fields):
    import torch
    for t, a in zip(d.q + d.s, fields):
        t.copy_(torch.from_numpy(a.reshape(-1)))
    for t in d.hq + d.hs:
        t.zero_()
    torch.cuda.synchronize()


def _h3(d, t):
    return t[: d.n].cpu().numpy().reshape(d.nz, d.ny, d.nx)


def _all_calls(d, p):
    return d.plane_means(), d.flow_moments(), d.flow_moments(p), d.scal_moments(0), d.scal_moments(0, p), d.AVG_IK_V(d.q[1])


def test_driver_methods_against_the_restatement_and_nothing_else_changes(T):
    """Dns.plane_means, flow_moments, scal_moments: the restatement is handed the device's own means; and after all of these calls one substep
    gives the bits of a driver on which none was made"""
    import torch
    a, b = _dns(), _dns()
    f0 = _dns_fields(a, 51)
    _set(a, f0)
    _set(b, f0)
    p = torch.from_numpy(np.random.default_rng(52).uniform(-1, 1, a.n) + 3.0).cuda()
    hp = _h3(a, p)
    u, v, w, s = f0
    m, F, Fp, S, Sp, rV = _all_calls(a, p)
    n = a.nx * a.nz
    for got, field in ((m["rU"], u), (m["rV"], v), (m["rW"], w), (m["rS"][0], s), (rV, v)):
        bound = 0.5 * (2.0 * (n - 1) * U53 * A.plane_sums(np.abs(field)) / n + 2.0 * U53 * np.abs(got))
        assert np.all(np.abs(got - A.exact_mean(field)) <= bound)
    assert np.array_equal(rV, m["rV"]) and np.array_equal(F["rU"], m["rU"]) and np.array_equal(Sp["rS"], m["rS"][0])
    for res, pp in ((F, None), (Fp, hp)):
        terms = A.flow_terms(u, v, w, pp, res["rU"], res["rV"], res["rW"], res.get("rP"))
        assert set(terms) | {"rU", "rV", "rW"} | ({"rP"} if pp is not None else set()) == set(res)
        _within_bound([res[k] for k in terms], terms, "Dns.flow_moments")
    for res, pp in ((S, None), (Sp, hp)):
        terms = A.scal_terms(s, u, v, w, pp, res["rS"], res["rU"], res["rV"], res["rW"], res.get("rP"))
        assert set(terms) | {"rS", "rU", "rV", "rW"} | ({"rP"} if pp is not None else set()) == set(res)
        _within_bound([res[k] for k in terms], terms, "Dns.scal_moments")
    for d in (a, b):
        d.begin_step()
        d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(2e-3 * KDT[0], KCO[0], True)
    torch.cuda.synchronize()
    for x, y in zip(a.q + a.s + a.hq + a.hs, b.q + b.s + b.hq + b.hs):
        assert torch.equal(x, y)


def test_a_recorded_substep_completes_before_the_fields_are_read(T):
    """with the deferred tail on, tlab_avg_ik_v right behind a recorded substep equals the call made after tlab_deferred_flush on a second driver"""
    from tlab_amd.lib import load, check, c_vp
    L = load()
    f0 = None
    got = []
    for flush in (False, True):
        d = _dns()
        f0 = f0 if f0 is not None else _dns_fields(d, 61)
        _set(d, f0)
        mk = lambda ts: (c_vp * max(1, len(ts)))(*[t.data_ptr() for t in ts])      # noqa: E731
        q, s, hq, hs, txc = mk(d.q), mk(d.s), mk(d.hq), mk(d.hs), mk(d.txc)
        dte = 2e-3 * KDT[0]
        check(L.tlab_deferred_enable(1), "enable")
        try:
            check(L.tlab_deferred_rhs(d._h, dte, q, s, hq, hs, txc), "rhs")
            for h, u in zip(d.hq + d.hs, d.q + d.s):
                check(L.tlab_deferred_axpy(d.n, dte, h.data_ptr(), u.data_ptr()), "axpy")
            for h in d.hq + d.hs:
                check(L.tlab_deferred_scal(d.n, KCO[0], h.data_ptr()), "scal")
            if flush:
                check(L.tlab_deferred_flush(), "flush")
            out = np.zeros((3, d.ny))      # the entry point itself, with no other call of the library in front of it
            check(L.tlab_avg_ik_v(d.nx, d.ny, d.nz, 3, q, c_vp(out.ctypes.data), d.ny), "tlab_avg_ik_v")
            got.append(out)
        finally:
            check(L.tlab_deferred_enable(0), "disable")
    assert np.array_equal(got[0], got[1])
    before = np.stack([A.avg_ik_v(a) for a in f0[:3]])
    assert not np.array_equal(got[0], before)                            # (the substep moved the means: the call did not read the old fields)
