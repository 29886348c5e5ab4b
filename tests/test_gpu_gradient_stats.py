"""The gradient statistics on the device (the programs GRAD_FLOW1-3, UGRADP, GRAD_SCAL1-2 of csrc/averages.hip behind tlab_avg_gradients_flow,
tlab_avg_ugradp, tlab_avg_gradients_scal and the two driver entry points) against the numpy restatement tests/gradient_stats_oracle.py.

Two kinds of data, as in tests/test_gpu_averages.py.  EXACT: independent integer fields in [-8, 8] stand in for the gradients, the velocities and
p, with dwdz = -dudx - dvdy, so that the dilatation is zero and every c23 and /3.0 of Phi and E** multiplies zero; every mean handed in is a
multiple of 1/4, including the vort* and Tau_* means on both sides: the restatement is handed the device's first-pass output, which is itself
exact here (the gradient fields are drawn with integer plane means, see _exact_fields) and must equal the restatement's.  A term is then a
product of at most four factors below 2^5 with 2 fractional bits each (a fourth power is below 2^17 with 8 fractional bits), a plane
has at most 8645 terms, so every term and every partial sum in any order is exact in fp64 and every column must equal the restatement bit for bit -- a missed or doubled element at a tail, a chunk seam or the 13th field pointer shows.
The exceptions are the three columns that hold t22 (Tyyy_v, Txyy_v, Tyzy_v), which carry a live c23: they are held to the rounding bound.
ROUNDING: uniform(-1, 1) plus a y-dependent offset, nonzero dilatation, the same means on both sides: the terms are the same doubles, only the
order of summation differs, so a column may differ by at most
    2 (n - 1) 2^-53 sum|term| / n + 2 2^-53 |value|,   n = nx nz
the derived bound of tests/test_gpu_averages.py."""
import os
import re

import numpy as np
import pytest

import gradient_stats_oracle as G

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
R = int(re.search(r"AVG_ROWS_PER_GROUP\s*=\s*(\d+)", open(os.path.join(ROOT, "tlab_amd", "csrc", "averages_host.hpp")).read()).group(1))
SHAPES = [(20, 12, 8), (70, 33, 9), (20, 12, 1), (130, 3, 2 * R + 1)]
U53 = 2.0 ** -53
T22 = ("Tyyy_v", "Txyy_v", "Tyzy_v")
KDT, KCO = [1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0]


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


def _balanced(rng, shape):
    """an integer field in [-8, 8] whose plane sums are n c(j) with integer c(j) in [-2, 2]: in every plane one random half of the points holds
    independent integers in [-6, 6] and the other half their negatives (n = nx nz is even for every shape here), plus c(j)"""
    nx, ny, nz = shape
    n = nx * nz
    assert n % 2 == 0
    a = np.empty((ny, n))
    for j in range(ny):
        perm = rng.permutation(n)
        vals = rng.integers(-6, 7, n // 2).astype(np.float64)
        a[j, perm[: n // 2]], a[j, perm[n // 2:]] = vals, -vals
    a += rng.integers(-2, 3, ny)[:, None]
    return np.ascontiguousarray(a.reshape(ny, nz, nx).transpose(1, 0, 2))


def _exact_fields(shape, seed):
    """nine gradients with zero dilatation, then s u v w p.  The velocities, s and p are independent integers in [-8, 8].  So are the gradients,
    except that their plane means are integers by construction (_balanced): the first pass hands its own output to the later passes as means
    (vort*, Tau_*, Fy), and only if those are dyadic are the later terms exact.  With freely drawn integers a plane mean is sum / (nx nz), which
    is not, and the columns that subtract it could be held to the rounding bound only."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    g = [_balanced(rng, shape) for _ in range(9)]
    g[8] = -g[0] - g[4]
    return g, [rng.integers(-8, 9, (nz, ny, nx)).astype(np.float64) for _ in range(5)]


def _rounding_fields(shape, seed):
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    off = 2.0 * np.cos(1.0 + np.arange(ny))[None, :, None]
    f = [np.ascontiguousarray(rng.uniform(-1, 1, (nz, ny, nx)) + (1.0 + 0.1 * i) * off) for i in range(14)]
    return f[:9], f[9:]


def _within_bound(got, terms, what, scale=1.0):
    """every profile of got (a dict) within scale x the bound of the docstring of the restatement's value; the largest fraction of the bound used"""
    worst = 0.0
    for name, t in terms.items():
        nz, ny, nx = t.shape
        n = nx * nz
        ref = G.avg_ik_v(t)
        bound = scale * (2.0 * (n - 1) * U53 * G.plane_sums(np.abs(t)) / n + 2.0 * U53 * np.abs(ref))
        err = np.abs(got[name] - ref)
        frac = float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())      # (a plane of zeros: bound 0, error 0)
        print("%s %s: largest error / bound = %.3f" % (what, name, frac))
        assert np.all(err <= bound), (what, name, frac)
        worst = max(worst, frac)
    return worst


def _flow_terms(g, u, v, w, p, first, fU, fV, fW, rP, rU_y, rV_y, rW_y):
    """all term fields of the flow call in column order; first: the six profiles of the first pass the later passes subtract"""
    t = dict(G.flow_terms1(g))
    t.update(G.flow_terms2(g, rU_y, rV_y, rW_y, first[0], first[1], first[2]))
    t.update(G.flow_terms3(g, u, v, w, p, first[3], first[4], first[5], fU, fV, fW, rP))
    return t


def _scal_terms(gs, s, u, v, w, p, Fy, fS, fU, fV, fW, rP, rS_y, fS_y):
    t = dict(G.scal_terms1(gs, rS_y))
    t.update(G.scal_terms2(gs, s, u, v, w, p, Fy, fS, fU, fV, fW, rP, fS_y))
    return t


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_data_equal_the_restatement_bit_for_bit(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    g, (s, u, v, w, p) = _exact_fields(shape, 11)
    dg = [_dev(a, offset) for a in g]
    ds, du, dv, dw, dp = (_dev(a, offset) for a in (s, u, v, w, p))
    rng = np.random.default_rng(12)
    fS, fU, fV, fW, rP, rU_y, rV_y, rW_y, rS_y, fS_y = (rng.integers(-8, 9, ny) / 4.0 for _ in range(10))
    for hp, gp, pm in ((None, None, None), (p, dp, rP)):
        got = O.avg_gradients_flow(nx, ny, nz, dg, du, dv, dw, fU, fV, fW, rU_y, rV_y, rW_y, gp, pm)
        names = O.FLOW_GRADIENTS + (O.FLOW_GRADIENTS_P if hp is not None else ())
        assert got.shape == (len(names), ny)
        assert np.all(got[:6] == np.round(got[:6]))                                  # the first pass is exact: integer plane means (_exact_fields)
        terms = _flow_terms(g, u, v, w, hp, got[:6], fU, fV, fW, pm, rU_y, rV_y, rW_y)
        assert tuple(terms) == names
        res = dict(zip(names, got))
        for name, t in terms.items():
            if name in T22:
                continue
            assert np.array_equal(res[name], G.avg_ik_v(t)), ("GRAD_FLOW", name, hp is not None)
        _within_bound(res, {k: terms[k] for k in T22}, "GRAD_FLOW exact")
        got = O.avg_gradients_scal(nx, ny, nz, dg[:3], ds, du, dv, dw, fS, fU, fV, fW, rS_y, gp, pm, fS_y if hp is not None else None)
        names = O.SCAL_GRADIENTS + (O.SCAL_GRADIENTS_P if hp is not None else ())
        assert got.shape == (len(names), ny)
        terms = _scal_terms(g[:3], s, u, v, w, hp, got[0], fS, fU, fV, fW, pm, rS_y, fS_y)
        assert tuple(terms) == names
        for (name, t), a in zip(terms.items(), got):
            assert np.array_equal(a, G.avg_ik_v(t)), ("GRAD_SCAL", name, hp is not None)
    assert np.array_equal(O.avg_ugradp(nx, ny, nz, du, dv, dw, dg[0], dg[1], dg[2]), G.avg_ik_v(G.ugradp_term(u, v, w, g[0], g[1], g[2])))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_rounding_data_within_the_summation_bound(T, shape, offset):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    g, (s, u, v, w, p) = _rounding_fields(shape, 21)
    dg = [_dev(a, offset) for a in g]
    ds, du, dv, dw, dp = (_dev(a, offset) for a in (s, u, v, w, p))
    fS, fU, fV, fW, rP = O.avg_ik_v(nx, ny, nz, [ds, du, dv, dw, dp])
    rng = np.random.default_rng(22)
    rU_y, rV_y, rW_y, rS_y, fS_y = (rng.uniform(-1, 1, ny) for _ in range(5))
    worst = 0.0
    for hp, gp, pm in ((None, None, None), (p, dp, rP)):
        got = O.avg_gradients_flow(nx, ny, nz, dg, du, dv, dw, fU, fV, fW, rU_y, rV_y, rW_y, gp, pm)
        names = O.FLOW_GRADIENTS + (O.FLOW_GRADIENTS_P if hp is not None else ())
        terms = _flow_terms(g, u, v, w, hp, got[:6], fU, fV, fW, pm, rU_y, rV_y, rW_y)      # the same means on both sides
        worst = max(worst, _within_bound(dict(zip(names, got)), terms, "GRAD_FLOW"))
        got = O.avg_gradients_scal(nx, ny, nz, dg[:3], ds, du, dv, dw, fS, fU, fV, fW, rS_y, gp, pm, fS_y if hp is not None else None)
        names = O.SCAL_GRADIENTS + (O.SCAL_GRADIENTS_P if hp is not None else ())
        terms = _scal_terms(g[:3], s, u, v, w, hp, got[0], fS, fU, fV, fW, pm, rS_y, fS_y)
        worst = max(worst, _within_bound(dict(zip(names, got)), terms, "GRAD_SCAL"))
    got = O.avg_ugradp(nx, ny, nz, du, dv, dw, dg[0], dg[1], dg[2])
    worst = max(worst, _within_bound({"ugradp": got}, {"ugradp": G.ugradp_term(u, v, w, g[0], g[1], g[2])}, "UGRADP"))
    print("gradient statistics %s offset %d: largest fraction of the summation bound %.3f" % (shape, offset, worst))


@pytest.mark.parametrize("shape", [(70, 33, 9), (130, 3, 2 * R + 1)])
def test_the_same_call_twice_gives_identical_bits(T, shape):
    import tlab_amd.operators as O
    nx, ny, nz = shape
    g, (s, u, v, w, p) = _rounding_fields(shape, 31)
    dg = [_dev(a, 0) for a in g]
    ds, du, dv, dw, dp = (_dev(a, 0) for a in (s, u, v, w, p))
    m = [np.cos(i + np.arange(ny)) for i in range(10)]
    flow = lambda: O.avg_gradients_flow(nx, ny, nz, dg, du, dv, dw, m[0], m[1], m[2], m[3], m[4], m[5], dp, m[6])      # noqa: E731
    scal = lambda: O.avg_gradients_scal(nx, ny, nz, dg[:3], ds, du, dv, dw, m[7], m[0], m[1], m[2], m[8], dp, m[6], m[9])      # noqa: E731
    f1, f2 = flow(), flow()
    assert np.array_equal(f1, f2)
    s1 = scal()                                                          # (another program uses the scratch in between)
    _ = O.avg_ugradp(nx, ny, nz, du, dv, dw, dg[0], dg[1], dg[2])
    f3, s2 = flow(), scal()
    assert np.array_equal(f1, f3) and np.array_equal(s1, s2)


def test_mixed_host_and_device_arrays_are_refused(T):
    import tlab_amd.operators as O
    shape = (20, 12, 8)
    nx, ny, nz = shape
    g, (s, u, v, w, p) = _rounding_fields(shape, 41)
    dg = [_dev(a, 0) for a in g]
    ds, du, dv, dw, dp = (_dev(a, 0) for a in (s, u, v, w, p))
    z = np.zeros(ny)
    with pytest.raises(T.TlabError, match="host and device"):
        O.avg_gradients_flow(nx, ny, nz, dg[:8] + [g[8]], du, dv, dw, z, z, z, z, z, z)
    with pytest.raises(T.TlabError, match="host and device"):           # ... also when the odd one out is the 13th field
        O.avg_gradients_flow(nx, ny, nz, dg, du, dv, dw, z, z, z, z, z, z, p, z)
    with pytest.raises(T.TlabError, match="host and device"):
        O.avg_ugradp(nx, ny, nz, du, dv, dw, dg[0], g[1], dg[2])
    with pytest.raises(T.TlabError, match="host and device"):
        O.avg_gradients_scal(nx, ny, nz, [dg[0], dg[1], g[2]], ds, du, dv, dw, z, z, z, z, z)
    with pytest.raises(T.TlabError, match="host and device"):
        O.avg_gradients_scal(nx, ny, nz, dg[:3], s, du, dv, dw, z, z, z, z, z)
    # all host after tlab_init: the host loop, bit for bit the restatement
    got = O.avg_gradients_flow(nx, ny, nz, g, u, v, w, z, z, z, z, z, z)
    ref = G.flow_averages(g, u, v, w, None, z, z, z, None, z, z, z)
    assert all(np.array_equal(a, r) for a, r in zip(got, ref.values()))


# ---- on a driver ----------------------------------------------------------------------------------------------------------------------------
def _dns():
    from tlab_amd.dns import Dns
    nx, ny, nz = 256, 64, 32
    x = np.arange(nx) / nx
    z = np.arange(nz) / nz
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    return Dns(x, y, z, nscal=1, visc=1.0 / 500.0, schmidt=(0.7,), yuniform=False, hyper_bc1_ext=0.1), (x, y, z)


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


def test_profile_derivative_against_the_oracle(T):
    """Dns.profile_derivative (rU_y .. of the statistics) against the numpy oracle's first derivative of a profile along the stretched y"""
    from oracle import tlab_oracle as O
    d, (x, y, z) = _dns()
    prof = np.stack([np.sin(3.0 * y) + y * y, np.cos(2.0 * y), np.exp(-y)])
    got = d.profile_derivative(prof)
    op = O.FdmPlan(y, False, False)
    for a, r in zip(prof, got):
        ref = O.opr_partial(2, O.OPR_P1, 1, d.ny, 1, 0, op, a.copy())[0].reshape(-1)
        assert np.abs(r - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(d.profile_derivative(prof[1])[0], got[1])         # one profile alone: the same line, the same bits


def test_driver_methods_against_the_restatement_and_nothing_else_changes(T):
    """Dns.flow_gradient_stats / scal_gradient_stats: the nine txc equal nine separate OPR_Partial calls bit for bit; the statistics lie within
    the bound of the restatement fed those device gradients and the device's own means; the finished profiles equal the reference's host lines
    applied in numpy to the raw columns; and after all calls one substep gives the bits of a driver on which none was made"""
    import torch
    import tlab_amd.operators as O
    (a, _), (b, _) = _dns(), _dns()
    f0 = _dns_fields(a, 51)
    _set(a, f0)
    _set(b, f0)
    p = torch.from_numpy(np.random.default_rng(52).uniform(-1, 1, a.n) + 3.0).cuda()
    hp = _h3(a, p)
    u, v, w, s = f0
    nx, ny, nz = a.nx, a.ny, a.nz
    part = (O.OPR_Partial_X, O.OPR_Partial_Y, O.OPR_Partial_Z)

    def separate(field):
        out = []
        for k in range(3):
            res = torch.empty_like(field)
            part[k](O.OPR_P1, nx, ny, nz, 0, a.g[k], field, res)
            out.append(res[: a.n].clone())
        return out

    gp = separate(p)
    ugradp_ref = G.ugradp_term(u, v, w, *[_h3(a, t) for t in gp])
    for pp, hpp in ((None, None), (p, hp)):
        F = a.flow_gradient_stats(pp)
        nine = [t for c in range(3) for t in separate(a.q[c])]
        for i, t in enumerate(nine):
            assert torch.equal(a.txc[i][: a.n], t), ("txc", i)
        g = [_h3(a, t) for t in nine]
        first = [F[k + "_raw"] if k.startswith("Tau") else F[k] for k in G.FLOW1_NAMES]
        terms = _flow_terms(g, u, v, w, hpp, first, F["rU"], F["rV"], F["rW"], F.get("rP"), F["rU_y"], F["rV_y"], F["rW_y"])
        raw = {k: F.get(k + "_raw", F[k]) for k in terms}
        _within_bound(raw, terms, "Dns.flow_gradient_stats")
        fin = G.finish_flow(raw, a.visc, F["rU_y"], F["rV_y"], F["rW_y"])
        assert set(fin) == {"Phi", "Tau_yy", "Tau_xy", "Tau_yz", "Exx", "Eyy", "Ezz", "Exy", "Exz", "Eyz"} | ({"PIxx", "PIyy", "PIzz"} if pp is not None else set())
        for k, r in fin.items():
            assert np.array_equal(F[k], r), ("finished", k)
        assert set(F) == (set(terms) | {k + "_raw" for k in fin} | {"rU", "rV", "rW", "rU_y", "rV_y", "rW_y"}
                          | ({"rP", "ugradp"} if pp is not None else set()))
        if pp is not None:
            _within_bound({"ugradp": F["ugradp"]}, {"ugradp": ugradp_ref}, "Dns ugradp")
        S = a.scal_gradient_stats(0, pp)
        gs = separate(a.s[0])
        for i, t in enumerate(gs):
            assert torch.equal(a.txc[i][: a.n], t), ("txc of the scalar", i)
        hs = [_h3(a, t) for t in gs]
        terms = _scal_terms(hs, s, u, v, w, hpp, S["Fy"], S["rS"], S["rU"], S["rV"], S["rW"], S.get("rP"), S["rS_y"], S["rS_y"])
        raw = {k: S.get(k + "_raw", S[k]) for k in terms}
        _within_bound(raw, terms, "Dns.scal_gradient_stats")
        assert np.array_equal(S["Ess"], G.finish_scal(raw, a.visc / 0.7)["Ess"])
    for d in (a, b):
        d.begin_step()
        d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(2e-3 * KDT[0], KCO[0], True)
    torch.cuda.synchronize()
    for x, y in zip(a.q + a.s + a.hq + a.hs, b.q + b.s + b.hq + b.hs):
        assert torch.equal(x, y)


def test_a_recorded_substep_completes_before_the_fields_are_read(T):
    """with the deferred tail on, tlab_dns_avg_gradients_flow right behind a recorded substep equals the call made after tlab_deferred_flush on a
    second driver"""
    from tlab_amd.lib import load, check, c_vp
    L = load()
    f0 = None
    got = []
    for flush in (False, True):
        d, _ = _dns()
        f0 = f0 if f0 is not None else _dns_fields(d, 61)
        _set(d, f0)
        mk = lambda ts: (c_vp * max(1, len(ts)))(*[t.data_ptr() for t in ts])      # noqa: E731
        q, s, hq, hs, txc = mk(d.q), mk(d.s), mk(d.hq), mk(d.hs), mk(d.txc)
        dte = 2e-3 * KDT[0]
        prof = [np.cos(i + np.arange(d.ny)) for i in range(6)]
        P_ = lambda a: c_vp(a.ctypes.data)      # noqa: E731
        call = lambda o: check(L.tlab_dns_avg_gradients_flow(d._h, q, None, txc, P_(prof[0]), P_(prof[1]), P_(prof[2]), None, P_(prof[3]),      # noqa: E731
                                                             P_(prof[4]), P_(prof[5]), P_(o), d.ny), "tlab_dns_avg_gradients_flow")
        before = np.zeros((50, d.ny))
        call(before)                                                     # the statistics of the fields as they are set
        check(L.tlab_deferred_enable(1), "enable")
        try:
            check(L.tlab_deferred_rhs(d._h, dte, q, s, hq, hs, txc), "rhs")
            for h, u in zip(d.hq + d.hs, d.q + d.s):
                check(L.tlab_deferred_axpy(d.n, dte, h.data_ptr(), u.data_ptr()), "axpy")
            for h in d.hq + d.hs:
                check(L.tlab_deferred_scal(d.n, KCO[0], h.data_ptr()), "scal")
            if flush:
                check(L.tlab_deferred_flush(), "flush")
            out = np.zeros((50, d.ny))      # the entry point itself, with no other call of the library in front of it
            call(out)
            got.append(out)
        finally:
            check(L.tlab_deferred_enable(0), "disable")
    assert np.array_equal(got[0], got[1])
    assert not np.array_equal(got[0], before)                            # (the substep moved the fields: the call did not read the old ones)
