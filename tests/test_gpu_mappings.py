"""The field mappings on the device (csrc/mappings.hip behind tlab_gradient_maps, tlab_dns_velocity_gradients, tlab_dns_scalar_gradient,
tlab_dns_fi_maps, tlab_dns_fi_diffusion, and the four Dns methods on top) against the numpy restatement tests/mappings_oracle.py, which
tests/test_mappings_host.py holds to the reference's own compiled routines.

The pass k_gradient_maps is compared with np.array_equal: one rounding per operation in the reference's order, every output, every map alone and
all maps in one call -- so the bits of a map do not depend on the maps that ride along.  The composed paths -- derivatives by other kernels than
the oracle's loops -- are held to the scatter bound of tests/scatter.py, per output.  What the Dns methods add on top of their parts (a scaling, a
ratio) is one IEEE operation and is compared exactly; their logarithms are within the 4 ulp of numpy that tests/test_gpu_sampling.py uses.

Sizes of the pass.  One thread takes two points per trip where every array is 16-byte aligned, one otherwise, 256 threads a workgroup, at most
GRADIENT_MAPS_MAX_BLOCKS workgroups (read from csrc/mappings_host.hpp): n = 1, 255, 256, 257 and 3 * 256 * 4 + 5 put the odd last point, a
partial workgroup and several workgroups on the 16-byte form, and n = 2 * blocks * 256 + 2 * 256 + 5 lies just past the grid cap of the 16-byte
form (and twice past that of the 8-byte form), so threads make a second trip of their loop.  A single pointer one double off -- an input, a
scalar gradient, an output -- takes the 8-byte form."""
import functools
import os
import re

import numpy as np
import pytest

import cases as C
import conditional_oracle as CO
import mappings_oracle as M
from conftest import rel_err
from launch_census import FAST, REF_HYPER, SMALL
from scatter import bound, scatter_of

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_HPP = open(os.path.join(ROOT, "tlab_amd", "csrc", "mappings_host.hpp")).read()
BLOCKS = int(re.search(r"GRADIENT_MAPS_MAX_BLOCKS\s*=\s*(\d+)", _HPP).group(1))
THREADS = int(re.search(r"GRADIENT_MAPS_THREADS\s*=\s*(\d+)", _HPP).group(1))
PAST_CAP = 2 * BLOCKS * THREADS + 2 * THREADS + 5
SIZES = [1, 255, 256, 257, 3 * 256 * 4 + 5, PAST_CAP]
VISC, SC = 1.0 / 800.0, (0.7,)
ALL = list(M.MAPS)


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def _dev(a, offset=0):
    """a device copy of a that starts `offset` doubles behind a 16-byte boundary"""
    import torch
    buf = torch.empty(a.size + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:offset + a.size]
    t.copy_(torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)))
    return t


def _outs(n, k, offsets=()):
    """k outputs full of NaN; those named in offsets one double off"""
    return [_dev(np.full(n, np.nan), 1 if i in offsets else 0) for i in range(k)]


def _flat(res, maps):
    return [a for m in maps for a in (res[m] if isinstance(res[m], tuple) else (res[m],))]


# ---- k_gradient_maps ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(n):
    """twelve gradients of n points, each on a scale of its own (the data of test_vorticity_from_gradients_is_the_formula_bit_for_bit), with every
    seventh point's scalar gradient zero (STRAIN_A's else-branch), and what the restatement gives: read-only, shared by the tests"""
    rng = np.random.default_rng(n)
    g = [rng.uniform(-2, 2, n) * 10.0 ** rng.integers(-3, 4) for _ in range(12)]
    for a in g[9:]:
        a[::7] = 0.0
    want = M.gradient_maps(g[:9], g[9:], M.MAPS)
    for a in g + [b for m in M.MAPS for b in want[m]]:
        a.setflags(write=False)
    return g, want


def _check(T, n, maps, dev, out, what):
    import torch
    _, want = _case(n)
    needs_s = any(m in M.SCALAR_MAPS for m in maps)
    ptrs = [o.data_ptr() for o in out]
    res = T.gradient_maps(dev[:9], dev[9:] if needs_s else None, maps, out=out)
    torch.cuda.synchronize()
    got = _flat(res, maps)
    assert [o.data_ptr() for o in got] == ptrs
    for a, b in zip(got, [w for m in maps for w in want[m]]):
        assert np.array_equal(a.cpu().numpy(), b), (n, what, maps)


@pytest.mark.parametrize("n", SIZES)
def test_all_maps_in_one_call_are_the_restatement_bit_for_bit(T, n):
    g, _ = _case(n)
    nout = sum(M.NOUT[m] for m in ALL)
    dev = [_dev(a) for a in g]
    _check(T, n, ALL, dev, _outs(n, nout), "aligned")
    # single pointers one double off: an input, a scalar gradient, the first and the last output
    for k in (1, 10):
        _check(T, n, ALL, [_dev(a, 1) if i == k else d for i, (a, d) in enumerate(zip(g, dev))], _outs(n, nout), "input %d off" % k)
    for k in (0, nout - 1):
        _check(T, n, ALL, dev, _outs(n, nout, (k,)), "output %d off" % k)


@pytest.mark.parametrize("n", SIZES)
def test_every_map_alone_is_the_restatement_bit_for_bit(T, n):
    """... with the very bits it has among all the others (both equal the restatement), aligned and with its last output one double off"""
    g, _ = _case(n)
    dev = [_dev(a) for a in g]
    for m in ALL:
        _check(T, n, [m], dev, _outs(n, M.NOUT[m]), "aligned")
        _check(T, n, [m], dev, _outs(n, M.NOUT[m], (M.NOUT[m] - 1,)), "output off")
    odd = [_dev(a, 1) if i in (4, 11) else d for i, (a, d) in enumerate(zip(g, dev))]
    for m in ALL:
        _check(T, n, [m], odd, _outs(n, M.NOUT[m]), "inputs 4, 11 off")


def test_the_pass_reads_no_gradient_it_does_not_need_and_takes_any_order(T):
    n = 257
    g, want = _case(n)
    dev = [_dev(a) for a in g]
    diag = [d if i in (0, 4, 8) else None for i, d in enumerate(dev[:9])]
    assert np.array_equal(T.gradient_maps(diag, None, "P")["P"].cpu().numpy(), want["P"][0])
    off = [None if i in (0, 4, 8) else d for i, d in enumerate(dev[:9])]
    got = T.gradient_maps(off, None, ["VORTICITY", "CURL"])
    assert np.array_equal(got["VORTICITY"].cpu().numpy(), want["VORTICITY"][0])
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got["CURL"], want["CURL"]))
    assert np.array_equal(T.gradient_maps([None] * 9, dev[9:], "GRADIENT")["GRADIENT"].cpu().numpy(), want["GRADIENT"][0])
    back = ALL[::-1]
    res = T.gradient_maps(dev[:9], dev[9:], back)
    for m in back:
        for a, b in zip(_flat(res, [m]), want[m]):
            assert np.array_equal(a.cpu().numpy(), b), m


def test_refusals_on_the_device(T):
    import torch
    n = 64
    g, _ = _case(257)
    dev = [_dev(a[:n]) for a in g]
    host = [np.array(a[:n]) for a in g]
    with pytest.raises(T.TlabError):                                           # a mix of host and device: an input, an output
        T.gradient_maps([host[0]] + dev[1:9], None, "Q")
    with pytest.raises(T.TlabError):
        T.gradient_maps(dev[:9], None, "Q", out=[np.zeros(n)])
    with pytest.raises(T.TlabError):                                           # aliasing
        T.gradient_maps(dev[:9], None, "Q", out=[dev[3]])
    buf = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    with pytest.raises(T.TlabError):
        T.gradient_maps(dev[:9], None, ["Q", "R"], out=[buf[:n], buf[n - 1:2 * n - 1]])
    with pytest.raises(T.TlabError):                                           # a missing ds3
        T.gradient_maps(dev[:9], None, "STRAIN_A")
    T.gradient_maps(dev[:9], None, ["Q", "R"], out=[buf[:n], buf[n:]])


# ---- the composed entry points on a driver --------------------------------------------------------------------------------------------------------
def _driver(T, shape, seed=3, stagger=False):
    import torch
    from tlab_amd.dns import Dns
    nx, ny, nz = shape
    x, y, z = C.grids(nx, ny, nz, True)
    q0, s0 = C.init_fields(nx, ny, nz, x, y, z, seed)
    d = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False, hyper_bc1_ext=REF_HYPER, stagger=stagger)
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(q0[i]))
    d.s[0].copy_(torch.from_numpy(s0[0]))
    return d, (x, y, z, q0, s0)


def _oracle(x, y, z):
    from oracle.tlab_oracle_rhs import DnsOracle
    return DnsOracle(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False)


def _oracle_p2(o):
    from oracle import tlab_oracle as O
    return lambda d, f: O.opr_partial(d, O.OPR_P2, o.nx, o.ny, o.nz, 0, o.g[d - 1], f)[0]


def _work(d, k):
    import torch
    return [torch.full((d.n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(k)]


@pytest.mark.parametrize("shape", [SMALL, FAST])
def test_fi_maps_with_all_maps(T, shape):
    import torch
    d, (x, y, z, q0, s0) = _driver(T, shape)
    nx, ny, nz = shape
    n = d.n
    before = [t.clone() for t in d.q + d.s]
    ds3 = _work(d, 3)
    res = T.fi_maps(d, d.q, d.s[0], ALL, d.txc[:9], ds3)
    got = [a.cpu().numpy() for a in _flat(res, ALL)]
    # the gradients left behind are twelve OPR_Partial calls, word for word, and the outputs are the pass over them
    grads = [t[:n].cpu().numpy() for t in d.txc[:9]] + [t.cpu().numpy() for t in ds3]
    r = torch.empty(n, dtype=torch.float64, device="cuda")
    for k, f in enumerate([d.q[0]] * 3 + [d.q[1]] * 3 + [d.q[2]] * 3 + [d.s[0]] * 3):
        (T.OPR_Partial_X, T.OPR_Partial_Y, T.OPR_Partial_Z)[k % 3](T.OPR_P1, nx, ny, nz, 0, d.g[k % 3], f, r)
        assert np.array_equal(grads[k], r.cpu().numpy()), k
    want = M.gradient_maps(grads[:9], grads[9:], ALL)
    for a, b in zip(got, [w for m in ALL for w in want[m]]):
        assert np.array_equal(a, b)
    for t, t0 in zip(d.q + d.s, before):
        assert torch.equal(t, t0)
    # ... and the velocity gradients and the scalar gradient on their own are the same arrays
    txc9, ds3b = _work(d, 9), _work(d, 3)
    T.velocity_gradients(d, d.q, txc9)
    T.scalar_gradient(d, d.s[0], ds3b)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(txc9 + ds3b, grads))

    o = _oracle(x, y, z)

    def run(u, v, w, s):
        du9 = [o.p1(dd, f) for f in (u, v, w) for dd in (1, 2, 3)]
        m = M.gradient_maps(du9, [o.p1(dd, s) for dd in (1, 2, 3)], ALL)
        return tuple(a for k in ALL for a in m[k])
    ref, sc = scatter_of(run, list(q0) + [s0[0]], nsamples=1)
    names = [("%s[%d]" % (m, k)) for m in ALL for k in range(M.NOUT[m])]
    for name, a, b, s in zip(names, got, ref, sc):
        err = rel_err(a, b)
        print("fi_maps %s %-24s err %.3e scatter %.3e" % (shape, name, err, s))
        assert err <= bound(s), name


@pytest.mark.parametrize("kind", sorted(M.FI_DIFFUSION))
def test_fi_diffusion(T, kind):
    import torch
    d, (x, y, z, q0, s0) = _driver(T, SMALL)
    rng = np.random.default_rng(11)
    p0 = np.cos(np.pi * np.tile(x, d.ny * d.nz)) + 0.1 * rng.uniform(-1, 1, d.n)      # a pressure-like field for STRAIN_PRESSURE
    f0 = p0 if kind == "STRAIN_PRESSURE" else s0[0]
    f = torch.from_numpy(f0).cuda() if kind in ("STRAIN_PRESSURE", "GRADIENT_DIFFUSION") else None
    before = [t.clone() for t in d.q + d.s]
    q = None if kind == "GRADIENT_DIFFUSION" else d.q
    got = T.fi_diffusion(d, kind, q, f, _work(d, 1)[0], _work(d, 6)).cpu().numpy()
    again = T.fi_diffusion(d, kind, q, f, _work(d, 1)[0], d.txc[:6]).cpu().numpy()
    assert np.array_equal(got, again)
    for t, t0 in zip(d.q + d.s, before):
        assert torch.equal(t, t0)
    o = _oracle(x, y, z)
    p2 = _oracle_p2(o)

    def run(u, v, w, ff):
        return (M.FI_DIFFUSION[kind](o.p1, p2, (u, v, w), ff),)
    (ref,), (sc,) = scatter_of(run, list(q0) + [f0], nsamples=1)
    err = rel_err(got, ref)
    print("fi_diffusion %s err %.3e scatter %.3e" % (kind, err, sc))
    assert err <= bound(sc)


def test_fi_diffusion_is_the_reference_call_sequence_on_the_device_operators(T):
    """VORTICITY_DIFFUSION restated with the public operators and torch for the pointwise lines (unfused single operations): equal bits"""
    import torch
    d, _ = _driver(T, SMALL)
    nx, ny, nz, n = d.nx, d.ny, d.nz, d.n
    P = (T.OPR_Partial_X, T.OPR_Partial_Y, T.OPR_Partial_Z)
    new = lambda: torch.empty(n, dtype=torch.float64, device="cuda")      # noqa: E731

    def p1(dd, f):
        r = new()
        P[dd - 1](T.OPR_P1, nx, ny, nz, 0, d.g[dd - 1], f, r)
        return r

    def p2(dd, f):
        r, w = new(), new()
        P[dd - 1](T.OPR_P2, nx, ny, nz, 0, d.g[dd - 1], f, r, w)
        return r
    u, v, w = d.q
    want = M.fi_vorticity_diffusion(p1, p2, u, v, w)
    got = T.fi_diffusion(d, "VORTICITY_DIFFUSION", d.q, None, new(), _work(d, 6))
    assert torch.equal(got, want)
    want = M.fi_strain_diffusion(p1, p2, u, v, w)
    got = T.fi_diffusion(d, "STRAIN_DIFFUSION", d.q, None, new(), _work(d, 6))
    assert torch.equal(got, want)


def test_named_forms_and_refusals_on_a_driver(T):
    import torch
    d, _ = _driver(T, SMALL)
    ds3 = _work(d, 3)
    allm = T.fi_maps(d, d.q, d.s[0], ALL, d.txc[:9], ds3)
    for fn, m in ((T.fi_strain, "STRAIN"), (T.fi_strain_tensor, "STRAIN_TENSOR"), (T.fi_curl, "CURL"), (T.fi_invariant_q, "Q"), (T.fi_invariant_r, "R"),
                  (T.fi_vorticity_production, "VORTICITY_PRODUCTION"), (T.fi_strain_production, "STRAIN_PRODUCTION")):
        got = fn(d, d.q, _work(d, 9))
        assert all(torch.equal(a, b) for a, b in zip(_flat({m: got}, [m]), _flat(allm, [m]))), m
    for fn, m in ((T.fi_gradient_production, "GRADIENT_PRODUCTION"), (T.fi_strain_a, "STRAIN_A")):
        got = fn(d, d.q, d.s[0], _work(d, 9), _work(d, 3))
        assert all(torch.equal(a, b) for a, b in zip(_flat({m: got}, [m]), _flat(allm, [m]))), m
    # FI_VORTICITY and FI_GRADIENT as the existing entry points give them
    assert torch.equal(allm["VORTICITY"], d.FI_VORTICITY()[: d.n])
    assert torch.equal(allm["GRADIENT"], T.fi_gradient(d, d.s[0], _work(d, 1)[0], _work(d, 1)[0]))
    with pytest.raises(T.TlabError):                                           # an output that is one of the gradient arrays
        T.fi_maps(d, d.q, None, "Q", d.txc[:9], out=[d.txc[4][: d.n]])
    with pytest.raises(T.TlabError):                                           # a scalar map without its arrays
        T.fi_maps(d, d.q, d.s[0], "STRAIN_A", d.txc[:9])
    with pytest.raises(T.TlabError):
        T.fi_diffusion(d, "GRADIENT_DIFFUSION", None, None, _work(d, 1)[0], _work(d, 6))
    st, _ = _driver(T, SMALL, stagger=True)
    with pytest.raises(T.TlabError, match=r"\(-2\)"):                          # TLAB_EUNSUPPORTED: the staggered grid
        T.velocity_gradients(st, st.q, [torch.empty(st.n, dtype=torch.float64, device="cuda") for _ in range(9)])


# ---- the Dns methods ------------------------------------------------------------------------------------------------------------------------------
def _ln_ok(ln, a, what):
    pos = a > 0.0
    assert pos.sum() > a.size // 2 and np.all(np.isneginf(ln[a == 0.0]))
    ln, want = ln[pos], np.log(a[pos])
    ulps = np.abs(ln - want) / np.spacing(np.abs(want))
    print("%s: worst distance to numpy %.2f ulp of the result" % (what, ulps.max()))
    assert np.all(ulps <= 4.0), (what, float(ulps.max()))


def test_dns_methods_are_the_composition_of_their_parts(T):
    import torch
    d, _ = _driver(T, SMALL)
    twin, _ = _driver(T, SMALL)
    n = d.n
    for a in d.hq + d.hs + twin.hq + twin.hs:
        a.fill_(0.25)
    before = [t.clone() for t in d.q + d.s + d.hq + d.hs]
    get = lambda t: t.cpu().numpy()      # noqa: E731

    inv = d.invariants()
    assert sorted(inv) == ["InvariantP", "InvariantQ", "InvariantR"]
    ens = d.enstrophy_equation()
    assert sorted(ens) == sorted(["EnstrophyW_iW_i", "LnEnstrophyW_iW_i", "ProductionW_iW_jS_ij", "DiffusionNuW_iLapW_i", "DilatationMsW_iW_iDivU",
                                  "RateAN_iN_jS_ij"])
    p = d.FI_PRESSURE_BOUSSINESQ(torch.empty(d.isize_txc_field, dtype=torch.float64, device="cuda"))
    stn = d.strain_equation()
    stn_p = d.strain_equation(p)
    assert sorted(stn) == sorted(["Strain2S_ijS_i", "LnStrain2S_ijS_i", "ProductionMs2S_ijS_jkS_ki", "DiffusionNuS_ijLapS_ij", "Pressure2S_ijP_ij"])
    grd = d.scalar_gradient_equation(0)
    assert sorted(grd) == sorted(["GradientG_iG_i", "LnGradientG_iG_i", "ProductionMsG_iG_jS_ij", "DiffusionNuG_iLapG_i", "StrainAMsN_iN_jS_ij"])
    for block in (inv, ens, stn, stn_p, grd):
        for k, t in block.items():
            assert t.shape == (n,) and t.dtype == torch.float64 and t.is_cuda, k
    for t, t0 in zip(d.q + d.s + d.hq + d.hs, before):
        assert torch.equal(t, t0)
    assert all(torch.equal(stn[k], stn_p[k]) for k in stn)

    parts = {m: get(a) for m, a in zip(["P", "Q", "R", "VORTICITY", "VORTICITY_PRODUCTION", "STRAIN", "STRAIN_PRODUCTION", "GRADIENT",
                                         "GRADIENT_PRODUCTION"],
                                        _flat(T.fi_maps(d, d.q, d.s[0], ["P", "Q", "R", "VORTICITY", "VORTICITY_PRODUCTION", "STRAIN", "STRAIN_PRODUCTION",
                                                                         "GRADIENT", "GRADIENT_PRODUCTION"], _work(d, 9), _work(d, 3)),
                                              ["P", "Q", "R", "VORTICITY", "VORTICITY_PRODUCTION", "STRAIN", "STRAIN_PRODUCTION", "GRADIENT",
                                               "GRADIENT_PRODUCTION"]))}
    dif = {k: get(T.fi_diffusion(d, k, d.q, {"GRADIENT_DIFFUSION": d.s[0], "STRAIN_PRESSURE": p}.get(k), _work(d, 1)[0], _work(d, 6)))
           for k in M.FI_DIFFUSION}
    visc, sch = d.visc, float(d.schmidt[0])
    want = {
        "InvariantP": parts["P"], "InvariantQ": parts["Q"], "InvariantR": parts["R"],
        "EnstrophyW_iW_i": parts["VORTICITY"], "ProductionW_iW_jS_ij": parts["VORTICITY_PRODUCTION"],
        "DiffusionNuW_iLapW_i": visc * dif["VORTICITY_DIFFUSION"], "DilatationMsW_iW_iDivU": parts["P"] * parts["VORTICITY"],
        "RateAN_iN_jS_ij": parts["VORTICITY_PRODUCTION"] / parts["VORTICITY"],
        "Strain2S_ijS_i": 2.0 * parts["STRAIN"], "ProductionMs2S_ijS_jkS_ki": 2.0 * parts["STRAIN_PRODUCTION"],
        "DiffusionNuS_ijLapS_ij": (2.0 * visc) * dif["STRAIN_DIFFUSION"], "Pressure2S_ijP_ij": 2.0 * dif["STRAIN_PRESSURE"],
        "GradientG_iG_i": parts["GRADIENT"], "ProductionMsG_iG_jS_ij": parts["GRADIENT_PRODUCTION"],
        "DiffusionNuG_iLapG_i": dif["GRADIENT_DIFFUSION"] * visc / sch, "StrainAMsN_iN_jS_ij": parts["GRADIENT_PRODUCTION"] / parts["GRADIENT"],
    }
    got = dict(inv, **ens, **stn, **grd)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, w in want.items():
            assert np.array_equal(get(got[k]), w, equal_nan=True), k
    _ln_ok(get(ens["LnEnstrophyW_iW_i"]), parts["VORTICITY"], "LnEnstrophyW_iW_i")
    _ln_ok(get(stn["LnStrain2S_ijS_i"]), 2.0 * parts["STRAIN"], "LnStrain2S_ijS_i")
    _ln_ok(get(grd["LnGradientG_iG_i"]), parts["GRADIENT"], "LnGradientG_iG_i")

    # a time step after the calls equals one on a twin driver that never made them
    d.TIME_RUNGEKUTTA(2e-3)
    twin.TIME_RUNGEKUTTA(2e-3)
    for a, b in zip(d.q + d.s + d.hq + d.hs, twin.q + twin.s + twin.hq + twin.hs):
        assert torch.equal(a, b)


def test_invariants_under_a_gate_feed_the_conditional_moments(T):
    """one composition into what exists: AVG_N_XZ of Dns.invariants() for the two levels of FI_GATE on the vorticity (opt_cond = 3) -- the counts
    equal the numpy restatement of tests/conditional_oracle.py on the same device fields, the means lie within its bound of two summation orders"""
    d, _ = _driver(T, SMALL)
    nx, ny, nz = SMALL
    inv = d.invariants()
    gate = d.FI_GATE(3, [0.1], relative=True)
    names = ["InvariantP", "InvariantQ", "InvariantR"]
    from tlab_amd.operators import avg_n_xz
    avg, sums, ns = avg_n_xz(nx, ny, nz, [inv[k] for k in names], 1, 2, gate, raw=True)
    f = [inv[k].cpu().numpy().reshape(nz, ny, nx) for k in names]
    g = gate.cpu().numpy().reshape(nz, ny, nx)
    assert set(np.unique(g)) == {1, 2}
    avg_r, sums_r, ns_r = CO.avg_n_xz(f, 1, 2, g)
    assert np.array_equal(ns, ns_r) and np.array_equal(avg, CO.central_of(sums, ns))
    nn = np.maximum(ns, 1)
    for v, k in enumerate(names):
        absum = np.array([[CO.raw_moment(np.abs(f[v][:, j, :]), 1, g[:, j, :] == l + 1)[0] for j in range(ny)] for l in range(2)])
        CO.within_bound(sums[:, v, 0] / nn, sums_r[:, v, 0] / nn, absum, ns, "gated mean of %s" % k)


# ---- a pending record of the deferred tail runs first ---------------------------------------------------------------------------------------------
def _entry(name):
    def deco(fn):
        fn.entry = name
        fn.opts = dict(pre=None, post=None, before=None, zeros=True, marker=False, relax=False, liquid=False, reset=None, probe=None)
        return fn
    return deco


def _pending_cases():
    """one raw ctypes call per entry point, as tests/test_gpu_deferred_entry_points.py shapes its cases: it reads state the pending substep
    changes (q, s[0]) and names what it wrote"""
    import ctypes
    from test_gpu_deferred_entry_points import N, P as A, PA, ok
    codes = (ctypes.c_int * 2)(1, 11)      # Q, STRAIN_A

    @_entry("tlab_gradient_maps")
    def maps(L, d, out):
        # the fields themselves stand for gradients: the pass reads what the substep updates
        du9 = PA([d.q[0], d.q[1], d.q[2], d.q[1], d.q[2], d.q[0], d.q[2], d.q[0], d.q[1]])
        ok(L.tlab_gradient_maps(N, du9, PA([d.s[0], d.q[0], d.q[1]]), codes, 2, PA(d.W[:4])), "tlab_gradient_maps")
        out["dev"] += [w[:N] for w in d.W[:4]]

    @_entry("tlab_dns_velocity_gradients")
    def vgrad(L, d, out):
        ok(L.tlab_dns_velocity_gradients(d._h, PA(d.q), PA(d.W[:9])), "tlab_dns_velocity_gradients")
        out["dev"] += [w[:N] for w in d.W[:9]]

    @_entry("tlab_dns_scalar_gradient")
    def sgrad(L, d, out):
        ok(L.tlab_dns_scalar_gradient(d._h, A(d.s[0]), PA(d.W[:3])), "tlab_dns_scalar_gradient")
        out["dev"] += [w[:N] for w in d.W[:3]]

    @_entry("tlab_dns_fi_maps")
    def fimaps(L, d, out):
        ok(L.tlab_dns_fi_maps(d._h, PA(d.q), A(d.s[0]), codes, 2, PA(d.W[:9]), PA(d.W[9:12]), PA(d.W[12:16])), "tlab_dns_fi_maps")
        out["dev"] += [w[:N] for w in d.W[12:16]]

    @_entry("tlab_dns_fi_diffusion")
    def diffusion(L, d, out):
        ok(L.tlab_dns_fi_diffusion(d._h, 0, PA(d.q), None, A(d.W[6]), PA(d.W[:6])), "tlab_dns_fi_diffusion")
        out["dev"] += [d.W[6][:N]]

    return [maps, vgrad, sgrad, fimaps, diffusion]


def test_a_pending_record_runs_first(T):
    """every entry point called through raw ctypes while the last substep of a step is only recorded: the record runs first, whole, as one fused
    substep -- what the call wrote and the fields equal, to the bit, the run with tlab_deferred_flush() in front, and differ from a call that ran
    ahead of the substep (the runs of tests/test_gpu_deferred_entry_points.py; tests/mappings_entry_points.py names this test)"""
    import torch
    from deferred_entry_points import STREAM
    from mappings_entry_points import ENTRY_POINTS, PENDING_TEST
    from test_gpu_deferred import _dns, _fields as _state
    from test_gpu_deferred_entry_points import Run, _same
    from tlab_amd.lib import load
    L = load()
    d = _dns(1)
    d.f0 = _state(d, 21)
    d.W = [torch.zeros(d.isize_txc_field, dtype=torch.float64, device="cuda") for _ in range(16)]
    d.liq = torch.zeros(d.n, dtype=torch.float64, device="cuda")
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
