"""DNS_FILTER of the single-domain driver (tlab_dns_set_filter, tlab_dns_filter; Dns.set_filter, Dns.DNS_FILTER): the filters on u, v, w and the
scalar in place, then the scalar bounds, then the diagnostic liquid -- and nothing else of the driver.

The filters are the three of tests/test_gpu_filter_boxes.py (KX periodic compactcutoff of 37 points, KY biased compact of 24, KZ periodic
explicit4 of 130) on the nodes of test_dealiased_burgers_off_the_cube, with the asserts that the tables belong to those nodes.  A driver needs an
even Imax (OPR_Fourier, opr_fourier.f90:72-75: the reference refuses an odd one and so does tlab_poisson_plan_create), so the 37 points cannot lie
along x: the box is 130 x 24 x 37, KZ filters along x and KX along z.  The same three tables, line lengths and periodicities, all extents
different; 37 x 24 x 130 itself is covered without a driver in tests/test_gpu_filter_stream.py.

Bound: equality of every 64-bit word with oracle.tlab_oracle_filter.opr_filter (and np.clip of it for the bounded scalar): the kernels keep the
reference's operation order (tests/test_gpu_filter_stream.py), the clip and the copy are exact."""
import numpy as np
import pytest
from test_oracle_filter import G, GB
from test_gpu_filter_boxes import KX, KY, KZ, device_filter, field, oracle_filters, refused, words

pytestmark = pytest.mark.gpu
NX, NY, NZ = 130, 24, 37
N = NX * NY * NZ
KEYS = (KZ, KY, KX)                    # along x, y, z
MIXTURE = (1.5, 0.1)                   # thermo_param of AirWaterLinear with one scalar: the weight of the scalar and the smoothing
DTE, KCO = 1e-3, -5.0 / 9.0


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def grid():
    x, z = np.arange(NX) / NX * 2.0, np.arange(NZ) / NZ * 2.0
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(NY) / (NY - 1) - 1)) / np.tanh(1.5))
    assert np.array_equal(x, GB["n130_x"]) and np.array_equal(y, G["n24_y"]) and np.array_equal(z, GB["n37_x"])    # the tables belong to these nodes
    return x, y, z


_CASE = {}


def case():
    """the initial fields u, v, w, s and the oracle's filter of each, once for the module"""
    if not _CASE:
        from oracle import tlab_oracle_filter as F
        _CASE["u0"] = [field([31, k], N) for k in range(4)]
        _CASE["uf"] = [F.opr_filter(NX, NY, NZ, oracle_filters(KEYS, None), u) for u in _CASE["u0"]]
        fs = _CASE["uf"][3]
        _CASE["lo"], _CASE["hi"] = (float(v) for v in np.quantile(fs, [0.1, 0.9]))      # inside the filtered range: the clip changes a fifth of the points
        assert fs.min() < _CASE["lo"] < _CASE["hi"] < fs.max()
    return _CASE


def driver(T, fields, filters=True, bounds=True, mixture=False):
    import torch
    from tlab_amd.dns import Dns
    x, y, z = grid()
    d = Dns(x, y, z, nscal=1, visc=1.0 / 500.0, schmidt=(1.0,), yuniform=False)
    if mixture:
        d.set_mixture("airwaterlinear", MIXTURE)
    if filters:
        d.set_filter(*(device_filter(T, k) for k in KEYS))
    if bounds:
        d.set_scalar_bounds([case()["lo"]], [case()["hi"]])
    for t, a in zip(d.q + d.s, fields):
        t.copy_(torch.from_numpy(a))
    return d


def host(t):
    return t.cpu().numpy()


def same(got, want, what):
    bad = int(np.count_nonzero(words(got) != words(want)))
    print("%s: words differing %d / %d" % (what, bad, want.size))
    assert bad == 0, (what, "%d of %d words differ" % (bad, want.size))


def test_filter_then_bounds(T):
    c = case()
    d = driver(T, c["u0"])
    tend = [field([37, k], N) for k in range(4)]                      # the tendencies must come through untouched
    import torch
    for t, a in zip(d.hq + d.hs, tend):
        t.copy_(torch.from_numpy(a))
    d.DNS_FILTER()
    for k, name in enumerate("uvw"):
        same(host(d.q[k]), c["uf"][k], name)
    clipped = np.clip(c["uf"][3], c["lo"], c["hi"])
    assert np.count_nonzero(clipped != c["uf"][3]) > N // 10         # the clip changes points
    same(host(d.s[0]), clipped, "s")
    for t, a, name in zip(d.hq + d.hs, tend, ("hq1", "hq2", "hq3", "hs1")):
        same(host(t), a, name)


def test_diagnostic_follows_the_bounds(T):
    """with a mixture the liquid is that of the filtered and clipped scalar"""
    c = case()
    d = driver(T, c["u0"], mixture=True)
    d.liquid.fill_(-7.0)
    d.DNS_FILTER()
    clipped = np.clip(c["uf"][3], c["lo"], c["hi"])
    same(host(d.s[0]), clipped, "s")
    e = driver(T, c["uf"][:3] + [clipped], filters=False, bounds=False, mixture=True)
    e.FI_DIAGNOSTIC()
    liq = host(e.liquid)
    assert np.ptp(liq) > 1e-3                                          # (the liquid depends on the scalar)
    same(host(d.liquid), liq, "liquid")


def test_without_a_filter_only_the_clip_and_the_diagnostic_act(T):
    c = case()
    d = driver(T, c["u0"], filters=False, mixture=True)
    d.liquid.fill_(-7.0)
    d.DNS_FILTER()
    for k, name in enumerate("uvw"):
        same(host(d.q[k]), c["u0"][k], name)
    lo, hi = c["lo"], c["hi"]
    clipped = np.clip(c["u0"][3], lo, hi)
    assert np.count_nonzero(clipped != c["u0"][3]) > 0
    same(host(d.s[0]), clipped, "s")
    e = driver(T, c["u0"][:3] + [clipped], filters=False, bounds=False, mixture=True)
    e.FI_DIAGNOSTIC()
    same(host(d.liquid), host(e.liquid), "liquid")
    # set and taken away again: the same
    d2 = driver(T, c["u0"], filters=True, bounds=False)
    d2.set_filter(None, None, None)
    d2.DNS_FILTER()
    for k, name in enumerate(("u", "v", "w", "s")):
        same(host((d2.q + d2.s)[k]), c["u0"][k], name + " (filter switched off)")


def test_the_driver_is_as_if_loaded_with_the_filtered_fields(T):
    """one substep after the filter equals the substep of a second driver that was loaded with the filtered fields from the host"""
    c = case()
    a = driver(T, c["u0"])
    a.DNS_FILTER()
    loaded = [host(t).copy() for t in a.q + a.s]
    b = driver(T, loaded, filters=False)
    for d in (a, b):
        d.begin_step()
        d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(DTE, KCO, True)
    names = ("u", "v", "w", "s", "hq1", "hq2", "hq3", "hs1")
    for ta, tb, name in zip(a.q + a.s + a.hq + a.hs, b.q + b.s + b.hq + b.hs, names):
        ha = host(ta)
        assert np.isfinite(ha).all(), name
        same(ha, host(tb), name + " after a substep")
    assert np.abs(host(a.q[0]) - loaded[0]).max() > 0.0             # (the substep did something)


def test_a_filter_of_the_wrong_size_is_refused_and_changes_nothing(T):
    c = case()
    d = driver(T, c["u0"], bounds=False)
    fx, fy, fz = (device_filter(T, k) for k in KEYS)
    refused(T, lambda: d.set_filter(fz, fy, fz), "filter size does not match")        # 37 points along x = 130
    refused(T, lambda: d.set_filter(fx, device_filter(T, "n64_t1_p0_b11"), fz), "filter size does not match")
    refused(T, lambda: d.set_filter(fx, fy, fz, (1, 0, 1)), "Repeat must be positive")
    d.DNS_FILTER()                                                     # the filters set before the refusals, once each
    for k, name in enumerate(("u", "v", "w", "s")):
        same(host((d.q + d.s)[k]), c["uf"][k], name + " after the refusals")
