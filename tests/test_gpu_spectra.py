"""The plane spectra and correlations on the device (csrc/spectra.hip behind tlab_spectrum_reduce, tlab_correlation_reduce, tlab_spectra_pair,
tlab_dns_spectra) against tests/golden/spectra_ref.npz -- the reference's own compiled module SpectraMod -- and the numpy restatement
tests/spectra_oracle.py, which tests/test_spectra_host.py holds to that fixture bit for bit.

Reduce kernels, every box of the fixture -- (16, 5, 8); (32, 7, 16) with nblock 1, 2, 3 (planes dropped); (8, 4, 32) (the ring cut-off binds);
(20, 6, 12) (no powers of two); (12, 3, 9) (odd nz); (130, 3, 4) (nx/2+1 = 66: a wave and an odd tail); (256, 2, 16) -- with the arrays at offset 0
and at offset 1 double from a 16-byte boundary (8-byte loads of the complex numbers):
  exact data (integer parts, nx*nz a power of two, variances powers of four): np.array_equal with the fixture, in any summation order;
  rounding data: every output within the bound of two summation orders that tests/test_gpu_averages.py uses, 2 (n-1) u sum|t| + 2 u |ref| with
  u = 2^-53, t the terms of that output as the restatement lists them (the restatement run on |t| with every term added) and n their count
  (the restatement run on ones).  The largest fraction of the bound used is printed.

End to end (spectra_pair, Dns.spectra from physical fields) against the restatement with numpy's FFT.  Tolerance per output: the summation bound
plus 4 x the largest difference, on that very case, between the restatement with numpy's fp64 FFT and the restatement with the transforms as a
direct DFT in np.longdouble; both figures are printed.  A correlation divides by the two plane variances; the restatement is given the
variances the device returned (themselves held to the summation bound of a covariance), because COV2V2D's running sum over nx*nz terms is up to
35 u from the exact mean at nx*nz = 4096 -- more than the transforms' whole error -- while the kernel's order stays within about 2 u.  A Poisson plan needs at least 8 points in every direction (tlab_fdm_plan_create), so the
end-to-end boxes are the (nx, nz) of the list above with ny = 8; (130, ., 4) and (12, ., 9) have no plan and stay with the reduce kernels.
(256, 8, 16) is the box on which the library's own x and z FFT kernels run."""
import functools
import json
import os

import numpy as np
import pytest

import spectra_oracle as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
U53 = 2.0 ** -53
KEYS = ("xz", "x", "z", "r", "variance")
E2E = [((16, 8, 8), 1), ((32, 8, 16), 1), ((32, 8, 16), 2), ((32, 8, 16), 3), ((8, 8, 32), 1), ((20, 8, 12), 1), ((256, 8, 16), 1)]


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(HERE, "golden", "spectra_ref.npz"))
    return g, json.loads(str(g["index"]))


def records(kind, exact):
    return [(n, r) for n, r in enumerate(golden()[1]) if r["kind"] == kind and r["exact"] == exact]


def ids(recs):
    return ["%s-nblock%d%s" % (r["box"], r["nblock"], "-cross" if r.get("cross") else "") for _, r in recs]


def box(r):
    return tuple(int(v) for v in r["box"].split("x"))


def _dev(a, offset):
    """a device copy of a real or complex array, as float64, that starts `offset` doubles behind a 16-byte boundary"""
    import torch
    flat = np.ascontiguousarray(a).reshape(-1)
    flat = flat.view(np.float64) if flat.dtype == np.complex128 else flat.astype(np.float64)
    buf = torch.empty(flat.size + 2, dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:offset + flat.size]
    t.copy_(torch.from_numpy(flat.copy()))
    return t


def _host(o):
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in o.items()}


def _bound(ref, abs_sum, count):
    return 2.0 * np.maximum(count - 1.0, 0.0) * U53 * abs_sum + 2.0 * U53 * np.abs(ref)


def spectrum_terms(nx, ny, nz, nblock, kr, ah, bh):
    """(sum |t|, n) of every output of the spectrum route"""
    nkx, nyo = nx // 2, ny // nblock
    power = ((S.product(ah, bh) * (1.0 / (nx * nz))) * (1.0 / (nx * nz)))[S.shuffle(nz)]
    res = []
    for p in (np.abs(power), np.ones_like(power)):
        Sx, var = np.zeros((nz, nyo, nkx)), np.zeros(ny)
        S.reduce_spectrum(nx, ny, nz, nblock, p, Sx, var)
        o = {"xz": Sx, "x": np.zeros((nyo, nkx)), "z": np.zeros((nyo, nz // 2)), "r": np.zeros((nyo, kr)), "variance": var}
        S.integrate_spectrum(nkx, nyo, nz, kr, Sx, o["x"], o["z"], o["r"], sign=+1)
        res.append(o)
    res[1]["variance"] = np.where(res[1]["variance"] > 0, float(nz * (nkx + 1)), 0.0)      # (a term 2 P is one term)
    return res


def correlation_terms(nx, ny, nz, nblock, nr, field, var1, var2):
    x = np.abs((field * (1.0 / (nx * nz))) * (1.0 / (nx * nz)))
    a = S.correlation(nx, ny, nz, nblock, nr, x, var1, var2, norm=1.0)
    n = S.correlation(nx, ny, nz, nblock, nr, np.ones_like(x), var1, var2, norm=1.0, normj=np.ones(ny))
    n["variance"] = np.ones(ny)
    return a, n


def _check_rounding(got, ref, terms, what):
    worst = 0.0
    for k in KEYS:
        bound = _bound(ref[k], terms[0][k], terms[1][k])
        err = np.abs(got[k] - ref[k])
        frac = float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max()) if err.size else 0.0
        print("%s %s: largest error / bound = %.3f" % (what, k, frac))
        assert np.all(err <= bound), (what, k, frac)
        worst = max(worst, frac)
    return worst


# ---- the reduce kernels against the fixture ----------------------------------------------------------------------------------------------------------
def _run_spectrum(n, r, offset):
    import tlab_amd.operators as O
    g, _ = golden()
    nx, ny, nz = box(r)
    ah, bh = g["ah_" + r["box"]], g["bh_" + r["box"]] if r["cross"] else None
    o = O.spectrum_reduce(nx, ny, nz, r["nblock"], r["kr_total"], _dev(ah, offset), None if bh is None else _dev(bh, offset), out2d=True)
    return _host(o), {k: g["%s_%d" % (k, n)] for k in KEYS}, (nx, ny, nz, r["nblock"], r["kr_total"], ah, bh)


def _run_correlation(n, r, offset, **kw):
    import tlab_amd.operators as O
    g, _ = golden()
    nx, ny, nz = box(r)
    f, v1, v2 = g["field_" + r["box"]], g["var1_" + r["box"]], g["var2_" + r["box"]]
    o = O.correlation_reduce(nx, ny, nz, r["nblock"], r["nr_total"], _dev(f, offset), v1, v2, **kw)
    return _host(o), {k: g["%s_%d" % (k, n)] for k in KEYS}, (nx, ny, nz, r["nblock"], r["nr_total"], f, v1, v2)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n,r", records("spectrum", True), ids=ids(records("spectrum", True)))
def test_spectrum_reduce_exact_data_bit_for_bit(T, n, r, offset):
    got, ref, _ = _run_spectrum(n, r, offset)
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n,r", records("spectrum", False), ids=ids(records("spectrum", False)))
def test_spectrum_reduce_rounding_data_within_the_summation_bound(T, n, r, offset):
    got, ref, args = _run_spectrum(n, r, offset)
    worst = _check_rounding(got, ref, spectrum_terms(*args), "spectrum %s" % r["box"])
    print("spectrum %s nblock %d cross %d offset %d: largest fraction of the summation bound %.3f" % (r["box"], r["nblock"], r["cross"], offset, worst))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n,r", records("correlation", True), ids=ids(records("correlation", True)))
def test_correlation_reduce_exact_data_bit_for_bit(T, n, r, offset):
    got, ref, _ = _run_correlation(n, r, offset, out2d=True)
    for k in KEYS:
        assert np.array_equal(got[k], ref[k]), k
    got, _, _ = _run_correlation(n, r, offset, icalc_radial=0)      # the row and the column alone, no rings
    assert "r" not in got and np.array_equal(got["x"], ref["x"]) and np.array_equal(got["z"], ref["z"]) and np.array_equal(got["variance"], ref["variance"])


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n,r", records("correlation", False), ids=ids(records("correlation", False)))
def test_correlation_reduce_rounding_data_within_the_summation_bound(T, n, r, offset):
    got, ref, args = _run_correlation(n, r, offset, out2d=True)
    assert np.array_equal(got["variance"], ref["variance"])      # variance2 is a copy of a scaled point
    worst = _check_rounding(got, ref, correlation_terms(*args), "correlation %s" % r["box"])
    print("correlation %s nblock %d offset %d: largest fraction of the summation bound %.3f" % (r["box"], r["nblock"], offset, worst))


def test_outputs_accumulate_and_repeat_their_bits(T):
    """a second call adds to the accumulators it is handed (exact data: twice the fixture), and two calls from zero give the same bits"""
    import tlab_amd.operators as O
    n, r = records("spectrum", True)[1]
    g, _ = golden()
    nx, ny, nz = box(r)
    ah = _dev(g["ah_" + r["box"]], 0)
    o = O.spectrum_reduce(nx, ny, nz, r["nblock"], r["kr_total"], ah, out2d=True)
    first = _host(o)
    o = O.spectrum_reduce(nx, ny, nz, r["nblock"], r["kr_total"], ah, out={k: o[k] for k in ("x", "z", "r", "xz")}, out2d=True)
    for k in ("x", "z", "r", "xz"):
        assert np.array_equal(_host(o)[k], 2.0 * first[k]), k
    n, r = records("spectrum", False)[0]
    nx, ny, nz = box(r)
    ah, bh = _dev(g["ah_" + r["box"]], 0), _dev(g["bh_" + r["box"]], 0)
    one = _host(O.spectrum_reduce(nx, ny, nz, r["nblock"], r["kr_total"], ah, bh, out2d=True))
    two = _host(O.spectrum_reduce(nx, ny, nz, r["nblock"], r["kr_total"], ah, bh, out2d=True))
    for k in KEYS:
        assert np.array_equal(one[k], two[k]), k


def test_cross_product_and_fluctuation_and_covariances(T):
    import torch
    import tlab_amd.operators as O
    g, _ = golden()
    ah, bh = g["ah_20x6x12"], g["bh_20x6x12"]
    for offset in (0, 1):
        a, b = _dev(ah, offset), _dev(bh, offset)
        c = O.cross_product(a, b).cpu().numpy().view(np.complex128).reshape(ah.shape)
        assert np.array_equal(c.real, S.product(ah, bh)) and np.array_equal(c.imag, bh.imag * ah.real - bh.real * ah.imag)
        c = O.cross_product(a).cpu().numpy().view(np.complex128).reshape(ah.shape)
        assert np.array_equal(c.real, S.product(ah)) and not c.imag.any()
    f = np.ascontiguousarray(g["field_20x6x12"]) + np.cos(np.arange(6))[None, :, None]
    nz, ny, nx = f.shape
    df = _dev(f, 1)
    mean = O.avg_ik_v(nx, ny, nz, [f])[0]
    fl = O.fluctuation(nx, ny, nz, df, mean, torch.empty_like(df))
    assert np.array_equal(fl.cpu().numpy().reshape(f.shape), f - mean[None, :, None])
    assert np.array_equal(df.cpu().numpy().reshape(f.shape), f)
    h = np.ascontiguousarray(g["field_20x6x12"][::-1])
    cov = O.avg_cov2v(nx, ny, nz, df, _dev(h, 1))
    ref = np.stack([S.cov2v2d(f, h), S.cov2v2d(f, f), S.cov2v2d(h, h)])
    n = nx * nz
    absum = np.stack([np.abs(f * h).sum(axis=(0, 2)), (f * f).sum(axis=(0, 2)), (h * h).sum(axis=(0, 2))]) / n
    assert np.all(np.abs(cov - ref) <= _bound(ref, absum, n))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fields(shape):
    """two fluctuation fields: uniform(-1, 1) + a few waves, the plane means removed; read-only"""
    nx, ny, nz = shape
    rng = np.random.default_rng(300 + nx + nz)
    x, z = np.arange(nx)[None, None, :] / nx, np.arange(nz)[:, None, None] / nz
    amp = 1.0 + np.arange(ny)[None, :, None] / ny
    a = S.fluctuation(rng.uniform(-1, 1, (nz, ny, nx)) + amp * np.cos(2 * np.pi * (x + 2 * z)))
    b = S.fluctuation(rng.uniform(-1, 1, (nz, ny, nx)) + amp * np.sin(2 * np.pi * (2 * x - z)) + 0.5 * a)
    for f in (a, b):
        f.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def _reference(shape, nblock, mode, cross):
    a, b = _fields(shape)
    return _reference_of(a, b if cross else None, nblock, mode)


def _reference_of(a, b, nblock, mode, var=None, kr=None):
    """the restatement with numpy's FFT, the tolerance of every output, and the yardstick: its distance to the long double DFT.
    var: the two variances that normalise the correlations (the device's own, held to the covariance bound by _check_pair): the restatement's
    COV2V2D sums nx*nz terms one after the other and is up to 35 u from the exact mean at nx*nz = 4096, the kernel's tree-like order about 2 u;
    a correlation divides by the variances, so with each side's own the two would differ by that much whatever the transforms do"""
    nz, ny, nx = a.shape
    kr = (min(nx // 2, nz // 2) if mode == 1 else min(nx, nz)) if kr is None else kr
    ref = S.pair(mode, nblock, kr, a, b, var=var)
    ld = S.pair(mode, nblock, kr, a, b, fft=S.fft_direct, ifft=S.ifft_direct, var=var)
    if mode == 1:
        terms = spectrum_terms(nx, ny, nz, nblock, kr, S.fft_numpy(a), None if b is None else S.fft_numpy(b))
    else:
        bh = S.fft_numpy(a if b is None else b)
        field = S.ifft_numpy(bh * np.conj(S.fft_numpy(a)), nx)
        terms = correlation_terms(nx, ny, nz, nblock, kr, field, *((ref["cov"][1], ref["cov"][2]) if var is None else var))
    yard = {k: float(np.abs(ref[k] - np.asarray(ld[k], dtype=np.float64)).max()) for k in KEYS}
    tol = {k: _bound(ref[k], terms[0][k], terms[1][k]) + 4.0 * yard[k] for k in KEYS}
    n = nx * nz
    bb = a if b is None else b
    cov_bound = np.stack([_bound(ref["cov"][i], np.abs(p * q).sum(axis=(0, 2)) / n, n) for i, (p, q) in enumerate(((a, bb), (a, a), (bb, bb)))])
    return ref, ld, tol, yard, cov_bound, kr


def _check_pair(got, shape, nblock, mode, cross, what, reference=None, keys=KEYS, unit=None):
    ref, ld, tol, yard, cov_bound, _ = reference or _reference(shape, nblock, mode, cross)
    ny_loc = shape[1] - shape[1] % nblock
    for k in keys:
        err = np.abs(got[k] - ref[k])
        print("%s %s: device error %.3e, FFT yardstick %.3e, largest error / tolerance %.3f"
              % (what, k, float(err.max()), yard[k], float(np.divide(err, tol[k], out=np.zeros_like(err), where=tol[k] > 0).max())))
        assert np.all(err <= tol[k]), (what, k)
    # Parseval, the reference's own check (spectra.f90:662-666): variance (variance2) against the plane covariance
    assert np.all(np.abs(got["cov"] - ref["cov"]) <= cov_bound)
    cov_bound = cov_bound[0]
    resid = np.abs(got["variance"] - got["cov"][0])[:ny_loc]
    allowed = (tol["variance"] + cov_bound)[:ny_loc]
    print("%s Parseval residual %.3e (allowed %.3e)" % (what, float(resid.max()), float(allowed.max())))
    assert np.all(resid <= allowed), what
    if mode == 2 and not cross:      # an auto-correlation is 1 at zero separation in every plane of a block
        for k in ("x", "z"):
            assert np.all(np.abs(got[k][:, 0] - (nblock if unit is None else unit)) <= tol[k][:, 0]), (what, k)


@functools.lru_cache(maxsize=None)
def _plan(shape):
    import tlab_amd as T
    nx, ny, nz = shape
    g = [T.FdmPlan(np.arange(nx) / nx, True, True), T.FdmPlan(np.linspace(0.0, 1.0, ny), False, True), T.FdmPlan(np.arange(nz) / nz, True, True)]
    return T.PoissonPlan(g[0], g[1], g[2], nx, ny, nz)


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape,nblock", E2E, ids=["%dx%dx%d-nblock%d" % (s + (n,)) for s, n in E2E])
def test_spectra_pair_end_to_end(T, shape, nblock, mode, cross):
    import tlab_amd.operators as O
    a, b = _fields(shape)
    kr = _reference(shape, nblock, mode, cross)[5]
    da, db = _dev(a, 0), _dev(b, 0)
    got = _host(O.spectra_pair(_plan(shape), mode, nblock, kr, da, db if cross else None, out2d=True))
    reference = _reference_of(a, b if cross else None, nblock, mode, var=(got["cov"][1], got["cov"][2])) if mode == 2 else None
    _check_pair(got, shape, nblock, mode, cross, "spectra_pair %s nblock %d mode %d cross %d" % (shape, nblock, mode, cross), reference=reference)
    assert np.array_equal(da.cpu().numpy(), a.reshape(-1)) and np.array_equal(db.cpu().numpy(), b.reshape(-1))      # a and b are inputs


def _dns(shape, seed=5):
    import torch
    from tlab_amd.dns import Dns
    nx, ny, nz = shape
    d = Dns(np.arange(nx) / nx, np.linspace(0.0, 1.0, ny), np.arange(nz) / nz, nscal=1, visc=1e-3, schmidt=(1.0,))
    rng = np.random.default_rng(seed)
    Y = 0.5 + 0.5 * np.sin(np.pi * np.linspace(0.0, 1.0, ny))[None, :, None]      # (no plane without fluctuations: a correlation divides by them)
    f = {}
    for name, t in zip("uvw1", d.q + d.s):
        f[name] = rng.uniform(-1, 1, (nz, ny, nx)) * Y + 0.25 * np.cos(np.arange(ny))[None, :, None]
        t.copy_(torch.from_numpy(f[name].reshape(-1)))
    for t in d.hq + d.hs:
        t.copy_(torch.from_numpy(rng.uniform(-1, 1, t.numel())))
    return d, f


def _scaled(reference, nblock, inv_samples, cov_extra):
    """the reference of a pair after spectra.f90:683-690 (x 1/nblock) and :709-722 (radial correlations x 1/samplesize); two more roundings.
    cov_extra: what the plane means of the driver, summed in another order than the restatement's, may add to a covariance"""
    ref, ld, tol, yard, cov_bound, kr = reference
    cov_bound = cov_bound + cov_extra
    scale = 1.0 / nblock if nblock > 1 else 1.0
    ref, tol, yard = dict(ref), dict(tol), dict(yard)
    for k in ("x", "z", "r", "xz"):
        f = scale * (inv_samples[None, :] if k == "r" and inv_samples is not None else 1.0)
        ref[k] = ref[k] * scale
        if k == "r" and inv_samples is not None:
            ref[k] = ref[k] * inv_samples[None, :]
        tol[k] = tol[k] * f + 4.0 * U53 * np.abs(ref[k])
        yard[k] = yard[k] * float(np.max(f))
    return ref, ld, tol, yard, cov_bound, kr


DNS = [((16, 8, 16), 3), ((256, 8, 16), 1)]


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("mode", ["spectra", "correlations"])
@pytest.mark.parametrize("shape,nblock", DNS, ids=["%dx%dx%d-nblock%d" % (s + (n,)) for s, n in DNS])
def test_dns_spectra(T, shape, nblock, mode, cross):
    d, f = _dns(shape)
    nx, ny, nz = shape
    m = 1 if mode == "spectra" else 2
    state = [t.clone() for t in d.q + d.s + d.hq + d.hs]
    res = d.spectra(mode, cross, nblock, out2d=True)
    again = d.spectra(mode, cross, nblock, out2d=True)
    for t, t0 in zip(d.q + d.s + d.hq + d.hs, state):      # q, s, hq, hs are left alone
        assert np.array_equal(t.cpu().numpy(), t0.cpu().numpy())
    assert list(res) == [("E" if m == 1 else "C") + a + b for a, b in S.pairs(1, cross, False)]      # the reference's pairs, in its order
    kr = min(nx, nz) if (m == 2 and cross) else min(nx // 2, nz // 2)      # spectra.f90:271-282: the full length for cross-correlations only
    inv = None
    if m == 2:
        ss = S.radial_samplesize(nx, nz, kr)
        inv = np.where(ss > 0, 1.0 / np.where(ss > 0, ss, 1.0), ss)
    fl = {k: S.fluctuation(v) for k, v in f.items()}
    # a plane mean summed in two orders differs by dm <= 2 (n-1) u mean|a|; the fluctuation fields then differ by a constant per plane, and
    # mean((a + da)(b + db)) - mean(a b) = da mean(b) + db mean(a) + da db, with |mean(a)|, |mean(b)| <= mean|a|, mean|b|
    n = nx * nz
    dm = {k: 2.0 * (n - 1) * U53 * np.abs(v).mean(axis=(0, 2)) for k, v in f.items()}
    am = {k: np.abs(v).mean(axis=(0, 2)) for k, v in fl.items()}
    for name, (a, b) in zip(res, S.pairs(1, cross, False)):
        e = res[name]
        for k in e:      # two consecutive calls: the same bits
            assert np.array_equal(e[k], again[name][k]), (name, k)
        assert ("r" in e) == (nx == nz)      # spectra: nx == nz; correlations: dx = 1/nx equal to dz = 1/nz
        extra = np.stack([dm[p] * am[q] + dm[q] * am[p] + dm[p] * dm[q] for p, q in ((a, b), (a, a), (b, b))])
        R = _scaled(_reference_of(fl[a], None if a == b else fl[b], nblock, m, var=(e["cov"][1], e["cov"][2]) if m == 2 else None, kr=kr), nblock, inv, extra)
        if "r" in e:
            assert e["r"].shape == (ny // nblock, kr)
        keys = tuple(k for k in KEYS if k in e)
        _check_pair(e, shape, nblock, m, a != b, "Dns.spectra %s %s nblock %d" % (shape, name, nblock), reference=R, keys=keys, unit=1.0)
        ny_loc = ny - ny % nblock
        assert e["parseval"] == float(np.abs(e["variance"] - e["cov"][0])[:ny_loc].max())


def test_dns_spectra_with_the_pressure(T):
    import tlab_amd.operators as O
    d, f = _dns((16, 8, 8))
    res = d.spectra("spectra", False, 1, p=True)
    assert list(res) == ["Euu", "Evv", "Eww", "Epp", "E11"]
    p = d.txc[2][: d.n].clone()
    mean = O.avg_ik_v(16, 8, 8, [p])[0]
    fl = O.fluctuation(16, 8, 8, p, mean, p.clone())
    one = _host(O.spectra_pair(d.poisson, 1, 1, 4, fl))
    for k in ("x", "z"):      # (the plane means of p come from another launch there: one rounding of the mean, far below this)
        assert np.allclose(res["Epp"][k], one[k], rtol=1e-9, atol=1e-9 * np.abs(one[k]).max()), k


def test_refusals(T):
    import torch
    L = T.load()
    z = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")      # noqa: E731
    a, o = z(2 * 5 * 3 * 4), [z(64) for _ in range(4)]
    var = np.zeros(8)
    call = lambda nx, ny, nz, nb, a_, x_: L.tlab_spectrum_reduce(nx, ny, nz, nb, 2, a_, None, None, x_, o[1].data_ptr(), o[2].data_ptr(), var.ctypes.data)      # noqa: E731
    assert call(8, 3, 4, 1, a.data_ptr(), o[0].data_ptr()) == 0
    assert call(7, 3, 4, 1, a.data_ptr(), o[0].data_ptr()) == -1                 # odd nx: TLAB_EINVAL
    assert call(8, 3, 4, 0, a.data_ptr(), o[0].data_ptr()) == -1                 # nblock = 0
    assert call(8, 3, 1, 1, a.data_ptr(), o[0].data_ptr()) == -2                 # nz = 1: TLAB_EUNSUPPORTED
    host = np.zeros(64)
    assert call(8, 3, 4, 1, a.data_ptr(), host.ctypes.data) == -1                # host and device arrays in one call
    assert b"host and device" in L.tlab_last_error()
    f = z(8 * 3 * 4)
    corr = lambda nx, nz, nb, x_: L.tlab_correlation_reduce(nx, 3, nz, nb, 2, f.data_ptr(), var.ctypes.data, var.ctypes.data, None, x_, o[1].data_ptr(),      # noqa: E731
                                                            o[2].data_ptr(), var.ctypes.data, 1)
    assert corr(8, 4, 1, o[0].data_ptr()) == 0 and corr(7, 4, 1, o[0].data_ptr()) == -1 and corr(8, 4, 0, o[0].data_ptr()) == -1
    assert corr(8, 1, 1, o[0].data_ptr()) == -2 and corr(8, 4, 1, host.ctypes.data) == -1
    plan = _plan((16, 8, 8))
    t = [z(plan.isize_txc_field) for _ in range(4)]
    cov = np.zeros(24)
    pair = lambda mode, nb: L.tlab_spectra_pair(plan._h, mode, nb, 4, t[3].data_ptr(), None, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), None,      # noqa: E731
                                                o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), cov.ctypes.data, var.ctypes.data)
    assert pair(1, 1) == 0 and pair(3, 1) == -1 and pair(1, 0) == -1 and pair(1, 9) == -1
