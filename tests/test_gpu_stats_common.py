"""What the five statistics files share through csrc/stats_common.hpp, where sharing could break them without any other test noticing.

1. Growth while nested.  Every file has a device scratch of its own that grows on demand, and composed entry points (tlab_dns_spectra,
tlab_dns_gate) hold a pointer into their file's scratch while they call entry points of another file.  One process calls tlab_pdf1v_n,
tlab_cavg1v_n and tlab_avg_n_xz on a small box, on a larger one (every scratch is regrown) and on the small one again, then the two composed
entry points on a driver whose sizes fit none of the buffers left behind.  Counts, nsample, gates and bin centres must equal the host branch of
the same entry point (numpy arrays) in every word; sums are held to the bound of two summation orders of tests/test_gpu_conditional.py
(conditional_oracle.within_bound), spectra to the tolerances of tests/test_gpu_spectra.py (its own helpers, imported); the small box gives the
same bits before and after the large one.

2. The refusal of a mix of host and device arrays, one entry point per file: TLAB_EINVAL and the text `<name>: host and device arrays in one
call`, whole.  (The existing refusal tests match "host and device" or the code alone; none holds the whole text of these five.)"""
import numpy as np
import pytest

import conditional_oracle as C
from test_gpu_conditional import _dev, _dev_gate, _fields, _gate

pytestmark = pytest.mark.gpu

SMALL, LARGE = (8, 4, 8), (24, 9, 16)
NBINS, NM, LEVELS = 16, 4, 3


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def _three(shape, dev):
    """(pdf1v_n, cavg1v_n raw, avg_n_xz raw) of one box on device copies or on the numpy arrays themselves; ibc = 2: all three passes of PDF1V_N"""
    import tlab_amd.operators as O
    nx, ny, nz = shape
    f, g = _fields(shape), np.array(_gate(shape))
    put = _dev if dev else np.array
    u, a, gate = [put(f["u"]), put(f["v"])], put(f["a"]), (_dev_gate(g) if dev else g)
    return (O.pdf1v_n(nx, ny, nz, u, NBINS, 2, gate=gate, igate=2),
            O.cavg1v_n(nx, ny, nz, u, a, NBINS, 1, None, None, gate, 2, raw=True),
            O.avg_n_xz(nx, ny, nz, u, NM, LEVELS, gate, raw=True))


def _check_three(shape, got):
    nx, ny, nz = shape
    f, g = _fields(shape), _gate(shape)
    pdf_h, (avg_h, s_h, cnt_h), (_, sums_h, ns_h) = _three(shape, False)
    pdf, (avg, s, cnt), (mom, sums, ns) = got
    assert np.array_equal(pdf, pdf_h), (shape, "PDF1V_N: counts and centres")
    assert np.array_equal(cnt, cnt_h) and np.array_equal(ns, ns_h), (shape, "counts of CAVG1V_N, nsample")
    assert np.array_equal(avg[:, :, NBINS:], avg_h[:, :, NBINS:]) and np.array_equal(s[:, :, NBINS:], s_h[:, :, NBINS:]), (shape, "centres")
    assert np.array_equal(avg[:, :, :NBINS], C.divide(s[:, :, :NBINS], cnt[:, :, :NBINS])), "one division per bin"
    assert np.array_equal(mom, C.central_of(sums, ns))
    # sums: the bound of two summation orders, as tests/test_gpu_conditional.py holds them (sum|a| per bin from the restatement)
    sa = C.cavg1v_n([f["u"], f["v"]], f["a"], NBINS, [1, 1], None, None, g, 2)[3]
    C.within_bound(avg[:, :, :NBINS], avg_h[:, :, :NBINS], sa[:, :, :NBINS], cnt_h[:, :, :NBINS], "%s <a|.>" % (shape,))
    nn = np.maximum(ns, 1)
    for v, k in enumerate(("u", "v")):
        for m in range(1, NM + 1):
            absum = np.array([[C.raw_moment(np.abs(f[k][:, j, :]), m, g[:, j, :] == l + 1)[0] for j in range(ny)] for l in range(LEVELS)])
            C.within_bound(sums[:, v, m - 1] / nn, sums_h[:, v, m - 1] / nn, absum, ns, "%s raw moment %s**%d" % (shape, k, m))


def _same(a, b):
    flat = lambda r: [x for part in r for x in (part if isinstance(part, tuple) else (part,))]      # noqa: E731
    return all(np.array_equal(x, y) for x, y in zip(flat(a), flat(b)))


def test_buffers_grow_while_calls_nest(T):
    import torch
    from test_gpu_spectra import KEYS, _check_pair, _dns, _reference_of, _scaled
    import spectra_oracle as S
    first = _three(SMALL, True)
    _check_three(SMALL, first)
    _check_three(LARGE, _three(LARGE, True))
    assert _same(_three(SMALL, True), first), "the small box after the large one: other bits"
    # the composed entry points on a driver, with every scratch at a size of other calls
    shape = (16, 8, 16)
    nx, ny, nz = shape
    d, f = _dns(shape)
    res, again = d.spectra("spectra", False, 1, out2d=True), d.spectra("spectra", False, 1, out2d=True)
    fl = {k: S.fluctuation(v) for k, v in f.items()}
    n, u53 = nx * nz, 2.0 ** -53
    dm = {k: 2.0 * (n - 1) * u53 * np.abs(v).mean(axis=(0, 2)) for k, v in f.items()}      # (the derivation: test_gpu_spectra.test_dns_spectra)
    am = {k: np.abs(v).mean(axis=(0, 2)) for k, v in fl.items()}
    assert list(res) == ["E" + a + b for a, b in S.pairs(1, False, False)]
    for name, (a, b) in zip(res, S.pairs(1, False, False)):
        e = res[name]
        assert all(np.array_equal(e[k], again[name][k]) for k in e), name
        extra = np.stack([2.0 * dm[a] * am[a] + dm[a] * dm[a]] * 3)
        R = _scaled(_reference_of(fl[a], None, 1, 1, kr=min(nx // 2, nz // 2)), 1, None, extra)
        _check_pair(e, shape, 1, 1, False, "Dns.spectra after the regrowth, %s" % name, reference=R, keys=tuple(k for k in KEYS if k in e), unit=1.0)
    # FI_GATE, opt_cond = 6 (tlab_avg_ik_v, tlab_fluctuation, tlab_minmax, tlab_gate_levels inside tlab_dns_gate): the indicator as
    # tests/test_gpu_conditional.py holds it, its gate equal to the host branch of tlab_gate_levels in every byte
    import tlab_amd.operators as O
    thr = [0.25, 0.5, 0.75]
    gate = d.FI_GATE(6, thr, relative=True).cpu().numpy()
    ind = d.txc[0][: d.n].cpu().numpy()
    assert np.allclose(ind.reshape(nz, ny, nx), f["1"] - f["1"].mean(axis=(0, 2))[None, :, None], rtol=0, atol=1e-13)
    assert np.array_equal(gate, O.gate_levels(ind, C.relative_thresholds(thr, ind))) and len(np.unique(gate)) >= 2
    assert np.array_equal(d.FI_GATE(6, thr, relative=True).cpu().numpy(), gate)
    _check_three(SMALL, _three(SMALL, True))
    torch.cuda.synchronize()


def test_a_mix_of_host_and_device_arrays_is_refused_in_the_same_words_by_every_file(T):
    import torch
    import tlab_amd.operators as O
    nx, ny, nz = SMALL
    dev = torch.zeros(nx * ny * nz, dtype=torch.float64, device="cuda")
    host = np.zeros(nx * ny * nz)
    acc = np.zeros(2 * 3 * ny * nx)                                                                       # (fields, avg_planes + 1, ny, nx)
    calls = {
        "tlab_avg_ik_v": lambda: O.avg_ik_v(nx, ny, nz, [dev, host]),                                     # averages.cpp
        "tlab_pdf_minmax_planes": lambda: O.pdf_minmax_planes(nx, ny, nz, [host, dev]),                   # pdfs.cpp
        "tlab_avg_phase_space": lambda: O.avg_phase_space(nx, ny, nz, [dev, dev], 2, 1, acc),             # sampling.cpp
        "tlab_fluctuation": lambda: O.fluctuation(nx, ny, nz, dev, np.zeros(ny), host),                   # spectra.cpp
        "tlab_gate_flux": lambda: O.gate_flux(dev, host, torch.zeros(dev.numel(), dtype=torch.int8, device="cuda")),      # conditional.cpp
    }
    for name, call in calls.items():
        with pytest.raises(T.TlabError) as e:
            call()
        assert T.load().tlab_last_error().decode() == name + ": host and device arrays in one call", name
        assert str(e.value) == "%s failed (-1): %s: host and device arrays in one call" % (name, name)      # -1: TLAB_EINVAL
