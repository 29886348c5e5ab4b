"""The block stats_intermittency of DNS_STATISTICS (dns_statistics.f90:99-117) on the device: tlab_fi_vorticity with its pointwise kernel
k_vorticity_magnitude (csrc/pointwise.hip), tlab_inter_n_xz with k_gate_count (csrc/pdfs.hip), and Dns.intermittency(), against the numpy
restatement tests/pressure_oracle.py, which tests/test_pressure_host.py holds to the reference's own compiled routines.

The pointwise kernel and the gate counts are compared with np.array_equal: one rounding per operation in the reference's order, and integer counts.
FI_VORTICITY as a whole -- six derivatives by other kernels than the oracle's loops -- is held to the scatter bound of tests/scatter.py.

Sizes.  k_vorticity_magnitude: one thread takes two points per pass of 256 threads, so n = 1, 255, 256, 257 and 3 * 256 * 4 + 5 put the odd last
point, a partial pass and more than one workgroup on the 16-byte form; one pointer one double off takes the 8-byte form.  k_gate_count: a lane takes
16 gate bytes where the row starts on a 16-byte boundary, so nx in {1, 15, 16, 17, 33} covers rows without a full load, exactly one, one and a
tail, and rows whose start alternates between the two forms; nz in {1, R - 1, R, R + 1} sits on the seam of the R = PDF_ROWS_PER_GROUP rows of a
workgroup; the gate one byte off moves every row to the other form."""
import os
import re

import numpy as np
import pytest

import cases as C
import pressure_oracle as P
from conftest import rel_err
from launch_census import FAST, REF_HYPER, SMALL
from scatter import bound, scatter_of

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
R = int(re.search(r"PDF_ROWS_PER_GROUP\s*=\s*(\d+)", open(os.path.join(ROOT, "tlab_amd", "csrc", "pdfs_host.hpp")).read()).group(1))
VISC, SC = 1.0 / 800.0, (0.7,)


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
    t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return t


# ---- k_vorticity_magnitude ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 256 * 4 + 5])
def test_vorticity_from_gradients_is_the_formula_bit_for_bit(T, n):
    import torch
    rng = np.random.default_rng(n)
    six = [rng.uniform(-2, 2, n) * 10.0 ** rng.integers(-3, 4) for _ in range(6)]
    want = P.vorticity_from_gradients(*six)
    assert np.array_equal(want, ((six[0] - six[1]) * (six[0] - six[1]) + (six[2] - six[3]) * (six[2] - six[3])) + (six[4] - six[5]) * (six[4] - six[5]))
    for off in [None] + list(range(7)):                    # all seven aligned; each single pointer one double off
        offs = [1 if k == off else 0 for k in range(7)]
        dev = [_dev(a, o) for a, o in zip(six, offs[:6])]
        out = _dev(np.full(n, np.nan), offs[6])
        guard = out.storage_offset()
        got = T.vorticity_from_gradients(*dev, result=out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr() and out.storage_offset() == guard
        assert np.array_equal(got.cpu().numpy(), want), (n, off)


def test_vorticity_from_gradients_refuses_a_mix_of_host_and_device(T):
    a = np.ones(16)
    with pytest.raises(T.TlabError):
        T.vorticity_from_gradients(_dev(a), a, a, a, a, a, result=np.zeros(16))


# ---- tlab_fi_vorticity ------------------------------------------------------------------------------------------------------------------------
def _driver(T, shape):
    import torch
    from tlab_amd.dns import Dns
    nx, ny, nz = shape
    x, y, z = C.grids(nx, ny, nz, True)
    q0, s0 = C.init_fields(nx, ny, nz, x, y, z, 3)
    d = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False, hyper_bc1_ext=REF_HYPER)
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(q0[i]))
    d.s[0].copy_(torch.from_numpy(s0[0]))
    return d, (x, y, z, q0, s0)


def _oracle(x, y, z, q):
    from oracle.tlab_oracle_rhs import DnsOracle
    o = DnsOracle(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False)
    o.q = [np.array(a) for a in q]
    return o


@pytest.mark.parametrize("shape", [SMALL, FAST])
def test_fi_vorticity(T, shape):
    import torch
    d, (x, y, z, q0, s0) = _driver(T, shape)
    nx, ny, nz = shape
    n = d.n
    before = [t.clone() for t in d.q]
    vort = d.FI_VORTICITY()
    assert vort.data_ptr() == d.txc[0].data_ptr()
    six = [t[:n].cpu().numpy() for t in d.txc[3:9]]
    # the six arrays are six OPR_Partial calls: v,x  u,y  u,z  w,x  w,y  v,z
    res = torch.empty(n, dtype=torch.float64, device="cuda")
    for k, (fld, fn) in enumerate(((1, T.OPR_Partial_X), (0, T.OPR_Partial_Y), (0, T.OPR_Partial_Z), (2, T.OPR_Partial_X), (2, T.OPR_Partial_Y),
                                   (1, T.OPR_Partial_Z))):
        fn(T.OPR_P1, nx, ny, nz, 0, d.g[k % 3], d.q[fld], res)
        assert np.array_equal(six[k], res.cpu().numpy()), k
    got = vort[:n].cpu().numpy()
    assert np.array_equal(got, P.vorticity_from_gradients(*six))
    for t, t0 in zip(d.q, before):
        assert torch.equal(t, t0)

    def run(u, v, w):
        return (P.fi_vorticity(_oracle(x, y, z, (u, v, w)))[0],)
    (ref,), (sc,) = scatter_of(run, q0, nsamples=1)
    err = rel_err(got, ref)
    print("fi_vorticity %s err %.3e scatter %.3e" % (shape, err, sc))
    assert err <= bound(sc)


# ---- k_gate_count ---------------------------------------------------------------------------------------------------------------------------------
def _gate(nx, ny, nz, seed):
    """values 0..5, plane 0 empty; with ny > 1 the last plane full of level 1"""
    g = np.random.default_rng(seed).integers(0, 6, (nz, ny, nx)).astype(np.int8)
    g[:, 0, :] = 0
    if ny > 1:
        g[:, ny - 1, :] = 1
    return g


def _dev_gate(g, offset):
    import torch
    buf = torch.empty(g.size + 16, dtype=torch.int8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:offset + g.size]
    t.copy_(torch.from_numpy(g.reshape(-1)))
    return t


@pytest.mark.parametrize("nz", [1, R - 1, R, R + 1])
@pytest.mark.parametrize("nx", [1, 15, 16, 17, 33])
def test_inter_n_xz_equals_the_restatement(T, nx, nz):
    for ny in (1, 5):
        g = _gate(nx, ny, nz, 1000 * nx + nz + ny)
        for np_ in (1, 4):
            want = P.inter_n_xz(g, np_)
            for offset in (0, 1):
                got = T.inter_n_xz(nx, ny, nz, np_, _dev_gate(g, offset))
                assert got.shape == (np_, ny)
                assert np.array_equal(got, want), (nx, ny, nz, np_, offset)
            assert not want[:, 0].any() and (ny == 1 or want[0, ny - 1] == 1.0)      # the empty plane and the full one


def test_inter_n_xz_levels_sum_to_one_and_negative_values_are_no_levels(T):
    """a check of its own, not the comparison: every row of a level-complete gate sums to 1 within 1 ulp * np"""
    nx, ny, nz, np_ = 48, 7, 2 * R + 3, 5
    g = np.random.default_rng(9).integers(1, np_ + 1, (nz, ny, nx)).astype(np.int8)
    got = T.inter_n_xz(nx, ny, nz, np_, _dev_gate(g, 0))
    assert np.all(np.abs(got.sum(axis=0) - 1.0) <= np_ * np.finfo(np.float64).eps)
    assert np.array_equal(got, P.inter_n_xz(g, np_))
    g2 = g.copy()
    g2[g == 2] = -2
    g2[g == 3] = 127                                                                  # a level above np is not counted either
    got2 = T.inter_n_xz(nx, ny, nz, np_, _dev_gate(g2, 0))
    assert np.array_equal(got2, P.inter_n_xz(g2, np_)) and not got2[1].any() and not got2[2].any() and np.array_equal(got2[0], got[0])
    top = T.inter_n_xz(nx, ny, nz, 127, _dev_gate(g2, 0))                             # the largest np: level 127 is the last row
    assert np.array_equal(top[126], got[2]) and np.array_equal(top[:5], got2)


def test_inter_n_xz_host_gate_after_init_takes_the_host_loop(T):
    """the gate decides the branch: a host gate after tlab_init takes the reference's loop"""
    g = _gate(20, 4, 6, 3)
    assert np.array_equal(T.inter_n_xz(20, 4, 6, 3, g), T.inter_n_xz(20, 4, 6, 3, _dev_gate(g, 0)))


# ---- the block itself ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, FAST])
def test_intermittency_block_and_the_state_of_the_driver(T, shape):
    import torch
    a, (x, y, z, q0, s0) = _driver(T, shape)
    b, _ = _driver(T, shape)
    nx, ny, nz = shape
    a.begin_step()
    p = a.FI_PRESSURE_BOUSSINESQ().clone()                                           # dns_statistics.f90:93 in front: p stays where it is
    got = a.intermittency()
    assert torch.equal(a.txc[2], p)
    assert list(got) == ["Vorticity"] and got["Vorticity"].shape == (ny,)
    # the block composed from the restatement, on the device's own vorticity (whose parity is test_fi_vorticity's): gate and counts are exact
    vort = a.txc[0][: a.n].cpu().numpy()
    want, gate = P.intermittency(vort, nx, ny, nz)
    assert np.array_equal(got["Vorticity"], want["Vorticity"])
    assert gate.sum() > 0 and got["Vorticity"].max() <= 1.0
    # ... and from the oracle's vorticity: the same fractions unless a point sits within rounding of the threshold
    ref, _ = P.intermittency(P.fi_vorticity(_oracle(x, y, z, q0))[0], nx, ny, nz)
    assert np.abs(got["Vorticity"] - ref["Vorticity"]).max() <= 2.0 / (nx * nz)
    b.begin_step()
    for m in (a, b):
        m.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(2e-3 / 3.0, -5.0 / 9.0, True)
    for t, u in zip(a.q + a.s + a.hq + a.hs, b.q + b.s + b.hq + b.hs):
        assert torch.equal(t, u)
