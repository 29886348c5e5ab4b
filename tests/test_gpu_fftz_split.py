"""k_fftz with the exchanges in two rounds (real parts, then imaginary parts, through a buffer of n * T doubles; fftz.hip) against the
whole-complex form it replaces for n <= 512 (TLAB_FFTZ_SPLIT=0): the same operations on the same operands, so the same bits.

Line lengths 16 (8 x 2), 32 (8 x 4), 64 (8 x 8), 128 (8 x 8 x 2) and 512 (8 x 8 x 8) cover every radix tail and the pure radix-8 chain; 27 and 45
lines are no multiple of 8 or 16 lines per workgroup, so the last workgroup is partial.  The transforms run on kx-pencil plans (nxl * ny lines of nz
points), the way tests/test_gpu_poisson.py::test_own_z_fft_matches_numpy drives them."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(16, 3, 9), (16, 5, 9), (32, 3, 9), (32, 5, 9), (64, 3, 9), (64, 5, 9), (128, 3, 9), (128, 5, 9), (512, 3, 9)]      # nz, nxl, ny
_INPUTS = {}


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def _input(nz, nxl, ny):
    """Random complex lines from a fixed seed with exact zeros and negative zeros in both parts; made once, never modified."""
    key = (nz, nxl, ny)
    if key not in _INPUTS:
        rng = np.random.default_rng(1000 * nz + nxl)
        re, im = rng.uniform(-1, 1, (nz, ny, nxl)), rng.uniform(-1, 1, (nz, ny, nxl))
        for part in (re, im):
            part[rng.uniform(size=part.shape) < 0.05] = 0.0
            part[rng.uniform(size=part.shape) < 0.05] = -0.0
        re[0, 0, 0], im[0, 0, 0] = -0.0, 0.0
        a = re + 1j * im
        a.setflags(write=False)
        _INPUTS[key] = a
    return _INPUTS[key]


def _transforms(T, monkeypatch, nz, nxl, ny, split):
    """(forward of the input, backward of that forward) of one form, as complex arrays (nz, ny, nxl)."""
    import torch
    from tlab_amd.lib import load, check, c_vp
    monkeypatch.delenv("TLAB_FFTZ_T", raising=False)
    if split is None:
        monkeypatch.delenv("TLAB_FFTZ_SPLIT", raising=False)
    else:
        monkeypatch.setenv("TLAB_FFTZ_SPLIT", split)
    nx = 16
    x, y, z = np.arange(nx) / nx, np.arange(ny) / (ny - 1.0), np.arange(nz) / nz
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, True), T.FdmPlan(z, True, True)]
    h = c_vp(0)
    L = load()
    check(L.tlab_poisson_plan_create_pencil(ctypes.byref(h), gp[0]._h, gp[1]._h, gp[2]._h, nx, ny, nz // 2, nz, 2, nxl), "pencil plan")
    a = _input(nz, nxl, ny)
    da = torch.from_numpy(np.array(a).view(np.float64).reshape(-1)).cuda()
    db, dc = torch.empty_like(da), torch.empty_like(da)
    check(L.tlab_poisson_fft_z(h, 1, da.data_ptr(), db.data_ptr()), "fft_z")
    check(L.tlab_poisson_fft_z(h, -1, db.data_ptr(), dc.data_ptr()), "fft_z")           # unnormalised, like FFTW
    fwd = db.cpu().numpy().view(np.complex128).reshape(nz, ny, nxl)
    back = dc.cpu().numpy().view(np.complex128).reshape(nz, ny, nxl)
    check(L.tlab_poisson_plan_destroy(h), "destroy")
    return fwd, back


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("nz,nxl,ny", CASES)
def test_split_exchange_equals_whole_complex_exchange_bit_for_bit(T, monkeypatch, nz, nxl, ny):
    """Default form against TLAB_FFTZ_SPLIT=0, forward and backward, compared as uint64 (signs of zeros included); either form against numpy.fft along z
    to 1e-13 of the largest output magnitude (a sanity bound on an fp64 transform of at most 512 points, not a parity claim); forward then backward
    gives n times the input to the same bound."""
    a = _input(nz, nxl, ny)
    new = _transforms(T, monkeypatch, nz, nxl, ny, None)
    old = _transforms(T, monkeypatch, nz, nxl, ny, "0")
    for name, u, v in (("forward", new[0], old[0]), ("backward", new[1], old[1])):
        ndiff = int((_bits(u) != _bits(v)).sum())
        print("nz %3d lines %2d %-8s words that differ: %d of %d" % (nz, nxl * ny, name, ndiff, _bits(u).size))
        assert ndiff == 0, (name, ndiff)
    ref = np.fft.fft(a, axis=0)
    for form, (fwd, back) in (("split", new), ("whole", old)):
        ef = np.abs(fwd - ref).max() / np.abs(ref).max()
        eb = np.abs(back - nz * a).max() / (nz * np.abs(a).max())
        print("nz %3d lines %2d %-5s forward vs numpy %.2e  round trip %.2e" % (nz, nxl * ny, form, ef, eb))
        assert ef <= 1e-13, (form, ef)
        assert eb <= 1e-13, (form, eb)


def test_poisson_is_bit_identical_between_the_two_exchanges(T, monkeypatch):
    """OPR_Poisson on a 32 x 16 x 32 box: p and dp/dy with the default form and with TLAB_FFTZ_SPLIT=0, as uint64."""
    import torch
    nx, ny, nz = 32, 16, 32
    x, z = np.arange(nx) / nx * 2 * np.pi, np.arange(nz) / nz * 2 * np.pi
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5)) * 2.0
    gp = [T.FdmPlan(x, True, True), T.FdmPlan(y, False, False), T.FdmPlan(z, True, True)]
    rng = np.random.default_rng(7)
    N = nx * ny * nz
    f = rng.uniform(-1, 1, N)
    hb, ht = rng.uniform(-1, 1, nx * nz), rng.uniform(-1, 1, nx * nz)
    monkeypatch.delenv("TLAB_FFTZ_T", raising=False)
    outs = {}
    for split in (None, "0"):
        if split is None:
            monkeypatch.delenv("TLAB_FFTZ_SPLIT", raising=False)
        else:
            monkeypatch.setenv("TLAB_FFTZ_SPLIT", split)
        plan = T.PoissonPlan(gp[0], gp[1], gp[2], nx, ny, nz)
        p = torch.from_numpy(f.copy()).cuda()
        t1 = torch.empty(plan.isize_txc_field, dtype=torch.float64, device="cuda")
        t2 = torch.empty_like(t1)
        dpdy = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        T.OPR_Poisson(plan, nx, ny, nz, T.BCS_NN, p, t1, t2, torch.from_numpy(hb).cuda(), torch.from_numpy(ht).cuda(), dpdy)
        outs[split] = (p.cpu().numpy(), dpdy.cpu().numpy())
    for k, name in enumerate(("p", "dp/dy")):
        assert np.isfinite(outs[None][k]).all() and np.abs(outs[None][k]).max() > 0.0
        assert (_bits(outs[None][k]) == _bits(outs["0"][k])).all(), name
