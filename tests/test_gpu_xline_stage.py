"""k_xline on 512-point periodic lines: the staged form (lane-linear 16-byte global accesses, change of layout through a wave-private LDS row; the
default) against the direct form (TLAB_XLINE_STAGE=0, read per launch).  Only data movement differs, so the two agree bit for bit -- operators and a
whole Runge-Kutta step -- and each keeps the 1e-12 parity of test_gpu_derivs.py with the oracle.  Every comparison also reads the library's profile:
each setting must have launched the kernel under its own name (k_xline<P1> / k_xline<BURGERS> against k_xline<P1,direct> / k_xline<BURGERS,direct>).

Shapes: 512 x 5 x 3 = 15 lines (not a multiple of the 4 lines of a workgroup; wall rows j = 0, 4), 512 x 16 x 8, and -- operators only -- 512 x 96 x 96
= 9216 lines: the grid is capped at 2048 workgroups of 4 lines, so that only beyond 8192 lines a workgroup takes a second line with its operand
requested ahead (the lines from 8192 on are the ones checked against the oracle there)."""
import ctypes

import numpy as np
import pytest
from conftest import rel_err
from cases import grids, init_fields

pytestmark = pytest.mark.gpu
TOL = 1e-12
NX = 512
SHAPES = [(5, 3), (16, 8)]


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


@pytest.fixture(scope="module")
def plans(T):
    from oracle import tlab_oracle as O
    x = np.arange(NX) / NX
    return T.FdmPlan(x, True, True), O.FdmPlan(x, True, True)


def _profiled(fn):
    """fn() with every launch timed by the library; returns the set of kernel names it launched"""
    import torch
    from tlab_amd.lib import load
    L = load()
    L.tlab_profile_filter(None); L.tlab_profile_reset(); L.tlab_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.tlab_profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 14)
    L.tlab_profile_report(buf, len(buf))
    L.tlab_profile_reset()
    return {ln.split("\t")[0] for ln in buf.value.decode().split("\n") if ln}


def _both(monkeypatch, fn, kernel):
    """fn() under the default and under TLAB_XLINE_STAGE=0; checks the kernel names; returns (staged, direct) results"""
    direct_name = kernel[:-1] + ",direct>"
    monkeypatch.delenv("TLAB_XLINE_STAGE", raising=False)
    out = {}
    names = _profiled(lambda: out.__setitem__("staged", fn()))
    assert kernel in names and direct_name not in names, names
    monkeypatch.setenv("TLAB_XLINE_STAGE", "0")
    names = _profiled(lambda: out.__setitem__("direct", fn()))
    assert direct_name in names and kernel not in names, names
    monkeypatch.delenv("TLAB_XLINE_STAGE")
    return out["staged"], out["direct"]


def _operands(ny, nz, seed):
    rng = np.random.default_rng(seed)
    N = NX * ny * nz
    i = np.arange(N)
    u = np.sin(0.37 * (i % NX)) * np.cos(0.11 * (i // NX)) + 0.1 * rng.uniform(-1, 1, N)
    v = np.cos(0.23 * (i % NX)) + 0.1 * rng.uniform(-1, 1, N)
    return u, v, rng.uniform(-1, 1, N)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("ny,nz", SHAPES)
def test_partial_x_plain_and_accumulating(T, plans, monkeypatch, ny, nz):
    import torch
    from oracle import tlab_oracle as O
    from tlab_amd.lib import load, check
    L = load()
    gp, op = plans
    u, ub, h0 = _operands(ny, nz, 7)
    du, dub = _dev(u), _dev(ub)
    tmp1, tmp2 = torch.empty_like(du), torch.empty_like(du)

    def plain():
        res = torch.full_like(du, float("nan"))
        T.OPR_Partial_X(T.OPR_P1, NX, ny, nz, 0, gp, du, res, tmp1)
        return res
    a, b = _both(monkeypatch, plain, "k_xline<P1>")
    assert torch.equal(a, b)
    ref = O.opr_partial(1, O.OPR_P1, NX, ny, nz, 0, op, u)[0]
    assert rel_err(a.cpu().numpy(), ref) <= TOL

    def accumulating():      # result += d/dx (u + 0.75 ub): old result and second operand in, the operand sum of the pressure forcing
        res = _dev(h0)
        check(L.tlab_opr_partial_add(1, gp._h, NX, ny, nz, 0, du.data_ptr(), dub.data_ptr(), 0.75, res.data_ptr(), 1, tmp1.data_ptr(), tmp2.data_ptr()),
              "tlab_opr_partial_add")
        return res
    a, b = _both(monkeypatch, accumulating, "k_xline<P1>")
    assert torch.equal(a, b)
    ref2 = h0 + O.opr_partial(1, O.OPR_P1, NX, ny, nz, 0, op, u + 0.75 * ub)[0]
    assert rel_err(a.cpu().numpy(), ref2) <= TOL


@pytest.mark.parametrize("ny,nz", SHAPES)
def test_burgers_x(T, plans, monkeypatch, ny, nz):
    import torch
    from oracle import tlab_oracle as O
    gp, op = plans
    u, v, _ = _operands(ny, nz, 11)
    du, dv = _dev(u), _dev(v)
    tmp = torch.empty_like(du)
    for ivel, vel, dvel in ((T.OPR_B_U_IN, v, dv), (T.OPR_B_SELF, u, du)):
        def run():
            res = torch.full_like(du, float("nan"))
            T.OPR_Burgers_X(ivel, 1e-3, NX, ny, nz, 0, gp, du, dvel, res, tmp)
            return res
        a, b = _both(monkeypatch, run, "k_xline<BURGERS>")
        assert torch.equal(a, b), ivel
        ref = O.opr_burgers(1, NX, ny, nz, 0, op, 1e-3, u, vel)[0]
        assert rel_err(a.cpu().numpy(), ref) <= TOL, ivel


def test_second_line_of_a_workgroup(T, plans, monkeypatch):
    """9216 lines on 2048 workgroups of 4: the first 256 workgroups take a second line set, whose operands the kernels request during the first"""
    import torch
    from oracle import tlab_oracle as O
    gp, op = plans
    ny = nz = 96
    first = 8192                       # first line of the second pass
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    N = NX * ny * nz
    du = 2.0 * torch.rand(N, dtype=torch.float64, device="cuda", generator=gen) - 1.0
    dv = 2.0 * torch.rand(N, dtype=torch.float64, device="cuda", generator=gen) - 1.0
    tmp = torch.empty_like(du)
    tail_u, tail_v = du[first * NX:].cpu().numpy(), dv[first * NX:].cpu().numpy()
    nt = ny * nz - first

    def p1():
        res = torch.full_like(du, float("nan"))
        T.OPR_Partial_X(T.OPR_P1, NX, ny, nz, 0, gp, du, res, tmp)
        return res
    a, b = _both(monkeypatch, p1, "k_xline<P1>")
    assert torch.equal(a, b)
    assert rel_err(a[first * NX:].cpu().numpy(), O.opr_partial(1, O.OPR_P1, NX, nt, 1, 0, op, tail_u)[0]) <= TOL

    def burgers():
        res = torch.full_like(du, float("nan"))
        T.OPR_Burgers_X(T.OPR_B_U_IN, 1e-3, NX, ny, nz, 0, gp, du, dv, res, tmp)
        return res
    a, b = _both(monkeypatch, burgers, "k_xline<BURGERS>")
    assert torch.equal(a, b)
    assert rel_err(a[first * NX:].cpu().numpy(), O.opr_burgers(1, NX, nt, 1, 0, op, 1e-3, tail_u, tail_v)[0]) <= TOL


@pytest.mark.parametrize("variant", ["dirichlet", "bounds", "freeslip"])
def test_rk_step_bit_identical(T, monkeypatch, variant):
    """begin_step + three substeps, one scalar, Dirichlet walls, 512 x 16 x 8: the overwriting and the accumulating fused Burgers launch with the
    scalar's finishing epilogue and the x term of the pressure forcing, the operand-sum derivative and the launch that finishes u; with bounds the
    CLIP instantiation; with free-slip walls and Neumann scalars the launch that finishes u takes its wall planes from given tendencies.
    q, s, hq, hs must not differ in a bit between the two settings."""
    import torch
    from tlab_amd.dns import Dns, RKM_EXP3
    ny, nz = 16, 8
    x, y, z = grids(NX, ny, nz, True)
    q0, s0 = init_fields(NX, ny, nz, x, y, z, 23)
    d = Dns(x, y, z, nscal=1, visc=1.0 / 800.0, schmidt=(0.7,), yuniform=False, rkm_mode=RKM_EXP3)
    if variant == "bounds":
        d.set_scalar_bounds([-0.2], [0.6], [1])       # the scalar spans about [-1.1, 1.1]: both ends bind
    if variant == "freeslip":
        d.set_bcs("freeslip", "freeslip", "neumann", "neumann")

    def step():
        for i in range(3):
            d.q[i].copy_(torch.from_numpy(q0[i]))
        d.s[0].copy_(torch.from_numpy(s0[0]))
        d.TIME_RUNGEKUTTA(2e-3)
        return [t.clone() for t in d.q + d.s + d.hq + d.hs]
    monkeypatch.delenv("TLAB_XLINE_STAGE", raising=False)
    out = {}
    names = _profiled(lambda: out.__setitem__("staged", step()))
    assert {"k_xline<BURGERS>", "k_xline<P1>"} <= names and not {"k_xline<BURGERS,direct>", "k_xline<P1,direct>"} & names, names
    monkeypatch.setenv("TLAB_XLINE_STAGE", "0")
    names = _profiled(lambda: out.__setitem__("direct", step()))
    assert {"k_xline<BURGERS,direct>", "k_xline<P1,direct>"} <= names and not {"k_xline<BURGERS>", "k_xline<P1>"} & names, names
    monkeypatch.delenv("TLAB_XLINE_STAGE")
    for k, (a, b) in enumerate(zip(out["staged"], out["direct"])):
        assert bool(torch.isfinite(a).all()), k
        assert torch.equal(a, b), k
    if variant == "bounds":
        s = out["staged"][3]
        assert bool((s == -0.2).any()) and bool((s == 0.6).any())       # the clip fired at both ends
