"""Phase averages, towers, saved planes and the pressure sampling of the last substep on the device (csrc/sampling.hip, the taps of csrc/rhs.cpp):
the cases of tests/test_sampling_host.py on device arrays with the same bitwise assertions against tests/sampling_oracle.py, the 8-byte path of
k_phase_space and a k-unroll with a remainder, FI_GRADIENT bitwise, log10(a + small_wp) within 4 ulp of numpy's -- the HIP math API documents 1 ulp
for the double log10, the GNU libc manual 2 ulp for x86_64; their sum plus one --, an armed Runge-Kutta step against an unarmed one in three
configurations, and Dns.PLANES_SAVE."""
import ctypes

import numpy as np
import pytest

import cases as K
import sampling_cases as C
import sampling_oracle as S
from launch_census import REF_HYPER

pytestmark = pytest.mark.gpu

BOX = (16, 12, 8)
VISC, SC, DT = 1.0 / 800.0, (0.7,), 2.0e-3
ptr = lambda a: a.data_ptr()       # noqa: E731


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


@pytest.fixture(scope="module")
def L(T):
    return T.load()


def put(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()


def put_odd(a):
    """a device copy that starts 8 bytes behind a 16-byte boundary: the 8-byte accesses of k_phase_space"""
    import torch
    a = np.asarray(a, dtype=np.float64)
    t = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[1:].view(a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return v


def get(t):
    return t.cpu().numpy()


# ---- the cases of the host tests ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.PHASE_BOXES)
def test_phase_averages_equal_the_restatement_bit_for_bit(T, shape):
    C.check_phase(T, shape, put, get)


def test_phase_averages_on_arrays_offset_by_8_bytes(T):
    """(130, 6, 19): 780 points a plane -- seven workgroups of 128 --, nz = 19 = 4 * 4 + 3 = 2 * 8 + 3: the unrolled loops leave a remainder"""
    C.check_phase(T, (130, 6, 19), put_odd, get)


def test_phase_refusals_leave_the_accumulator_untouched(T, L):
    C.check_phase_refusals(L, put, get, ptr)
    a, avg = put(np.ones((3, 4, 6))), np.zeros((1, 2, 4, 6))
    one = (C.vp * 1)(a.data_ptr())
    assert L.tlab_avg_phase_space(6, 4, 3, 3, 1, one, 1, 1, C.vp(avg.ctypes.data)) == C.EINVAL      # a device field, a host accumulator
    assert b"host and device" in L.tlab_last_error()


@pytest.mark.parametrize("shape,stride", C.TOWER_CASES)
@pytest.mark.parametrize("exact", [True, False])
def test_towers_equal_the_restatement(T, shape, stride, exact):
    C.check_towers(T, shape, stride, put, get, exact)


def test_tower_refusals(T, L):
    C.check_tower_refusals(T, L, put, get)


@pytest.mark.parametrize("shape", [(20, 12, 8), (7, 5, 3), (6, 4, 1)])
def test_planes_in_the_three_directions(T, L, shape):
    C.check_planes(T, L, shape, put, get, ptr)


# ---- PLANES_LOG's pointwise passes ----------------------------------------------------------------------------------------------------------
def _driver(T, stagger=False, pfilter=False, keep=None):
    import torch
    from tlab_amd.dns import Dns
    nx, ny, nz = BOX
    x, y, z = K.grids(nx, ny, nz, True)
    q0, s0 = K.init_fields(nx, ny, nz, x, y, z, 3)
    d = Dns(x, y, z, nscal=1, visc=VISC, schmidt=SC, yuniform=False, hyper_bc1_ext=REF_HYPER, stagger=stagger)
    if pfilter:
        keep.append(T.Filter(2, ny, False, None, 1, 1))      # [PressureFilter] along y: explicit6, biased at the walls
        d.set_pressure_filter(None, keep[-1], None)
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(np.array(q0[i])))
    d.s[0].copy_(torch.from_numpy(np.array(s0[0])))
    return d


def test_fi_gradient_is_the_reference_statement_on_the_device_derivatives(T):
    import torch
    d = _driver(T)
    nx, ny, nz = BOX
    der = [torch.empty_like(d.s[0]) for _ in range(3)]
    for i, opr in enumerate((T.OPR_Partial_X, T.OPR_Partial_Y, T.OPR_Partial_Z)):
        opr(T.OPR_P1, nx, ny, nz, 0, d.g[i], d.s[0], der[i])
    want = S.fi_gradient(*[get(t) for t in der])
    got = get(T.fi_gradient(d, d.s[0], torch.empty_like(d.s[0]), torch.empty_like(d.s[0])))
    assert np.abs(want).max() > 0.0 and np.array_equal(got, want)


def test_log10_small_within_four_ulp_of_numpy(T):
    rng = np.random.default_rng(7)
    a = np.concatenate([[0.0, 1.0e-20, 1.0, 10.0, 1.0e10], 10.0 ** rng.uniform(-25, 12, 4091), rng.uniform(0.5, 2.0, 4096)])      # 8192 values, around 1 too
    want = np.log10(a + 1.0e-20)
    got = get(T.log10_small(put(a)))
    ulps = np.abs(got - want) / np.spacing(np.abs(want))
    print("log10_small: worst distance to numpy %.2f ulp of the result" % ulps.max())
    assert np.all(ulps <= 4.0), float(ulps.max())


# ---- the pressure of the last substep ---------------------------------------------------------------------------------------------------------
def _copy_state(src, dst):
    for a, b in zip(src.q + src.s + src.hq + src.hs, dst.q + dst.s + dst.hq + dst.hs):
        b.copy_(a)


@pytest.mark.parametrize("form", ["noslip", "pfilter", "stagger"])
def test_an_armed_step_samples_the_pressure_of_its_last_substep(T, form):
    import torch
    nx, ny, nz = BOX
    keep = []
    a, b, c = (_driver(T, stagger=form == "stagger", pfilter=form == "pfilter", keep=keep) for _ in range(3))
    a.set_towers((4, 1, 2), 2)
    a.set_phase_average(2, 0, 4)                        # avg_planes = 2; step 3 samples at (3 + 1) / 2 = 2: plane mod((2 - 1) - 0, 2) + 1 = 2
    a.TIME_RUNGEKUTTA(DT, itime=3, rtime=0.375)
    # the same step unarmed; the last substep's pressure from the RHS on a copy of the state in front of it
    b.begin_step()
    for k in range(b.rkm_endstep - 1):
        b.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(DT * b.kdt[k], b.kco[k], True)
    _copy_state(b, c)
    last = b.rkm_endstep - 1
    c.RHS_GLOBAL_INCOMPRESSIBLE_1(DT * c.kdt[last])
    p = c.txc[0][: c.n].clone()
    if form == "stagger":                               # back on the velocity nodes (rhs_global_incompressible_1.f90:294-297)
        t5, t4 = torch.empty_like(p), torch.empty_like(p)
        T.OPR_Partial_Z(T.OPR_P0_INT_PV, nx, ny, nz, 0, c.g[2], p, t5)
        T.OPR_Partial_X(T.OPR_P0_INT_PV, nx, ny, nz, 0, c.g[0], t5, t4)
        p = t4
    b.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(DT * b.kdt[last], 1.0, False)
    assert float(p.abs().max()) > 0.0
    for name in ("q", "s", "hq", "hs"):
        for i, (x, y) in enumerate(zip(getattr(a, name), getattr(b, name))):
            assert torch.equal(x, y), (form, name, i)
    # the tower's pressure slot and the phase plane: the stand-alone entry points on that pressure
    ref_t = T.Tower(nx, ny, nz, (4, 1, 2), 2)
    ref_buf = torch.zeros(ref_t.bufsize, dtype=torch.float64, device="cuda")
    ref_t.accumulate(4, [p], 3, 0.375, ref_buf)
    got_buf = a.tower_buffer()
    assert torch.equal(got_buf, ref_buf), form
    v = a.tower.views(get(got_buf))
    assert v["it"][0] == 3.0 and v["t"][0] == 0.375 and np.abs(v["p"][0]).max() > 0.0 and np.all(v["u"] == 0.0)
    assert (a.tower.accumulation, a.tower.mode_check) == (1, 4)
    ref_avg = torch.zeros_like(a.avg_p)
    T.avg_phase_space(nx, ny, nz, [p], 2, 2, ref_avg)
    assert torch.equal(a.phase_buffers()["p"], ref_avg) and float(ref_avg[0, 1].abs().max()) > 0.0 and float(ref_avg[0, 0].abs().max()) == 0.0
    # the arm is gone: another step changes neither buffer; the rest of the step's samples completes the towers' step
    before_t, before_p = got_buf.clone(), a.avg_p.clone()
    a.TIME_RUNGEKUTTA(DT)
    assert torch.equal(a.tower_buffer(), before_t) and torch.equal(a.avg_p, before_p)
    a.tower_accumulate(itime=4, rtime=0.5)
    assert (a.tower.accumulation, a.tower.mode_check) == (2, 0)
    assert a.phase_average(4) and not a.phase_average(5)
    want = torch.zeros_like(a.avg_flow)
    T.avg_phase_space(nx, ny, nz, a.q, 2, 2, want)
    assert torch.equal(a.avg_flow, want)


def test_the_route_that_stops_at_the_pressure_refuses_an_armed_driver(T, L):
    import torch
    from tlab_amd.lib import TlabError
    d = _driver(T)
    avg = torch.zeros((1, 2, BOX[1], BOX[0]), dtype=torch.float64, device="cuda")
    assert L.tlab_dns_arm_pressure_sampling(d._h, None, None, 1, 0.0, avg.data_ptr(), 1, 1) == 0
    with pytest.raises(TlabError, match="armed"):
        d.FI_PRESSURE_BOUSSINESQ()
    d.FI_PRESSURE_BOUSSINESQ()                          # the refusal cleared the arm
    assert float(avg.abs().max()) == 0.0
    assert L.tlab_dns_arm_pressure_sampling(d._h, None, None, 1, 0.0, avg.data_ptr(), 1, 2) == C.EINVAL      # plane_id past avg_planes
    host = np.zeros(avg.numel())
    assert L.tlab_dns_arm_pressure_sampling(d._h, None, None, 1, 0.0, C.vp(host.ctypes.data), 1, 1) == C.EINVAL      # a host accumulator


# ---- Dns.PLANES_SAVE --------------------------------------------------------------------------------------------------------------------------
def test_planes_save_layout_and_order(T):
    import torch
    d = _driver(T)
    nx, ny, nz = BOX
    ip, jp, kp = (1, nx), (1, 5, ny), (nz,)
    di, dj, dk = d.PLANES_SAVE(iplanes=ip, jplanes=jp, kplanes=kp, log=True, single=False)
    nvars = 3 + 1 + 1 + 1 + 1                           # u, v, w, s, p, log10 enstrophy, log10 grad s
    assert di.shape == (nz, nvars * 2, ny) and dj.shape == (nz, nvars * 3, nx) and dk.shape == (nvars * 1, ny, nx)
    p = d.FI_PRESSURE_BOUSSINESQ()[: d.n].clone()
    five = d.q + d.s + [p]
    for idir, nodes, got in ((1, ip, di), (2, jp, dj), (3, kp, dk)):
        want = T.planes_gather(nx, ny, nz, five, idir, nodes)
        m = 5 * len(nodes)
        assert torch.equal(got[:m] if idir == 3 else got[:, :m], want), idir
    ens = get(T.log10_small(d.FI_VORTICITY()[: d.n].clone())).reshape(nz, ny, nx)
    assert np.array_equal(get(dk)[5], ens[nz - 1])
    assert np.array_equal(get(dj)[:, 15:18, :], ens[:, [0, 4, ny - 1], :])
    grad = get(T.log10_small(T.fi_gradient(d, d.s[0], torch.empty_like(d.s[0]), torch.empty_like(d.s[0])))).reshape(nz, ny, nx)
    assert np.array_equal(get(di)[:, 12:14, :], np.transpose(grad[:, :, [0, nx - 1]], (0, 2, 1)))
    si, sj, sk = d.PLANES_SAVE(iplanes=ip, log=False)   # single precision by default; an empty list gives None
    assert sj is None and sk is None and si.dtype == torch.float32 and si.shape == (nz, 10, ny)
    assert torch.equal(si, di[:, :10].to(torch.float32))
