"""Scalar bounds limiting ([Control] ScalLimit; DNS_BOUNDS_LIMIT, dns_local.f90:67-90, called after the update of every substep, time.f90:248-250)
inside the device substep: tlab_dns_set_scalar_bounds and its slab / pencil forms against an oracle that clips after its update."""
import numpy as np
import pytest
from conftest import rel_err
from scatter import substep_scatter, bound
from cases import grids, init_fields

pytestmark = pytest.mark.gpu

LO, HI, ACTIVE = [0.1, -1.0, -0.2], [0.9, 1.0, 0.3], [1, 0, 1]


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def _oracle_class():
    from oracle.tlab_oracle_rhs import DnsOracle

    class BoundedOracle(DnsOracle):
        """time_substep of the oracle + DNS_BOUNDS_LIMIT after the update: s = min(max(s, lo), hi) for the active scalars."""
        bounds = None

        def time_substep(self, dte, kco=1.0, scale=False):
            self.rhs_global_incompressible_1(dte)
            for i in range(3):
                self.q[i] = self.q[i] + dte * self.hq[i]
            for i in range(self.nscal):
                self.s[i] = self.s[i] + dte * self.hs[i]
            if self.bounds is not None:
                lo, hi, act = self.bounds
                for i in range(len(act)):
                    if act[i]:
                        self.s[i] = np.minimum(np.maximum(self.s[i], lo[i]), hi[i])
            if scale:
                for i in range(3):
                    self.hq[i] = kco * self.hq[i]
                for i in range(self.nscal):
                    self.hs[i] = kco * self.hs[i]
    return BoundedOracle


def _case(nx=256, ny=32, nz=16):
    x, y, z = grids(nx, ny, nz, True)
    q0, s0 = init_fields(nx, ny, nz, x, y, z, 31)
    s = s0[0]
    return x, y, z, q0, [s, 0.5 * s + 0.3, -0.6 * s]      # scalar 1 within ~[-1.1, 1.1], scalar 3 within ~[-0.7, 0.7]: both bounds bind


def _load(d, q0, s0):
    import torch
    for i in range(3):
        d.q[i].copy_(torch.from_numpy(q0[i]))
    for i, a in enumerate(s0):
        d.s[i].copy_(torch.from_numpy(a))


def _schedule(d, dtime):
    n = d.rkm_endstep
    return [(dtime * d.kdt[k], d.kco[k] if k < n - 1 else 1.0, k < n - 1, k == 0) for k in range(n)]


ROUTES = ["fused_dirichlet", "fused_neumann", "surface", "literal"]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("mode", ["exp3", "exp4"])
def test_bounded_rk_step_against_the_oracle(T, route, mode):
    from tlab_amd.dns import Dns, RKM_EXP3, RKM_EXP4, scalar_bcs
    x, y, z, q0, s0 = _case()
    visc, sc = 1.0 / 800.0, (0.7, 1.0, 1.3)
    d = Dns(x, y, z, nscal=3, visc=visc, schmidt=sc, yuniform=False, rkm_mode=RKM_EXP3 if mode == "exp3" else RKM_EXP4)
    Oracle = _oracle_class()
    setup = []
    if route == "fused_neumann":
        d.set_bcs("noslip", "noslip", "neumann", "neumann")
        setup.append(lambda o: (setattr(o, "scal_jmin", [scalar_bcs("neumann")] * 3), setattr(o, "scal_jmax", [scalar_bcs("neumann")] * 3)))
    elif route == "surface":
        d.set_surface_bcs(["linear"] * 3, ["static"] * 3, [0.35] * 3, [0.0] * 3)
        setup.append(lambda o: (setattr(o, "sfc_jmin", [1] * 3), setattr(o, "cpl_jmin", [0.35] * 3)))
    elif route == "literal":
        d.set_fusion(False)
    d.set_scalar_bounds(LO, HI, ACTIVE)
    _load(d, q0, s0)
    sched = _schedule(d, 2e-3)

    def make(bounds):
        def mk():
            o = Oracle(x, y, z, nscal=3, visc=visc, schmidt=sc, yuniform=False, hyper_bc1_ext=0.0)
            o.bounds = bounds
            for f in setup:
                f(o)
            return o
        return mk
    B, S = substep_scatter(make((LO, HI, ACTIVE)), q0, s0, sched, nsamples=3)
    Bu, _ = substep_scatter(make(None), q0, s0, sched, nsamples=0)
    d.TIME_RUNGEKUTTA(2e-3)
    k = len(sched) - 1
    for name in ("q", "s", "hq", "hs"):
        for i, (b, scat) in enumerate(zip(B[k][name], S[k][name])):
            e = rel_err(getattr(d, name)[i].cpu().numpy(), b)
            assert e <= bound(scat), (route, mode, name, i, "err %.2e" % e)
    for i in (0, 2):
        s = d.s[i].cpu().numpy()
        assert s.min() >= LO[i] and s.max() <= HI[i]
        assert (s == LO[i]).any() and (s == HI[i]).any()                      # the clip fired at both ends
        su = Bu[k]["s"][i]
        assert su.min() < LO[i] and su.max() > HI[i]                          # ... where the unclipped run leaves the interval


@pytest.mark.parametrize("route", ["fused_dirichlet", "fused_neumann", "literal"])
def test_bounds_that_never_bind_change_nothing(T, route):
    """Bounds far outside the fields: the bounded kernels give the unbounded results bit for bit, and after set_scalar_bounds(None) the plain ones."""
    import torch
    from tlab_amd.dns import Dns
    x, y, z, q0, s0 = _case()
    d = Dns(x, y, z, nscal=3, visc=1.0 / 800.0, schmidt=(0.7, 1.0, 1.3), yuniform=False)
    if route == "fused_neumann":
        d.set_bcs("noslip", "noslip", "neumann", "neumann")
    if route == "literal":
        d.set_fusion(False)

    def step():
        _load(d, q0, s0)
        d.TIME_RUNGEKUTTA(2e-3)
        torch.cuda.synchronize()
        return [t.clone() for t in d.q + d.s + d.hq + d.hs]
    plain = step()
    d.set_scalar_bounds([-1e3] * 3, [1e3] * 3)
    wide = step()
    d.set_scalar_bounds(None)
    again = step()
    for a, b, c in zip(plain, wide, again):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_refusals(T):
    from tlab_amd.dns import Dns
    x, y, z, q0, s0 = _case(64, 16, 8)
    d = Dns(x, y, z, nscal=2, visc=1.0 / 800.0, schmidt=(0.7, 1.0), yuniform=False)
    for lo, hi in (([0.5, 0.0], [0.4, 1.0]), ([float("nan"), 0.0], [1.0, 1.0]), ([0.0, 0.0], [1.0, float("nan")]), ([0.0] * 3, [1.0] * 3)):
        with pytest.raises(T.TlabError):
            d.set_scalar_bounds(lo, hi)
    d.set_scalar_bounds([0.5, 0.0], [0.4, 1.0], active=[0, 1])         # an inactive scalar's bounds are not looked at
    from tlab_amd.lib import load
    import torch
    a = torch.zeros(8, dtype=torch.float64, device="cuda")
    assert load().tlab_pw_clip(a.data_ptr(), 1.0, 0.0, 8) != 0


@pytest.mark.parametrize("bcs", ["dirichlet", "neumann"])
def test_decomposed_drivers_with_bounds_equal_the_single_domain(T, bcs):
    """Loopback z-slabs (P = 2, 4) and 2 x 2 loopback pencils with bounds equal the single domain within the bound of test_gpu_slab_native.py
    (the one-ulp scatter of the bounded oracle)."""
    import torch
    from tlab_amd.dns import Dns, scalar_bcs
    from tlab_amd.slab import NativeSlabDns
    from tlab_amd.pencil import NativePencilDns
    nx, ny, nz = 128, 24, 256          # slabs of 64 / 128 planes (thinner ones take the K-transposition scheme), pencils of 64 x 128 columns
    x, y, z, q0, s0 = _case(nx, ny, nz)
    kw = dict(nscal=3, visc=1.0 / 800.0, schmidt=(0.7, 1.0, 1.3), yuniform=False)
    d = Dns(x, y, z, **kw)
    d.set_bcs("noslip", "noslip", bcs, bcs)
    d.set_scalar_bounds(LO, HI, ACTIVE)
    _load(d, q0, s0)
    d.TIME_RUNGEKUTTA(2e-3)
    one = {"q": [t.clone() for t in d.q], "s": [t.clone() for t in d.s]}
    Oracle = _oracle_class()

    def make():
        o = Oracle(x, y, z, hyper_bc1_ext=0.0, **kw)
        o.bounds = (LO, HI, ACTIVE)
        o.scal_jmin = o.scal_jmax = [scalar_bcs(bcs)] * 3
        return o
    sched = [(2e-3 * d.kdt[k], d.kco[k] if k < 2 else 1.0, k < 2, k == 0) for k in range(3)]
    _, S = substep_scatter(make, q0, s0, sched, nsamples=2)
    del d
    drivers = [("slab%d" % P, NativeSlabDns("loopback", x, y, z, size=P, **kw)) for P in (2, 4)]
    drivers.append(("pencil2x2", NativePencilDns("loopback", 2, 2, x, y, z, **kw)))
    for tag, m in drivers:
        m.set_bcs("noslip", "noslip", bcs, bcs)
        m.set_scalar_bounds(LO, HI, ACTIVE)
        for i in range(3):
            m.scatter("q", i, torch.from_numpy(q0[i]).cuda())
            m.scatter("s", i, torch.from_numpy(s0[i]).cuda())
        for k in range(m.rkm_endstep):
            m.substep_of_cycle(k, 2e-3)
        torch.cuda.synchronize()
        for name in ("q", "s"):
            for i, rf in enumerate(one[name]):
                got = _gather(m, name, i, nx, ny, nz)
                err = float((got - rf).abs().max() / rf.abs().max())
                assert err <= bound(S[2][name][i]), (tag, name, i, err)
                if name == "s" and ACTIVE[i]:
                    assert float(got.min()) >= LO[i] and float(got.max()) <= HI[i] and bool((got == LO[i]).any())
        m.close()


def _gather(m, name, i, nx, ny, nz):
    import torch
    if not hasattr(m, "pro"):
        return torch.cat([m.st[r][name][i] for r in m.local_ranks])
    out = torch.empty(nz, ny, nx, dtype=torch.float64, device="cuda")
    for r, t in m.gather_local(name, i).items():
        pi, pk = m.pro(r)
        out[pk * m.kmax:(pk + 1) * m.kmax, :, pi * m.imax:(pi + 1) * m.imax] = t.view(m.kmax, ny, m.imax)
    return out.reshape(-1)
