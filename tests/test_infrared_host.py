"""The host side of the cloud-top physics, without a GPU: the restated first-order integral behind the infrared source against the reference's own
compiled FDM_Int1_Solve (tests/golden/infrared_tau.npz, made by tests/golden/make_golden_infrared.py through oracle/ref_lib.py), its sign and
boundary rows against an analytic integral, the restated liquid by hand, and the argument checks of the new setters that need no device.

THERMO_AIRWATER_LINEAR and the exp / product lines of IR_RTE1_OnlyLiquid are not reachable through oracle/ref_lib.py: tests/infrared_oracle.py
restates them, and nothing but that restatement pins them."""
import ctypes
import math
import os

import numpy as np

from infrared_oracle import CloudOracle, airwater_linear, infrared_gray_liquid, optical_depth
from oracle import tlab_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "infrared_tau.npz")
EINVAL, EUNSUPPORTED = -1, -2


def test_restated_optical_depth_matches_the_reference():
    g = np.load(GOLDEN)
    n, nlines = int(g["n"]), int(g["nlines"])
    for name, uniform in (("uniform", True), ("stretched", False)):
        y, a, tau = g[name + "_y"], g[name + "_a"], g[name + "_tau"]
        assert a.shape == (n, nlines) and (a >= 0.0).all() and (a == 0.0).any()
        gy = O.FdmPlan(y, False, uniform)
        got = optical_depth(gy, a.T.reshape(-1), 1, n, nlines)[:, :, 0].T          # (nz = nlines, ny, nx = 1) -> (n, nlines)
        e = float(np.abs(got - tau).max() / np.abs(tau).max())
        print("%s: restatement against the reference %.2e" % (name, e))
        assert e <= 1e-13, (name, e)
        assert np.all(tau[n - 1] == 0.0) and np.all(tau[0] < 0.0)


def test_optical_depth_is_minus_the_integral_from_the_top():
    """a sanity bound on the sign and the boundary rows, not a parity bound: 2e-4 measured at 16 points"""
    n = 16
    for uniform in (True, False):
        y = np.arange(n) / (n - 1.0) if uniform else 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(n) / (n - 1) - 1)) / np.tanh(1.5))
        gy = O.FdmPlan(y, False, uniform)
        a = 1.0 + np.sin(2.0 * y)                                                   # integral: y - cos(2 y) / 2
        F = y - 0.5 * np.cos(2.0 * y)
        tau = optical_depth(gy, a, 1, n, 1)[0, :, 0]
        e = float(np.abs(tau - (F - F[-1])).max() / np.abs(F - F[-1]).max())
        print("uniform %s: against the analytic integral %.2e" % (uniform, e))
        assert e <= 1e-3, (uniform, e)


def test_restated_liquid_by_hand():
    s = [np.array([0.5, -0.25, 2.0]), np.array([1.0, 0.5, -1.0])]
    assert np.array_equal(airwater_linear((-1.0, 0.0), s[:1]), np.array([0.5, 1.25, 0.0]))
    assert np.array_equal(airwater_linear((-1.0, 0.5, 0.0), s), np.array([1.0, 1.5, 0.0]))
    d = 0.005625
    got = airwater_linear((-1.0, 0.5, d), s)
    for g, xi in zip(got, (1.0, 1.5, -1.5)):
        assert g == d * math.log(math.exp((1.0 / d) * xi) + 1.0)
    assert abs(got[0] - 1.0) < 1e-15 and 0.0 <= got[2] < 1e-100                     # far from the kink it is max(xi, 0)


def test_source_of_a_uniform_layer():
    """a = const: tau = -a (top - y), source = a exp(tau) flux_top to the accuracy of the scheme; the upward term mirrors it"""
    nx, ny, nz = 2, 33, 1
    y = np.arange(ny) / (ny - 1.0)
    gy = O.FdmPlan(y, False, True)
    liq = np.full(nx * ny * nz, 0.5)
    down = infrared_gray_liquid(gy, 4.0, -3.0, 0.0, liq, nx, ny, nz).reshape(nz, ny, nx)
    want = 2.0 * np.exp(-2.0 * (1.0 - y)) * -3.0
    assert np.abs(down[0, :, 0] - want).max() <= 1e-6 * np.abs(want).max()
    both = infrared_gray_liquid(gy, 4.0, -3.0, 1.5, liq, nx, ny, nz).reshape(nz, ny, nx)
    want = want + 2.0 * np.exp(-2.0 * y) * 1.5
    assert np.abs(both[0, :, 0] - want).max() <= 1e-6 * np.abs(want).max()


def test_oracle_without_cloud_physics_is_the_sources_oracle():
    from sources_oracle import SourcesOracle
    from cases import grids, init_fields
    nx, ny, nz = 16, 12, 8
    x, y, z = grids(nx, ny, nz, True)
    q0, s0 = init_fields(nx, ny, nz, x, y, z, 5)
    bod = (6, (0.0, -2.0, 0.0), 1, (1.0, 0.1), 1, None)
    outs = []
    for cls in (SourcesOracle, CloudOracle):
        o = cls(x, y, z, nscal=1, visc=1e-3, schmidt=(1.0,), yuniform=False, hyper_bc1_ext=0.0)
        o.q, o.s = [a.copy() for a in q0], [a.copy() for a in s0]
        o.set_body_forces(None, bod)
        o.time_substep(1e-3, -5.0 / 9.0, True)
        outs.append(o.q + o.s + o.hq + o.hs)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_argument_checks_that_need_no_device():
    """the type is checked before the handle, as in tlab_dns_set_buoyancy"""
    from tlab_amd.lib import load
    L = load()
    par = (ctypes.c_double * 3)(-1.2, 0.8, 0.0)
    assert L.tlab_dns_set_mixture(None, 11, par, 3) == EUNSUPPORTED                # MIXT_TYPE_AIRWATER
    assert L.tlab_dns_set_mixture(None, 5, par, 3) == EUNSUPPORTED
    assert L.tlab_dns_set_mixture(None, 12, par, 3) == EINVAL                      # a supported mixture and no driver
    assert L.tlab_dns_set_mixture(None, 0, None, 0) == EINVAL
    assert L.tlab_dns_set_infrared(None, 2, 1, 1.0, 1.0, 0.0) == EUNSUPPORTED      # gray
    assert L.tlab_dns_set_infrared(None, 3, 1, 1.0, 1.0, 0.0) == EUNSUPPORTED      # band
    assert L.tlab_dns_set_infrared(None, 7, 1, 1.0, 1.0, 0.0) == EINVAL
    assert L.tlab_dns_set_infrared(None, 1, 1, 1.0, 1.0, 0.0) == EINVAL
    assert len(L.tlab_last_error()) > 0
    assert L.tlab_dns_info(None, 5) == -1
    for name in ("tlab_dns_diagnostic", "tlab_dns_sources_scal"):
        assert getattr(L, name)(*([None] * len(getattr(L, name).argtypes))) < 0     # refused, not run
