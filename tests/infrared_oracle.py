"""The oracle with the cloud-top physics of the reference: THERMO_AIRWATER_LINEAR (src/thermodynamics/thermo_airwater.f90:483-516), which
FI_DIAGNOSTIC calls for the diagnostic liquid (physics/fi_diagnostic.f90:44-47); Radiation_Infrared_Y, TYPE_IR_GRAY_LIQUID (physics/radiation.f90:
265-283) with IR_RTE1_OnlyLiquid (:401-444); TLab_Sources_Scal (physics/tlab_sources.f90:152-168), called before the RHS as
TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT does (tools/dns/time.f90:611), and FI_DIAGNOSTIC after the update (:248).  TEST INFRASTRUCTURE (numpy only:
numpy never fuses a multiply with an add, so these are the reference's roundings).

The first-order integral is the restatement oracle/tlab_oracle_poisson.py::int1_initialize / int1_solve, which tests/golden/infrared_tau.npz pins to
the reference's own compiled FDM_Int1_Solve (tests/test_infrared_host.py).  THERMO_AIRWATER_LINEAR and the exp / product lines are not reachable
through oracle/ref_lib.py: they are pinned by restatement only."""
import numpy as np

from oracle import tlab_oracle_poisson as OP
from oracle.tlab_oracle import BCS_MAX
from sources_oracle import SourcesOracle, SMALL_WP

MIXT_TYPE_NONE, MIXT_TYPE_AIRWATER_LINEAR = 0, 12
TYPE_IR_NONE, TYPE_IR_GRAY_LIQUID = 0, 1


def airwater_linear(params, s):
    """THERMO_AIRWATER_LINEAR: the normalized liquid from the list s of prognostic scalars (inb_scal = len(s)); params = thermo_param"""
    p = [float(v) for v in params]
    ns = len(s)
    if ns == 1:
        xi = 1.0 + p[0] * s[0]
    else:
        xi = 1.0 + p[0] * s[0] + p[1] * s[1]
    if abs(p[ns]) < SMALL_WP:
        return np.maximum(xi, 0.0)
    dummy = p[ns]
    dummy2 = 1.0 / dummy
    return dummy * np.log(np.exp(dummy2 * xi) + 1.0)


_PLANS = {}


def int0_max(gy):
    """fdm_Int0(BCS_MAX) of the y plan: FDM_Int1_Initialize(nodes, der1, lambda = 0, BCS_MAX), made once per plan"""
    if id(gy) not in _PLANS:
        _PLANS[id(gy)] = (gy, OP.int1_initialize(gy.der1, 0.0, BCS_MAX))
    return _PLANS[id(gy)][1]


def optical_depth(gy, a, nx, ny, nz):
    """p_tau of IR_RTE1_OnlyLiquid :416-417: FDM_Int1_Solve of the absorption a (flat, nz ny nx) with tau(ny) = 0 -- minus the integral from y to the
    top.  Returns (nz, ny, nx)."""
    p = int0_max(gy)
    f = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(nz, ny, nx).transpose(1, 0, 2)).reshape(ny, nz * nx, 1)
    res = np.zeros_like(f)                                      # res[ny-1] = 0: the boundary condition
    OP.int1_solve(p, p.rhs, f, res)
    return res.reshape(ny, nz, nx).transpose(1, 0, 2)


def infrared_gray_liquid(gy, kappa, ft, fb, liquid, nx, ny, nz):
    """Radiation_Infrared_Y, TYPE_IR_GRAY_LIQUID: the source, flat (nz ny nx)"""
    a = (float(kappa) * np.asarray(liquid, dtype=np.float64)).reshape(nz, ny, nx)
    f = np.exp(optical_depth(gy, a, nx, ny, nz))
    if abs(float(fb)) > 0.0:
        src = a * (f * float(ft) + f[:, 0:1, :] / f * float(fb))
    else:
        src = a * f * float(ft)
    return src.reshape(-1)


def sources_scal(gy, ir, s_all, hs, nx, ny, nz):
    """TLab_Sources_Scal in place on the list hs.  ir = (type, scalar (1-based), kappa, flux_top, flux_bottom) or None; s_all: the scalars and,
    last, the liquid (infraredProps%scalar(1) = inb_scal_array)"""
    if ir is None or ir[0] == TYPE_IR_NONE:
        return
    type, scalar, kappa, ft, fb = ir
    if type != TYPE_IR_GRAY_LIQUID:
        raise ValueError("infrared type %r is not restated here" % (type,))
    hs[scalar - 1] = hs[scalar - 1] + infrared_gray_liquid(gy, kappa, ft, fb, s_all[-1], nx, ny, nz)


class CloudOracle(SourcesOracle):
    """SourcesOracle + the diagnostic liquid and the infrared source: time_substep adds the flow and the scalar sources before the RHS and
    recomputes the liquid after the update; the buoyancy sees s + [liquid]"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.mixture = None                 # thermo_param of AirWaterLinear, or None
        self.infrared = None
        self.liquid = None

    def set_mixture(self, params):
        self.mixture = None if params is None else [float(v) for v in params]
        self.liquid = None

    def set_infrared(self, type, scalar, kappa, flux_top, flux_bottom):
        self.infrared = (type, scalar, kappa, flux_top, flux_bottom)

    def fi_diagnostic(self):
        if self.mixture is not None:
            self.liquid = airwater_linear(self.mixture, self.s)

    def s_all(self):
        if self.mixture is None:
            return self.s
        if self.liquid is None:             # the caller's FI_DIAGNOSTIC before the first substep
            self.fi_diagnostic()
        return self.s + [self.liquid]

    def sources_flow(self):
        from sources_oracle import sources_flow
        sources_flow(self.coriolis, self.buoyancy, self.q, self.s_all(), self.hq, self.nx, self.ny, self.nz)

    def sources_scal(self):
        if self.mixture is not None:
            sources_scal(self.g[1], self.infrared, self.s_all(), self.hs, self.nx, self.ny, self.nz)

    def time_substep(self, dte, kco=1.0, scale=False):
        self.sources_flow()                                                                                          # time.f90:610
        self.sources_scal()                                                                                          # :611
        super(SourcesOracle, self).time_substep(dte, kco, scale)                                                     # :612 ...
        self.fi_diagnostic()                                                                                         # :248
