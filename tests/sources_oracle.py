"""The oracle with the body forces of the reference: Rotation_Coriolis (src/physics/rotation.f90:103-143) and Gravity_Buoyancy
(src/physics/gravity.f90:232-342) restated in their operation order, and TLab_Sources_Flow (src/physics/tlab_sources.f90:36-92, non-BLAS branch)
called before the RHS as TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT does (tools/dns/time.f90:610-612).  TEST INFRASTRUCTURE (numpy only: numpy never
fuses a multiply with an add, so these are the reference's roundings).

tests/test_sources_host.py pins it: without forces it is BufferOracle bit for bit, with forces three points per type are checked by hand."""
import math

import numpy as np

from buffer_oracle import BufferOracle

EQNS_COR_NONE, EQNS_COR_EXPLICIT, EQNS_COR_NORMALIZED = 0, 4, 12
EQNS_BOD_NONE, EQNS_BOD_EXPLICIT, EQNS_BOD_HOMOGENEOUS, EQNS_BOD_LINEAR, EQNS_BOD_BILINEAR, EQNS_BOD_QUADRATIC = 0, 4, 5, 6, 7, 8
EQNS_BOD_NORMALIZEDMEAN, EQNS_BOD_SUBTRACTMEAN = 9, 10
SMALL_WP = 1.0e-20


def coriolis(type, vector, parameters, q, hq):
    """Rotation_Coriolis :118-141, in place on the list hq (r) from the list q (u); vector already holds the Rossby number"""
    f1, f2, f3 = (float(v) for v in vector)
    u, v, w = q[0], q[1], q[2]
    if type == EQNS_COR_EXPLICIT:
        hq[0] = hq[0] + f3 * v - f2 * w
        hq[1] = hq[1] + f1 * w - f3 * u
        hq[2] = hq[2] + f2 * u - f1 * v
    elif type == EQNS_COR_NORMALIZED:
        geo_u = math.cos(parameters[0]) * parameters[1]
        geo_w = -math.sin(parameters[0]) * parameters[1]
        hq[0] = hq[0] + f2 * (geo_w - w)
        hq[2] = hq[2] + f2 * (u - geo_u)


def buoyancy(type, nscalars, parameters, inb_scal_array, s, ref, nx, ny, nz):
    """Gravity_Buoyancy :244-339: b, flat (nz ny nx), from the list s; parameters: the list as the ini file gives it (missing entries are zero);
    ref: bbackground (ny values).  nscalars = locProps%scalar(1)."""
    par = [float(v) for v in parameters] + [0.0] * 16
    r = np.asarray(ref, dtype=np.float64).reshape(1, ny, 1)
    S = [np.asarray(a).reshape(nz, ny, nx) for a in s]
    if type == EQNS_BOD_HOMOGENEOUS:
        b = np.full((nz, ny, nx), par[0])
    elif type == EQNS_BOD_LINEAR:
        c1, c2, c3, c0 = par[0], par[1], par[2], par[inb_scal_array]
        if nscalars == 1:
            b = c1 * S[0] - (r - c0)
        elif nscalars == 2:
            b = c1 * S[0] + c2 * S[1] - (r - c0)
        elif nscalars == 3:
            b = c1 * S[0] + c2 * S[1] + c3 * S[2] - (r - c0)
        else:
            b = np.zeros((nz, ny, nx)) + (c0 - r)
            for i in range(nscalars):
                if abs(par[i]) > SMALL_WP:
                    b = b + par[i] * S[i]
    elif type == EQNS_BOD_BILINEAR:
        c0, c1, c2 = par[0], par[1], par[2]
        b = c0 * S[0] + c1 * S[1] + c2 * S[0] * S[1] - r
    elif type == EQNS_BOD_QUADRATIC:
        c0 = -par[0] / (par[1] / 2.0) ** 2
        c1 = par[1]
        b = c0 * S[0] * (S[0] - c1) - r
    else:
        raise ValueError("buoyancy type %r is not restated here" % (type,))
    return b.reshape(-1)


def sources_flow(cor, bod, q, s, hq, nx, ny, nz):
    """TLab_Sources_Flow :54-92 in place on the list hq.  cor = (type, vector, parameters) or None; bod = (type, vector, nscalars, parameters,
    inb_scal_array, bbackground or None) or None"""
    if cor is not None and cor[0] != EQNS_COR_NONE:
        coriolis(cor[0], cor[1], cor[2], q, hq)
    if bod is not None and bod[0] != EQNS_BOD_NONE:
        type, vector, nscalars, parameters, inb, ref = bod
        ref = np.zeros(ny) if ref is None else ref
        for iq in range(3):
            if abs(float(vector[iq])) > 0.0:                       # buoyancy%active(iq), gravity.f90:92-94
                b = buoyancy(type, nscalars, parameters, inb, s, ref, nx, ny, nz)
                hq[iq] = hq[iq] + float(vector[iq]) * b


class SourcesOracle(BufferOracle):
    """BufferOracle + [Rotation] and [BodyForce]: time_substep adds the forces to hq before the RHS, which accumulates onto hq"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.coriolis = None
        self.buoyancy = None

    def set_body_forces(self, coriolis=None, buoyancy=None):
        self.coriolis, self.buoyancy = coriolis, buoyancy

    def sources_flow(self):
        sources_flow(self.coriolis, self.buoyancy, self.q, self.s, self.hq, self.nx, self.ny, self.nz)

    def time_substep(self, dte, kco=1.0, scale=False):
        self.sources_flow()                                                                                          # time.f90:610
        super().time_substep(dte, kco, scale)                                                                        # :612 ...
