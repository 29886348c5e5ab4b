"""The oracle with the sponge layer of [BufferZone] Type = relaxation (tools/dns/boundary_buffer.f90): DnsOracle's rhs_global_incompressible_1 and
time_substep restated with BOUNDARY_BUFFER_RELAX_FLOW (rhs_global_incompressible_1.f90:170-172, between the last Burgers sum and the pressure
forcing) and BOUNDARY_BUFFER_RELAX_SCAL (time.f90:628-630, after the RHS and before the update) in the reference's places, plus INI_BLOCK's
construction of tau (:359-371) and ref (:291-333, LoadBuffer = no, temporal mode) for the J zones.  TEST INFRASTRUCTURE (numpy only).

tests/test_buffer_host.py pins it: without zones it is DnsOracle bit for bit, with zones three planes are checked by hand."""
import numpy as np

from oracle import tlab_oracle as O
from oracle import tlab_oracle_poisson as OP
from oracle.tlab_oracle_rhs import DnsOracle

FORM_POWER_MIN, FORM_POWER_MAX = 1, 2


def buffer_tau(nodes, offset, size, strength, sigma, form):
    """INI_BLOCK :359-371: tau(jloc, iq), shape (size, nfields) -- in the reference's operation order ((y - y0) * (1 / L)) ** sigma"""
    nodes = np.asarray(nodes, dtype=np.float64)
    strength, sigma = np.atleast_1d(strength).astype(np.float64), np.atleast_1d(sigma).astype(np.float64)
    tau = np.zeros((size, len(strength)))
    dummy = 1.0 / (nodes[offset + size - 1] - nodes[offset])
    for iq in range(len(strength)):
        for jloc in range(size):
            j = offset + jloc
            d = (nodes[j] - nodes[offset]) if form == FORM_POWER_MAX else (nodes[offset + size - 1] - nodes[j])
            tau[jloc, iq] = strength[iq] * float(d * dummy) ** sigma[iq]
    return tau


def read_block(params, nfields):
    """BOUNDARY_BUFFER_READBLOCK :108-121: Parameters<tag> -> (strength(:), sigma(:)) from 1, 2 or nfields + 1 values"""
    p = [float(v) for v in np.atleast_1d(params)]
    if len(p) == 1:
        return [p[0]] * nfields, [2.0] * nfields
    if len(p) == 2:
        return [p[0]] * nfields, [p[1]] * nfields
    if len(p) == nfields + 1:
        return p[:nfields], [p[nfields]] * nfields
    raise ValueError("BufferZone.Parameters: 1, 2 or nfields + 1 values")


def plane_mean(a3, j):
    """COV2V2D(.., j, rho = 1, a) (utils/averages.f90:244-267): serial sum with i fastest, then k, of the plane j (times 1.0), / (nx nz)"""
    return float(np.cumsum(np.ascontiguousarray(a3[:, j, :]).ravel())[-1]) / float(a3.shape[0] * a3.shape[2])


def buffer_ref(fields, nx, ny, nz, offset, size, hard=None):
    """INI_BLOCK :307-315: ref(:, jloc, :, iq) = the plane mean of field iq at j = offset + jloc, or HardValues(iq); shape (nfields, nz, size, nx)"""
    ref = np.zeros((len(fields), nz, size, nx))
    for iq, a in enumerate(fields):
        a3 = np.asarray(a).reshape(nz, ny, nx)
        for jloc in range(size):
            ref[iq, :, jloc, :] = plane_mean(a3, offset + jloc) if hard is None else float(hard[iq])
    return ref


class Block:
    """buffer_dt of one J zone: offset (0-based first plane), size, tau (size, nfields), ref (nfields, nz, size, nx)"""

    def __init__(self, offset, size, tau, ref):
        self.offset, self.size, self.tau, self.ref = int(offset), int(size), np.asarray(tau), np.asarray(ref)


def relax_block(item, a, h, nx, ny, nz):
    """RELAX_BLOCK :479-485 (idir = 2), in place on the list h: h(:, j, :, iq) -= tau(jloc, iq) * (a(:, j, :, iq) - ref(:, jloc, :, iq))"""
    for iq in range(len(h)):
        a3, h3 = a[iq].reshape(nz, ny, nx), h[iq].reshape(nz, ny, nx)
        for jloc in range(item.size):
            j = item.offset + jloc
            h3[:, j, :] = h3[:, j, :] - item.tau[jloc, iq] * (a3[:, j, :] - item.ref[iq, :, jloc, :])


class BufferOracle(DnsOracle):
    """DnsOracle + BuffFlowJmin / BuffFlowJmax / BuffScalJmin / BuffScalJmax (None: size 0)"""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.buff_flow = [None, None]      # Jmin, Jmax
        self.buff_scal = [None, None]

    def set_buffer_zones(self, points_jmin=0, points_jmax=0, params_u=(1.0, 2.0), params_s=(1.0, 2.0), hard_u=None, hard_s=None):
        """BOUNDARY_BUFFER_INITIALIZE for the J zones from the fields the oracle holds NOW (LoadBuffer = no)"""
        nx, ny, nz = self.nx, self.ny, self.nz
        y = self.g[1].nodes
        for end, size, form in ((0, points_jmin, FORM_POWER_MIN), (1, points_jmax, FORM_POWER_MAX)):
            offset = 0 if end == 0 else ny - size
            for group, fields, params, hard in (("flow", self.q, params_u, hard_u), ("scal", self.s, params_s, hard_s)):
                blk = None
                if size > 0 and len(fields) > 0:
                    strength, sigma = read_block(params, len(fields))
                    blk = Block(offset, size, buffer_tau(y, offset, size, strength, sigma, form), buffer_ref(fields, nx, ny, nz, offset, size, hard))
                (self.buff_flow if group == "flow" else self.buff_scal)[end] = blk

    def buffer_relax_flow(self):
        for item in self.buff_flow:            # Jmin before Jmax (:452-455)
            if item is not None:
                relax_block(item, self.q, self.hq, self.nx, self.ny, self.nz)

    def buffer_relax_scal(self):
        for item in self.buff_scal:
            if item is not None:
                relax_block(item, self.s, self.hs, self.nx, self.ny, self.nz)

    def rhs_global_incompressible_1(self, dte):
        nx, ny, nz = self.nx, self.ny, self.nz
        u, v, w = self.q
        hq, hs = self.hq, self.hs
        nu = self.visc
        sref_b = [hs[i].reshape(nz, ny, nx)[:, 0, :].copy() if self.sfc_jmin[i] == 1 else np.zeros((nz, nx)) for i in range(self.nscal)]
        sref_t = [hs[i].reshape(nz, ny, nx)[:, ny - 1, :].copy() if self.sfc_jmax[i] == 1 else np.zeros((nz, nx)) for i in range(self.nscal)]
        tmp1 = self.burgers(1, nu, u, u); tmp2 = self.burgers(2, nu, v, v); tmp3 = self.burgers(3, nu, w, w)      # :98-100
        tmp7 = self.burgers(2, nu, u, v); tmp8 = self.burgers(3, nu, u, w)                                          # :103-104
        hq[0] = hq[0] + tmp1 + tmp7 + tmp8
        tmp7 = self.burgers(1, nu, v, u); tmp8 = self.burgers(3, nu, v, w)                                          # :115-116
        hq[1] = hq[1] + tmp2 + tmp7 + tmp8
        tmp7 = self.burgers(1, nu, w, u); tmp8 = self.burgers(2, nu, w, v)                                          # :127-128
        hq[2] = hq[2] + tmp3 + tmp7 + tmp8
        for i in range(self.nscal):                                                                                # :149-162
            kap = self.visc / self.schmidt[i]
            t1 = self.burgers(1, kap, self.s[i], u); t2 = self.burgers(2, kap, self.s[i], v); t3 = self.burgers(3, kap, self.s[i], w)
            hs[i] = hs[i] + t1 + t2 + t3
        self.buffer_relax_flow()                                                                                    # :170-172: flow part needs to be projected
        if self.remove_divergence:
            dummy = 1.0 / dte                                                                                       # :188-201
            tmp2 = hq[1] + v * dummy
            tmp3 = hq[0] + u * dummy
            tmp4 = hq[2] + w * dummy
        else:                                                                                                       # :234-250
            tmp2, tmp3, tmp4 = hq[1].copy(), hq[0].copy(), hq[2].copy()
        if self.anelastic is not None:                                                                              # :211-214
            rb, ri = self.anelastic
            tmp2, tmp3, tmp4 = self.weight(rb, tmp2), self.weight(rb, tmp3), self.weight(rb, tmp4)
        VP0, VP1, PV0, PV1 = O.OPR_P0_INT_VP, O.OPR_P1_INT_VP, O.OPR_P0_INT_PV, O.OPR_P1_INT_PV
        if self.stagger:                                                                                            # :216-226
            tmp1 = self.pint(3, VP0, self.p1(2, self.pint(1, VP0, tmp2)))
            tmp2 = self.pint(3, VP0, self.pint(1, VP1, tmp3))
            tmp3 = self.pint(3, VP1, self.pint(1, VP0, tmp4))
        else:
            tmp1 = self.p1(2, tmp2); tmp2 = self.p1(1, tmp3); tmp3 = self.p1(3, tmp4)                               # :228-230
        tmp1 = tmp1 + tmp2 + tmp3                                                                                   # :258
        h2 = (self.pint(3, VP0, self.pint(1, VP0, hq[1])) if self.stagger else hq[1]).reshape(nz, ny, nx)           # :266-273
        hb, ht = h2[:, 0, :].copy(), h2[:, ny - 1, :].copy()                                                        # :279-280
        if self.anelastic is not None:                                                                              # :275-277
            hb, ht = hb * rb[0], ht * rb[ny - 1]
        if self.direct:
            p, dpdy = OP.opr_poisson_fxz_direct(self.poisson, tmp1, hb, ht, gy_der=self.g[1])
        else:
            p, dpdy = self.solve_poisson(tmp1, hb, ht)                                                              # :284
        if any(f is not None for f in self.pressure_filter):                                                       # :286-290
            from oracle.tlab_oracle_filter import opr_filter
            p = opr_filter(nx, ny, nz, self.pressure_filter, p)
            dpdy = opr_filter(nx, ny, nz, self.pressure_filter, dpdy)
        self.p = p
        if self.stagger:                                                                                            # :307-317
            dpdy = self.pint(1, PV0, self.pint(3, PV0, dpdy))
            tmp4 = self.pint(1, PV0, self.pint(3, PV1, p))
            tmp2 = self.pint(1, PV1, self.pint(3, PV0, p))
        else:
            tmp2 = self.p1(1, p); tmp4 = self.p1(3, p)                                                              # :319-320
        if self.anelastic is not None:                                                                              # :326-329
            hq[0] = hq[0] - self.weight(ri, tmp2); hq[1] = hq[1] - self.weight(ri, dpdy); hq[2] = hq[2] - self.weight(ri, tmp4)
        else:
            hq[0] = hq[0] - tmp2; hq[1] = hq[1] - dpdy; hq[2] = hq[2] - tmp4                                        # :349-351
        types = list(zip(self.flow_jmin, self.flow_jmax)) + list(zip(self.scal_jmin, self.scal_jmax))
        for ia, (a, (tmin, tmax)) in enumerate(zip(hq + hs, types)):                                                # :363-375, :379-396
            ref_b = np.zeros((nz, nx)); ref_t = np.zeros((nz, nx))
            if ia >= 3:
                ref_b, ref_t = sref_b[ia - 3], sref_t[ia - 3]
            ibc = (1 if tmin == 4 else 0) + (2 if tmax == 4 else 0)
            if ibc > 0:
                nb, nt = self.neumann_y(ibc, a)
                if ibc & 1:
                    ref_b = nb
                if ibc & 2:
                    ref_t = nt
            if ia >= 3 and (self.sfc_jmin[ia - 3] == 1 or self.sfc_jmax[ia - 3] == 1):                              # BOUNDARY_BCS_SURFACE_Y
                i = ia - 3
                diff = self.visc / self.schmidt[i]
                t1 = self.p1(2, self.s[i]).reshape(nz, ny, nx)
                avg1 = self._avg1v2d(t1, 0)
                if self.sfc_jmin[i] == 1:
                    hfx = diff * t1[:, 0, :]
                    ref_b = ref_b + self.cpl_jmin[i] * (hfx - diff * avg1)
                if self.sfc_jmax[i] == 1:
                    hfx = -diff * t1[:, ny - 1, :]
                    ref_t = ref_t + self.cpl_jmax[i] * (hfx - diff * avg1)
            b = a.reshape(nz, ny, nx)
            b[:, 0, :] = ref_b
            b[:, ny - 1, :] = ref_t

    def time_substep(self, dte, kco=1.0, scale=False):
        self.rhs_global_incompressible_1(dte)                                                                      # time.f90:604
        self.buffer_relax_scal()                                                                                    # time.f90:628-630
        for i in range(3):
            self.q[i] = self.q[i] + dte * self.hq[i]                                                                # time.f90:651
        for i in range(self.nscal):
            self.s[i] = self.s[i] + dte * self.hs[i]
        if scale:
            for i in range(3):
                self.hq[i] = kco * self.hq[i]                                                                       # time.f90:283
            for i in range(self.nscal):
                self.hs[i] = kco * self.hs[i]
