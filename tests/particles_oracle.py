"""numpy restatement of the reference's Lagrangian particles as its serial branch does them, with the reference's line numbers beside each block:
FIELD_TO_PARTICLE / Interpolate_Inside_Zones (src/particles/particle_interpolate.f90:186-332), RHS_PART_1 (src/tools/dns/rhs_part_1.f90:43-54,
:112-123), TIME_SUBSTEP_PARTICLE (src/tools/dns/time.f90:906-1070, serial branch :1014-1036), LOCATE_Y (src/utils/locate_y.f90) and the scaling of
l_hq (time.f90:215, :300-304).  One numpy operation per operation of the reference, in its order: no fused multiply-add can occur, so the device
kernel, which does not contract either, gives the same bits.

These routines cannot be reached through oracle/ref_lib.py; tests/test_particles_host.py pins the restatement by properties that do not depend on it
being right (linear fields are reproduced, LOCATE_Y against searchsorted, uniform flow, exponential relaxation).

The halo zones and the particle sorting of the reference (Sort_Into_Grid, Sort_Into_Halos) only serve to reach f(1) from the last cell of a periodic
direction: here the upper corner of that cell is index 0.  TEST INFRASTRUCTURE (numpy only)."""
import numpy as np

PART_TRACER, PART_INERTIA = 1, 2                       # particle_vars.f90:8-14
BCS_NONE, BCS_STICK, BCS_SPECULAR = 0, 1, 2            # particle_vars.f90:28-30


def grid_scale(nodes, periodic):
    """g%scale of FDM_CreatePlan (fdm/fdm.f90:162-167)"""
    n = len(nodes)
    if n <= 1:
        return 1.0
    s = nodes[n - 1] - nodes[0]
    if periodic:
        s = s * (1.0 + 1.0 / float(n - 1))
    return float(s)


def locate_y(yp, y):
    """LOCATE_Y (locate_y.f90:13-22): the bisection loop itself, 1-based jm, jp, jc"""
    y = np.asarray(y, dtype=np.float64)
    ny = len(y)
    out = np.empty(len(yp), dtype=np.int32)
    for ip, v in enumerate(np.asarray(yp, dtype=np.float64)):
        jp, jm = ny, 1
        jc = (jm + jp) // 2
        while (v - y[jc - 1]) * (v - y[jc]) > 0.0 and jc > jm:
            if v < y[jc - 1]:
                jp = jc
            else:
                jm = jc
            jc = (jm + jp) // 2
        out[ip] = jc
    return out


def _cell(xp, dinv, n):
    """particle_interpolate.f90:239-248: (0-based lower corner clamped into the field, fraction from the unclamped floor)"""
    a = xp * dinv
    fl = np.floor(a)
    return np.clip(fl, 0, n - 1).astype(np.int64), a - fl


class Particles:
    """x, y, z: the grid nodes (x, z periodic); q = [u, v, w] flat (nz ny nx) arrays are handed to substep()."""

    def __init__(self, x, y, z, type=PART_TRACER, bcs=None, stokes=0.0, settling=0.0):
        self.x, self.y, self.z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
        self.nx, self.ny, self.nz = len(x), len(y), len(z)
        self.type = type
        self.bcs = (BCS_SPECULAR if type == PART_INERTIA else BCS_NONE) if bcs is None else bcs      # particle_procs.f90:65-67
        self.stokes, self.settling = float(stokes), float(settling)
        self.ncol = 6 if type == PART_INERTIA else 3
        self.sx, self.sy, self.sz = grid_scale(self.x, True), grid_scale(self.y, False), grid_scale(self.z, True)
        self.dxi, self.dzi = float(self.nx) / self.sx, float(self.nz) / self.sz      # :203-204
        self.l_q = self.l_hq = self.nodes = None

    def set(self, l_q, l_hq=None):
        self.l_q = [np.array(a, dtype=np.float64) for a in l_q]
        assert len(self.l_q) == self.ncol
        self.l_hq = [np.zeros_like(a) for a in self.l_q] if l_hq is None else [np.array(a, dtype=np.float64) for a in l_hq]
        self.nodes = locate_y(self.l_q[1], self.y)

    def weights(self):
        """(i0, i1, j0, j1, k0, k1, c1..c4, l5, l6) of particle_interpolate.f90:239-269"""
        i0, l1 = _cell(self.l_q[0], self.dxi, self.nx)
        i1 = np.where(i0 + 1 == self.nx, 0, i0 + 1)
        l2 = 1.0 - l1
        if self.nz > 1:
            k0, l5 = _cell(self.l_q[2], self.dzi, self.nz)
            k1 = np.where(k0 + 1 == self.nz, 0, k0 + 1)
        else:
            k0 = k1 = np.zeros_like(i0)
            l5 = np.zeros_like(l1)
        l6 = 1.0 - l5
        j0 = np.clip(self.nodes.astype(np.int64) - 1, 0, self.ny - 2)
        j1 = j0 + 1
        l3 = (self.l_q[1] - self.y[j0]) / (self.y[j1] - self.y[j0])
        l4 = 1.0 - l3
        return i0, i1, j0, j1, k0, k1, l1 * l3, l1 * l4, l4 * l2, l2 * l3, l5, l6

    def interpolate(self, f, target):
        """data_out + A + B of particle_interpolate.f90:277-285 (3-D) and :320-324 (2-D), left to right"""
        f = np.asarray(f).reshape(self.nz, self.ny, self.nx)
        i0, i1, j0, j1, k0, k1, c1, c2, c3, c4, l5, l6 = self.weights()
        a = ((c3 * f[k0, j0, i0] + c4 * f[k0, j1, i0]) + c1 * f[k0, j1, i1]) + c2 * f[k0, j0, i1]
        if self.nz == 1:
            return target + a
        b = ((c3 * f[k1, j0, i0] + c4 * f[k1, j1, i0]) + c1 * f[k1, j1, i1]) + c2 * f[k1, j0, i1]
        return (target + a * l6) + b * l5

    def cell_keys(self):
        """the key of the device sort: (k0 ny + j0) nx + i0"""
        i0, _, j0, _, k0, _ = self.weights()[:6]
        return (k0 * self.ny + j0) * self.nx + i0

    def begin_step(self):
        self.l_hq = [np.zeros_like(a) for a in self.l_q]      # time.f90:215

    def substep(self, q, dte, kco=1.0, scale=False):
        lq, lh = self.l_q, self.l_hq
        # RHS_PART_1
        if self.type == PART_TRACER:                                     # rhs_part_1.f90:45-48, :112-113
            new = [self.interpolate(q[i], lh[i]) for i in range(3)]
            lh[:3] = new
        else:                                                            # :50-54, :115-123
            ui = [self.interpolate(q[i], np.zeros_like(lq[0])) for i in range(3)]
            dummy = 1.0 / self.stokes
            dummy2 = self.settling / self.stokes
            for i in range(3):
                lh[i] = lh[i] + lq[3 + i]
            lh[3] = lh[3] + dummy * (ui[0] - lq[3])
            lh[4] = lh[4] + dummy * (ui[1] - lq[4]) - dummy2
            lh[5] = lh[5] + dummy * (ui[2] - lq[5])
        for i in range(self.ncol):                                       # time.f90:926-928
            lq[i] = lq[i] + dte * lh[i]
        # time.f90:1016-1036, one wrap at most
        x_right = self.x[0] + self.sx
        lq[0] = np.where(lq[0] > x_right, lq[0] - self.sx, np.where(lq[0] < self.x[0], lq[0] + self.sx, lq[0]))
        if self.nz > 1:
            z_right = self.z[0] + self.sz
            lq[2] = np.where(lq[2] > z_right, lq[2] - self.sz, np.where(lq[2] < self.z[0], lq[2] + self.sz, lq[2]))
        # time.f90:1040-1062
        y_right = self.y[0] + self.sy
        above, below = lq[1] > y_right, lq[1] < self.y[0]
        if self.bcs == BCS_SPECULAR:
            lq[1] = np.where(above, 2.0 * y_right - lq[1], np.where(below, 2.0 * self.y[0] - lq[1], lq[1]))
            if self.ncol == 6:
                lq[4] = np.where(above | below, -lq[4], lq[4])
        elif self.bcs == BCS_STICK:
            lq[1] = np.where(above, y_right, np.where(below, self.y[0], lq[1]))
        self.nodes = locate_y(lq[1], self.y)                             # time.f90:1067
        if scale:                                                        # time.f90:300-304
            for i in range(self.ncol):
                lh[i] = kco * lh[i]

    def step(self, q_of_substep, dtime, kdt, kco):
        """TIME_RUNGEKUTTA for the particles: q_of_substep(k) gives the velocities the k-th substep sees"""
        self.begin_step()
        n = len(kdt)
        for k in range(n):
            last = k == n - 1
            self.substep(q_of_substep(k), dtime * kdt[k], 1.0 if last else kco[k], not last)
