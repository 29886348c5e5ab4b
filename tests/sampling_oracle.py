"""numpy restatement of the sampling between two statistics steps: AvgPhaseSpaceExec and AvgPhaseStress of statistics/avg_phase.f90,
DNS_TOWER_INITIALIZE / DNS_TOWER_ACCUMULATE / TOWER_AVG_IK_V of tools/dns/dns_tower.f90, the copies of PLANES_SAVE of tools/dns/planes.f90 and
FI_GRADIENT of mappings/fi_gradient.f90 -- one statement per line, the reference's line numbers beside it.

Fields are numpy arrays a3[k, j, i] (x fastest, the reference's a(imax, jmax, kmax)).  Sums are sequential `+=` in the reference's order, never
np.sum; numpy neither fuses nor reorders an elementwise statement, and its float64 division is IEEE's."""
import numpy as np

STRESS_IDS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # uu 1, uv 2, uw 3, vv 4, vw 5, ww 6 as the calls give them (avg_phase.f90:230-235)


def fortran_mod(a, p):
    """MOD(a, p) of integers: the sign of a"""
    return int(np.fmod(a, p))


def avg_phase_plane_id(itr, it_first, it_save):
    plane_id = 1                                                          # avg_phase.f90:142
    if it_save != 0:
        plane_id = fortran_mod((itr - 1) - it_first, it_save) + 1         # :143
    return plane_id


def _phase_store(avg, ifld, localsum, avg_planes, plane_id):
    avg[ifld, plane_id - 1] = localsum                                    # :186 (:273)
    avg[ifld, avg_planes] = avg[ifld, avg_planes] + avg[ifld, plane_id - 1] / avg_planes      # :195 (:282)


def avg_phase_space(fields, nz_total, avg_planes, plane_id, avg):
    """AvgPhaseSpaceExec for index 1, 2, 4 (:164-200).  avg: (nf, avg_planes + 1, ny, nx), changed in place"""
    for ifld, field in enumerate(fields):                                 # :165
        localsum = np.zeros(field.shape[1:])                              # :166
        for k in range(field.shape[0]):                                   # :168
            localsum = localsum + field[k] / float(nz_total)              # :173
        _phase_store(avg, ifld, localsum, avg_planes, plane_id)
    return avg


def avg_phase_stress(u, v, w, nz_total, avg_planes, plane_id, avg_stress):
    """AvgPhaseStress (:204-287).  avg_stress: (6, avg_planes + 1, ny, nx), changed in place"""
    q = (u, v, w)
    for stress_id, (a, b) in enumerate(STRESS_IDS):
        wrk2d = np.zeros(u.shape[1:])                                     # :252
        wrk3d = q[a] * q[b]                                               # :254
        for k in range(u.shape[0]):                                       # :256
            wrk2d = wrk2d + wrk3d[k] / float(nz_total)                    # :260
        _phase_store(avg_stress, stress_id, wrk2d, avg_planes, plane_id)
    return avg_stress


class Tower:
    """DNS_TOWER's module state on one rank (ims_offset = 0)"""

    def __init__(self, nx, ny, nz, stride, nitera_save):
        self.nx, self.ny, self.nz, self.nsave = nx, ny, nz, nitera_save
        self.consistent = True
        pos = []
        for n, s in zip((nx, ny, nz), stride):
            count = sum(1 for i in range(n) if fortran_mod(i - 1, s) == 0)              # dns_tower.f90:116-132
            p = [i + 1 for i in range(n) if fortran_mod(i, s) == 0]                     # :164-186
            self.consistent = self.consistent and len(p) == count                       # else the second loop writes past tower_ipos
            pos.append(np.array(p))
        self.ipos, self.jpos, self.kpos = pos
        self.imax, self.jmax, self.kmax = (len(p) for p in pos)
        tip = self.imax * self.kmax                                                     # :151
        self.acc_field = nitera_save * self.jmax * tip                                  # :154
        self.acc_mean = nitera_save * self.jmax                                         # :155
        self.bufsize = 5 * self.acc_field + 5 * self.acc_mean + 2 * nitera_save         # :156
        self.buf = np.zeros(self.bufsize)
        self.accumulation, self.mode_check = 1, 0                                       # :201

    def _slot(self, name):
        names = ("u", "v", "w", "p", "s")
        if name in names:
            return names.index(name) * self.acc_field
        return 5 * self.acc_field + ("um", "vm", "wm", "pm", "sm").index(name) * self.acc_mean

    def avg_ik_v(self, a):
        """TOWER_AVG_IK_V (:502-546)"""
        avg = np.zeros(self.jmax)                                                       # :522-524
        for k in range(self.nz):                                                        # :526
            for j in range(self.jmax):                                                  # :527
                row = a[k, self.jpos[j] - 1]
                s = avg[j]
                for i in range(self.nx):                                                # :528
                    s = s + row[i]                                                      # :529
                avg[j] = s
        return avg / float(np.float32(self.nx * self.nz))                               # :535 (a default real)

    def accumulate(self, index, fields, itime, rtime):
        """DNS_TOWER_ACCUMULATE (:207-289); the columns at tower_jpos (identical to the reference's 1:tower_jmax:tower_jstride for stride_y = 1)"""
        assert self.mode_check + index <= 7 and self.accumulation <= self.nsave
        tip, acc = self.imax * self.kmax, self.accumulation - 1
        names = {4: ("p",), 1: ("u", "v", "w"), 2: ("s",)}[index]
        if index == 4:
            self.buf[5 * self.acc_field + 5 * self.acc_mean + acc] = rtime              # :236
            self.buf[5 * self.acc_field + 5 * self.acc_mean + self.nsave + acc] = itime # :237
        for name, v in zip(names, fields):
            ip = self._slot(name) + acc * self.jmax * tip                               # :229
            for kk in range(self.kmax):                                                 # :238
                for ii in range(self.imax):                                             # :239
                    self.buf[ip:ip + self.jmax] = v[self.kpos[kk] - 1, self.jpos - 1, self.ipos[ii] - 1]      # :240
                    ip = ip + self.jmax                                                 # :241
            ipm = self._slot(name + "m") + acc * self.jmax                              # :244
            self.buf[ipm:ipm + self.jmax] = self.avg_ik_v(v)                            # :246
        self.mode_check = self.mode_check + index                                       # :279
        if self.mode_check == 7:                                                        # :281
            self.mode_check = 0
            self.accumulation = self.accumulation + 1


def planes_gather(fields, idir, nodes):
    """PLANES_SAVE's copies (planes.f90:286-290, :304-308, :330-338) as C-ordered arrays: data_i -> (nz, size, ny), data_j -> (nz, size, nx),
    data_k -> (size, ny, nx)"""
    nz, ny, nx = fields[0].shape
    n = len(nodes)
    size = len(fields) * n
    out = np.zeros({1: (nz, size, ny), 2: (nz, size, nx), 3: (size, ny, nx)}[idir])
    offset = 0
    for f in fields:
        for m, node in enumerate(nodes):
            if idir == 3:
                out[offset + m] = f[node - 1]                             # :288
            elif idir == 2:
                out[:, offset + m, :] = f[:, node - 1, :]                 # :306
            else:
                out[:, offset + m, :] = f[:, :, node - 1]                 # :334
        offset = offset + n
    return out


def fi_gradient(sx, sy, sz):
    """FI_GRADIENT's pointwise statements on the three derivatives (fi_gradient.f90:36-40)"""
    result = sx * sx + sy * sy                                            # :38
    result = result + sz * sz                                             # :40
    return result


def summation_bound(a, jpos, ref):
    """the bound tests/test_gpu_averages.py uses for AVG_IK_V, at the planes jpos: 2 (n - 1) u sum|a| / n + 2 u |ref|, u = 2^-53, n = nx nz"""
    nz, ny, nx = a.shape
    n = nx * nz
    sums = np.array([np.abs(a[:, j - 1, :]).sum() for j in jpos])
    return 2.0 * (n - 1) * 2.0 ** -53 * sums / n + 2.0 * 2.0 ** -53 * np.abs(ref)
