"""numpy restatement of the reference's transfers between particles and fields, on top of particles_oracle.Particles (its weights and corners):
PARTICLE_TO_FIELD (src/particles/particle_to_field.f90:12-154) and ParticleTrajectories_Initialize / _Accumulate
(src/tools/dns/particle_trajectories.f90:104-149, :156-230), with the reference's line numbers beside each block.  FIELD_TO_PARTICLE of any field is
Particles.interpolate itself.  The loops are the reference's loops, particle by particle: slow and literal on purpose.

The seam: the reference accumulates into an (imax + 1, jmax, kmax + 1) array.  Its serial build copies (1:imax, 1:kmax) out of it, which drops what
fell on column imax + 1 and plane kmax + 1 (periodic=False); its MPI build adds those to column / plane 1 of the neighbour (periodic=True: here index
0 of the same field).  A particle at x = scale lies in cell nx - 1 with fraction 0 (the reference writes past its array there).
TEST INFRASTRUCTURE (numpy only)."""
import numpy as np


def deposit(P, property=None, periodic=True, only_seam=False):
    """(field, cnt, mag), flat nz ny nx arrays: the deposit of particle_to_field.f90:89-151 in the reference's particle and corner order; per node
    the number of contributions and the sum of their magnitudes.  only_seam: the contributions that periodic=False drops, and nothing else."""
    nx, ny, nz = P.nx, P.ny, P.nz
    npart = len(P.l_q[0])
    prop = np.ones(npart) if property is None else np.asarray(property, dtype=np.float64)
    i0, i1, j0, j1, k0, k1, c1, c2, c3, c4, l5, l6 = P.weights()
    field = np.zeros(nx * ny * nz)
    cnt = np.zeros(nx * ny * nz, dtype=np.int64)
    mag = np.zeros(nx * ny * nz)
    for p in range(npart):
        pr = prop[p]
        xseam = i1[p] == 0
        # (i, j, cube) in the order of :131-134 / :138-141
        quad = ((i0[p], j0[p], c3[p], False), (i0[p], j1[p], c4[p], False), (i1[p], j1[p], c1[p], xseam), (i1[p], j0[p], c2[p], xseam))
        if nz == 1:
            planes = ((k0[p], None, False),)
        else:
            planes = ((k0[p], l6[p], False), (k1[p], l5[p], k1[p] == 0))      # :138-141, :144-147
        for k, length, zseam in planes:
            for i, j, cube, xs in quad:
                w = pr * cube if length is None else pr * cube * length
                seam = bool(xs or zseam)
                if only_seam != seam and (only_seam or not periodic):
                    continue
                o = (int(k) * ny + int(j)) * nx + int(i)
                field[o] = field[o] + w
                cnt[o] += 1
                mag[o] += abs(w)
    return field, cnt, mag


def default_tags(isize_part_total, isize_traj):
    """TrajFileName = void (particle_trajectories.f90:114-122)"""
    stride = isize_part_total // isize_traj
    tags = np.array([1 + (j - 1) * stride for j in range(1, isize_traj + 1)], dtype=np.int64)
    assert tags[-1] <= isize_part_total
    return tags


def new_l_traj(isize_traj, nitera_save, inb_traj, fill=0.0):
    """l_traj(isize_traj + 1, nitera_save, inb_traj) in fp32 (:105), as the C-ordered array of its column-major layout: [iv, counter, row]"""
    return np.full((inb_traj, nitera_save, isize_traj + 1), fill, dtype=np.float32)


def trajectories(P, tags, traj_tags, rtime, counter, l_traj, fields=()):
    """ParticleTrajectories_Accumulate for the 1-based column `counter` (the caller advances it, :175): the fields interpolated onto zero targets
    for EVERY particle (:183-203), the time (:210), and the literal double loop of :216-227."""
    inb_part = len(P.l_q)
    data = [P.interpolate(f, np.zeros(len(P.l_q[0]))) for f in fields]
    nvar = len(data)
    l_traj[0:inb_part + nvar, counter - 1, 0] = np.float32(rtime)
    for i in range(len(tags)):
        for j in range(len(traj_tags)):
            if tags[i] == traj_tags[j]:
                for iv in range(inb_part):
                    l_traj[iv, counter - 1, 1 + j] = np.float32(P.l_q[iv][i])
                for iv in range(nvar):
                    l_traj[inb_part + iv, counter - 1, 1 + j] = np.float32(data[iv][i])
    return l_traj
