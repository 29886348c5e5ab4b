"""tests/transfers_oracle.py pinned by properties that do not depend on the restatement being right (no GPU): the deposit is the adjoint of the
interpolation that tests/test_particles_host.py pins, it conserves the property, periodic=False is periodic=True without the seam contributions; the
trajectory array has the reference's layout; the Fortran wrappers compile against the C interfaces; the argument checks of the new entry points."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cases import grids
from particles_oracle import Particles, PART_TRACER, PART_INERTIA
from transfers_oracle import deposit, default_tags, new_l_traj, trajectories

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHAPES = [(20, 12, 8), (70, 33, 9), (20, 12, 1)]
U = 2.0 ** -53


def _particles(shape, n, seed, type=PART_TRACER):
    nx, ny, nz = shape
    x, y, z = grids(nx, ny, nz, True)
    if nz == 1:
        z = np.zeros(1)
    P = Particles(x, y, z, type=type, stokes=0.3)
    rng = np.random.default_rng(seed)
    lq = [rng.uniform(0.0, P.sx, n), rng.uniform(y[0], y[-1], n), rng.uniform(0.0, P.sz, n)]
    hand = [(0.5 * (x[-1] + P.sx), None, None), (None, None, 0.5 * (z[-1] + P.sz)), (0.5 * (x[-1] + P.sx), None, 0.5 * (z[-1] + P.sz)),
            (x[3], y[4], z[min(2, nz - 1)]), (0.0, y[0], 0.0), (P.sx, y[-1], P.sz)]      # seam cells, on nodes, the corners of the box, x = scale
    for p, h in enumerate(hand[:n]):
        for i in range(3):
            if h[i] is not None:
                lq[i][p] = h[i]
    lq += [rng.uniform(-0.5, 0.5, n) for _ in range(P.ncol - 3)]
    P.set(lq)
    return P, rng


@pytest.mark.parametrize("shape", SHAPES)
def test_deposit_is_the_adjoint_of_the_interpolation(shape):
    """sum_nodes deposit(p) f = sum_particles p interpolate(f): both are sum_p sum_corners p w f, in two orders.  Bound: every product p w f is
    rounded at most three times more on one side than on the other and the sums have np and nnodes terms; 2^-53 (8 np + nnodes) sum|p| max|f|."""
    n = 1000
    P, rng = _particles(shape, n, 11)
    nn = P.nx * P.ny * P.nz
    f = rng.uniform(-1.0, 1.0, nn)
    prop = rng.uniform(-1.0, 2.0, n)
    field, cnt, mag = deposit(P, prop, True)
    lhs = float(np.sum(field * f))
    rhs = float(np.sum(prop * P.interpolate(f, np.zeros(n))))
    bound = U * (8 * n + nn) * float(np.abs(prop).sum()) * float(np.abs(f).max())
    print("%s adjointness: %.3e against %.3e" % (shape, abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound
    assert cnt.sum() == (8 if shape[2] > 1 else 4) * n


@pytest.mark.parametrize("shape", SHAPES)
def test_periodic_deposit_conserves_the_property(shape):
    """the eight weights of a particle sum to 1: sum(field) = sum(property) within 2^-53 (np + nnodes + 16) sum|p|"""
    n = 1000
    P, rng = _particles(shape, n, 12)
    nn = P.nx * P.ny * P.nz
    for prop in (rng.uniform(-1.0, 2.0, n), None):
        field, _, _ = deposit(P, prop, True)
        total = float(n) if prop is None else float(prop.sum())
        mass = float(n) if prop is None else float(np.abs(prop).sum())
        err = abs(float(field.sum()) - total)
        print("%s conservation: %.3e against %.3e" % (shape, err, U * (n + nn + 16) * mass))
        assert err <= U * (n + nn + 16) * mass
    dropped, _, _ = deposit(P, None, False)
    assert float(dropped.sum()) < n - 1.0      # the serial reference loses what the seam cells put on their upper corners


@pytest.mark.parametrize("shape", SHAPES)
def test_not_periodic_is_periodic_without_the_seam_contributions(shape):
    n = 1000
    P, rng = _particles(shape, n, 13)
    nx, ny, nz = shape
    prop = rng.uniform(0.5, 2.0, n)
    ft, ct, mt = deposit(P, prop, True)
    ff, cf, mf = deposit(P, prop, False)
    fs, cs, ms = deposit(P, prop, True, only_seam=True)
    assert cs.sum() > 0 and np.array_equal(ct, cf + cs)
    # the seam contributions land on column 0 and plane 0 only
    landed = cs.reshape(nz, ny, nx) > 0
    inside = landed.copy()
    inside[:, :, 0] = False
    if nz > 1:
        inside[0] = False
    assert not inside.any()
    # where none landed the two fields have the same bits; where some did, they differ by their sum up to the rounding of the other order
    none = cs == 0
    assert np.array_equal(ft[none].view(np.int64), ff[none].view(np.int64))
    assert (np.abs(ft - (ff + fs)) <= 2.0 * np.maximum(ct - 1, 0) * U * mt).all()
    assert (fs[~none] >= 0).all() and fs.sum() > 0      # (the particle at x = scale puts weight 0 across the seam)


def test_property_none_counts_every_particle_once():
    for shape in SHAPES:
        P, _ = _particles(shape, 300, 14)
        a, ca, _ = deposit(P, None, True)
        b, cb, _ = deposit(P, np.ones(300), True)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)) and np.array_equal(ca, cb)


def test_a_particle_on_a_node_deposits_there_alone():
    """weights 1, 0, 0, ...: the whole property on the node, and x = scale on node nx of the seam cell with nothing across the seam"""
    nx, ny, nz = SHAPES[0]
    x, y, z = grids(nx, ny, nz, True)
    P = Particles(x, y, z)
    P.set([np.array([0.0, P.sx]), np.array([y[4], y[2]]), np.array([0.0, P.sz])])      # (x(4) nx / scale need not be the integer 3: the ends are exact)
    field, cnt, _ = deposit(P, np.array([2.5, -4.0]), True)
    f3 = field.reshape(nz, ny, nx)
    assert f3[0, 4, 0] == 2.5 and f3[nz - 1, 2, nx - 1] == -4.0
    assert np.count_nonzero(field) == 2 and cnt.sum() == 16


def test_trajectory_layout_and_default_tags():
    """l_traj(isize_traj + 1, nitera_save, inb_traj) (particle_trajectories.f90:105), the default tags 1 + (j - 1) (total / number) (:114-118), the
    time in row 1 (:210), the tracked particles' columns in row 1 + j wherever the tag sits in the particle arrays (:216-227)"""
    assert np.array_equal(default_tags(1000, 7), 1 + 142 * np.arange(7)) and np.array_equal(default_tags(5, 5), [1, 2, 3, 4, 5])
    assert np.array_equal(default_tags(64, 1), [1])
    shape = SHAPES[0]
    n, ntraj, nsave = 50, 4, 3
    P, rng = _particles(shape, n, 15, type=PART_INERTIA)
    f = [rng.uniform(-1.0, 1.0, P.nx * P.ny * P.nz) for _ in range(2)]
    tags = rng.permutation(np.arange(1, n + 1)).astype(np.int64)      # as after a sort
    tt = np.array([37, 5, 999, 12], dtype=np.int64)                   # unsorted, one that nobody carries
    lt = new_l_traj(ntraj, nsave, 6 + 2, fill=-7.0)
    assert lt.shape == (8, nsave, ntraj + 1) and lt.dtype == np.float32 and lt.flags["C_CONTIGUOUS"]
    trajectories(P, tags, tt, 0.125, 2, lt, f)
    assert (lt[:, 0] == -7.0).all() and (lt[:, 2] == -7.0).all()      # the other columns
    assert (lt[:, 1, 0] == np.float32(0.125)).all()
    assert (lt[:, 1, 3] == -7.0).all()                                # tag 999
    vals = [P.interpolate(a, np.zeros(n)) for a in f]
    for j, t in enumerate(tt):
        if t == 999:
            continue
        i = int(np.flatnonzero(tags == t)[0])
        want = [P.l_q[iv][i] for iv in range(6)] + [v[i] for v in vals]
        assert np.array_equal(lt[:, 1, 1 + j], np.array(want).astype(np.float32))
    # the flat index of (row, counter, iv) is the column-major one
    flat = lt.ravel()
    assert flat[(1 + 1) + (ntraj + 1) * ((2 - 1) + nsave * 7)] == lt[7, 1, 2]


def test_transfer_wrappers_compile_against_the_c_interfaces(tmp_path):
    """tlab_amd/fortran/tlab_amd_particles.f90 with a caller of the four transfer wrappers shaped like the reference's call sites (module arrays of
    rank 2, l_g%nodes, l_g%tags, a single-precision l_traj of rank 3)"""
    import re
    fortran = os.path.join(ROOT, "tlab_amd", "fortran")
    fc = shutil.which("amdflang")
    mod = os.path.join(ROOT, "oracle", "_ref", "mod")                   # TLab_AMD_Check of tlab_amd_c.f90 writes through the reference's TLab_WorkFlow
    if fc is None or not os.path.isdir(mod):
        pytest.skip("amdflang or the reference's module files (oracle/_ref/mod) are not here")
    run = lambda *a: subprocess.run([fc, "-cpp", "-O2", "-I", mod, "-module-dir", str(tmp_path), "-c", *a], cwd=tmp_path,      # noqa: E731
                                    capture_output=True, text=True)
    r = run(os.path.join(fortran, "tlab_amd_c.f90"), "-o", str(tmp_path / "c.o"))
    assert r.returncode == 0, r.stderr
    r = run("-I", str(tmp_path), os.path.join(fortran, "tlab_amd_particles.f90"), "-o", str(tmp_path / "p.o"))
    assert r.returncode == 0, r.stderr
    src = open(os.path.join(fortran, "tlab_amd_particles.f90")).read()
    assert re.findall(r"^\s*use\s+(\w+)", src, flags=re.M | re.I) == ["TLab_AMD_C"]
    assert max(len(l) for l in src.splitlines()) <= 160
    (tmp_path / "caller.f90").write_text(
        "subroutine caller(dns, q, s, txc, l_q, l_txc, nodes, tags, l_traj, l_traj_tags, n, isize_part, np, isize_traj, nitera_save, inb_traj)\n"
        "    use TLab_AMD_C\n"
        "    use TLab_AMD_Particles\n"
        "    type(c_ptr) :: dns, fields(4), targets(4)\n"
        "    integer :: n, isize_part, np, isize_traj, nitera_save, inb_traj, inb_part, counter, iv\n"
        "    real(c_double), target :: q(n, 3), s(n, 1), txc(n, 2), l_q(isize_part, *), l_txc(isize_part, 4)\n"
        "    real(c_double) :: rtime\n"
        "    integer(c_int) :: nodes(isize_part)\n"
        "    integer(c_long_long) :: tags(isize_part), l_traj_tags(isize_traj)\n"
        "    real(c_float) :: l_traj(isize_traj + 1, nitera_save, inb_traj)\n"
        "    do iv = 1, 3\n"
        "        fields(iv) = c_loc(q(1, iv)); targets(iv) = c_loc(l_txc(1, iv))\n"
        "    end do\n"
        "    fields(4) = c_loc(s(1, 1)); targets(4) = c_loc(l_txc(1, 4))\n"
        "    call TLab_AMD_Field_To_Particle(dns, 4, fields, np, isize_part, l_q, nodes, targets)\n"
        "    call TLab_AMD_Particle_To_Field(dns, np, isize_part, l_q, nodes, txc(:, 1))\n"
        "    call TLab_AMD_Particle_To_Field(dns, np, isize_part, l_q, nodes, txc(:, 2), property=l_txc(:, 4), periodic=.false.)\n"
        "    call TLab_AMD_Trajectories_Set(dns, isize_traj, l_traj_tags)\n"
        "    call TLab_AMD_Trajectories_Accumulate(dns, rtime, counter, nitera_save, np, isize_part, inb_part, l_q, nodes, tags, 4, fields, l_traj)\n"
        "end subroutine caller\n")
    r = run("-I", str(tmp_path), str(tmp_path / "caller.f90"), "-o", str(tmp_path / "caller.o"))
    assert r.returncode == 0, r.stderr


def test_argument_checks_of_the_new_entries(tmp_path):
    """tools/particles_host_check.cpp (csrc/particles_host.hpp without a device) built plainly and run: every refusal of the header's list gives
    TLAB_EINVAL and stores nothing, np = 0 reads no pointer, exactly the listed entries of each pointer array are read"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "particles_host_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "particles_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "particles_host_check ok" in r.stdout, r.stdout + r.stderr
    src = open(os.path.join(ROOT, "tools", "particles_host_check.cpp")).read()
    for name in ("particle_check_sample", "particle_check_deposit", "particle_trajectory_table", "particle_check_trajectories"):
        assert name in src
