#!/usr/bin/env python3
"""Golden vectors of the reference's module SpectraMod (tools/statistics/spectra_pool.f90): REDUCE_SPECTRUM, INTEGRATE_SPECTRUM,
REDUCE_CORRELATION and RADIAL_SAMPLESIZE, recorded from the reference's own code.  spectra_pool.f90 and the modules it uses (the closure that
oracle/ref_deps.py finds for base/tlab_constants.f90, fdm/fdm.f90, base/io_fields.f90 and base/tlab_memory.f90) are compiled where they lie, with
amdflang, into a temporary directory outside the repository, behind the small bind(C) driver below, which sets g(:)%size, isize_txc_dimz and
isize_wrk1d; the calls go through ctypes.  Only inputs and outputs are written: tests/golden/spectra_ref.npz.  Never run by a test or by the build.

The reference's transforms (operators/opr_fourier.f90) need FFTW and are not built, so the records feed the routines with transformed fields and
physical fields that this script makes: the spectral product Re(b^ conj(a^)), scaled (P*norm)*norm as tools/statistics/spectra.f90:641 does, is
laid out in the reference's shuffled kz order for REDUCE_SPECTRUM; REDUCE_CORRELATION gets (field*norm)*norm (:653).  A record holds a^, b^ in the
natural kz order (or the unscaled field) and what the reference returned.

Exact-data records (nx*nz a power of two; integer parts; variances that are powers of four): every product and partial sum is exactly
representable, and this script asserts that the reference's output equals the integer evaluation of tests/spectra_oracle.py times the power of
two -- so that the exactness is a property of the input.  Rounding-data records: uniform(-1, 1) parts.
Run in the build container:  python3 tests/golden/make_golden_spectra.py [reference root]"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# g of module FDM is protected: the sizes are set through a dummy argument of an external procedure, in a file of its own
SETTER = """
subroutine spectra_set_sizes(gg, nx, ny, nz)
    use FDM, only: fdm_dt
    implicit none
    type(fdm_dt) :: gg(3)
    integer :: nx, ny, nz
    gg(1)%size = nx; gg(2)%size = ny; gg(3)%size = nz
end subroutine
"""

DRIVER = """
module spectra_driver
    use iso_c_binding
    use FDM, only: g
    use TLab_Memory, only: isize_txc_dimz, isize_wrk1d
    use SpectraMod
    implicit none
    external spectra_set_sizes
contains
    subroutine c_setup(nx, ny, nz) bind(C, name='c_setup')
        integer(c_int), value :: nx, ny, nz
        call spectra_set_sizes(g, nx, ny, nz)
        isize_txc_dimz = (nx + 2)*ny
        isize_wrk1d = ny
    end subroutine
    subroutine c_reduce_spectrum(nx, ny, nz, nblock, in, out, variance) bind(C, name='c_reduce_spectrum')
        integer(c_int), value :: nx, ny, nz, nblock
        real(c_double) :: in((nx + 2)*ny, nz), out(nx/2, ny/nblock, 2*nz), variance(ny, 2)
        call REDUCE_SPECTRUM(nx, ny, nz, nblock, in, out, in, variance)
    end subroutine
    subroutine c_integrate_spectrum(nkx, ny, nz, kr_total, spec_2d, data_x, data_z, spec_r) bind(C, name='c_integrate_spectrum')
        integer(c_int), value :: nkx, ny, nz, kr_total
        real(c_double) :: spec_2d(nkx, ny, nz), data_x(nkx, ny), data_z(nz/2, ny), spec_r(kr_total, ny)
        real(c_double) :: tmp_x(nkx, ny, 2), tmp_z(ny, nz, 2), wrk2d(ny, nz, 2)
        call INTEGRATE_SPECTRUM(nkx, ny, nz, kr_total, ny, spec_2d, data_x, data_z, spec_r, tmp_x, tmp_z, wrk2d)
    end subroutine
    subroutine c_reduce_correlation(nx, ny, nz, nblock, nr_total, in, d2, dx, dz, dr, var1, var2, icalc) bind(C, name='c_reduce_correlation')
        integer(c_int), value :: nx, ny, nz, nblock, nr_total, icalc
        real(c_double) :: in(nx, ny, nz), d2(nx, ny/nblock, nz), dx(nx, ny/nblock), dz(nz, ny/nblock), dr(nr_total, ny/nblock), var1(ny, 2), var2(ny)
        call REDUCE_CORRELATION(nx, ny, nz, nblock, nr_total, in, d2, dx, dz, dr, var1, var2, icalc)
    end subroutine
    subroutine c_radial_samplesize(nx, nz, nr_total, samplesize) bind(C, name='c_radial_samplesize')
        integer(c_int), value :: nx, nz, nr_total
        real(c_double) :: samplesize(nr_total)
        call RADIAL_SAMPLESIZE(nx, nz, nr_total, samplesize)
    end subroutine
end module
"""

# (nx, ny, nz), nblocks, exact data
CASES = [((16, 5, 8), (1,), True), ((32, 7, 16), (1, 2, 3), True), ((8, 4, 32), (1,), True), ((256, 2, 16), (1,), True),
         ((20, 6, 12), (1, 2), False), ((12, 3, 9), (1,), False), ((130, 3, 4), (1,), False)]


def kr_of(nx, nz):
    """kr_total of tools/statistics/spectra.f90: the smaller of the two numbers of modes kept, min(nx/2, nz/2)"""
    return min(nx // 2, nz // 2)


def inputs(shape, exact, seed):
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    sh = (nz, ny, nx // 2 + 1)
    if exact:
        ah = rng.integers(-4, 5, sh) + 1j * rng.integers(-4, 5, sh)
        bh = rng.integers(-4, 5, sh) + 1j * rng.integers(-4, 5, sh)
        field = rng.integers(-8, 9, (nz, ny, nx)).astype(np.float64)
        var1, var2 = 4.0 ** rng.integers(-2, 3, ny), 4.0 ** rng.integers(-2, 3, ny)
        var1[0] = 0.0                                        # a plane without variance: the norm is 1 (spectra_pool.f90:322-324)
    else:
        ah = rng.uniform(-1, 1, sh) + 1j * rng.uniform(-1, 1, sh)
        bh = rng.uniform(-1, 1, sh) + 1j * rng.uniform(-1, 1, sh)
        field = rng.uniform(-1, 1, (nz, ny, nx))
        var1, var2 = rng.uniform(0.5, 2.0, ny), rng.uniform(0.5, 2.0, ny)
    return ah.astype(np.complex128), bh.astype(np.complex128), field, var1, var2


def build(ref, tmp):
    os.environ["TLAB_REFERENCE"] = ref
    from oracle import ref_deps
    for fname, text in (("setter.f90", SETTER), ("driver.f90", DRIVER)):
        with open(os.path.join(tmp, fname), "w") as f:
            f.write(text)
    # (the external procedures that fdm.f90's closure calls -- the banded solvers, the transposition, the log files -- only have to link)
    external = ["utils/linear3.f90", "utils/linear5.f90", "utils/linear7.f90", "utils/tlab_transpose.f90", "base/io_ascii.f90"]
    src = ref_deps.closure(["base/tlab_constants.f90", "fdm/fdm.f90", "base/io_fields.f90", "base/tlab_memory.f90"], external)
    src += [os.path.join(ref, "src", "tools", "statistics", "spectra_pool.f90"), os.path.join(tmp, "setter.f90"), os.path.join(tmp, "driver.f90")]
    flags = ["-cpp", "-O2", "-fPIC", "-I" + os.path.join(ref, "src", "include"), "-DGITBRANCH='golden'", "-DGITHASH='golden'", "-module-dir", tmp]
    objs = []
    for i, s in enumerate(src):
        o = os.path.join(tmp, "o%02d.o" % i)
        subprocess.run(["amdflang", *flags, "-c", s, "-o", o], cwd=tmp, check=True)
        objs.append(o)
    lib = os.path.join(tmp, "libspectra_ref.so")
    subprocess.run(["amdflang", "-shared", "-fPIC", *objs, "-o", lib], cwd=tmp, check=True)
    return ctypes.CDLL(lib)


def ints(a):
    return np.round(a).astype(np.int64)


if __name__ == "__main__":
    import spectra_oracle as S
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TLAB_REFERENCE", "/root/reference")
    out, index = {}, []
    dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)
        for shape, nblocks, exact in CASES:
            nx, ny, nz = shape
            name = "%dx%dx%d" % shape
            kr, nkx, nxh = kr_of(nx, nz), nx // 2, nx // 2 + 1
            norm = 1.0 / (nx * nz)
            ah, bh, field, var1, var2 = inputs(shape, exact, 1000 + nx + nz)
            out["ah_" + name], out["bh_" + name], out["field_" + name], out["var1_" + name], out["var2_" + name] = ah, bh, field, var1, var2
            L.c_setup(nx, ny, nz)
            for nblock in nblocks:
                nyo = ny // nblock
                for cross in (0, 1):
                    b = bh if cross else ah
                    power = (S.product(ah, b) * norm) * norm
                    cin = np.zeros((nz, ny, nxh, 2))
                    cin[..., 0] = power[S.shuffle(nz)]
                    cin[..., 1] = 0.25                                 # (the imaginary part is not read for the power)
                    o2, var = np.zeros((2 * nz, nyo, nkx)), np.zeros((2, ny))
                    L.c_reduce_spectrum(nx, ny, nz, nblock, dp(cin), dp(o2), dp(var))
                    S2 = np.ascontiguousarray(o2[:nz])
                    ox, oz, orr = np.zeros((nyo, nkx)), np.zeros((nyo, nz // 2)), np.zeros((nyo, kr))
                    L.c_integrate_spectrum(nkx, nyo, nz, kr, dp(S2), dp(ox), dp(oz), dp(orr))
                    n = len(index)
                    out["xz_%d" % n], out["x_%d" % n], out["z_%d" % n], out["r_%d" % n], out["variance_%d" % n] = S2, ox, oz, orr, var[0].copy()
                    index.append({"kind": "spectrum", "box": name, "nblock": nblock, "cross": cross, "kr_total": kr, "exact": exact})
                    if exact:
                        pint = (ints(b.real) * ints(ah.real) + ints(b.imag) * ints(ah.imag))[S.shuffle(nz)]
                        Si, vi = np.zeros((nz, nyo, nkx), dtype=np.int64), np.zeros(ny, dtype=np.int64)
                        S.reduce_spectrum(nx, ny, nz, nblock, pint, Si, vi)
                        xi, zi, ri = (np.zeros(a.shape, dtype=np.int64) for a in (ox, oz, orr))
                        S.integrate_spectrum(nkx, nyo, nz, kr, Si, xi, zi, ri)
                        for got, want in ((S2, Si), (ox, xi), (oz, zi), (orr, ri), (var[0], vi)):
                            assert np.array_equal(got, (want.astype(np.float64) * norm) * norm), (name, nblock, cross)
                # REDUCE_CORRELATION on the scaled field
                x = (field * norm) * norm
                v12 = np.ascontiguousarray(np.stack([var1, var2]))
                d2, dx, dz, dr, v2 = np.zeros((nz, nyo, nx)), np.zeros((nyo, nx)), np.zeros((nyo, nz)), np.zeros((nyo, kr)), np.zeros(ny)
                L.c_reduce_correlation(nx, ny, nz, nblock, kr, dp(x), dp(d2), dp(dx), dp(dz), dp(dr), dp(v12), dp(v2), 1)
                n = len(index)
                out["xz_%d" % n], out["x_%d" % n], out["z_%d" % n], out["r_%d" % n], out["variance_%d" % n] = d2, dx, dz, dr, v2
                index.append({"kind": "correlation", "box": name, "nblock": nblock, "nr_total": kr, "exact": exact})
                if exact:      # integers: every plane's factor 2**-e as a shift against the largest
                    nj = S.corr_norms(var1, var2)
                    e = ints(-np.log2(nj))
                    assert np.array_equal(nj, 2.0 ** -e)
                    E = int(e.max())
                    I2, Ix, Iz, Ir, Iv = (np.zeros(a.shape, dtype=np.int64) for a in (d2, dx, dz, dr, v2))
                    S.reduce_correlation(nx, ny, nz, nblock, kr, ints(field), 2 ** (E - e), I2, Ix, Iz, Ir, Iv)
                    for got, want in ((d2, I2), (dx, Ix), (dz, Iz), (dr, Ir)):
                        assert np.array_equal(got, ((want.astype(np.float64) * 2.0 ** -E) * norm) * norm), (name, nblock)
                    assert np.array_equal(v2, (Iv.astype(np.float64) * norm) * norm)
            ss = np.zeros(kr)
            L.c_radial_samplesize(nx, nz, kr, dp(ss))
            out["samplesize_%d" % len(index)] = ss
            index.append({"kind": "samplesize", "box": name, "nr_total": kr})
    out["index"] = np.array(json.dumps(index))
    np.savez_compressed(os.path.join(HERE, "spectra_ref.npz"), **out)
    print("wrote spectra_ref.npz: %d records, %d bytes" % (len(index), os.path.getsize(os.path.join(HERE, "spectra_ref.npz"))))
