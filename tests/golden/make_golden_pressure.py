#!/usr/bin/env python3
"""Golden records of the head of DNS_STATISTICS_TEMPORAL (dns_statistics.f90:93-117) from the reference's own compiled code:
tests/golden/pressure_ref.npz, read by tests/test_pressure_host.py.  Never run by a test or by the build.

FI_PRESSURE_BOUSSINESQ.  Of the two ways to record it the SECOND was taken.  The routine cannot be compiled where it lies: its module closure holds
OPR_Burgers and OPR_Elliptic, which pull in opr_fourier.f90 and with it the FFTW header fftw3.f03, absent from the build container (oracle/ref_driver.f90
says the same of the substep).  So the statements of the routine (tests/pressure_oracle.py::fi_pressure_boussinesq, one line per statement) are
composed from the reference's compiled routines through oracle/ref_lib.py, as oracle/tlab_ref_rhs.py::RefComposedDns composes the substep: every
derivative, every Burgers term and every per-mode solve of the Poisson equation run in the reference's Fortran, the pointwise sums and the Fourier
transforms in numpy.  The advecting velocity of a Burgers term is the one the routine PASSES (zeros in the diffusion block); what the reference's
OPR_Burgers would make of it instead is DESIGN.md section 2.  Cases: DCMP_TOTAL with an explicit Coriolis term and a linear buoyancy, DCMP_ADVDIFF,
DCMP_ADVECTION, DCMP_DIFFUSION, on 16 x 12 x 8 with a stretched y and 24 x 14 x 10 with a uniform y.

FI_VORTICITY: the same composition (six OPR_Partial of the reference, the three statements :41-51 in numpy).  The record holds the result, not the
six derivative arrays.

INTER1V2D: utils/averages.f90 is compiled where it lies, behind the small bind(C) driver below, for every plane and the levels 1..3 of a gate
with the levels 0..3 and an empty plane.

Inputs come from seeds (tests/pressure_oracle.py::golden_case); of every field the file holds each GOLDEN_STRIDE-th point and the maximum of its
magnitude, which keeps it to a few tens of KB.  One subprocess per box: the reference keeps its plans in module variables.
Run in the build container:  python3 tests/golden/make_golden_pressure.py [reference root]"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DRIVER = """
module inter_driver
    use iso_c_binding
    use Averages
    implicit none
contains
    function c_inter1v2d(nx, ny, nz, j, igate, gate) result(avg) bind(C, name='c_inter1v2d')
        integer(c_int), value :: nx, ny, nz, j, igate
        integer(c_int8_t) :: gate(nx, ny, nz)
        real(c_double) :: avg
        avg = INTER1V2D(nx, ny, nz, j, int(igate, 1), gate)
    end function
end module
"""


def worker(box, out):
    import pressure_oracle as P
    from oracle.tlab_ref_rhs import RefComposedDns
    case = P.golden_case(box)
    o = P.golden_oracle(case, RefComposedDns)
    res = {}
    for name in P.GOLDEN_CASES:
        forces = (P.GOLDEN_COR, P.GOLDEN_BOD) if name == "total" else (None, None)
        res["p_" + name] = P.fi_pressure_boussinesq(o, name, *forces)
    res["vorticity"] = P.fi_vorticity(o)[0]
    np.savez(out, **res)


def inter_of_reference(ref, gate, np_):
    nz, ny, nx = gate.shape
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "driver.f90"), "w") as f:
            f.write(DRIVER)
        src = [os.path.join(ref, "src", "base", "tlab_constants.f90"), os.path.join(ref, "src", "utils", "averages.f90"), os.path.join(tmp, "driver.f90")]
        lib = os.path.join(tmp, "libinter_ref.so")
        subprocess.run(["amdflang", "-cpp", "-O2", "-fPIC", "-shared", "-module-dir", tmp, *src, "-o", lib], cwd=tmp, check=True)
        L = ctypes.CDLL(lib)
        L.c_inter1v2d.restype = ctypes.c_double
        g = np.ascontiguousarray(gate)
        return np.array([[L.c_inter1v2d(nx, ny, nz, j + 1, ip, g.ctypes.data_as(ctypes.c_void_p)) for j in range(ny)] for ip in range(1, np_ + 1)])


def main():
    import pressure_oracle as P
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TLAB_REFERENCE", "/root/reference")
    out = {"stride": np.array(P.GOLDEN_STRIDE)}
    with tempfile.TemporaryDirectory() as tmp:
        for box in P.GOLDEN_BOXES:
            f = os.path.join(tmp, box + ".npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", box, f], check=True, env=dict(os.environ, TLAB_REFERENCE=ref))
            R = np.load(f)
            for k in R.files:
                out["%s_%s" % (box, k)] = R[k][::P.GOLDEN_STRIDE].copy()
                out["%s_%s_max" % (box, k)] = np.array(np.abs(R[k]).max())
                print("%s %-12s max %.6e" % (box, k, np.abs(R[k]).max()), flush=True)
            out["%s_inter" % box] = inter_of_reference(ref, P.golden_case(box)["gate"], 3)
    path = os.path.join(HERE, "pressure_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3])
    else:
        main()
