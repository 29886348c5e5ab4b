#!/usr/bin/env python3
"""Golden vectors of the reference's conditional statistics, recorded from the reference's own code: AVG1V2D and AVG1V2D1G (utils/averages.f90),
PDF1V2D / PDF1V2D1G / PDF2V2D WITH their optional a, avg arguments (utils/pdfs.f90) and RAW_TO_CENTRAL (statistics/avg_xz.f90).
base/tlab_constants.f90, utils/averages.f90, utils/pdfs.f90 and statistics/avg_xz.f90 are compiled where they lie, with amdflang, into a temporary
directory outside the repository, behind the small bind(C) driver below; the calls go through ctypes.  Only inputs and outputs are written:
tests/golden/conditional_ref.npz.  Never run by a test or by the build.

RAW_TO_CENTRAL: statistics/avg_xz.f90 DOES link here -- the driver holds stand-in modules for the names it uses (TLab_Pointers, TLab_WorkFlow) and
a stub for IO_WRITE_AVERAGES, none of which RAW_TO_CENTRAL touches -- so the records `central` are the reference's own routine for nm = 2 .. 10
and tlab_raw_to_central is held to them bit for bit.

Boxes (20,12,8), (7,5,3), (6,1,4).  Fields: u, v uniform(-1, 1) + cos(j) (rounding data); q4 multiples of 1/4 in [-2, 2] and i2 integers in
[-2, 2] (every power and every partial sum exact for nm <= 4 and nm = 10); two fields of a record are not stored: "c" means u with the plane
ny/2 set to 0.75 (a constant plane: a zero step) and "uv" the product u*v.  The gate holds the levels 0 .. 3; where the box has the planes, plane 1 has no point of level 2 and
plane 2 exactly one of level 3.
  moments  AVG1V2D (row 0) and AVG1V2D1G for the levels 1 .. 3 (rows 1 .. 3), imom = 1 .. 10, every plane: (4, 10, ny)
  cavg1v   per plane and the volume (the box (nx*ny, 1, nz)): (ny + 1, nbins + 2, 2) = [.., 0] pdf with its two centres, [.., 1] avg (nbins used)
  cavg2v   the same over PDF2V2D: (ny + 1, nb1*nb2 + 2 + 2*nb1, 2)
  central  RAW_TO_CENTRAL of the first nm entries of `central_in`, nm = 2 .. 10: (10,) each, the tail zero
The records are listed in the JSON string `index`.  Run in the build container:  python3 tests/golden/make_golden_conditional.py [reference root]"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

STANDINS = """
module TLab_Pointers
    use TLab_Constants, only: wp
    implicit none
    type :: pointers_dt
        sequence
        character(len=32) :: tag
        real(wp), pointer :: field(:)
    end type pointers_dt
end module
module TLab_WorkFlow
    implicit none
contains
    subroutine TLab_Write_ASCII(file, lineloc, flag_all)
        character(len=*), intent(in) :: file, lineloc
        logical, intent(in), optional :: flag_all
    end subroutine
end module
subroutine IO_WRITE_AVERAGES(fname, itime, rtime, ny, nv, ng, y, varname, groupname, avg)
    use TLab_Constants, only: wp, wi
    character(len=*) fname, varname(*), groupname(*)
    integer(wi) itime, ny, nv, ng
    real(wp) rtime, y(*), avg(*)
end subroutine
"""

DRIVER = """
module cond_driver
    use iso_c_binding
    use Averages
    use PDFS
    implicit none
contains
    function c_avg1v2d(nx, ny, nz, j, imom, a) bind(C, name='c_avg1v2d') result(r)
        integer(c_int), value :: nx, ny, nz, j, imom
        real(c_double) :: a(nx, ny, nz), r
        r = AVG1V2D(nx, ny, nz, j, imom, a)
    end function
    function c_avg1v2d1g(nx, ny, nz, j, igate, imom, a, gate) bind(C, name='c_avg1v2d1g') result(r)
        integer(c_int), value :: nx, ny, nz, j, igate, imom
        real(c_double) :: a(nx, ny, nz), r
        integer(c_int8_t) :: gate(nx, ny, nz)
        r = AVG1V2D1G(nx, ny, nz, j, int(igate, 1), imom, a, gate)
    end function
    subroutine c_cavg1v2d(ilim, nx, ny, nz, j, umin, umax, u, nbins, pdf, a, avg) bind(C, name='c_cavg1v2d')
        integer(c_int), value :: ilim, nx, ny, nz, j, nbins
        real(c_double), value :: umin, umax
        real(c_double) :: u(nx, ny, nz), a(nx, ny, nz), pdf(nbins + 2), avg(nbins), wrk(nbins)
        call PDF1V2D(ilim, nx, ny, nz, j, umin, umax, u, nbins, pdf, wrk, a, avg)
    end subroutine
    subroutine c_cavg1v2d1g(ilim, nx, ny, nz, j, igate, gate, umin, umax, u, nbins, pdf, a, avg) bind(C, name='c_cavg1v2d1g')
        integer(c_int), value :: ilim, nx, ny, nz, j, nbins, igate
        integer(c_int8_t) :: gate(nx, ny, nz)
        real(c_double), value :: umin, umax
        real(c_double) :: u(nx, ny, nz), a(nx, ny, nz), pdf(nbins + 2), avg(nbins), wrk(nbins)
        call PDF1V2D1G(ilim, nx, ny, nz, j, int(igate, 1), gate, umin, umax, u, nbins, pdf, wrk, a, avg)
    end subroutine
    subroutine c_cavg2v2d(nx, ny, nz, j, u, v, nbins, pdf, a, avg) bind(C, name='c_cavg2v2d')
        integer(c_int), value :: nx, ny, nz, j
        integer(c_int) :: nbins(2)
        real(c_double) :: u(nx, ny, nz), v(nx, ny, nz), a(nx, ny, nz), pdf(nbins(1)*nbins(2) + 2 + 2*nbins(1)), avg(nbins(1)*nbins(2))
        real(c_double) :: wrk(nbins(1), max(nbins(2), 3))
        call PDF2V2D(nx, ny, nz, j, u, v, nbins, pdf, wrk, a, avg)
    end subroutine
    subroutine c_raw_to_central(nm, moments) bind(C, name='c_raw_to_central')
        integer(c_int), value :: nm
        real(c_double) :: moments(nm)
        external RAW_TO_CENTRAL
        call RAW_TO_CENTRAL(nm, moments)
    end subroutine
end module
"""

BOXES = {"a": (20, 12, 8), "b": (7, 5, 3), "c": (6, 1, 4)}      # (nx, ny, nz)
NBINS = (1, 2, 32, 100)


def fields(box, seed):
    nx, ny, nz = box
    rng = np.random.default_rng(seed)
    off = np.cos(np.arange(ny))[None, :, None]
    F = {k: rng.uniform(-1, 1, (nz, ny, nx)) + off for k in ("u", "v")}
    F["q4"] = rng.integers(-8, 9, (nz, ny, nx)).astype(np.float64) / 4.0
    F["i2"] = rng.integers(-2, 3, (nz, ny, nx)).astype(np.float64)
    gate = rng.integers(0, 4, (nz, ny, nx)).astype(np.int8)
    if ny > 2:
        gate[:, 1, :][gate[:, 1, :] == 2] = 1                        # no point of level 2 in plane 1
        gate[:, 2, :][gate[:, 2, :] == 3] = 0
        gate[nz // 2, 2, nx // 2] = 3                                # one point of level 3 in plane 2
    return F, gate


def constant_plane(u):
    c = u.copy()
    c[:, u.shape[1] // 2, :] = 0.75
    return c


def build(ref, tmp):
    for name, text in (("standins.f90", STANDINS), ("driver.f90", DRIVER)):
        with open(os.path.join(tmp, name), "w") as f:
            f.write(text)
    src = os.path.join(ref, "src")
    files = [os.path.join(src, "base", "tlab_constants.f90"), os.path.join(src, "utils", "averages.f90"), os.path.join(src, "utils", "pdfs.f90"),
             os.path.join(tmp, "standins.f90"), os.path.join(src, "statistics", "avg_xz.f90"), os.path.join(tmp, "driver.f90")]
    lib = os.path.join(tmp, "libcond_ref.so")
    subprocess.run(["amdflang", "-cpp", "-O2", "-fPIC", "-shared", "-I", os.path.join(src, "include"), "-module-dir", tmp, *files, "-o", lib],
                   cwd=tmp, check=True)
    L = ctypes.CDLL(lib)
    L.c_avg1v2d.restype = L.c_avg1v2d1g.restype = ctypes.c_double
    return L


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TLAB_REFERENCE", "/root/reference")
    out, index = {}, []
    dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    D = ctypes.c_double
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)

        def planes(ny):      # (nx factor, ny, j) of every call CAVG1V_N makes: the planes, then the volume as the box (nx*ny, 1, nz)
            return [(1, ny, j + 1) for j in range(ny)] + ([(ny, 1, 1)] if ny > 1 else [])

        def record(meta, res):
            out["out_%d" % len(index)] = res
            index.append(meta)

        for name, box in BOXES.items():
            nx, ny, nz = box
            F, gate = fields(box, 11 + len(name) + nx)
            for k, a in F.items():
                out["in_%s_%s" % (name, k)] = a
            out["in_%s_gate" % name] = gate
            F["c"], F["uv"] = constant_plane(F["u"]), F["u"] * F["v"]
            for fld in ("u", "q4", "i2"):
                res = np.zeros((4, 10, ny))
                for j in range(ny):
                    for m in range(1, 11):
                        res[0, m - 1, j] = L.c_avg1v2d(nx, ny, nz, j + 1, m, dp(F[fld]))
                        for lev in (1, 2, 3):
                            res[lev, m - 1, j] = L.c_avg1v2d1g(nx, ny, nz, j + 1, lev, m, dp(F[fld]), dp(gate))
                record({"kind": "moments", "box": name, "field": fld}, res)
            cases = [("u", "v", il, lo, hi, nb, 0) for il, lo, hi in ((1, 0.0, 0.0), (0, -0.5, 0.8)) for nb in NBINS] + \
                    [("u", "v", il, lo, hi, 32, 2) for il, lo, hi in ((1, 0.0, 0.0), (0, -0.5, 0.8))] + \
                    [("c", "v", 1, 0.0, 0.0, 32, 0), ("c", "v", 0, 0.75, 0.75, 32, 0), ("c", "v", 1, 0.0, 0.0, 32, 1)] + \
                    [("u", "q4", il, lo, hi, 32, ig) for il, lo, hi in ((1, 0.0, 0.0), (0, -0.5, 0.8)) for ig in (0, 1)] + \
                    [("q4", "i2", 0, -2.0, 2.0, 16, 0), ("q4", "i2", 1, 0.0, 0.0, 16, 3)]
            if name == "a":      # (the largest box leaves the two largest tables to the others: the file stays below pdfs_ref.npz)
                cases = [c for c in cases if not (c[5] == 100 and c[2] == 0)]
            for fld, afld, ilim, lo, hi, nb, igate in cases:
                res = np.zeros((ny + 1, nb + 2, 2))
                for row, (fx, ny_, j) in enumerate(planes(ny)):
                    pdf, avg = np.zeros(nb + 2), np.zeros(nb)
                    if igate:
                        L.c_cavg1v2d1g(ilim, nx * fx, ny_, nz, j, igate, dp(gate), D(lo), D(hi), dp(F[fld]), nb, dp(pdf), dp(F[afld]), dp(avg))
                    else:
                        L.c_cavg1v2d(ilim, nx * fx, ny_, nz, j, D(lo), D(hi), dp(F[fld]), nb, dp(pdf), dp(F[afld]), dp(avg))
                    res[row, :, 0] = pdf
                    res[row, :nb, 1] = avg
                record({"kind": "cavg1v", "box": name, "field": fld, "a": afld, "ilim": ilim, "umin": lo, "umax": hi, "nbins": nb, "igate": igate}, res)
            for afld, nb2 in (("uv", (8, 8)), ("uv", (32, 5)), ("uv", (1, 3)), ("q4", (8, 8))):
                if name == "a" and nb2 == (32, 5):
                    continue
                n = nb2[0] * nb2[1]
                res = np.zeros((ny + 1, n + 2 + 2 * nb2[0], 2))
                nbc = (ctypes.c_int * 2)(*nb2)
                for row, (fx, ny_, j) in enumerate(planes(ny)):
                    pdf, avg = np.zeros(res.shape[1]), np.zeros(n)
                    L.c_cavg2v2d(nx * fx, ny_, nz, j, dp(F["u"]), dp(F["v"]), nbc, dp(pdf), dp(F[afld]), dp(avg))
                    res[row, :, 0] = pdf
                    res[row, :n, 1] = avg
                record({"kind": "cavg2v", "box": name, "u": "u", "v": "v", "a": afld, "nbins": list(nb2)}, res)
        raw = np.array([0.3125, 1.75, -0.421875, 6.5, 2.25, 19.0, -7.125, 88.5, 3.0625, 410.0]) * np.random.default_rng(5).uniform(0.9, 1.1, 10)
        out["central_in"] = raw
        for nm in range(2, 11):
            res = np.zeros(10)
            res[:nm] = raw[:nm]
            L.c_raw_to_central(nm, dp(res))
            record({"kind": "central", "nm": nm}, res)
    out["index"] = np.array(json.dumps(index))
    for name, box in BOXES.items():
        out["box_%s" % name] = np.array(box)
    path = os.path.join(HERE, "conditional_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote conditional_ref.npz: %d records, %d bytes" % (len(index), os.path.getsize(path)))
