#!/usr/bin/env python3
"""Golden vectors of the reference's module PDFS (utils/pdfs.f90): PDF1V2D, PDF1V2D1G, PDF2V2D and PDF_ANALIZE, recorded from the reference's own
code.  base/tlab_constants.f90 and utils/pdfs.f90 are compiled where they lie, with amdflang, into a temporary directory outside the repository,
behind the small bind(C) driver below; the calls go through ctypes.  Only inputs and outputs are written: tests/golden/pdfs_ref.npz.  Never run
by a test or by the build.

A few small boxes; nbins 1, 2, 32, 100; local and external intervals (one of them degenerate, one with integer data on bin edges, values at umax
and values slightly below umin); a constant plane; a gate with an empty plane and a one-point plane; every plane and the volume, which the
reference takes as the box (nx*ny, 1, nz).  The records are listed in the JSON string `index`: kind, box, field(s), parameters -> `out_<n>`.
Run in the build container:  python3 tests/golden/make_golden_pdfs.py [reference root]"""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

DRIVER = """
module pdfs_driver
    use iso_c_binding
    use PDFS
    implicit none
contains
    subroutine c_pdf1v2d(ilim, nx, ny, nz, j, umin, umax, u, nbins, pdf) bind(C, name='c_pdf1v2d')
        integer(c_int), value :: ilim, nx, ny, nz, j, nbins
        real(c_double), value :: umin, umax
        real(c_double) :: u(nx, ny, nz), pdf(nbins + 2), wrk(nbins)
        call PDF1V2D(ilim, nx, ny, nz, j, umin, umax, u, nbins, pdf, wrk)
    end subroutine
    subroutine c_pdf1v2d1g(ilim, nx, ny, nz, j, igate, gate, umin, umax, u, nbins, pdf) bind(C, name='c_pdf1v2d1g')
        integer(c_int), value :: ilim, nx, ny, nz, j, nbins, igate
        integer(c_int8_t) :: gate(nx, ny, nz)
        real(c_double), value :: umin, umax
        real(c_double) :: u(nx, ny, nz), pdf(nbins + 2), wrk(nbins)
        call PDF1V2D1G(ilim, nx, ny, nz, j, int(igate, 1), gate, umin, umax, u, nbins, pdf, wrk)
    end subroutine
    subroutine c_pdf2v2d(nx, ny, nz, j, u, v, nbins, pdf) bind(C, name='c_pdf2v2d')
        integer(c_int), value :: nx, ny, nz, j
        integer(c_int) :: nbins(2)
        real(c_double) :: u(nx, ny, nz), v(nx, ny, nz), pdf(nbins(1)*nbins(2) + 2 + 2*nbins(1)), wrk(nbins(1), max(nbins(2), 3))
        call PDF2V2D(nx, ny, nz, j, u, v, nbins, pdf, wrk)
    end subroutine
    subroutine c_pdf_analize(ibc, nbins, pdf, umin, umax, plim, nplim) bind(C, name='c_pdf_analize')
        integer(c_int), value :: ibc, nbins
        real(c_double), value :: plim
        real(c_double) :: pdf(nbins + 2), umin, umax
        integer(c_int) :: nplim
        call PDF_ANALIZE(ibc, nbins, pdf, umin, umax, plim, nplim)
    end subroutine
end module
"""

BOXES = {"a": (20, 12, 8), "b": (7, 5, 3), "c": (6, 1, 4)}      # (nx, ny, nz)
NBINS = (1, 2, 32, 100)


def fields(box, seed):
    nx, ny, nz = box
    rng = np.random.default_rng(seed)
    off = np.cos(np.arange(ny))[None, :, None]
    u = rng.uniform(-1, 1, (nz, ny, nx)) + off
    v = rng.uniform(-1, 1, (nz, ny, nx)) + 0.5 * u
    c = rng.uniform(-1, 1, (nz, ny, nx)) + off
    c[:, ny // 2, :] = 0.75                                          # a constant plane
    w = rng.integers(-8, 9, (nz, ny, nx)).astype(np.float64)         # on the edges of 16 bins of [-8, 8]
    e = rng.uniform(0.0, 1.0, (nz, ny, nx))                          # for [0.25, 0.75]: values slightly below umin and above umax
    e.reshape(-1)[:4] = [0.25, 0.75, 0.25 - 1.0 / 256, 0.25 - 1.0 / 64]
    gate = (rng.uniform(size=(nz, ny, nx)) > 0.5).astype(np.int8)
    if ny > 2:
        gate[:, 1, :] = 0                                            # an empty plane
        gate[:, 2, :] = 0
        gate[nz // 2, 2, nx // 2] = 1                                # a one-point plane
    return {"u": u, "v": v, "c": c, "w": w, "e": e}, gate


def build(ref, tmp):
    with open(os.path.join(tmp, "driver.f90"), "w") as f:
        f.write(DRIVER)
    src = [os.path.join(ref, "src", "base", "tlab_constants.f90"), os.path.join(ref, "src", "utils", "pdfs.f90"), os.path.join(tmp, "driver.f90")]
    lib = os.path.join(tmp, "libpdfs_ref.so")
    subprocess.run(["amdflang", "-cpp", "-O2", "-fPIC", "-shared", "-module-dir", tmp, *src, "-o", lib], cwd=tmp, check=True)
    return ctypes.CDLL(lib)


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TLAB_REFERENCE", "/root/reference")
    out, index = {}, []
    dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    D = ctypes.c_double
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)

        def planes(ny):      # (nx factor, ny, j) of every call PDF1V_N makes: the planes, then the volume as the box (nx*ny, 1, nz)
            return [(1, ny, j + 1) for j in range(ny)] + ([(ny, 1, 1)] if ny > 1 else [])

        def record(meta, res):
            out["out_%d" % len(index)] = res
            index.append(meta)

        for name, box in BOXES.items():
            nx, ny, nz = box
            F, gate = fields(box, 7 + len(name) + nx)
            for k, a in F.items():
                out["in_%s_%s" % (name, k)] = a
            out["in_%s_gate" % name] = gate
            cases = [("u", 1, 0.0, 0.0, nb) for nb in NBINS] + [("u", 0, -0.5, 0.8, nb) for nb in NBINS] + \
                    [("c", 1, 0.0, 0.0, 32), ("c", 0, 0.75, 0.75, 32), ("w", 0, -8.0, 8.0, 16), ("w", 1, 0.0, 0.0, 16), ("e", 0, 0.25, 0.75, 8)]
            for fld, ilim, lo, hi, nb in cases:
                for gated in (0, 1):
                    res = np.zeros((ny + 1, nb + 2))
                    for row, (fx, ny_, j) in enumerate(planes(ny)):
                        pdf = np.zeros(nb + 2)
                        if gated:
                            L.c_pdf1v2d1g(ilim, nx * fx, ny_, nz, j, 1, dp(gate), D(lo), D(hi), dp(F[fld]), nb, dp(pdf))
                        else:
                            L.c_pdf1v2d(ilim, nx * fx, ny_, nz, j, D(lo), D(hi), dp(F[fld]), nb, dp(pdf))
                        res[row] = pdf
                    record({"kind": "pdf1v", "box": name, "field": fld, "ilim": ilim, "umin": lo, "umax": hi, "nbins": nb, "igate": gated}, res)
                    if fld == "u" and ilim == 1:
                        for ibc in range(4):
                            ana = np.zeros((ny + 1, 3))
                            for row in range(len(planes(ny))):
                                a, b, n = D(0.0), D(0.0), ctypes.c_int(0)
                                L.c_pdf_analize(ibc, nb, dp(np.ascontiguousarray(res[row])), ctypes.byref(a), ctypes.byref(b), D(1.0e-4), ctypes.byref(n))
                                ana[row] = a.value, b.value, n.value
                            record({"kind": "analize", "box": name, "of": len(index) - 1 - ibc, "ibc": ibc, "nbins": nb, "plim": 1.0e-4}, ana)
            for nb2 in ((8, 8), (32, 5), (1, 3)):
                res = np.zeros((ny + 1, nb2[0] * nb2[1] + 2 + 2 * nb2[0]))
                nbc = (ctypes.c_int * 2)(*nb2)
                for row, (fx, ny_, j) in enumerate(planes(ny)):
                    pdf = np.zeros(res.shape[1])
                    L.c_pdf2v2d(nx * fx, ny_, nz, j, dp(F["u"]), dp(F["v"]), nbc, dp(pdf))
                    res[row] = pdf
                record({"kind": "pdf2v", "box": name, "u": "u", "v": "v", "nbins": list(nb2)}, res)
    out["index"] = np.array(json.dumps(index))
    for name, box in BOXES.items():
        out["box_%s" % name] = np.array(box)
    np.savez_compressed(os.path.join(HERE, "pdfs_ref.npz"), **out)
    print("wrote pdfs_ref.npz: %d records" % len(index))
