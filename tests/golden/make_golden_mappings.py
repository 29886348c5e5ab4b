#!/usr/bin/env python3
"""Golden vectors of the reference's field mappings, recorded from the reference's own code: mappings/fi_vectorcalculus.f90, fi_vorticity.f90,
fi_strain.f90 and fi_gradient.f90 are compiled where they lie, with amdflang, into a temporary directory outside the repository, behind the
stand-in modules and the small bind(C) driver below; the calls go through ctypes.  Only inputs and outputs are written:
tests/golden/mappings_ref.npz.  Never run by a test or by the build.

What the four files `use` is stood in for: FDM's g (an empty type), IBM_VARS with imode_ibm = 0, a stub IBM_BCS_FIELD, OPR_Elliptic with a stub
OPR_Poisson (FI_SOLENOIDAL alone calls it; it is not recorded), and an OPR_Partial whose X / Y / Z operators are the periodic one-point
difference f(i+1) - f(i) along their direction, OPR_P2 that difference taken twice.  Each stand-in result is one rounding, so numpy reproduces
the stand-in exactly (tests/mappings_oracle.py: standin_operators), and the records are the reference's compiled pointwise arithmetic and call
order end to end: a reassociation, a contraction or a statement the restatement orders differently changes bits here.

Boxes (9, 8, 6) and (5, 4, 3): 31 arrays of full-entropy doubles per point do not compress, and the file stays below pdfs_ref.npz.  Fields
u, v, w, p, s: uniform(-1, 1) + cos of the row index; s is set to a constant in a block of the box, so its gradient vanishes there and
FI_STRAIN_A takes its else-branch.  Records, one per box and routine, each a stack of the routine's outputs
(nout, n): P Q R STRAIN STRAIN_TENSOR CURL VORTICITY VORTICITY_PRODUCTION STRAIN_PRODUCTION GRADIENT GRADIENT_PRODUCTION STRAIN_A
VORTICITY_DIFFUSION STRAIN_DIFFUSION GRADIENT_DIFFUSION STRAIN_PRESSURE.  Run in the build container:
python3 tests/golden/make_golden_mappings.py [reference root]"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

STANDINS = """
module FDM
    implicit none
    type :: fdm_dt
        integer :: dir = 0
    end type fdm_dt
    type(fdm_dt) :: g(3)
end module
module IBM_VARS
    implicit none
    integer :: imode_ibm = 0
    logical :: ibm_partial = .false.
end module
module OPR_Elliptic
    use TLab_Constants, only: wp, wi
    implicit none
contains
    subroutine OPR_Poisson(nx, ny, nz, ibc, p, tmp1, tmp2, bcs_hb, bcs_ht)
        integer(wi) nx, ny, nz, ibc
        real(wp) p(*), tmp1(*), tmp2(*), bcs_hb(*), bcs_ht(*)
    end subroutine
end module
subroutine IBM_BCS_FIELD(a)
    use TLab_Constants, only: wp
    real(wp) a(*)
end subroutine
module OPR_Partial
    use TLab_Constants, only: wp, wi
    use FDM, only: fdm_dt
    implicit none
    integer(wi), parameter, public :: OPR_P1 = 1, OPR_P2 = 2, OPR_P2_P1 = 3, OPR_P1_INT_VP = 5, OPR_P1_INT_PV = 6
    integer(wi), parameter, public :: OPR_P0_INT_VP = 7, OPR_P0_INT_PV = 8
contains
    ! result(i) = u(i + 1) - u(i) along direction dir, periodic
    subroutine diff(dir, nx, ny, nz, u, result)
        integer(wi), intent(in) :: dir, nx, ny, nz
        real(wp), intent(in) :: u(nx, ny, nz)
        real(wp), intent(out) :: result(nx, ny, nz)
        integer(wi) i, j, k
        do k = 1, nz
            do j = 1, ny
                do i = 1, nx
                    select case (dir)
                    case (1)
                        result(i, j, k) = u(mod(i, nx) + 1, j, k) - u(i, j, k)
                    case (2)
                        result(i, j, k) = u(i, mod(j, ny) + 1, k) - u(i, j, k)
                    case default
                        result(i, j, k) = u(i, j, mod(k, nz) + 1) - u(i, j, k)
                    end select
                end do
            end do
        end do
    end subroutine
    subroutine partial(dir, type, nx, ny, nz, u, result)
        integer(wi), intent(in) :: dir, type, nx, ny, nz
        real(wp), intent(in) :: u(nx*ny*nz)
        real(wp), intent(out) :: result(nx*ny*nz)
        real(wp), allocatable :: first(:)
        if (type == OPR_P1) then
            call diff(dir, nx, ny, nz, u, result)
        else if (type == OPR_P2) then
            allocate (first(nx*ny*nz))
            call diff(dir, nx, ny, nz, u, first)
            call diff(dir, nx, ny, nz, first, result)
        else
            error stop 'stand-in OPR_Partial: type not stood in for'
        end if
    end subroutine
    subroutine OPR_Partial_X(type, nx, ny, nz, bcs, g, u, result, tmp1)
        integer(wi), intent(in) :: type, nx, ny, nz, bcs(:, :)
        type(fdm_dt), intent(in) :: g
        real(wp), intent(in) :: u(nx*ny*nz)
        real(wp), intent(out) :: result(nx*ny*nz)
        real(wp), intent(inout), optional :: tmp1(nx*ny*nz)
        call partial(1, type, nx, ny, nz, u, result)
    end subroutine
    subroutine OPR_Partial_Y(type, nx, ny, nz, bcs, g, u, result, tmp1)
        integer(wi), intent(in) :: type, nx, ny, nz, bcs(:, :)
        type(fdm_dt), intent(in) :: g
        real(wp), intent(in) :: u(nx*ny*nz)
        real(wp), intent(out) :: result(nx*ny*nz)
        real(wp), intent(inout), optional :: tmp1(nx*ny*nz)
        call partial(2, type, nx, ny, nz, u, result)
    end subroutine
    subroutine OPR_Partial_Z(type, nx, ny, nz, bcs, g, u, result, tmp1)
        integer(wi), intent(in) :: type, nx, ny, nz, bcs(:, :)
        type(fdm_dt), intent(in) :: g
        real(wp), intent(in) :: u(nx*ny*nz)
        real(wp), intent(out) :: result(nx*ny*nz)
        real(wp), intent(inout), optional :: tmp1(nx*ny*nz)
        call partial(3, type, nx, ny, nz, u, result)
    end subroutine
end module
"""

# every routine behind one entry: o(n, *) takes the outputs in the order of tlab_amd_mappings.h, t(n, 6) is work space
DRIVER = """
subroutine c_mapping(id, nx, ny, nz, u, v, w, p, s, o) bind(C, name='c_mapping')
    use iso_c_binding
    use FI_VECTORCALCULUS
    use FI_VORTICITY_EQN
    use FI_STRAIN_EQN
    use FI_GRADIENT_EQN
    implicit none
    integer(c_int), value :: id, nx, ny, nz
    real(c_double) :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz), p(nx*ny*nz), s(nx*ny*nz), o(nx*ny*nz, 6)
    real(c_double), allocatable :: t(:, :)
    allocate (t(nx*ny*nz, 6))
    select case (id)
    case (0)
        call FI_INVARIANT_P(nx, ny, nz, u, v, w, o(:, 1), t(:, 1))
    case (1)
        call FI_INVARIANT_Q(nx, ny, nz, u, v, w, o(:, 1), t(:, 1), t(:, 2), t(:, 3))
    case (2)
        call FI_INVARIANT_R(nx, ny, nz, u, v, w, o(:, 1), t(:, 1), t(:, 2), t(:, 3), t(:, 4), t(:, 5))
    case (3)
        call FI_STRAIN(nx, ny, nz, u, v, w, o(:, 1), t(:, 1), t(:, 2))
    case (4)
        call FI_STRAIN_TENSOR(nx, ny, nz, u, v, w, o(:, 1), o(:, 2), o(:, 3), o(:, 4), o(:, 5), o(:, 6))
    case (5)
        call FI_CURL(nx, ny, nz, u, v, w, o(:, 1), o(:, 2), o(:, 3), o(:, 4))
    case (6)
        call FI_VORTICITY(nx, ny, nz, u, v, w, o(:, 1), t(:, 1), t(:, 2))
    case (7)
        call FI_VORTICITY_PRODUCTION(nx, ny, nz, u, v, w, o(:, 1), t(:, 1), t(:, 2), t(:, 3), t(:, 4), t(:, 5))
    case (8)
        call FI_STRAIN_PRODUCTION(nx, ny, nz, u, v, w, o(:, 1), t(:, 1), t(:, 2), t(:, 3), t(:, 4), t(:, 5))
    case (9)
        call FI_GRADIENT(nx, ny, nz, s, o(:, 1), t(:, 1))
    case (10)
        call FI_GRADIENT_PRODUCTION(nx, ny, nz, s, u, v, w, o(:, 1), t(:, 1), t(:, 2), t(:, 3), t(:, 4), t(:, 5))
    case (11)
        call FI_STRAIN_A(nx, ny, nz, s, u, v, w, o(:, 1), o(:, 2), t(:, 1), t(:, 2), t(:, 3), o(:, 3))
    case (12)
        call FI_VORTICITY_DIFFUSION(nx, ny, nz, u, v, w, o(:, 1), t(:, 1), t(:, 2), t(:, 3), t(:, 4), t(:, 5))
    case (13)
        call FI_STRAIN_DIFFUSION(nx, ny, nz, u, v, w, o(:, 1), t(:, 1), t(:, 2), t(:, 3), t(:, 4), t(:, 5))
    case (14)
        call FI_GRADIENT_DIFFUSION(nx, ny, nz, s, o(:, 1), t(:, 1), t(:, 2), t(:, 3), t(:, 4), t(:, 5))
    case (15)
        call FI_STRAIN_PRESSURE(nx, ny, nz, u, v, w, p, o(:, 1), t(:, 1), t(:, 2), t(:, 3), t(:, 4))
    end select
end subroutine
"""

BOXES = {"a": (9, 8, 6), "b": (5, 4, 3)}      # (nx, ny, nz)
ROUTINES = ("P", "Q", "R", "STRAIN", "STRAIN_TENSOR", "CURL", "VORTICITY", "VORTICITY_PRODUCTION", "STRAIN_PRODUCTION", "GRADIENT",
            "GRADIENT_PRODUCTION", "STRAIN_A", "VORTICITY_DIFFUSION", "STRAIN_DIFFUSION", "GRADIENT_DIFFUSION", "STRAIN_PRESSURE")
NOUT = {"STRAIN_TENSOR": 6, "CURL": 4, "STRAIN_A": 3}


def fields(box, seed):
    nx, ny, nz = box
    rng = np.random.default_rng(seed)
    off = np.cos(np.arange(ny))[None, :, None]
    F = {k: rng.uniform(-1, 1, (nz, ny, nx)) + off for k in ("u", "v", "w", "p", "s")}
    F["s"][: max(nz // 2, 2), : max(ny // 2, 2), : max(nx // 2, 2)] = 0.375      # a constant block: the gradient of s vanishes inside it
    return F


def build(ref, tmp):
    for name, text in (("standins.f90", STANDINS), ("driver.f90", DRIVER)):
        with open(os.path.join(tmp, name), "w") as f:
            f.write(text)
    src = os.path.join(ref, "src")
    files = [os.path.join(src, "base", "tlab_constants.f90"), os.path.join(tmp, "standins.f90")] + \
            [os.path.join(src, "mappings", f) for f in ("fi_vectorcalculus.f90", "fi_vorticity.f90", "fi_strain.f90", "fi_gradient.f90")] + \
            [os.path.join(tmp, "driver.f90")]
    lib = os.path.join(tmp, "libmappings_ref.so")
    subprocess.run(["amdflang", "-cpp", "-O2", "-fPIC", "-shared", "-I", os.path.join(src, "include"), "-module-dir", tmp, *files, "-o", lib],
                   cwd=tmp, check=True)
    return ctypes.CDLL(lib)


if __name__ == "__main__":
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TLAB_REFERENCE", "/root/reference")
    out = {}
    dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        L = build(ref, tmp)
        for name, box in BOXES.items():
            nx, ny, nz = box
            n = nx * ny * nz
            F = fields(box, 23 + nx)
            out["box_%s" % name] = np.array(box)
            for k, a in F.items():
                out["in_%s_%s" % (name, k)] = a
            for rid, routine in enumerate(ROUTINES):
                o = np.zeros((6, n))      # Fortran o(n, 6)
                L.c_mapping(rid, nx, ny, nz, dp(F["u"]), dp(F["v"]), dp(F["w"]), dp(F["p"]), dp(F["s"]), dp(o))
                out["out_%s_%s" % (name, routine)] = o[: NOUT.get(routine, 1)].copy()
    path = os.path.join(HERE, "mappings_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote mappings_ref.npz: %d records, %d bytes" % (len(BOXES) * len(ROUTINES), os.path.getsize(path)))
