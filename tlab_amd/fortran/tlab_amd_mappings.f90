!########################################################################
! The field mappings of the reference (mappings/fi_strain.f90, fi_vectorcalculus.f90, fi_vorticity.f90, fi_gradient.f90) for a host whose fields
! live in device memory: every routine has the reference's argument list behind the driver's handle dns (TLab_AMD_DNS_Handle(), whose plans
! are g(1:3)).
!   The first-derivative routines -- TLab_AMD_FI_Strain, _Strain_Tensor, _Curl, _Invariant_Q, _Invariant_R, _Vorticity_Production,
!   _Strain_Production, _Gradient_Production, _Strain_A -- take the nine velocity gradients (and the scalar's three) once and make ONE pass over
!   them (tlab_dns_fi_maps) where the reference differentiates for every statement.  The gradients go into device arrays this module owns, made on
!   first use and kept (TLab_AMD_Mappings_Free gives them back); the scalar gradient goes where the reference leaves it (grad_x .. grad_z,
!   normal1 .. normal3).
!   The diffusion and pressure terms -- TLab_AMD_FI_Vorticity_Diffusion, _Strain_Diffusion, _Gradient_Diffusion, _Strain_Pressure -- make the
!   reference's OPR_Partial calls in the reference's order on the caller's work arrays (tlab_dns_fi_diffusion).
! What the reference returns in a work array is returned: FI_CURL's tmp (the squared magnitude), FI_STRAIN_A's tmp1 (grad(a).grad(a)) and its
! normals.  The contents of every other work array are unspecified on return.  Device arrays throughout.  It depends on TLab_AMD_C alone.
!########################################################################
module TLab_AMD_Mappings
    use TLab_AMD_C
    implicit none
    private
    public :: TLab_AMD_FI_Strain, TLab_AMD_FI_Strain_Tensor, TLab_AMD_FI_Curl, TLab_AMD_FI_Invariant_Q, TLab_AMD_FI_Invariant_R
    public :: TLab_AMD_FI_Vorticity_Production, TLab_AMD_FI_Vorticity_Diffusion
    public :: TLab_AMD_FI_Strain_Production, TLab_AMD_FI_Strain_Diffusion, TLab_AMD_FI_Strain_Pressure
    public :: TLab_AMD_FI_Gradient_Production, TLab_AMD_FI_Gradient_Diffusion, TLab_AMD_FI_Strain_A
    public :: TLab_AMD_Mappings_Free

    ! the TLAB_MAP_* and TLAB_FI_* codes of tlab_amd_mappings.h
    integer(c_int), parameter :: MAP_Q = 1, MAP_R = 2, MAP_STRAIN = 3, MAP_STRAIN_TENSOR = 4, MAP_CURL = 5, MAP_VORTICITY_PRODUCTION = 7
    integer(c_int), parameter :: MAP_STRAIN_PRODUCTION = 8, MAP_GRADIENT_PRODUCTION = 10, MAP_STRAIN_A = 11
    integer(c_int), parameter :: FI_VORTICITY_DIFFUSION = 0, FI_STRAIN_DIFFUSION = 1, FI_GRADIENT_DIFFUSION = 2, FI_STRAIN_PRESSURE = 3

    type(c_ptr), save :: grad9(9) = c_null_ptr      ! the nine velocity gradients: device arrays of grad_n doubles
    integer(c_size_t), save :: grad_n = 0

contains
    subroutine Gradient_Arrays(n)
        integer, intent(in) :: n
        integer i
        if (int(n, c_size_t) <= grad_n) return
        call TLab_AMD_Mappings_Free()
        do i = 1, 9
            call TLab_AMD_Check(tlab_malloc(grad9(i), int(n, c_size_t)*8_c_size_t), 'tlab_malloc')
        end do
        grad_n = int(n, c_size_t)
    end subroutine Gradient_Arrays

    subroutine TLab_AMD_Mappings_Free()
        integer i
        do i = 1, 9
            if (c_associated(grad9(i))) call TLab_AMD_Check(tlab_free(grad9(i)), 'tlab_free')
            grad9(i) = c_null_ptr
        end do
        grad_n = 0
    end subroutine TLab_AMD_Mappings_Free

    ! one map of the velocity gradients alone into out(1:nout)
    subroutine Velocity_Map(dns, n, u, v, w, map, out)
        type(c_ptr), intent(in) :: dns, out(:)
        integer, intent(in) :: n
        real(c_double), intent(in), target :: u(n), v(n), w(n)
        integer(c_int), intent(in) :: map
        type(c_ptr) :: q(3)
        call Gradient_Arrays(n)
        q = [c_loc(u), c_loc(v), c_loc(w)]
        call TLab_AMD_Check(tlab_dns_fi_maps(dns, q, c_null_ptr, [map], 1_c_int, grad9, c_null_ptr, out), 'tlab_dns_fi_maps')
    end subroutine Velocity_Map

    ! ... and of the scalar gradient too, which stays in ds3
    subroutine Scalar_Map(dns, n, s, u, v, w, map, ds3, out)
        type(c_ptr), intent(in) :: dns, out(:)
        type(c_ptr), intent(in), target :: ds3(3)
        integer, intent(in) :: n
        real(c_double), intent(in), target :: s(n), u(n), v(n), w(n)
        integer(c_int), intent(in) :: map
        type(c_ptr) :: q(3)
        call Gradient_Arrays(n)
        q = [c_loc(u), c_loc(v), c_loc(w)]
        call TLab_AMD_Check(tlab_dns_fi_maps(dns, q, c_loc(s), [map], 1_c_int, grad9, c_loc(ds3), out), 'tlab_dns_fi_maps')
    end subroutine Scalar_Map

    subroutine Diffusion(dns, kind, n, u, v, w, f, result, work)
        type(c_ptr), intent(in) :: dns, f, result, work(5)
        integer(c_int), intent(in) :: kind
        integer, intent(in) :: n
        real(c_double), intent(in), target :: u(n), v(n), w(n)
        type(c_ptr), target :: q(3)
        type(c_ptr) :: work6(6)
        call Gradient_Arrays(n)
        q = [c_loc(u), c_loc(v), c_loc(w)]
        work6(1:5) = work
        work6(6) = grad9(1)                             ! (the sixth work array of tlab_dns_fi_diffusion is not touched)
        call TLab_AMD_Check(tlab_dns_fi_diffusion(dns, kind, c_loc(q), f, result, work6), 'tlab_dns_fi_diffusion')
    end subroutine Diffusion

    ! ---- fi_strain.f90 ----
    subroutine TLab_AMD_FI_Strain(dns, nx, ny, nz, u, v, w, result, tmp1, tmp2)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)
        real(c_double), intent(inout), target :: tmp1(nx*ny*nz), tmp2(nx*ny*nz)
        call Velocity_Map(dns, nx*ny*nz, u, v, w, MAP_STRAIN, [c_loc(result)])
    end subroutine TLab_AMD_FI_Strain

    subroutine TLab_AMD_FI_Strain_Tensor(dns, nx, ny, nz, u, v, w, tmp1, tmp2, tmp3, tmp4, tmp5, tmp6)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: tmp1(nx*ny*nz), tmp2(nx*ny*nz), tmp3(nx*ny*nz), tmp4(nx*ny*nz), tmp5(nx*ny*nz), tmp6(nx*ny*nz)
        call Velocity_Map(dns, nx*ny*nz, u, v, w, MAP_STRAIN_TENSOR, &
                          [c_loc(tmp1), c_loc(tmp2), c_loc(tmp3), c_loc(tmp4), c_loc(tmp5), c_loc(tmp6)])
    end subroutine TLab_AMD_FI_Strain_Tensor

    subroutine TLab_AMD_FI_Strain_Production(dns, nx, ny, nz, u, v, w, result, s_12, s_13, s_23, tmp1, tmp2)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)
        real(c_double), intent(inout), target :: s_12(nx*ny*nz), s_13(nx*ny*nz), s_23(nx*ny*nz), tmp1(nx*ny*nz), tmp2(nx*ny*nz)
        call Velocity_Map(dns, nx*ny*nz, u, v, w, MAP_STRAIN_PRODUCTION, [c_loc(result)])
    end subroutine TLab_AMD_FI_Strain_Production

    subroutine TLab_AMD_FI_Strain_Diffusion(dns, nx, ny, nz, u, v, w, result, strain, tmp1, tmp2, tmp3, tmp4)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)
        real(c_double), intent(inout), target :: strain(nx*ny*nz), tmp1(nx*ny*nz), tmp2(nx*ny*nz), tmp3(nx*ny*nz), tmp4(nx*ny*nz)
        call Diffusion(dns, FI_STRAIN_DIFFUSION, nx*ny*nz, u, v, w, c_null_ptr, c_loc(result), &
                       [c_loc(strain), c_loc(tmp1), c_loc(tmp2), c_loc(tmp3), c_loc(tmp4)])
    end subroutine TLab_AMD_FI_Strain_Diffusion

    subroutine TLab_AMD_FI_Strain_Pressure(dns, nx, ny, nz, u, v, w, p, result, tmp1, tmp2, tmp3, tmp4)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz), p(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)
        real(c_double), intent(inout), target :: tmp1(nx*ny*nz), tmp2(nx*ny*nz), tmp3(nx*ny*nz), tmp4(nx*ny*nz)
        call Gradient_Arrays(nx*ny*nz)                  ! (the term has no field array: the first work array is one of the module's)
        call Diffusion(dns, FI_STRAIN_PRESSURE, nx*ny*nz, u, v, w, c_loc(p), c_loc(result), &
                       [grad9(2), c_loc(tmp1), c_loc(tmp2), c_loc(tmp3), c_loc(tmp4)])
    end subroutine TLab_AMD_FI_Strain_Pressure

    subroutine TLab_AMD_FI_Strain_A(dns, nx, ny, nz, a, u, v, w, strain1, strain2, normal1, normal2, normal3, tmp1)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: a(nx*ny*nz), u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: strain1(nx*ny*nz), strain2(nx*ny*nz), normal1(nx*ny*nz), normal2(nx*ny*nz), normal3(nx*ny*nz)
        real(c_double), intent(out), target :: tmp1(nx*ny*nz)      ! returns grad(a).grad(a)
        call Scalar_Map(dns, nx*ny*nz, a, u, v, w, MAP_STRAIN_A, [c_loc(normal1), c_loc(normal2), c_loc(normal3)], &
                        [c_loc(strain1), c_loc(strain2), c_loc(tmp1)])
    end subroutine TLab_AMD_FI_Strain_A

    ! ---- fi_vectorcalculus.f90 ----
    subroutine TLab_AMD_FI_Curl(dns, nx, ny, nz, u, v, w, wx, wy, wz, tmp)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: wx(nx*ny*nz), wy(nx*ny*nz), wz(nx*ny*nz), tmp(nx*ny*nz)      ! tmp returns wx*wx + wy*wy + wz*wz
        call Velocity_Map(dns, nx*ny*nz, u, v, w, MAP_CURL, [c_loc(wx), c_loc(wy), c_loc(wz), c_loc(tmp)])
    end subroutine TLab_AMD_FI_Curl

    subroutine TLab_AMD_FI_Invariant_Q(dns, nx, ny, nz, u, v, w, result, tmp1, tmp2, tmp3)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)
        real(c_double), intent(inout), target :: tmp1(nx*ny*nz), tmp2(nx*ny*nz), tmp3(nx*ny*nz)
        call Velocity_Map(dns, nx*ny*nz, u, v, w, MAP_Q, [c_loc(result)])
    end subroutine TLab_AMD_FI_Invariant_Q

    subroutine TLab_AMD_FI_Invariant_R(dns, nx, ny, nz, u, v, w, result, tmp1, tmp2, tmp3, tmp4, tmp5)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)
        real(c_double), intent(inout), target :: tmp1(nx*ny*nz), tmp2(nx*ny*nz), tmp3(nx*ny*nz), tmp4(nx*ny*nz), tmp5(nx*ny*nz)
        call Velocity_Map(dns, nx*ny*nz, u, v, w, MAP_R, [c_loc(result)])
    end subroutine TLab_AMD_FI_Invariant_R

    ! ---- fi_vorticity.f90 ----
    subroutine TLab_AMD_FI_Vorticity_Production(dns, nx, ny, nz, u, v, w, result, vort_x, vort_y, vort_z, tmp1, tmp2)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)
        real(c_double), intent(inout), target :: vort_x(nx*ny*nz), vort_y(nx*ny*nz), vort_z(nx*ny*nz), tmp1(nx*ny*nz), tmp2(nx*ny*nz)
        call Velocity_Map(dns, nx*ny*nz, u, v, w, MAP_VORTICITY_PRODUCTION, [c_loc(result)])
    end subroutine TLab_AMD_FI_Vorticity_Production

    subroutine TLab_AMD_FI_Vorticity_Diffusion(dns, nx, ny, nz, u, v, w, result, vort, tmp1, tmp2, tmp3, tmp4)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)
        real(c_double), intent(inout), target :: vort(nx*ny*nz), tmp1(nx*ny*nz), tmp2(nx*ny*nz), tmp3(nx*ny*nz), tmp4(nx*ny*nz)
        call Diffusion(dns, FI_VORTICITY_DIFFUSION, nx*ny*nz, u, v, w, c_null_ptr, c_loc(result), &
                       [c_loc(vort), c_loc(tmp1), c_loc(tmp2), c_loc(tmp3), c_loc(tmp4)])
    end subroutine TLab_AMD_FI_Vorticity_Diffusion

    ! ---- fi_gradient.f90 ----
    subroutine TLab_AMD_FI_Gradient_Production(dns, nx, ny, nz, s, u, v, w, result, grad_x, grad_y, grad_z, tmp1, tmp2)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: s(nx*ny*nz), u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)
        real(c_double), intent(inout), target :: grad_x(nx*ny*nz), grad_y(nx*ny*nz), grad_z(nx*ny*nz), tmp1(nx*ny*nz), tmp2(nx*ny*nz)
        call Scalar_Map(dns, nx*ny*nz, s, u, v, w, MAP_GRADIENT_PRODUCTION, [c_loc(grad_x), c_loc(grad_y), c_loc(grad_z)], [c_loc(result)])
    end subroutine TLab_AMD_FI_Gradient_Production

    subroutine TLab_AMD_FI_Gradient_Diffusion(dns, nx, ny, nz, s, result, grad, tmp1, tmp2, tmp3, tmp4)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: s(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)
        real(c_double), intent(inout), target :: grad(nx*ny*nz), tmp1(nx*ny*nz), tmp2(nx*ny*nz), tmp3(nx*ny*nz), tmp4(nx*ny*nz)
        type(c_ptr) :: work6(6)
        call Gradient_Arrays(nx*ny*nz)
        work6 = [c_loc(grad), c_loc(tmp1), c_loc(tmp2), c_loc(tmp3), c_loc(tmp4), grad9(1)]
        call TLab_AMD_Check(tlab_dns_fi_diffusion(dns, FI_GRADIENT_DIFFUSION, c_null_ptr, c_loc(s), c_loc(result), work6), &
                            'tlab_dns_fi_diffusion')
    end subroutine TLab_AMD_FI_Gradient_Diffusion

end module TLab_AMD_Mappings
