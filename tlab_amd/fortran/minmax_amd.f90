!########################################################################
! MINMAX (utils/minmax.f90 of the reference) for a host whose fields live in device memory: a replacement FILE for utils/minmax.f90 in the host's
! build, same name and signature.  The array is classified like the DAXPY / DSCAL guard (tlab_pointer_on_device): device memory is reduced by a
! kernel (tlab_device_minmax), host memory by the host loop; a host array never reaches a kernel.  The MPI_ALLREDUCE of the two scalars stays.
!########################################################################
subroutine MINMAX(imax, jmax, kmax, a, amn, amx)
    use TLab_Constants, only: wp, wi
    use TLab_AMD_C, only: tlab_minmax_any, TLab_AMD_Check
    use, intrinsic :: iso_c_binding
#ifdef USE_MPI
    use mpi_f08
#endif

    implicit none

    integer(wi) imax, jmax, kmax
    real(wp), target :: a(imax*jmax*kmax)
    real(wp) amn, amx

! -----------------------------------------------------------------------
#ifdef USE_MPI
    real(wp) pamn, pamx
    integer ims_err
#endif

! #######################################################################
    call TLab_AMD_Check(tlab_minmax_any(c_loc(a), int(imax, c_long_long)*int(jmax, c_long_long)*int(kmax, c_long_long), amn, amx), 'tlab_minmax_any')

#ifdef USE_MPI
    pamn = amn
    pamx = amx
    call MPI_ALLREDUCE(pamn, amn, 1, MPI_REAL8, MPI_MIN, MPI_COMM_WORLD, ims_err)
    call MPI_ALLREDUCE(pamx, amx, 1, MPI_REAL8, MPI_MAX, MPI_COMM_WORLD, ims_err)
#endif

    return
end subroutine MINMAX
