!########################################################################
! DNS_BOUNDS_LIMIT (tools/dns/dns_local.f90:67-90 of the reference) on device memory: the scalar loop of the host's routine, turned into a call of
! this subroutine by dns_local_device.sed.  One tlab_deferred_clip per active scalar: with the deferred tail on it is recorded after the DAXPYs of
! the substep and becomes part of the one fused substep (csrc/deferred.cpp); off, it runs as tlab_pw_clip on the current stream.  The host never
! touches the arrays itself.
!########################################################################
module TLab_AMD_Bounds
    use TLab_AMD_C
    implicit none
    private
    public :: TLab_AMD_Bounds_Limit

contains

    ! s(n, nscal) in device memory; per scalar: active, and the bounds smin <= smax (bound_s(is)%active, %min, %max of the host)
    subroutine TLab_AMD_Bounds_Limit(s, n, nscal, active, smin, smax)
        integer, intent(in) :: n, nscal
        real(c_double), intent(inout), target :: s(n, nscal)
        logical, intent(in) :: active(nscal)
        real(c_double), intent(in) :: smin(nscal), smax(nscal)
        integer is

        do is = 1, nscal
            if (active(is)) then
                call TLab_AMD_Check(tlab_deferred_clip(int(n, c_long_long), smin(is), smax(is), c_loc(s(1, is))), 'tlab_deferred_clip')
            end if
        end do
    end subroutine TLab_AMD_Bounds_Limit

end module TLab_AMD_Bounds
