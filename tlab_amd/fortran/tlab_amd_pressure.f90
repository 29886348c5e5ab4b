!########################################################################
! FI_PRESSURE_BOUSSINESQ (src/physics/fi_pressure_boussinesq.f90:8-280) for a host whose arrays live in device memory:
!   TLab_AMD_FI_Pressure_Boussinesq  the reference's argument list -- q, s, p, tmp1, tmp2, tmp, decomposition -- behind the driver's handle and
!                                    followed by what the reference reads from TLab_Memory: the leading dimension of the caller's tmp (the
!                                    distance between two of its arrays: isize_txc_field for txc(1, 4)) and how many arrays it holds
!                                    (inb_txc - 3).  One call of tlab_dns_pressure: the Burgers, forcing and Poisson stages of the device
!                                    substep on tmp(:, 1:3) as the three sums, with p as the forcing array.  A decomposition the device does not
!                                    carry stops the run there (TLab_AMD_Check).
! The host never touches the arrays itself; the call returns with the launches enqueued.  dns: TLab_AMD_DNS_Handle() of tlab_amd_dns.f90; the
! recipe passes it (INTEGRATION.md), so that this module depends on the C interfaces alone.
!########################################################################
module TLab_AMD_Pressure
    use TLab_AMD_C
    implicit none
    private
    public :: TLab_AMD_FI_Pressure_Boussinesq

    integer, parameter :: MAXA = 32

contains
    subroutine TLab_AMD_FI_Pressure_Boussinesq(dns, q, s, p, tmp1, tmp2, tmp, decomposition, ldtmp, ntmp)
        type(c_ptr), intent(in) :: dns
        real(c_double), intent(in), target :: q(*), s(*)
        real(c_double), intent(inout), target :: p(*), tmp1(*), tmp2(*), tmp(*)
        integer, intent(in) :: decomposition, ldtmp, ntmp

        type(c_ptr) :: pq(3), ps(MAXA), pt(MAXA)
        integer(c_long_long) :: n
        integer :: ns, i

        n = tlab_dns_info(dns, 4_c_int)
        ns = int(tlab_dns_info(dns, 5_c_int))      ! inb_scal_array: with a mixture s carries the liquid behind the scalars
        if (n <= 0 .or. ns > MAXA .or. ntmp > MAXA .or. ldtmp < n) then
            call TLab_AMD_Check(-1_c_int, 'TLab_AMD_FI_Pressure_Boussinesq: bad handle, too many arrays or ldtmp below the field size')
        end if
        do i = 1, 3
            pq(i) = c_loc(q(1 + (i - 1)*n))
        end do
        ps = c_null_ptr
        do i = 1, ns
            ps(i) = c_loc(s(1 + (i - 1)*n))
        end do
        pt = c_null_ptr
        do i = 1, ntmp
            pt(i) = c_loc(tmp(1 + int(i - 1, c_long_long)*ldtmp))
        end do
        call TLab_AMD_Check(tlab_dns_pressure(dns, int(decomposition, c_int), pq, ps, c_loc(p), c_loc(tmp1), c_loc(tmp2), pt, int(ntmp, c_int)), &
                            'tlab_dns_pressure')
    end subroutine TLab_AMD_FI_Pressure_Boussinesq

end module TLab_AMD_Pressure
