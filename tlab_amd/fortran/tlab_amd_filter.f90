!########################################################################
! DNS_FILTER (tools/dns/dns_filter.f90; dns_main.f90 calls it every nitera_filter steps after TIME_RUNGEKUTTA) for a host whose fields live in
! device memory:
!   TLab_AMD_OPR_Filter_Fields   the loops `call OPR_FILTER(imax, jmax, kmax, FilterDomain, q(1, iq), txc)` (dns_filter.f90:69-74) as ONE call on
!                                nf fields that lie one behind the other: the directional branch of OPR_FILTER, x, y, z in that order, each
!                                repeat(d) times, in place and without txc (tlab_opr_filter_fields: the streaming kernels).  fx, fy, fz: the
!                                handles of tlab_filter_create for FilterDomain(1:3) after OPR_FILTER_INITIALIZE, c_null_ptr for DNS_FILTER_NONE
!   TLab_AMD_DNS_Set_Filter      FilterDomain of the device driver, once after FILTER_READBLOCK / OPR_FILTER_INITIALIZE; the handles stay the host's
!   TLab_AMD_DNS_Filter          call DNS_FILTER() becomes call TLab_AMD_DNS_Filter(dns, q, s): the filters on q(:, 1:3) and s(:, 1:inb_scal), then
!                                DNS_BOUNDS_LIMIT with the bounds the driver holds, then FI_DIAGNOSTIC where it holds a mixture.  The kin
!                                statistics of DNS_FILTER (FI_RTKE, FI_DISSIPATION, AVG_IK_V before and after) are not made here.
! A filter whose size is not the extent along its direction, and a Repeat below one, stop the run (TLab_AMD_Check) before anything is launched.
! Nothing here synchronises the stream.  dns: TLab_AMD_DNS_Handle() of tlab_amd_dns.f90; the recipe passes it (INTEGRATION.md), so that this
! module depends on the C interfaces alone.
!########################################################################
module TLab_AMD_Filter
    use TLab_AMD_C
    implicit none
    private
    public :: TLab_AMD_OPR_Filter_Fields, TLab_AMD_DNS_Set_Filter, TLab_AMD_DNS_Filter

    integer, parameter :: MAXA = 32

    interface
        integer(c_int) function tlab_opr_filter_fields(nx, ny, nz, fx, fy, fz, repeat, nf, u) bind(C, name='tlab_opr_filter_fields')
            import :: c_int, c_ptr
            integer(c_int), value :: nx, ny, nz, nf
            type(c_ptr), value :: fx, fy, fz
            integer(c_int), intent(in) :: repeat(3)
            type(c_ptr), intent(in) :: u(*)
        end function
        integer(c_int) function tlab_dns_set_filter(dns, fx, fy, fz, repeat) bind(C, name='tlab_dns_set_filter')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns, fx, fy, fz
            integer(c_int), intent(in) :: repeat(3)
        end function
        integer(c_int) function tlab_dns_filter(dns, q, s) bind(C, name='tlab_dns_filter')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
            type(c_ptr), intent(in) :: q(*), s(*)
        end function
    end interface

contains
    ! do iq = 1, inb_flow; call OPR_FILTER(imax, jmax, kmax, FilterDomain, q(1, iq), txc); end do becomes
    ! call TLab_AMD_OPR_Filter_Fields(imax, jmax, kmax, fx, fy, fz, FilterDomain(:)%repeat, inb_flow, q)
    subroutine TLab_AMD_OPR_Filter_Fields(nx, ny, nz, fx, fy, fz, repeat, nf, u)
        integer, intent(in) :: nx, ny, nz, repeat(3), nf
        type(c_ptr), intent(in) :: fx, fy, fz
        real(c_double), intent(inout), target :: u(nx*ny*nz, nf)
        type(c_ptr) :: pu(MAXA)
        integer :: i

        if (nf > MAXA) call TLab_AMD_Check(-1_c_int, 'TLab_AMD_OPR_Filter_Fields: too many fields')
        pu = c_null_ptr
        do i = 1, nf
            pu(i) = c_loc(u(1, i))
        end do
        call TLab_AMD_Check(tlab_opr_filter_fields(int(nx, c_int), int(ny, c_int), int(nz, c_int), fx, fy, fz, int(repeat, c_int), int(nf, c_int), pu), &
                            'tlab_opr_filter_fields')
    end subroutine TLab_AMD_OPR_Filter_Fields

    subroutine TLab_AMD_DNS_Set_Filter(dns, fx, fy, fz, repeat)
        type(c_ptr), intent(in) :: dns, fx, fy, fz
        integer, intent(in) :: repeat(3)

        call TLab_AMD_Check(tlab_dns_set_filter(dns, fx, fy, fz, int(repeat, c_int)), 'tlab_dns_set_filter')
    end subroutine TLab_AMD_DNS_Set_Filter

    subroutine TLab_AMD_DNS_Filter(dns, q, s)
        type(c_ptr), intent(in) :: dns
        real(c_double), intent(inout), target :: q(*), s(*)
        type(c_ptr) :: pq(3), ps(MAXA)
        integer(c_long_long) :: n
        integer :: ns, i

        n = tlab_dns_info(dns, 4_c_int)
        ns = int(tlab_dns_info(dns, 5_c_int))      ! inb_scal_array: with a mixture s carries the liquid behind the scalars
        if (n <= 0 .or. ns > MAXA) call TLab_AMD_Check(-1_c_int, 'TLab_AMD_DNS_Filter: bad handle or too many scalars')
        do i = 1, 3
            pq(i) = c_loc(q(1 + (i - 1)*n))
        end do
        ps = c_null_ptr
        do i = 1, ns
            ps(i) = c_loc(s(1 + (i - 1)*n))
        end do
        call TLab_AMD_Check(tlab_dns_filter(dns, pq, ps), 'tlab_dns_filter')
    end subroutine TLab_AMD_DNS_Filter

end module TLab_AMD_Filter
