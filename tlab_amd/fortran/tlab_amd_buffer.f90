!########################################################################
! The relaxation buffer zones of the reference (tools/dns/boundary_buffer.f90, [BufferZone] Type = relaxation) on the device, for a host whose
! boundary_buffer.f90 went through boundary_buffer_device.sed:
!   TLab_AMD_Buffer_Push        hands one block (item%tau, item%ref as INI_BLOCK made them) to the driver, which copies them into device memory and
!                               applies the flow blocks inside its RHS and the scalar blocks inside its substep, in the reference's places;
!   TLab_AMD_Buffer_Relax_Scal  BOUNDARY_BUFFER_RELAX_SCAL: one tlab_deferred_relax_scal -- with the deferred tail on it is recorded after the RHS and
!                               becomes part of the one fused substep (csrc/deferred.cpp); off, it runs on the current stream.
! The host never touches hs itself.  dns: the driver's handle (TLab_AMD_DNS_Handle() of tlab_amd_dns.f90; the recipe passes it, so that this module
! depends on the C interfaces alone).
!########################################################################
module TLab_AMD_Buffer
    use TLab_AMD_C
    implicit none
    private
    public :: TLab_AMD_Buffer_Push, TLab_AMD_Buffer_Relax_Scal
    integer, parameter, public :: TLAB_AMD_BUFFER_IMIN = 1, TLAB_AMD_BUFFER_IMAX = 2, TLAB_AMD_BUFFER_JMIN = 3, TLAB_AMD_BUFFER_JMAX = 4
    integer, parameter, public :: TLAB_AMD_BUFFER_FLOW = 0, TLAB_AMD_BUFFER_SCAL = 1

contains

    ! iend: TLAB_AMD_BUFFER_*MIN / *MAX (the I ends are refused by the library: x is periodic there); group: _FLOW / _SCAL; tau(size, nfields) and
    ! ref(imax, size, kmax, nfields) in HOST memory; size = 0 switches the block off (tau, ref are not looked at)
    subroutine TLab_AMD_Buffer_Push(dns, iend, group, size, nfields, tau, ref)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: iend, group, size, nfields
        real(c_double), intent(in), target :: tau(*), ref(*)

        if (size <= 0) then
            call TLab_AMD_Check(tlab_dns_set_buffer_zone(dns, int(iend, c_int), int(group, c_int), 0_c_int, int(nfields, c_int), c_null_ptr, c_null_ptr), &
                                'tlab_dns_set_buffer_zone')
        else
            call TLab_AMD_Check(tlab_dns_set_buffer_zone(dns, int(iend, c_int), int(group, c_int), int(size, c_int), int(nfields, c_int), &
                                                         c_loc(tau), c_loc(ref)), 'tlab_dns_set_buffer_zone')
        end if
    end subroutine TLab_AMD_Buffer_Push

    subroutine TLab_AMD_Buffer_Relax_Scal(dns)
        type(c_ptr), intent(in) :: dns

        call TLab_AMD_Check(tlab_deferred_relax_scal(dns), 'tlab_deferred_relax_scal')
    end subroutine TLab_AMD_Buffer_Relax_Scal

end module TLab_AMD_Buffer
