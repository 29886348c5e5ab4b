!########################################################################
! The body forces of the reference (TLab_Sources_Flow, src/physics/tlab_sources.f90:36-92: Rotation_Coriolis, then hq_i = hq_i + g_i b with b of
! Gravity_Buoyancy) on the device, for a host whose tlab_sources.f90 went through tlab_sources_device.sed:
!   TLab_AMD_Sources_Flow  pushes [Rotation] and [BodyForce] to the driver when they differ from what it pushed last (tlab_dns_set_coriolis,
!                          tlab_dns_set_buoyancy: a type the device does not carry stops the run there), then one tlab_deferred_sources_flow -- with
!                          the deferred tail on it is kept as a marker and becomes part of the one fused substep with the RHS that follows
!                          (csrc/deferred.cpp); off, it runs on the current stream.
! The host never touches q, s, hq itself.  dns: the driver's handle (TLab_AMD_DNS_Handle() of tlab_amd_dns.f90; the recipe passes it, so that this
! module depends on the C interfaces alone).
!########################################################################
module TLab_AMD_Sources
    use TLab_AMD_C
    implicit none
    private
    public :: TLab_AMD_Sources_Flow

    integer, parameter :: MAXP = 32
    logical, save :: pushed = .false.
    type(c_ptr), save :: last_dns = c_null_ptr
    integer, save :: last_cor = -1, last_bod = -1, last_nscal = -1, last_inb = -1, last_np = -1, last_nb = -1
    real(c_double), save :: last_cv(3) = 0.0_c_double, last_cp(2) = 0.0_c_double, last_bv(3) = 0.0_c_double, last_bp(MAXP) = 0.0_c_double
    real(c_double), allocatable, save :: last_bb(:)

contains

    ! cor_*: coriolis%type, %vector (already divided by Rossby), %parameters; bod_*: buoyancy%type, %vector (already divided by Froude), %scalar(1),
    ! %parameters; inb_scal_array of TLab_Memory; bbackground(jmax) of module Gravity (not allocated: zeros); q, s, hq: the module arrays, in device memory
    subroutine TLab_AMD_Sources_Flow(dns, cor_type, cor_vector, cor_parameters, bod_type, bod_vector, bod_nscal, bod_parameters, inb_scal_array, &
                                     bbackground, q, s, hq)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: cor_type, bod_type, bod_nscal, inb_scal_array
        real(c_double), intent(in) :: cor_vector(3), cor_parameters(:), bod_vector(3), bod_parameters(:)
        real(c_double), intent(in), allocatable, target :: bbackground(:)
        real(c_double), intent(in), target :: q(*), s(*)
        real(c_double), intent(inout), target :: hq(*)

        type(c_ptr) :: pq(3), phq(3), ps(MAXP), pb
        real(c_double) :: cp(2), bp(MAXP)
        integer :: np, nb, ns, i
        integer(c_long_long) :: n
        logical :: same

        n = tlab_dns_info(dns, 4_c_int)
        ns = int(tlab_dns_info(dns, 3_c_int))
        if (n <= 0 .or. ns > MAXP) call TLab_AMD_Check(-1_c_int, 'TLab_AMD_Sources_Flow: bad handle or too many scalars')
        cp = 0.0_c_double
        cp(1:min(2, size(cor_parameters))) = cor_parameters(1:min(2, size(cor_parameters)))
        np = min(MAXP, size(bod_parameters))
        bp = 0.0_c_double
        bp(1:np) = bod_parameters(1:np)
        nb = 0
        if (allocated(bbackground)) nb = size(bbackground)

        same = pushed .and. c_associated(dns, last_dns) .and. cor_type == last_cor .and. bod_type == last_bod .and. bod_nscal == last_nscal .and. &
               inb_scal_array == last_inb .and. np == last_np .and. nb == last_nb
        if (same) same = all(cor_vector == last_cv) .and. all(cp == last_cp) .and. all(bod_vector == last_bv) .and. all(bp == last_bp)
        if (same .and. nb > 0) same = all(bbackground == last_bb)
        if (.not. same) then
            call TLab_AMD_Check(tlab_dns_set_coriolis(dns, int(cor_type, c_int), cor_vector, cp), 'tlab_dns_set_coriolis')
            pb = c_null_ptr
            if (nb > 0) pb = c_loc(bbackground)
            call TLab_AMD_Check(tlab_dns_set_buoyancy(dns, int(bod_type, c_int), bod_vector, int(bod_nscal, c_int), bp, int(np, c_int), &
                                                      int(inb_scal_array, c_int), pb), 'tlab_dns_set_buoyancy')
            pushed = .true.; last_dns = dns
            last_cor = cor_type; last_bod = bod_type; last_nscal = bod_nscal; last_inb = inb_scal_array; last_np = np; last_nb = nb
            last_cv = cor_vector; last_cp = cp; last_bv = bod_vector; last_bp = bp
            if (allocated(last_bb)) deallocate (last_bb)
            allocate (last_bb(nb))
            if (nb > 0) last_bb = bbackground
        end if

        do i = 1, 3
            pq(i) = c_loc(q(1 + (i - 1)*n)); phq(i) = c_loc(hq(1 + (i - 1)*n))
        end do
        ps = c_null_ptr
        do i = 1, ns
            ps(i) = c_loc(s(1 + (i - 1)*n))
        end do
        call TLab_AMD_Check(tlab_deferred_sources_flow(dns, pq, ps, phq), 'tlab_deferred_sources_flow')
    end subroutine TLab_AMD_Sources_Flow

end module TLab_AMD_Sources
