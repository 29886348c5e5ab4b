!########################################################################
! The Lagrangian particles of the reference (TIME_SUBSTEP_PARTICLE, src/tools/dns/time.f90:906-1070: RHS_PART_1, the update, the periodic wraps, the
! wall condition and LOCATE_Y; and the scaling of l_hq, :300-304) on the device, for a host whose l_q, l_hq and l_g%nodes live in device memory:
!   TLab_AMD_Substep_Particle  pushes [Particles] to the driver when it differs from what it pushed last (tlab_dns_set_particles: a type the device
!                              does not carry stops the run there), then one tlab_dns_substep_particle -- the whole body of TIME_SUBSTEP_PARTICLE
!                              and, with scale_tendencies, the l_hq loop of TIME_RUNGEKUTTA that follows it.
!   TLab_AMD_Locate_Particles  LOCATE_Y on its own (after Particle_Initialize_Fields or a restart).
!   TLab_AMD_Sort_Particles    tlab_dns_particle_sort with a scratch array this module keeps: every so many steps, never inside a substep.
! and the transfers between the particles and the grid, which the reference calls from the time loop and the statistics:
!   TLab_AMD_Field_To_Particle        FIELD_TO_PARTICLE of any fields (additive onto the particle arrays handed over).
!   TLab_AMD_Particle_To_Field        PARTICLE_TO_FIELD; periodic (default .true.) adds the seam's contributions to column / plane 1.
!   TLab_AMD_Trajectories_Set         l_traj_tags of ParticleTrajectories_Initialize to the driver.
!   TLab_AMD_Trajectories_Accumulate  the body of ParticleTrajectories_Accumulate behind "counter = counter + 1", l_traj in device memory.
! The host never touches l_q, l_hq or the nodes itself between IO.  dns: the driver's handle (TLab_AMD_DNS_Handle() of tlab_amd_dns.f90; the recipe
! passes it, so that this module depends on the C interfaces alone).  The particle substep reads q and goes BEFORE the flow substep of the same stage
! (time.f90:231-233); with the deferred tail on, a recorded substep runs first.
!########################################################################
module TLab_AMD_Particles
    use TLab_AMD_C
    implicit none
    private
    public :: TLab_AMD_Substep_Particle, TLab_AMD_Locate_Particles, TLab_AMD_Sort_Particles
    public :: TLab_AMD_Field_To_Particle, TLab_AMD_Particle_To_Field, TLab_AMD_Trajectories_Set, TLab_AMD_Trajectories_Accumulate

    integer, parameter :: MAXC = 6                       ! inb_part of the types the device carries: 3 (tracer), 6 (inertia)
    logical, save :: pushed = .false.
    type(c_ptr), save :: last_dns = c_null_ptr
    integer, save :: last_type = -1, last_bcs = -1
    real(c_double), save :: last_stokes = 0.0_c_double, last_settling = 0.0_c_double
    type(c_ptr), save :: scratch = c_null_ptr
    integer(c_long_long), save :: scratch_bytes = 0_c_long_long

    interface
        integer(c_int) function tlab_dns_set_particles(dns, itype, bcs, stokes, settling) bind(C, name='tlab_dns_set_particles')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: dns
            integer(c_int), value :: itype, bcs
            real(c_double), value :: stokes, settling
        end function
        integer(c_int) function tlab_dns_particle_locate(dns, np, y_part, nodes) bind(C, name='tlab_dns_particle_locate')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: dns, y_part, nodes
            integer(c_long_long), value :: np
        end function
        integer(c_int) function tlab_dns_substep_particle(dns, dte, kco, scale_tendencies, np, q, l_q, l_hq, nodes) &
            bind(C, name='tlab_dns_substep_particle')
            import :: c_int, c_ptr, c_double, c_long_long
            type(c_ptr), value :: dns, nodes
            real(c_double), value :: dte, kco
            integer(c_int), value :: scale_tendencies
            integer(c_long_long), value :: np
            type(c_ptr), intent(in) :: q(*), l_q(*), l_hq(*)
        end function
        integer(c_int) function tlab_dns_particle_sort(dns, np, l_q, l_hq, nodes, tags, scratch, scratch_bytes, scratch_needed) &
            bind(C, name='tlab_dns_particle_sort')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: dns, nodes, tags, scratch
            integer(c_long_long), value :: np, scratch_bytes
            type(c_ptr), intent(in) :: l_q(*), l_hq(*)
            integer(c_long_long), intent(out) :: scratch_needed
        end function
        integer(c_int) function tlab_dns_field_to_particle(dns, nvar, fields, np, l_q, nodes, out) bind(C, name='tlab_dns_field_to_particle')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: dns, nodes
            integer(c_int), value :: nvar
            integer(c_long_long), value :: np
            type(c_ptr), intent(in) :: fields(*), l_q(*), out(*)
        end function
        integer(c_int) function tlab_dns_set_trajectories(dns, ntraj, tags) bind(C, name='tlab_dns_set_trajectories')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: dns
            integer(c_long_long), value :: ntraj
            integer(c_long_long), intent(in) :: tags(*)
        end function
        integer(c_int) function tlab_dns_trajectories_accumulate(dns, rtime, counter, nsave, np, l_q, nodes, tags, nvar, fields, l_traj) &
            bind(C, name='tlab_dns_trajectories_accumulate')
            import :: c_int, c_ptr, c_double, c_long_long
            type(c_ptr), value :: dns, nodes, tags, l_traj
            real(c_double), value :: rtime
            integer(c_long_long), value :: counter, nsave, np
            integer(c_int), value :: nvar
            type(c_ptr), intent(in) :: l_q(*), fields(*)
        end function
        integer(c_int) function tlab_dns_particle_to_field(dns, np, l_q, nodes, property, periodic, field) &
            bind(C, name='tlab_dns_particle_to_field')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: dns, nodes, property, field
            integer(c_long_long), value :: np
            integer(c_int), value :: periodic
            type(c_ptr), intent(in) :: l_q(*)
        end function
    end interface

contains

    ! part_type, part_bcs: part%type, part_bcs of PARTICLE_VARS; stokes, settling of NavierStokes
    subroutine push(dns, part_type, part_bcs, stokes, settling)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: part_type, part_bcs
        real(c_double), intent(in) :: stokes, settling

        if (pushed .and. c_associated(dns, last_dns) .and. part_type == last_type .and. part_bcs == last_bcs .and. stokes == last_stokes .and. &
            settling == last_settling) return
        call TLab_AMD_Check(tlab_dns_set_particles(dns, int(part_type, c_int), int(part_bcs, c_int), stokes, settling), 'tlab_dns_set_particles')
        pushed = .true.; last_dns = dns
        last_type = part_type; last_bcs = part_bcs; last_stokes = stokes; last_settling = settling
    end subroutine push

    ! the columns of l_q(isize_part, *) and l_hq(isize_part, *) as device pointers
    subroutine columns(inb_part, isize_part, l_q, l_hq, pq, ph)
        integer, intent(in) :: inb_part, isize_part
        real(c_double), intent(in), target :: l_q(*), l_hq(*)
        type(c_ptr), intent(out) :: pq(MAXC), ph(MAXC)
        integer :: i
        integer(c_long_long) :: m

        if (inb_part < 3 .or. inb_part > MAXC) call TLab_AMD_Check(-1_c_int, 'TLab_AMD_Particles: inb_part must be 3 (tracer) or 6 (inertia)')
        m = int(isize_part, c_long_long)
        pq = c_null_ptr; ph = c_null_ptr
        do i = 1, inb_part
            pq(i) = c_loc(l_q(1 + (i - 1)*m)); ph(i) = c_loc(l_hq(1 + (i - 1)*m))
        end do
    end subroutine columns

    ! The body of a patched TIME_SUBSTEP_PARTICLE:
    !   call TLab_AMD_Substep_Particle(TLab_AMD_DNS_Handle(), part%type, part_bcs, stokes, settling, dte, kco(rkm_substep), rkm_substep < rkm_endstep, &
    !                                  l_g%np, isize_part, inb_part, q, l_q, l_hq, l_g%nodes)
    ! q(isize_field, 3), l_q(isize_part, inb_part_array), l_hq(isize_part, inb_part), nodes(isize_part): the module arrays, in device memory.
    ! With scale_tendencies the loop of time.f90:300-304 is done here and must leave the host's TIME_RUNGEKUTTA.
    subroutine TLab_AMD_Substep_Particle(dns, part_type, part_bcs, stokes, settling, dte, kco, scale_tendencies, np, isize_part, inb_part, &
                                         q, l_q, l_hq, nodes)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: part_type, part_bcs, np, isize_part, inb_part
        real(c_double), intent(in) :: stokes, settling, dte, kco
        logical, intent(in) :: scale_tendencies
        real(c_double), intent(in), target :: q(*)
        real(c_double), intent(inout), target :: l_q(*), l_hq(*)
        integer(c_int), intent(inout), target :: nodes(*)

        type(c_ptr) :: pv(3), pq(MAXC), ph(MAXC)
        integer(c_long_long) :: n
        integer(c_int) :: iscale
        integer :: i

        n = tlab_dns_info(dns, 4_c_int)
        if (n <= 0) call TLab_AMD_Check(-1_c_int, 'TLab_AMD_Substep_Particle: bad handle')
        call push(dns, part_type, part_bcs, stokes, settling)
        do i = 1, 3
            pv(i) = c_loc(q(1 + (i - 1)*n))
        end do
        call columns(inb_part, isize_part, l_q, l_hq, pq, ph)
        iscale = 0_c_int
        if (scale_tendencies) iscale = 1_c_int
        call TLab_AMD_Check(tlab_dns_substep_particle(dns, dte, kco, iscale, int(np, c_long_long), pv, pq, ph, c_loc(nodes)), &
                            'tlab_dns_substep_particle')
    end subroutine TLab_AMD_Substep_Particle

    ! LOCATE_Y(l_g%np, l_q(1, 2), l_g%nodes, ...): the settings are pushed first (the y table of the driver is written then)
    subroutine TLab_AMD_Locate_Particles(dns, part_type, part_bcs, stokes, settling, np, isize_part, l_q, nodes)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: part_type, part_bcs, np, isize_part
        real(c_double), intent(in) :: stokes, settling
        real(c_double), intent(in), target :: l_q(*)
        integer(c_int), intent(inout), target :: nodes(*)

        call push(dns, part_type, part_bcs, stokes, settling)
        call TLab_AMD_Check(tlab_dns_particle_locate(dns, int(np, c_long_long), c_loc(l_q(1 + int(isize_part, c_long_long))), c_loc(nodes)), &
                            'tlab_dns_particle_locate')
    end subroutine TLab_AMD_Locate_Particles

    ! tags: l_g%tags (integer(longi)), in device memory like the rest; the scratch grows when the driver asks for more
    subroutine TLab_AMD_Sort_Particles(dns, np, isize_part, inb_part, l_q, l_hq, nodes, tags)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: np, isize_part, inb_part
        real(c_double), intent(inout), target :: l_q(*), l_hq(*)
        integer(c_int), intent(inout), target :: nodes(*)
        integer(c_long_long), intent(inout), target :: tags(*)

        type(c_ptr) :: pq(MAXC), ph(MAXC)
        integer(c_long_long) :: need, dummy

        call columns(inb_part, isize_part, l_q, l_hq, pq, ph)
        call TLab_AMD_Check(tlab_dns_particle_sort(dns, int(np, c_long_long), pq, ph, c_null_ptr, c_null_ptr, c_null_ptr, 0_c_long_long, need), &
                            'tlab_dns_particle_sort (size)')
        if (need > scratch_bytes) then
            if (c_associated(scratch)) call TLab_AMD_Check(tlab_free(scratch), 'tlab_free')
            scratch = c_null_ptr; scratch_bytes = 0_c_long_long
            call TLab_AMD_Check(tlab_malloc(scratch, int(need, c_size_t)), 'tlab_malloc')
            scratch_bytes = need
        end if
        call TLab_AMD_Check(tlab_dns_particle_sort(dns, int(np, c_long_long), pq, ph, c_loc(nodes), c_loc(tags), scratch, scratch_bytes, dummy), &
                            'tlab_dns_particle_sort')
    end subroutine TLab_AMD_Sort_Particles

    ! the columns of l_q(isize_part, *) alone
    subroutine positions(inb_part, isize_part, l_q, pq)
        integer, intent(in) :: inb_part, isize_part
        real(c_double), intent(in), target :: l_q(*)
        type(c_ptr), intent(out) :: pq(MAXC)
        integer :: i

        if (inb_part < 3 .or. inb_part > MAXC) call TLab_AMD_Check(-1_c_int, 'TLab_AMD_Particles: inb_part must be 3 (tracer) or 6 (inertia)')
        pq = c_null_ptr
        do i = 1, inb_part
            pq(i) = c_loc(l_q(1 + (i - 1)*int(isize_part, c_long_long)))
        end do
    end subroutine positions

    ! FIELD_TO_PARTICLE(data_in(1:nvar), data(1:nvar), l_g, l_q): fields(iv) = c_loc of the field data_in(iv) points to, out(iv) = c_loc of the
    ! particle array data(iv) points to, all in device memory.  Additive, as there: the caller zeroes the targets when it wants the value alone.
    subroutine TLab_AMD_Field_To_Particle(dns, nvar, fields, np, isize_part, l_q, nodes, out)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: nvar, np, isize_part
        type(c_ptr), intent(in) :: fields(nvar), out(nvar)
        real(c_double), intent(in), target :: l_q(*)
        integer(c_int), intent(in), target :: nodes(*)

        type(c_ptr) :: pq(MAXC)

        call positions(3, isize_part, l_q, pq)
        call TLab_AMD_Check(tlab_dns_field_to_particle(dns, int(nvar, c_int), fields, int(np, c_long_long), pq, c_loc(nodes), out), &
                            'tlab_dns_field_to_particle')
    end subroutine TLab_AMD_Field_To_Particle

    ! PARTICLE_TO_FIELD(l_q, particle_property, field_out, wrk3d) without the work array.  Without `property` every particle counts 1 (the number
    ! density).  periodic (default .true.): the contributions to column imax + 1 and plane kmax + 1 are added to column / plane 1, as the reference
    ! does across ranks; .false.: they are dropped, as its serial build does.
    subroutine TLab_AMD_Particle_To_Field(dns, np, isize_part, l_q, nodes, field, property, periodic)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: np, isize_part
        real(c_double), intent(in), target :: l_q(*)
        integer(c_int), intent(in), target :: nodes(*)
        real(c_double), intent(inout), target :: field(*)
        real(c_double), intent(in), target, optional :: property(*)
        logical, intent(in), optional :: periodic

        type(c_ptr) :: pq(MAXC), pp
        integer(c_int) :: iper

        call positions(3, isize_part, l_q, pq)
        pp = c_null_ptr
        if (present(property)) pp = c_loc(property)
        iper = 1_c_int
        if (present(periodic)) then
            if (.not. periodic) iper = 0_c_int
        end if
        call TLab_AMD_Check(tlab_dns_particle_to_field(dns, int(np, c_long_long), pq, c_loc(nodes), pp, iper, c_loc(field)), &
                            'tlab_dns_particle_to_field')
    end subroutine TLab_AMD_Particle_To_Field

    ! l_traj_tags(1:isize_traj) of ParticleTrajectories_Initialize (host memory); isize_traj = 0 switches the trajectories off
    subroutine TLab_AMD_Trajectories_Set(dns, isize_traj, l_traj_tags)
        type(c_ptr), intent(in) :: dns
        integer, intent(in) :: isize_traj
        integer(c_long_long), intent(in) :: l_traj_tags(*)

        call TLab_AMD_Check(tlab_dns_set_trajectories(dns, int(isize_traj, c_long_long), l_traj_tags), 'tlab_dns_set_trajectories')
    end subroutine TLab_AMD_Trajectories_Set

    ! ParticleTrajectories_Accumulate after its "counter = counter + 1": l_traj(isize_traj + 1, nitera_save, inb_part + nvar) in device memory;
    ! fields(1:nvar) = c_loc of q(:, iv) and s(:, iv) (TrajType = eulerian) or of the vorticity components the caller made (vorticity); nvar = 0
    ! for TrajType = basic (fields is not read then).  No l_txc is needed: only the tracked particles are interpolated.
    subroutine TLab_AMD_Trajectories_Accumulate(dns, rtime, counter, nitera_save, np, isize_part, inb_part, l_q, nodes, tags, nvar, fields, l_traj)
        type(c_ptr), intent(in) :: dns
        real(c_double), intent(in) :: rtime
        integer, intent(in) :: counter, nitera_save, np, isize_part, inb_part, nvar
        real(c_double), intent(in), target :: l_q(*)
        integer(c_int), intent(in), target :: nodes(*)
        integer(c_long_long), intent(in), target :: tags(*)
        type(c_ptr), intent(in) :: fields(*)
        real(c_float), intent(inout), target :: l_traj(*)

        type(c_ptr) :: pq(MAXC)

        call positions(inb_part, isize_part, l_q, pq)
        call TLab_AMD_Check(tlab_dns_trajectories_accumulate(dns, rtime, int(counter, c_long_long), int(nitera_save, c_long_long), &
                                                             int(np, c_long_long), pq, c_loc(nodes), c_loc(tags), int(nvar, c_int), fields, &
                                                             c_loc(l_traj)), 'tlab_dns_trajectories_accumulate')
    end subroutine TLab_AMD_Trajectories_Accumulate

end module TLab_AMD_Particles
