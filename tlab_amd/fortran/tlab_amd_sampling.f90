!########################################################################
! The sampling of the time loop between two statistics steps (dns_main.f90:282-303, rhs_global_incompressible_1.f90:292-305, planes.f90) for a host
! whose fields live in device memory:
!   TLab_AMD_AvgPhaseSpace          AvgPhaseSpace (statistics/avg_phase.f90:100-202) for index 1, 2, 4: the reference's argument list, followed by what
!                                   its module holds -- the accumulator (avg_flow | avg_scal | avg_p), avg_planes and g(3)%size
!   TLab_AMD_AvgPhaseStress         AvgPhaseStress (:204-287) together with AvgPhaseSpace(index 1) in ONE pass over q: avg_flow and avg_stress
!   TLab_AMD_Tower_Accumulate       DNS_TOWER_ACCUMULATE(v, index, wrk1d) (tools/dns/dns_tower.f90:207-289) on a tower plan (tlab_tower_create: the
!                                   state of DNS_TOWER_INITIALIZE) and the caller's tower_buf; itime, rtime as TLab_Time holds them
!   TLab_AMD_Planes_Gather          the copies of PLANES_SAVE (tools/dns/planes.f90:279-342) for one direction into data_i | data_j | data_k
!   TLab_AMD_Arm_Pressure_Sampling  before the last substep of a step (rkm_substep == rkm_endstep): the device RHS hands its pressure to the towers
!                                   and the phase average between the solve and the gradient, as rhs_global_incompressible_1.f90:298-302 does
! The arrays are classified by the library: host arrays take a host loop that is the reference's statement, device arrays the kernels; a mix is
! refused.  Nothing here synchronises the stream.  Files (DNS_TOWER_WRITE, IO_Write_AvgPhase, IO_Write_Subarray) stay with the host.
!########################################################################
module TLab_AMD_Sampling
    use TLab_AMD_C
    implicit none
    private
    public :: TLab_AMD_AvgPhaseSpace, TLab_AMD_AvgPhaseStress, TLab_AMD_Tower_Accumulate, TLab_AMD_Planes_Gather, TLab_AMD_Arm_Pressure_Sampling
    public :: tlab_tower_create, tlab_tower_destroy, tlab_tower_sizes, tlab_tower_reset, tlab_avg_phase_plane_id

    interface
        integer(c_int) function tlab_avg_phase_space(nx, ny, nz, nz_total, nf, fields, avg_planes, plane_id, avg) bind(C, name='tlab_avg_phase_space')
            import :: c_int, c_ptr
            integer(c_int), value :: nx, ny, nz, nz_total, nf, avg_planes, plane_id
            type(c_ptr), intent(in) :: fields(*)
            type(c_ptr), value :: avg
        end function
        integer(c_int) function tlab_avg_phase_flow(nx, ny, nz, nz_total, u, v, w, avg_planes, plane_id, avg_flow, avg_stress) &
            bind(C, name='tlab_avg_phase_flow')
            import :: c_int, c_ptr
            integer(c_int), value :: nx, ny, nz, nz_total, avg_planes, plane_id
            type(c_ptr), value :: u, v, w, avg_flow, avg_stress
        end function
        integer(c_int) function tlab_avg_phase_plane_id(itr, it_first, it_save) bind(C, name='tlab_avg_phase_plane_id')
            import :: c_int
            integer(c_int), value :: itr, it_first, it_save
        end function
        integer(c_int) function tlab_tower_create(tower, nx, ny, nz, stride, nitera_save) bind(C, name='tlab_tower_create')
            import :: c_int, c_ptr
            type(c_ptr), intent(out) :: tower
            integer(c_int), value :: nx, ny, nz, nitera_save
            integer(c_int), intent(in) :: stride(3)
        end function
        integer(c_int) function tlab_tower_destroy(tower) bind(C, name='tlab_tower_destroy')
            import :: c_int, c_ptr
            type(c_ptr), value :: tower
        end function
        integer(c_int) function tlab_tower_sizes(tower, sizes) bind(C, name='tlab_tower_sizes')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: tower
            integer(c_long_long), intent(out) :: sizes(8)
        end function
        integer(c_int) function tlab_tower_reset(tower) bind(C, name='tlab_tower_reset')
            import :: c_int, c_ptr
            type(c_ptr), value :: tower
        end function
        integer(c_int) function tlab_tower_accumulate(tower, index, fields, itime, rtime, tower_buf) bind(C, name='tlab_tower_accumulate')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: tower, tower_buf
            integer(c_int), value :: index, itime
            real(c_double), value :: rtime
            type(c_ptr), intent(in) :: fields(*)
        end function
        integer(c_int) function tlab_planes_gather(nx, ny, nz, nvars, fields, dir, n, nodes, out, single) bind(C, name='tlab_planes_gather')
            import :: c_int, c_ptr
            integer(c_int), value :: nx, ny, nz, nvars, dir, n, single
            type(c_ptr), intent(in) :: fields(*)
            integer(c_int), intent(in) :: nodes(*)
            type(c_ptr), value :: out
        end function
        integer(c_int) function tlab_dns_arm_pressure_sampling(dns, tower, tower_buf, itime, rtime, phase_avg, avg_planes, plane_id) &
            bind(C, name='tlab_dns_arm_pressure_sampling')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: dns, tower, tower_buf, phase_avg
            integer(c_int), value :: itime, avg_planes, plane_id
            real(c_double), value :: rtime
        end function
    end interface

contains
    ! call AvgPhaseSpace(wrk2d, inb_flow, itime, nitera_first, nitera_save, 1) becomes
    ! call TLab_AMD_AvgPhaseSpace(wrk2d, inb_flow, itime, nitera_first, nitera_save, q, kmax, avg_flow, avg_planes, g(3)%size)
    subroutine TLab_AMD_AvgPhaseSpace(localsum, nfield, itr, it_first, it_save, field, nz, avg, avg_planes, nz_total)
        real(c_double), intent(inout) :: localsum(:, :)                 ! (imax, jmax): gives the plane; not written
        integer, intent(in) :: nfield, itr, it_first, it_save, nz, avg_planes, nz_total
        real(c_double), intent(in), target :: field(size(localsum, 1), size(localsum, 2), nz, nfield)
        real(c_double), intent(inout), target :: avg(*)
        type(c_ptr) :: pf(nfield)
        integer :: i

        do i = 1, nfield
            pf(i) = c_loc(field(1, 1, 1, i))
        end do
        call TLab_AMD_Check(tlab_avg_phase_space(size(localsum, 1), size(localsum, 2), nz, nz_total, nfield, pf, avg_planes, &
                                                 tlab_avg_phase_plane_id(itr, it_first, it_save), c_loc(avg)), 'tlab_avg_phase_space')
    end subroutine TLab_AMD_AvgPhaseSpace

    ! call AvgPhaseSpace(wrk2d, 3, ..., 1); call AvgPhaseStress(q, itime, nitera_first, nitera_save) become
    ! call TLab_AMD_AvgPhaseStress(q, itime, nitera_first, nitera_save, imax, jmax, kmax, avg_flow, avg_stress, avg_planes, g(3)%size)
    subroutine TLab_AMD_AvgPhaseStress(q, itr, it_first, it_save, nx, ny, nz, avg_flow, avg_stress, avg_planes, nz_total)
        integer, intent(in) :: itr, it_first, it_save, nx, ny, nz, avg_planes, nz_total
        real(c_double), intent(in), target :: q(nx*ny*nz, 3)
        real(c_double), intent(inout), target :: avg_flow(*), avg_stress(*)

        call TLab_AMD_Check(tlab_avg_phase_flow(nx, ny, nz, nz_total, c_loc(q(1, 1)), c_loc(q(1, 2)), c_loc(q(1, 3)), avg_planes, &
                                                tlab_avg_phase_plane_id(itr, it_first, it_save), c_loc(avg_flow), c_loc(avg_stress)), &
                            'tlab_avg_phase_flow')
    end subroutine TLab_AMD_AvgPhaseStress

    ! call DNS_TOWER_ACCUMULATE(q, 1, wrk1d) becomes call TLab_AMD_Tower_Accumulate(q, 1, wrk1d, tower, tower_buf, imax, jmax, kmax, itime, rtime)
    subroutine TLab_AMD_Tower_Accumulate(v, index, wrk1d, tower, tower_buf, nx, ny, nz, itime, rtime)
        integer, intent(in) :: index, nx, ny, nz, itime
        real(c_double), intent(in), target :: v(nx, ny, nz, *)
        real(c_double), intent(inout) :: wrk1d(*)                       ! not used: the means need no work array
        type(c_ptr), intent(in) :: tower
        real(c_double), intent(inout), target :: tower_buf(*)
        real(c_double), intent(in) :: rtime
        type(c_ptr) :: pv(3)
        integer :: i

        pv = c_null_ptr
        do i = 1, merge(3, 1, index == 1)
            pv(i) = c_loc(v(1, 1, 1, i))
        end do
        call TLab_AMD_Check(tlab_tower_accumulate(tower, index, pv, itime, rtime, c_loc(tower_buf)), 'tlab_tower_accumulate')
    end subroutine TLab_AMD_Tower_Accumulate

    ! data_k(:, :, 1 + offset:n + offset) = vars(iv)%field(:, :, kplanes%nodes(1:n)) for all iv (planes.f90:286-290) becomes
    ! call TLab_AMD_Planes_Gather(imax, jmax, kmax, nvars, vars, 3, kplanes%n, kplanes%nodes, data_k); single: data is real(4)
    subroutine TLab_AMD_Planes_Gather(nx, ny, nz, nvars, vars, dir, n, nodes, data, single)
        integer, intent(in) :: nx, ny, nz, nvars, dir, n, nodes(n)
        type(c_ptr), intent(in) :: vars(nvars)                          ! c_loc of every field, in the order of PLANES_SAVE
        type(c_ptr), intent(in) :: data
        logical, intent(in), optional :: single
        integer :: is

        is = 0
        if (present(single)) is = merge(1, 0, single)
        call TLab_AMD_Check(tlab_planes_gather(nx, ny, nz, nvars, vars, dir, n, nodes, data, is), 'tlab_planes_gather')
    end subroutine TLab_AMD_Planes_Gather

    ! in TIME_RUNGEKUTTA, before the last substep: if (rkm_substep == rkm_endstep) call TLab_AMD_Arm_Pressure_Sampling(dns, ...); a target that is
    ! not due this step is passed as c_null_ptr (use_tower .and. mod(itime, stride) == 0; PhAvg%active .and. mod(itime + 1, PhAvg%stride) == 0)
    subroutine TLab_AMD_Arm_Pressure_Sampling(dns, tower, tower_buf, itime, rtime, avg_p, avg_planes, itr, it_first, it_save)
        type(c_ptr), intent(in) :: dns, tower, tower_buf, avg_p
        integer, intent(in) :: itime, avg_planes, itr, it_first, it_save
        real(c_double), intent(in) :: rtime

        call TLab_AMD_Check(tlab_dns_arm_pressure_sampling(dns, tower, tower_buf, itime, rtime, avg_p, avg_planes, &
                                                           tlab_avg_phase_plane_id(itr, it_first, it_save)), 'tlab_dns_arm_pressure_sampling')
    end subroutine TLab_AMD_Arm_Pressure_Sampling
end module TLab_AMD_Sampling
