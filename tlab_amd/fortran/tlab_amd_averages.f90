!########################################################################
! The plane averages of module Averages (utils/averages.f90 of the reference) and the covariance blocks of AVG_FLOW_XZ / AVG_SCAL_XZ for a host whose
! fields live in device memory:
!   TLab_AMD_AVG_IK_V, TLab_AMD_AVG1V2D_V   the reference's AVG_IK_V (:301-327) and AVG1V2D_V (:142-167), same argument lists: a call site on a
!                                           device array changes its name and nothing else.  With USE_MPI the MPI_ALLREDUCE and the division of the
!                                           reference (:320-324, :161-165) follow the local call.
!   TLab_AMD_Avg_Moments_Flow               the statements of avg_flow_xz.f90:513-553 and :597-654 (incompressible branch) that form a whole-field
!                                           product and average it: one pass over u, v, w (and p) instead of one temporary and one AVG_IK_V per
!                                           output.  out(jmax, 18 or 22): columns of the caller's mean2d in the order of include/tlab_amd.h.
!   TLab_AMD_Avg_Moments_Scal               the same for avg_scal_xz.f90:373-455: out(jmax, 10 or 11).
!   TLab_AMD_Avg_Gradients_Flow            the groups of Section 3 of AVG_FLOW_XZ on the nine gradient arrays (avg_flow_xz.f90:988-1248, with p also
!                                           the pressure strain :681-699) in three passes: out(jmax, 50 or 56) in the order of include/tlab_amd.h,
!                                           RAW: the caller's host lines (Phi*visc*2, Tau*visc, E = (E*visc - Tau*rU_y)*2, PIxx*2, Txxy -= ..) stay.
!                                           The arguments are AVG_FLOW_XZ's own arrays dudx .. dwdz, u, v, w, p_loc and its mean2d macros.
!   TLab_AMD_Avg_UGradP                     avg_flow_xz.f90:673-674 on u, v, w and the three derivatives of p (there in dwdx, dwdy, dwdz)
!   TLab_AMD_Avg_Gradients_Scal             avg_scal_xz.f90:451-453, :607, :714-745 on dsdx, dsdy, dsdz: out(jmax, 15 or 18)
!                                           With USE_MPI every pass is followed by the reference's MPI_ALLREDUCE (averages.f90:320-324), so that the
!                                           means a later pass subtracts are the global ones, as the reference's AVG_IK_V returns them.
!   TLab_AMD_FI_Vorticity, TLab_AMD_Inter_N_XZ  the block stats_intermittency of DNS_STATISTICS (dns_statistics.f90:99-117): FI_VORTICITY
!                                           (mappings/fi_vorticity.f90:28-59) on the driver's plans with one pass over the six derivatives, and the
!                                           calculation of INTER_N_XZ (statistics/avg_xz.f90:109-153) for all planes and levels in one pass over
!                                           the gate.  With USE_MPI the avg/real(npro) and MPI_ALLREDUCE of INTER1V2D (averages.f90:233-236) follow;
!                                           like every USE_MPI branch of this module, that one is NOT compiled by this project's build or tests.
!   TLab_AMD_FI_Gate, TLab_AMD_AVG_N_XZ     the conditional block of tools/statistics/averages.f90 (opt_main 3-18): the partition of FI_GATE
!                                           (mappings/fi_gate.f90, opt_cond 2-7) on the driver's plans and the moments of AVG_N_XZ
!                                           (statistics/avg_xz.f90:10-70) of one gate level from one pass over the gate and the fields.  Single
!                                           rank: the decomposed form reduces the sums and nsample of tlab_avg_n_xz, then tlab_raw_to_central.
! The arrays are classified by the library (tlab_pointer_on_device): host arrays take a host loop in the reference's order, so the routines serve
! either kind; a mix is refused.  The profiles are host memory.  The moment routines give the LOCAL averages: a decomposed host reduces them as it
! does the profiles of AVG_IK_V.  What the reference adds on the host afterwards (Ty1, Txyy, Tyyy, Tyzy) stays with the caller.
!########################################################################
module TLab_AMD_Averages
    use TLab_AMD_C
#ifdef USE_MPI
    use mpi_f08
    use TLabMPI_VARS, only: ims_npro_i, ims_npro_k, ims_err
#endif
    implicit none
    private
    public :: TLab_AMD_AVG_IK_V, TLab_AMD_AVG1V2D_V, TLab_AMD_Avg_Moments_Flow, TLab_AMD_Avg_Moments_Scal
    public :: TLab_AMD_Avg_Gradients_Flow, TLab_AMD_Avg_UGradP, TLab_AMD_Avg_Gradients_Scal
    public :: TLab_AMD_FI_Vorticity, TLab_AMD_Inter_N_XZ, TLab_AMD_FI_Gate, TLab_AMD_AVG_N_XZ, TLab_AMD_AVG_N_XZ_Levels

contains
    subroutine TLab_AMD_AVG_IK_V(nx, ny, nz, a, avg, wrk)
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: a(nx, ny, nz)
        real(c_double), intent(out) :: avg(ny)
        real(c_double), intent(inout) :: wrk(ny)
        type(c_ptr) :: pa(1)

        pa(1) = c_loc(a)
        call TLab_AMD_Check(tlab_avg_ik_v(nx, ny, nz, 1, pa, avg, ny), 'tlab_avg_ik_v')
#ifdef USE_MPI
        call MPI_ALLREDUCE(avg, wrk, ny, MPI_REAL8, MPI_SUM, MPI_COMM_WORLD, ims_err)
        avg = wrk/real(ims_npro_i*ims_npro_k, c_double)
#endif
    end subroutine TLab_AMD_AVG_IK_V

    subroutine TLab_AMD_AVG1V2D_V(nx, ny, nz, imom, a, avg, wrk)
        integer, intent(in) :: nx, ny, nz, imom
        real(c_double), intent(in), target :: a(nx, ny, nz)
        real(c_double), intent(out) :: avg(ny)
        real(c_double), intent(inout) :: wrk(ny)

        call TLab_AMD_Check(tlab_avg1v2d_v(nx, ny, nz, imom, c_loc(a), avg), 'tlab_avg1v2d_v')
#ifdef USE_MPI
        wrk = avg/real(ims_npro_i*ims_npro_k, c_double)
        call MPI_ALLREDUCE(wrk, avg, ny, MPI_REAL8, MPI_SUM, MPI_COMM_WORLD, ims_err)
#endif
    end subroutine TLab_AMD_AVG1V2D_V

    ! out(:, 1:18) = Rxx Ryy Rzz Rxy Rxz Ryz rU3 rU4 rV3 rV4 rW3 rW4 Txxy Tyyy Tzzy Txyy Txzy Tyzy; with p and rP also (:, 19:22) = rP2 <u'p'> <v'p'> <w'p'>
    subroutine TLab_AMD_Avg_Moments_Flow(nx, ny, nz, u, v, w, fU, fV, fW, out, p, rP)
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx, ny, nz), v(nx, ny, nz), w(nx, ny, nz)
        real(c_double), intent(in), target :: fU(ny), fV(ny), fW(ny)
        real(c_double), intent(out), target :: out(ny, *)
        real(c_double), intent(in), target, optional :: p(nx, ny, nz), rP(ny)
        type(c_ptr) :: pp, pm

        pp = c_null_ptr; pm = c_null_ptr
        if (present(p)) pp = c_loc(p)
        if (present(rP)) pm = c_loc(rP)
        call TLab_AMD_Check(tlab_avg_moments_flow(nx, ny, nz, c_loc(u), c_loc(v), c_loc(w), pp, c_loc(fU), c_loc(fV), c_loc(fW), pm, &
                                                  c_loc(out), ny), 'tlab_avg_moments_flow')
    end subroutine TLab_AMD_Avg_Moments_Flow

    ! out(:, 1:10) = rS2 rS3 rS4 Rsu Rsv Rsw Tssy1 Tsuy1 Tsvy1 Tswy1; with p and rP also (:, 11) = Tsvy3
    subroutine TLab_AMD_Avg_Moments_Scal(nx, ny, nz, s, u, v, w, fS, fU, fV, fW, out, p, rP)
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: s(nx, ny, nz), u(nx, ny, nz), v(nx, ny, nz), w(nx, ny, nz)
        real(c_double), intent(in), target :: fS(ny), fU(ny), fV(ny), fW(ny)
        real(c_double), intent(out), target :: out(ny, *)
        real(c_double), intent(in), target, optional :: p(nx, ny, nz), rP(ny)
        type(c_ptr) :: pp, pm

        pp = c_null_ptr; pm = c_null_ptr
        if (present(p)) pp = c_loc(p)
        if (present(rP)) pm = c_loc(rP)
        call TLab_AMD_Check(tlab_avg_moments_scal(nx, ny, nz, c_loc(s), c_loc(u), c_loc(v), c_loc(w), pp, c_loc(fS), c_loc(fU), c_loc(fV), &
                                                  c_loc(fW), pm, c_loc(out), ny), 'tlab_avg_moments_scal')
    end subroutine TLab_AMD_Avg_Moments_Scal

    ! out(:, 1:50) in the order of include/tlab_amd.h (vortx .. Tyzy_v); with p and rP also (:, 51:56) = PIxx PIyy PIzz PIxy PIxz PIyz.  wrk(ny, *): as
    ! many columns as out (used with USE_MPI only)
    subroutine TLab_AMD_Avg_Gradients_Flow(nx, ny, nz, dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz, u, v, w, &
                                           fU, fV, fW, rU_y, rV_y, rW_y, out, wrk, p, rP)
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target, dimension(nx, ny, nz) :: dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz, u, v, w
        real(c_double), intent(in), target :: fU(ny), fV(ny), fW(ny), rU_y(ny), rV_y(ny), rW_y(ny)
        real(c_double), intent(out), target :: out(ny, *)
        real(c_double), intent(inout) :: wrk(ny, *)
        real(c_double), intent(in), target, optional :: p(nx, ny, nz), rP(ny)
        type(c_ptr) :: pp, pm, g(13), m(7)
        integer :: ip

        pp = c_null_ptr; pm = c_null_ptr; ip = 0
        if (present(p)) pp = c_loc(p)
        if (present(rP)) pm = c_loc(rP)
        if (present(p)) ip = 1
        g(1:9) = [c_loc(dudx), c_loc(dudy), c_loc(dudz), c_loc(dvdx), c_loc(dvdy), c_loc(dvdz), c_loc(dwdx), c_loc(dwdy), c_loc(dwdz)]
#ifdef USE_MPI
        g(10:13) = [c_loc(u), c_loc(v), c_loc(w), pp]
        m(1) = c_null_ptr
        call TLab_AMD_Check(tlab_avg_gradients_pass(1, 0, nx, ny, nz, g, m, c_loc(out(1, 1)), ny), 'tlab_avg_gradients_pass')
        call Reduce(ny, 6, out(1, 1), wrk)
        m(1:6) = [c_loc(rU_y), c_loc(rV_y), c_loc(rW_y), c_loc(out(1, 1)), c_loc(out(1, 2)), c_loc(out(1, 3))]
        call TLab_AMD_Check(tlab_avg_gradients_pass(2, 0, nx, ny, nz, g, m, c_loc(out(1, 7)), ny), 'tlab_avg_gradients_pass')
        m(1:7) = [c_loc(out(1, 4)), c_loc(out(1, 5)), c_loc(out(1, 6)), c_loc(fU), c_loc(fV), c_loc(fW), pm]
        call TLab_AMD_Check(tlab_avg_gradients_pass(3, ip, nx, ny, nz, g, m, c_loc(out(1, 45)), ny), 'tlab_avg_gradients_pass')
        call Reduce(ny, 44 + 6*ip, out(1, 7), wrk)
#else
        call TLab_AMD_Check(tlab_avg_gradients_flow(nx, ny, nz, g(1:9), c_loc(u), c_loc(v), c_loc(w), pp, c_loc(fU), c_loc(fV), c_loc(fW), pm, &
                                                    c_loc(rU_y), c_loc(rV_y), c_loc(rW_y), c_loc(out), ny), 'tlab_avg_gradients_flow')
#endif
    end subroutine TLab_AMD_Avg_Gradients_Flow

    ! avg = the plane average of u*dpdx + v*dpdy + w*dpdz; the argument list of AVG_IK_V behind the fields
    subroutine TLab_AMD_Avg_UGradP(nx, ny, nz, u, v, w, dpdx, dpdy, dpdz, avg, wrk)
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target, dimension(nx, ny, nz) :: u, v, w, dpdx, dpdy, dpdz
        real(c_double), intent(out), target :: avg(ny)
        real(c_double), intent(inout) :: wrk(ny)

        call TLab_AMD_Check(tlab_avg_ugradp(nx, ny, nz, c_loc(u), c_loc(v), c_loc(w), c_loc(dpdx), c_loc(dpdy), c_loc(dpdz), c_loc(avg)), &
                            'tlab_avg_ugradp')
#ifdef USE_MPI
        call Reduce(ny, 1, avg, wrk)
#endif
    end subroutine TLab_AMD_Avg_UGradP

    ! out(:, 1:15) = Fy Ess S_x2 S_y2 S_z2 S_x3 S_y3 S_z3 S_x4 S_y4 S_z4 Tssy2 Tsuy2_d Tsvy2_d Tswy2_d; with p, rP and fS_y also (:, 16:18) = PIsu PIsv PIsw
    subroutine TLab_AMD_Avg_Gradients_Scal(nx, ny, nz, dsdx, dsdy, dsdz, s, u, v, w, fS, fU, fV, fW, rS_y, out, wrk, p, rP, fS_y)
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target, dimension(nx, ny, nz) :: dsdx, dsdy, dsdz, s, u, v, w
        real(c_double), intent(in), target :: fS(ny), fU(ny), fV(ny), fW(ny), rS_y(ny)
        real(c_double), intent(out), target :: out(ny, *)
        real(c_double), intent(inout) :: wrk(ny, *)
        real(c_double), intent(in), target, optional :: p(nx, ny, nz), rP(ny), fS_y(ny)
        type(c_ptr) :: pp, pm, py, g(8), m(7)
        integer :: ip

        pp = c_null_ptr; pm = c_null_ptr; py = c_null_ptr; ip = 0
        if (present(p)) pp = c_loc(p)
        if (present(rP)) pm = c_loc(rP)
        if (present(fS_y)) py = c_loc(fS_y)
        if (present(p)) ip = 1
        g(1:3) = [c_loc(dsdx), c_loc(dsdy), c_loc(dsdz)]
#ifdef USE_MPI
        m(1) = c_loc(rS_y)
        call TLab_AMD_Check(tlab_avg_gradients_pass(4, 0, nx, ny, nz, g, m, c_loc(out(1, 1)), ny), 'tlab_avg_gradients_pass')
        call Reduce(ny, 11, out(1, 1), wrk)
        g(1:8) = [c_loc(dsdy), c_loc(s), c_loc(u), c_loc(v), c_loc(w), pp, c_loc(dsdx), c_loc(dsdz)]
        m(1:7) = [c_loc(out(1, 1)), c_loc(fS), c_loc(fU), c_loc(fV), c_loc(fW), pm, py]
        call TLab_AMD_Check(tlab_avg_gradients_pass(5, ip, nx, ny, nz, g, m, c_loc(out(1, 12)), ny), 'tlab_avg_gradients_pass')
        call Reduce(ny, 4 + 3*ip, out(1, 12), wrk)
#else
        call TLab_AMD_Check(tlab_avg_gradients_scal(nx, ny, nz, g(1:3), c_loc(s), c_loc(u), c_loc(v), c_loc(w), pp, c_loc(fS), c_loc(fU), &
                                                    c_loc(fV), c_loc(fW), pm, c_loc(rS_y), py, c_loc(out), ny), 'tlab_avg_gradients_scal')
#endif
    end subroutine TLab_AMD_Avg_Gradients_Scal

    ! FI_VORTICITY(nx, ny, nz, u, v, w, result, tmp1, tmp2) with six work arrays in place of two: txc6(i) = c_loc(txc(1, .)) hold v,x u,y u,z w,x w,y
    ! v,z on return.  dns: the driver's handle (TLab_AMD_DNS_Handle()), whose plans are g(1:3).  Device arrays.
    subroutine TLab_AMD_FI_Vorticity(dns, nx, ny, nz, u, v, w, result, txc6)
        type(c_ptr), intent(in) :: dns, txc6(6)
        integer, intent(in) :: nx, ny, nz
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), w(nx*ny*nz)
        real(c_double), intent(out), target :: result(nx*ny*nz)

        call TLab_AMD_Check(tlab_fi_vorticity(dns, c_loc(u), c_loc(v), c_loc(w), c_loc(result), txc6), 'tlab_fi_vorticity')
    end subroutine TLab_AMD_FI_Vorticity

    ! The calculation of INTER_N_XZ: the reference's argument list minus fname, itime, rtime, parname and y -- the file is written by the host, from
    ! inter, as before (avg_xz.f90:144-150).  wrk(ny, np) is used with USE_MPI only, where INTER1V2D's avg/real(npro) and MPI_ALLREDUCE follow.
    subroutine TLab_AMD_Inter_N_XZ(nx, ny, nz, np, gate, inter, wrk)
        integer, intent(in) :: nx, ny, nz, np
        integer(1), intent(in), target :: gate(*)
        real(c_double), intent(out) :: inter(ny, np)
        real(c_double), intent(inout) :: wrk(ny, np)

        call TLab_AMD_Check(tlab_inter_n_xz(nx, ny, nz, np, c_loc(gate), inter), 'tlab_inter_n_xz')
#ifdef USE_MPI
        wrk = inter/real(ims_npro_i*ims_npro_k, c_double)
        call MPI_ALLREDUCE(wrk, inter, ny*np, MPI_REAL8, MPI_SUM, MPI_COMM_WORLD, ims_err)
#endif
    end subroutine TLab_AMD_Inter_N_XZ

    ! FI_GATE: the reference's argument list with the driver's handle in front (its plans are g(1:3)) and the arrays as addresses: q(3), s(*) and
    ! txc(7) = c_loc(q(1, .)) .. of device arrays.  The indicator is left in txc(1) as in the reference (opt_cond 2 and 5 read their field in
    ! place); opt_cond 3 takes txc(2:7) as work arrays, 4 takes txc(2).  gate_threshold(igate_size - 1) is not changed.
    subroutine TLab_AMD_FI_Gate(dns, opt_cond, opt_cond_relative, opt_cond_scal, nx, ny, nz, igate_size, gate_threshold, q, s, txc, gate)
        type(c_ptr), intent(in) :: dns, q(3), s(*), txc(7)
        integer, intent(in) :: opt_cond, opt_cond_relative, opt_cond_scal, nx, ny, nz, igate_size
        real(c_double), intent(in) :: gate_threshold(igate_size)
        integer(1), intent(out), target :: gate(nx*ny*nz)

        call TLab_AMD_Check(tlab_dns_gate(dns, opt_cond, opt_cond_relative, opt_cond_scal, igate_size, gate_threshold, q, s, txc, c_loc(gate)), &
                            'tlab_dns_gate')
    end subroutine TLab_AMD_FI_Gate

    ! The calculation of AVG_N_XZ: the reference's argument list minus fname, itime, rtime and y -- the file is written by the host, from avg, as
    ! before (avg_xz.f90:55-66).  vars(nv) are the addresses of the fields, c_loc(vars(iv)%field) of the reference's pointers_dt.  igate = 0: the
    ! ungated moments; igate > 0: those of the level igate alone.  The library computes the levels 1 .. igate on the way (four a launch) and this
    ! routine keeps the last: a tool that LOOPS over the levels, as tools/statistics/averages.f90 does, calls TLab_AMD_AVG_N_XZ_Levels once
    ! instead and pays one pass for all of them, not one per level.  Single rank.
    subroutine TLab_AMD_AVG_N_XZ(nx, ny, nz, nv, nm, vars, igate, gate, avg)
        integer, intent(in) :: nx, ny, nz, nv, nm
        type(c_ptr), intent(in) :: vars(nv)
        integer(1), intent(in), target :: gate(*), igate
        real(c_double), intent(out) :: avg(ny, nm, nv)
        real(c_double), allocatable, target :: levels(:, :, :, :)
        type(c_ptr) :: pg

        pg = c_null_ptr
        if (igate > 0) pg = c_loc(gate)
        allocate (levels(ny, nm, nv, max(int(igate), 1)))
        call TLab_AMD_Check(tlab_avg_n_xz(nx, ny, nz, nv, nm, vars, max(int(igate), 0), pg, c_loc(levels), c_null_ptr, c_null_ptr), 'tlab_avg_n_xz')
        avg = levels(:, :, :, max(int(igate), 1))
    end subroutine TLab_AMD_AVG_N_XZ

    ! AVG_N_XZ for igate = 1 .. np in ONE pass over the gate and the fields: avg(:, :, :, igate) is what the reference's call returns for that
    ! level; np = 0: the ungated moments in avg(:, :, :, 1) (the gate is not read).  Single rank.
    subroutine TLab_AMD_AVG_N_XZ_Levels(nx, ny, nz, nv, nm, vars, np, gate, avg)
        integer, intent(in) :: nx, ny, nz, nv, nm, np
        type(c_ptr), intent(in) :: vars(nv)
        integer(1), intent(in), target :: gate(*)
        real(c_double), intent(out), target :: avg(ny, nm, nv, max(np, 1))
        type(c_ptr) :: pg

        pg = c_null_ptr
        if (np > 0) pg = c_loc(gate)
        call TLab_AMD_Check(tlab_avg_n_xz(nx, ny, nz, nv, nm, vars, np, pg, c_loc(avg), c_null_ptr, c_null_ptr), 'tlab_avg_n_xz')
    end subroutine TLab_AMD_AVG_N_XZ_Levels

#ifdef USE_MPI
    ! the reduction of AVG_IK_V (averages.f90:320-324) on nc columns of local averages
    subroutine Reduce(ny, nc, avg, wrk)
        integer, intent(in) :: ny, nc
        real(c_double), intent(inout) :: avg(ny*nc), wrk(ny*nc)

        call MPI_ALLREDUCE(avg, wrk, ny*nc, MPI_REAL8, MPI_SUM, MPI_COMM_WORLD, ims_err)
        avg = wrk/real(ims_npro_i*ims_npro_k, c_double)
    end subroutine Reduce
#endif

end module TLab_AMD_Averages
