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

end module TLab_AMD_Averages
