!########################################################################
! The plane PDFs of the reference (statistics/pdf.f90 over module PDFS, utils/pdfs.f90) for a host whose fields live in device memory:
!   TLab_AMD_PDF1V_N   the calculation of PDF1V_N (:14-91): the reference's argument list minus fname, time and y -- the file is written by the
!                      host, from pdf, as before (:93-115).  u(nv) are the addresses of the fields, c_loc(u(iv)%field) of the reference's
!                      pointers_dt (this module depends on TLab_AMD_C alone); gate may be any int8 array when igate == 0.
!                      All fields share three passes (min/max; histogram; histogram on the intervals of PDF_ANALIZE) instead of four strided
!                      passes per field and plane.
!   TLab_AMD_PDF2V     the calculation of PDF2V (:123-159), single rank.
!   TLab_AMD_CAVG1V_N, TLab_AMD_CAVG2V   the calculations of CAVG1V_N and CAVG2V (statistics/cavg.f90:7-89, :93-155): the reference's argument
!                      lists minus fname, time and y; single rank (the decomposed form reduces the sum and pdf outputs of tlab_cavg1v_n).
! The arrays are classified by the library (tlab_pointer_on_device): host arrays take the reference's loops on the host, so the routines serve
! either kind; a mix is refused.  pdf is host memory.
! With USE_MPI the reference's MPI_ALLREDUCEs (utils/pdfs.f90:59-64, :92-95) stand between the passes: min and max of every plane are reduced,
! then the counts.  That branch uses what the reference's module PDFS uses there; it is NOT compiled by this project's build or tests.  The joint
! PDF has no decomposed form here: with USE_MPI TLab_AMD_PDF2V gives the local histogram on the local intervals.
!########################################################################
module TLab_AMD_PDFs
    use TLab_AMD_C
#ifdef USE_MPI
    use mpi_f08
#endif
    implicit none
    private
    public :: TLab_AMD_PDF1V_N, TLab_AMD_PDF2V, TLab_AMD_CAVG1V_N, TLab_AMD_CAVG2V

contains
    subroutine TLab_AMD_PDF1V_N(nx, ny, nz, nv, nbins, ibc, umin, umax, u, igate, gate, pdf)
        integer, intent(in) :: nx, ny, nz, nv, nbins, ibc(nv)
        real(c_double), intent(in) :: umin(nv), umax(nv)
        type(c_ptr), intent(in) :: u(nv)
        integer(1), intent(in), target :: gate(*), igate
        real(c_double), intent(out) :: pdf(nbins + 2, ny + 1, nv)
        type(c_ptr) :: pg
#ifdef USE_MPI
        real(c_double), allocatable :: lo(:, :), hi(:, :), wrk(:, :), sub(:, :, :)
        type(c_ptr), allocatable :: us(:)
        integer, allocatable :: idx(:), ilim(:)
        integer :: iv, j, ns, nplim, ims_err
#endif

        pg = c_null_ptr
        if (igate /= 0) pg = c_loc(gate)
#ifdef USE_MPI
        allocate (lo(ny + 1, nv), hi(ny + 1, nv), wrk(ny + 1, nv), idx(nv), ilim(nv), us(nv))
        call TLab_AMD_Check(tlab_pdf_minmax_planes(nx, ny, nz, nv, u, int(igate, c_int), pg, lo, hi), 'tlab_pdf_minmax_planes')
        call MPI_ALLREDUCE(lo, wrk, (ny + 1)*nv, MPI_REAL8, MPI_MIN, MPI_COMM_WORLD, ims_err)
        lo = wrk
        call MPI_ALLREDUCE(hi, wrk, (ny + 1)*nv, MPI_REAL8, MPI_MAX, MPI_COMM_WORLD, ims_err)
        hi = wrk
        do iv = 1, nv
            if (ibc(iv) == 0) then
                lo(:, iv) = umin(iv); hi(:, iv) = umax(iv)
            end if
        end do
        call TLab_AMD_Check(tlab_pdf_histogram_planes(nx, ny, nz, nv, nbins, ibc, lo, hi, u, int(igate, c_int), pg, pdf), 'tlab_pdf_histogram_planes')
        call Reduce_Counts(nbins, (ny + 1)*nv, pdf)

        ns = 0                                          ! PDF_ANALIZE of the reduced histograms, then the analysed intervals as external ones
        do iv = 1, nv
            if (ibc(iv) > 1) then
                ns = ns + 1; idx(ns) = iv; us(ns) = u(iv); ilim(ns) = 0
                do j = 1, ny + 1
                    if (j <= ny .or. ny > 1) then
                        call TLab_AMD_Check(tlab_pdf_analize(ibc(iv) - 2, nbins, pdf(:, j, iv), lo(j, ns), hi(j, ns), 1.0e-4_c_double, nplim), &
                                            'tlab_pdf_analize')
                    end if
                end do
            end if
        end do
        if (ns > 0) then
            allocate (sub(nbins + 2, ny + 1, ns))
            call TLab_AMD_Check(tlab_pdf_histogram_planes(nx, ny, nz, ns, nbins, ilim, lo, hi, us, int(igate, c_int), pg, sub), &
                                'tlab_pdf_histogram_planes')
            call Reduce_Counts(nbins, (ny + 1)*ns, sub)
            do iv = 1, ns
                pdf(:, :, idx(iv)) = sub(:, :, iv)
            end do
        end if
#else
        call TLab_AMD_Check(tlab_pdf1v_n(nx, ny, nz, nv, nbins, ibc, umin, umax, u, int(igate, c_int), pg, pdf), 'tlab_pdf1v_n')
#endif
    end subroutine TLab_AMD_PDF1V_N

    subroutine TLab_AMD_PDF2V(nx, ny, nz, nbins, u, v, pdf)
        integer, intent(in) :: nx, ny, nz, nbins(2)
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz)
        real(c_double), intent(out) :: pdf(nbins(1)*nbins(2) + 2 + 2*nbins(1), ny + 1)

        call TLab_AMD_Check(tlab_pdf2v(nx, ny, nz, nbins, c_loc(u), c_loc(v), pdf), 'tlab_pdf2v')
    end subroutine TLab_AMD_PDF2V

    ! avg(1:nbins, j, iv) = <a | u(iv)> in the nbins bins of plane j, then the centres of the first and the last bin; the volume as plane ny + 1
    subroutine TLab_AMD_CAVG1V_N(nx, ny, nz, nv, nbins, ibc, umin, umax, u, igate, gate, a, avg)
        integer, intent(in) :: nx, ny, nz, nv, nbins, ibc(nv)
        real(c_double), intent(in) :: umin(nv), umax(nv)
        type(c_ptr), intent(in) :: u(nv)
        integer(1), intent(in), target :: gate(*), igate
        real(c_double), intent(in), target :: a(nx*ny*nz)
        real(c_double), intent(out) :: avg(nbins + 2, ny + 1, nv)
        type(c_ptr) :: pg

        pg = c_null_ptr
        if (igate /= 0) pg = c_loc(gate)
        call TLab_AMD_Check(tlab_cavg1v_n(nx, ny, nz, nv, nbins, ibc, umin, umax, u, int(igate, c_int), pg, c_loc(a), avg, c_null_ptr, c_null_ptr), &
                            'tlab_cavg1v_n')
    end subroutine TLab_AMD_CAVG1V_N

    subroutine TLab_AMD_CAVG2V(nx, ny, nz, nbins, u, v, a, avg)
        integer, intent(in) :: nx, ny, nz, nbins(2)
        real(c_double), intent(in), target :: u(nx*ny*nz), v(nx*ny*nz), a(nx*ny*nz)
        real(c_double), intent(out) :: avg(nbins(1)*nbins(2) + 2 + 2*nbins(1), ny + 1)

        call TLab_AMD_Check(tlab_cavg2v(nx, ny, nz, nbins, c_loc(u), c_loc(v), c_loc(a), avg), 'tlab_cavg2v')
    end subroutine TLab_AMD_CAVG2V

#ifdef USE_MPI
    ! the reduction of PDF1V2D (utils/pdfs.f90:92-95) on np histograms: the counts are summed, the two centres behind them stay
    subroutine Reduce_Counts(nbins, np, pdf)
        integer, intent(in) :: nbins, np
        real(c_double), intent(inout) :: pdf(nbins + 2, np)
        real(c_double), allocatable :: loc(:, :), glo(:, :)
        integer :: ims_err

        allocate (loc(nbins, np), glo(nbins, np))
        loc = pdf(1:nbins, :)
        call MPI_ALLREDUCE(loc, glo, nbins*np, MPI_REAL8, MPI_SUM, MPI_COMM_WORLD, ims_err)
        pdf(1:nbins, :) = glo
    end subroutine Reduce_Counts
#endif

end module TLab_AMD_PDFs
