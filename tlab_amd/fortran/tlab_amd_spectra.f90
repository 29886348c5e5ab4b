!########################################################################
! The plane spectra and correlations of the reference (tools/statistics/spectra.f90 with module SpectraMod, spectra_pool.f90) for a host whose
! fields live in device memory; the argument order is SpectraMod's (sizes, input, outputs), with what may be absent as optional arguments behind.
!   TLab_AMD_Reduce_Spectrum     REDUCE_SPECTRUM and INTEGRATE_SPECTRUM in one call, with the output arrays of both: a_hat and b_hat are the
!                                transformed fields themselves, complex (nx/2+1, ny, nz) in the natural kz order as 2 reals each (b_hat absent:
!                                an auto pair), not their product; the product, the scaling of spectra.f90:641 and the kz shuffle happen inside.
!                                out2d(nx/2, ny/nblock, nz) is the power half of REDUCE_SPECTRUM's out (the phase half is not built) and may be
!                                absent; outx, outz, outr and out2d are accumulated into; variance(ny) is written.
!   TLab_AMD_Integrate_Spectrum  the same call for a caller that keeps the reference's two names: it needs the transformed fields too, because
!                                the block-reduced spectrum never leaves the device in between.
!   TLab_AMD_Reduce_Correlation  REDUCE_CORRELATION on the UNSCALED field the inverse transforms return (the scaling of spectra.f90:653 happens
!                                inside); variance1(:, 1:2) normalise, variance2(ny) is written; data_r is touched only with icalc_radial == 1.
!   TLab_AMD_Radial_Samplesize   RADIAL_SAMPLESIZE, counted from zero.
!   TLab_AMD_Spectra_Pair        spectra.f90:620-659 for one pair of fluctuation fields on the transforms of a Poisson plan of the library
!                                (plan: its handle); mode 1 spectra, 2 correlations; tmp1-3: (nx+2)*ny*nz reals each; cov(ny, 3), variance(ny).
! The field-sized arrays are classified by the library (tlab_pointer_on_device): host arrays take the reference's loops on the host, so the first
! four routines serve either kind; a mix is refused.  variance, variance1, variance2, cov and samplesize are host memory.  Single rank: the MPI
! reductions of the tool are not built.  This module depends on TLab_AMD_C alone.
!########################################################################
module TLab_AMD_Spectra
    use TLab_AMD_C
    implicit none
    private
    public :: TLab_AMD_Reduce_Spectrum, TLab_AMD_Integrate_Spectrum, TLab_AMD_Reduce_Correlation, TLab_AMD_Radial_Samplesize
    public :: TLab_AMD_Spectra_Pair

contains
    subroutine TLab_AMD_Reduce_Spectrum(nx, ny, nz, nblock, kr_total, a_hat, outx, outz, outr, variance, b_hat, out2d)
        integer, intent(in) :: nx, ny, nz, nblock, kr_total
        real(c_double), intent(in), target :: a_hat(*)
        real(c_double), intent(inout), target :: outx(nx/2, ny/nblock), outz(nz/2, ny/nblock), outr(kr_total, ny/nblock)
        real(c_double), intent(out) :: variance(ny)
        real(c_double), intent(in), target, optional :: b_hat(*)
        real(c_double), intent(inout), target, optional :: out2d(nx/2, ny/nblock, nz)
        type(c_ptr) :: pb, p2

        pb = c_null_ptr; p2 = c_null_ptr
        if (present(b_hat)) pb = c_loc(b_hat)
        if (present(out2d)) p2 = c_loc(out2d)
        call TLab_AMD_Check(tlab_spectrum_reduce(nx, ny, nz, nblock, kr_total, c_loc(a_hat), pb, p2, c_loc(outx), c_loc(outz), c_loc(outr), &
                                                 variance), 'tlab_spectrum_reduce')
    end subroutine TLab_AMD_Reduce_Spectrum

    subroutine TLab_AMD_Integrate_Spectrum(nx, ny, nz, nblock, kr_total, a_hat, outx, outz, outr, variance, b_hat, out2d)
        integer, intent(in) :: nx, ny, nz, nblock, kr_total
        real(c_double), intent(in), target :: a_hat(*)
        real(c_double), intent(inout), target :: outx(nx/2, ny/nblock), outz(nz/2, ny/nblock), outr(kr_total, ny/nblock)
        real(c_double), intent(out) :: variance(ny)
        real(c_double), intent(in), target, optional :: b_hat(*)
        real(c_double), intent(inout), target, optional :: out2d(nx/2, ny/nblock, nz)

        call TLab_AMD_Reduce_Spectrum(nx, ny, nz, nblock, kr_total, a_hat, outx, outz, outr, variance, b_hat, out2d)
    end subroutine TLab_AMD_Integrate_Spectrum

    subroutine TLab_AMD_Reduce_Correlation(nx, ny, nz, nblock, nr_total, in, data_2d, data_x, data_z, data_r, variance1, variance2, icalc_radial)
        integer, intent(in) :: nx, ny, nz, nblock, nr_total
        real(c_double), intent(in), target :: in(nx, ny, nz)
        real(c_double), intent(inout), target :: data_2d(nx, ny/nblock, nz), data_x(nx, ny/nblock), data_z(nz, ny/nblock)
        real(c_double), intent(inout), target :: data_r(nr_total, ny/nblock)
        real(c_double), intent(in) :: variance1(:, :)             ! (isize_wrk1d, 2) in the reference: the first ny rows are read
        real(c_double), intent(out) :: variance2(ny)
        integer, intent(in), optional :: icalc_radial
        real(c_double) :: var1(ny), var2(ny)
        integer :: icalc

        icalc = 0
        if (present(icalc_radial)) icalc = icalc_radial
        var1 = variance1(1:ny, 1); var2 = variance1(1:ny, 2)
        call TLab_AMD_Check(tlab_correlation_reduce(nx, ny, nz, nblock, nr_total, c_loc(in), var1, var2, c_loc(data_2d), c_loc(data_x), &
                                                    c_loc(data_z), c_loc(data_r), variance2, icalc), 'tlab_correlation_reduce')
    end subroutine TLab_AMD_Reduce_Correlation

    subroutine TLab_AMD_Radial_Samplesize(nx, nz, nr_total, samplesize)
        integer, intent(in) :: nx, nz, nr_total
        real(c_double), intent(out) :: samplesize(nr_total)

        call TLab_AMD_Check(tlab_radial_samplesize(nx, nz, nr_total, samplesize), 'tlab_radial_samplesize')
    end subroutine TLab_AMD_Radial_Samplesize

    subroutine TLab_AMD_Spectra_Pair(plan, mode, nblock, kr_total, a, tmp1, tmp2, tmp3, outx, outz, outr, cov, variance, b, out2d)
        type(c_ptr), intent(in) :: plan
        integer, intent(in) :: mode, nblock, kr_total
        real(c_double), intent(in), target :: a(*)
        real(c_double), intent(inout), target :: tmp1(*), tmp2(*), tmp3(*), outx(*), outz(*), outr(*)
        real(c_double), intent(out) :: cov(*), variance(*)
        real(c_double), intent(in), target, optional :: b(*)
        real(c_double), intent(inout), target, optional :: out2d(*)
        type(c_ptr) :: pb, p2

        pb = c_null_ptr; p2 = c_null_ptr
        if (present(b)) pb = c_loc(b)
        if (present(out2d)) p2 = c_loc(out2d)
        call TLab_AMD_Check(tlab_spectra_pair(plan, mode, nblock, kr_total, c_loc(a), pb, c_loc(tmp1), c_loc(tmp2), c_loc(tmp3), p2, c_loc(outx), &
                                              c_loc(outz), c_loc(outr), cov, variance), 'tlab_spectra_pair')
    end subroutine TLab_AMD_Spectra_Pair

end module TLab_AMD_Spectra
