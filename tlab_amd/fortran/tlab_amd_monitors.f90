!########################################################################
! The two monitors the main loop calls after every Runge-Kutta step (tools/dns/dns_main.f90:268, :273), on the device arrays of the host:
!   TLab_AMD_Courant     the incompressible pmax(1:2) of TIME_COURANT (tools/dns/time.f90:395-466), of THIS rank: the host's own MPI_ALLREDUCE
!                        (:522) follows.  Called by the recipe time_courant_device.sed.
!   TLab_AMD_Dilatation  DilMin / DilMax of DNS_BOUNDS_CONTROL (dns_local.f90:157-187) over the whole box, and the global (i, j, k) of each, which
!                        its failure branch prints (:193-225).  Called by the recipe dns_bounds_control_device.sed.
! Both pick the single-domain, slab or pencil driver by the rules of tlab_amd_dns.f90 (TLab_AMD_Slab_Active, TLab_AMD_Pencil_Active), and both run
! a recorded substep of the deferred tail first (it updates q).
!########################################################################
module TLab_AMD_Monitors
    use, intrinsic :: iso_c_binding
    use TLab_Constants, only: wp
    use TLab_Arrays, only: q, txc
    use TLab_AMD_C
    use TLab_AMD_DNS, only: TLab_AMD_DNS_Handle, TLab_AMD_Slab_Active, TLab_AMD_Slab_Handle, TLab_AMD_Pencil_Active, TLab_AMD_Pencil_Handle
    implicit none
    private
    public :: TLab_AMD_Courant, TLab_AMD_Dilatation

contains

    subroutine TLab_AMD_Courant(pmax)
        real(wp), intent(out) :: pmax(2)
        real(c_double) pm(2), dt
        type(c_ptr) pq(3)

        if (TLab_AMD_Pencil_Active()) then
            call TLab_AMD_Check(tlab_pencil_dns_courant_local(TLab_AMD_Pencil_Handle(), pm), 'tlab_pencil_dns_courant_local')
        else if (TLab_AMD_Slab_Active()) then
            call TLab_AMD_Check(tlab_slab_dns_courant_local(TLab_AMD_Slab_Handle(), pm), 'tlab_slab_dns_courant_local')
        else
            pq = [c_loc(q(1, 1)), c_loc(q(1, 2)), c_loc(q(1, 3))]
            dt = 0.0_c_double
            call TLab_AMD_Check(tlab_time_courant(TLab_AMD_DNS_Handle(), pq, 0.0_c_double, 0.0_c_double, pm, dt), 'tlab_time_courant')
        end if
        pmax = pm
    end subroutine TLab_AMD_Courant

    ! dmin, dmax = min / max of div(q); imn, imx = global 1-based (i, j, k) of their first occurrence (minloc / maxloc, ims_offset_i / _k included).
    ! Destroys txc(:, 1), txc(:, 6), txc(:, 7) (single domain; txc(:, 3:5) too in anelastic runs) or txc(:, 1), txc(:, 2), txc(:, 7), txc(:, 8)
    ! (slabs, pencils).  ibm = imode_ibm of the host: IBM runs are refused (IBM_BCS_FIELD is not built on the device), as are staggered ones.
    subroutine TLab_AMD_Dilatation(dmin, dmax, imn, imx, ibm)
        real(wp), intent(out) :: dmin, dmax
        integer, intent(out) :: imn(3), imx(3)
        integer, intent(in), optional :: ibm
        real(c_double) mn, mx
        integer(c_int) lmn(3), lmx(3)
        type(c_ptr) pq(3), ptxc(9)
        integer is

        if (present(ibm)) then
            if (ibm == 1) call TLab_AMD_Check(-2_c_int, 'DNS_BOUNDS_CONTROL: IBM runs keep the reference''s host code (TLAB_EUNSUPPORTED)')
        end if
        if (TLab_AMD_Pencil_Active()) then
            call TLab_AMD_Check(tlab_pencil_dns_dilatation_extremes(TLab_AMD_Pencil_Handle(), mn, mx, lmn, lmx), 'tlab_pencil_dns_dilatation_extremes')
        else if (TLab_AMD_Slab_Active()) then
            call TLab_AMD_Check(tlab_slab_dns_dilatation_extremes(TLab_AMD_Slab_Handle(), mn, mx, lmn, lmx), 'tlab_slab_dns_dilatation_extremes')
        else
            if (size(txc, 2) < 7) call TLab_AMD_Check(-1_c_int, 'TLab_AMD_Dilatation: needs inb_txc >= 7')
            pq = [c_loc(q(1, 1)), c_loc(q(1, 2)), c_loc(q(1, 3))]
            ptxc = c_null_ptr
            do is = 1, min(size(txc, 2), 9)
                ptxc(is) = c_loc(txc(1, is))
            end do
            call TLab_AMD_Check(tlab_dns_dilatation_extremes(TLab_AMD_DNS_Handle(), pq, ptxc, mn, mx, lmn, lmx), 'tlab_dns_dilatation_extremes')
        end if
        dmin = mn; dmax = mx
        imn = lmn; imx = lmx
    end subroutine TLab_AMD_Dilatation

end module TLab_AMD_Monitors
