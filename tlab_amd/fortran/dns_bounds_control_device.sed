# tools/dns/dns_local.f90 of the reference -> DNS_BOUNDS_CONTROL with its dilatation check on the device (INTEGRATION.md section 3c).
# Applied by the host's build to $(REF)/src/tools/dns/dns_local.f90 where it lies, after dns_local_device.sed; nothing of that file is kept here.
#
# In the incompressible / anelastic branch, FI_INVARIANT_P (with its anelastic weights, :160-170), MINMAX and the sign change (:184-187) become one
# call of TLab_AMD_Dilatation (tlab_amd_monitors.f90): DilMin / DilMax and the global (i, j, k) of each from the device.  IBM runs are refused
# there.  In the failure branch the maxval / minval / maxloc / minloc of wrk3d (:193-225) take those values; the locations already carry
# ims_offset_i / ims_offset_k.  The bound test (:190) and the log lines stay the reference's own.
/^ *subroutine DNS_BOUNDS_CONTROL/,/^ *end subroutine DNS_BOUNDS_CONTROL/{
/^ *use TLab_Arrays *$/a\
        use TLab_AMD_Monitors, only: TLab_AMD_Dilatation
/^ *integer(wi) idummy(3) *$/a\
        integer dil_imn(3), dil_imx(3)
/^            if (nse_eqns == DNS_EQNS_ANELASTIC) then *$/,/^            end if *$/d
/^            if (imode_ibm == 1) then *$/,/^            end if *$/d
/^ *call MINMAX(imax, jmax, kmax, txc(1, 1), d_max_loc, d_min_loc) *$/c\
            call TLab_AMD_Dilatation(d_min_loc, d_max_loc, dil_imn, dil_imx, imode_ibm)
/^ *d_min_loc = -d_min_loc; d_max_loc = -d_max_loc *$/d
/^ *wrk3d = -txc(:, 1) *$/d
/^ *loc_max(1:imax, 1:jmax, 1:kmax) => wrk3d(1:imax\*jmax\*kmax) *$/d
s/^\( *\)dummy = maxval(wrk3d) *$/\1dummy = d_max_loc/
s/^\( *\)dummy = minval(wrk3d) *$/\1dummy = d_min_loc/
s/^\( *\)idummy = maxloc(loc_max) *$/\1idummy = dil_imx/
s/^\( *\)idummy = minloc(loc_max) *$/\1idummy = dil_imn/
/^ *idummy(1) = idummy(1) + ims_offset_i *$/d
/^ *idummy(3) = idummy(3) + ims_offset_k *$/d
}
