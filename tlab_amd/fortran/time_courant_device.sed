# tools/dns/time.f90 of the reference -> TIME_COURANT with its incompressible CFL maximum on the device (INTEGRATION.md section 3c).
# Applied by the host's build to $(REF)/src/tools/dns/time.f90 where it lies; nothing of that file is kept in this repo.
#
# The loops over u, v, w into p_wrk3d and the maxval(p_wrk3d) that follows them (time.f90:402-423, :452) are host loops over device memory
# (tlab_memory_device.sed).  In the incompressible / anelastic branch they become one call of TLab_AMD_Courant (tlab_amd_monitors.f90): this
# rank's pmax(1:2) from the device.  The compressible branch keeps its maxval; the MPI_ALLREDUCE (:522), the choice of dtime and logs_data(2:3)
# (:543-544) stay the reference's own code.
/^ *subroutine TIME_COURANT/,/^ *end subroutine TIME_COURANT/{
/^ *use TLab_Pointers_3D, only: u, v, w, p_wrk3d, p, rho, vis *$/a\
        use TLab_AMD_Monitors, only: TLab_AMD_Courant
/Incompressible: Calculate global maximum of u\/dx + v\/dy + w\/dz/,/^ *end if *$/{
/^ *if (z%size > 1) then *$/,/^ *end if *$/{
/^ *end if *$/c\
            call TLab_AMD_Courant(pmax(1:2))
d
}
}
s/^\( *\)pmax(1) = maxval(p_wrk3d) *$/\1if (nse_eqns == DNS_EQNS_INTERNAL .or. nse_eqns == DNS_EQNS_TOTAL) pmax(1) = maxval(p_wrk3d)/
}
