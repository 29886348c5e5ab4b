# src/physics/tlab_sources.f90 of the reference -> the body forces on the device (INTEGRATION.md section 3b).
# Applied by the host's build to $(REF)/src/physics/tlab_sources.f90 where it lies; nothing of that file is kept in this repo.
#
# TLab_Sources_Flow runs before the RHS in every substep (tools/dns/time.f90:610) and is a host loop over q, s, hq in device memory.
#  - Inside TLab_Sources_Flow the Rotation_Coriolis call becomes one call of TLab_AMD_Sources_Flow (tlab_amd_sources.f90), which pushes the settings
#    of [Rotation] and [BodyForce] when they changed and hands the routine to the driver; the buoyancy block (Gravity_Buoyancy and the loop over hq)
#    goes.
#  - Subsidence and the special forcing stay host loops over device memory: a guard stops the run when either is active.
#  - Nothing outside TLab_Sources_Flow changes (TLab_Sources_Scal is not covered).
/^ *subroutine TLab_Sources_Flow/,/^ *end subroutine TLab_Sources_Flow/{
/^ *use TLab_Time, only: rtime/a\
        use TLab_AMD_C, only: TLab_AMD_Check\
        use TLab_AMD_Sources, only: TLab_AMD_Sources_Flow\
        use TLab_AMD_DNS, only: TLab_AMD_DNS_Handle
/^ *call Rotation_Coriolis(coriolis, imax, jmax, kmax, q, hq)/c\
        if (any(subsidenceProps%active) .or. any(forcingProps%active)) &\
            call TLab_AMD_Check(-2, 'TLab_Sources_Flow: subsidence and SpecialForcing are not built on the device')\
        call TLab_AMD_Sources_Flow(TLab_AMD_DNS_Handle(), coriolis%type, coriolis%vector, coriolis%parameters, &\
                                   buoyancy%type, buoyancy%vector, buoyancy%scalar(1), buoyancy%parameters, &\
                                   inb_scal_array, bbackground, q, s, hq)
/^ *if (buoyancy%active(iq)) then/,/^!\$omp end parallel/d
/^ *! Buoyancy\. Remember/,/^ *! Subsidence/{
/^ *end if *$/d
}
}
