# tools/dns/boundary_buffer.f90 of the reference -> the relaxation zones on the device (INTEGRATION.md section 3b).
# Applied by the host's build to $(REF)/src/tools/dns/boundary_buffer.f90 where it lies; nothing of that file is kept in this repo.
#
# BOUNDARY_BUFFER_RELAX_FLOW is only ever called from RHS_GLOBAL_INCOMPRESSIBLE_1, which the library replaces: without this recipe the flow part is
# lost.  BOUNDARY_BUFFER_RELAX_SCAL is a host array statement over hs in device memory: with the deferred tail on it would run before the recorded RHS.
#  - At the end of BOUNDARY_BUFFER_INITIALIZE the blocks INI_BLOCK made are pushed to the driver (TLab_AMD_Buffer_Push, tlab_amd_buffer.f90): the four
#    J blocks, and an I block that has points, which the library refuses loudly (x is periodic there).
#  - The DEFAULT branch (incompressible, anelastic) of BOUNDARY_BUFFER_RELAX_SCAL becomes one call of TLab_AMD_Buffer_Relax_Scal.
/^ *subroutine BOUNDARY_BUFFER_INITIALIZE/,/^ *end subroutine BOUNDARY_BUFFER_INITIALIZE/{
/^ *subroutine BOUNDARY_BUFFER_INITIALIZE/a\
        use TLab_AMD_Buffer, only: TLab_AMD_Buffer_Push\
        use TLab_AMD_DNS, only: TLab_AMD_DNS_Handle
/^ *return *$/i\
        if (BuffFlowImin%size > 0) call TLab_AMD_Buffer_Push(TLab_AMD_DNS_Handle(), 1, 0, BuffFlowImin%size, BuffFlowImin%nfields, BuffFlowImin%tau, BuffFlowImin%ref)\
        if (BuffFlowImax%size > 0) call TLab_AMD_Buffer_Push(TLab_AMD_DNS_Handle(), 2, 0, BuffFlowImax%size, BuffFlowImax%nfields, BuffFlowImax%tau, BuffFlowImax%ref)\
        if (BuffScalImin%size > 0) call TLab_AMD_Buffer_Push(TLab_AMD_DNS_Handle(), 1, 1, BuffScalImin%size, BuffScalImin%nfields, BuffScalImin%tau, BuffScalImin%ref)\
        if (BuffScalImax%size > 0) call TLab_AMD_Buffer_Push(TLab_AMD_DNS_Handle(), 2, 1, BuffScalImax%size, BuffScalImax%nfields, BuffScalImax%tau, BuffScalImax%ref)\
        if (BuffFlowJmin%size > 0) call TLab_AMD_Buffer_Push(TLab_AMD_DNS_Handle(), 3, 0, BuffFlowJmin%size, BuffFlowJmin%nfields, BuffFlowJmin%tau, BuffFlowJmin%ref)\
        if (BuffFlowJmax%size > 0) call TLab_AMD_Buffer_Push(TLab_AMD_DNS_Handle(), 4, 0, BuffFlowJmax%size, BuffFlowJmax%nfields, BuffFlowJmax%tau, BuffFlowJmax%ref)\
        if (BuffScalJmin%size > 0) call TLab_AMD_Buffer_Push(TLab_AMD_DNS_Handle(), 3, 1, BuffScalJmin%size, BuffScalJmin%nfields, BuffScalJmin%tau, BuffScalJmin%ref)\
        if (BuffScalJmax%size > 0) call TLab_AMD_Buffer_Push(TLab_AMD_DNS_Handle(), 4, 1, BuffScalJmax%size, BuffScalJmax%nfields, BuffScalJmax%tau, BuffScalJmax%ref)
}
/^ *subroutine BOUNDARY_BUFFER_RELAX_SCAL()/,/^ *end subroutine BOUNDARY_BUFFER_RELAX_SCAL *$/{
/^ *subroutine BOUNDARY_BUFFER_RELAX_SCAL()/a\
        use TLab_AMD_Buffer, only: TLab_AMD_Buffer_Relax_Scal\
        use TLab_AMD_DNS, only: TLab_AMD_DNS_Handle
/^ *case DEFAULT/,/^ *end select/{
/call RELAX_BLOCK(1, BuffScalImin, s, hs)/c\
            call TLab_AMD_Buffer_Relax_Scal(TLab_AMD_DNS_Handle())
/call RELAX_BLOCK(/d
}
}
