# tools/dns/dns_local.f90 of the reference -> DNS_BOUNDS_LIMIT with its scalar loop on the device (INTEGRATION.md section 3b).
# Applied by the host's build to $(REF)/src/tools/dns/dns_local.f90 where it lies; nothing of that file is kept in this repo.
#
# The loop `s(:, is) = min(max(s(:, is), bound_s(is)%min), bound_s(is)%max)` over the active scalars is an array statement of the host over
# device memory (s is in HBM, tlab_memory_device.sed): with the deferred tail on it would run before the recorded update and be overwritten by it.
# It becomes one call of TLab_AMD_Bounds_Limit (tlab_amd_bounds.f90), which hands each active scalar to tlab_deferred_clip.  bound_r / bound_p
# (q(:, 5), q(:, 6): compressible runs only) are left as they are.
/^ *subroutine DNS_BOUNDS_LIMIT/,/^ *end subroutine DNS_BOUNDS_LIMIT/{
/^ *use TLab_Arrays *$/a\
        use TLab_AMD_Bounds, only: TLab_AMD_Bounds_Limit
/^ *do is = 1, inb_scal/,/^ *end do/{
/^ *end do/c\
        call TLab_AMD_Bounds_Limit(s, size(s, 1), inb_scal, bound_s(1:inb_scal)%active, bound_s(1:inb_scal)%min, bound_s(1:inb_scal)%max)
d
}
}
