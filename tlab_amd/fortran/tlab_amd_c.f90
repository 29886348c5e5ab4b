!########################################################################
! ISO_C_BINDING interfaces of the C ABI in include/tlab_amd.h.
! One interface per entry point; names and argument order are those of the header.
!########################################################################
module TLab_AMD_C
    use, intrinsic :: iso_c_binding
    implicit none
    public

    ! struct tlab_slab_transport (include/tlab_amd.h): filled by tlab_comm_slab_transport / tlab_slab_transport_loopback, or by the host with the
    ! five entry points of its own (GPU-aware MPI)
    type, bind(C) :: tlab_slab_transport
        type(c_ptr) :: ctx = c_null_ptr
        integer(c_int) :: nranks = 1, nlocal = 1, first = 0
        type(c_funptr) :: ring_start = c_null_funptr, alltoallv_start = c_null_funptr, wait = c_null_funptr, allreduce = c_null_funptr, &
                          destroy = c_null_funptr
    end type tlab_slab_transport

    ! struct tlab_pencil_transport: MPI_Alltoallv inside the world / ims_comm_x / ims_comm_z communicators for the x/z pencil driver (tlab_pencil_dns_*)
    type, bind(C) :: tlab_pencil_transport
        type(c_ptr) :: ctx = c_null_ptr
        integer(c_int) :: npro_i = 1, npro_k = 1, nlocal = 1, first = 0
        type(c_funptr) :: alltoallv_start = c_null_funptr, wait = c_null_funptr, allreduce = c_null_funptr, destroy = c_null_funptr
    end type tlab_pencil_transport

    interface
        integer(c_int) function tlab_finalize() bind(C, name='tlab_finalize')
            import :: c_int
        end function
        integer(c_int) function tlab_fdm_plan_create(plan, n, nodes, periodic, uniform, scheme1, scheme2, hyper_bc1_ext) bind(C, name='tlab_fdm_plan_create')
            import :: c_int, c_ptr, c_double
            type(c_ptr), intent(out) :: plan
            integer(c_int), value :: n, periodic, uniform, scheme1, scheme2
            real(c_double), intent(in) :: nodes(*)
            real(c_double), value :: hyper_bc1_ext
        end function
        integer(c_int) function tlab_device_count() bind(C, name='tlab_device_count')
            import :: c_int
        end function
        integer(c_int) function tlab_init(device) bind(C, name='tlab_init')
            import :: c_int
            integer(c_int), value :: device
        end function
        integer(c_int) function tlab_sync() bind(C, name='tlab_sync')
            import :: c_int
        end function
        function tlab_last_error() bind(C, name='tlab_last_error') result(p)
            import :: c_ptr
            type(c_ptr) :: p
        end function
        integer(c_int) function tlab_malloc(p, bytes) bind(C, name='tlab_malloc')
            import :: c_int, c_ptr, c_size_t
            type(c_ptr), intent(out) :: p
            integer(c_size_t), value :: bytes
        end function
        integer(c_int) function tlab_free(p) bind(C, name='tlab_free')
            import :: c_int, c_ptr
            type(c_ptr), value :: p
        end function
        integer(c_int) function tlab_memcpy_h2d(dst, src, bytes) bind(C, name='tlab_memcpy_h2d')
            import :: c_int, c_ptr, c_size_t
            type(c_ptr), value :: dst, src
            integer(c_size_t), value :: bytes
        end function
        integer(c_int) function tlab_memcpy_d2h(dst, src, bytes) bind(C, name='tlab_memcpy_d2h')
            import :: c_int, c_ptr, c_size_t
            type(c_ptr), value :: dst, src
            integer(c_size_t), value :: bytes
        end function
        integer(c_int) function tlab_fdm_plan_create_from_arrays(plan, n, periodic, need_1der, ndl1, ndr1, lhs1, rhs1, &
                                                                 ndl2, ndr2, lhs2, rhs2) bind(C, name='tlab_fdm_plan_create_from_arrays')
            import :: c_int, c_ptr, c_double
            type(c_ptr), intent(out) :: plan
            integer(c_int), value :: n, periodic, need_1der, ndl1, ndr1, ndl2, ndr2
            real(c_double), intent(in) :: lhs1(*), rhs1(*), lhs2(*), rhs2(*)
        end function
        integer(c_int) function tlab_fdm_plan_set_aux(plan, mwn1, mwn2, jac, nodes) bind(C, name='tlab_fdm_plan_set_aux')
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, mwn1, mwn2, jac, nodes
        end function
        integer(c_int) function tlab_fdm_plan_set_scheme(plan, mode1, mode2) bind(C, name='tlab_fdm_plan_set_scheme')
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: mode1, mode2
        end function
        integer(c_int) function tlab_fdm_plan_set_stagger(plan, mode) bind(C, name='tlab_fdm_plan_set_stagger')
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: mode
        end function
        integer(c_int) function tlab_fdm_plan_destroy(plan) bind(C, name='tlab_fdm_plan_destroy')
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
        end function
        integer(c_int) function tlab_opr_partial(dir, plan, itype, nx, ny, nz, ibc, u, res, tmp1) bind(C, name='tlab_opr_partial')
            import :: c_int, c_ptr
            integer(c_int), value :: dir, itype, nx, ny, nz, ibc
            type(c_ptr), value :: plan, u, res, tmp1
        end function
        integer(c_int) function tlab_opr_burgers(dir, plan, ivel, nx, ny, nz, ibc, nu, s, u, res, tmp1, write_transposed) &
            bind(C, name='tlab_opr_burgers')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: dir, ivel, nx, ny, nz, ibc, write_transposed
            real(c_double), value :: nu
            type(c_ptr), value :: plan, s, u, res, tmp1
        end function
        integer(c_int) function tlab_opr_burgers_set_anelastic(ny, rbackground, ribackground) bind(C, name='tlab_opr_burgers_set_anelastic')
            import :: c_int, c_ptr
            integer(c_int), value :: ny
            type(c_ptr), value :: rbackground, ribackground      ! host arrays of ny doubles (c_null_ptr: incompressible)
        end function
        integer(c_int) function tlab_filter_create(f, itype, n, periodic, bcsmin, bcsmax, inb_filter, coeffs) bind(C, name='tlab_filter_create')
            import :: c_int, c_ptr
            type(c_ptr), intent(out) :: f
            integer(c_int), value :: itype, n, periodic, bcsmin, bcsmax, inb_filter
            type(c_ptr), value :: coeffs                          ! host array f%coeffs(n, inb_filter)
        end function
        integer(c_int) function tlab_filter_destroy(f) bind(C, name='tlab_filter_destroy')
            import :: c_int, c_ptr
            type(c_ptr), value :: f
        end function
        integer(c_int) function tlab_opr_filter_1d(dir, f, nx, ny, nz, u, res) bind(C, name='tlab_opr_filter_1d')
            import :: c_int, c_ptr
            integer(c_int), value :: dir, nx, ny, nz
            type(c_ptr), value :: f, u, res
        end function
        integer(c_int) function tlab_opr_burgers_set_dealiasing(dir, f) bind(C, name='tlab_opr_burgers_set_dealiasing')
            import :: c_int, c_ptr
            integer(c_int), value :: dir
            type(c_ptr), value :: f
        end function
        integer(c_int) function tlab_dns_set_anelastic(dns, rbackground, ribackground) bind(C, name='tlab_dns_set_anelastic')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns, rbackground, ribackground
        end function
        integer(c_int) function tlab_poisson_plan_create(plan, gx, gy, gz, nx, ny, nz) bind(C, name='tlab_poisson_plan_create')
            import :: c_int, c_ptr
            type(c_ptr), intent(out) :: plan
            type(c_ptr), value :: gx, gy, gz
            integer(c_int), value :: nx, ny, nz
        end function
        integer(c_int) function tlab_poisson_plan_create_direct(plan, gx, gy, gz, nx, ny, nz, gy_elliptic) &
            bind(C, name='tlab_poisson_plan_create_direct')
            import :: c_int, c_ptr
            type(c_ptr), intent(out) :: plan
            type(c_ptr), value :: gx, gy, gz, gy_elliptic
            integer(c_int), value :: nx, ny, nz
        end function
        integer(c_int) function tlab_opr_poisson(plan, nx, ny, nz, ibc, p, tmp1, tmp2, bcs_hb, bcs_ht, dpdy) bind(C, name='tlab_opr_poisson')
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, p, tmp1, tmp2, bcs_hb, bcs_ht, dpdy
            integer(c_int), value :: nx, ny, nz, ibc
        end function
        integer(c_int) function tlab_opr_helmholtz(plan, nx, ny, nz, ibc, alpha, a, tmp1, tmp2, bcs_hb, bcs_ht) bind(C, name='tlab_opr_helmholtz')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: plan, a, tmp1, tmp2, bcs_hb, bcs_ht
            integer(c_int), value :: nx, ny, nz, ibc
            real(c_double), value :: alpha
        end function
        integer(c_int) function tlab_transpose(a, nra, nca, b) bind(C, name='tlab_transpose')
            import :: c_int, c_ptr
            type(c_ptr), value :: a, b
            integer(c_int), value :: nra, nca
        end function
        ! ---- RHS assembly / Runge-Kutta substep / wall boundary conditions (include/tlab_amd.h, "next" row n1) ----
        integer(c_int) function tlab_dns_create(dns, gx, gy, gz, poisson, nx, ny, nz, nscal, visc, schmidt) bind(C, name='tlab_dns_create')
            import :: c_int, c_ptr, c_double
            type(c_ptr), intent(out) :: dns
            type(c_ptr), value :: gx, gy, gz, poisson
            integer(c_int), value :: nx, ny, nz, nscal
            real(c_double), value :: visc
            real(c_double), intent(in) :: schmidt(*)
        end function
        integer(c_int) function tlab_dns_destroy(dns) bind(C, name='tlab_dns_destroy')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
        end function
        integer(c_int) function tlab_dns_set_bcs(dns, flow_jmin, flow_jmax, scal_jmin, scal_jmax) bind(C, name='tlab_dns_set_bcs')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
            integer(c_int), intent(in) :: flow_jmin(3), flow_jmax(3), scal_jmin(*), scal_jmax(*)
        end function
        integer(c_int) function tlab_dns_set_remove_divergence(dns, on) bind(C, name='tlab_dns_set_remove_divergence')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
            integer(c_int), value :: on
        end function
        integer(c_int) function tlab_dns_set_surface_bcs(dns, sfc_jmin, sfc_jmax, cpl_jmin, cpl_jmax) bind(C, name='tlab_dns_set_surface_bcs')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: dns
            integer(c_int), intent(in) :: sfc_jmin(*), sfc_jmax(*)
            real(c_double), intent(in) :: cpl_jmin(*), cpl_jmax(*)
        end function
        integer(c_int) function tlab_dns_begin_step(dns) bind(C, name='tlab_dns_begin_step')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
        end function
        integer(c_int) function tlab_dns_place_blocks(dns, ncand, cand_q, cand_s, cand_hq, cand_hs, cand_txc, txc_stride, dtime, random_trials, seed, &
                                                      choice, report) bind(C, name='tlab_dns_place_blocks')
            import :: c_int, c_ptr, c_double, c_long_long
            type(c_ptr), value :: dns
            integer(c_int), value :: ncand, random_trials, seed
            type(c_ptr), intent(in) :: cand_q(*), cand_s(*), cand_hq(*), cand_hs(*), cand_txc(*)
            integer(c_long_long), value :: txc_stride
            real(c_double), value :: dtime
            integer(c_int), intent(out) :: choice(5)
            real(c_double), intent(out) :: report(5)
        end function
        ! ---- the substep's tail for an unpatched time loop (include/tlab_amd.h: tlab_deferred_*, csrc/deferred.cpp) ----
        integer(c_int) function tlab_deferred_enable(on) bind(C, name='tlab_deferred_enable')
            import :: c_int
            integer(c_int), value :: on
        end function
        integer(c_int) function tlab_deferred_rhs(dns, dte, q, s, hq, hs, txc) bind(C, name='tlab_deferred_rhs')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: dns
            real(c_double), value :: dte
            type(c_ptr), intent(in) :: q(*), s(*), hq(*), hs(*), txc(*)
        end function
        integer(c_int) function tlab_deferred_slab_rhs(slab, dte) bind(C, name='tlab_deferred_slab_rhs')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: slab
            real(c_double), value :: dte
        end function
        integer(c_int) function tlab_deferred_pencil_rhs(pencil, dte) bind(C, name='tlab_deferred_pencil_rhs')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: pencil
            real(c_double), value :: dte
        end function
        integer(c_int) function tlab_deferred_axpy(n, a, x, y) bind(C, name='tlab_deferred_axpy')
            import :: c_int, c_ptr, c_double, c_long_long
            integer(c_long_long), value :: n
            real(c_double), value :: a
            type(c_ptr), value :: x, y
        end function
        integer(c_int) function tlab_deferred_scal(n, a, x) bind(C, name='tlab_deferred_scal')
            import :: c_int, c_ptr, c_double, c_long_long
            integer(c_long_long), value :: n
            real(c_double), value :: a
            type(c_ptr), value :: x
        end function
        integer(c_int) function tlab_deferred_zero(a, n) bind(C, name='tlab_deferred_zero')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: a
            integer(c_long_long), value :: n
        end function
        integer(c_int) function tlab_deferred_flush() bind(C, name='tlab_deferred_flush')
            import :: c_int
        end function
        integer(c_int) function tlab_deferred_stats(counts) bind(C, name='tlab_deferred_stats')
            import :: c_int, c_long_long
            integer(c_long_long), intent(out) :: counts(6)
        end function
        ! DNS_BOUNDS_LIMIT of an unchanged host (dns_local_device.sed, TLab_AMD_Bounds_Limit): x = min(max(x, lo), hi), recorded like the BLAS calls
        integer(c_int) function tlab_deferred_clip(n, lo, hi, x) bind(C, name='tlab_deferred_clip')
            import :: c_int, c_ptr, c_double, c_long_long
            integer(c_long_long), value :: n
            real(c_double), value :: lo, hi
            type(c_ptr), value :: x
        end function
        integer(c_int) function tlab_deferred_clip_stats(counts) bind(C, name='tlab_deferred_clip_stats')
            import :: c_int, c_long_long
            integer(c_long_long), intent(out) :: counts(2)
        end function
        integer(c_int) function tlab_pointer_on_device(p) bind(C, name='tlab_pointer_on_device')
            import :: c_int, c_ptr
            type(c_ptr), value :: p
        end function
        integer(c_int) function tlab_pw_clip(a, lo, hi, n) bind(C, name='tlab_pw_clip')
            import :: c_int, c_ptr, c_double, c_long_long
            type(c_ptr), value :: a
            real(c_double), value :: lo, hi
            integer(c_long_long), value :: n
        end function
        ! [Control] ScalLimit of a patched host: the driver applies the bounds inside its substep (n <= nscal entries; active = c_null_ptr: off)
        integer(c_int) function tlab_dns_set_scalar_bounds(dns, n, active, lo, hi) bind(C, name='tlab_dns_set_scalar_bounds')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns, active, lo, hi
            integer(c_int), value :: n
        end function
        integer(c_int) function tlab_slab_dns_set_scalar_bounds(slab, n, active, lo, hi) bind(C, name='tlab_slab_dns_set_scalar_bounds')
            import :: c_int, c_ptr
            type(c_ptr), value :: slab, active, lo, hi
            integer(c_int), value :: n
        end function
        integer(c_int) function tlab_pencil_dns_set_scalar_bounds(pencil, n, active, lo, hi) bind(C, name='tlab_pencil_dns_set_scalar_bounds')
            import :: c_int, c_ptr
            type(c_ptr), value :: pencil, active, lo, hi
            integer(c_int), value :: n
        end function
        ! [BufferZone] Type = relaxation at Jmin / Jmax of a patched host (single-domain driver): iend = 3 Jmin / 4 Jmax, group = 0 flow / 1 scalars,
        ! tau(size, nfields) and ref(imax, size, kmax, nfields) = item%tau, item%ref of boundary_buffer.f90 as they stand (HOST); size = 0: off
        integer(c_int) function tlab_dns_set_buffer_type(dns, itype) bind(C, name='tlab_dns_set_buffer_type')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
            integer(c_int), value :: itype
        end function
        integer(c_int) function tlab_dns_set_buffer_zone(dns, iend, group, size, nfields, tau, ref) bind(C, name='tlab_dns_set_buffer_zone')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns, tau, ref
            integer(c_int), value :: iend, group, size, nfields
        end function
        integer(c_int) function tlab_buffer_tau(n, nodes, offset, size, strength, sigma, form, tau_out) bind(C, name='tlab_buffer_tau')
            import :: c_int, c_double
            integer(c_int), value :: n, offset, size, form
            real(c_double), value :: strength, sigma
            real(c_double), intent(in) :: nodes(*)
            real(c_double), intent(out) :: tau_out(*)
        end function
        ! BOUNDARY_BUFFER_RELAX_SCAL of an unchanged time loop: recorded after the deferred RHS, part of the one fused substep (csrc/deferred.cpp)
        integer(c_int) function tlab_deferred_relax_scal(dns) bind(C, name='tlab_deferred_relax_scal')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
        end function
        integer(c_int) function tlab_deferred_relax_stats(counts) bind(C, name='tlab_deferred_relax_stats')
            import :: c_int, c_long_long
            integer(c_long_long), intent(out) :: counts(2)
        end function
        ! [Rotation] and [BodyForce] of a patched host (tlab_amd_sources.f90): vector(3), parameters and bbackground(jmax) in HOST memory; itype = the
        ! reference's EQNS_COR_* / EQNS_BOD_* codes; nscalars = buoyancy%scalar(1); bbackground may be c_null_ptr (zeros)
        integer(c_int) function tlab_dns_set_coriolis(dns, itype, vector, parameters) bind(C, name='tlab_dns_set_coriolis')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: dns
            integer(c_int), value :: itype
            real(c_double), intent(in) :: vector(3), parameters(2)
        end function
        integer(c_int) function tlab_dns_set_buoyancy(dns, itype, vector, nscalars, parameters, nparameters, inb_scal_array, bbackground) &
            bind(C, name='tlab_dns_set_buoyancy')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: dns, bbackground
            integer(c_int), value :: itype, nscalars, nparameters, inb_scal_array
            real(c_double), intent(in) :: vector(3), parameters(*)
        end function
        integer(c_long_long) function tlab_dns_info(dns, what) bind(C, name='tlab_dns_info')      ! 0 nx, 1 ny, 2 nz, 3 nscal, 4 points of a field
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: dns
            integer(c_int), value :: what
        end function
        ! TLab_Sources_Flow on (q, s, hq): on its own, and as the marker of the deferred tail (csrc/deferred.cpp)
        integer(c_int) function tlab_dns_sources_flow(dns, q, s, hq) bind(C, name='tlab_dns_sources_flow')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
            type(c_ptr), intent(in) :: q(*), s(*), hq(*)      ! host arrays of device pointers
        end function
        ! FI_PRESSURE_BOUSSINESQ (tlab_amd_pressure.f90): p, tmp1, tmp2 and the ntmp arrays of tmp hold isize_txc_field values each
        integer(c_int) function tlab_dns_pressure(dns, decomposition, q, s, p, tmp1, tmp2, tmp, ntmp) bind(C, name='tlab_dns_pressure')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns, p, tmp1, tmp2
            integer(c_int), value :: decomposition, ntmp
            type(c_ptr), intent(in) :: q(3), s(*), tmp(*)
        end function
        integer(c_int) function tlab_deferred_sources_flow(dns, q, s, hq) bind(C, name='tlab_deferred_sources_flow')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
            type(c_ptr), intent(in) :: q(*), s(*), hq(*)
        end function
        integer(c_int) function tlab_deferred_sources_stats(counts) bind(C, name='tlab_deferred_sources_stats')
            import :: c_int, c_long_long
            integer(c_long_long), intent(out) :: counts(2)
        end function
        integer(c_int) function tlab_dns_buffer_relax_flow(dns, q, hq) bind(C, name='tlab_dns_buffer_relax_flow')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
            type(c_ptr), intent(in) :: q(*), hq(*)        ! host arrays of device pointers
        end function
        integer(c_int) function tlab_dns_buffer_relax_scal(dns, s, hs) bind(C, name='tlab_dns_buffer_relax_scal')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
            type(c_ptr), intent(in) :: s(*), hs(*)
        end function
        integer(c_int) function tlab_rhs_global_incompressible_1(dns, dte, q, s, hq, hs, txc) bind(C, name='tlab_rhs_global_incompressible_1')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: dns
            real(c_double), value :: dte
            type(c_ptr), intent(in) :: q(*), s(*), hq(*), hs(*), txc(*)        ! host arrays of device pointers
        end function
        integer(c_int) function tlab_time_substep_incompressible_explicit(dns, dte, kco, scale_tendencies, q, s, hq, hs, txc) &
            bind(C, name='tlab_time_substep_incompressible_explicit')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: dns
            real(c_double), value :: dte, kco
            integer(c_int), value :: scale_tendencies
            type(c_ptr), intent(in) :: q(*), s(*), hq(*), hs(*), txc(*)
        end function
        integer(c_int) function tlab_time_courant(dns, q, cfla, cfld, pmax, dtime) bind(C, name='tlab_time_courant')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: dns
            type(c_ptr), intent(in) :: q(*)
            real(c_double), value :: cfla, cfld
            real(c_double), intent(out) :: pmax(2), dtime
        end function
        integer(c_int) function tlab_pw_rk_update(q, h, dte, kco, scale, n) bind(C, name='tlab_pw_rk_update')
            import :: c_int, c_ptr, c_double, c_long_long
            type(c_ptr), value :: q, h
            real(c_double), value :: dte, kco
            integer(c_int), value :: scale
            integer(c_long_long), value :: n
        end function
        integer(c_int) function tlab_pw_fill(a, val, n) bind(C, name='tlab_pw_fill')
            import :: c_int, c_ptr, c_double, c_long_long
            type(c_ptr), value :: a
            real(c_double), value :: val
            integer(c_long_long), value :: n
        end function
        integer(c_int) function tlab_pw_scale(a, alpha, n) bind(C, name='tlab_pw_scale')
            import :: c_int, c_ptr, c_double, c_long_long
            type(c_ptr), value :: a
            real(c_double), value :: alpha
            integer(c_long_long), value :: n
        end function
        ! ---- x/z pencils (ims_npro_i > 1): tlab_pencil_dns_* of include/tlab_amd.h ----
        integer(c_int) function tlab_pencil_transport_loopback(tr, npro_i, npro_k) bind(C, name='tlab_pencil_transport_loopback')
            import :: c_int, tlab_pencil_transport
            type(tlab_pencil_transport), intent(out) :: tr
            integer(c_int), value :: npro_i, npro_k
        end function
        ! the partitioned z systems of a slab (include/tlab_amd.h): used here as the test whether slabs of kmax planes are thick enough (TLAB_EUNSUPPORTED: no)
        integer(c_int) function tlab_zslab_plan_create(plan, gz, kmax, koffset, chunk) bind(C, name='tlab_zslab_plan_create')
            import :: c_int, c_ptr
            type(c_ptr), intent(out) :: plan
            type(c_ptr), value :: gz
            integer(c_int), value :: kmax, koffset, chunk
        end function
        integer(c_int) function tlab_zslab_plan_destroy(plan) bind(C, name='tlab_zslab_plan_destroy')
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
        end function
        integer(c_int) function tlab_pencil_dns_create(d, tr, gx, gy, gz, nx, ny, nz_total, nscal, visc, schmidt) bind(C, name='tlab_pencil_dns_create')
            import :: c_int, c_ptr, c_double, tlab_pencil_transport
            type(c_ptr), intent(out) :: d
            type(tlab_pencil_transport), intent(in) :: tr
            type(c_ptr), value :: gx, gy, gz
            integer(c_int), value :: nx, ny, nz_total, nscal
            real(c_double), value :: visc
            real(c_double), intent(in) :: schmidt(*)
        end function
        integer(c_int) function tlab_pencil_dns_destroy(d) bind(C, name='tlab_pencil_dns_destroy')
            import :: c_int, c_ptr
            type(c_ptr), value :: d
        end function
        integer(c_int) function tlab_pencil_dns_bind(d, l, q, s, hq, hs, txc) bind(C, name='tlab_pencil_dns_bind')
            import :: c_int, c_ptr
            type(c_ptr), value :: d
            integer(c_int), value :: l
            type(c_ptr), intent(in) :: q(*), s(*), hq(*), hs(*), txc(*)
        end function
        integer(c_long_long) function tlab_pencil_dns_info(d, what) bind(C, name='tlab_pencil_dns_info')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: d
            integer(c_int), value :: what
        end function
        integer(c_int) function tlab_pencil_dns_set_bcs(d, flow_jmin, flow_jmax, scal_jmin, scal_jmax) bind(C, name='tlab_pencil_dns_set_bcs')
            import :: c_int, c_ptr
            type(c_ptr), value :: d
            integer(c_int), intent(in) :: flow_jmin(*), flow_jmax(*), scal_jmin(*), scal_jmax(*)
        end function
        integer(c_int) function tlab_pencil_dns_begin_step(d) bind(C, name='tlab_pencil_dns_begin_step')
            import :: c_int, c_ptr
            type(c_ptr), value :: d
        end function
        integer(c_int) function tlab_pencil_dns_rhs(d, dte) bind(C, name='tlab_pencil_dns_rhs')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            real(c_double), value :: dte
        end function
        integer(c_int) function tlab_pencil_dns_substep(d, dte, kco, scale) bind(C, name='tlab_pencil_dns_substep')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            real(c_double), value :: dte, kco
            integer(c_int), value :: scale
        end function
        ! ---- the decomposed substep (ims_npro_k > 1): tlab_slab_dns_* of include/tlab_amd.h ----
        integer(c_int) function tlab_slab_transport_loopback(tr, nranks) bind(C, name='tlab_slab_transport_loopback')
            import :: c_int, tlab_slab_transport
            type(tlab_slab_transport), intent(out) :: tr
            integer(c_int), value :: nranks
        end function
        integer(c_int) function tlab_slab_dns_create(d, tr, gx, gy, gz, nx, ny, nz_total, nscal, visc, schmidt, gy_elliptic) bind(C, name='tlab_slab_dns_create')
            import :: c_int, c_ptr, c_double, tlab_slab_transport
            type(c_ptr), intent(out) :: d
            type(tlab_slab_transport), intent(in) :: tr
            type(c_ptr), value :: gx, gy, gz, gy_elliptic
            integer(c_int), value :: nx, ny, nz_total, nscal
            real(c_double), value :: visc
            real(c_double), intent(in) :: schmidt(*)
        end function
        integer(c_int) function tlab_slab_dns_destroy(d) bind(C, name='tlab_slab_dns_destroy')
            import :: c_int, c_ptr
            type(c_ptr), value :: d
        end function
        integer(c_int) function tlab_slab_dns_bind(d, l, q, s, hq, hs, txc) bind(C, name='tlab_slab_dns_bind')
            import :: c_int, c_ptr
            type(c_ptr), value :: d
            integer(c_int), value :: l
            type(c_ptr), intent(in) :: q(*), s(*), hq(*), hs(*), txc(*)
        end function
        integer(c_long_long) function tlab_slab_dns_info(d, what) bind(C, name='tlab_slab_dns_info')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: d
            integer(c_int), value :: what
        end function
        integer(c_int) function tlab_slab_dns_set_bcs(d, flow_jmin, flow_jmax, scal_jmin, scal_jmax) bind(C, name='tlab_slab_dns_set_bcs')
            import :: c_int, c_ptr
            type(c_ptr), value :: d
            integer(c_int), intent(in) :: flow_jmin(*), flow_jmax(*), scal_jmin(*), scal_jmax(*)
        end function
        integer(c_int) function tlab_slab_dns_begin_step(d) bind(C, name='tlab_slab_dns_begin_step')
            import :: c_int, c_ptr
            type(c_ptr), value :: d
        end function
        integer(c_int) function tlab_slab_dns_set_surface_bcs(d, sfc_jmin, sfc_jmax, cpl_jmin, cpl_jmax) bind(C, name='tlab_slab_dns_set_surface_bcs')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            integer(c_int), intent(in) :: sfc_jmin(*), sfc_jmax(*)
            real(c_double), intent(in) :: cpl_jmin(*), cpl_jmax(*)
        end function
        integer(c_int) function tlab_slab_dns_set_remove_divergence(d, on) bind(C, name='tlab_slab_dns_set_remove_divergence')
            import :: c_int, c_ptr
            type(c_ptr), value :: d
            integer(c_int), value :: on
        end function
        integer(c_int) function tlab_slab_dns_rhs(d, dte) bind(C, name='tlab_slab_dns_rhs')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            real(c_double), value :: dte
        end function
        integer(c_int) function tlab_slab_dns_substep(d, dte, kco, scale_tendencies) bind(C, name='tlab_slab_dns_substep')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            real(c_double), value :: dte, kco
            integer(c_int), value :: scale_tendencies
        end function
        integer(c_int) function tlab_slab_dns_time_courant(d, cfla, cfld, pmax, dtime) bind(C, name='tlab_slab_dns_time_courant')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            real(c_double), value :: cfla, cfld
            real(c_double), intent(out) :: pmax(2), dtime
        end function
        integer(c_int) function tlab_slab_dns_dilatation_bounds(d, dil_min, dil_max) bind(C, name='tlab_slab_dns_dilatation_bounds')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            real(c_double), intent(out) :: dil_min, dil_max
        end function
        ! the monitors of the main loop (TIME_COURANT, DNS_BOUNDS_CONTROL; module TLab_AMD_Monitors)
        integer(c_int) function tlab_slab_dns_courant_local(d, pmax) bind(C, name='tlab_slab_dns_courant_local')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            real(c_double), intent(out) :: pmax(2)
        end function
        integer(c_int) function tlab_pencil_dns_courant_local(d, pmax) bind(C, name='tlab_pencil_dns_courant_local')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            real(c_double), intent(out) :: pmax(2)
        end function
        integer(c_int) function tlab_dns_dilatation_extremes(d, q, txc, dil_min, dil_max, loc_min, loc_max) bind(C, name='tlab_dns_dilatation_extremes')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            type(c_ptr), intent(in) :: q(*), txc(*)
            real(c_double), intent(out) :: dil_min, dil_max
            integer(c_int), intent(out) :: loc_min(3), loc_max(3)
        end function
        integer(c_int) function tlab_slab_dns_dilatation_extremes(d, dil_min, dil_max, loc_min, loc_max) bind(C, name='tlab_slab_dns_dilatation_extremes')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            real(c_double), intent(out) :: dil_min, dil_max
            integer(c_int), intent(out) :: loc_min(3), loc_max(3)
        end function
        integer(c_int) function tlab_pencil_dns_dilatation_extremes(d, dil_min, dil_max, loc_min, loc_max) bind(C, name='tlab_pencil_dns_dilatation_extremes')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: d
            real(c_double), intent(out) :: dil_min, dil_max
            integer(c_int), intent(out) :: loc_min(3), loc_max(3)
        end function
        integer(c_int) function tlab_minmax_any(a, n, amn, amx) bind(C, name='tlab_minmax_any')
            import :: c_int, c_ptr, c_double, c_long_long
            type(c_ptr), value :: a
            integer(c_long_long), value :: n
            real(c_double), intent(out) :: amn, amx
        end function
        ! plane statistics (tlab_amd_averages.f90): fields of either kind (all device or all host), profiles in host memory
        integer(c_int) function tlab_avg_ik_v(nx, ny, nz, nf, a, avg, ldavg) bind(C, name='tlab_avg_ik_v')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz, nf, ldavg
            type(c_ptr), intent(in) :: a(*)
            real(c_double), intent(out) :: avg(*)
        end function
        integer(c_int) function tlab_avg1v2d_v(nx, ny, nz, imom, a, avg) bind(C, name='tlab_avg1v2d_v')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz, imom
            type(c_ptr), value :: a
            real(c_double), intent(out) :: avg(*)
        end function
        integer(c_int) function tlab_avg_moments_flow(nx, ny, nz, u, v, w, p, fU, fV, fW, rP, out, ldout) bind(C, name='tlab_avg_moments_flow')
            import :: c_int, c_ptr
            integer(c_int), value :: nx, ny, nz, ldout
            type(c_ptr), value :: u, v, w, p, fU, fV, fW, rP, out
        end function
        integer(c_int) function tlab_avg_moments_scal(nx, ny, nz, s, u, v, w, p, fS, fU, fV, fW, rP, out, ldout) bind(C, name='tlab_avg_moments_scal')
            import :: c_int, c_ptr
            integer(c_int), value :: nx, ny, nz, ldout
            type(c_ptr), value :: s, u, v, w, p, fS, fU, fV, fW, rP, out
        end function
        ! ... on derivative fields: grad(9) = dudx dudy dudz dvdx dvdy dvdz dwdx dwdy dwdz, grads(3) = dsdx dsdy dsdz
        integer(c_int) function tlab_avg_gradients_flow(nx, ny, nz, grad, u, v, w, p, fU, fV, fW, rP, rU_y, rV_y, rW_y, out, ldout) &
            bind(C, name='tlab_avg_gradients_flow')
            import :: c_int, c_ptr
            integer(c_int), value :: nx, ny, nz, ldout
            type(c_ptr), intent(in) :: grad(9)
            type(c_ptr), value :: u, v, w, p, fU, fV, fW, rP, rU_y, rV_y, rW_y, out
        end function
        integer(c_int) function tlab_avg_ugradp(nx, ny, nz, u, v, w, dpdx, dpdy, dpdz, out) bind(C, name='tlab_avg_ugradp')
            import :: c_int, c_ptr
            integer(c_int), value :: nx, ny, nz
            type(c_ptr), value :: u, v, w, dpdx, dpdy, dpdz, out
        end function
        integer(c_int) function tlab_avg_gradients_scal(nx, ny, nz, grads, s, u, v, w, p, fS, fU, fV, fW, rP, rS_y, fS_y, out, ldout) &
            bind(C, name='tlab_avg_gradients_scal')
            import :: c_int, c_ptr
            integer(c_int), value :: nx, ny, nz, ldout
            type(c_ptr), intent(in) :: grads(3)
            type(c_ptr), value :: s, u, v, w, p, fS, fU, fV, fW, rP, rS_y, fS_y, out
        end function
        integer(c_int) function tlab_avg_gradients_pass(pass, with_p, nx, ny, nz, fields, means, out, ldout) bind(C, name='tlab_avg_gradients_pass')
            import :: c_int, c_ptr
            integer(c_int), value :: pass, with_p, nx, ny, nz, ldout
            type(c_ptr), intent(in) :: fields(*), means(*)
            type(c_ptr), value :: out
        end function
        ! plane PDFs (tlab_amd_pdfs.f90): fields and gate of either kind (all device or all host), intervals and histograms in host memory
        integer(c_int) function tlab_pdf1v_n(nx, ny, nz, nv, nbins, ibc, umin, umax, u, igate, gate, pdf) bind(C, name='tlab_pdf1v_n')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz, nv, nbins, igate
            integer(c_int), intent(in) :: ibc(*)
            real(c_double), intent(in) :: umin(*), umax(*)
            type(c_ptr), intent(in) :: u(*)
            type(c_ptr), value :: gate
            real(c_double), intent(out) :: pdf(*)
        end function
        integer(c_int) function tlab_pdf_minmax_planes(nx, ny, nz, nv, u, igate, gate, umin, umax) bind(C, name='tlab_pdf_minmax_planes')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz, nv, igate
            type(c_ptr), intent(in) :: u(*)
            type(c_ptr), value :: gate
            real(c_double), intent(out) :: umin(*), umax(*)
        end function
        integer(c_int) function tlab_pdf_histogram_planes(nx, ny, nz, nv, nbins, ilim, umin, umax, u, igate, gate, pdf) &
            bind(C, name='tlab_pdf_histogram_planes')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz, nv, nbins, igate
            integer(c_int), intent(in) :: ilim(*)
            real(c_double), intent(in) :: umin(*), umax(*)
            type(c_ptr), intent(in) :: u(*)
            type(c_ptr), value :: gate
            real(c_double), intent(out) :: pdf(*)
        end function
        integer(c_int) function tlab_pdf_analize(ibc, nbins, pdf, umin, umax, plim, nplim) bind(C, name='tlab_pdf_analize')
            import :: c_int, c_double
            integer(c_int), value :: ibc, nbins
            real(c_double), intent(in) :: pdf(*)
            real(c_double), intent(inout) :: umin, umax
            real(c_double), value :: plim
            integer(c_int), intent(out) :: nplim
        end function
        integer(c_int) function tlab_pdf2v(nx, ny, nz, nbins, u, v, pdf) bind(C, name='tlab_pdf2v')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz
            integer(c_int), intent(in) :: nbins(2)
            type(c_ptr), value :: u, v
            real(c_double), intent(out) :: pdf(*)
        end function
        integer(c_int) function tlab_gate_threshold(a, n, thr, gate) bind(C, name='tlab_gate_threshold')
            import :: c_int, c_ptr, c_double, c_long_long
            type(c_ptr), value :: a, gate
            integer(c_long_long), value :: n
            real(c_double), value :: thr
        end function
        ! intermittency (tlab_amd_averages.f90): FI_VORTICITY on the driver's plans, txc6(6) the addresses of six work arrays; INTER_N_XZ of a gate
        ! of either kind, inter(ny, np) in host memory
        integer(c_int) function tlab_fi_vorticity(dns, u, v, w, result, txc6) bind(C, name='tlab_fi_vorticity')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns, u, v, w, result
            type(c_ptr), intent(in) :: txc6(6)
        end function
        integer(c_int) function tlab_inter_n_xz(nx, ny, nz, np, gate, inter) bind(C, name='tlab_inter_n_xz')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz, np
            type(c_ptr), value :: gate
            real(c_double), intent(out) :: inter(*)
        end function
        ! conditional statistics (declared in tlab_amd/csrc/tlab_amd_conditional.h; wrappers in tlab_amd_averages.f90, tlab_amd_pdfs.f90):
        ! the partition of FI_GATE, AVG_N_XZ for the levels 1 .. np of a gate in one
        ! pass (np = 0: ungated; avg, sums, nsample may be c_null_ptr, not all three), RAW_TO_CENTRAL, CAVG1V_N and CAVG2V; results in host memory
        integer(c_int) function tlab_gate_levels(a, n, igate_size, thr, gate) bind(C, name='tlab_gate_levels')
            import :: c_int, c_ptr, c_double, c_long_long
            type(c_ptr), value :: a, gate
            integer(c_long_long), value :: n
            integer(c_int), value :: igate_size
            real(c_double), intent(in) :: thr(*)
        end function
        integer(c_int) function tlab_gate_flux(a, v, n, gate) bind(C, name='tlab_gate_flux')
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: a, v, gate
            integer(c_long_long), value :: n
        end function
        integer(c_int) function tlab_dns_gate(dns, opt_cond, opt_cond_relative, opt_cond_scal, igate_size, gate_threshold, q, s, txc, gate) &
            bind(C, name='tlab_dns_gate')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: dns, gate
            integer(c_int), value :: opt_cond, opt_cond_relative, opt_cond_scal, igate_size
            real(c_double), intent(in) :: gate_threshold(*)
            type(c_ptr), intent(in) :: q(*), s(*), txc(*)
        end function
        integer(c_int) function tlab_avg_n_xz(nx, ny, nz, nv, nm, u, np, gate, avg, sums, nsample) bind(C, name='tlab_avg_n_xz')
            import :: c_int, c_ptr
            integer(c_int), value :: nx, ny, nz, nv, nm, np
            type(c_ptr), intent(in) :: u(*)
            type(c_ptr), value :: gate, avg, sums, nsample
        end function
        integer(c_int) function tlab_raw_to_central(nm, moments) bind(C, name='tlab_raw_to_central')
            import :: c_int, c_double
            integer(c_int), value :: nm
            real(c_double), intent(inout) :: moments(*)
        end function
        integer(c_int) function tlab_cavg1v_n(nx, ny, nz, nv, nbins, ibc, umin, umax, u, igate, gate, a, avg, sum, pdf) bind(C, name='tlab_cavg1v_n')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz, nv, nbins, igate
            integer(c_int), intent(in) :: ibc(*)
            real(c_double), intent(in) :: umin(*), umax(*)
            type(c_ptr), intent(in) :: u(*)
            type(c_ptr), value :: gate, a, sum, pdf
            real(c_double), intent(out) :: avg(*)
        end function
        integer(c_int) function tlab_cavg2v(nx, ny, nz, nbins, u, v, a, avg) bind(C, name='tlab_cavg2v')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz
            integer(c_int), intent(in) :: nbins(2)
            type(c_ptr), value :: u, v, a
            real(c_double), intent(out) :: avg(*)
        end function
        ! field mappings (declared in tlab_amd/csrc/tlab_amd_mappings.h; wrappers in tlab_amd_mappings.f90): the maps TLAB_MAP_* of the nine velocity
        ! gradients (and the scalar gradient) in one pass, the derivatives that feed it on the driver's plans, and the diffusion / pressure terms
        ! TLAB_FI_* composed from OPR_Partial.  du9, ds3, maps, out, q, txc9, work6: host arrays (of addresses); ds3 may be c_null_ptr
        integer(c_int) function tlab_gradient_maps(n, du9, ds3, maps, nmaps, out) bind(C, name='tlab_gradient_maps')
            import :: c_int, c_ptr, c_long_long
            integer(c_long_long), value :: n
            type(c_ptr), intent(in) :: du9(9), out(*)
            type(c_ptr), value :: ds3
            integer(c_int), intent(in) :: maps(*)
            integer(c_int), value :: nmaps
        end function
        integer(c_int) function tlab_dns_velocity_gradients(dns, q, txc9) bind(C, name='tlab_dns_velocity_gradients')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns
            type(c_ptr), intent(in) :: q(3), txc9(9)
        end function
        integer(c_int) function tlab_dns_scalar_gradient(dns, s, ds3) bind(C, name='tlab_dns_scalar_gradient')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns, s
            type(c_ptr), intent(in) :: ds3(3)
        end function
        integer(c_int) function tlab_dns_fi_maps(dns, q, s, maps, nmaps, txc9, ds3, out) bind(C, name='tlab_dns_fi_maps')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns, s, ds3
            type(c_ptr), intent(in) :: q(3), txc9(9), out(*)
            integer(c_int), intent(in) :: maps(*)
            integer(c_int), value :: nmaps
        end function
        integer(c_int) function tlab_dns_fi_diffusion(dns, kind, q, f, result, work6) bind(C, name='tlab_dns_fi_diffusion')
            import :: c_int, c_ptr
            type(c_ptr), value :: dns, q, f, result
            integer(c_int), value :: kind
            type(c_ptr), intent(in) :: work6(6)
        end function
        ! plane spectra and correlations (tlab_amd_spectra.f90); a_hat .. outr: device or host arrays of one kind, the profiles host memory
        integer(c_int) function tlab_spectrum_reduce(nx, ny, nz, nblock, kr_total, a_hat, b_hat, out2d, outx, outz, outr, variance) &
            bind(C, name='tlab_spectrum_reduce')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz, nblock, kr_total
            type(c_ptr), value :: a_hat, b_hat, out2d, outx, outz, outr
            real(c_double), intent(out) :: variance(*)
        end function
        integer(c_int) function tlab_correlation_reduce(nx, ny, nz, nblock, nr_total, in, var1, var2, out2d, outx, outz, outr, variance2, &
                                                        icalc_radial) bind(C, name='tlab_correlation_reduce')
            import :: c_int, c_ptr, c_double
            integer(c_int), value :: nx, ny, nz, nblock, nr_total, icalc_radial
            type(c_ptr), value :: in, out2d, outx, outz, outr
            real(c_double), intent(in) :: var1(*), var2(*)
            real(c_double), intent(out) :: variance2(*)
        end function
        integer(c_int) function tlab_radial_samplesize(nx, nz, nr_total, samplesize) bind(C, name='tlab_radial_samplesize')
            import :: c_int, c_double
            integer(c_int), value :: nx, nz, nr_total
            real(c_double), intent(out) :: samplesize(*)
        end function
        integer(c_int) function tlab_spectra_pair(plan, mode, nblock, kr_total, a, b, tmp1, tmp2, tmp3, out2d, outx, outz, outr, cov, variance) &
            bind(C, name='tlab_spectra_pair')
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: plan, a, b, tmp1, tmp2, tmp3, out2d, outx, outz, outr
            integer(c_int), value :: mode, nblock, kr_total
            real(c_double), intent(out) :: cov(*), variance(*)
        end function
        integer(c_int) function tlab_boundary_bcs_neumann_y(plan, ibc, nx, ny, nz, u, bcs_hb, bcs_ht, tmp1) bind(C, name='tlab_boundary_bcs_neumann_y')
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, u, bcs_hb, bcs_ht, tmp1
            integer(c_int), value :: ibc, nx, ny, nz
        end function
    end interface

contains
    ! Error convention of the reference: a line in tlab.err and TLab_Stop (base/tlab_workflow.f90:105-207); codes from include/dns_error.h.
    subroutine TLab_AMD_Check(rc, what)
        use TLab_Constants, only: efile
        use TLab_WorkFlow, only: TLab_Write_ASCII, TLab_Stop
        integer(c_int), intent(in) :: rc
        character(len=*), intent(in) :: what
        character(kind=c_char), pointer :: msg(:)
        character(len=512) :: text
        integer i
        integer, parameter :: DNS_ERROR_UNDEVELOP = 104          ! include/dns_error.h:99
        if (rc == 0) return
        call c_f_pointer(tlab_last_error(), msg, [512])
        text = ''
        do i = 1, 512
            if (msg(i) == c_null_char) exit
            text(i:i) = msg(i)
        end do
        call TLab_Write_ASCII(efile, 'tlab_amd. '//what//' failed: '//trim(text))
        write (*, '(a)') 'tlab_amd: '//what//' failed: '//trim(text)
        call TLab_Stop(DNS_ERROR_UNDEVELOP)
    end subroutine TLab_AMD_Check

end module TLab_AMD_C
