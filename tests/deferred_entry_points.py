"""How every entry point of include/tlab_amd.h relates to a pending record of the deferred tail (csrc/deferred.cpp).  A plain module: neither a
conftest nor a test.  tests/test_deferred_entry_points_host.py holds it against the header (a new symbol without a row fails there) and against
the cases of tests/test_gpu_deferred_entry_points.py.

  stream      enqueues work on the caller's device arrays or on a driver's arrays: it must see a pending record already executed
  setter      changes state that a replayed substep reads: the pending substep must run with the OLD state
  deferred    the layer's own tlab_deferred_* functions
  lifetime    init, finalize, malloc, free, the stream itself, *_create and *_destroy: checked by reading only -- a destroy flushes first (a miss
              would leave a dangling record, and a use-after-free is nothing to run on a shared machine), a create has nothing to do with a record
  host        no device work on a caller's or driver's array, and no state that a replay reads
  decomposed  needs a slab or pencil handle: only classified here, test_decomposed_replay_* (tests/test_gpu_deferred.py) is their test
"""
STREAM, SETTER, DEFERRED, LIFETIME, HOST, DECOMPOSED = "stream", "setter", "deferred", "lifetime", "host", "decomposed"

ENTRY_POINTS = {
    # ---- runtime (csrc/runtime.cpp)
    "tlab_init": LIFETIME,
    "tlab_device_count": HOST,
    "tlab_finalize": LIFETIME,                       # tlab_deferred_enable(0) first: runs what is recorded
    "tlab_last_error": HOST,
    "tlab_set_stream": LIFETIME,                     # flushes on the OLD stream, then switches (by reading; no GPU case may name it)
    "tlab_sync": STREAM,
    "tlab_malloc": LIFETIME,
    "tlab_free": LIFETIME,                           # flushes first
    "tlab_memcpy_h2d": STREAM,
    "tlab_memcpy_d2h": STREAM,
    # ---- plans
    "tlab_fdm_plan_create": LIFETIME,
    "tlab_fdm_plan_create_from_arrays": LIFETIME,
    "tlab_fdm_plan_set_aux": HOST,                   # mwn, jac, nodes: copied by tlab_poisson_plan_create / tlab_dns_create / tlab_dns_set_particles, never read by a substep
    "tlab_fdm_plan_set_scheme": SETTER,              # der%direct and the cached systems are what every derivative launch of a substep reads
    "tlab_fdm_plan_set_stagger": SETTER,             # destroys and rebuilds the interpolation filters a staggered driver's substep launches
    "tlab_fdm_plan_destroy": LIFETIME,               # flushes first
    "tlab_fdm_plan_get": HOST,
    "tlab_fdm_plan_info": HOST,
    # ---- operators
    "tlab_opr_partial": STREAM,
    "tlab_opr_burgers": STREAM,
    "tlab_opr_burgers_set_anelastic": SETTER,        # the drivers follow this state (rhs.cpp: tlab_internal_anelastic_state)
    "tlab_filter_create": LIFETIME,
    "tlab_filter_destroy": LIFETIME,                 # flushes first
    "tlab_opr_filter_1d": STREAM,
    "tlab_opr_filter": STREAM,
    "tlab_opr_filter_fields": STREAM,
    "tlab_opr_burgers_set_dealiasing": SETTER,       # tlab_internal_dealiasing() sends a substep down the unfused Burgers sequence, which filters with it
    "tlab_poisson_plan_create": LIFETIME,
    "tlab_poisson_plan_destroy": LIFETIME,           # flushes first
    "tlab_opr_poisson": STREAM,
    "tlab_poisson_set_exact": HOST,                  # read by the plans created AFTER the call only
    "tlab_poisson_plan_create_direct": LIFETIME,
    "tlab_opr_helmholtz": STREAM,
    "tlab_poisson_plan_create_direct_decomposed": LIFETIME,
    "tlab_poisson_direct_ode": STREAM,
    "tlab_poisson_plan_create_slab": LIFETIME,
    "tlab_poisson_plan_create_pencil": LIFETIME,
    "tlab_pencil_repack": STREAM,
    "tlab_pencil_repack_blocks": STREAM,
    "tlab_poisson_set_wall_planes": STREAM,
    "tlab_poisson_fft_x": STREAM,
    "tlab_poisson_fft_x_packed": STREAM,
    "tlab_poisson_fft_x_packed_final": STREAM,
    "tlab_poisson_fft_z": STREAM,
    "tlab_poisson_ode": STREAM,
    "tlab_opr_burgers_add": STREAM,
    "tlab_opr_partial_add": STREAM,
    "tlab_opr_gradient_final": STREAM,
    "tlab_opr_burgers_add_n": STREAM,
    "tlab_zslab_plan_create": LIFETIME,
    "tlab_zslab_plan_destroy": LIFETIME,             # flushes first
    "tlab_zslab_partial_z": STREAM,
    "tlab_zslab_burgers_z": STREAM,
    "tlab_zslab_burgers_z_n": STREAM,
    "tlab_zslab_gradient_final_z": STREAM,
    # ---- the single-domain driver
    "tlab_dns_create": LIFETIME,
    "tlab_dns_destroy": LIFETIME,                    # flushes first
    "tlab_dns_set_fusion": SETTER,
    "tlab_dns_set_scalar_bounds": SETTER,
    "tlab_dns_set_buffer_type": SETTER,
    "tlab_dns_set_buffer_zone": SETTER,
    "tlab_buffer_tau": HOST,
    "tlab_dns_buffer_relax_flow": STREAM,
    "tlab_dns_buffer_relax_scal": STREAM,
    "tlab_dns_set_coriolis": SETTER,
    "tlab_dns_set_buoyancy": SETTER,
    "tlab_dns_sources_flow": STREAM,
    "tlab_dns_pressure": STREAM,
    "tlab_dns_set_mixture": SETTER,
    "tlab_dns_diagnostic": STREAM,
    "tlab_dns_set_infrared": SETTER,
    "tlab_dns_sources_scal": STREAM,
    "tlab_dns_info": HOST,
    "tlab_dns_set_particles": SETTER,
    "tlab_dns_particle_locate": STREAM,
    "tlab_dns_substep_particle": STREAM,
    "tlab_dns_particle_sort": STREAM,
    "tlab_dns_field_to_particle": STREAM,
    "tlab_dns_set_trajectories": SETTER,
    "tlab_dns_trajectories_accumulate": STREAM,
    "tlab_dns_particle_to_field": STREAM,
    "tlab_dns_begin_step": SETTER,                   # the one-shot flag the next RHS of the driver reads
    "tlab_dns_place_arrays": STREAM,
    "tlab_dns_place_blocks": STREAM,
    "tlab_dns_set_bcs": SETTER,
    "tlab_dns_set_pressure_filter": SETTER,
    "tlab_dns_set_filter": SETTER,
    "tlab_dns_filter": STREAM,
    "tlab_dns_set_remove_divergence": SETTER,
    "tlab_dns_set_surface_bcs": SETTER,
    "tlab_dns_set_anelastic": SETTER,
    "tlab_dns_set_slab": SETTER,
    "tlab_dns_arm_pressure_sampling": SETTER,        # one-shot like tlab_dns_begin_step: the next RHS of the driver takes the samples
    "tlab_rhs_global_incompressible_1": STREAM,
    "tlab_time_substep_incompressible_explicit": STREAM,
    "tlab_boundary_bcs_neumann_y": STREAM,
    # ---- the deferred tail itself
    "tlab_deferred_enable": DEFERRED,
    "tlab_deferred_rhs": DEFERRED,
    "tlab_deferred_axpy": DEFERRED,
    "tlab_deferred_scal": DEFERRED,
    "tlab_deferred_zero": DEFERRED,
    "tlab_deferred_flush": DEFERRED,
    "tlab_deferred_clip": DEFERRED,
    "tlab_deferred_relax_scal": DEFERRED,
    "tlab_deferred_relax_stats": DEFERRED,
    "tlab_deferred_sources_flow": DEFERRED,
    "tlab_deferred_sources_stats": DEFERRED,
    "tlab_deferred_stats": DEFERRED,
    "tlab_deferred_clip_stats": DEFERRED,
    "tlab_deferred_slab_rhs": DEFERRED,
    "tlab_deferred_pencil_rhs": DEFERRED,
    "tlab_pointer_on_device": HOST,
    # ---- monitors
    "tlab_time_courant": STREAM,
    "tlab_fi_invariant_p": STREAM,
    "tlab_minmax": STREAM,
    "tlab_fi_vorticity": STREAM,
    "tlab_vorticity_from_gradients": STREAM,
    "tlab_dns_dilatation_extremes": STREAM,
    "tlab_device_minmax": STREAM,
    "tlab_minmax_any": STREAM,
    # ---- plane statistics, PDFs, spectra
    "tlab_avg_ik_v": STREAM,
    "tlab_avg1v2d_v": STREAM,
    "tlab_avg_moments_flow": STREAM,
    "tlab_avg_moments_scal": STREAM,
    "tlab_avg_gradients_flow": STREAM,
    "tlab_avg_ugradp": STREAM,
    "tlab_avg_gradients_scal": STREAM,
    "tlab_avg_gradients_pass": STREAM,
    "tlab_dns_avg_gradients_flow": STREAM,
    "tlab_dns_avg_gradients_scal": STREAM,
    "tlab_inter_n_xz": STREAM,
    "tlab_spectrum_reduce": STREAM,
    "tlab_correlation_reduce": STREAM,
    "tlab_radial_samplesize": HOST,
    "tlab_cross_product": STREAM,
    "tlab_fluctuation": STREAM,
    "tlab_avg_cov2v": STREAM,
    "tlab_spectra_pair": STREAM,
    "tlab_dns_spectra": STREAM,
    "tlab_pdf1v_n": STREAM,
    "tlab_pdf_minmax_planes": STREAM,
    "tlab_pdf_histogram_planes": STREAM,
    "tlab_pdf_analize": HOST,
    "tlab_pdf2v": STREAM,
    "tlab_gate_threshold": STREAM,
    # ---- the decomposed drivers
    "tlab_slab_transport_loopback": LIFETIME,        # makes a transport: no launch, no handle of a driver
    "tlab_pencil_transport_loopback": LIFETIME,
    "tlab_pencil_dns_create": LIFETIME,
    "tlab_pencil_dns_destroy": LIFETIME,             # flushes first
    "tlab_pencil_dns_bind": DECOMPOSED,
    "tlab_pencil_dns_info": DECOMPOSED,
    "tlab_pencil_dns_set_bcs": DECOMPOSED,
    "tlab_pencil_dns_set_buffer_zone": DECOMPOSED,
    "tlab_pencil_dns_set_coriolis": DECOMPOSED,
    "tlab_pencil_dns_set_buoyancy": DECOMPOSED,
    "tlab_pencil_dns_set_scalar_bounds": DECOMPOSED,
    "tlab_pencil_dns_begin_step": DECOMPOSED,
    "tlab_pencil_dns_rhs": DECOMPOSED,
    "tlab_pencil_dns_trace": DECOMPOSED,
    "tlab_pencil_dns_substep": DECOMPOSED,
    "tlab_pencil_dns_time_courant": DECOMPOSED,
    "tlab_pencil_dns_courant_local": DECOMPOSED,
    "tlab_pencil_dns_dilatation_bounds": DECOMPOSED,
    "tlab_pencil_dns_dilatation_extremes": DECOMPOSED,
    "tlab_slab_dns_create": LIFETIME,
    "tlab_slab_dns_destroy": LIFETIME,               # flushes first
    "tlab_slab_dns_bind": DECOMPOSED,
    "tlab_slab_dns_info": DECOMPOSED,
    "tlab_slab_dns_set_bcs": DECOMPOSED,
    "tlab_slab_dns_begin_step": DECOMPOSED,
    "tlab_slab_dns_set_remove_divergence": DECOMPOSED,
    "tlab_slab_dns_set_buffer_zone": DECOMPOSED,
    "tlab_slab_dns_set_coriolis": DECOMPOSED,
    "tlab_slab_dns_set_buoyancy": DECOMPOSED,
    "tlab_slab_dns_set_scalar_bounds": DECOMPOSED,
    "tlab_slab_dns_set_surface_bcs": DECOMPOSED,
    "tlab_slab_dns_rhs": DECOMPOSED,
    "tlab_slab_dns_substep": DECOMPOSED,
    "tlab_slab_dns_time_courant": DECOMPOSED,
    "tlab_slab_dns_dilatation_bounds": DECOMPOSED,
    "tlab_slab_dns_dilatation_extremes": DECOMPOSED,
    "tlab_slab_dns_courant_local": DECOMPOSED,
    # ---- the pointwise loops
    "tlab_pw_add3": STREAM,
    "tlab_pw_axpy3": STREAM,
    "tlab_pw_sum3": STREAM,
    "tlab_pw_sub3": STREAM,
    "tlab_pw_rk_update": STREAM,
    "tlab_pw_fill": STREAM,
    "tlab_pw_clip": STREAM,
    "tlab_pw_scale": STREAM,
    "tlab_pw_final_update": STREAM,
    "tlab_pw_get_wall_planes": STREAM,
    "tlab_pw_fill_wall_planes": STREAM,
    "tlab_pw_set_wall_planes": STREAM,
    # ---- sampling
    "tlab_avg_phase_space": STREAM,
    "tlab_avg_phase_flow": STREAM,
    "tlab_avg_phase_plane_id": HOST,
    "tlab_tower_create": LIFETIME,
    "tlab_tower_destroy": LIFETIME,                  # flushes first (a recorded RHS armed with the tower samples into it)
    "tlab_tower_sizes": HOST,                        # flushes first all the same: sizes[6], sizes[7] are advanced by a recorded RHS that was armed
    "tlab_tower_positions": HOST,
    "tlab_tower_accumulate": STREAM,
    "tlab_tower_reset": SETTER,                      # tower_accumulation: where an armed pressure sample of a recorded RHS is stored
    "tlab_planes_gather": STREAM,
    "tlab_fi_gradient": STREAM,
    "tlab_log10_small": STREAM,
    # ---- the rest
    "tlab_transpose": STREAM,
    "tlab_last_kernel_path": HOST,
    "tlab_force_kernel_path": SETTER,                # the kernel family every operator launch of a substep is sent to
    "tlab_set_tuning": SETTER,                       # chunk sizes and tile policies of the kernels a substep launches
    "tlab_profile_enable": HOST,
    "tlab_profile_filter": HOST,
    "tlab_profile_reset": HOST,
    "tlab_profile_report": HOST,
    "tlab_debug_host_chunked_solve": HOST,
    "tlab_debug_int1_tables": HOST,
    "tlab_debug_pack_map": HOST,
    "tlab_debug_int1_solve": HOST,                   # host buffers in and out: the device work is on private copies, no array of a caller or a driver
}

# stream and setter entries without a case in tests/test_gpu_deferred_entry_points.py, each with its reason.  A reason opens with the object the
# set-up needs and that file does not otherwise build (OBJECTS), or with "departure:" for the few entries that have no case for another cause
# (DEPARTURES names them: the host test holds the list, so that it cannot grow unseen)
OBJECTS = ("particles", "towers", "spectra rings", "PDF work space", "Poisson plan")
DEPARTURES = ("tlab_dns_place_arrays", "tlab_dns_place_blocks", "tlab_dns_set_slab", "tlab_fdm_plan_set_stagger")
_PARTICLES = "particles: needs a driver with particles (tlab_dns_set_particles) and the particle arrays; flushes through tlab_current_stream() (csrc/particles.hip)"
_SPECTRA = "spectra rings: needs the spectra rings and the radial sample tables of csrc/spectra.cpp; tlab_internal_deferred_flush() is its first statement"
NOT_EXERCISED = {
    "tlab_dns_set_particles": _PARTICLES,
    "tlab_dns_set_trajectories": _PARTICLES,
    "tlab_dns_particle_locate": _PARTICLES,
    "tlab_dns_substep_particle": _PARTICLES,
    "tlab_dns_particle_sort": _PARTICLES,
    "tlab_dns_field_to_particle": _PARTICLES,
    "tlab_dns_trajectories_accumulate": _PARTICLES,
    "tlab_dns_particle_to_field": _PARTICLES,
    "tlab_spectrum_reduce": _SPECTRA,
    "tlab_correlation_reduce": _SPECTRA,
    "tlab_spectra_pair": _SPECTRA,
    "tlab_dns_spectra": _SPECTRA,
    "tlab_poisson_fft_x_packed_final": "Poisson plan: needs the packed spectral buffer of a decomposed Poisson plan as its input; takes the stream through tlab_current_stream()",
    "tlab_poisson_direct_ode": "Poisson plan: needs a direct (CompactDirect6) Poisson plan; takes the stream through tlab_current_stream()",
    "tlab_dns_set_slab": "departure: the only offset a single-domain driver accepts is the 0 it has (koffset + nz <= the z plan's size): no other value to set; read by "
                         "the monitors, not by a substep; tlab_internal_deferred_flush() is its first statement",
    # no deterministic output exists for these two: the pool arrays are undefined afterwards and the answer is a timing.  They run the driver's own
    # substep entry points, whose case is tlab_time_substep_incompressible_explicit
    "tlab_dns_place_arrays": "departure: its outputs are timings and arrays left undefined: nothing a case could compare; every trial goes through the driver's substep, which flushes",
    "tlab_dns_place_blocks": "departure: its outputs are timings and arrays left undefined: nothing a case could compare; every trial goes through the driver's substep, which flushes",
    # the one call that changes a value (mode 0) makes a pending staggered substep FAIL instead of changing its result: no old-against-new to compare
    "tlab_fdm_plan_set_stagger": "departure: no value-changing setting to compare (modes 1, 2 rebuild the same tables, mode 0 makes the substep fail); flushes first, by reading",
}
