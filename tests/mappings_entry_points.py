"""How every entry point of tlab_amd/csrc/tlab_amd_mappings.h relates to a pending record of the deferred tail (csrc/deferred.cpp), in the
classes of tests/deferred_entry_points.py, which is the table of include/tlab_amd.h and is not this header's.  A plain module: neither a conftest
nor a test.  tests/test_mappings_symbols.py holds it against the header and against the cases of tests/test_gpu_mappings.py.

  stream  enqueues work on the caller's device arrays or on a driver's arrays: it must see a pending record already executed.  EVERY one has a
          case in test_a_pending_record_runs_first (tests/test_gpu_mappings.py): this table has no list of entries that are not exercised
  host    no device work on a caller's or driver's array, and no state that a replay reads (none here)
"""
from deferred_entry_points import STREAM

ENTRY_POINTS = {
    "tlab_gradient_maps": STREAM,
    "tlab_dns_velocity_gradients": STREAM,
    "tlab_dns_scalar_gradient": STREAM,
    "tlab_dns_fi_maps": STREAM,
    "tlab_dns_fi_diffusion": STREAM,
}
PENDING_TEST = "test_a_pending_record_runs_first"      # in tests/test_gpu_mappings.py
