"""How every entry point of tlab_amd/csrc/tlab_amd_conditional.h relates to a pending record of the deferred tail (csrc/deferred.cpp), in the
classes of tests/deferred_entry_points.py, which is the table of include/tlab_amd.h and is not this header's.  A plain module: neither a conftest
nor a test.  tests/test_conditional_symbols.py holds it against the header and against the cases of tests/test_gpu_conditional.py.

  stream  enqueues work on the caller's device arrays or on a driver's arrays: it must see a pending record already executed.  EVERY one has a
          case in test_a_pending_record_runs_first (tests/test_gpu_conditional.py): this table has no list of entries that are not exercised
  host    no device work on a caller's or driver's array, and no state that a replay reads
"""
from deferred_entry_points import HOST, STREAM

ENTRY_POINTS = {
    "tlab_gate_levels": STREAM,
    "tlab_gate_flux": STREAM,
    "tlab_dns_gate": STREAM,
    "tlab_avg_n_xz": STREAM,
    "tlab_raw_to_central": HOST,                     # host arithmetic on nm numbers
    "tlab_cavg1v_n": STREAM,
    "tlab_cavg2v": STREAM,
}
PENDING_TEST = "test_a_pending_record_runs_first"      # in tests/test_gpu_conditional.py
