#!/usr/bin/env python3
"""The reference library's first / second derivatives on the seeded 1-D lines of tests/test_oracle_derivs.py::test_oracle_vs_reference_library_1d,
and its TLab_Transpose of the seeded array of test_transpose_bit_exact_vs_reference (oracle/_ref).  Run where oracle/_ref is built:
    python3 tests/golden/make_golden_ref1d.py  ->  tests/golden/ref_lib_1d.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
from oracle import ref_lib as R  # noqa: E402
from test_oracle_derivs import REF_1D, REF_1D_CASES, ref_1d_outputs, ref_transpose_input  # noqa: E402

if __name__ == "__main__":
    if not R.available():
        sys.exit("oracle/_ref/libtlab_ref.so missing")
    out = {}
    for n, periodic, stretch in REF_1D_CASES:
        for k, v in ref_1d_outputs(n, periodic, stretch).items():
            out["n%d_p%d_s%d_%s" % (n, periodic, stretch, k)] = v
    out["transpose"] = R.transpose(ref_transpose_input())
    np.savez_compressed(REF_1D, **out)
    print(REF_1D, len(out), "arrays")
