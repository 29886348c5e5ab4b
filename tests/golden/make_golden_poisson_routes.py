#!/usr/bin/env python3
"""y-plan tables of the direct scheme on 33 UNIFORM nodes, made by the reference's FDM_CreatePlan through oracle/_ref with (mode1, mode2) =
(CompactJacobian6, CompactDirect6): the direct plan of the marching shape of tests/test_gpu_poisson.py::test_transform_routes_vs_oracle (the
other fixtures of the direct scheme sit on tanh-stretched nodes).  Same layout as poisson_direct_modes_c4_40.npz: tab_<key>, y, mode2.

    make -C oracle && python3 tests/golden/make_golden_poisson_routes.py"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import ref_lib as R  # noqa: E402

KEYS = ("ndl1", "ndr1", "ndl2", "ndr2", "need_1der", "lhs1", "rhs1", "lu1", "rhs_b1", "rhs_t1", "mwn1", "lhs2", "rhs2", "lu2", "mwn2", "jac")

if __name__ == "__main__":
    if not R.available():
        sys.exit("oracle/_ref/libtlab_ref.so missing")
    n = 33
    y = np.arange(n) / (n - 1.0) * 2.0
    R.init(4, n, 4)
    R.fdm_create(2, y, False, False, 6, 16)
    tab = R.fdm_arrays(2, n)
    out = {"tab_" + k: np.asarray(tab[k]) for k in KEYS}
    out["y"] = y
    out["mode2"] = 16
    np.savez_compressed(os.path.join(HERE, "poisson_routes_y33.npz"), **out)
    print("wrote poisson_routes_y33")
