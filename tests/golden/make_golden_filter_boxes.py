#!/usr/bin/env python3
"""Second fixture for the 1-D filters (OPR_FILTER_1D, operators/opr_filter.f90:393-460), made like filters.npz by the reference's own filter
modules through oracle/_ref (make_golden_filters.py; that file and its fixture stay as they are): coefficient tables and filtered random lines
at the line lengths the tests on whole boxes need (tests/test_gpu_filter_boxes.py) --

    8    the smallest size tlab_filter_create accepts: the interior loops run for one to three rows, the end stencils overlap
    37   odd and prime: no multiple of a transpose tile or a wave
    130  a little over 128: more than one transpose tile per line, plus a remainder

for the types compact (1), explicit6 (2), explicit4 (3), compactcutoff (9), periodic and non-periodic with the end conditions of filters.npz.

    make -C oracle && python3 tests/golden/make_golden_filter_boxes.py"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import ref_lib as R  # noqa: E402
from oracle import tlab_oracle as O  # noqa: E402

LENGTHS = (8, 37, 130)

if __name__ == "__main__":
    if not R.available():
        sys.exit("oracle/_ref/libtlab_ref.so missing")
    out = {}
    rng = np.random.default_rng(20261020)
    R.init(max(LENGTHS), max(LENGTHS), 8)
    cases = []
    for n in LENGTHS:
        y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(n) / (n - 1) - 1)) / np.tanh(1.5))
        x = np.arange(n) / n * 2.0
        jy, jx = O.FdmPlan(y, False, False).jac[:, 0], O.FdmPlan(x, True, True).jac[:, 0]
        out["n%d_y" % n], out["n%d_x" % n], out["n%d_jy" % n], out["n%d_jx" % n] = y, x, jy, jx
        u = rng.uniform(-1, 1, (n, 6))
        out["n%d_u" % n] = u
        for t in (1, 2, 3, 9):
            for per, nodes, jac, bcs in ((True, x, jx, [(0, 0)]), (False, y, jy, [(1, 1), (2, 6), (6, 2), (6, 6)])):
                for b0, b1 in bcs:
                    key = "n%d_t%d_p%d_b%d%d" % (n, t, int(per), b0, b1)
                    c = R.filter_init(t, nodes, jac, per, b0, b1)
                    out[key + "_coeffs"] = c
                    out[key + "_res"] = R.filter_1d(t, per, b0, b1, c, u)
                    cases.append(key)
    out["cases"] = np.array(cases)
    np.savez_compressed(os.path.join(HERE, "filter_boxes.npz"), **out)
    print("wrote filter_boxes.npz", len(cases), "cases")
