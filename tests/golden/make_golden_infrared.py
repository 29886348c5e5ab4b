#!/usr/bin/env python3
"""Golden vectors of the optical depth of IR_RTE1_OnlyLiquid (physics/radiation.f90:416-417): FDM_Int1_Solve on fdm_Int0(BCS_MAX), i.e.
FDM_Int1_Initialize(lambda = 0, BCS_MAX) of the y plan (fdm/fdm_integral.f90:58-87, :219-314), from the reference itself (oracle/_ref) for a
handful of lines of a smooth non-negative absorption on a uniform and a stretched 33-point grid.  THERMO_AIRWATER_LINEAR and the exp / product
lines of the radiation routine are not reachable through oracle/ref_lib.py.
Run in the build container:  python3 tests/golden/make_golden_infrared.py  ->  tests/golden/infrared_tau.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from oracle import ref_lib as R  # noqa: E402

BCS_MAX = 2


def nodes(n, stretch):
    return 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(n) / (n - 1) - 1)) / np.tanh(1.5)) if stretch else np.arange(n) / (n - 1.0)


def absorption(y, nlines):
    """kappa l of a cloud layer: smooth, non-negative, zero below and above the layer in some lines; (n, nlines)"""
    Y = ((y - y[0]) / (y[-1] - y[0]))[:, None]
    k = np.arange(nlines)[None, :]
    return np.maximum(0.0, (3.0 + 0.5 * k) * np.sin((1.0 + 0.15 * k) * np.pi * Y) * (1.0 + 0.3 * np.cos(0.9 * k)) - 0.2 * k)


if __name__ == "__main__":
    if not R.available():
        sys.exit("oracle/_ref/libtlab_ref.so missing")
    n, nlines = 33, 6
    out = {"n": n, "nlines": nlines}
    for name, stretch in (("uniform", False), ("stretched", True)):
        y = nodes(n, stretch)
        R.init(4, n, 4)
        R.fdm_create(2, y, False, not stretch)
        R.int1_create(0.0, BCS_MAX)
        a = absorption(y, nlines)
        tau, _ = R.int1_solve(BCS_MAX, a, np.zeros_like(a))           # p_tau(:, ny) = 0
        out[name + "_y"], out[name + "_a"], out[name + "_tau"] = y, a, tau
    np.savez_compressed(os.path.join(HERE, "infrared_tau.npz"), **out)
    print("wrote infrared_tau.npz")
