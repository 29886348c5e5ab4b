"""The line algorithms of the streaming filter kernels (tlab_amd/csrc/filter_lines.hpp) compiled for the host and run on single lines: every case
of both filter fixtures against oracle.tlab_oracle_filter.opr_filter_1d, word for word.  No GPU: tests/filter_lines_host.cpp gives filter_line a
serial sweep with a tile of 5 points -- shorter than any line, no divisor of a line length, so every sweep ends in a partial tile and the values
that lag behind the tile cross tile ends -- and stores the tile shifted by the lag exactly as the kernel's stage does.  What this cannot see is the
addressing of the device stage (tests/test_gpu_filter_stream.py).

Bound: equality of every 64-bit word.  The expression trees are k_filter1d's, FP contraction is off (-ffp-contract=off), and the oracle equals
the reference's filter modules bit for bit at these line lengths (tests/test_oracle_filter.py)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from test_oracle_filter import G, GB, filter_of, fixture_of

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEYS = [str(k) for k in G["cases"]] + [str(k) for k in GB["cases"]]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = next((c for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler on this machine"
    so = str(tmp_path_factory.mktemp("filter_lines") / "libfilter_lines_host.so")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                    "-I" + os.path.join(ROOT, "tlab_amd", "csrc"), os.path.join(ROOT, "tests", "filter_lines_host.cpp"), "-o", so], check=True)
    L = ctypes.CDLL(so)
    dp = ctypes.POINTER(ctypes.c_double)
    L.host_filter.argtypes = [ctypes.c_int] * 5 + [dp, dp]
    L.host_filter.restype = None
    return L


@pytest.mark.parametrize("key", KEYS)
def test_line_algorithms_vs_oracle(host, key):
    from oracle import tlab_oracle_filter as F
    dp = ctypes.POINTER(ctypes.c_double)
    n, t, per, b0, b1 = (int(v) for v in re.match(r"n(\d+)_t(\d+)_p(\d)_b(\d)(\d)", key).groups())
    c = np.asfortranarray(fixture_of(key)[key + "_coeffs"], dtype=np.float64)
    lines = np.random.default_rng([n, t, per, b0, b1]).uniform(-1, 1, (3, n))
    want = np.ascontiguousarray(F.opr_filter_1d(filter_of(key)[0], np.ascontiguousarray(lines.T)).T)      # the oracle takes (n, nlines)
    got = lines.copy()
    for line in got:
        host.host_filter(t, per, n, 0 if per else b0, 0 if per else b1, c.ctypes.data_as(dp) if c.size else None, line.ctypes.data_as(dp))
    bad = int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))
    assert bad == 0, (key, "%d of %d words differ from the oracle" % (bad, got.size))
