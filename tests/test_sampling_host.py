"""Phase averages, towers and saved planes without a GPU: the host branch of the entry points (tlab_init is never called here: every array is host
memory) against the numpy restatement tests/sampling_oracle.py bit for bit, the refusals, the exported symbols and the Fortran module."""
import ctypes
import os
import re

import numpy as np
import pytest

import sampling_cases as C
import sampling_oracle as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
put = lambda a: np.array(a, dtype=np.float64)       # noqa: E731  (a copy: the cases change their accumulators in place)
get = lambda a: a                                    # noqa: E731
ptr = lambda a: a.ctypes.data                        # noqa: E731

SYMBOLS = ["tlab_avg_phase_space", "tlab_avg_phase_flow", "tlab_avg_phase_plane_id", "tlab_tower_create", "tlab_tower_destroy", "tlab_tower_sizes",
           "tlab_tower_accumulate", "tlab_tower_reset", "tlab_planes_gather", "tlab_fi_gradient", "tlab_log10_small", "tlab_dns_arm_pressure_sampling"]


@pytest.fixture(scope="module")
def T():
    import tlab_amd.operators as T
    return T


@pytest.fixture(scope="module")
def L():
    import tlab_amd
    return tlab_amd.load()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_constant_field_averages_to_its_constant_times_the_share_of_the_box():
    u = np.full((8, 3, 4), 0.75)
    avg = np.zeros((1, 3, 3, 4))
    S.avg_phase_space([u], 16, 2, 1, avg)               # nz = 8 of nz_total = 16: half of the average
    assert np.all(avg[0, 0] == 0.375) and np.all(avg[0, 1] == 0.0) and np.all(avg[0, 2] == 0.1875)
    S.avg_phase_space([u], 16, 2, 2, avg)
    assert np.all(avg[0, 2] == 0.375)


def test_oracle_tower_counts():
    t = S.Tower(16, 12, 8, (4, 1, 2), 3)
    assert (list(t.ipos), list(t.kpos), t.jmax) == ([1, 5, 9, 13], [1, 3, 5, 7], 12)
    assert t.bufsize == 5 * 3 * 12 * 16 + 5 * 3 * 12 + 6


# ---- the host branch of the entry points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", C.PHASE_BOXES)
def test_phase_averages_equal_the_restatement_bit_for_bit(T, shape):
    C.check_phase(T, shape, put, get)


def test_plane_id_and_the_refusals(T, L):
    for itr, first, save in ((1, 0, 4), (4, 0, 4), (5, 0, 4), (9, 3, 5), (3, 5, 4), (1, 7, 3), (12, 0, 0), (2, 9, 1)):      # (3, 5, 4), (1, 7, 3): a negative mod
        assert T.avg_phase_plane_id(itr, first, save) == S.avg_phase_plane_id(itr, first, save), (itr, first, save)
    assert T.avg_phase_plane_id(3, 5, 4) == -2 and T.avg_phase_plane_id(12, 0, 0) == 1
    C.check_phase_refusals(L, put, get, ptr)


@pytest.mark.parametrize("shape,stride", C.TOWER_CASES)
@pytest.mark.parametrize("exact", [True, False])
def test_towers_equal_the_restatement(T, shape, stride, exact):
    C.check_towers(T, shape, stride, put, get, exact)


def test_tower_refusals(T, L):
    C.check_tower_refusals(T, L, put, get)


@pytest.mark.parametrize("shape", [(20, 12, 8), (7, 5, 3), (6, 4, 1)])
def test_planes_in_the_three_directions(T, L, shape):
    C.check_planes(T, L, shape, put, get, ptr)


def test_log10_small_on_the_host(T):
    a = np.array([0.0, 1.0, 1e-20, 3.5e7])
    assert np.array_equal(T.log10_small(a.copy()), np.log10(a + 1.0e-20))


def test_mixed_arrays_and_missing_drivers_are_refused(L):
    assert L.tlab_fi_gradient(None, None, None, None) != 0                       # no tlab_init, no driver
    assert L.tlab_dns_arm_pressure_sampling(None, None, None, 1, 0.0, None, 1, 1) != 0
    assert L.tlab_tower_accumulate(None, 4, None, 1, 0.0, None) == C.EINVAL
    assert L.tlab_log10_small(0, None) == C.EINVAL


# ---- symbols, Fortran module ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_fortran_module_names_them():
    import tlab_amd
    lib = ctypes.CDLL(tlab_amd.lib_path())
    assert not [n for n in SYMBOLS if not hasattr(lib, n)]
    src = open(os.path.join(ROOT, "tlab_amd", "fortran", "tlab_amd_sampling.f90")).read()
    for proc in ("TLab_AMD_AvgPhaseSpace", "TLab_AMD_AvgPhaseStress", "TLab_AMD_Tower_Accumulate", "TLab_AMD_Planes_Gather",
                 "TLab_AMD_Arm_Pressure_Sampling"):
        assert re.search(r"subroutine\s+%s\b" % proc, src, flags=re.I), proc
    for n in ("tlab_avg_phase_space", "tlab_avg_phase_flow", "tlab_tower_accumulate", "tlab_planes_gather", "tlab_dns_arm_pressure_sampling"):
        assert "name='%s'" % n in src or 'name="%s"' % n in src, n
    assert max(len(l) for l in src.splitlines()) <= 160
    assert "tlab_amd_sampling" in open(os.path.join(ROOT, "tlab_amd", "fortran", "Makefile")).read()
