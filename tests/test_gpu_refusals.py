"""GPU test: the exact (return code, tlab_last_error() text) of the refusals that sit behind the device check of the operators (check_common,
csrc/operators.cpp) and of the filter entry points that need a filter object, over the raw C ABI.  Every case is an argument check that returns
before a kernel is enqueued, so the boxes are 64 x 1 x 1 (x lines of a periodic plan) and 8 x 40 x 1 (y lines of a stretched wall-bounded plan)
and nothing is computed.  The refusals that need no device are in tests/test_refusals_host.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
P1, P2, P2_P1, P1_INT_VP, P0_INT_PV = 1, 2, 3, 5, 8
IBM_TYPE = 4        # not one of the types above: what the reference has beyond them (the IBM variants) is not built on the device
B_SELF, B_U_IN = 0, 1


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    from tlab_amd import lib as L
    T.init(0)
    lib = L.load()

    class E:
        pass
    e = E()
    e.lib = lib
    e.x64 = T.FdmPlan(np.arange(64) / 64.0, True, True)                                 # periodic, uniform, no stagger tables
    y = np.arange(40) / 39.0
    e.y40 = T.FdmPlan(y + 0.1 * y * (1.0 - y), False, False)                            # non-periodic, stretched: the second derivative needs the first
    e.a, e.b, e.c, e.d = (torch.zeros(8 * 40, dtype=torch.float64, device="cuda") for _ in range(4))
    f = ctypes.c_void_p()
    assert lib.tlab_filter_create(ctypes.byref(f), 2, 64, 1, 0, 0, 0, ctypes.POINTER(ctypes.c_double)()) == 0        # explicit6, 64 points, periodic
    e.f64 = f.value
    yield e
    lib.tlab_filter_destroy(e.f64)


def refused(e, rc, code, text):
    assert rc == code
    assert e.lib.tlab_last_error().decode() == text


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def ptrs(*ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def test_aliased_arrays_are_refused_by_each_operator(env):
    e, l = env, env.lib
    a, b, c = ptr(e.a), ptr(e.b), ptr(e.c)
    g = e.x64._h
    refused(e, l.tlab_opr_partial(1, g, P1, 64, 1, 1, 0, a, a, None), EINVAL, "u, result, tmp1 must be distinct")
    refused(e, l.tlab_opr_partial(1, g, P2_P1, 64, 1, 1, 0, a, b, b), EINVAL, "u, result, tmp1 must be distinct")
    refused(e, l.tlab_opr_burgers(1, g, B_SELF, 64, 1, 1, 0, 1.0, a, None, b, a, 0), EINVAL, "s, result, tmp1 must be distinct")
    refused(e, l.tlab_opr_burgers(1, g, B_U_IN, 64, 1, 1, 0, 1.0, a, b, b, c, 0), EINVAL, "velocity must not alias result / tmp1")
    refused(e, l.tlab_opr_burgers_add(1, g, 64, 1, 1, 0, 1.0, a, b, a, None, None), EINVAL, "tlab_opr_burgers_add: null or aliased arrays")
    nu = (ctypes.c_double * 1)(1.0)
    refused(e, l.tlab_opr_burgers_add_n(1, g, 64, 1, 1, 0, 1, nu, ptrs(e.a), b, ptrs(e.a), None, None, 0), EINVAL,
            "tlab_opr_burgers_add_n: null or aliased arrays")
    refused(e, l.tlab_opr_gradient_final(1, g, 64, 1, 1, a, b, b, 1.0, 1.0, 0, None), EINVAL, "tlab_opr_gradient_final: null or aliased arrays")
    refused(e, l.tlab_opr_partial_add(1, g, 64, 1, 1, 0, a, None, 0.0, a, 0, None, None), EINVAL, "tlab_opr_partial_add: null or aliased arrays")
    refused(e, l.tlab_boundary_bcs_neumann_y(e.y40._h, 1, 8, 40, 1, a, b, c, a), EINVAL, "BOUNDARY_BCS_NEUMANN_Y: null or aliased arrays")
    refused(e, l.tlab_transpose(a, 8, 40, a), EINVAL, "tlab_transpose: bad arguments")


def test_opr_partial_types_and_scratch(env):
    e, l = env, env.lib
    a, b = ptr(e.a), ptr(e.b)
    refused(e, l.tlab_opr_partial(1, e.x64._h, IBM_TYPE, 64, 1, 1, 0, a, b, None), EUNSUPPORTED,
            "OPR_Partial type not built on the device (the IBM variants stay on the CPU path)")
    refused(e, l.tlab_opr_partial(2, e.y40._h, P2, 8, 40, 1, 0, a, b, None), EINVAL, "OPR_P2 on a non-uniform grid needs tmp1 (opr_partial.f90:96)")
    refused(e, l.tlab_opr_partial(2, e.y40._h, P2_P1, 8, 40, 1, 0, a, b, None), EINVAL, "OPR_P2_P1 needs tmp1")


def test_interpolatory_operators(env):
    e, l = env, env.lib
    a, b = ptr(e.a), ptr(e.b)
    refused(e, l.tlab_opr_partial(2, e.y40._h, P1_INT_VP, 8, 40, 1, 0, a, b, None), EUNSUPPORTED,
            "interpolatory operators along y are not built (the RHS staggers x and z only)")
    refused(e, l.tlab_opr_partial(1, e.x64._h, P0_INT_PV, 64, 1, 1, 0, a, b, None), EINVAL,
            "the plan has no interpolation tables: tlab_fdm_plan_set_stagger")


def test_boundary_bcs_neumann_y(env):
    e, l = env, env.lib
    a, b, c, d = ptr(e.a), ptr(e.b), ptr(e.c), ptr(e.d)
    refused(e, l.tlab_boundary_bcs_neumann_y(e.x64._h, 1, 1, 64, 1, a, b, c, d), EINVAL, "BOUNDARY_BCS_NEUMANN_Y: periodic direction")
    refused(e, l.tlab_boundary_bcs_neumann_y(e.y40._h, 0, 8, 40, 1, a, b, c, d), EINVAL,
            "BOUNDARY_BCS_NEUMANN_Y: ibc must be 1 (jmin), 2 (jmax) or 3 (both)")


def test_burgers_arguments(env):
    e, l = env, env.lib
    a, b, c = ptr(e.a), ptr(e.b), ptr(e.c)
    refused(e, l.tlab_opr_burgers(1, e.x64._h, 2, 64, 1, 1, 0, 1.0, a, None, b, c, 0), EINVAL, "ivel must be OPR_B_SELF or OPR_B_U_IN")
    nu = (ctypes.c_double * 5)(1.0, 1.0, 1.0, 1.0, 1.0)
    s, r = ptrs(e.a, e.a, e.a, e.a, e.a), ptrs(e.b, e.b, e.b, e.b, e.b)
    refused(e, l.tlab_opr_burgers_add_n(1, e.x64._h, 64, 1, 1, 0, 5, nu, s, c, r, None, None, 0), EINVAL,
            "tlab_opr_burgers_add_n: bad arguments (1 to 4 fields)")


def test_anelastic_profiles(env):
    e, l = env, env.lib
    a, b, c = ptr(e.a), ptr(e.b), ptr(e.c)
    dp = ctypes.POINTER(ctypes.c_double)
    rb = np.linspace(1.0, 2.0, 40)
    ri = 1.0 / rb
    bad = ri * 1.001
    refused(e, l.tlab_opr_burgers_set_anelastic(40, rb.ctypes.data_as(dp), bad.ctypes.data_as(dp)), EINVAL, "ribackground must be 1 / rbackground")
    assert l.tlab_opr_burgers_set_anelastic(40, rb.ctypes.data_as(dp), ri.ctypes.data_as(dp)) == 0
    try:
        refused(e, l.tlab_opr_burgers(1, e.x64._h, B_SELF, 64, 1, 1, 0, 1.0, a, None, b, c, 0), EINVAL, "anelastic profiles were given for another ny")
    finally:
        assert l.tlab_opr_burgers_set_anelastic(0, None, None) == 0


def test_filter_sizes_that_do_not_match_the_box(env):
    e, l = env, env.lib
    a, b = ptr(e.a), ptr(e.b)
    refused(e, l.tlab_opr_filter_1d(1, e.f64, 32, 1, 1, a, b), EINVAL, "filter size does not match the field size along dir")
    refused(e, l.tlab_opr_filter_1d(2, e.f64, 8, 40, 1, a, b), EINVAL, "filter size does not match the field size along dir")
    refused(e, l.tlab_opr_filter(32, 1, 1, e.f64, None, None, None, a, b), EINVAL,
            "tlab_opr_filter: filter size does not match the field size along its direction")
    refused(e, l.tlab_opr_filter(8, 40, 1, None, e.f64, None, None, a, b), EINVAL,
            "tlab_opr_filter: filter size does not match the field size along its direction")
    rep = (ctypes.c_int * 3)(0, 1, 1)
    refused(e, l.tlab_opr_filter(64, 1, 1, e.f64, None, None, rep, a, b), EINVAL, "tlab_opr_filter: Filter.Repeat must be positive (opr_filter.f90:198-204)")
    refused(e, l.tlab_opr_filter_fields(32, 1, 1, e.f64, None, None, None, 1, ptrs(e.a)), EINVAL,
            "tlab_opr_filter_fields: filter size does not match the field size along its direction")
