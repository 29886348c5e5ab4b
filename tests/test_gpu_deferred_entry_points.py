"""Every public entry point that enqueues work, or that changes what a substep reads, called through RAW ctypes while the last substep of a step is
still only recorded by the deferred tail (csrc/deferred.cpp): the record must run first, whole, as ONE fused substep.  The Python wrappers of
tlab_amd.operators hand the library torch's stream before every call, and that call flushes -- which is how the operators of csrc/operators.cpp could take the
stream without a flush and no test saw it.  A Fortran host goes straight to the C ABI, as the calls here do; nothing in this file hands the library a
stream, and the wrappers' helper is made to raise while a case runs.

tests/deferred_entry_points.py classifies the ABI; CASES below holds one call per `stream` and `setter` name (VARIANTS: further calls of a name).
Driver: tests/test_gpu_deferred.py's, 256 x 64 x 32, stretched y, one scalar -- the smallest box on which these operators take their fused paths.

stream case (L, d, out): reads a state array of the driver (q[0]; q[1] for the y operators; s[0] as the transported field), writes into the test's own
scratch d.W (tmp1 / tmp2: the driver's txc[5:], as a Fortran host would), and names what it wrote in out["dev"] / out["host"].  Four runs:
  off      layer off: RHS + DAXPYs execute at once, then the call                          -> the result in the right order
  on       layer on: zero fills, RHS, DAXPYs recorded, then the call, then tlab_sync
  flushed  the same with tlab_deferred_flush() in front of the call
  reversed layer off: the call FIRST, then RHS + DAXPYs                                      -> what a call that ran ahead of the record gives
`on` equals `flushed` to the bit in everything the call wrote and in q, s, hq, hs, and the counters of both say: one fused substep, the zero fills its
begin_step, nothing literal.  That is the claim "the call flushed first", with no tolerance.  `off` differs from `reversed` in what the call wrote
(in the fields, where the call works in place on them): the case can see a call that ran ahead.  Calls whose input must be larger than a field
(spectral arrays) read the driver's txc[0], which the substep leaves its pressure in.

setter case: the substep is recorded, the setter called, tlab_sync: the fields are those of the run with tlab_deferred_flush() in front of the
setter -- the pending substep ran with the OLD state.  Its power: with the layer off the same sequence after the setter differs from the one before
it (where a replay never reads the setting -- it replays without bounds, and the monitors' and filters' settings belong to other entry points -- the
entry point that does read it is run behind the sequence, `probe`).  Every setting is put back after every run."""
import ctypes
import numpy as np
import pytest

from deferred_entry_points import ENTRY_POINTS, SETTER
from test_gpu_deferred import _dns, _fields, _stats, _two

pytestmark = pytest.mark.gpu

NX, NY, NZ = 256, 64, 32
N = NX * NY * NZ
DTE, KCO, NU = 1e-3, -5.0 / 9.0, 1.0 / 500.0
ZK, ZNX, ZNY = 64, 7, 5            # the smallest z-slab plan of tests/test_gpu_zslab_operators.py: 64 of 192 planes, 7 x 5 points each
ZNL = ZNX * ZNY
c_vp, c_int, c_dbl, c_ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong

CASES, VARIANTS = {}, {}


def case(name, variant=None, **opts):
    """opts: pre / post (run once around all runs of the case), before (run in every run, on the fresh fields, ahead of the sequence), zeros (the record opens with the zero fills; False: tendencies hold garbage and the
    replay accumulates), marker / relax (the record carries TLab_Sources_Flow / the scalar relaxation), liquid (s carries a liquid array),
    reset (setters: puts the old setting back), probe (setters: a reader run behind the sequence in the power runs)"""
    def deco(fn):
        fn.entry, fn.opts = name, dict(dict(pre=None, post=None, before=None, zeros=True, marker=False, relax=False, liquid=False, reset=None, probe=None), **opts)
        if variant is None:
            assert name not in CASES
            CASES[name] = fn
        else:
            VARIANTS["%s[%s]" % (name, variant)] = fn
        return fn
    return deco


def P(t, offset=0):
    return c_vp(t.data_ptr() + 8 * offset)


def PA(ts):
    return (c_vp * len(ts))(*[t.data_ptr() for t in ts])


def H(a):
    return a.ctypes.data


def ok(code, what=""):
    from tlab_amd.lib import check
    check(code, what)


def host(out, n, value=0.0):
    a = np.full(n, value)
    out["host"].append(a)
    return a


# ---------------------------------------------------------------------------------------------------------------------------------------------
# csrc/operators.cpp: the operators
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _partial(dir, type, u, tmp=False):
    def call(L, d, out):
        u_ = d.q[1] if u == "v" else d.q[0]
        ok(L.tlab_opr_partial(dir, d.g[dir - 1]._h, type, NX, NY, NZ, 0, P(u_), P(d.W[0]), P(d.txc[5]) if tmp else None), "tlab_opr_partial")
        out["dev"] += [d.W[0][:N]] + ([d.txc[5][:N]] if tmp else [])
    return call


case("tlab_opr_partial")(_partial(1, 1, "u"))
case("tlab_opr_partial", "y P1")(_partial(2, 1, "v"))
case("tlab_opr_partial", "z P1")(_partial(3, 1, "u"))
case("tlab_opr_partial", "x P2")(_partial(1, 2, "u", tmp=True))
case("tlab_opr_partial", "y P2_P1")(_partial(2, 3, "v", tmp=True))
case("tlab_opr_partial", "z P2")(_partial(3, 2, "u", tmp=True))


@case("tlab_opr_partial", "x P0_INT_VP")
def _(L, d, out):
    ok(L.tlab_opr_partial(1, d.gxs._h, 7, NX, NY, NZ, 0, P(d.q[0]), P(d.W[0]), None), "tlab_opr_partial")
    out["dev"] += [d.W[0][:N]]


def _partial_add(L, d, out):
    ok(L.tlab_opr_partial_add(1, d.g[0]._h, NX, NY, NZ, 0, P(d.q[0]), P(d.q[2]), 0.5, P(d.W[0]), 1, P(d.txc[5]), P(d.txc[6])), "tlab_opr_partial_add")
    out["dev"] += [d.W[0][:N]]
    out["path"] = L.tlab_last_kernel_path()


case("tlab_opr_partial_add")(_partial_add)                                     # the fused kernel (path 2: wave per x line)
# ... and the reference's own sequence through tmp1, tmp2: the generic kernels are forced BEFORE anything is recorded (the switch flushes too)
case("tlab_opr_partial_add", "unfused", pre=lambda L, d: ok(L.tlab_force_kernel_path(1)), post=lambda L, d: ok(L.tlab_force_kernel_path(0)))(
    lambda L, d, out: _partial_add(L, d, out))


@case("tlab_opr_burgers")
def _(L, d, out):
    ok(L.tlab_opr_burgers(1, d.g[0]._h, 1, NX, NY, NZ, 0, NU, P(d.s[0]), P(d.q[0]), P(d.W[0]), P(d.txc[5]), 0), "tlab_opr_burgers")
    out["dev"] += [d.W[0][:N]]


@case("tlab_opr_burgers", "y")
def _(L, d, out):
    ok(L.tlab_opr_burgers(2, d.g[1]._h, 1, NX, NY, NZ, 0, NU, P(d.s[0]), P(d.q[1]), P(d.W[0]), P(d.txc[5]), 0), "tlab_opr_burgers")
    out["dev"] += [d.W[0][:N]]


@case("tlab_opr_burgers_add")
def _(L, d, out):
    ok(L.tlab_opr_burgers_add(1, d.g[0]._h, NX, NY, NZ, 0, NU, P(d.s[0]), P(d.q[0]), P(d.W[0]), P(d.txc[5]), P(d.txc[6])), "tlab_opr_burgers_add")
    out["dev"] += [d.W[0][:N]]


@case("tlab_opr_burgers_add_n")
def _(L, d, out):
    nu = (c_dbl * 2)(NU, NU / 0.7)
    ok(L.tlab_opr_burgers_add_n(1, d.g[0]._h, NX, NY, NZ, 0, 2, nu, PA([d.s[0], d.q[2]]), P(d.q[0]), PA(d.W[:2]), P(d.txc[5]), P(d.txc[6]), 1),
       "tlab_opr_burgers_add_n")
    out["dev"] += [d.W[0][:N], d.W[1][:N]]


@case("tlab_opr_gradient_final")
def _(L, d, out):
    ok(L.tlab_opr_gradient_final(1, d.g[0]._h, NX, NY, NZ, P(d.q[0]), P(d.W[0]), P(d.W[1]), DTE, KCO, 1, P(d.txc[5])), "tlab_opr_gradient_final")
    out["dev"] += [d.W[0][:N], d.W[1][:N]]


@case("tlab_boundary_bcs_neumann_y")
def _(L, d, out):
    ok(L.tlab_boundary_bcs_neumann_y(d.g[1]._h, 3, NX, NY, NZ, P(d.q[1]), P(d.W[0]), P(d.W[1]), P(d.txc[5])), "tlab_boundary_bcs_neumann_y")
    out["dev"] += [d.W[0][:NX * NZ], d.W[1][:NX * NZ]]


@case("tlab_transpose")
def _(L, d, out):
    ok(L.tlab_transpose(P(d.q[0]), NX, NY * NZ, P(d.W[0])), "tlab_transpose")
    out["dev"] += [d.W[0][:N]]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# runtime: the sync and the copies (what they return is read AFTER them, by a copy torch enqueues)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@case("tlab_sync")
def _(L, d, out):
    ok(L.tlab_sync(), "tlab_sync")
    d.W[0][:N].copy_(d.q[0])
    out["dev"] += [d.W[0][:N]]


@case("tlab_memcpy_d2h")
def _(L, d, out):
    ok(L.tlab_memcpy_d2h(H(host(out, N)), P(d.q[0]), 8 * N), "tlab_memcpy_d2h")


@case("tlab_memcpy_h2d")
def _(L, d, out):                       # in place on u: the substep must not run on top of the copy
    ok(L.tlab_memcpy_h2d(P(d.q[0]), H(d.host_field), 8 * N), "tlab_memcpy_h2d")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the pointwise loops
# ---------------------------------------------------------------------------------------------------------------------------------------------
@case("tlab_pw_add3")
def _(L, d, out):
    ok(L.tlab_pw_add3(P(d.W[0]), P(d.q[0]), P(d.q[1]), P(d.q[2]), N))
    out["dev"] += [d.W[0][:N]]


@case("tlab_pw_axpy3")
def _(L, d, out):
    ok(L.tlab_pw_axpy3(P(d.W[0]), P(d.W[1]), P(d.W[2]), P(d.hq[0]), P(d.hq[1]), P(d.hq[2]), P(d.q[0]), P(d.q[1]), P(d.q[2]), 1.0 / DTE, N))
    out["dev"] += [w[:N] for w in d.W[:3]]


@case("tlab_pw_sum3")
def _(L, d, out):
    ok(L.tlab_pw_sum3(P(d.W[0]), P(d.q[0]), P(d.s[0]), N))
    out["dev"] += [d.W[0][:N]]


@case("tlab_pw_sub3")
def _(L, d, out):
    ok(L.tlab_pw_sub3(P(d.W[0]), P(d.W[1]), P(d.W[2]), P(d.q[0]), P(d.q[1]), P(d.q[2]), N))
    out["dev"] += [w[:N] for w in d.W[:3]]


@case("tlab_pw_rk_update")
def _(L, d, out):                       # W += 0.5 u (scale = 0: the second array is only read)
    ok(L.tlab_pw_rk_update(P(d.W[0]), P(d.q[0]), 0.5, 1.0, 0, N))
    out["dev"] += [d.W[0][:N]]


@case("tlab_pw_fill")
def _(L, d, out):                       # in place on a tendency: a fill that ran ahead is accumulated over by the RHS
    ok(L.tlab_pw_fill(P(d.hq[0]), 3.0, N))


@case("tlab_pw_clip")
def _(L, d, out):                       # in place on the scalar: a clip that ran ahead is undone by the update
    ok(L.tlab_pw_clip(P(d.s[0]), -0.05, 0.05, N))


@case("tlab_pw_scale")
def _(L, d, out):                       # in place on a tendency
    ok(L.tlab_pw_scale(P(d.hq[1]), KCO, N))


@case("tlab_pw_final_update")
def _(L, d, out):
    ok(L.tlab_pw_final_update(P(d.W[0]), P(d.W[1]), P(d.q[0]), None, None, DTE, KCO, 1, NX, NY, NZ))
    out["dev"] += [d.W[0][:N], d.W[1][:N]]


@case("tlab_pw_get_wall_planes")
def _(L, d, out):                       # (u is zero on its walls: the box is taken one row up, NZ - 1 planes of it, so that the planes read hold data)
    ok(L.tlab_pw_get_wall_planes(P(d.q[0], NX), P(d.W[0]), P(d.W[1]), NX, NY, NZ - 1))
    out["dev"] += [d.W[0][:NX * NZ], d.W[1][:NX * NZ]]


@case("tlab_pw_fill_wall_planes")
def _(L, d, out):                       # in place on a tendency, whose wall planes the RHS sets itself
    ok(L.tlab_pw_fill_wall_planes(P(d.hq[0]), 2.0, -2.0, NX, NY, NZ))


@case("tlab_pw_set_wall_planes")
def _(L, d, out):                       # the planes handed in are rows 5.. and 9.. of u
    ok(L.tlab_pw_set_wall_planes(P(d.W[0]), P(d.q[0], 5 * NX), P(d.q[0], 9 * NX), NX, NY, NZ))
    out["dev"] += [d.W[0][:N]]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# z-slab operators: the operand is u read as 70 planes of 7 x 5 points, the slab its planes 3 .. 66
# ---------------------------------------------------------------------------------------------------------------------------------------------
@case("tlab_zslab_partial_z")
def _(L, d, out):
    ok(L.tlab_zslab_partial_z(d.zplan, 1, ZNX, ZNY, P(d.q[0], 3 * ZNL), None, 0.0, P(d.W[0]), P(d.W[1]), None, None, P(d.W[2]), 0), "tlab_zslab_partial_z")
    out["dev"] += [d.W[0][:ZNL], d.W[1][:ZNL]]


@case("tlab_zslab_burgers_z")
def _(L, d, out):
    ok(L.tlab_zslab_burgers_z(d.zplan, 1, ZNX, ZNY, NU, P(d.s[0], 3 * ZNL), P(d.q[0], 3 * ZNL), P(d.W[0]), P(d.W[1]), None, None, P(d.W[2]), 0),
       "tlab_zslab_burgers_z")
    out["dev"] += [d.W[0][:2 * ZNL], d.W[1][:2 * ZNL]]


@case("tlab_zslab_burgers_z_n")
def _(L, d, out):
    nu = (c_dbl * 2)(NU, NU / 0.7)
    s = (c_vp * 2)(P(d.s[0], 3 * ZNL).value, P(d.q[2], 3 * ZNL).value)
    ok(L.tlab_zslab_burgers_z_n(d.zplan, 1, ZNX, ZNY, 2, nu, s, P(d.q[0], 3 * ZNL), P(d.W[0]), P(d.W[1]), None, None, PA(d.W[2:4]), 0), "tlab_zslab_burgers_z_n")
    out["dev"] += [d.W[0][:4 * ZNL], d.W[1][:4 * ZNL]]


@case("tlab_zslab_gradient_final_z")
def _(L, d, out):                       # phase 2 with zero messages from the neighbours
    ok(L.tlab_zslab_gradient_final_z(d.zplan, ZNX, ZNY, P(d.q[0], 3 * ZNL), P(d.W[2]), P(d.W[3]), P(d.W[0]), P(d.W[1]), DTE, KCO, 1),
       "tlab_zslab_gradient_final_z")
    out["dev"] += [d.W[0][:ZK * ZNL], d.W[1][:ZK * ZNL]]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# filters
# ---------------------------------------------------------------------------------------------------------------------------------------------
@case("tlab_opr_filter_1d")
def _(L, d, out):
    ok(L.tlab_opr_filter_1d(1, d.fx._h, NX, NY, NZ, P(d.q[0]), P(d.W[0])), "tlab_opr_filter_1d")
    out["dev"] += [d.W[0][:N]]


@case("tlab_opr_filter")
def _(L, d, out):                       # in place on u
    ok(L.tlab_opr_filter(NX, NY, NZ, d.fx._h, None, None, None, P(d.q[0]), P(d.txc[5])), "tlab_opr_filter")


@case("tlab_opr_filter_fields")
def _(L, d, out):                       # in place on u and the scalar
    ok(L.tlab_opr_filter_fields(NX, NY, NZ, d.fx._h, None, None, None, 2, PA([d.q[0], d.s[0]])), "tlab_opr_filter_fields")


def _set_filter(L, d, on):
    ok(L.tlab_dns_set_filter(d._h, d.fx._h if on else None, None, None, None), "tlab_dns_set_filter")


@case("tlab_dns_filter", pre=lambda L, d: _set_filter(L, d, True), post=lambda L, d: _set_filter(L, d, False))
def _dns_filter(L, d, out):             # in place on q and s
    ok(L.tlab_dns_filter(d._h, PA(d.q), PA(d.s)), "tlab_dns_filter")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the Poisson stages on the driver's own plan; spectral inputs are the driver's txc[0] (the pressure of the substep)
# ---------------------------------------------------------------------------------------------------------------------------------------------
@case("tlab_poisson_fft_x")
def _(L, d, out):
    ok(L.tlab_poisson_fft_x(d.poisson._h, 1, P(d.q[0]), P(d.W[0])), "tlab_poisson_fft_x")
    out["dev"] += [d.W[0]]


@case("tlab_poisson_fft_x_packed")
def _(L, d, out):
    ok(L.tlab_poisson_fft_x_packed(d.poisson._h, 1, P(d.q[0]), P(d.W[0]), 1, (c_int * 1)(0), (c_ll * 1)(0)), "tlab_poisson_fft_x_packed")
    out["dev"] += [d.W[0]]


@case("tlab_poisson_set_wall_planes")
def _(L, d, out):
    ok(L.tlab_poisson_set_wall_planes(d.poisson._h, P(d.W[0]), P(d.q[0], 5 * NX), P(d.q[0], 9 * NX)), "tlab_poisson_set_wall_planes")
    out["dev"] += [d.W[0]]


@case("tlab_poisson_fft_z")
def _(L, d, out):
    ok(L.tlab_poisson_fft_z(d.poisson._h, 1, P(d.txc[0]), P(d.W[0])), "tlab_poisson_fft_z")
    out["dev"] += [d.W[0]]


@case("tlab_poisson_ode")
def _(L, d, out):
    ok(L.tlab_poisson_ode(d.poisson._h, P(d.txc[0]), P(d.W[0]), P(d.W[1])), "tlab_poisson_ode")
    out["dev"] += [d.W[0], d.W[1]]


@case("tlab_opr_poisson")
def _(L, d, out):                       # in place on txc[0]; zero Neumann data
    ok(L.tlab_opr_poisson(d.poisson._h, NX, NY, NZ, 3, P(d.txc[0]), P(d.W[0]), P(d.W[1]), P(d.W[2]), P(d.W[3]), P(d.W[4])), "tlab_opr_poisson")
    out["dev"] += [d.txc[0], d.W[4]]


@case("tlab_opr_helmholtz")
def _(L, d, out):
    ok(L.tlab_opr_helmholtz(d.poisson._h, NX, NY, NZ, 3, -10.0, P(d.txc[0]), P(d.W[0]), P(d.W[1]), P(d.W[2]), P(d.W[3])), "tlab_opr_helmholtz")
    out["dev"] += [d.txc[0]]


@case("tlab_pencil_repack")
def _(L, d, out):                       # u read as a complex slab (64, 64, 32)
    ok(L.tlab_pencil_repack(P(d.q[0]), P(d.W[0]), 64, NY, NZ, 1, (c_int * 1)(0), 1), "tlab_pencil_repack")
    out["dev"] += [d.W[0][:N // 2]]


@case("tlab_pencil_repack_blocks")
def _(L, d, out):
    ok(L.tlab_pencil_repack_blocks(P(d.q[0]), P(d.W[0]), 64, NY, NZ, 1, (c_int * 1)(0), (c_ll * 1)(0), 1), "tlab_pencil_repack_blocks")
    out["dev"] += [d.W[0][:N // 2]]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the driver's own stream entry points
# ---------------------------------------------------------------------------------------------------------------------------------------------
@case("tlab_rhs_global_incompressible_1")
def _rhs_into_scratch(L, d, out):       # tendencies of the test's own
    ok(L.tlab_rhs_global_incompressible_1(d._h, DTE, PA(d.q), PA(d.s), PA(d.W[:3]), PA(d.W[3:4]), PA(d.txc)), "tlab_rhs_global_incompressible_1")
    out["dev"] += [w[:N] for w in d.W[:4]]


@case("tlab_time_substep_incompressible_explicit")
def _substep(L, d, out):                # in place: the second substep of the step
    ok(L.tlab_time_substep_incompressible_explicit(d._h, 0.9 * DTE, KCO, 1, PA(d.q), PA(d.s), PA(d.hq), PA(d.hs), PA(d.txc)),
       "tlab_time_substep_incompressible_explicit")


def _coriolis(L, d, on):
    ok(L.tlab_dns_set_coriolis(d._h, 4 if on else 0, (c_dbl * 3)(0.3, -0.2, 0.5) if on else None, (c_dbl * 2)(0.0, 1.0) if on else None), "tlab_dns_set_coriolis")


@case("tlab_dns_sources_flow", pre=lambda L, d: _coriolis(L, d, True), post=lambda L, d: _coriolis(L, d, False))
def _(L, d, out):
    ok(L.tlab_dns_sources_flow(d._h, PA(d.q), PA(d.s), PA(d.W[:3])), "tlab_dns_sources_flow")
    out["dev"] += [w[:N] for w in d.W[:3]]


def _zone(L, d, group, size):
    nf = 3 if group == 0 else 1
    tau = np.ascontiguousarray(np.tile(0.5 + 0.25 * np.arange(max(size, 1)), (nf, 1)))       # (size, nfields) column-major
    ref = np.full((nf, NZ, max(size, 1), NX), 0.3)
    dp = ctypes.POINTER(c_dbl)
    ok(L.tlab_dns_set_buffer_zone(d._h, 3, group, size, nf, tau.ctypes.data_as(dp) if size else None, ref.ctypes.data_as(dp) if size else None),
       "tlab_dns_set_buffer_zone")


def _zones_on(group):
    def pre(L, d):
        ok(L.tlab_dns_set_buffer_type(d._h, 1), "tlab_dns_set_buffer_type")
        _zone(L, d, group, 8)
    return pre


def _zones_off(L, d):
    ok(L.tlab_dns_set_buffer_type(d._h, 0), "tlab_dns_set_buffer_type")


@case("tlab_dns_buffer_relax_flow", pre=_zones_on(0), post=_zones_off)
def _(L, d, out):
    ok(L.tlab_dns_buffer_relax_flow(d._h, PA(d.q), PA(d.W[:3])), "tlab_dns_buffer_relax_flow")
    out["dev"] += [w[:N] for w in d.W[:3]]


@case("tlab_dns_buffer_relax_scal", pre=_zones_on(1), post=_zones_off)
def _(L, d, out):
    ok(L.tlab_dns_buffer_relax_scal(d._h, PA(d.s), PA(d.W[:1])), "tlab_dns_buffer_relax_scal")
    out["dev"] += [d.W[0][:N]]


def _mixture(L, d, on):
    par = (c_dbl * 2)(0.5, 0.1)
    ok(L.tlab_dns_set_mixture(d._h, 12 if on else 0, par if on else None, 2 if on else 0), "tlab_dns_set_mixture")


def _infrared(L, d, on):
    ok(L.tlab_dns_set_infrared(d._h, 1 if on else 0, 1, 3.0, 2.0, 0.0), "tlab_dns_set_infrared")


def _cloud_on(L, d):
    _mixture(L, d, True)
    _infrared(L, d, True)


def _cloud_off(L, d):
    _infrared(L, d, False)
    _mixture(L, d, False)


@case("tlab_dns_diagnostic", pre=lambda L, d: _mixture(L, d, True), post=lambda L, d: _mixture(L, d, False), liquid=True)
def _(L, d, out):                       # the liquid into an array of the test's own (the substep refreshes the driver's)
    ok(L.tlab_dns_diagnostic(d._h, PA([d.s[0], d.W[0]])), "tlab_dns_diagnostic")
    out["dev"] += [d.W[0][:N]]


@case("tlab_dns_sources_scal", pre=_cloud_on, post=_cloud_off, liquid=True)
def _(L, d, out):                       # reads the driver's liquid, which the substep refreshes at its end; nothing is called in front of it
    ok(L.tlab_dns_sources_scal(d._h, PA([d.s[0], d.liq]), PA(d.W[:1]), PA(d.txc)), "tlab_dns_sources_scal")
    out["dev"] += [d.W[0][:N]]


@case("tlab_dns_pressure")
def _(L, d, out):
    ok(L.tlab_dns_pressure(d._h, 3, PA(d.q), PA(d.s), P(d.W[0]), P(d.W[1]), P(d.W[2]), PA(d.W[3:6]), 3), "tlab_dns_pressure")
    out["dev"] += [d.W[0][:N]]


@case("tlab_time_courant")
def _(L, d, out):
    pmax, dt = host(out, 2), host(out, 1)
    dp = ctypes.POINTER(c_dbl)
    ok(L.tlab_time_courant(d._h, PA(d.q), 0.6, 0.15, pmax.ctypes.data_as(dp), dt.ctypes.data_as(dp)), "tlab_time_courant")


def _dilatation(L, d, out):
    dp, ip = ctypes.POINTER(c_dbl), ctypes.POINTER(c_int)
    mn, mx = host(out, 1), host(out, 1)
    lmin, lmax = np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)
    out["host"] += [lmin, lmax]
    ok(L.tlab_dns_dilatation_extremes(d._h, PA(d.q), PA(d.txc), mn.ctypes.data_as(dp), mx.ctypes.data_as(dp), lmin.ctypes.data_as(ip), lmax.ctypes.data_as(ip)),
       "tlab_dns_dilatation_extremes")


case("tlab_dns_dilatation_extremes")(_dilatation)


@case("tlab_fi_invariant_p")
def _(L, d, out):
    ok(L.tlab_fi_invariant_p(d._h, P(d.q[0]), P(d.q[1]), P(d.q[2]), P(d.W[0]), P(d.txc[5])), "tlab_fi_invariant_p")
    out["dev"] += [d.W[0][:N]]


@case("tlab_fi_vorticity")
def _(L, d, out):
    ok(L.tlab_fi_vorticity(d._h, P(d.q[0]), P(d.q[1]), P(d.q[2]), P(d.W[0]), PA(d.W[1:7])), "tlab_fi_vorticity")
    out["dev"] += [d.W[0][:N]]


@case("tlab_fi_gradient")
def _(L, d, out):
    ok(L.tlab_fi_gradient(d._h, P(d.s[0]), P(d.W[0]), P(d.txc[5])), "tlab_fi_gradient")
    out["dev"] += [d.W[0][:N]]


def _minmax(entry):
    def call(L, d, out):
        dp = ctypes.POINTER(c_dbl)
        mn, mx = host(out, 1), host(out, 1)
        if entry == "tlab_minmax":
            ok(L.tlab_minmax(d._h, P(d.q[0]), NX, NY, NZ, mn.ctypes.data_as(dp), mx.ctypes.data_as(dp)), entry)
        else:
            ok(getattr(L, entry)(P(d.q[0]), N, mn.ctypes.data_as(dp), mx.ctypes.data_as(dp)), entry)
    return call


for _e in ("tlab_minmax", "tlab_minmax_any", "tlab_device_minmax"):
    case(_e)(_minmax(_e))


@case("tlab_vorticity_from_gradients")
def _(L, d, out):
    ok(L.tlab_vorticity_from_gradients(N, P(d.q[0]), P(d.q[1]), P(d.q[2]), P(d.s[0]), P(d.q[1]), P(d.q[0]), P(d.W[0])), "tlab_vorticity_from_gradients")
    out["dev"] += [d.W[0][:N]]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# plane statistics and sampling: profiles come back on the host
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _means(k):
    return [np.full(NY, 0.01 * (i + 1)) for i in range(k)]


@case("tlab_avg_ik_v")
def _(L, d, out):
    ok(L.tlab_avg_ik_v(NX, NY, NZ, 2, PA([d.q[0], d.s[0]]), H(host(out, 2 * NY)), NY), "tlab_avg_ik_v")


@case("tlab_avg1v2d_v")
def _(L, d, out):
    ok(L.tlab_avg1v2d_v(NX, NY, NZ, 2, P(d.q[0]), H(host(out, NY))), "tlab_avg1v2d_v")


@case("tlab_avg_moments_flow")
def _(L, d, out):
    m = _means(3)
    ok(L.tlab_avg_moments_flow(NX, NY, NZ, P(d.q[0]), P(d.q[1]), P(d.q[2]), None, H(m[0]), H(m[1]), H(m[2]), None, H(host(out, 18 * NY)), NY), "tlab_avg_moments_flow")


@case("tlab_avg_moments_scal")
def _(L, d, out):
    m = _means(4)
    ok(L.tlab_avg_moments_scal(NX, NY, NZ, P(d.s[0]), P(d.q[0]), P(d.q[1]), P(d.q[2]), None, H(m[0]), H(m[1]), H(m[2]), H(m[3]), None, H(host(out, 10 * NY)), NY),
       "tlab_avg_moments_scal")


def _nine(d):
    return PA([d.q[0], d.q[1], d.q[2], d.s[0], d.q[0], d.q[1], d.q[2], d.s[0], d.q[0]])


@case("tlab_avg_gradients_flow")
def _(L, d, out):                       # (the nine "derivatives" are the state arrays themselves: any fields serve the reduction)
    m = _means(6)
    ok(L.tlab_avg_gradients_flow(NX, NY, NZ, _nine(d), P(d.q[0]), P(d.q[1]), P(d.q[2]), None, H(m[0]), H(m[1]), H(m[2]), None, H(m[3]), H(m[4]), H(m[5]),
                                 H(host(out, 50 * NY)), NY), "tlab_avg_gradients_flow")


@case("tlab_avg_ugradp")
def _(L, d, out):
    ok(L.tlab_avg_ugradp(NX, NY, NZ, P(d.q[0]), P(d.q[1]), P(d.q[2]), P(d.s[0]), P(d.q[0]), P(d.q[1]), H(host(out, NY))), "tlab_avg_ugradp")


@case("tlab_avg_gradients_scal")
def _(L, d, out):
    m = _means(6)
    ok(L.tlab_avg_gradients_scal(NX, NY, NZ, PA([d.q[0], d.q[1], d.q[2]]), P(d.s[0]), P(d.q[0]), P(d.q[1]), P(d.q[2]), None, H(m[0]), H(m[1]), H(m[2]), H(m[3]),
                                 None, H(m[4]), H(m[5]), H(host(out, 15 * NY)), NY), "tlab_avg_gradients_scal")


@case("tlab_avg_gradients_pass")
def _(L, d, out):                       # pass 4: dsdx dsdy dsdz with the mean rS_y, 11 columns
    m = _means(1)
    ok(L.tlab_avg_gradients_pass(4, 0, NX, NY, NZ, PA([d.q[0], d.q[1], d.s[0]]), (c_vp * 1)(H(m[0])), H(host(out, 11 * NY)), NY), "tlab_avg_gradients_pass")


@case("tlab_dns_avg_gradients_flow")
def _(L, d, out):
    m = _means(6)
    ok(L.tlab_dns_avg_gradients_flow(d._h, PA(d.q), None, PA(d.txc), H(m[0]), H(m[1]), H(m[2]), None, H(m[3]), H(m[4]), H(m[5]), H(host(out, 50 * NY)), NY),
       "tlab_dns_avg_gradients_flow")


@case("tlab_dns_avg_gradients_scal")
def _(L, d, out):
    m = _means(6)
    ok(L.tlab_dns_avg_gradients_scal(d._h, P(d.s[0]), PA(d.q), None, PA(d.txc), H(m[0]), H(m[1]), H(m[2]), H(m[3]), None, H(m[4]), H(m[5]), H(host(out, 15 * NY)), NY),
       "tlab_dns_avg_gradients_scal")


@case("tlab_avg_cov2v")
def _(L, d, out):
    ok(L.tlab_avg_cov2v(NX, NY, NZ, P(d.q[0]), P(d.s[0]), H(host(out, 3 * NY)), NY), "tlab_avg_cov2v")


@case("tlab_fluctuation")
def _(L, d, out):
    m = _means(1)
    ok(L.tlab_fluctuation(NX, NY, NZ, P(d.q[0]), H(m[0]), P(d.W[0])), "tlab_fluctuation")
    out["dev"] += [d.W[0][:N]]


@case("tlab_cross_product")
def _(L, d, out):                       # u and the scalar read as N / 2 complex numbers
    ok(L.tlab_cross_product(N // 2, P(d.q[0]), P(d.s[0]), P(d.W[0])), "tlab_cross_product")
    out["dev"] += [d.W[0][:N]]


@case("tlab_gate_threshold")
def _(L, d, out):                       # one byte per point into the first N bytes of the scratch
    ok(L.tlab_gate_threshold(P(d.q[0]), N, 0.0, P(d.W[0])), "tlab_gate_threshold")
    out["dev"] += [d.W[0][:N // 8]]


@case("tlab_pdf_minmax_planes")
def _(L, d, out):
    ok(L.tlab_pdf_minmax_planes(NX, NY, NZ, 2, PA([d.q[0], d.s[0]]), 0, None, H(host(out, 2 * (NY + 1))), H(host(out, 2 * (NY + 1)))), "tlab_pdf_minmax_planes")


@case("tlab_pdf_histogram_planes")
def _(L, d, out):                       # external intervals [-2, 2] in every plane, 32 bins
    ilim = np.zeros(2, dtype=np.int32)
    lo, hi = np.full(2 * (NY + 1), -2.0), np.full(2 * (NY + 1), 2.0)
    ok(L.tlab_pdf_histogram_planes(NX, NY, NZ, 2, 32, H(ilim), H(lo), H(hi), PA([d.q[0], d.s[0]]), 0, None, H(host(out, 34 * (NY + 1) * 2))), "tlab_pdf_histogram_planes")


@case("tlab_pdf1v_n")
def _(L, d, out):                       # local intervals, 32 bins
    ibc = np.array([1, 1], dtype=np.int32)
    ok(L.tlab_pdf1v_n(NX, NY, NZ, 2, 32, H(ibc), None, None, PA([d.q[0], d.s[0]]), 0, None, H(host(out, 34 * (NY + 1) * 2))), "tlab_pdf1v_n")


@case("tlab_pdf2v")
def _(L, d, out):
    nb = np.array([8, 8], dtype=np.int32)
    ok(L.tlab_pdf2v(NX, NY, NZ, H(nb), P(d.q[0]), P(d.s[0]), H(host(out, (64 + 2 + 16) * (NY + 1)))), "tlab_pdf2v")


@case("tlab_inter_n_xz")
def _(L, d, out):                       # the gate is the first N bytes of u as they lie: how often each byte value 1 .. 127 occurs in a plane
    ok(L.tlab_inter_n_xz(NX, NY, NZ, 127, P(d.q[0]), H(host(out, NY * 127))), "tlab_inter_n_xz")


@case("tlab_avg_phase_space")
def _(L, d, out):
    ok(L.tlab_avg_phase_space(NX, NY, NZ, NZ, 2, PA([d.q[0], d.s[0]]), 2, 1, P(d.W[0])), "tlab_avg_phase_space")
    out["dev"] += [d.W[0][:NX * NY * 3 * 2]]


@case("tlab_avg_phase_flow")
def _(L, d, out):
    ok(L.tlab_avg_phase_flow(NX, NY, NZ, NZ, P(d.q[0]), P(d.q[1]), P(d.q[2]), 2, 1, P(d.W[0]), P(d.W[1])), "tlab_avg_phase_flow")
    out["dev"] += [d.W[0][:NX * NY * 3 * 3], d.W[1][:NX * NY * 3 * 6]]


@case("tlab_tower_accumulate")
def _(L, d, out):                       # u, v, w at the towers of every eighth point, into a buffer of the test's own
    ok(L.tlab_tower_reset(d.tower), "tlab_tower_reset")
    ok(L.tlab_tower_accumulate(d.tower, 1, PA(d.q), 0, 0.0, P(d.W[0])), "tlab_tower_accumulate")
    out["dev"] += [d.W[0][:d.tower_bufsize]]


@case("tlab_planes_gather")
def _(L, d, out):                       # the planes j = 5 and j = 40 of u and the scalar, as doubles
    ok(L.tlab_planes_gather(NX, NY, NZ, 2, PA([d.q[0], d.s[0]]), 2, 2, (c_int * 2)(5, 40), P(d.W[0]), 0), "tlab_planes_gather")
    out["dev"] += [d.W[0][:NX * 4 * NZ]]


@case("tlab_log10_small")
def _(L, d, out):                       # in place on a tendency (NaN where it is negative: the comparison is of bits)
    ok(L.tlab_log10_small(N, P(d.hs[0])), "tlab_log10_small")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# setters: out["dev"] names what else the setting can reach
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _onoff(entry, on, off, **opts):
    def apply(L, d, out):
        ok(on(L, d), entry)
    case(entry, reset=lambda L, d: ok(off(L, d), entry), **opts)(apply)


_onoff("tlab_dns_set_fusion", lambda L, d: L.tlab_dns_set_fusion(d._h, 0), lambda L, d: L.tlab_dns_set_fusion(d._h, 1))
_onoff("tlab_dns_set_remove_divergence", lambda L, d: L.tlab_dns_set_remove_divergence(d._h, 0), lambda L, d: L.tlab_dns_set_remove_divergence(d._h, 1))
_onoff("tlab_force_kernel_path", lambda L, d: L.tlab_force_kernel_path(1), lambda L, d: L.tlab_force_kernel_path(0))
_onoff("tlab_set_tuning", lambda L, d: L.tlab_set_tuning(1, 16), lambda L, d: L.tlab_set_tuning(1, 0))       # 16 rows per wave in the y / z tile kernels
_onoff("tlab_opr_burgers_set_dealiasing", lambda L, d: L.tlab_opr_burgers_set_dealiasing(1, d.fx._h), lambda L, d: L.tlab_opr_burgers_set_dealiasing(1, None))
# CompactDirect6 reading of the y plan's first-derivative tables, and back to CompactJacobian6 / CompactJacobian6Hyper
_onoff("tlab_fdm_plan_set_scheme", lambda L, d: L.tlab_fdm_plan_set_scheme(d.g[1]._h, 16, 7), lambda L, d: L.tlab_fdm_plan_set_scheme(d.g[1]._h, 6, 7))


def _rho(d):
    dp = ctypes.POINTER(c_dbl)
    rb = 1.0 + 0.2 * np.asarray(d.y)
    ri = 1.0 / rb
    return rb, ri, rb.ctypes.data_as(dp), ri.ctypes.data_as(dp)


def _dns_anelastic(L, d):
    _, _, a, b = keep = _rho(d)
    rc = L.tlab_dns_set_anelastic(d._h, a, b)
    del keep
    return rc


def _opr_anelastic(L, d):
    _, _, a, b = keep = _rho(d)
    rc = L.tlab_opr_burgers_set_anelastic(NY, a, b)
    del keep
    return rc


_onoff("tlab_dns_set_anelastic", _dns_anelastic, lambda L, d: L.tlab_dns_set_anelastic(d._h, None, None))
_onoff("tlab_opr_burgers_set_anelastic", _opr_anelastic, lambda L, d: L.tlab_opr_burgers_set_anelastic(0, None, None))


def _bcs(L, d, free):
    v = (c_int * 3)(4, 3, 4) if free else (c_int * 3)(3, 3, 3)          # freeslip: {Neumann, Dirichlet, Neumann}
    s = (c_int * 1)(4 if free else 3)
    return L.tlab_dns_set_bcs(d._h, v, v, s, s)


_onoff("tlab_dns_set_bcs", lambda L, d: _bcs(L, d, True), lambda L, d: _bcs(L, d, False))


def _surface(L, d, on):
    t, c = (c_int * 1)(1 if on else 0), (c_dbl * 1)(0.5 if on else 0.0)
    return L.tlab_dns_set_surface_bcs(d._h, t, t, c, c)


_onoff("tlab_dns_set_surface_bcs", lambda L, d: _surface(L, d, True), lambda L, d: _surface(L, d, False))


def _pfilter(L, d, on):
    return L.tlab_dns_set_pressure_filter(d._h, d.fx._h if on else None, None, None, (c_int * 3)(1, 1, 1))


_onoff("tlab_dns_set_pressure_filter", lambda L, d: _pfilter(L, d, True), lambda L, d: _pfilter(L, d, False))


# the flow blocks of the zones act inside the RHS: [BufferZone] Type first, then the block
@case("tlab_dns_set_buffer_zone", pre=lambda L, d: ok(L.tlab_dns_set_buffer_type(d._h, 1)), post=_zones_off, reset=lambda L, d: _zone(L, d, 0, 0))
def _(L, d, out):
    _zone(L, d, 0, 8)


@case("tlab_dns_set_buffer_type", pre=_zones_on(0), post=_zones_off, reset=_zones_on(0))
def _(L, d, out):                       # Type = none switches the block of the set-up off
    ok(L.tlab_dns_set_buffer_type(d._h, 0), "tlab_dns_set_buffer_type")


# the body forces are in a replay only when the record carries the TLab_Sources_Flow marker
@case("tlab_dns_set_coriolis", marker=True, reset=lambda L, d: _coriolis(L, d, False))
def _(L, d, out):
    _coriolis(L, d, True)


def _buoyancy(L, d, on):
    from tlab_amd.dns import body_force_args
    bod = {"type": "linear", "vector": (0.3, -2.0, 0.2), "scalars": 1, "parameters": (1.0, 0.1), "inb_scal_array": 1, "bbackground": 0.2 * np.asarray(d.y)}
    _, args, keep = body_force_args(1, None, bod if on else None)
    ok(L.tlab_dns_set_buoyancy(d._h, *args), "tlab_dns_set_buoyancy")
    del keep


@case("tlab_dns_set_buoyancy", marker=True, reset=lambda L, d: _buoyancy(L, d, False))
def _(L, d, out):
    _buoyancy(L, d, True)


@case("tlab_dns_begin_step", zeros=False, reset=lambda L, d: _rhs_into_scratch(L, d, {"dev": []}))
def _(L, d, out):                       # the record has no zero fills and the tendencies hold garbage: a flag set ahead of the replay would make it overwrite
    ok(L.tlab_dns_begin_step(d._h), "tlab_dns_begin_step")


def _arm(L, d, on):
    ok(L.tlab_dns_arm_pressure_sampling(d._h, None, None, 0, 0.0, P(d.W[0]) if on else None, 1, 1), "tlab_dns_arm_pressure_sampling")


@case("tlab_dns_arm_pressure_sampling", reset=lambda L, d: _arm(L, d, False))
def _(L, d, out):                       # armed after the record: the replay must not take the sample
    _arm(L, d, True)
    out["dev"] += [d.W[0][:NX * NY * 2]]


def _tower_armed(L, d):
    """one whole step accumulated by hand (indices 1, 2, 4: tower_accumulation = 2), then the driver armed: the pressure sample of the next RHS belongs in slot 2"""
    ok(L.tlab_tower_reset(d.tower), "tlab_tower_reset")
    for index, fields in ((1, d.q), (2, d.s), (4, d.q[:1])):
        ok(L.tlab_tower_accumulate(d.tower, index, PA(fields), 0, 0.25, P(d.W[0])), "tlab_tower_accumulate")
    ok(L.tlab_dns_arm_pressure_sampling(d._h, d.tower, P(d.W[0]), 1, 0.5, None, 1, 1), "tlab_dns_arm_pressure_sampling")


@case("tlab_tower_reset", before=_tower_armed, reset=lambda L, d: _arm(L, d, False))
def _(L, d, out):                       # a reset that ran ahead of the record sends the pending sample to slot 1 and leaves the counters at (1, 4)
    ok(L.tlab_tower_reset(d.tower), "tlab_tower_reset")
    sizes = (c_ll * 8)()
    ok(L.tlab_tower_sizes(d.tower, sizes), "tlab_tower_sizes")
    out["dev"] += [d.W[0][:d.tower_bufsize]]
    out["host"] += [np.array(list(sizes), dtype=np.int64)]


# settings no replay reads: the record runs without bounds (test_replay_leaves_the_drivers_own_settings_alone), [Filter] is DNS_FILTER's, the mixture's liquid FI_DIAGNOSTIC's and the infrared term TLab_Sources_Scal's -- their readers are the probes
def _bounds(L, d, on):
    ok(L.tlab_dns_set_scalar_bounds(d._h, 1, (c_int * 1)(1) if on else None, (c_dbl * 1)(-0.05), (c_dbl * 1)(0.05)), "tlab_dns_set_scalar_bounds")


@case("tlab_dns_set_scalar_bounds", reset=lambda L, d: _bounds(L, d, False), probe=_substep)
def _(L, d, out):
    _bounds(L, d, True)


@case("tlab_dns_set_filter", reset=lambda L, d: _set_filter(L, d, False), probe=_dns_filter)
def _(L, d, out):
    _set_filter(L, d, True)


def _liquid_probe(L, d, out):
    ok(L.tlab_dns_diagnostic(d._h, PA([d.s[0], d.W[1]])), "tlab_dns_diagnostic")
    out["dev"] += [d.W[1][:N]]


@case("tlab_dns_set_mixture", liquid=True, reset=lambda L, d: _mixture(L, d, False), probe=_liquid_probe)
def _(L, d, out):
    _mixture(L, d, True)


def _infrared_probe(L, d, out):
    ok(L.tlab_dns_diagnostic(d._h, PA([d.s[0], d.W[1]])), "tlab_dns_diagnostic")
    ok(L.tlab_dns_sources_scal(d._h, PA([d.s[0], d.W[1]]), PA(d.W[:1]), PA(d.txc)), "tlab_dns_sources_scal")
    out["dev"] += [d.W[0][:N]]


@case("tlab_dns_set_infrared", liquid=True, pre=lambda L, d: _mixture(L, d, True), post=lambda L, d: _mixture(L, d, False),
      reset=lambda L, d: _infrared(L, d, False), probe=_infrared_probe)
def _(L, d, out):
    _infrared(L, d, True)


IDS = sorted(CASES) + sorted(VARIANTS)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the runs
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from tlab_amd.lib import load, check
    from tlab_amd.operators import FdmPlan, Filter
    L = load()
    check(L.tlab_init(0), "tlab_init")
    d = _dns(1)
    d.f0 = _fields(d, 21)
    d.W = [torch.zeros(d.isize_txc_field, dtype=torch.float64, device="cuda") for _ in range(8)]
    d.liq = torch.zeros(d.n, dtype=torch.float64, device="cuda")
    d.host_field = np.random.default_rng(3).uniform(-1, 1, d.n)
    d.fx = Filter(2, NX, True)                                                  # explicit6 along the periodic x
    d.gxs = FdmPlan(np.arange(NX) / NX, True, True, stagger=True)               # an x plan with the interpolation tables
    zn = np.arange(3 * ZK) / (3 * ZK) * 2.0
    d.gz192, d.zplan = c_vp(0), c_vp(0)
    check(L.tlab_fdm_plan_create(ctypes.byref(d.gz192), 3 * ZK, zn.ctypes.data_as(ctypes.POINTER(c_dbl)), 1, 1, 6, 7, 0.1), "tlab_fdm_plan_create")
    check(L.tlab_zslab_plan_create(ctypes.byref(d.zplan), d.gz192, ZK, 0, 0), "tlab_zslab_plan_create")
    d.tower, sizes = c_vp(0), (c_ll * 8)()
    check(L.tlab_tower_create(ctypes.byref(d.tower), NX, NY, NZ, (c_int * 3)(8, 8, 8), 2), "tlab_tower_create")
    check(L.tlab_tower_sizes(d.tower, sizes), "tlab_tower_sizes")
    d.tower_bufsize = int(sizes[5])
    assert (d.nx, d.ny, d.nz, d.n) == (NX, NY, NZ, N) and (ZK + 6) * ZNL <= N and 0 < d.tower_bufsize <= d.isize_txc_field
    yield L, d
    L.tlab_tower_destroy(d.tower)
    check(L.tlab_deferred_enable(0), "disable")
    L.tlab_zslab_plan_destroy(d.zplan)
    L.tlab_fdm_plan_destroy(d.gz192)


@pytest.fixture(autouse=True)
def no_wrapper_hands_the_library_a_stream(monkeypatch):
    """the wrappers' helper flushes a record as a side effect: a case that reached it would prove nothing"""
    import tlab_amd.dns
    import tlab_amd.operators

    def refuse():
        raise AssertionError("a case of this file went through a Python wrapper that hands the library a stream")
    monkeypatch.setattr(tlab_amd.operators, "_use_torch_stream", refuse)
    monkeypatch.setattr(tlab_amd.dns, "_use_torch_stream", refuse)


def test_the_guard_refuses_the_wrappers(env):
    import tlab_amd as T
    L, d = env
    with pytest.raises(AssertionError, match="hands the library a stream"):
        T.OPR_Partial_X(T.OPR_P1, NX, NY, NZ, 0, d.g[0], d.q[0], d.W[0][:N], None)


def _bits(t):
    import torch
    t = t if hasattr(t, "data_ptr") else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32 if t.element_size() == 4 else torch.int8)


def _same(a, b):
    import torch
    assert len(a) == len(b), (len(a), len(b))
    return all(u.shape == v.shape and torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


class Run:
    def __init__(self, L, d, fn):
        self.L, self.d, self.fn, self.o = L, d, fn, fn.opts
        self.state = d.s + ([d.liq] if self.o["liquid"] else [])
        self.ptrs = (PA(d.q), PA(self.state), PA(d.hq), PA(d.hs), PA(d.txc))

    def start(self, tendencies):
        import torch
        d = self.d
        for t, a in zip(d.q + d.s, d.f0):
            t.copy_(a)
        for t in d.hq + d.hs:
            t.fill_(tendencies)
        for t in d.txc + d.W + [d.liq]:
            t.zero_()
        torch.cuda.synchronize()

    def sequence(self, on):
        """[TLab_Sources_Flow,] RHS, [scalar relaxation,] DAXPY per field: recorded with the layer on, executed at once with it off.  With a liquid the
        literal sequence ends with FI_DIAGNOSTIC (time.f90:248), which the fused substep of a replay does itself at its end"""
        L, d = self.L, self.d
        q, s, hq, hs, txc = self.ptrs
        if self.o["marker"]:
            ok(L.tlab_deferred_sources_flow(d._h, q, s, hq), "sources marker")
        ok(L.tlab_deferred_rhs(d._h, DTE, q, s, hq, hs, txc), "rhs")
        if self.o["relax"]:
            ok(L.tlab_deferred_relax_scal(d._h), "relax")
        for h, u in zip(d.hq + d.hs, d.q + d.s):
            ok(L.tlab_deferred_axpy(d.n, DTE, P(h), P(u)), "axpy")
        if self.o["liquid"] and not on:
            ok(L.tlab_dns_diagnostic(d._h, s), "diagnostic")

    def collect(self, out):
        import torch
        ok(self.L.tlab_sync(), "tlab_sync")
        torch.cuda.synchronize()
        d = self.d
        fields = [t.clone() for t in d.q + d.s + d.hq + d.hs]
        wrote = [t.clone() for t in out["dev"]] + [torch.from_numpy(np.array(a, copy=True)) for a in out["host"]]
        return wrote, fields

    def layer_off(self, steps):
        """steps: "sequence", "call", "probe" in the order given; the tendencies start at zero (garbage where the record has no zero fills)"""
        L = self.L
        self.start(0.0 if self.o["zeros"] else 7.0)
        out = {"dev": [], "host": []}
        ok(L.tlab_deferred_enable(0), "disable")
        if self.o["before"]:
            self.o["before"](L, self.d)
        for step in steps:
            if step == "sequence":
                self.sequence(False)
            elif step == "call":
                self.fn(L, self.d, out)
            elif self.o["probe"]:
                self.o["probe"](L, self.d, out)
        return self.collect(out)

    def layer_on(self, flush_first):
        """the pending last substep of a step, then the call; returns what it wrote, the fields and the counters' change"""
        L, d = self.L, self.d
        self.start(7.0)                      # garbage the zero fills must take care of
        out = {"dev": [], "host": []}
        if self.o["before"]:
            self.o["before"](L, d)
        before = _stats(L) + list(_two(L.tlab_deferred_sources_stats)) + list(_two(L.tlab_deferred_relax_stats))
        ok(L.tlab_deferred_enable(1), "enable")
        try:
            if self.o["zeros"]:
                for t in d.hq + d.hs:
                    ok(L.tlab_deferred_zero(P(t), d.n), "zero")
            self.sequence(True)
            if flush_first:
                ok(L.tlab_deferred_flush(), "tlab_deferred_flush")
            self.fn(L, d, out)
            got = self.collect(out)
        finally:
            ok(L.tlab_deferred_enable(0), "disable")
        after = _stats(L) + list(_two(L.tlab_deferred_sources_stats)) + list(_two(L.tlab_deferred_relax_stats))
        return got + ([a - b for a, b in zip(after, before)],)


@pytest.mark.parametrize("cid", IDS)
def test_a_pending_record_runs_whole_before_the_call(env, cid):
    L, d = env
    fn = CASES.get(cid) or VARIANTS[cid]
    o = fn.opts
    setter = ENTRY_POINTS[fn.entry] == SETTER
    reset = (lambda: o["reset"](L, d)) if setter else (lambda: None)
    assert not setter or o["reset"] is not None
    run = Run(L, d, fn)
    # one fused substep [that carried the marker / the relaxation], the zero fills its begin_step, nothing literal or eager
    whole = [1, 0, 1 if o["zeros"] else 0, 0, 0, 0, 1 if o["marker"] else 0, 0, 1 if o["relax"] else 0, 0]
    if o["pre"]:
        o["pre"](L, d)
    try:
        try:
            wrote_on, fields_on, counters_on = run.layer_on(False)
        finally:
            reset()
        try:
            wrote_fl, fields_fl, counters_fl = run.layer_on(True)
        finally:
            reset()
        # the power of the case, on the reference path alone: right order against the order of a call that ran ahead of the record
        if setter:      # (the setter closes the right order too, so that both runs name the same arrays)
            try:
                right = run.layer_off(["sequence", "probe", "call"])
            finally:
                reset()
            try:
                ahead = run.layer_off(["call", "sequence", "probe"])
            finally:
                reset()
        else:
            right = run.layer_off(["sequence", "call"])
            ahead = run.layer_off(["call", "sequence"])
    finally:
        if o["post"]:
            o["post"](L, d)
    differs = not _same(right[0], ahead[0]) if right[0] and not setter else not _same(right[0] + right[1], ahead[0] + ahead[1])
    print(cid, "counters", counters_on, counters_fl, "ahead differs", differs)
    assert differs, "the case cannot see a call that ran ahead of the record: what it compares does not depend on the order"
    assert counters_fl == whole, ("with tlab_deferred_flush() in front", counters_fl)
    assert _same(wrote_on, wrote_fl), "the call did not see the recorded substep executed: what it wrote differs from the run with tlab_deferred_flush() in front"
    assert _same(fields_on, fields_fl), "q, s, hq, hs differ from the run with tlab_deferred_flush() in front"
    assert counters_on == whole, ("the record was not run as one whole fused substep", counters_on)
