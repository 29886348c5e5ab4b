"""CPU test: the exact (return code, tlab_last_error() text) of refused calls, entry point by entry point, over the raw C ABI.

Every row is an argument refusal that is decided before the first HIP call, so it answers the same with and without a device: TLAB_EINVAL or
TLAB_EUNSUPPORTED only (a refusal "tlab_init has not been called" is TLAB_EHIP here and something else on a machine with a GPU: those refusals are in
tests/test_gpu_refusals.py).  One row at least for every public entry point of csrc/runtime.cpp, fdm_plan.cpp, operators.cpp, filter.hip,
filter_stream.hip, poisson*.hip, pointwise.hip and comm.hip (libtlab_amd_comm.so) that has such a refusal, and one more for every other kind of
failure such an entry point can meet before a HIP call (an unsupported scheme, a std::runtime_error of a helper file).  The expected values are read
off include/tlab_amd.h and the sources.  text None: the entry point answers with a value and leaves the error string alone."""
import ctypes

import numpy as np
import pytest

from tlab_amd import comm as C
from tlab_amd import lib as L

EINVAL, EUNSUPPORTED = -1, -2
P = ctypes.c_void_p
X = 8       # a pointer that is not null and that a refused call never follows


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class Plans:
    """The plans the rows need, made once: per64 periodic uniform, wall32 non-periodic uniform, arr16 from (zero) arrays, without a Jacobian."""

    def __init__(self, lib):
        self.out = P()
        self.per64 = self._create(lib, np.arange(64) / 64.0, 1)
        self.wall32 = self._create(lib, np.arange(32) / 31.0, 0)
        z = np.zeros(16 * 8)
        h = P()
        assert lib.tlab_fdm_plan_create_from_arrays(ctypes.byref(h), 16, 1, 0, 3, 3, _dp(z), _dp(z), 3, 5, _dp(z), _dp(z)) == 0
        self.arr16 = h.value
        self.nodes = np.arange(64) / 64.0
        self.stretched = np.arange(32, dtype=np.float64) ** 1.5
        self.f = np.zeros(64)
        self.start_bad = (ctypes.c_int * 3)(0, 5, 3)
        self.base = (ctypes.c_longlong * 3)(0, 0, 0)

    @staticmethod
    def _create(lib, nodes, periodic):
        h = P()
        assert lib.tlab_fdm_plan_create(ctypes.byref(h), nodes.size, _dp(nodes), periodic, 1, 6, 6, 0.0) == 0
        return h.value


@pytest.fixture(scope="module")
def env():
    lib = L.load()
    return lib, C.load(), Plans(lib)


NULLP = ctypes.POINTER(P)()
NULLD = ctypes.POINTER(ctypes.c_double)()
NULLI = ctypes.POINTER(ctypes.c_int)()
BAD_ARRAYS = "tlab_fdm_plan_create_from_arrays: bad arguments"
DIRECT1 = "direct first derivative: non-periodic direction, tridiagonal LHS, 3 or 5 RHS diagonals (FDM_C1N4_Direct / FDM_C1N6_Direct)"
FILTER_TYPES = ("filter type: compact (1), explicit6 (2), explicit4 (3), compactcutoff (9) -- the spectral / Helmholtz types are 3-D filters, "
                "not OPR_FILTER_1D")

# (id, call(lib, comm, plans) -> return code, expected code, expected text)
ROWS = [
    # ---- csrc/fdm_plan.cpp
    ("fdm_plan_create:null", lambda l, c, p: l.tlab_fdm_plan_create(NULLP, 64, _dp(p.nodes), 1, 1, 6, 6, 0.0), EINVAL, "tlab_fdm_plan_create: bad arguments"),
    ("fdm_plan_create:n=3", lambda l, c, p: l.tlab_fdm_plan_create(ctypes.byref(p.out), 3, _dp(p.nodes), 1, 1, 6, 6, 0.0), EINVAL,
     "tlab_fdm_plan_create: a direction needs 1 or >= 8 points"),
    ("fdm_plan_create:periodic-stretched", lambda l, c, p: l.tlab_fdm_plan_create(ctypes.byref(p.out), 32, _dp(p.stretched), 1, 0, 6, 6, 0.0), EINVAL,
     "grid must be uniform in a periodic direction (fdm.f90:117-120)"),
    ("fdm_plan_create:scheme1=99", lambda l, c, p: l.tlab_fdm_plan_create(ctypes.byref(p.out), 64, _dp(p.nodes), 0, 1, 99, 6, 0.0), EUNSUPPORTED,
     "first-derivative scheme not supported (CompactJacobian4/6/6Penta only)"),
    ("fdm_plan_create:scheme2=99", lambda l, c, p: l.tlab_fdm_plan_create(ctypes.byref(p.out), 64, _dp(p.nodes), 0, 1, 6, 99, 0.0), EUNSUPPORTED,
     "second-derivative scheme not supported (CompactJacobian4/6/6Hyper only)"),
    ("fdm_plan_create_from_arrays:n=4", lambda l, c, p: l.tlab_fdm_plan_create_from_arrays(ctypes.byref(p.out), 4, 1, 0, 3, 3, _dp(p.f), _dp(p.f), 3, 5, _dp(p.f), _dp(p.f)),
     EINVAL, BAD_ARRAYS),
    ("fdm_plan_create_from_arrays:ndl1=4", lambda l, c, p: l.tlab_fdm_plan_create_from_arrays(ctypes.byref(p.out), 16, 1, 0, 4, 3, _dp(p.f), _dp(p.f), 3, 5, _dp(p.f), _dp(p.f)),
     EUNSUPPORTED, "LHS: 3 diagonals (first derivative: or 5 with 7 RHS diagonals, CompactJacobian6Penta)"),
    ("fdm_plan_create_from_arrays:ndr2=6", lambda l, c, p: l.tlab_fdm_plan_create_from_arrays(ctypes.byref(p.out), 16, 1, 0, 3, 3, _dp(p.f), _dp(p.f), 3, 6, _dp(p.f), _dp(p.f)),
     EUNSUPPORTED, "unsupported number of RHS diagonals"),
    ("fdm_plan_set_aux:null", lambda l, c, p: l.tlab_fdm_plan_set_aux(None, None, None, None, None), EINVAL, "tlab_fdm_plan_set_aux: null plan"),
    ("fdm_plan_set_scheme:null", lambda l, c, p: l.tlab_fdm_plan_set_scheme(None, 6, 6), EINVAL, "tlab_fdm_plan_set_scheme: null plan"),
    ("fdm_plan_set_scheme:direct1-periodic", lambda l, c, p: l.tlab_fdm_plan_set_scheme(p.per64, 16, 6), EINVAL, DIRECT1),
    ("fdm_plan_set_scheme:direct2-periodic", lambda l, c, p: l.tlab_fdm_plan_set_scheme(p.per64, 6, 16), EINVAL,
     "direct second derivative: non-periodic direction with 5 RHS diagonals"),
    ("fdm_plan_set_stagger:null", lambda l, c, p: l.tlab_fdm_plan_set_stagger(None, 1), EINVAL, "tlab_fdm_plan_set_stagger: null plan"),
    ("fdm_plan_set_stagger:mode=3", lambda l, c, p: l.tlab_fdm_plan_set_stagger(p.per64, 3), EINVAL,
     "tlab_fdm_plan_set_stagger: mode 0 off, 1 tables + interpolatory wavenumbers, 2 tables only"),
    ("fdm_plan_set_stagger:no-jacobian", lambda l, c, p: l.tlab_fdm_plan_set_stagger(p.arr16, 1), EINVAL,
     "tlab_fdm_plan_set_stagger: the plan has no Jacobian (tlab_fdm_plan_set_aux)"),
    ("fdm_plan_set_stagger:non-periodic", lambda l, c, p: l.tlab_fdm_plan_set_stagger(p.wall32, 1), EUNSUPPORTED,
     "staggered grid only along periodic directions (fdm.f90:239-246)"),
    ("fdm_plan_info:null", lambda l, c, p: l.tlab_fdm_plan_info(None, 0), EINVAL, None),
    ("fdm_plan_info:what=99", lambda l, c, p: l.tlab_fdm_plan_info(p.per64, 99), EINVAL, None),
    ("fdm_plan_get:null", lambda l, c, p: l.tlab_fdm_plan_get(None, 1, _dp(p.f), 64), EINVAL, None),
    ("fdm_plan_get:short-buffer", lambda l, c, p: l.tlab_fdm_plan_get(p.per64, 1, _dp(p.f), 1), EINVAL, None),
    ("debug_host_chunked_solve:null", lambda l, c, p: l.tlab_debug_host_chunked_solve(None, 1, 0, 4, _dp(p.f)), EINVAL, "bad arguments"),
    ("debug_host_chunked_solve:chunks=7", lambda l, c, p: l.tlab_debug_host_chunked_solve(p.per64, 1, 0, 7, _dp(p.f)), EINVAL,
     "chunked: n not divisible by the number of chunks"),      # a std::runtime_error of a helper file (chunked.cpp)
    # ---- csrc/operators.cpp: what check_common refuses before it asks for the device
    ("opr_partial:null-plan", lambda l, c, p: l.tlab_opr_partial(1, None, 1, 64, 1, 1, 0, X, 2 * X, None), EINVAL, "null plan"),
    ("opr_partial:dir=4", lambda l, c, p: l.tlab_opr_partial(4, p.per64, 1, 64, 1, 1, 0, X, 2 * X, None), EINVAL, "dir must be 1, 2 or 3"),
    ("opr_partial:nz=0", lambda l, c, p: l.tlab_opr_partial(1, p.per64, 1, 64, 1, 0, 0, X, 2 * X, None), EINVAL, "bad sizes"),
    ("opr_partial:int32", lambda l, c, p: l.tlab_opr_partial(1, p.per64, 1, 64, 65536, 1024, 0, X, 2 * X, None), EINVAL,
     "local field exceeds int32 indexing (reference limit, tlab_memory.f90:175)"),
    ("opr_partial:ibc=4", lambda l, c, p: l.tlab_opr_partial(1, p.per64, 1, 64, 1, 1, 4, X, 2 * X, None), EINVAL, "ibc must be 0..3"),
    ("opr_partial:plan-size", lambda l, c, p: l.tlab_opr_partial(1, p.per64, 1, 32, 1, 1, 0, X, 2 * X, None), EINVAL,
     "plan size does not match the field size along dir"),
    ("opr_burgers:null-plan", lambda l, c, p: l.tlab_opr_burgers(1, None, 1, 64, 1, 1, 0, 1.0, X, None, 2 * X, 3 * X, 0), EINVAL, "null plan"),
    ("opr_burgers_add:dir=0", lambda l, c, p: l.tlab_opr_burgers_add(0, p.per64, 64, 1, 1, 0, 1.0, X, 2 * X, 3 * X, None, None), EINVAL, "dir must be 1, 2 or 3"),
    ("opr_burgers_add_n:null-plan", lambda l, c, p: l.tlab_opr_burgers_add_n(1, None, 64, 1, 1, 0, 1, NULLD, NULLP, None, NULLP, None, None, 0), EINVAL, "null plan"),
    ("opr_gradient_final:plan-size", lambda l, c, p: l.tlab_opr_gradient_final(3, p.per64, 64, 1, 8, X, 2 * X, 3 * X, 1.0, 1.0, 0, None), EINVAL,
     "plan size does not match the field size along dir"),
    ("opr_partial_add:ibc=-1", lambda l, c, p: l.tlab_opr_partial_add(1, p.per64, 64, 1, 1, -1, X, None, 0.0, 2 * X, 0, None, None), EINVAL, "ibc must be 0..3"),
    ("boundary_bcs_neumann_y:null-plan", lambda l, c, p: l.tlab_boundary_bcs_neumann_y(None, 1, 8, 32, 1, X, 2 * X, 3 * X, 4 * X), EINVAL, "null plan"),
    ("transpose:aliased", lambda l, c, p: l.tlab_transpose(X, 4, 4, X), EINVAL, "tlab_transpose: bad arguments"),
    ("set_tuning:key=99", lambda l, c, p: l.tlab_set_tuning(99, 0), EINVAL, "tlab_set_tuning: unknown key"),
    ("set_tuning:lines=24", lambda l, c, p: l.tlab_set_tuning(3, 24), EINVAL, "tlab_set_tuning: unknown key"),
    ("opr_burgers_set_dealiasing:dir=0", lambda l, c, p: l.tlab_opr_burgers_set_dealiasing(0, None), EINVAL, "dir must be 1, 2 or 3"),
    # ---- csrc/filter.hip
    ("filter_create:null", lambda l, c, p: l.tlab_filter_create(NULLP, 1, 64, 1, 0, 0, 10, _dp(p.f)), EINVAL, "tlab_filter_create: null handle"),
    ("filter_create:tophat", lambda l, c, p: l.tlab_filter_create(ctypes.byref(p.out), 8, 64, 1, 0, 0, 0, NULLD), EUNSUPPORTED,
     "tophat filters (flt_tophat.f90) are not built on the device path"),
    ("filter_create:type=5", lambda l, c, p: l.tlab_filter_create(ctypes.byref(p.out), 5, 64, 1, 0, 0, 0, NULLD), EUNSUPPORTED, FILTER_TYPES),
    ("filter_create:size=4", lambda l, c, p: l.tlab_filter_create(ctypes.byref(p.out), 2, 4, 1, 0, 0, 0, NULLD), EINVAL, "tlab_filter_create: at least 8 points"),
    ("filter_create:no-coeffs", lambda l, c, p: l.tlab_filter_create(ctypes.byref(p.out), 1, 64, 1, 0, 0, 10, NULLD), EINVAL,
     "tlab_filter_create: f%coeffs with at least inb_filter columns (opr_filter.f90:121-139)"),
    ("opr_filter_1d:null", lambda l, c, p: l.tlab_opr_filter_1d(1, None, 64, 1, 1, X, 2 * X), EINVAL, "tlab_opr_filter_1d: bad arguments (out of place)"),
    ("opr_filter_1d:dir=4", lambda l, c, p: l.tlab_opr_filter_1d(4, X, 64, 1, 1, 2 * X, 3 * X), EINVAL, "tlab_opr_filter_1d: bad sizes"),
    ("opr_filter:in-place", lambda l, c, p: l.tlab_opr_filter(64, 1, 1, None, None, None, NULLI, X, X), EINVAL, "tlab_opr_filter: bad arguments"),
    # ---- csrc/poisson.hip (poisson_direct.hip, poisson_int1.hip, poisson_ode.hip have no entry points of their own)
    ("poisson_plan_create:null", lambda l, c, p: l.tlab_poisson_plan_create(ctypes.byref(p.out), None, None, None, 64, 32, 64), EINVAL,
     "tlab_poisson_plan_create: null argument"),
    ("poisson_plan_create_slab:null", lambda l, c, p: l.tlab_poisson_plan_create_slab(NULLP, p.per64, p.wall32, p.per64, 64, 32, 16, 64, 0, 4), EINVAL,
     "tlab_poisson_plan_create: null argument"),
    ("poisson_plan_create_pencil:nxl=0", lambda l, c, p: l.tlab_poisson_plan_create_pencil(ctypes.byref(p.out), p.per64, p.wall32, p.per64, 64, 32, 16, 64, 0, 0), EINVAL,
     "tlab_poisson_plan_create_pencil: bad decomposition"),
    ("poisson_plan_create_pencil:null", lambda l, c, p: l.tlab_poisson_plan_create_pencil(NULLP, p.per64, p.wall32, p.per64, 64, 32, 16, 64, 0, 8), EINVAL,
     "tlab_poisson_plan_create: null argument"),
    ("poisson_plan_create_direct:null-elliptic", lambda l, c, p: l.tlab_poisson_plan_create_direct(ctypes.byref(p.out), p.per64, p.wall32, p.per64, 64, 32, 64, None), EINVAL,
     "tlab_poisson_plan_create_direct: null elliptic plan"),
    ("poisson_plan_create_direct:null", lambda l, c, p: l.tlab_poisson_plan_create_direct(NULLP, p.per64, p.wall32, p.per64, 64, 32, 64, p.wall32), EINVAL,
     "tlab_poisson_plan_create: null argument"),
    ("poisson_plan_create_direct_decomposed:mode=2", lambda l, c, p: l.tlab_poisson_plan_create_direct_decomposed(ctypes.byref(p.out), p.per64, p.wall32, p.per64, 64, 32, 16,
                                                                                                                64, 2, 0, 4, p.wall32), EINVAL,
     "tlab_poisson_plan_create_direct_decomposed: bad arguments"),
    ("opr_poisson:null", lambda l, c, p: l.tlab_opr_poisson(None, 64, 32, 64, 3, X, 2 * X, 3 * X, 4 * X, 5 * X, None), EINVAL, "tlab_opr_poisson: null argument"),
    ("poisson_set_wall_planes:null", lambda l, c, p: l.tlab_poisson_set_wall_planes(None, X, 2 * X, 3 * X), EINVAL, "null argument"),
    ("poisson_fft_x:null", lambda l, c, p: l.tlab_poisson_fft_x(None, 1, X, 2 * X), EINVAL, "tlab_poisson_fft_x: bad arguments"),
    ("poisson_fft_x_packed:null", lambda l, c, p: l.tlab_poisson_fft_x_packed(None, 1, X, 2 * X, 1, X, X), EINVAL, "tlab_poisson_fft_x_packed: bad arguments"),
    ("poisson_fft_x_packed_final:null", lambda l, c, p: l.tlab_poisson_fft_x_packed_final(None, X, 2 * X, 3 * X, 1.0, 1.0, 0, 1, X, X), EINVAL,
     "tlab_poisson_fft_x_packed_final: bad arguments"),
    ("poisson_fft_z:null", lambda l, c, p: l.tlab_poisson_fft_z(None, 1, X, 2 * X), EINVAL, "tlab_poisson_fft_z: bad arguments"),
    ("poisson_ode:null", lambda l, c, p: l.tlab_poisson_ode(None, None, None, None), EINVAL, "tlab_poisson_ode: bad arguments"),
    ("opr_helmholtz:null", lambda l, c, p: l.tlab_opr_helmholtz(None, 64, 32, 64, 3, 1.0, X, 2 * X, 3 * X, 4 * X, 5 * X), EINVAL, "tlab_opr_helmholtz: null argument"),
    ("poisson_direct_ode:null", lambda l, c, p: l.tlab_poisson_direct_ode(None, 3, X, X), EINVAL, "tlab_poisson_direct_ode: bad arguments"),
    ("debug_int1_solve:ibc=3", lambda l, c, p: l.tlab_debug_int1_solve(p.wall32, 3, 0, 1, _dp(p.f), _dp(p.f), _dp(p.f), _dp(p.f), _dp(p.f)), EINVAL,
     "tlab_debug_int1_solve: bad arguments"),
    # ---- csrc/pointwise.hip
    ("pw_clip:lo>hi", lambda l, c, p: l.tlab_pw_clip(X, 1.0, 0.0, 8), EINVAL, "tlab_pw_clip: null array, n < 0, NaN bounds or lo > hi"),
    ("pencil_repack:9-peers", lambda l, c, p: l.tlab_pencil_repack(X, 2 * X, 33, 8, 4, 9, p.start_bad, 1), EINVAL, "tlab_pencil_repack: bad arguments (1..8 peers)"),
    ("pencil_repack_blocks:null", lambda l, c, p: l.tlab_pencil_repack_blocks(None, 2 * X, 33, 8, 4, 3, p.start_bad, p.base, 1), EINVAL,
     "tlab_pencil_repack_blocks: bad arguments (1..16 blocks, the first at kx = 0)"),
    ("pencil_repack_blocks:starts", lambda l, c, p: l.tlab_pencil_repack_blocks(X, 2 * X, 33, 8, 4, 3, p.start_bad, p.base, 1), EINVAL,
     "tlab_pencil_repack_blocks: block starts must increase within [0, nx/2+1]"),
    # ---- csrc/comm.hip (libtlab_amd_comm.so)
    ("comm_get_unique_id:null", lambda l, c, p: c.tlab_comm_get_unique_id(None), EINVAL, "tlab_comm_get_unique_id: null buffer"),
    ("comm_init:null", lambda l, c, p: c.tlab_comm_init(NULLP, X, 1, 0, 1, 1), EINVAL, "tlab_comm_init: null argument"),
    ("comm_info:null", lambda l, c, p: c.tlab_comm_info(None, 0), EINVAL, None),
    ("comm_allreduce_max:null", lambda l, c, p: c.tlab_comm_allreduce_max(None, X, 1), EINVAL, "tlab_comm_allreduce_max: bad arguments"),
    ("comm_slab_transport:null", lambda l, c, p: c.tlab_comm_slab_transport(None, X), EINVAL, "tlab_comm_slab_transport: null argument"),
    ("comm_pencil_transport:null", lambda l, c, p: c.tlab_comm_pencil_transport(None, X), EINVAL, "tlab_comm_pencil_transport: null argument"),
    ("trp_plan_create:null", lambda l, c, p: c.tlab_trp_plan_create(NULLP, None, 1, 8, 8, 1, 0, 1), EINVAL, "tlab_trp_plan_create: null argument"),
    ("trp_plan_info:null", lambda l, c, p: c.tlab_trp_plan_info(None, 0), EINVAL, None),
    ("trp_plan_set_wire:null", lambda l, c, p: c.tlab_trp_plan_set_wire(None, 1), EINVAL, "tlab_trp_plan_set_wire: null plan"),
    ("trp_pack:null", lambda l, c, p: c.tlab_trp_pack(None, 1, X, 2 * X), EINVAL, "tlab_trp_pack: bad arguments"),
    ("trp_unpack:null", lambda l, c, p: c.tlab_trp_unpack(None, 1, X, 2 * X), EINVAL, "tlab_trp_unpack: bad arguments"),
    ("trp_start:null", lambda l, c, p: c.tlab_trp_start(None, 1, X, 2 * X), EINVAL, "tlab_trp_start: bad arguments (in and out must differ)"),
    ("trp_exec:null", lambda l, c, p: c.tlab_trp_exec(None, 1, X, 2 * X), EINVAL, "tlab_trp_start: bad arguments (in and out must differ)"),
    ("trp_wait:null", lambda l, c, p: c.tlab_trp_wait(None), EINVAL, "tlab_trp_wait: null plan"),
]


@pytest.mark.parametrize("name,call,code,text", ROWS, ids=[r[0] for r in ROWS])
def test_refused_call_answers_with_its_code_and_text(env, name, call, code, text):
    lib, comm, plans = env
    # another refusal first, so that the text found afterwards is this call's
    other = lib.tlab_set_tuning(99, 0) if text != "tlab_set_tuning: unknown key" else lib.tlab_pw_clip(None, 0.0, 1.0, 1)
    assert other == EINVAL
    before = lib.tlab_last_error()
    assert call(lib, comm, plans) == code
    assert lib.tlab_last_error().decode() == (text if text is not None else before.decode())


def test_every_row_is_an_argument_refusal():
    assert len({r[0] for r in ROWS}) == len(ROWS)
    assert all(r[2] in (EINVAL, EUNSUPPORTED) for r in ROWS)
