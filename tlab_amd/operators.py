"""Host-side mirror of the reference's operator interface for the hot path (same names, argument order and
meaning as the Fortran module procedures), working on torch CUDA tensors whose storage is handed to the C ABI
as raw device pointers.  torch is plumbing here (HBM allocation, streams); all arithmetic is in the HIP kernels.

    OPR_Partial_X(type, nx, ny, nz, bcs, g, u, result, tmp1)        operators/opr_partial.f90:31
    OPR_Burgers_X(ivel, is, nx, ny, nz, bcs, s, u, result, tmp1, u_t) physics/opr_burgers.f90:190
    TLab_Transpose(a, nra, nca, ma, b, mb)                           utils/tlab_transpose.f90:14

Fields are flat fp64 tensors of nx*ny*nz elements, x fastest, exactly the reference's u(nx*ny*nz).
"""
import ctypes
import numpy as np

from .lib import load, check, TlabError, c_vp

# operators/opr_partial.f90:19-21, physics/opr_burgers.f90:29-30, base/tlab_constants.f90:63-66, fdm_derivative.f90:51-54
OPR_P1, OPR_P2, OPR_P2_P1 = 1, 2, 3
OPR_P1_INT_VP, OPR_P1_INT_PV, OPR_P0_INT_VP, OPR_P0_INT_PV = 5, 6, 7, 8      # interpolatory operators of the staggered pressure grid
OPR_B_SELF, OPR_B_U_IN = 0, 1
BCS_DD, BCS_ND, BCS_DN, BCS_NN = 0, 1, 2, 3
FDM_COM4_JACOBIAN, FDM_COM6_JACOBIAN_PENTA, FDM_COM6_JACOBIAN, FDM_COM6_JACOBIAN_HYPER = 4, 5, 6, 7
FDM_COM6_DIRECT, FDM_COM4_DIRECT = 16, 17

_initialised = False


def init(device=0):
    """tlab_init: selects the GPU.  Raises TlabError if no MI355X is visible."""
    global _initialised
    check(load().tlab_init(int(device)), "tlab_init")
    _initialised = True


def sync():
    check(load().tlab_sync(), "tlab_sync")


def _use_torch_stream():
    import torch
    load().tlab_set_stream(c_vp(torch.cuda.current_stream().cuda_stream))


def _ptr(t, n=None, name="tensor"):
    import torch
    if t is None:
        return c_vp(0)
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
        raise TlabError("%s must be a contiguous float64 CUDA tensor" % name)
    if n is not None and t.numel() < n:
        raise TlabError("%s has %d elements, needs %d" % (name, t.numel(), n))
    return c_vp(t.data_ptr())


class FdmPlan:
    """type(fdm_dt) (fdm/fdm.f90:14-29): compact-FDM plan of one direction, owned by the library.

    FdmPlan(nodes, periodic, uniform, ...) restates FDM_CreatePlan (fdm/fdm.f90:143-252).
    FdmPlan.from_arrays(...) takes the tables an unchanged Fortran host built in FDM_Initialize.
    hyper_bc1_ext: see include/tlab_amd.h (0.1 reproduces the flang-built reference)."""

    _KEYS = {"lhs1": (1, 5), "rhs1": (2, 7), "lu1": (3, None), "rhs_b1": (4, None), "rhs_t1": (5, None), "mwn1": (6, 1),
             "lhs2": (7, 5), "rhs2": (8, 12), "lu2": (9, None), "mwn2": (10, 1), "jac": (11, 3), "lu0i": (12, 5), "lu1i": (13, 5)}

    def __init__(self, nodes, periodic, uniform, scheme1=FDM_COM6_JACOBIAN, scheme2=FDM_COM6_JACOBIAN_HYPER,
                 hyper_bc1_ext=0.1, stagger=False):
        """stagger: [Staggering] StaggerHorizontalPressure (a periodic direction gets the interpolation tables and the interpolatory der1%mwn,
        fdm.f90:236-248); non-periodic directions ignore it, as the reference does."""
        nodes = np.ascontiguousarray(nodes, dtype=np.float64)
        self.size = int(nodes.shape[0])
        self.periodic = bool(periodic)
        self.uniform = bool(uniform)
        self._h = c_vp(0)
        check(load().tlab_fdm_plan_create(ctypes.byref(self._h), self.size,
                                          nodes.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(self.periodic),
                                          int(self.uniform), int(scheme1), int(scheme2), float(hyper_bc1_ext)),
              "tlab_fdm_plan_create")
        if stagger and self.periodic:
            self.set_stagger(1)

    def set_stagger(self, mode):
        """tlab_fdm_plan_set_stagger: 1 tables + interpolatory wavenumbers, 2 tables only (host-built plans), 0 off"""
        check(load().tlab_fdm_plan_set_stagger(self._h, int(mode)), "tlab_fdm_plan_set_stagger")

    @classmethod
    def from_arrays(cls, n, periodic, need_1der, lhs1, rhs1, lhs2, rhs2, ndl1=3):
        """lhs*/rhs*: numpy arrays [row, diagonal] (as oracle / golden files hold them); rhs2 includes the 3
        Jacobian-correction columns after its ndr2 diagonals.  ndl1 = 5 with 7 rhs1 diagonals: CompactJacobian6Penta."""
        self = cls.__new__(cls)
        self.size, self.periodic, self.uniform = int(n), bool(periodic), not bool(need_1der)
        self._h = c_vp(0)
        ndr1, ndr2 = rhs1.shape[1], rhs2.shape[1] - 3
        f = [np.asfortranarray(a, dtype=np.float64) for a in (lhs1[:, :ndl1], rhs1, lhs2[:, :3], rhs2)]
        dp = ctypes.POINTER(ctypes.c_double)
        check(load().tlab_fdm_plan_create_from_arrays(ctypes.byref(self._h), self.size, int(periodic), int(need_1der),
                                                      int(ndl1), ndr1, f[0].ctypes.data_as(dp), f[1].ctypes.data_as(dp),
                                                      3, ndr2, f[2].ctypes.data_as(dp), f[3].ctypes.data_as(dp)),
              "tlab_fdm_plan_create_from_arrays")
        return self

    @classmethod
    def from_tables(cls, tab, periodic=False, scheme1=FDM_COM6_JACOBIAN, scheme2=FDM_COM6_JACOBIAN_HYPER):
        """Everything a Fortran host hands over for one direction: tab = dict with ndr1, ndr2, need_1der, lhs1, rhs1, lhs2, rhs2, mwn1,
        mwn2, jac (as oracle/ref_lib.fdm_arrays / the golden files hold them), plus the mode_fdm of both derivatives
        (FDM_COM6_DIRECT = 16 as scheme2: per-row right-hand side, SpaceOrder2 = CompactDirect6)."""
        rhs1 = np.asarray(tab["rhs1"])[:, :int(tab["ndr1"])]
        rhs2 = np.asarray(tab["rhs2"])[:, :int(tab["ndr2"]) + 3]
        self = cls.from_arrays(np.asarray(tab["lhs1"]).shape[0], periodic, int(tab["need_1der"]), np.asarray(tab["lhs1"]), rhs1,
                               np.asarray(tab["lhs2"]), rhs2)
        dp = ctypes.POINTER(ctypes.c_double)
        aux = [np.ascontiguousarray(tab[k], dtype=np.float64) if k in tab else None for k in ("mwn1", "mwn2")]
        jac = np.asfortranarray(tab["jac"], dtype=np.float64) if "jac" in tab else None
        nodes = np.ascontiguousarray(tab["nodes"], dtype=np.float64) if "nodes" in tab else None
        ptr = lambda a: a.ctypes.data_as(dp) if a is not None else None      # noqa: E731
        check(load().tlab_fdm_plan_set_aux(self._h, ctypes.cast(ptr(aux[0]), c_vp), ctypes.cast(ptr(aux[1]), c_vp),
                                           ctypes.cast(ptr(jac), c_vp), ctypes.cast(ptr(nodes), c_vp)), "tlab_fdm_plan_set_aux")
        check(load().tlab_fdm_plan_set_scheme(self._h, int(scheme1), int(scheme2)), "tlab_fdm_plan_set_scheme")
        return self

    def info(self, what):
        return load().tlab_fdm_plan_info(self._h, what)

    @property
    def need_1der(self):
        return bool(self.info(5))

    def table(self, key):
        """Plan table as a numpy array indexed [row, diagonal] like the oracle's."""
        which, cols = self._KEYS[key]
        n = self.size
        buf = np.zeros(n * 24 + 64)
        m = load().tlab_fdm_plan_get(self._h, which, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), buf.shape[0])
        if m < 0:
            raise TlabError("tlab_fdm_plan_get(%s) failed" % key)
        if key == "rhs_b1":
            return buf[:m].reshape(8, 4).T.copy()
        if key == "rhs_t1":
            return buf[:m].reshape(7, 5).T.copy()
        if cols == 1:
            return buf[:m].copy()
        return buf[:m].reshape(m // n, n).T.copy()

    def debug_host_chunked_solve(self, which, ibc, chunks, f):
        f = np.ascontiguousarray(f, dtype=np.float64).copy()
        check(load().tlab_debug_host_chunked_solve(self._h, which, ibc, chunks, f.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
              "tlab_debug_host_chunked_solve")
        return f

    def __del__(self):
        try:
            if self._h:
                load().tlab_fdm_plan_destroy(self._h)
        except Exception:
            pass


def _ibc(bcs):
    """ibc = bcs(1,1) + 2*bcs(2,1) (opr_partial.f90:91); bcs is the reference's 2x2 integer array (or an int ibc)."""
    if isinstance(bcs, (int, np.integer)):
        return int(bcs)
    b = np.asarray(bcs)
    return int(b[0, 0]) + 2 * int(b[1, 0])


def _partial(idir, type, nx, ny, nz, bcs, g, u, result, tmp1=None):
    n = nx * ny * nz
    _use_torch_stream()
    check(load().tlab_opr_partial(idir, g._h, int(type), nx, ny, nz, _ibc(bcs), _ptr(u, n, "u"), _ptr(result, n, "result"),
                                  _ptr(tmp1, n, "tmp1")), "tlab_opr_partial")


def OPR_Partial_X(type, nx, ny, nz, bcs, g, u, result, tmp1=None):
    _partial(1, type, nx, ny, nz, bcs, g, u, result, tmp1)


def OPR_Partial_Y(type, nx, ny, nz, bcs, g, u, result, tmp1=None):
    _partial(2, type, nx, ny, nz, bcs, g, u, result, tmp1)


def OPR_Partial_Z(type, nx, ny, nz, bcs, g, u, result, tmp1=None):
    _partial(3, type, nx, ny, nz, bcs, g, u, result, tmp1)


def BOUNDARY_BCS_NEUMANN_Y(ibc, nx, ny, nz, g, u, bcs_hb, bcs_ht, tmp1):
    """tools/dns/boundary_bcs.f90:368: wall planes (nx*nz) of u such that du/dy = 0 at jmin (ibc=1), jmax (2) or both (3)."""
    n = nx * ny * nz
    _use_torch_stream()
    check(load().tlab_boundary_bcs_neumann_y(g._h, int(ibc), nx, ny, nz, _ptr(u, n, "u"), _ptr(bcs_hb, nx * nz, "bcs_hb"),
                                             _ptr(bcs_ht, nx * nz, "bcs_ht"), _ptr(tmp1, n, "tmp1")), "tlab_boundary_bcs_neumann_y")


def _burgers(idir, ivel, nu, nx, ny, nz, bcs, g, s, u, result, tmp1, write_transposed):
    n = nx * ny * nz
    b = np.asarray(bcs) if not isinstance(bcs, (int, np.integer)) else None
    if b is not None and b.shape == (2, 2) and int(b[0, 1]) + int(b[1, 1]) > 0:
        raise TlabError("OPR_Burgers: only developed for biased BCs (opr_burgers.f90:460-463)")
    _use_torch_stream()
    check(load().tlab_opr_burgers(idir, g._h, int(ivel), nx, ny, nz, _ibc(bcs), float(nu), _ptr(s, n, "s"), _ptr(u, n, "u"),
                                  _ptr(result, n, "result"), _ptr(tmp1, n, "tmp1"), int(write_transposed)),
          "tlab_opr_burgers")


# `is` (scalar index selecting the diffusivity in the reference's module state) becomes the diffusivity itself:
# nu = visc for is = 0, visc/schmidt(is) otherwise (opr_burgers.f90:94-98).  u_t is accepted and ignored (see tlab_amd.h).
def OPR_Burgers_X(ivel, nu, nx, ny, nz, bcs, g, s, u, result, tmp1, u_t=None, write_transposed=False):
    _burgers(1, ivel, nu, nx, ny, nz, bcs, g, s, u, result, tmp1, write_transposed)


def OPR_Burgers_Y(ivel, nu, nx, ny, nz, bcs, g, s, u, result, tmp1, u_t=None, write_transposed=False):
    _burgers(2, ivel, nu, nx, ny, nz, bcs, g, s, u, result, tmp1, write_transposed)


def OPR_Burgers_Z(ivel, nu, nx, ny, nz, bcs, g, s, u, result, tmp1, u_t=None, write_transposed=False):
    _burgers(3, ivel, nu, nx, ny, nz, bcs, g, s, u, result, tmp1, write_transposed)


class Filter:
    """type(filter_dt) of operators/opr_filter.f90:28-41 with the coefficient table OPR_FILTER_INITIALIZE made on the host: ftype = 1 compact,
    2 explicit6, 3 explicit4, 9 compactcutoff; coeffs: numpy [row, column] (n, inb_filter) or None (explicit6); bcsmin / bcsmax: DNS_FILTER_BCS_*
    (filters/flt_base.f90: 1 biased, 2 free, 6 zero ...)."""

    def __init__(self, ftype, n, periodic, coeffs=None, bcsmin=1, bcsmax=1):
        self.type, self.size, self.periodic = int(ftype), int(n), bool(periodic)
        self._h = c_vp(0)
        dp = ctypes.POINTER(ctypes.c_double)
        if coeffs is None:
            nc, ptr = 0, None
        else:
            self._c = np.asfortranarray(coeffs, dtype=np.float64)
            nc, ptr = self._c.shape[1], self._c.ctypes.data_as(dp)
        check(load().tlab_filter_create(ctypes.byref(self._h), self.type, self.size, int(self.periodic), 0 if periodic else int(bcsmin),
                                        0 if periodic else int(bcsmax), nc, ptr), "tlab_filter_create")

    def __del__(self):
        try:
            if self._h:
                load().tlab_filter_destroy(self._h)
        except Exception:
            pass


def OPR_FILTER_1D(idir, f, nx, ny, nz, u, result):
    """OPR_FILTER_1D (opr_filter.f90:393-460) along direction idir of a field, out of place."""
    _use_torch_stream()
    check(load().tlab_opr_filter_1d(int(idir), f._h, nx, ny, nz, _ptr(u), _ptr(result)), "tlab_opr_filter_1d")


def OPR_FILTER(nx, ny, nz, fx, fy, fz, u, tmp, repeat=None):
    """OPR_FILTER (opr_filter.f90:283-392), directional branch: the x, then the y, then the z Filter (None = DNS_FILTER_NONE), each repeat[d]
    times (None: once), on u in place; tmp: scratch of the same size."""
    _use_torch_stream()
    n = int(nx) * int(ny) * int(nz)
    rp = None if repeat is None else (ctypes.c_int * 3)(*(int(r) for r in repeat))
    h = [f._h if f is not None else None for f in (fx, fy, fz)]
    check(load().tlab_opr_filter(nx, ny, nz, h[0], h[1], h[2], rp, _ptr(u, n, "u"), _ptr(tmp, n, "tmp")), "tlab_opr_filter")


def OPR_FILTER_FIELDS(nx, ny, nz, fx, fy, fz, fields, repeat=None):
    """OPR_FILTER's directional branch on every tensor of `fields` at once, in place and without a tmp (tlab_opr_filter_fields: the streaming
    kernels).  Every word of a result equals OPR_FILTER's on the same field."""
    _use_torch_stream()
    n = int(nx) * int(ny) * int(nz)
    fields = list(fields)
    rp = None if repeat is None else (ctypes.c_int * 3)(*(int(r) for r in repeat))
    h = [f._h if f is not None else None for f in (fx, fy, fz)]
    u = (c_vp * max(len(fields), 1))(*(_ptr(t, n, "field %d" % i) for i, t in enumerate(fields)))
    check(load().tlab_opr_filter_fields(nx, ny, nz, h[0], h[1], h[2], rp, len(fields), u), "tlab_opr_filter_fields")


def set_dealiasing(idir, f):
    """Dealiasing(idir) of OPR_Burgers ([Dealiasing], opr_burgers.f90:33, 71): a Filter, or None for DNS_FILTER_NONE.  Module state of the
    operator, as in the reference; the caller keeps the Filter alive while it is set."""
    check(load().tlab_opr_burgers_set_dealiasing(int(idir), f._h if f is not None else None), "tlab_opr_burgers_set_dealiasing")


class PoissonPlan:
    """Module state of OPR_Elliptic (operators/opr_elliptic.f90:64-81) + OPR_Fourier plans, built by
    OPR_Elliptic_Initialize / OPR_Fourier_Initialize in the reference; here one object owned by the library."""

    def __init__(self, gx, gy, gz, nx, ny, nz, gy_elliptic=None):
        """gy_elliptic: the reference's fdm_loc of EllipticOrder = CompactDirect6 (a y plan with the direct second derivative and its nodes,
        FdmPlan.from_tables) -> OPR_Poisson_FourierXZ_Direct; None -> the factorized solver built from gy%der1."""
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.isize_txc_field = (self.nx + 2) * self.ny * self.nz     # base/tlab_memory.f90:186-187
        self._keep = (gx, gy, gz, gy_elliptic)
        self._h = c_vp(0)
        self.direct = gy_elliptic is not None
        if self.direct:
            check(load().tlab_poisson_plan_create_direct(ctypes.byref(self._h), gx._h, gy._h, gz._h, self.nx, self.ny, self.nz, gy_elliptic._h),
                  "tlab_poisson_plan_create_direct")
        else:
            check(load().tlab_poisson_plan_create(ctypes.byref(self._h), gx._h, gy._h, gz._h, self.nx, self.ny, self.nz),
                  "tlab_poisson_plan_create")

    def __del__(self):
        try:
            if self._h:
                load().tlab_poisson_plan_destroy(self._h)
        except Exception:
            pass


def OPR_Poisson(plan, nx, ny, nz, ibc, p, tmp1, tmp2, bcs_hb, bcs_ht, dpdy=None):
    """OPR_Poisson(nx, ny, nz, ibc, p, tmp1, tmp2, bcs_hb, bcs_ht, dpdy)  operators/opr_elliptic.f90:33-46.
    `plan` replaces the reference's module state.  tmp1, tmp2 need (nx+2)*ny*nz elements."""
    n = nx * ny * nz
    _use_torch_stream()
    check(load().tlab_opr_poisson(plan._h, nx, ny, nz, int(ibc), _ptr(p, n, "p"), _ptr(tmp1, plan.isize_txc_field, "tmp1"),
                                  _ptr(tmp2, plan.isize_txc_field, "tmp2"), _ptr(bcs_hb, nx * nz, "bcs_hb"),
                                  _ptr(bcs_ht, nx * nz, "bcs_ht"), _ptr(dpdy, n, "dpdy")), "tlab_opr_poisson")


def poisson_set_exact(on):
    """Factorized Poisson plans created after this call use the marching per-mode solver that repeats the reference's operations one by one
    (bit-faithful up to the FFTs, 2x the time of the per-mode stage) instead of the register-chunked one; include/tlab_amd.h."""
    check(load().tlab_poisson_set_exact(int(bool(on))), "tlab_poisson_set_exact")


def OPR_Helmholtz(plan, nx, ny, nz, ibc, alpha, a, tmp1, tmp2, bcs_hb, bcs_ht):
    """OPR_Helmholtz(nx, ny, nz, ibc, alpha, a, tmp1, tmp2, bcs_hb, bcs_ht)  operators/opr_elliptic.f90:48-62: lap a + alpha a = f.
    Direct plan (PoissonPlan(..., gy_elliptic=...)): OPR_Helmholtz_FourierXZ_Direct :562-628, any boundary type; factorized plan:
    OPR_Helmholtz_FourierXZ_Factorize :466-557, BCS_NN or BCS_DD (the tables of an alpha are built on its first call)."""
    n = nx * ny * nz
    _use_torch_stream()
    check(load().tlab_opr_helmholtz(plan._h, nx, ny, nz, int(ibc), float(alpha), _ptr(a, n, "a"), _ptr(tmp1, plan.isize_txc_field, "tmp1"),
                                    _ptr(tmp2, plan.isize_txc_field, "tmp2"), _ptr(bcs_hb, nx * nz, "bcs_hb"), _ptr(bcs_ht, nx * nz, "bcs_ht")),
          "tlab_opr_helmholtz")


def TLab_Transpose(a, nra, nca, b):
    """b(nca, nra) = transpose of Fortran a(nra, nca); bit-exact."""
    _use_torch_stream()
    check(load().tlab_transpose(_ptr(a, nra * nca, "a"), nra, nca, _ptr(b, nra * nca, "b")), "tlab_transpose")


# ---- plane statistics: module Averages and the covariance blocks of AVG_FLOW_XZ / AVG_SCAL_XZ (include/tlab_amd.h) ----------------------------
FLOW_MOMENTS = ("Rxx", "Ryy", "Rzz", "Rxy", "Rxz", "Ryz", "rU3", "rU4", "rV3", "rV4", "rW3", "rW4", "Txxy", "Tyyy", "Tzzy", "Txyy", "Txzy", "Tyzy")
FLOW_MOMENTS_P = ("rP2", "up", "vp", "wp")          # <p'p'>, <u'p'>, <v'p'> (Ty2), <w'p'>
SCAL_MOMENTS = ("rS2", "rS3", "rS4", "Rsu", "Rsv", "Rsw", "Tssy1", "Tsuy1", "Tsvy1", "Tswy1")
SCAL_MOMENTS_P = ("Tsvy3",)


def _field_ptr(a, n, name, keep):
    """the address of a field of n float64: a contiguous torch tensor (device or host) or a numpy array; None -> NULL"""
    if a is None:
        return c_vp(0)
    if isinstance(a, np.ndarray):
        if a.dtype != np.float64 or not a.flags.c_contiguous or a.size < n:
            raise TlabError("%s must be a contiguous float64 array of at least %d elements" % (name, n))
        keep.append(a)
        return c_vp(a.ctypes.data)
    import torch
    if not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or not a.is_contiguous() or a.numel() < n:
        raise TlabError("%s must be a contiguous float64 tensor of at least %d elements" % (name, n))
    keep.append(a)
    return c_vp(a.data_ptr())


def _profile(a, ny, name, keep):
    if a is None:
        return c_vp(0)
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (ny,):
        raise TlabError("%s must hold ny = %d values" % (name, ny))
    keep.append(a)
    return c_vp(a.ctypes.data)


def _stream_if_device(fields):
    if any(f is not None and not isinstance(f, np.ndarray) and f.is_cuda for f in fields):
        _use_torch_stream()


def avg_ik_v(nx, ny, nz, fields):
    """AVG_IK_V (utils/averages.f90:301) of several fields in one pass: numpy (len(fields), ny).  fields: torch tensors or numpy arrays."""
    keep, n = [], nx * ny * nz
    fields = list(fields)
    ptrs = (c_vp * max(len(fields), 1))(*[_field_ptr(f, n, "field %d" % i, keep).value for i, f in enumerate(fields)])
    out = np.zeros((max(len(fields), 1), ny))
    _stream_if_device(fields)
    check(load().tlab_avg_ik_v(nx, ny, nz, len(fields), ptrs, c_vp(out.ctypes.data), ny), "tlab_avg_ik_v")
    return out[:len(fields)]


def avg1v2d_v(nx, ny, nz, imom, a):
    """AVG1V2D_V (utils/averages.f90:142): the plane average of a**imom, numpy (ny,)."""
    keep = []
    out = np.zeros(ny)
    _stream_if_device([a])
    check(load().tlab_avg1v2d_v(nx, ny, nz, int(imom), _field_ptr(a, nx * ny * nz, "a", keep), c_vp(out.ctypes.data)), "tlab_avg1v2d_v")
    return out


def avg_moments_flow(nx, ny, nz, u, v, w, fU, fV, fW, p=None, rP=None):
    """The covariances of AVG_FLOW_XZ that need no derivative: numpy (18 or 22, ny), rows in the order of FLOW_MOMENTS (+ FLOW_MOMENTS_P)."""
    keep, n = [], nx * ny * nz
    out = np.zeros((22 if p is not None else 18, ny))
    _stream_if_device([u, v, w, p])
    check(load().tlab_avg_moments_flow(nx, ny, nz, _field_ptr(u, n, "u", keep), _field_ptr(v, n, "v", keep), _field_ptr(w, n, "w", keep),
                                       _field_ptr(p, n, "p", keep), _profile(fU, ny, "fU", keep), _profile(fV, ny, "fV", keep),
                                       _profile(fW, ny, "fW", keep), _profile(rP, ny, "rP", keep), c_vp(out.ctypes.data), ny),
          "tlab_avg_moments_flow")
    return out


def avg_moments_scal(nx, ny, nz, s, u, v, w, fS, fU, fV, fW, p=None, rP=None):
    """The moments and fluxes of one scalar in AVG_SCAL_XZ: numpy (10 or 11, ny), rows in the order of SCAL_MOMENTS (+ SCAL_MOMENTS_P)."""
    keep, n = [], nx * ny * nz
    out = np.zeros((11 if p is not None else 10, ny))
    _stream_if_device([s, u, v, w, p])
    check(load().tlab_avg_moments_scal(nx, ny, nz, _field_ptr(s, n, "s", keep), _field_ptr(u, n, "u", keep), _field_ptr(v, n, "v", keep),
                                       _field_ptr(w, n, "w", keep), _field_ptr(p, n, "p", keep), _profile(fS, ny, "fS", keep),
                                       _profile(fU, ny, "fU", keep), _profile(fV, ny, "fV", keep), _profile(fW, ny, "fW", keep),
                                       _profile(rP, ny, "rP", keep), c_vp(out.ctypes.data), ny), "tlab_avg_moments_scal")
    return out


# ---- ... and the groups on the velocity and scalar gradients (Section 3 of AVG_FLOW_XZ; include/tlab_amd.h lists the terms) --------------------
def _chains(names):
    return tuple("%s%d" % (n, k) for n in names for k in (2, 3, 4))


FLOW_GRADIENTS = (("vortx", "vorty", "vortz", "Tau_yy", "Tau_xy", "Tau_yz") + _chains(("U_x", "V_y", "W_z", "U_y", "U_z", "V_x", "V_z", "W_x", "W_y"))
                  + ("U_ii2", "vortx2", "vorty2", "vortz2", "Phi", "Exx", "Eyy", "Ezz", "Exy", "Exz", "Eyz")
                  + ("Txxy_v", "Tyyy_v", "Tzzy_v", "Txyy_v", "Txzy_v", "Tyzy_v"))
FLOW_GRADIENTS_P = ("PIxx", "PIyy", "PIzz", "PIxy", "PIxz", "PIyz")
SCAL_GRADIENTS = ("Fy", "Ess", "S_x2", "S_y2", "S_z2", "S_x3", "S_y3", "S_z3", "S_x4", "S_y4", "S_z4", "Tssy2", "Tsuy2_d", "Tsvy2_d", "Tswy2_d")
SCAL_GRADIENTS_P = ("PIsu", "PIsv", "PIsw")


def avg_gradients_flow(nx, ny, nz, grad, u, v, w, fU, fV, fW, rU_y, rV_y, rW_y, p=None, rP=None):
    """The groups of AVG_FLOW_XZ on the nine velocity derivatives grad = (dudx, dudy, dudz, dvdx, .., dwdz): numpy (50 or 56, ny), rows in the
    order of FLOW_GRADIENTS (+ FLOW_GRADIENTS_P), raw (before the visc, c23 and 2.0 of the reference's host lines)."""
    keep, n = [], nx * ny * nz
    grad = list(grad)
    if len(grad) != 9:
        raise TlabError("grad must hold the nine velocity derivatives")
    ptrs = (c_vp * 9)(*[_field_ptr(g, n, "grad %d" % i, keep).value for i, g in enumerate(grad)])
    out = np.zeros((56 if p is not None else 50, ny))
    _stream_if_device(grad + [u, v, w, p])
    check(load().tlab_avg_gradients_flow(nx, ny, nz, ptrs, _field_ptr(u, n, "u", keep), _field_ptr(v, n, "v", keep), _field_ptr(w, n, "w", keep),
                                         _field_ptr(p, n, "p", keep), _profile(fU, ny, "fU", keep), _profile(fV, ny, "fV", keep),
                                         _profile(fW, ny, "fW", keep), _profile(rP, ny, "rP", keep), _profile(rU_y, ny, "rU_y", keep),
                                         _profile(rV_y, ny, "rV_y", keep), _profile(rW_y, ny, "rW_y", keep), c_vp(out.ctypes.data), ny),
          "tlab_avg_gradients_flow")
    return out


def avg_ugradp(nx, ny, nz, u, v, w, dpdx, dpdy, dpdz):
    """The plane average of u*dpdx + v*dpdy + w*dpdz (avg_flow_xz.f90:673), numpy (ny,)."""
    keep, n = [], nx * ny * nz
    out = np.zeros(ny)
    fields = [u, v, w, dpdx, dpdy, dpdz]
    _stream_if_device(fields)
    check(load().tlab_avg_ugradp(nx, ny, nz, *[_field_ptr(f, n, "field %d" % i, keep) for i, f in enumerate(fields)], c_vp(out.ctypes.data)),
          "tlab_avg_ugradp")
    return out


def avg_gradients_scal(nx, ny, nz, grads, s, u, v, w, fS, fU, fV, fW, rS_y, p=None, rP=None, fS_y=None):
    """The groups of AVG_SCAL_XZ on grads = (dsdx, dsdy, dsdz): numpy (15 or 18, ny), rows in the order of SCAL_GRADIENTS (+ SCAL_GRADIENTS_P),
    raw.  With p also rP and fS_y."""
    keep, n = [], nx * ny * nz
    grads = list(grads)
    if len(grads) != 3:
        raise TlabError("grads must hold dsdx, dsdy, dsdz")
    ptrs = (c_vp * 3)(*[_field_ptr(g, n, "grads %d" % i, keep).value for i, g in enumerate(grads)])
    out = np.zeros((18 if p is not None else 15, ny))
    _stream_if_device(grads + [s, u, v, w, p])
    check(load().tlab_avg_gradients_scal(nx, ny, nz, ptrs, _field_ptr(s, n, "s", keep), _field_ptr(u, n, "u", keep), _field_ptr(v, n, "v", keep),
                                         _field_ptr(w, n, "w", keep), _field_ptr(p, n, "p", keep), _profile(fS, ny, "fS", keep),
                                         _profile(fU, ny, "fU", keep), _profile(fV, ny, "fV", keep), _profile(fW, ny, "fW", keep),
                                         _profile(rP, ny, "rP", keep), _profile(rS_y, ny, "rS_y", keep), _profile(fS_y, ny, "fS_y", keep),
                                         c_vp(out.ctypes.data), ny), "tlab_avg_gradients_scal")
    return out


# ---- plane PDFs: module PDFS and PDF1V_N / PDF2V (include/tlab_amd.h) --------------------------------------------------------------------------
def _gate_ptr(gate, n, keep):
    """the address of an int8 gate of n points: a contiguous torch tensor (device or host) or a numpy array; None -> NULL"""
    if gate is None:
        return c_vp(0)
    if isinstance(gate, np.ndarray):
        if gate.dtype != np.int8 or not gate.flags.c_contiguous or gate.size < n:
            raise TlabError("gate must be a contiguous int8 array of at least %d elements" % n)
        keep.append(gate)
        return c_vp(gate.ctypes.data)
    import torch
    if not isinstance(gate, torch.Tensor) or gate.dtype != torch.int8 or not gate.is_contiguous() or gate.numel() < n:
        raise TlabError("gate must be a contiguous int8 tensor of at least %d elements" % n)
    keep.append(gate)
    return c_vp(gate.data_ptr())


def _field_ptrs(fields, n, keep):
    return (c_vp * max(len(fields), 1))(*[_field_ptr(f, n, "field %d" % i, keep).value for i, f in enumerate(fields)])


def pdf1v_n(nx, ny, nz, fields, nbins, ibc, umin=None, umax=None, gate=None, igate=0):
    """The calculation of PDF1V_N (statistics/pdf.f90:14) for several fields in shared passes: numpy (nv, ny + 1, nbins + 2) -- nbins counts and
    the centres of the first and the last bin per plane, the volume as the last plane (zero when ny == 1).  ibc: one value or one per field
    (0: the external interval umin, umax of the field; 1: local; 2..5: local, PDF_ANALIZE(ibc - 2), then the analysed interval)."""
    fields = list(fields)
    nv, n, keep = len(fields), nx * ny * nz, []
    ibc_ = np.ascontiguousarray(np.broadcast_to(np.asarray(ibc, dtype=np.int32), (max(nv, 1),)))
    lo = None if umin is None else np.ascontiguousarray(np.broadcast_to(np.asarray(umin, dtype=np.float64), (max(nv, 1),)))
    hi = None if umax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(umax, dtype=np.float64), (max(nv, 1),)))
    out = np.zeros((max(nv, 1), ny + 1, max(int(nbins), 0) + 2))
    _stream_if_device(fields)
    check(load().tlab_pdf1v_n(nx, ny, nz, nv, int(nbins), c_vp(ibc_.ctypes.data), c_vp(lo.ctypes.data if lo is not None else 0),
                              c_vp(hi.ctypes.data if hi is not None else 0), _field_ptrs(fields, n, keep), int(igate), _gate_ptr(gate, n, keep),
                              c_vp(out.ctypes.data)), "tlab_pdf1v_n")
    return out[:nv]


def pdf_minmax_planes(nx, ny, nz, fields, gate=None, igate=0):
    """The min/max pass of pdf1v_n on its own: (umin, umax), numpy (nv, ny + 1) each, the volume's as the last plane."""
    fields = list(fields)
    nv, n, keep = len(fields), nx * ny * nz, []
    lo, hi = np.zeros((max(nv, 1), ny + 1)), np.zeros((max(nv, 1), ny + 1))
    _stream_if_device(fields)
    check(load().tlab_pdf_minmax_planes(nx, ny, nz, nv, _field_ptrs(fields, n, keep), int(igate), _gate_ptr(gate, n, keep), c_vp(lo.ctypes.data),
                                        c_vp(hi.ctypes.data)), "tlab_pdf_minmax_planes")
    return lo[:nv], hi[:nv]


def pdf_histogram_planes(nx, ny, nz, fields, nbins, ilim, umin, umax, gate=None, igate=0):
    """The histogram pass of pdf1v_n on its own, with the intervals of every plane handed in: umin, umax numpy (nv, ny + 1); ilim: one value or
    one per field, 0 = external intervals.  numpy (nv, ny + 1, nbins + 2)."""
    fields = list(fields)
    nv, n, keep = len(fields), nx * ny * nz, []
    ilim_ = np.ascontiguousarray(np.broadcast_to(np.asarray(ilim, dtype=np.int32), (max(nv, 1),)))
    lo, hi = (np.ascontiguousarray(a, dtype=np.float64) for a in (umin, umax))
    if lo.shape != (nv, ny + 1) or hi.shape != (nv, ny + 1):
        raise TlabError("umin and umax must have the shape (nv, ny + 1)")
    out = np.zeros((max(nv, 1), ny + 1, max(int(nbins), 0) + 2))
    _stream_if_device(fields)
    check(load().tlab_pdf_histogram_planes(nx, ny, nz, nv, int(nbins), c_vp(ilim_.ctypes.data), c_vp(lo.ctypes.data), c_vp(hi.ctypes.data),
                                           _field_ptrs(fields, n, keep), int(igate), _gate_ptr(gate, n, keep), c_vp(out.ctypes.data)),
          "tlab_pdf_histogram_planes")
    return out[:nv]


def pdf_analize(ibc, nbins, pdf, plim=1.0e-4):
    """PDF_ANALIZE (utils/pdfs.f90:329): (umin_ext, umax_ext, nplim) of one pdf(nbins + 2)."""
    pdf = np.ascontiguousarray(pdf, dtype=np.float64)
    if pdf.shape != (nbins + 2,):
        raise TlabError("pdf must hold nbins + 2 values")
    lo, hi, npl = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int(0)
    check(load().tlab_pdf_analize(int(ibc), int(nbins), c_vp(pdf.ctypes.data), ctypes.byref(lo), ctypes.byref(hi), float(plim), ctypes.byref(npl)),
          "tlab_pdf_analize")
    return lo.value, hi.value, npl.value


def pdf2v(nx, ny, nz, nbins, u, v):
    """The calculation of PDF2V (statistics/pdf.f90:123): numpy (ny + 1, nb1*nb2 + 2 + 2*nb1), bin (up, vp) at (vp-1)*nb1 + up, then the centres
    of the first and last u-bin and, per u-bin, of the first and last v-bin; the volume as the last plane (zero when ny == 1)."""
    keep, n = [], nx * ny * nz
    nb = np.ascontiguousarray(nbins, dtype=np.int32)
    if nb.shape != (2,):
        raise TlabError("nbins must hold two values")
    out = np.zeros((ny + 1, max(int(nb[0]) * int(nb[1]), 0) + 2 + 2 * max(int(nb[0]), 0)))
    _stream_if_device([u, v])
    check(load().tlab_pdf2v(nx, ny, nz, c_vp(nb.ctypes.data), _field_ptr(u, n, "u", keep), _field_ptr(v, n, "v", keep), c_vp(out.ctypes.data)),
          "tlab_pdf2v")
    return out


def gate_threshold(a, thr, gate=None):
    """gate = a > thr ? 1 : 0 as int8 (the gate of dns_statistics.f90:106-110), of the kind of a: a torch tensor or a numpy array."""
    keep = []
    if isinstance(a, np.ndarray):
        n = a.size
        gate = np.empty(n, dtype=np.int8) if gate is None else gate
    else:
        import torch
        n = a.numel()
        gate = torch.empty(n, dtype=torch.int8, device=a.device) if gate is None else gate
    _stream_if_device([a])
    check(load().tlab_gate_threshold(_field_ptr(a, n, "a", keep), n, float(thr), _gate_ptr(gate, n, keep)), "tlab_gate_threshold")
    return gate


# ---- intermittency: FI_VORTICITY and INTER_N_XZ, the block stats_intermittency of DNS_STATISTICS (dns_statistics.f90:99-117) -------------------
def fi_vorticity(dns, u, v, w, result, txc6):
    """FI_VORTICITY (mappings/fi_vorticity.f90:28) with the plans of the driver dns: result = (v,x - u,y)^2 + (u,z - w,x)^2 + (w,y - v,z)^2.
    txc6: six work tensors, which hold v,x  u,y  u,z  w,x  w,y  v,z on return.  Returns result."""
    txc6 = list(txc6)
    if len(txc6) != 6:
        raise TlabError("txc6 must hold six work arrays")
    ptrs = (c_vp * 6)(*[_ptr(t, dns.n, "txc6[%d]" % i).value for i, t in enumerate(txc6)])
    _use_torch_stream()
    check(load().tlab_fi_vorticity(dns._h, _ptr(u, dns.n, "u"), _ptr(v, dns.n, "v"), _ptr(w, dns.n, "w"), _ptr(result, dns.n, "result"), ptrs),
          "tlab_fi_vorticity")
    return result


def vorticity_from_gradients(vx, uy, uz, wx, wy, vz, result=None):
    """The pointwise pass of FI_VORTICITY on its own: ((vx - uy)^2 + (uz - wx)^2) + (wy - vz)^2, of the kind of its arguments (torch tensors or
    numpy arrays)."""
    keep, fields = [], [vx, uy, uz, wx, wy, vz]
    if isinstance(vx, np.ndarray):
        n = vx.size
        result = np.empty(n) if result is None else result
    else:
        import torch
        n = vx.numel()
        result = torch.empty_like(vx) if result is None else result
    _stream_if_device(fields)
    check(load().tlab_vorticity_from_gradients(n, *[_field_ptr(f, n, "field %d" % i, keep) for i, f in enumerate(fields)],
                                               _field_ptr(result, n, "result", keep)), "tlab_vorticity_from_gradients")
    return result


def inter_n_xz(nx, ny, nz, np_, gate):
    """The calculation of INTER_N_XZ (statistics/avg_xz.f90:109): the area fraction of the levels 1 .. np_ of an int8 gate in every plane, numpy
    (np_, ny) -- row ip - 1 is column ip of the reference's inter(ny, np).  gate: a torch tensor or a numpy array."""
    keep = []
    out = np.zeros((max(int(np_), 1), ny))
    _stream_if_device([gate])
    check(load().tlab_inter_n_xz(nx, ny, nz, int(np_), _gate_ptr(gate, nx * ny * nz, keep), c_vp(out.ctypes.data)), "tlab_inter_n_xz")
    return out


# ---- conditional statistics: FI_GATE's partition, AVG_N_XZ with a gate, CAVG1V_N / CAVG2V (csrc/tlab_amd_conditional.h) ------------------------
def _new_gate(a, gate):
    """(n, gate): an int8 gate of the kind of a (a torch tensor or a numpy array), a new one unless handed in"""
    if isinstance(a, np.ndarray):
        return a.size, (np.empty(a.size, dtype=np.int8) if gate is None else gate)
    import torch
    return a.numel(), (torch.empty(a.numel(), dtype=torch.int8, device=a.device) if gate is None else gate)


def gate_levels(a, thresholds, gate=None):
    """The loop of FI_GATE (mappings/fi_gate.f90:85-90): the first n with a < thresholds[n - 1], else len(thresholds) + 1, as int8 of the kind
    of a.  thresholds: ascending, absolute."""
    keep = []
    thr = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
    n, gate = _new_gate(a, gate)
    _stream_if_device([a])
    check(load().tlab_gate_levels(_field_ptr(a, n, "a", keep), n, thr.size + 1, c_vp(thr.ctypes.data if thr.size else 0), _gate_ptr(gate, n, keep)),
          "tlab_gate_levels")
    return gate


def gate_flux(a, v, gate=None):
    """The quadrant partition of FI_GATE (opt_cond = 7, fi_gate.f90:65-71) of the indicator a and the velocity v, as int8 of the kind of a."""
    keep = []
    n, gate = _new_gate(a, gate)
    _stream_if_device([a, v])
    check(load().tlab_gate_flux(_field_ptr(a, n, "a", keep), _field_ptr(v, n, "v", keep), n, _gate_ptr(gate, n, keep)), "tlab_gate_flux")
    return gate


def dns_gate(dns, opt_cond, thresholds, q, s, txc, relative=False, scal=1, gate=None):
    """FI_GATE (mappings/fi_gate.f90) for opt_cond 2 .. 7 on the box of the driver dns: an int8 tensor.  q, s, txc: lists of device tensors; the
    indicator goes into txc[0] (opt_cond 3: txc[1..6] are work arrays, 4: txc[1]); 2 and 5 read their field in place and need no txc."""
    import torch
    thr = np.ascontiguousarray(thresholds if thresholds is not None else [], dtype=np.float64).reshape(-1)
    gate = torch.empty(dns.n, dtype=torch.int8, device="cuda") if gate is None else gate
    arr = lambda ts: (c_vp * max(len(ts), 1))(*[_ptr(t, dns.n, "array %d" % i).value for i, t in enumerate(ts)])      # noqa: E731
    _use_torch_stream()
    check(load().tlab_dns_gate(dns._h, int(opt_cond), 1 if relative else 0, int(scal), thr.size + 1, c_vp(thr.ctypes.data if thr.size else 0),
                               arr(list(q)), arr(list(s)), arr(list(txc)), _gate_ptr(gate, dns.n, [])), "tlab_dns_gate")
    return gate


def avg_n_xz(nx, ny, nz, fields, nm, np_=0, gate=None, raw=False):
    """The calculation of AVG_N_XZ (statistics/avg_xz.f90:10) for the levels 1 .. np_ of an int8 gate in one pass (np_ = 0: ungated, one level):
    numpy (L, nv, nm, ny) with L = max(np_, 1) -- the mean and the central moments 2 .. nm of every field, level and plane.  raw: (avg, sums,
    nsample) with the undivided sums of a**m in the same shape and the counts (L, ny) as int64."""
    fields = list(fields)
    nv, n, keep, L = len(fields), nx * ny * nz, [], max(int(np_), 1)
    shape = (L, max(nv, 1), max(int(nm), 1), ny)
    avg, sums, ns = np.zeros(shape), np.zeros(shape), np.zeros((L, ny), dtype=np.int64)
    _stream_if_device(fields + [gate])
    check(load().tlab_avg_n_xz(nx, ny, nz, nv, int(nm), _field_ptrs(fields, n, keep), int(np_), _gate_ptr(gate, n, keep), c_vp(avg.ctypes.data),
                               c_vp(sums.ctypes.data if raw else 0), c_vp(ns.ctypes.data if raw else 0)), "tlab_avg_n_xz")
    return (avg, sums, ns) if raw else avg


def raw_to_central(moments):
    """RAW_TO_CENTRAL (statistics/avg_xz.f90:72): the raw moments 1 .. nm of one sample to its mean and central moments, a new numpy array."""
    m = np.array(moments, dtype=np.float64).reshape(-1)
    check(load().tlab_raw_to_central(m.size, c_vp(m.ctypes.data)), "tlab_raw_to_central")
    return m


def cavg1v_n(nx, ny, nz, fields, a, nbins, ibc=1, umin=None, umax=None, gate=None, igate=0, raw=False):
    """The calculation of CAVG1V_N (statistics/cavg.f90:7): numpy (nv, ny + 1, nbins + 2) -- per plane the averages of a over the nbins bins of
    every field, then the centres of the first and the last bin; the volume as the last plane (zero when ny == 1).  ibc: one value or one per
    field, 0: the external interval umin, umax of the field, anything else: the local one.  raw: (avg, sum, pdf) with the undivided sums of a
    and the counts in the same shape."""
    fields = list(fields)
    nv, n, keep = len(fields), nx * ny * nz, []
    ibc_ = np.ascontiguousarray(np.broadcast_to(np.asarray(ibc, dtype=np.int32), (max(nv, 1),)))
    lo = None if umin is None else np.ascontiguousarray(np.broadcast_to(np.asarray(umin, dtype=np.float64), (max(nv, 1),)))
    hi = None if umax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(umax, dtype=np.float64), (max(nv, 1),)))
    shape = (max(nv, 1), ny + 1, max(int(nbins), 0) + 2)
    avg, sum_, pdf = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    _stream_if_device(fields + [a, gate])
    check(load().tlab_cavg1v_n(nx, ny, nz, nv, int(nbins), c_vp(ibc_.ctypes.data), c_vp(lo.ctypes.data if lo is not None else 0),
                               c_vp(hi.ctypes.data if hi is not None else 0), _field_ptrs(fields, n, keep), int(igate), _gate_ptr(gate, n, keep),
                               _field_ptr(a, n, "a", keep), c_vp(avg.ctypes.data), c_vp(sum_.ctypes.data if raw else 0),
                               c_vp(pdf.ctypes.data if raw else 0)), "tlab_cavg1v_n")
    return (avg[:nv], sum_[:nv], pdf[:nv]) if raw else avg[:nv]


def cavg2v(nx, ny, nz, nbins, u, v, a):
    """The calculation of CAVG2V (statistics/cavg.f90:93): numpy (ny + 1, nb1*nb2 + 2 + 2*nb1) in the layout of pdf2v, the first nb1*nb2 entries
    of a plane the averages of a over the bins of (u, v)."""
    keep, n = [], nx * ny * nz
    nb = np.ascontiguousarray(nbins, dtype=np.int32)
    if nb.shape != (2,):
        raise TlabError("nbins must hold two values")
    out = np.zeros((ny + 1, max(int(nb[0]) * int(nb[1]), 0) + 2 + 2 * max(int(nb[0]), 0)))
    _stream_if_device([u, v, a])
    check(load().tlab_cavg2v(nx, ny, nz, c_vp(nb.ctypes.data), _field_ptr(u, n, "u", keep), _field_ptr(v, n, "v", keep), _field_ptr(a, n, "a", keep),
                             c_vp(out.ctypes.data)), "tlab_cavg2v")
    return out


# ---- spectra and correlations in horizontal planes: tools/statistics/spectra.f90 with module SpectraMod (include/tlab_amd.h) ------------------------
# Arrays of a call are all torch CUDA tensors or all host arrays (numpy, or torch CPU tensors); the results are of the kind of the inputs, shaped
# C-ordered: a Fortran out(i, j, k) is out[k, j, i].  Accumulators handed in through `out` are added to, as in the reference.
def _complex_ptr(a, n, name, keep):
    """the address of n complex numbers: a numpy complex128 array, a torch complex128 tensor, or either as 2 n float64 (re, im interleaved)"""
    if a is None:
        return c_vp(0)
    if isinstance(a, np.ndarray):
        if a.dtype == np.complex128:
            a = a.view(np.float64)
    elif a.is_complex():
        import torch
        a = torch.view_as_real(a)
    return _field_ptr(a, 2 * n, name, keep)


def _accumulators(like, shapes, out):
    """zeroed arrays of the kind of `like` for the keys of shapes that `out` (a dict, or None) does not hold"""
    res = dict(out) if out else {}
    for k, shp in shapes.items():
        if k in res:
            continue
        if isinstance(like, np.ndarray):
            res[k] = np.zeros(shp)
        else:
            import torch
            res[k] = torch.zeros(shp, dtype=torch.float64, device=like.device)
    return res


def spectrum_reduce(nx, ny, nz, nblock, kr_total, a_hat, b_hat=None, out=None, out2d=False):
    """tlab_spectrum_reduce: REDUCE_SPECTRUM + INTEGRATE_SPECTRUM (spectra_pool.f90) from the transformed fields a_hat, b_hat (None: auto),
    complex (nz, ny, nx/2+1) in the natural kz order.  A dict: "x" (ny/nblock, nx/2), "z" (ny/nblock, nz/2), "r" (ny/nblock, kr_total), with
    out2d "xz" (nz, ny/nblock, nx/2) in the reference's shuffled kz order, and "variance", numpy (ny,), the Parseval control."""
    keep, n, nyo = [], (nx // 2 + 1) * ny * nz, ny // max(int(nblock), 1)
    shapes = {"x": (nyo, nx // 2), "z": (nyo, nz // 2), "r": (nyo, max(int(kr_total), 0))}
    if out2d:
        shapes["xz"] = (nz, nyo, nx // 2)
    o = _accumulators(a_hat, shapes, out)
    var = np.zeros(ny)
    _stream_if_device([a_hat])
    check(load().tlab_spectrum_reduce(nx, ny, nz, int(nblock), int(kr_total), _complex_ptr(a_hat, n, "a_hat", keep), _complex_ptr(b_hat, n, "b_hat", keep),
                                      _field_ptr(o.get("xz"), nz * nyo * (nx // 2), "xz", keep), _field_ptr(o["x"], nyo * (nx // 2), "x", keep),
                                      _field_ptr(o["z"], nyo * (nz // 2), "z", keep), _field_ptr(o["r"], nyo * int(kr_total), "r", keep),
                                      c_vp(var.ctypes.data)), "tlab_spectrum_reduce")
    o["variance"] = var
    return o


def correlation_reduce(nx, ny, nz, nblock, nr_total, field, var1, var2, out=None, out2d=False, icalc_radial=1):
    """tlab_correlation_reduce: spectra.f90:653 and REDUCE_CORRELATION on the real field (nz, ny, nx) that the inverse transforms return, with
    the variances var1, var2 (ny values, host).  A dict: "x" (ny/nblock, nx), "z" (ny/nblock, nz), with icalc_radial "r" (ny/nblock, nr_total), with
    out2d "xz" (nz, ny/nblock, nx), and "variance", numpy (ny,): variance2."""
    keep, nyo = [], ny // max(int(nblock), 1)
    shapes = {"x": (nyo, nx), "z": (nyo, nz)}
    if icalc_radial == 1:
        shapes["r"] = (nyo, max(int(nr_total), 0))
    if out2d:
        shapes["xz"] = (nz, nyo, nx)
    o = _accumulators(field, shapes, out)
    var = np.zeros(ny)
    _stream_if_device([field])
    check(load().tlab_correlation_reduce(nx, ny, nz, int(nblock), int(nr_total), _field_ptr(field, nx * ny * nz, "field", keep),
                                         _profile(var1, ny, "var1", keep), _profile(var2, ny, "var2", keep),
                                         _field_ptr(o.get("xz"), nz * nyo * nx, "xz", keep), _field_ptr(o["x"], nyo * nx, "x", keep),
                                         _field_ptr(o["z"], nyo * nz, "z", keep), _field_ptr(o.get("r"), nyo * int(nr_total), "r", keep),
                                         c_vp(var.ctypes.data), int(icalc_radial)), "tlab_correlation_reduce")
    o["variance"] = var
    return o


def radial_samplesize(nx, nz, nr_total):
    """RADIAL_SAMPLESIZE (spectra_pool.f90:365): the number of separations (i, k) of a plane (nx, nz) in every ring, numpy (nr_total,)"""
    s = np.zeros(max(int(nr_total), 1))
    check(load().tlab_radial_samplesize(nx, nz, int(nr_total), c_vp(s.ctypes.data)), "tlab_radial_samplesize")
    return s


def cross_product(a_hat, b_hat=None, c=None):
    """c = b_hat conj(a_hat) (|a_hat|**2 with b_hat None) for complex arrays of one size; c defaults to b_hat (a_hat for an auto pair): in place"""
    keep = []
    c = (a_hat if b_hat is None else b_hat) if c is None else c
    is_complex = a_hat.dtype == np.complex128 if isinstance(a_hat, np.ndarray) else a_hat.is_complex()
    n = (a_hat.size if isinstance(a_hat, np.ndarray) else a_hat.numel()) // (1 if is_complex else 2)
    _stream_if_device([c])
    check(load().tlab_cross_product(n, _complex_ptr(a_hat, n, "a_hat", keep), _complex_ptr(b_hat, n, "b_hat", keep), _complex_ptr(c, n, "c", keep)),
          "tlab_cross_product")
    return c


def fluctuation(nx, ny, nz, a, mean, out):
    """out = a - mean(j): FI_FLUCTUATION_INPLACE (mappings/fi_dissipation.f90:119) into another array, mean: ny host values (avg_ik_v)"""
    keep = []
    _stream_if_device([a])
    check(load().tlab_fluctuation(nx, ny, nz, _field_ptr(a, nx * ny * nz, "a", keep), _profile(mean, ny, "mean", keep),
                                  _field_ptr(out, nx * ny * nz, "out", keep)), "tlab_fluctuation")
    return out


def avg_cov2v(nx, ny, nz, a, b):
    """The three COV2V2D of spectra.f90:624-628 in one pass: numpy (3, ny), the plane means of a*b, a*a, b*b"""
    keep, n = [], nx * ny * nz
    out = np.zeros((3, ny))
    _stream_if_device([a, b])
    check(load().tlab_avg_cov2v(nx, ny, nz, _field_ptr(a, n, "a", keep), _field_ptr(b, n, "b", keep), c_vp(out.ctypes.data), ny), "tlab_avg_cov2v")
    return out


def spectra_pair(plan, mode, nblock, kr_total, a, b=None, tmp=None, out=None, out2d=False):
    """tlab_spectra_pair: the loop body of spectra.f90:620-659 for one pair of fluctuation fields a, b (None: auto) on the transforms of a
    PoissonPlan.  mode: "spectra" | "correlations" (or 1 | 2).  tmp: three CUDA tensors of plan.isize_txc_field values (made when None).  The dict
    of spectrum_reduce / correlation_reduce plus "cov", numpy (3, ny): the covariances a*b, a*a, b*b of every plane."""
    import torch
    mode = {"spectra": 1, "correlations": 2}.get(mode, mode)
    nx, ny, nz = plan.nx, plan.ny, plan.nz
    keep, n, nyo = [], nx * ny * nz, ny // max(int(nblock), 1)
    n1, nz1 = (nx // 2, nz // 2) if mode == 1 else (nx, nz)
    shapes = {"x": (nyo, n1), "z": (nyo, nz1), "r": (nyo, max(int(kr_total), 0))}
    if out2d:
        shapes["xz"] = (nz, nyo, n1)
    o = _accumulators(a, shapes, out)
    if tmp is None:
        tmp = [torch.empty(plan.isize_txc_field, dtype=torch.float64, device=a.device) for _ in range(3)]
    cov, var = np.zeros((3, ny)), np.zeros(ny)
    _use_torch_stream()
    check(load().tlab_spectra_pair(plan._h, int(mode), int(nblock), int(kr_total), _field_ptr(a, n, "a", keep), _field_ptr(b, n, "b", keep),
                                   *[_ptr(t, plan.isize_txc_field, "tmp") for t in tmp], _field_ptr(o.get("xz"), nz * nyo * n1, "xz", keep),
                                   _field_ptr(o["x"], nyo * n1, "x", keep), _field_ptr(o["z"], nyo * nz1, "z", keep),
                                   _field_ptr(o["r"], nyo * int(kr_total), "r", keep), c_vp(cov.ctypes.data), c_vp(var.ctypes.data)), "tlab_spectra_pair")
    o["cov"], o["variance"] = cov, var
    return o


# ---- sampling between two statistics steps: phase averages (statistics/avg_phase.f90), towers (tools/dns/dns_tower.f90), saved planes
# (tools/dns/planes.f90).  The accumulators are the caller's arrays, of the kind of the fields (torch tensors or numpy arrays); no call synchronises.
def avg_phase_plane_id(itr, it_first, it_save):
    """plane_id of AvgPhaseSpaceExec (statistics/avg_phase.f90:142-143): mod((itr - 1) - it_first, it_save) + 1 with Fortran's mod; 1 for it_save = 0"""
    return int(load().tlab_avg_phase_plane_id(int(itr), int(it_first), int(it_save)))


def avg_phase_space(nx, ny, nz, fields, avg_planes, plane_id, avg, nz_total=None):
    """AvgPhaseSpace for index 1, 2 or 4 (statistics/avg_phase.f90:123): the z-average of every field into plane plane_id (1-based) of avg, laid out
    (len(fields), avg_planes + 1, ny, nx), and avg[:, -1] += that plane / avg_planes.  nz_total: g(3)%size (default nz).  Returns avg."""
    keep, fields = [], list(fields)
    ptrs = (c_vp * max(len(fields), 1))(*[_field_ptr(f, nx * ny * nz, "field %d" % i, keep).value for i, f in enumerate(fields)])
    _stream_if_device(fields + [avg])
    check(load().tlab_avg_phase_space(nx, ny, nz, nz if nz_total is None else int(nz_total), len(fields), ptrs, int(avg_planes), int(plane_id),
                                      _field_ptr(avg, nx * ny * (int(avg_planes) + 1) * len(fields), "avg", keep)), "tlab_avg_phase_space")
    return avg


def avg_phase_flow(nx, ny, nz, u, v, w, avg_planes, plane_id, avg_flow, avg_stress, nz_total=None):
    """AvgPhaseSpace(index 1) and AvgPhaseStress (:204) in one pass over u, v, w: avg_flow (3, avg_planes + 1, ny, nx) and avg_stress (6, ...), the
    stresses in the order uu, uv, uw, vv, vw, ww."""
    keep, n, m = [], nx * ny * nz, nx * ny * (int(avg_planes) + 1)
    _stream_if_device([u, v, w, avg_flow, avg_stress])
    check(load().tlab_avg_phase_flow(nx, ny, nz, nz if nz_total is None else int(nz_total), _field_ptr(u, n, "u", keep), _field_ptr(v, n, "v", keep),
                                     _field_ptr(w, n, "w", keep), int(avg_planes), int(plane_id), _field_ptr(avg_flow, 3 * m, "avg_flow", keep),
                                     _field_ptr(avg_stress, 6 * m, "avg_stress", keep)), "tlab_avg_phase_flow")
    return avg_flow, avg_stress


class Tower:
    """Module DNS_TOWER (tools/dns/dns_tower.f90) without its files: where the towers stand ([SaveTowers] Stride) and which slot of the caller's
    buffer the next call fills.  The buffer has the reference's layout, so the host's DNS_TOWER_WRITE works on a copy of it."""

    def __init__(self, nx, ny, nz, stride, nitera_save):
        self._h = c_vp()
        self.nx, self.ny, self.nz, self.nitera_save = int(nx), int(ny), int(nz), int(nitera_save)
        st = (ctypes.c_int * 3)(*[int(s) for s in stride])
        check(load().tlab_tower_create(ctypes.byref(self._h), self.nx, self.ny, self.nz, st, self.nitera_save), "tlab_tower_create")
        s = self.sizes()
        self.imax, self.jmax, self.kmax, self.isize_acc_field, self.isize_acc_mean, self.bufsize = s[:6]
        self.ipos, self.jpos, self.kpos = (self._positions(d, n) for d, n in ((1, self.imax), (2, self.jmax), (3, self.kmax)))

    def sizes(self):
        out = (ctypes.c_longlong * 8)()
        check(load().tlab_tower_sizes(self._h, out), "tlab_tower_sizes")
        return [int(x) for x in out]

    def _positions(self, idir, n):
        out = (ctypes.c_int * max(n, 1))()
        check(load().tlab_tower_positions(self._h, idir, out), "tlab_tower_positions")
        return np.array(out[:n], dtype=np.int64)

    accumulation = property(lambda self: self.sizes()[6])      # tower_accumulation
    mode_check = property(lambda self: self.sizes()[7])        # tower_mode_check

    def accumulate(self, index, fields, itime, rtime, buf):
        """DNS_TOWER_ACCUMULATE(v, index): index 1 = (u, v, w), 2 = (the first scalar,), 4 = (the pressure,)"""
        keep, fields = [], list(fields)
        ptrs = (c_vp * max(len(fields), 1))(*[_field_ptr(f, self.nx * self.ny * self.nz, "field %d" % i, keep).value for i, f in enumerate(fields)])
        if len(fields) != (3 if index == 1 else 1):
            raise TlabError("index %d takes %d fields" % (index, 3 if index == 1 else 1))
        _stream_if_device(fields + [buf])
        check(load().tlab_tower_accumulate(self._h, int(index), ptrs, int(itime), float(rtime), _field_ptr(buf, self.bufsize, "tower_buf", keep)),
              "tlab_tower_accumulate")

    def reset(self):
        check(load().tlab_tower_reset(self._h), "tlab_tower_reset")

    def views(self, buf):
        """the buffer by name, as DNS_TOWER_INITIALIZE points into it (:188-200): u, v, w, p, s (nitera_save, kmax, imax, jmax); um .. sm
        (nitera_save, jmax); t, it (nitera_save,)"""
        out, at = {}, 0
        for name in ("u", "v", "w", "p", "s"):
            out[name] = buf[at:at + self.isize_acc_field].reshape(self.nitera_save, self.kmax, self.imax, self.jmax)
            at += self.isize_acc_field
        for name in ("um", "vm", "wm", "pm", "sm"):
            out[name] = buf[at:at + self.isize_acc_mean].reshape(self.nitera_save, self.jmax)
            at += self.isize_acc_mean
        for name in ("t", "it"):
            out[name] = buf[at:at + self.nitera_save]
            at += self.nitera_save
        return out

    def __del__(self):
        try:
            if self._h:
                load().tlab_tower_destroy(self._h)
                self._h = c_vp()
        except Exception:       # noqa: BLE001
            pass


def planes_gather(nx, ny, nz, fields, idir, nodes, single=False, out=None):
    """The copies of PLANES_SAVE (tools/dns/planes.f90:279-342) for one direction: idir 1 -> data_i as (nz, nvars * n, ny), 2 -> data_j (nz, nvars * n,
    nx), 3 -> data_k (nvars * n, ny, nx); slot v * n + m = plane nodes[m] (1-based) of field v.  single: float32, rounded to nearest."""
    keep, fields, nodes = [], list(fields), [int(m) for m in nodes]
    size = len(fields) * len(nodes)
    shape = {1: (nz, size, ny), 2: (nz, size, nx), 3: (size, ny, nx)}.get(int(idir), (0,))
    ptrs = (c_vp * max(len(fields), 1))(*[_field_ptr(f, nx * ny * nz, "field %d" % i, keep).value for i, f in enumerate(fields)])
    if out is None:
        if fields and not isinstance(fields[0], np.ndarray):
            import torch
            out = torch.zeros(shape, dtype=torch.float32 if single else torch.float64, device=fields[0].device)
        else:
            out = np.zeros(shape, dtype=np.float32 if single else np.float64)
    _stream_if_device(fields + [out])
    optr = c_vp(out.ctypes.data) if isinstance(out, np.ndarray) else c_vp(out.data_ptr())
    check(load().tlab_planes_gather(nx, ny, nz, len(fields), ptrs, int(idir), len(nodes), (ctypes.c_int * max(len(nodes), 1))(*nodes), optr,
                                    1 if single else 0), "tlab_planes_gather")
    return out


def fi_gradient(dns, s, result, tmp):
    """FI_GRADIENT (mappings/fi_gradient.f90:26) with the plans of the driver dns: result = (s,x^2 + s,y^2) + s,z^2.  Returns result."""
    _use_torch_stream()
    check(load().tlab_fi_gradient(dns._h, _ptr(s, dns.n, "s"), _ptr(result, dns.n, "result"), _ptr(tmp, dns.n, "tmp")), "tlab_fi_gradient")
    return result


def log10_small(a):
    """a = log10(a + small_wp) in place (planes.f90:250), a torch tensor or a numpy array.  Returns a."""
    keep = []
    n = a.size if isinstance(a, np.ndarray) else a.numel()
    _stream_if_device([a])
    check(load().tlab_log10_small(n, _field_ptr(a, n, "a", keep)), "tlab_log10_small")
    return a


# ---- field mappings: the first-derivative maps in one pass over the gradients, the diffusion and pressure terms (csrc/tlab_amd_mappings.h) ------
# name -> (TLAB_MAP_* code, outputs, reads the scalar gradient)
MAPS = {
    "P": (0, 1, False), "Q": (1, 1, False), "R": (2, 1, False), "STRAIN": (3, 1, False), "STRAIN_TENSOR": (4, 6, False), "CURL": (5, 4, False),
    "VORTICITY": (6, 1, False), "VORTICITY_PRODUCTION": (7, 1, False), "STRAIN_PRODUCTION": (8, 1, False), "GRADIENT": (9, 1, True),
    "GRADIENT_PRODUCTION": (10, 1, True), "STRAIN_A": (11, 3, True),
}
FI_DIFFUSION_KINDS = {"VORTICITY_DIFFUSION": 0, "STRAIN_DIFFUSION": 1, "GRADIENT_DIFFUSION": 2, "STRAIN_PRESSURE": 3}


def _map_call(maps, like, n, out, keep):
    """(codes, output pointers, the dict handed back) of a call that names `maps`; out: a flat list of the outputs, new arrays like `like` if None"""
    maps = [maps] if isinstance(maps, str) else list(maps)
    unknown = [m for m in maps if m not in MAPS]
    if unknown or not maps:
        raise TlabError("maps: names of %s, got %r" % (", ".join(MAPS), unknown or maps))
    nout = sum(MAPS[m][1] for m in maps)
    if out is None:
        if isinstance(like, np.ndarray):
            out = [np.empty(n) for _ in range(nout)]
        else:
            import torch
            out = [torch.empty(n, dtype=torch.float64, device=like.device) for _ in range(nout)]
    out = list(out)
    if len(out) != nout:
        raise TlabError("out must hold %d arrays, one per output of the maps" % nout)
    codes = (ctypes.c_int * len(maps))(*[MAPS[m][0] for m in maps])
    ptrs = (c_vp * nout)(*[_field_ptr(o, n, "out[%d]" % i, keep).value for i, o in enumerate(out)])
    res, k = {}, 0
    for m in maps:
        res[m] = out[k] if MAPS[m][1] == 1 else tuple(out[k:k + MAPS[m][1]])
        k += MAPS[m][1]
    return codes, ptrs, res


def gradient_maps(du9, ds3, maps, out=None):
    """The maps `maps` (names of MAPS, or one name) of the velocity gradients du9 = [u,x u,y u,z v,x v,y v,z w,x w,y w,z] and, for GRADIENT,
    GRADIENT_PRODUCTION and STRAIN_A, of the scalar gradient ds3 = [s,x s,y s,z] (else None), in one pass that reads each gradient once: torch
    tensors (k_gradient_maps) or numpy arrays (the host loop), not a mix.  An entry of du9 / ds3 that no requested map reads may be None.
    A dict name -> array, or a tuple of arrays for STRAIN_TENSOR (Sxx Syy Szz Sxy Sxz Syz), CURL (wx wy wz, their squared magnitude) and
    STRAIN_A (strain1, strain2, G.G); out: the output arrays in that order, new ones if None.  Every operation is the reference's."""
    keep, du9 = [], list(du9)
    ds3 = [None] * 3 if ds3 is None else list(ds3)
    if len(du9) != 9 or len(ds3) != 3:
        raise TlabError("du9 must hold nine arrays and ds3 three")
    given = [a for a in du9 + ds3 if a is not None]
    if not given:
        raise TlabError("no gradient given")
    n = given[0].size if isinstance(given[0], np.ndarray) else given[0].numel()
    codes, optrs, res = _map_call(maps, given[0], n, out, keep)
    _stream_if_device(given)
    dptr = (c_vp * 9)(*[_field_ptr(a, n, "du9[%d]" % i, keep).value for i, a in enumerate(du9)])
    sptr = (c_vp * 3)(*[_field_ptr(a, n, "ds3[%d]" % i, keep).value for i, a in enumerate(ds3)]) if any(a is not None for a in ds3) else None
    check(load().tlab_gradient_maps(n, dptr, sptr, codes, len(codes), optrs), "tlab_gradient_maps")
    return res


def _dev_ptrs(arrays, n, name):
    return (c_vp * len(arrays))(*[_ptr(a, n, "%s[%d]" % (name, i)).value for i, a in enumerate(arrays)])


def velocity_gradients(dns, q, txc9):
    """OPR_Partial_X/Y/Z(OPR_P1) of q[0..2] by the plans of the driver dns, bcs = 0, into txc9 = [u,x u,y u,z v,x v,y v,z w,x w,y w,z]."""
    _use_torch_stream()
    check(load().tlab_dns_velocity_gradients(dns._h, _dev_ptrs(list(q)[:3], dns.n, "q"), _dev_ptrs(list(txc9), dns.n, "txc9")),
          "tlab_dns_velocity_gradients")
    return txc9


def scalar_gradient(dns, s, ds3):
    """The same of one scalar into ds3 = [s,x s,y s,z]."""
    _use_torch_stream()
    check(load().tlab_dns_scalar_gradient(dns._h, _ptr(s, dns.n, "s"), _dev_ptrs(list(ds3), dns.n, "ds3")), "tlab_dns_scalar_gradient")
    return ds3


def fi_maps(dns, q, s, maps, txc9, ds3=None, out=None):
    """velocity_gradients(q) into txc9, scalar_gradient(s) into ds3 where a map reads it, then gradient_maps: any set of FI_INVARIANT_P/Q/R,
    FI_STRAIN, FI_STRAIN_TENSOR, FI_CURL, FI_VORTICITY, FI_VORTICITY_PRODUCTION, FI_STRAIN_PRODUCTION, FI_GRADIENT, FI_GRADIENT_PRODUCTION and
    FI_STRAIN_A on the box of the driver dns from nine (twelve) derivatives, which stay in txc9 / ds3.  Device tensors; a dict as gradient_maps."""
    txc9 = list(txc9)
    if len(txc9) != 9:
        raise TlabError("txc9 must hold nine arrays")
    codes, optrs, res = _map_call(maps, txc9[0], dns.n, out, [])
    _use_torch_stream()
    check(load().tlab_dns_fi_maps(dns._h, _dev_ptrs(list(q)[:3], dns.n, "q"), _ptr(s, dns.n, "s"), codes, len(codes), _dev_ptrs(txc9, dns.n, "txc9"),
                                  _dev_ptrs(list(ds3), dns.n, "ds3") if ds3 is not None else None, optrs), "tlab_dns_fi_maps")
    return res


def fi_diffusion(dns, kind, q, f, result, work6):
    """FI_VORTICITY_DIFFUSION, FI_STRAIN_DIFFUSION, FI_GRADIENT_DIFFUSION (f: the scalar) or FI_STRAIN_PRESSURE (f: the pressure) -- kind: a key
    of FI_DIFFUSION_KINDS -- into result, the reference's OPR_Partial calls in the reference's order on the plans of the driver dns; no
    viscosity is multiplied.  work6: six work tensors ([0]: vort / strain / grad, [1..4]: tmp1 .. tmp4).  Returns result."""
    code = FI_DIFFUSION_KINDS.get(kind) if isinstance(kind, str) else int(kind)
    if code is None:
        raise TlabError("kind: one of %s" % ", ".join(FI_DIFFUSION_KINDS))
    work6 = list(work6)
    if len(work6) != 6:
        raise TlabError("work6 must hold six work arrays")
    _use_torch_stream()
    check(load().tlab_dns_fi_diffusion(dns._h, code, _dev_ptrs(list(q)[:3], dns.n, "q") if q is not None else None, _ptr(f, dns.n, "f"),
                                       _ptr(result, dns.n, "result"), _dev_ptrs(work6, dns.n, "work6")), "tlab_dns_fi_diffusion")
    return result


# the reference's routines by name: the map on the driver's box, its gradients left in txc9 (and ds3)
def _named(name, scalar):
    if scalar:
        def f(dns, q, s, txc9, ds3, out=None):
            return fi_maps(dns, q, s, name, txc9, ds3, out)[name]
    else:
        def f(dns, q, txc9, out=None):
            return fi_maps(dns, q, None, name, txc9, out=out)[name]
    f.__doc__ = "FI_%s of the reference on the driver dns: fi_maps with the one map %s." % (name if len(name) > 1 else "INVARIANT_" + name, name)
    return f


fi_strain, fi_strain_tensor, fi_curl = _named("STRAIN", False), _named("STRAIN_TENSOR", False), _named("CURL", False)
fi_invariant_q, fi_invariant_r = _named("Q", False), _named("R", False)
fi_vorticity_production, fi_strain_production = _named("VORTICITY_PRODUCTION", False), _named("STRAIN_PRODUCTION", False)
fi_gradient_production, fi_strain_a = _named("GRADIENT_PRODUCTION", True), _named("STRAIN_A", True)
