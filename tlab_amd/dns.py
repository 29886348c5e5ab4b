"""Host-side mirror of the RK driver around the hot path: module arrays q, s, hq, hs, txc (base/tlab_memory.f90:10-17),
RHS_GLOBAL_INCOMPRESSIBLE_1 (tools/dns/rhs_global_incompressible_1.f90:15), TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT and
TIME_RUNGEKUTTA (tools/dns/time.f90:559, :185).  Fields are torch CUDA tensors (HBM residency); every arithmetic
operation runs in the HIP library."""
import ctypes
import numpy as np

from .lib import load, check, TlabError, c_vp
from .operators import FdmPlan, PoissonPlan, _use_torch_stream

RKM_EXP3, RKM_EXP4 = 3, 4
DNS_BCS_DIRICHLET, DNS_BCS_NEUMANN = 3, 4          # tools/dns/boundary_bcs.f90:18-19


def velocity_bcs(kind):
    """[BoundaryConditions] VelocityJmin/Jmax keyword -> BcsFlowJm%type(1:3), tools/dns/boundary_bcs.f90:112-121."""
    kind = kind.strip().lower()
    if kind == "noslip":
        return [DNS_BCS_DIRICHLET] * 3
    if kind == "freeslip":
        return [DNS_BCS_NEUMANN, DNS_BCS_DIRICHLET, DNS_BCS_NEUMANN]
    raise TlabError("BoundaryConditions.Velocity: noslip or freeslip")


def scalar_bcs(kind):
    kind = kind.strip().lower()
    if kind == "dirichlet":
        return DNS_BCS_DIRICHLET
    if kind == "neumann":
        return DNS_BCS_NEUMANN
    raise TlabError("BoundaryConditions.Scalar: dirichlet or neumann")


def _bcs_arrays(nscal, velocity_jmin, velocity_jmax, scalar_jmin, scalar_jmax):
    IA = ctypes.c_int * 3
    fj0, fj1 = IA(*velocity_bcs(velocity_jmin)), IA(*velocity_bcs(velocity_jmax))
    SA = ctypes.c_int * max(nscal, 1)
    as_list = lambda v: [v] * nscal if isinstance(v, str) else list(v)      # noqa: E731
    sj0 = SA(*[scalar_bcs(k) for k in as_list(scalar_jmin)] or [DNS_BCS_DIRICHLET])
    sj1 = SA(*[scalar_bcs(k) for k in as_list(scalar_jmax)] or [DNS_BCS_DIRICHLET])
    return fj0, fj1, sj0, sj1


def _bounds_arrays(lo, hi, active):
    """ctypes arrays of the scalar bounds (lo = None: off).  Lists may be shorter than nscal (the scalars beyond them are not limited); the
    library refuses more entries than nscal, NaN bounds and lo > hi."""
    if lo is None and hi is None:
        return 0, None, None, None
    if lo is None or hi is None:
        raise ValueError("set_scalar_bounds: give both lo and hi, or neither (off)")
    lo, hi = [float(v) for v in np.atleast_1d(lo)], [float(v) for v in np.atleast_1d(hi)]
    act = [1] * len(lo) if active is None else [int(bool(a)) for a in np.atleast_1d(active)]
    if not (len(lo) == len(hi) == len(act)):
        raise ValueError("set_scalar_bounds: lo, hi and active differ in length")
    n = len(lo)
    m = max(n, 1)
    return n, (ctypes.c_int * m)(*act), (ctypes.c_double * m)(*lo), (ctypes.c_double * m)(*hi)


def zone_tables(y, nx, ny, nz, nscal, points_jmin, points_jmax, params_u, params_s, hard_u, hard_s, ref, global_field):
    """The blocks of Dns.set_buffer_zones for a decomposed driver, over the GLOBAL box: yields (end, group, size, nfields, tau, g) with tau (nfields,
    size) = (size, nfields) column-major and g the reference fields (nfields, nz, size, nx), or g = None for a block that is off.  The plane means of
    LoadBuffer = no span the whole plane (COV2V2D all-reduces over the ranks): global_field(name, i) returns field i of "q" / "s" as a host array
    (nz, ny, nx), or None where not every rank is local -- then hard_* or ref must be given."""
    L = load()
    dp = ctypes.POINTER(ctypes.c_double)
    y = np.ascontiguousarray(y, dtype=np.float64)
    for end, key, size, form in ((3, "jmin", int(points_jmin), 1), (4, "jmax", int(points_jmax), 2)):
        offset = 0 if end == 3 else ny - size
        for group, gkey, name, params, hard in ((0, "flow", "q", params_u, hard_u), (1, "scal", "s", params_s, hard_s)):
            nf = 3 if group == 0 else nscal
            if size == 0 or nf == 0:
                yield end, group, 0, nf, None, None
                continue
            p = [float(v) for v in np.atleast_1d(params)]
            if len(p) == 1:
                strength, sigma = [p[0]] * nf, 2.0
            elif len(p) == 2:
                strength, sigma = [p[0]] * nf, p[1]
            elif len(p) == nf + 1:
                strength, sigma = p[:nf], p[nf]
            else:
                raise TlabError("BufferZone.Parameters: 1, 2 or nfields + 1 values")
            tau = np.zeros((nf, max(size, 1)))
            for iq in range(nf):
                check(L.tlab_buffer_tau(ny, y.ctypes.data_as(dp), offset, size, strength[iq], sigma, form, tau[iq].ctypes.data_as(dp)), "tlab_buffer_tau")
            if ref is not None and (gkey, key) in ref:
                g = np.ascontiguousarray(ref[(gkey, key)], dtype=np.float64)
                if g.shape != (nf, nz, size, nx):
                    raise TlabError("buffer zone ref: global shape (nfields, nz, size, nx)")
            else:
                g = np.empty((nf, nz, size, nx))
                for iq in range(nf):
                    if hard is not None:
                        g[iq] = float(hard[iq])
                        continue
                    a3 = global_field(name, iq)
                    if a3 is None:
                        raise TlabError("set_buffer_zones: the plane means span all ranks; give hard_u / hard_s or ref when ranks live in other processes")
                    for jloc in range(size):      # COV2V2D (utils/averages.f90:244-267): serial sum, i fastest then k, / (nx nz)
                        g[iq, :, jloc, :] = float(np.cumsum(np.ascontiguousarray(a3[:, offset + jloc, :]).ravel())[-1]) / float(nx * nz)
            yield end, group, size, nf, tau, g


CORIOLIS_TYPES = {"none": 0, "explicit": 4, "normalized": 12}
BUOYANCY_TYPES = {"none": 0, "explicit": 4, "homogeneous": 5, "linear": 6, "bilinear": 7, "quadratic": 8, "normalizedmean": 9, "subtractmean": 10}


PRESSURE_DECOMPOSITIONS = {"total": 0, "advection": 2, "advdiff": 3, "diffusion": 4, "coriolis": 5, "buoyancy": 6}      # DCMP_* (include/dns_const.h:30-36)
MIXTURES = {"none": 0, "airwaterlinear": 12}                                  # MIXT_TYPE_* of the reference
INFRARED_TYPES = {"none": 0, "grayliquid": 1, "bulk1dlocal": 1, "gray": 2, "band": 3}
PART_TYPES = {"none": 0, "tracer": 1, "inertia": 2, "bilinearcloudthree": 4, "bilinearcloudfour": 5, "tiniaone": 6}      # PART_TYPE_* of the reference
PART_BCS = {"none": 0, "stick": 1, "specular": 2}


def body_force_args(nscal, coriolis, buoyancy):
    """The arguments of tlab_*_set_coriolis and tlab_*_set_buoyancy (after the handle) from the small dicts or tuples of set_body_forces."""
    dp = ctypes.POINTER(ctypes.c_double)

    def arr(v, n=None):
        a = np.zeros(0 if v is None else len(v)) if n is None else np.zeros(n)
        if v is not None:
            v = np.atleast_1d(np.asarray(v, dtype=np.float64))
            a[:min(len(a), len(v))] = v[:len(a)]
        return a

    def code(v, table, what):
        if isinstance(v, str):
            if v.strip().lower() not in table:
                raise TlabError("%s: one of %s" % (what, ", ".join(table)))
            return table[v.strip().lower()]
        return int(v)
    if coriolis is None:
        cor = (0, None, None)
    else:
        c = dict(zip(("type", "vector", "parameters"), coriolis)) if isinstance(coriolis, (tuple, list)) else dict(coriolis)
        vec, par = arr(c.get("vector", (0.0, 0.0, 0.0)), 3), arr(c.get("parameters", (0.0, 1.0)), 2)
        cor = (code(c.get("type", "explicit"), CORIOLIS_TYPES, "Rotation.Type"), vec, par)
    if buoyancy is None:
        bod = (0, None, 0, None, 0, nscal, None)
    else:
        b = dict(zip(("type", "vector", "parameters", "bbackground"), buoyancy)) if isinstance(buoyancy, (tuple, list)) else dict(buoyancy)
        par = arr(b.get("parameters", ()))
        bb = None if b.get("bbackground") is None else np.ascontiguousarray(b["bbackground"], dtype=np.float64)
        bod = (code(b.get("type", "linear"), BUOYANCY_TYPES, "BodyForce.Type"), arr(b.get("vector", (0.0, 0.0, 0.0)), 3), int(b.get("scalars", nscal)), par,
               len(par), int(b.get("inb_scal_array", nscal)), bb)
    p = lambda a: None if a is None or len(a) == 0 else a.ctypes.data_as(dp)      # noqa: E731
    keep = (cor, bod)                                                              # (the arrays live as long as the pointers)
    return (cor[0], p(cor[1]), p(cor[2])), (bod[0], p(bod[1]), bod[2], p(bod[3]), bod[4], bod[5], p(bod[6])), keep


def _extremes(mn, mx, lmin, lmax, locations):
    """(DilMin, DilMax[, (i, j, k) of the minimum, (i, j, k) of the maximum]) of the dilatation_extremes methods"""
    if not locations:
        return mn.value, mx.value
    return mn.value, mx.value, tuple(lmin), tuple(lmax)


def device_minmax(a):
    """MINMAX's local part (utils/minmax.f90) of a contiguous float64 device tensor: (min, max)."""
    _use_torch_stream()
    mn, mx = ctypes.c_double(0.0), ctypes.c_double(0.0)
    check(load().tlab_device_minmax(c_vp(a.data_ptr()), a.numel(), ctypes.byref(mn), ctypes.byref(mx)), "tlab_device_minmax")
    return mn.value, mx.value


def rk_coefficients(mode):
    """TIME_INITIALIZE, tools/dns/time.f90:86-108."""
    if mode == RKM_EXP3:   # Williamson 1980
        return ([1.0 / 3.0, 15.0 / 16.0, 8.0 / 15.0], [-5.0 / 9.0, -153.0 / 128.0])
    if mode == RKM_EXP4:   # Carpenter & Kennedy 1994
        kdt = [1432997174477.0 / 9575080441755.0, 5161836677717.0 / 13612068292357.0, 1720146321549.0 / 2090206949498.0,
               3134564353537.0 / 4481467310338.0, 2277821191437.0 / 14882151754819.0]
        kco = [-567301805773.0 / 1357537059087.0, -2404267990393.0 / 2016746695238.0, -3550918686646.0 / 2091501179385.0,
               -1275806237668.0 / 842570457699.0]
        return (kdt, kco)
    raise TlabError("only the explicit low-storage schemes RungeKuttaExplicit3/4 are built")


class Dns:
    """imax, jmax, kmax, inb_scal, visc, schmidt + the allocated arrays of TLab_Initialize_Memory (tlab_memory.f90:164-216)."""

    def __init__(self, x, y, z, nscal=1, visc=1.0 / 5000.0, schmidt=(1.0,), yuniform=True, rkm_mode=RKM_EXP3,
                 hyper_bc1_ext=0.0, device="cuda", plans=None, gy_elliptic=None, stagger=False):
        import torch
        self.nx, self.ny, self.nz = len(x), len(y), len(z)
        self.n = self.nx * self.ny * self.nz
        self.y = np.ascontiguousarray(y, dtype=np.float64)          # g(2)%nodes: the buffer zones' strength (set_buffer_zones)
        self._dxz = tuple(float(a[1] - a[0]) if len(a) > 1 else 0.0 for a in (x, z))      # the uniform spacings of x and z (spectra)
        self.nscal = int(nscal)
        self.visc = float(visc)
        self.schmidt = np.ascontiguousarray(schmidt, dtype=np.float64)[: self.nscal]
        # plans: optional (gx, gy, gz) built elsewhere, e.g. FdmPlan.from_tables with a host's CompactDirect6 tables in y
        self.g = list(plans) if plans is not None else [
            FdmPlan(x, True, True, hyper_bc1_ext=hyper_bc1_ext, stagger=stagger), FdmPlan(y, False, yuniform, hyper_bc1_ext=hyper_bc1_ext),
            FdmPlan(z, True, True, hyper_bc1_ext=hyper_bc1_ext, stagger=stagger)]
        # stagger: [Staggering] StaggerHorizontalPressure -- the driver reads it off the x plan (tlab_fdm_plan_info 7)
        # gy_elliptic: the y plan of EllipticOrder = CompactDirect6 (fdm_loc, opr_elliptic.f90:107-124) -> OPR_Poisson_FourierXZ_Direct
        self.poisson = PoissonPlan(self.g[0], self.g[1], self.g[2], self.nx, self.ny, self.nz, gy_elliptic=gy_elliptic)
        self.isize_txc_field = self.poisson.isize_txc_field
        f = lambda m: [torch.zeros(m, dtype=torch.float64, device=device) for _ in range(1)][0]   # noqa: E731
        self.q = [f(self.n) for _ in range(3)]
        self.s = [f(self.n) for _ in range(self.nscal)]
        self.hq = [f(self.n) for _ in range(3)]
        self.hs = [f(self.n) for _ in range(self.nscal)]
        self.txc = [f(self.isize_txc_field) for _ in range(9)]          # inb_txc = 9 (dns_read_local.f90:711)
        self.kdt, self.kco = rk_coefficients(rkm_mode)
        self.rkm_endstep = len(self.kdt)
        self._h = c_vp(0)
        sc = self.schmidt if self.nscal else np.zeros(1)
        check(load().tlab_dns_create(ctypes.byref(self._h), self.g[0]._h, self.g[1]._h, self.g[2]._h, self.poisson._h,
                                     self.nx, self.ny, self.nz, self.nscal, self.visc,
                                     sc.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), "tlab_dns_create")
        self._ptrs = None
        self.liquid = None                                              # the diagnostic array s(:, inb_scal_array) of a mixture (set_mixture)
        # [Particles] (set_particles): l_q, l_hq lists of device tensors (the columns), l_g%nodes (int32), l_g%tags (int64)
        self.l_q = self.l_hq = self.l_nodes = self.l_tags = None
        self.part_type, self.np = PART_TYPES["none"], 0
        self._part_ptrs = self._part_scratch = None
        # trajectories (set_trajectories): l_traj (float32, device), the tracked tags, the sampled fields, the counter and nitera_save
        self.l_traj = self.l_traj_tags = None
        self.traj_fields, self.traj_counter, self.traj_nsave = [], 0, 0

    def set_bcs(self, velocity_jmin="noslip", velocity_jmax="noslip", scalar_jmin="dirichlet", scalar_jmax="dirichlet"):
        """Wall boundary conditions in y by the reference's dns.ini keywords ([BoundaryConditions], boundary_bcs.f90:102-190)."""
        fj0, fj1, sj0, sj1 = _bcs_arrays(self.nscal, velocity_jmin, velocity_jmax, scalar_jmin, scalar_jmax)
        check(load().tlab_dns_set_bcs(self._h, fj0, fj1, sj0, sj1), "tlab_dns_set_bcs")

    def set_pressure_filter(self, fx=None, fy=None, fz=None, repeat=None):
        """[PressureFilter]: tlab_amd.Filter objects per direction (None = no filter); the caller keeps them alive."""
        self._pfilters = (fx, fy, fz)
        rp = (ctypes.c_int * 3)(*(repeat or (1, 1, 1)))
        h = [f._h if f is not None else None for f in (fx, fy, fz)]
        check(load().tlab_dns_set_pressure_filter(self._h, h[0], h[1], h[2], rp), "tlab_dns_set_pressure_filter")

    def set_filter(self, fx=None, fy=None, fz=None, repeat=None):
        """[Filter] (FilterDomain of DNS_FILTER): tlab_amd.Filter objects per direction (None = no filter, all None switches it off), each applied
        repeat[d] times; the caller keeps them alive.  A filter whose size is not the extent along its direction is refused and changes nothing."""
        rp = None if repeat is None else (ctypes.c_int * 3)(*(int(r) for r in repeat))
        h = [f._h if f is not None else None for f in (fx, fy, fz)]
        check(load().tlab_dns_set_filter(self._h, h[0], h[1], h[2], rp), "tlab_dns_set_filter")
        self._dfilters = (fx, fy, fz)

    def DNS_FILTER(self):
        """DNS_FILTER (tools/dns/dns_filter.f90) without its kin statistics, what dns_main.f90 calls every nitera_filter steps after TIME_RUNGEKUTTA:
        the filters of set_filter on u, v, w and the scalars in place, then the scalar bounds, then the diagnostic liquid of a mixture."""
        _use_torch_stream()
        q, s = self._arrays()[:2]
        check(load().tlab_dns_filter(self._h, q, s), "tlab_dns_filter")

    def set_remove_divergence(self, on):
        """dns.ini remove_divergence (default on): forcing = div(hq + q/dte); off: div(hq)."""
        check(load().tlab_dns_set_remove_divergence(self._h, int(bool(on))), "tlab_dns_set_remove_divergence")

    def set_surface_bcs(self, sfc_jmin=None, sfc_jmax=None, coupling_jmin=None, coupling_jmax=None):
        """[BoundaryConditions] Scalar<i>SfcTypeJmin/Jmax = "static" | "linear" and Scalar<i>CouplingJmin/Jmax per scalar (boundary_bcs.f90:76-87)."""
        ns = max(self.nscal, 1)
        code = lambda v: [1 if str(t).lower() == "linear" else 0 for t in (v or ["static"] * ns)]      # noqa: E731
        s0, s1 = (ctypes.c_int * ns)(*code(sfc_jmin)[:ns]), (ctypes.c_int * ns)(*code(sfc_jmax)[:ns])
        c0 = (ctypes.c_double * ns)(*[float(v) for v in (coupling_jmin or [0.0] * ns)][:ns])
        c1 = (ctypes.c_double * ns)(*[float(v) for v in (coupling_jmax or [0.0] * ns)][:ns])
        check(load().tlab_dns_set_surface_bcs(self._h, s0, s1, c0, c1), "tlab_dns_set_surface_bcs")

    def set_anelastic(self, rbackground=None, ribackground=None):
        """nse_eqns = anelastic with the background density profile rbackground(ny) (ribackground defaults to 1 / rbackground); None: incompressible.
        Module state of the Burgers operator, like the reference's rhoinv: it applies to every plan of the process until switched off."""
        dp = ctypes.POINTER(ctypes.c_double)
        if rbackground is None:
            check(load().tlab_dns_set_anelastic(self._h, None, None), "tlab_dns_set_anelastic")
            return
        rb = np.ascontiguousarray(rbackground, dtype=np.float64)
        ri = np.ascontiguousarray(1.0 / rb if ribackground is None else ribackground, dtype=np.float64)
        if rb.shape != (self.ny,) or ri.shape != (self.ny,):
            raise TlabError("anelastic profiles: ny values each")
        check(load().tlab_dns_set_anelastic(self._h, rb.ctypes.data_as(dp), ri.ctypes.data_as(dp)), "tlab_dns_set_anelastic")

    def set_scalar_bounds(self, lo=None, hi=None, active=None):
        """[Control] ScalLimit = yes, MinScalar / MaxScalar (DNS_BOUNDS_LIMIT, dns_local.f90:67-90): after the update of every substep each active
        scalar becomes min(max(s, lo), hi).  lo, hi, active: one entry per scalar (active defaults to all); None switches limiting off."""
        n, act, l, h = _bounds_arrays(lo, hi, active)
        check(load().tlab_dns_set_scalar_bounds(self._h, n, act, l, h), "tlab_dns_set_scalar_bounds")

    def set_buffer_zones(self, points_jmin=0, points_jmax=0, params_u=(1.0, 2.0), params_s=(1.0, 2.0), hard_u=None, hard_s=None, ref=None,
                         type="relaxation", points_imin=0, points_imax=0):
        """[BufferZone] Type = relaxation with PointsUJmin = PointsSJmin = points_jmin, PointsUJmax = PointsSJmax = points_jmax (the reference demands
        the pairs equal, dns_read_local.f90:380-386), ParametersU / ParametersS = 1, 2 or nfields + 1 values (strength(s), sigma; boundary_buffer.f90:91-139).
        The reference fields are built like INI_BLOCK with LoadBuffer = no (:291-333) from the fields the object holds NOW: per plane the mean in the
        reference's serial order, or the constants hard_u (3) / hard_s (nscal) of HardValues; or ref = {("flow" | "scal", "jmin" | "jmax"): array of
        shape (nfields, nz, size, nx)} as a loaded buffer would give them.  points 0 switches that end off.  type "filter" / "both" and zones at
        Imin / Imax are refused by the library (TLAB_EUNSUPPORTED)."""
        L = load()
        dp = ctypes.POINTER(ctypes.c_double)
        code = {"none": 0, "relaxation": 1, "filter": 2, "both": 3}.get(str(type).strip().lower())
        if code is None:
            raise TlabError("BufferZone.Type: none, relaxation, filter or both")
        check(L.tlab_dns_set_buffer_type(self._h, code), "tlab_dns_set_buffer_type")
        for end, pts in ((1, points_imin), (2, points_imax)):
            if int(pts) > 0:
                check(L.tlab_dns_set_buffer_zone(self._h, end, 0, int(pts), 3, None, None), "tlab_dns_set_buffer_zone")
        if code == 0:
            return
        y = self.y
        for end, key, size, form in ((3, "jmin", int(points_jmin), 1), (4, "jmax", int(points_jmax), 2)):
            offset = 0 if end == 3 else self.ny - size
            for group, gkey, fields, params, hard in ((0, "flow", self.q, params_u, hard_u), (1, "scal", self.s, params_s, hard_s)):
                nf = len(fields)
                if size == 0 or nf == 0:
                    check(L.tlab_dns_set_buffer_zone(self._h, end, group, 0, nf, None, None), "tlab_dns_set_buffer_zone")
                    continue
                p = [float(v) for v in np.atleast_1d(params)]
                if len(p) == 1:
                    strength, sigma = [p[0]] * nf, 2.0
                elif len(p) == 2:
                    strength, sigma = [p[0]] * nf, p[1]
                elif len(p) == nf + 1:
                    strength, sigma = p[:nf], p[nf]
                else:
                    raise TlabError("BufferZone.Parameters: 1, 2 or nfields + 1 values")
                tau = np.zeros((nf, max(size, 1)))                      # (size, nfields) column-major
                for iq in range(nf):
                    check(L.tlab_buffer_tau(self.ny, y.ctypes.data_as(dp), offset, size, strength[iq], sigma, form, tau[iq].ctypes.data_as(dp)), "tlab_buffer_tau")
                if ref is not None and (gkey, key) in ref:
                    r = np.ascontiguousarray(ref[(gkey, key)], dtype=np.float64)
                    if r.shape != (nf, self.nz, size, self.nx):
                        raise TlabError("buffer zone ref: shape (nfields, nz, size, nx)")
                else:
                    r = np.empty((nf, self.nz, size, self.nx))
                    for iq, t in enumerate(fields):
                        if hard is not None:
                            r[iq] = float(hard[iq])
                            continue
                        a3 = t.view(self.nz, self.ny, self.nx)[:, offset:offset + size, :].cpu().numpy()
                        for jloc in range(size):      # COV2V2D (utils/averages.f90:244-267): serial sum, i fastest then k, / (nx nz)
                            r[iq, :, jloc, :] = float(np.cumsum(np.ascontiguousarray(a3[:, jloc, :]).ravel())[-1]) / float(self.nx * self.nz)
                check(L.tlab_dns_set_buffer_zone(self._h, end, group, size, nf, tau.ctypes.data_as(dp), r.ctypes.data_as(dp)), "tlab_dns_set_buffer_zone")

    def buffer_relax_flow(self):
        """BOUNDARY_BUFFER_RELAX_FLOW on (q, hq) as an operator of its own."""
        _use_torch_stream()
        q, _, hq, _, _ = self._arrays()
        check(load().tlab_dns_buffer_relax_flow(self._h, q, hq), "tlab_dns_buffer_relax_flow")

    def buffer_relax_scal(self):
        """BOUNDARY_BUFFER_RELAX_SCAL on (s, hs) as an operator of its own."""
        _use_torch_stream()
        _, s, _, hs, _ = self._arrays()
        check(load().tlab_dns_buffer_relax_scal(self._h, s, hs), "tlab_dns_buffer_relax_scal")

    def set_body_forces(self, coriolis=None, buoyancy=None):
        """[Rotation] and [BodyForce] (TLab_Sources_Flow, applied once per substep before the pressure forcing).  None switches the term off.
        coriolis: {"type": "explicit" | "normalized", "vector": f / Rossby (3), "parameters": (angle, geostrophic speed)} or the tuple (type, vector,
        parameters).  buoyancy: {"type": "homogeneous" | "linear" | "bilinear" | "quadratic", "vector": g / Froude (3), "parameters": (...),
        "scalars": buoyancy%scalar(1) (default nscal), "inb_scal_array": (default nscal; linear: c0 = parameters[inb_scal_array]),
        "bbackground": ny values or None} or the tuple (type, vector, parameters[, bbackground]).  "explicit", "normalizedmean" and "subtractmean"
        buoyancy are refused by the library (TLAB_EUNSUPPORTED)."""
        cor, bod, keep = body_force_args(self.nscal, coriolis, buoyancy)
        check(load().tlab_dns_set_coriolis(self._h, *cor), "tlab_dns_set_coriolis")
        check(load().tlab_dns_set_buoyancy(self._h, *bod), "tlab_dns_set_buoyancy")
        del keep

    def sources_flow(self):
        """TLab_Sources_Flow on (q, s, hq) as an operator of its own: hq += Coriolis + buoyancy."""
        _use_torch_stream()
        q, s, hq, _, _ = self._arrays()
        check(load().tlab_dns_sources_flow(self._h, q, s, hq), "tlab_dns_sources_flow")

    def set_mixture(self, name="airwaterlinear", parameters=()):
        """[Thermodynamics] Type = Linear, Mixture = AirWaterLinear with thermo_param = parameters (at least nscal + 1 values), or "none".  With a
        mixture the driver holds the diagnostic liquid as Dns.liquid (inb_scal_array = nscal + 1; Dns.s keeps its nscal tensors): call
        FI_DIAGNOSTIC() once the scalars are loaded, every substep refreshes it after its update.  Other mixtures are refused by the library."""
        import torch
        code = MIXTURES.get(name.strip().lower()) if isinstance(name, str) else int(name)
        if code is None:
            raise TlabError("Thermodynamics.Mixture: one of %s" % ", ".join(MIXTURES))
        par = np.ascontiguousarray(parameters, dtype=np.float64).reshape(-1)
        dp = ctypes.POINTER(ctypes.c_double)
        check(load().tlab_dns_set_mixture(self._h, code, par.ctypes.data_as(dp) if len(par) else None, len(par)), "tlab_dns_set_mixture")
        self.liquid = torch.zeros(self.n, dtype=torch.float64, device=self.q[0].device) if code != 0 else None
        self._ptrs = None

    def FI_DIAGNOSTIC(self):
        """physics/fi_diagnostic.f90:44-47: the liquid from the prognostic scalars (THERMO_AIRWATER_LINEAR)."""
        _use_torch_stream()
        check(load().tlab_dns_diagnostic(self._h, self._arrays()[1]), "tlab_dns_diagnostic")

    def set_infrared(self, type="grayliquid", scalar=1, kappa=0.0, flux_top=0.0, flux_bottom=0.0):
        """[Infrared] as Radiation_Initialize leaves it: type "none" | "grayliquid" ("bulk1dlocal" is the same), the 1-based scalar the heating acts
        on, kappa(1,1), auxiliar(1) (downward flux at the top), auxiliar(2) (upward flux at the bottom).  The absorbing field is the liquid."""
        code = INFRARED_TYPES.get(type.strip().lower()) if isinstance(type, str) else int(type)
        if code is None:
            raise TlabError("Infrared.Type: one of %s" % ", ".join(INFRARED_TYPES))
        check(load().tlab_dns_set_infrared(self._h, code, int(scalar), float(kappa), float(flux_top), float(flux_bottom)), "tlab_dns_set_infrared")

    def sources_scal(self):
        """TLab_Sources_Scal on (s, hs) as an operator of its own: hs[scalar-1] += the infrared heating; txc[0], txc[1] are scratch."""
        _use_torch_stream()
        _, s, _, hs, txc = self._arrays()
        check(load().tlab_dns_sources_scal(self._h, s, hs, txc), "tlab_dns_sources_scal")

    def set_particles(self, type="tracer", number=0, bcs=None, stokes=0.0, settling=0.0):
        """[Particles] Type = tracer | inertia with `number` particles (l_g%np), BoundaryCondition bcs = None (the reference's default for the type) |
        "none" | "stick" | "specular", and stokes / settling of [Parameters].  Allocates l_q, l_hq (lists of inb_part device tensors, zero), l_nodes
        (int32) and l_tags (int64, 1..np); the caller fills the positions (and velocities) and calls locate_particles() once.  "none" takes them away."""
        import torch
        code = PART_TYPES.get(type.strip().lower()) if isinstance(type, str) else int(type)
        wall = -1 if bcs is None else (PART_BCS.get(bcs.strip().lower()) if isinstance(bcs, str) else int(bcs))
        if code is None or wall is None:
            raise TlabError("Particles.Type: one of %s; BoundaryCondition: one of %s" % (", ".join(PART_TYPES), ", ".join(PART_BCS)))
        if int(number) < 0:
            raise TlabError("set_particles: number < 0")
        check(load().tlab_dns_set_particles(self._h, code, wall, float(stokes), float(settling)), "tlab_dns_set_particles")
        self.part_type, self.np = code, int(number) if code else 0
        self._part_ptrs = self._part_scratch = None
        if code == 0 or self.l_traj is not None:      # (the driver drops its table with the particles; a new population needs a new l_traj)
            if code != 0:
                check(load().tlab_dns_set_trajectories(self._h, 0, None), "tlab_dns_set_trajectories")
            self.l_traj = self.l_traj_tags = None
            self.traj_fields, self.traj_counter, self.traj_nsave = [], 0, 0
        if code == 0:
            self.l_q = self.l_hq = self.l_nodes = self.l_tags = None
            return
        dev, ncol = self.q[0].device, 6 if code == PART_TYPES["inertia"] else 3
        m = max(self.np, 1)
        self.l_q = [torch.zeros(m, dtype=torch.float64, device=dev)[:self.np] for _ in range(ncol)]
        self.l_hq = [torch.zeros(m, dtype=torch.float64, device=dev)[:self.np] for _ in range(ncol)]
        self.l_nodes = torch.ones(m, dtype=torch.int32, device=dev)[:self.np]
        self.l_tags = torch.arange(1, m + 1, dtype=torch.int64, device=dev)[:self.np]

    def _particle_arrays(self):
        if self.l_q is None:
            raise TlabError("no particles are set on this driver (set_particles)")
        if self._part_ptrs is None:
            arr = lambda ts: (c_vp * len(ts))(*[t.data_ptr() for t in ts])      # noqa: E731
            self._part_ptrs = (arr(self.l_q), arr(self.l_hq))
        return self._part_ptrs

    def locate_particles(self):
        """LOCATE_Y: l_nodes from the y positions l_q[1]."""
        _use_torch_stream()
        self._particle_arrays()
        check(load().tlab_dns_particle_locate(self._h, self.np, self.l_q[1].data_ptr(), self.l_nodes.data_ptr()), "tlab_dns_particle_locate")

    def TIME_SUBSTEP_PARTICLE(self, dte, kco=1.0, scale_tendencies=False):
        """tools/dns/time.f90:906-1070 with the scaling of l_hq (:300-304); reads q, so it goes before the flow substep of the same stage."""
        _use_torch_stream()
        lq, lhq = self._particle_arrays()
        check(load().tlab_dns_substep_particle(self._h, float(dte), float(kco), int(scale_tendencies), self.np, self._arrays()[0], lq, lhq,
                                               self.l_nodes.data_ptr()), "tlab_dns_substep_particle")

    def sort_particles(self):
        """tlab_dns_particle_sort: l_q, l_hq, l_nodes, l_tags permuted together by cell (the scratch is kept for the next call)."""
        import torch
        _use_torch_stream()
        lq, lhq = self._particle_arrays()
        L = load()
        need = ctypes.c_longlong(0)
        check(L.tlab_dns_particle_sort(self._h, self.np, lq, lhq, None, None, None, 0, ctypes.byref(need)), "tlab_dns_particle_sort")
        if self._part_scratch is None or self._part_scratch.numel() < need.value:
            self._part_scratch = torch.empty(max(need.value, 1), dtype=torch.uint8, device=self.q[0].device)
        check(L.tlab_dns_particle_sort(self._h, self.np, lq, lhq, self.l_nodes.data_ptr(), self.l_tags.data_ptr(), self._part_scratch.data_ptr(),
                                       self._part_scratch.numel(), None), "tlab_dns_particle_sort")

    def _positions(self):
        lq, _ = self._particle_arrays()
        return lq

    def FIELD_TO_PARTICLE(self, fields, out=None):
        """FIELD_TO_PARTICLE (particle_interpolate.f90:186-332) of a list of device fields (nx ny nz each) at the particles: ADDS onto the tensors of
        `out` (np each) as the reference does; out = None allocates zeros.  Returns out."""
        import torch
        _use_torch_stream()
        lq = self._positions()
        fields = list(fields)
        if out is None:
            out = [torch.zeros(max(self.np, 1), dtype=torch.float64, device=self.q[0].device)[:self.np] for _ in fields]
        out = list(out)
        if len(out) != len(fields):
            raise TlabError("FIELD_TO_PARTICLE: as many targets as fields")
        arr = lambda ts: (c_vp * max(len(ts), 1))(*[t.data_ptr() for t in ts])      # noqa: E731
        check(load().tlab_dns_field_to_particle(self._h, len(fields), arr(fields), self.np, lq, self.l_nodes.data_ptr(), arr(out)),
              "tlab_dns_field_to_particle")
        return out

    def PARTICLE_TO_FIELD(self, property=None, out=None, periodic=True):
        """PARTICLE_TO_FIELD (particle_to_field.f90): the trilinear deposit of a particle property (device tensor of np; None: 1 per particle, the
        number density) onto the grid.  periodic=True adds what falls on the seam's upper corners to index 0 (the decomposed reference; conserves the
        property), False drops it (the serial reference).  The sums are atomic: a node with several contributions is reproduced up to rounding."""
        import torch
        _use_torch_stream()
        lq = self._positions()
        if out is None:
            out = torch.empty(self.n, dtype=torch.float64, device=self.q[0].device)
        check(load().tlab_dns_particle_to_field(self._h, self.np, lq, self.l_nodes.data_ptr(), None if property is None else property.data_ptr(),
                                                int(bool(periodic)), out.data_ptr()), "tlab_dns_particle_to_field")
        return out

    def set_trajectories(self, number=None, tags=None, nsave=1, fields=()):
        """ParticleTrajectories_Initialize (particle_trajectories.f90:104-149): track `tags`, or with tags = None the reference's default list of
        `number` tags 1 + (j - 1) (np // number); l_traj is the reference's l_traj(number + 1, nsave, inb_part + len(fields)) as a zeroed float32
        tensor of shape (inb_part + len(fields), nsave, number + 1); `fields` are the device fields sampled behind the prognostic columns
        (TrajType = eulerian: d.q + d.s).  number = 0 (or an empty list) switches the trajectories off."""
        import torch
        self._particle_arrays()
        if tags is None:
            number = int(number or 0)
            if number < 0 or number > self.np:
                raise TlabError("set_trajectories: the number of trajectories must lie in 0 .. np")       # particle_trajectories.f90:76-79
            stride = self.np // number if number else 0
            tags = [1 + j * stride for j in range(number)]
        tg = np.ascontiguousarray(np.asarray(tags, dtype=np.int64).ravel())
        check(load().tlab_dns_set_trajectories(self._h, len(tg), tg.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))), "tlab_dns_set_trajectories")
        self.l_traj = self.l_traj_tags = None
        self.traj_fields, self.traj_counter, self.traj_nsave = [], 0, 0
        if len(tg) == 0:
            return
        if int(nsave) < 1:
            raise TlabError("set_trajectories: nsave < 1")
        self.l_traj_tags, self.traj_fields, self.traj_nsave = tg, list(fields), int(nsave)
        self.l_traj = torch.zeros(len(self.l_q) + len(self.traj_fields), self.traj_nsave, len(tg) + 1, dtype=torch.float32, device=self.q[0].device)

    def ParticleTrajectories_Accumulate(self, rtime):
        """particle_trajectories.f90:156-230: the next column of l_traj (the counter advances; after nsave calls, write and call
        trajectories_written())."""
        _use_torch_stream()
        lq = self._positions()
        if self.l_traj is None:
            raise TlabError("no trajectories are set on this driver (set_trajectories)")
        f = self.traj_fields
        fp = (c_vp * max(len(f), 1))(*[t.data_ptr() for t in f])
        check(load().tlab_dns_trajectories_accumulate(self._h, float(rtime), self.traj_counter + 1, self.traj_nsave, self.np, lq,
                                                      self.l_nodes.data_ptr(), self.l_tags.data_ptr(), len(f), fp, self.l_traj.data_ptr()),
              "tlab_dns_trajectories_accumulate")
        self.traj_counter += 1

    def trajectories_written(self):
        """the end of ParticleTrajectories_Write (:266-267): l_traj = 0, counter = 0 (the file output itself is the caller's)."""
        if self.l_traj is not None:
            _use_torch_stream()
            self.l_traj.zero_()
        self.traj_counter = 0

    def set_fusion(self, on):
        """on (default): pointwise sums folded into the operator kernels; off: the reference's literal sequence."""
        check(load().tlab_dns_set_fusion(self._h, int(bool(on))), "tlab_dns_set_fusion")

    def _arrays(self):
        if self._ptrs is None:
            def arr(ts):
                a = (c_vp * max(len(ts), 1))()
                for i, t in enumerate(ts):
                    a[i] = t.data_ptr()
                return a
            s = self.s + ([self.liquid] if self.liquid is not None else [])      # s(isize_field, inb_scal_array): the liquid behind the scalars
            self._ptrs = tuple(arr(t) for t in (self.q, s, self.hq, self.hs, self.txc))
        return self._ptrs

    def RHS_GLOBAL_INCOMPRESSIBLE_1(self, dte):
        _use_torch_stream()
        q, s, hq, hs, txc = self._arrays()
        check(load().tlab_rhs_global_incompressible_1(self._h, float(dte), q, s, hq, hs, txc), "tlab_rhs_global_incompressible_1")

    def TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(self, dte, kco=1.0, scale_tendencies=False):
        _use_torch_stream()
        q, s, hq, hs, txc = self._arrays()
        check(load().tlab_time_substep_incompressible_explicit(self._h, float(dte), float(kco), int(scale_tendencies), q, s, hq, hs, txc),
              "tlab_time_substep_incompressible_explicit")

    def load_fields(self, flow_name=None, scal_name=None):
        """Restart files of the reference: <flow_name>.1..3 = u, v, w; <scal_name>.1..nscal (IO_Read_Fields, io_fields.f90:150).
        Returns (nt, params) of the last header read."""
        import torch
        from . import io as tio
        nt, params = None, None
        for name, dst in ((flow_name, self.q), (scal_name, self.s)):
            if name is None or not dst:
                continue
            fields, nt, params = tio.io_read_fields(name, self.nx, self.ny, self.nz, len(dst))
            for t, a in zip(dst, fields):
                t.copy_(torch.from_numpy(a))
        return nt, params

    def save_fields(self, flow_name=None, scal_name=None, nt=0, params=()):
        """IO_Write_Fields (io_fields.f90:346): files the reference's own tools (averages.x, visuals.x, dns.x) read back."""
        from . import io as tio
        for name, src in ((flow_name, self.q), (scal_name, self.s)):
            if name is not None and src:
                tio.io_write_fields(name, self.nx, self.ny, self.nz, nt, [t.cpu().numpy() for t in src], params)

    def TIME_COURANT(self, cfla, cfld):
        """tools/dns/time.f90:365-548.  Returns ((pmax1, pmax2), dtime): the CFL and diffusion maxima and the time step they allow."""
        _use_torch_stream()
        q = self._arrays()[0]
        pmax = (ctypes.c_double * 2)()
        dt = ctypes.c_double(0.0)
        check(load().tlab_time_courant(self._h, q, float(cfla), float(cfld), pmax, ctypes.byref(dt)), "tlab_time_courant")
        return (pmax[0], pmax[1]), dt.value

    def FI_INVARIANT_P(self, result, tmp1):
        """mappings/fi_vectorcalculus.f90:111: result = -div(q)."""
        _use_torch_stream()
        check(load().tlab_fi_invariant_p(self._h, self.q[0].data_ptr(), self.q[1].data_ptr(), self.q[2].data_ptr(), result.data_ptr(), tmp1.data_ptr()),
              "tlab_fi_invariant_p")

    def dilatation_bounds(self):
        """DNS_BOUNDS_CONTROL, tools/dns/dns_local.f90:157-187 (incompressible): (DilMin, DilMax) = logs_data(10:11) of dns.out."""
        self.FI_INVARIANT_P(self.txc[0], self.txc[1])
        mn, mx = ctypes.c_double(0.0), ctypes.c_double(0.0)
        check(load().tlab_minmax(self._h, self.txc[0].data_ptr(), self.nx, self.ny, self.nz, ctypes.byref(mn), ctypes.byref(mx)), "tlab_minmax")
        return -mx.value, -mn.value

    def dilatation_extremes(self, locations=True):
        """DNS_BOUNDS_CONTROL with the location of its failure branch (dns_local.f90:157-230): (DilMin, DilMax) = min / max of div(q), and with
        locations also the 1-based (i, j, k) of the first occurrence of each in Fortran order (minloc / maxloc).  Destroys txc[0], txc[5], txc[6]
        (and txc[2..4] in anelastic runs, which weight q by rbackground first)."""
        _use_torch_stream()
        q, _, _, _, txc = self._arrays()
        mn, mx = ctypes.c_double(0.0), ctypes.c_double(0.0)
        lmin, lmax = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
        check(load().tlab_dns_dilatation_extremes(self._h, q, txc, ctypes.byref(mn), ctypes.byref(mx), lmin if locations else None,
                                                   lmax if locations else None), "tlab_dns_dilatation_extremes")
        return _extremes(mn, mx, lmin, lmax, locations)

    def AVG_IK_V(self, a):
        """AVG_IK_V (utils/averages.f90:301) of one field of the box: the profile of its plane averages, numpy (ny,)."""
        from .operators import avg_ik_v
        return avg_ik_v(self.nx, self.ny, self.nz, [a])[0]

    def plane_means(self):
        """rU, rV, rW and rS (a list, one profile per scalar) from one pass over q + s (AVG_FLOW_XZ :458-460, AVG_SCAL_XZ :358)."""
        from .operators import avg_ik_v
        m = avg_ik_v(self.nx, self.ny, self.nz, self.q + self.s)
        return {"rU": m[0], "rV": m[1], "rW": m[2], "rS": [m[3 + i] for i in range(self.nscal)]}

    def flow_moments(self, p=None):
        """The covariances of AVG_FLOW_XZ that need no derivative (avg_flow_xz.f90:513-553, :597-654), incompressible: fU = rU.  Takes the
        means first (and rP of a pressure field p), then one pass; a dict of profiles keyed by the reference's names (operators.FLOW_MOMENTS,
        with p also FLOW_MOMENTS_P), plus the means."""
        from .operators import avg_moments_flow, FLOW_MOMENTS, FLOW_MOMENTS_P
        m = self.plane_means()
        rP = self.AVG_IK_V(p) if p is not None else None
        out = avg_moments_flow(self.nx, self.ny, self.nz, self.q[0], self.q[1], self.q[2], m["rU"], m["rV"], m["rW"], p, rP)
        r = dict(zip(FLOW_MOMENTS + (FLOW_MOMENTS_P if p is not None else ()), out))
        r.update(rU=m["rU"], rV=m["rV"], rW=m["rW"])
        if p is not None:
            r["rP"] = rP
        return r

    def scal_moments(self, is_, p=None):
        """The moments and fluxes of scalar is_ (0-based) in AVG_SCAL_XZ (avg_scal_xz.f90:373-455), incompressible: fS = rS.  As flow_moments."""
        from .operators import avg_moments_scal, SCAL_MOMENTS, SCAL_MOMENTS_P
        m = self.plane_means()
        rP = self.AVG_IK_V(p) if p is not None else None
        out = avg_moments_scal(self.nx, self.ny, self.nz, self.s[is_], self.q[0], self.q[1], self.q[2], m["rS"][is_], m["rU"], m["rV"], m["rW"], p, rP)
        r = dict(zip(SCAL_MOMENTS + (SCAL_MOMENTS_P if p is not None else ()), out))
        r.update(rS=m["rS"][is_], rU=m["rU"], rV=m["rV"], rW=m["rW"])
        if p is not None:
            r["rP"] = rP
        return r

    def plane_pdfs(self, p=None, nbins=32, ibc=2, gate=None, igate=0, umin=0.0, umax=0.0):
        """The block stats_pdfs of DNS_STATISTICS (dns_statistics.f90:122-148): the histograms of PDF1V_N for u, v, w, (p,) and every scalar in
        one call of tlab_pdf1v_n -- three passes over the fields for all planes and the volume.  A dict keyed by the reference's tags u v w (p)
        s1 s2 ..: numpy (ny + 1, nbins + 2) each, nbins counts and the centres of the first and the last bin per plane, the volume last.  gate
        (an int8 tensor of the box) with igate != 0: only points with gate == igate take part; umin, umax: the external interval(s) of ibc = 0.  No file is written."""
        from .operators import pdf1v_n
        fields = self.q + ([p] if p is not None else []) + self.s
        tags = ["u", "v", "w"] + (["p"] if p is not None else []) + ["s%d" % (i + 1) for i in range(self.nscal)]
        out = pdf1v_n(self.nx, self.ny, self.nz, fields, nbins, ibc, umin, umax, gate, igate)
        return dict(zip(tags, out))

    def FI_PRESSURE_BOUSSINESQ(self, p=None, decomposition="total"):
        """physics/fi_pressure_boussinesq.f90:8: the pressure of q (and s, through the body forces) into p, which is returned; default
        self.txc[2], the array DNS_STATISTICS hands (dns_statistics.f90:93).  self.txc[0], [1] and [3..8] are the work space, as there; advection
        and diffusion need a seventh sum array, which the driver allocates once.  decomposition: a key of PRESSURE_DECOMPOSITIONS or its code.
        q, s, hq, hs and the state of the driver are unchanged; the call returns with its launches enqueued."""
        import torch
        code = PRESSURE_DECOMPOSITIONS.get(decomposition.strip().lower()) if isinstance(decomposition, str) else int(decomposition)
        if code is None:
            raise TlabError("decomposition: one of %s" % ", ".join(PRESSURE_DECOMPOSITIONS))
        p = self.txc[2] if p is None else p
        tmp = [t for t in self.txc[3:] if t.data_ptr() != p.data_ptr()]
        if code in (PRESSURE_DECOMPOSITIONS["advection"], PRESSURE_DECOMPOSITIONS["diffusion"]) and len(tmp) < 7:
            if getattr(self, "_pressure_tmp", None) is None:
                self._pressure_tmp = torch.empty(self.isize_txc_field, dtype=torch.float64, device=self.q[0].device)
            tmp.append(self._pressure_tmp)
        if p.numel() < self.isize_txc_field:
            raise TlabError("p must hold isize_txc_field = %d values" % self.isize_txc_field)
        _use_torch_stream()
        q, s = self._arrays()[:2]
        ptmp = (c_vp * len(tmp))(*[t.data_ptr() for t in tmp])
        check(load().tlab_dns_pressure(self._h, code, q, s, p.data_ptr(), self.txc[0].data_ptr(), self.txc[1].data_ptr(), ptmp, len(tmp)),
              "tlab_dns_pressure")
        return p

    def FI_VORTICITY(self, result=None):
        """mappings/fi_vorticity.f90:28: the squared magnitude of the vorticity of q into result (default self.txc[0], as in DNS_STATISTICS);
        self.txc[3..8] hold the six derivatives v,x  u,y  u,z  w,x  w,y  v,z on return (self.txc[2], where FI_PRESSURE_BOUSSINESQ leaves the
        pressure, is not touched).  Returns result."""
        from .operators import fi_vorticity
        return fi_vorticity(self, self.q[0], self.q[1], self.q[2], self.txc[0] if result is None else result, self.txc[3:9])

    def intermittency(self):
        """The block stats_intermittency of DNS_STATISTICS (dns_statistics.f90:99-117): FI_VORTICITY into self.txc[0], MINMAX, the gate
        txc[0] > (1.0e-3*1.0e-3)*amax -- the reference's arithmetic; its comment says 0.1 %, its code 1e-6 -- and INTER_N_XZ with one level.
        {"Vorticity": numpy (ny,)}, the area fraction of the gate in every plane.  No file is written."""
        from .operators import gate_threshold, inter_n_xz
        vort = self.FI_VORTICITY()
        mn, mx = ctypes.c_double(0.0), ctypes.c_double(0.0)
        check(load().tlab_minmax(self._h, vort.data_ptr(), self.nx, self.ny, self.nz, ctypes.byref(mn), ctypes.byref(mx)), "tlab_minmax")
        gate = gate_threshold(vort[: self.n], (1.0e-3 * 1.0e-3) * mx.value)
        return {"Vorticity": inter_n_xz(self.nx, self.ny, self.nz, 1, gate)[0]}

    def FI_GATE(self, opt_cond, thresholds, relative=False, scal=None):
        """mappings/fi_gate.f90:3 for opt_cond 2 .. 7: the partition of the box as an int8 tensor.  2: scalar `scal` (1-based, default 1), 3: the
        vorticity, 4: the scalar gradient, 5: the vertical velocity, 6: the scalar fluctuation, 7: the quadrants of the scalar fluctuation and v
        (no thresholds).  thresholds: ascending, one fewer than levels; relative: multiplied by (umax - umin) of the indicator first.  The
        indicator of 3, 4, 6, 7 is left in self.txc[0]; self.txc[3..8] are the work space of 3 and self.txc[3] of 4.  q, s, hq, hs and the state
        of the driver are unchanged."""
        from .operators import dns_gate
        return dns_gate(self, opt_cond, thresholds, self.q, self.s, [self.txc[0]] + self.txc[3:9], relative, 1 if scal is None else scal)

    def conditional_moments(self, gate, np, nm=4, p=None):
        """The conditional block of tools/statistics/averages.f90 (opt_main = 4): AVG_N_XZ of U V W (P) Scalar1 .. for every level 1 .. np of
        the int8 tensor gate, from one pass over the gate and the fields.  A dict keyed by the reference's tags: numpy (np, nm, ny) each -- the
        mean and the central moments 2 .. nm per level and plane -- plus "nsample" (np, ny), the points of every level.  No file is written."""
        from .operators import avg_n_xz
        fields = self.q + ([p] if p is not None else []) + self.s
        tags = ["U", "V", "W"] + (["P"] if p is not None else []) + ["Scalar%d" % (i + 1) for i in range(self.nscal)]
        avg, _, ns = avg_n_xz(self.nx, self.ny, self.nz, fields, nm, np, gate, raw=True)
        out = {t: avg[:, i] for i, t in enumerate(tags)}
        out["nsample"] = ns
        return out

    def conditional_averages(self, a, fields=None, nbins=32, ibc=1, gate=None, igate=0, umin=0.0, umax=0.0):
        """CAVG1V_N (statistics/cavg.f90:7) of the field a given each of u, v, w and every scalar (fields: another dict tag -> tensor): a dict
        tag -> numpy (ny + 1, nbins + 2), the averages of a over the nbins bins of the variable and the centres of the first and the last bin
        per plane, the volume last.  ibc = 0: the external interval(s) umin, umax; gate with igate != 0: only points with gate == igate.  No file
        is written."""
        from .operators import cavg1v_n
        if fields is None:
            fields = dict(zip(["u", "v", "w"] + ["s%d" % (i + 1) for i in range(self.nscal)], self.q + self.s))
        out = cavg1v_n(self.nx, self.ny, self.nz, list(fields.values()), a, nbins, ibc, umin, umax, gate, igate)
        return dict(zip(fields, out))

    # ---- the variables of tools/statistics/averages.f90, opt_main 5 .. 8 (:661-762): what the reference puts into vars(:) before AVG_N_XZ ----
    def _new_fields(self, k):
        import torch
        return [torch.empty(self.n, dtype=torch.float64, device=self.q[0].device) for _ in range(k)]

    def invariants(self):
        """opt_main = 8 (averages.f90:756-762): {"InvariantP", "InvariantQ", "InvariantR"} as device tensors, from nine derivatives into
        self.txc[0..8] and one pass over them (the reference: 23 OPR_Partial calls).  q, s, hq, hs and the state of the driver are unchanged."""
        from .operators import fi_maps
        r = fi_maps(self, self.q, None, ["P", "Q", "R"], self.txc[:9], out=self._new_fields(3))
        return {"InvariantP": r["P"], "InvariantQ": r["Q"], "InvariantR": r["R"]}

    def enstrophy_equation(self):
        """opt_main = 5 (averages.f90:661-685), incompressible, without the Baroclinic entry (FI_VORTICITY_BAROCLINIC is not built): a dict keyed
        by the reference's tags with device tensors -- EnstrophyW_iW_i, LnEnstrophyW_iW_i, ProductionW_iW_jS_ij, DiffusionNuW_iLapW_i (visc x
        FI_VORTICITY_DIFFUSION), DilatationMsW_iW_iDivU (P x enstrophy) and RateAN_iN_jS_ij (production / enstrophy).  The nine gradients are
        taken ONCE for the enstrophy, its production and the dilatation (self.txc[0..8]); the diffusion term then makes the reference's calls
        with self.txc[0..5] as its work space.  q, s, hq, hs and the state of the driver are unchanged."""
        import torch
        from .operators import fi_diffusion, fi_maps
        r = fi_maps(self, self.q, None, ["VORTICITY", "VORTICITY_PRODUCTION", "P"], self.txc[:9], out=self._new_fields(3))
        ens, prod = r["VORTICITY"], r["VORTICITY_PRODUCTION"]
        dif = fi_diffusion(self, "VORTICITY_DIFFUSION", self.q, None, self._new_fields(1)[0], self.txc[:6])
        return {"EnstrophyW_iW_i": ens, "LnEnstrophyW_iW_i": torch.log(ens), "ProductionW_iW_jS_ij": prod, "DiffusionNuW_iLapW_i": self.visc * dif,
                "DilatationMsW_iW_iDivU": r["P"] * ens, "RateAN_iN_jS_ij": prod / ens}

    def strain_equation(self, p=None):
        """opt_main = 6 (averages.f90:696-721): Strain2S_ijS_i (2 x FI_STRAIN), LnStrain2S_ijS_i, ProductionMs2S_ijS_jkS_ki (2 x
        FI_STRAIN_PRODUCTION), DiffusionNuS_ijLapS_ij ((2 visc) x FI_STRAIN_DIFFUSION) and Pressure2S_ijP_ij (2 x FI_STRAIN_PRESSURE) as device
        tensors.  p: the pressure; None takes FI_PRESSURE_BOUSSINESQ first, into an array of the method's.  Strain and production share one
        pass over the nine gradients (self.txc[0..8]); the two composed terms use self.txc[0..5].  q, s, hq, hs are unchanged."""
        import torch
        from .operators import fi_diffusion, fi_maps
        if p is None:
            p = self.FI_PRESSURE_BOUSSINESQ(torch.empty(self.isize_txc_field, dtype=torch.float64, device=self.q[0].device))
        prs = fi_diffusion(self, "STRAIN_PRESSURE", self.q, p, self._new_fields(1)[0], self.txc[:6])
        r = fi_maps(self, self.q, None, ["STRAIN", "STRAIN_PRODUCTION"], self.txc[:9], out=self._new_fields(2))
        dif = fi_diffusion(self, "STRAIN_DIFFUSION", self.q, None, self._new_fields(1)[0], self.txc[:6])
        strain2 = 2.0 * r["STRAIN"]
        return {"Strain2S_ijS_i": strain2, "LnStrain2S_ijS_i": torch.log(strain2), "ProductionMs2S_ijS_jkS_ki": 2.0 * r["STRAIN_PRODUCTION"],
                "DiffusionNuS_ijLapS_ij": (2.0 * self.visc) * dif, "Pressure2S_ijP_ij": 2.0 * prs}

    def scalar_gradient_equation(self, iscal=0):
        """opt_main = 7 (averages.f90:731-746) for scalar iscal (0-based): GradientG_iG_i, LnGradientG_iG_i, ProductionMsG_iG_jS_ij,
        DiffusionNuG_iLapG_i (FI_GRADIENT_DIFFUSION x visc / schmidt[iscal]) and StrainAMsN_iN_jS_ij (production / gradient, as the reference
        computes that entry) as device tensors.  Gradient and production share one pass over twelve derivatives (self.txc[0..8] and three
        arrays of the method's).  q, s, hq, hs are unchanged."""
        import torch
        from .operators import fi_diffusion, fi_maps
        s = self.s[iscal]
        r = fi_maps(self, self.q, s, ["GRADIENT", "GRADIENT_PRODUCTION"], self.txc[:9], self._new_fields(3), self._new_fields(2))
        grad, prod = r["GRADIENT"], r["GRADIENT_PRODUCTION"]
        dif = fi_diffusion(self, "GRADIENT_DIFFUSION", None, s, self._new_fields(1)[0], self.txc[:6])
        # (a device operand: torch divides by a host number through its reciprocal, which is not the reference's division)
        schmidt = torch.tensor(float(self.schmidt[iscal]), dtype=torch.float64, device=dif.device)
        return {"GradientG_iG_i": grad, "LnGradientG_iG_i": torch.log(grad), "ProductionMsG_iG_jS_ij": prod,
                "DiffusionNuG_iLapG_i": torch.div(dif * self.visc, schmidt), "StrainAMsN_iN_jS_ij": prod / grad}

    def spectra(self, mode="spectra", cross=False, nblock=1, p=None, out2d=False):
        """tools/statistics/spectra.f90, opt_main 1-4, for the fields of the driver, without its files: mode "spectra" (power and co-spectra)
        or "correlations", cross False (every variable with itself: u, v, w, (p,) and the scalars) or True (uv, uw, vw and us, vs, ws per
        scalar), sums over blocks of nblock planes.  p: a pressure field, or True to take FI_PRESSURE_BOUSSINESQ first, as the tool does.
        A dict keyed by the reference's variable names (Euu, Evv, .., E11, or Cuv, ..); each entry holds numpy "x" (ny/nblock, nx/2 or nx),
        "z" (ny/nblock, nz/2 or nz), "r" (ny/nblock, kr_total: min(nx, nz) for cross-correlations, min(nx/2, nz/2) otherwise) where the
        reference writes it (nx == nz for spectra, equal x and z spacing for correlations), with
        out2d "xz", all after the reference's 1/nblock (:683-690) and, for radial correlations, the division by the sample size (:709-722);
        "cov" (3, ny), "variance" (ny,) and "parseval" = max |variance - cov[0]| over the planes kept (:662-666).  txc[0], [1], [3..5] are
        the work space; q, s, hq, hs and the state of the driver are unchanged."""
        import torch
        from .operators import radial_samplesize
        m = {"spectra": 1, "correlations": 2}.get(mode)
        if m is None:
            raise TlabError('mode: "spectra" or "correlations"')
        if p is True:
            p = self.FI_PRESSURE_BOUSSINESQ()
        nx, ny, nz, nyo = self.nx, self.ny, self.nz, self.ny // max(int(nblock), 1)
        n1, nz1 = (nx // 2, nz // 2) if m == 1 else (nx, nz)
        kr = min(nx, nz) if (m == 2 and cross) else min(nx // 2, nz // 2)     # kr_total, :271-282: the full length for cross-correlations only
        var = ["u", "v", "w"] + (["p"] if p is not None else []) + [str(i + 1) for i in range(self.nscal)]
        if not cross:
            pairs = [(a, a) for a in var]
        else:
            pairs = [("u", "v"), ("u", "w"), ("v", "w")] + [(a, str(i + 1)) for i in range(self.nscal) for a in "uvw"]
        npairs = len(pairs)
        dev = self.q[0].device
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)      # noqa: E731
        ox, oz, orr = z(npairs, nyo, n1), z(npairs, nyo, nz1), z(npairs, nyo, kr)
        o2 = z(npairs, nz, nyo, n1) if out2d else None
        cov, variance = np.zeros((npairs, 3, ny)), np.zeros((npairs, ny))
        _use_torch_stream()
        q, s, _, _, txc = self._arrays()
        check(load().tlab_dns_spectra(self._h, m, int(bool(cross)), int(nblock), kr, q, s, txc, p.data_ptr() if p is not None else None,
                                      o2.data_ptr() if out2d else None, ox.data_ptr(), oz.data_ptr(), orr.data_ptr(), cov.ctypes.data,
                                      variance.ctypes.data), "tlab_dns_spectra")
        # icalc_radial, :406-408: g(1)%jac(1, 1) == g(3)%jac(1, 1) there; here the two uniform spacings, equal up to the rounding of the nodes
        radial = nx == nz if m == 1 else abs(self._dxz[0] - self._dxz[1]) <= 1.0e-12 * max(abs(self._dxz[0]), abs(self._dxz[1]))
        scale = 1.0 / float(nblock) if nblock > 1 else 1.0                  # :684-690
        ox, oz, orr = ox.cpu().numpy() * scale, oz.cpu().numpy() * scale, orr.cpu().numpy() * scale
        if m == 2 and radial:
            ss = radial_samplesize(nx, nz, kr)
            orr = orr * np.where(ss > 0.0, 1.0 / np.where(ss > 0.0, ss, 1.0), ss)[None, None, :]      # :709-722
        res, ny_loc = {}, nyo * int(nblock)
        for i, (a, b) in enumerate(pairs):
            e = {"x": ox[i], "z": oz[i], "cov": cov[i], "variance": variance[i],
                 "parseval": float(np.abs(variance[i, :ny_loc] - cov[i, 0, :ny_loc]).max())}
            if radial:
                e["r"] = orr[i]
            if out2d:
                e["xz"] = o2[i].cpu().numpy() * scale
            res[("E" if m == 1 else "C") + a + b] = e
        return res

    def profile_derivative(self, profiles):
        """OPR_Partial_Y(OPR_P1, 1, jmax, 1, bcs, g(2), ..) of profiles (numpy (n, ny)) with the driver's y plan: numpy (n, ny).  The line
        kernels have no test on a box of one line, so profile i is replicated along x into plane i of a box (nx, ny, n) -- lines of the length
        every substep runs -- and line 0 of each plane is returned."""
        import torch
        from .operators import OPR_Partial_Y, OPR_P1
        prof = np.atleast_2d(np.asarray(profiles, dtype=np.float64))
        n = prof.shape[0]
        box = np.ascontiguousarray(np.broadcast_to(prof[:, :, None], (n, self.ny, self.nx)))
        a = torch.from_numpy(box.reshape(-1)).to(self.q[0].device)
        res = torch.empty_like(a)
        OPR_Partial_Y(OPR_P1, self.nx, self.ny, n, 0, self.g[1], a, res)
        return np.ascontiguousarray(res.cpu().numpy().reshape(n, self.ny, self.nx)[:, :, 0])

    def flow_gradient_stats(self, p=None):
        """Section 3 of AVG_FLOW_XZ (avg_flow_xz.f90:976-1248, with p also :670-699), incompressible, constant transport: the nine velocity
        derivatives into self.txc (which hold dudx .. dwdz on return) and the plane statistics on them.  A dict keyed by
        operators.FLOW_GRADIENTS (with p also FLOW_GRADIENTS_P and "ugradp"): the finished profiles of the reference -- Phi, Tau_yy, Tau_xy,
        Tau_yz, Exx .. Eyz, PIxx, PIyy, PIzz after its host lines (:1140, :1187-1203, :1263-1268, :687-689) with the driver's visc -- and the
        raw columns of those under "<name>_raw"; plus the means rU rV rW (rP) and rU_y rV_y rW_y."""
        from .operators import FLOW_GRADIENTS, FLOW_GRADIENTS_P
        _use_torch_stream()
        m = self.plane_means()
        rP = self.AVG_IK_V(p) if p is not None else None
        rU_y, rV_y, rW_y = self.profile_derivative([m["rU"], m["rV"], m["rW"]])
        q, _, _, _, txc = self._arrays()
        ny = self.ny
        out = np.zeros((57 if p is not None else 50, ny))
        prof = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        check(load().tlab_dns_avg_gradients_flow(self._h, q, p.data_ptr() if p is not None else None, txc, prof(m["rU"]), prof(m["rV"]),
                                                 prof(m["rW"]), prof(rP) if p is not None else None, prof(rU_y), prof(rV_y), prof(rW_y),
                                                 prof(out), ny), "tlab_dns_avg_gradients_flow")
        names = FLOW_GRADIENTS + (FLOW_GRADIENTS_P if p is not None else ())
        r = dict(zip(names, out))
        visc, c23 = self.visc, 2.0 / 3.0
        for k in ("Phi", "Tau_yy", "Tau_xy", "Tau_yz", "Exx", "Eyy", "Ezz", "Exy", "Exz", "Eyz") + (("PIxx", "PIyy", "PIzz") if p is not None else ()):
            r[k + "_raw"] = r[k]
        r["Phi"] = r["Phi_raw"] * visc * 2.0                                         # :1140
        r["Tau_yy"] = r["Tau_yy_raw"] * visc * c23                                   # :1187
        r["Tau_xy"] = r["Tau_xy_raw"] * visc                                         # :1195
        r["Tau_yz"] = r["Tau_yz_raw"] * visc                                         # :1203
        r["Exx"] = (r["Exx_raw"] * visc - r["Tau_xy"] * rU_y) * 2.0                  # :1263-1268
        r["Eyy"] = (r["Eyy_raw"] * visc - r["Tau_yy"] * rV_y) * 2.0
        r["Ezz"] = (r["Ezz_raw"] * visc - r["Tau_yz"] * rW_y) * 2.0
        r["Exy"] = r["Exy_raw"] * visc - r["Tau_xy"] * rV_y - r["Tau_yy"] * rU_y
        r["Exz"] = r["Exz_raw"] * visc - r["Tau_xy"] * rW_y - r["Tau_yz"] * rU_y
        r["Eyz"] = r["Eyz_raw"] * visc - r["Tau_yy"] * rW_y - r["Tau_yz"] * rV_y
        if p is not None:
            for k in ("PIxx", "PIyy", "PIzz"):
                r[k] = r[k + "_raw"] * 2.0                                           # :687-689
            r["ugradp"] = out[56]
            r["rP"] = rP
        r.update(rU=m["rU"], rV=m["rV"], rW=m["rW"], rU_y=rU_y, rV_y=rV_y, rW_y=rW_y)
        return r

    def scal_gradient_stats(self, is_, p=None):
        """The gradient groups of scalar is_ (0-based) in AVG_SCAL_XZ (avg_scal_xz.f90:451-453, :607-610, :714-756), incompressible (fS = rS,
        fS_y = rS_y): dsdx dsdy dsdz into self.txc[0..2] and the plane statistics on them.  A dict keyed by operators.SCAL_GRADIENTS (with p
        also SCAL_GRADIENTS_P): Ess finished (Ess*diff*2, diff = visc / schmidt, :610) with the raw column under "Ess_raw"; plus the means."""
        from .operators import SCAL_GRADIENTS, SCAL_GRADIENTS_P
        _use_torch_stream()
        m = self.plane_means()
        rP = self.AVG_IK_V(p) if p is not None else None
        rS = m["rS"][is_]
        rS_y = self.profile_derivative([rS])[0]
        q, _, _, _, txc = self._arrays()
        ny = self.ny
        out = np.zeros((18 if p is not None else 15, ny))
        prof = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        check(load().tlab_dns_avg_gradients_scal(self._h, self.s[is_].data_ptr(), q, p.data_ptr() if p is not None else None, txc, prof(rS),
                                                 prof(m["rU"]), prof(m["rV"]), prof(m["rW"]), prof(rP) if p is not None else None, prof(rS_y),
                                                 prof(rS_y) if p is not None else None, prof(out), ny), "tlab_dns_avg_gradients_scal")
        r = dict(zip(SCAL_GRADIENTS + (SCAL_GRADIENTS_P if p is not None else ()), out))
        r["Ess_raw"] = r["Ess"]
        r["Ess"] = r["Ess_raw"] * (self.visc / float(self.schmidt[is_])) * 2.0      # :610
        r.update(rS=rS, rU=m["rU"], rV=m["rV"], rW=m["rW"], rS_y=rS_y)
        if p is not None:
            r["rP"] = rP
        return r

    def begin_step(self):
        """hq = hs = 0 of TIME_RUNGEKUTTA (time.f90:212-216) without touching the arrays: the next substep overwrites them."""
        check(load().tlab_dns_begin_step(self._h), "tlab_dns_begin_step")
        if self.l_hq is not None and self.np > 0:      # l_hq = 0 (time.f90:215): the particle substep accumulates onto it
            _use_torch_stream()
            for t in self.l_hq:
                check(load().tlab_pw_fill(t.data_ptr(), 0.0, self.np), "tlab_pw_fill")

    def place_arrays(self, pool=40, random_trials=16, dtime=1e-3, seed=0):
        """tlab_dns_place_arrays: q, s, hq, hs, txc move to the allocations (out of a pool of `pool` fresh ones of the txc size) on which the substep runs
        fastest; the fields keep their values, the tendencies are zeroed.  Returns {"ms_first", "ms_best", "ms_median", "ms_worst", "trials", "pool",
        "seconds"}: ms_first / ms_best from the repeats at the end of the search (the allocator's order and the assignment kept, three steps each, back
        to back), median / worst over the single timings of the search."""
        import time
        import torch
        nroles = 2 * (3 + self.nscal) + 9
        m = self.isize_txc_field
        t0 = time.perf_counter()
        state = [t.clone() for t in self.q + self.s]
        dev = self.q[0].device
        self.q = self.s = self.hq = self.hs = self.txc = self._ptrs = None       # the driver's own arrays go back to the allocator before the pool is made
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        pool = max(nroles, min(int(pool), int(0.7 * free / (8.0 * m))))
        cand = []
        try:
            for _ in range(pool):
                cand.append(torch.zeros(m, dtype=torch.float64, device=dev))
        except RuntimeError:      # out of memory: search among what there is (at least the roles themselves must fit, as they did before)
            for _ in range(min(4, max(0, len(cand) - nroles))):      # some headroom for what else the run allocates
                cand.pop()
            torch.cuda.empty_cache()
            if len(cand) < nroles:
                # not even the roles fit beside the saved state: the driver gets arrays of its original sizes back, with its fields, before the error leaves
                cand = None
                torch.cuda.empty_cache()
                ns = self.nscal
                self.q = [r for r in state[:3]]
                self.s = [r for r in state[3:3 + ns]]
                self.hq = [torch.zeros(self.n, dtype=torch.float64, device=dev) for _ in range(3)]
                self.hs = [torch.zeros(self.n, dtype=torch.float64, device=dev) for _ in range(ns)]
                self.txc = [torch.zeros(m, dtype=torch.float64, device=dev) for _ in range(9)]
                self._ptrs = None
                raise
            pool = len(cand)
        parr = (c_vp * pool)(*[t.data_ptr() for t in cand])
        sarr = (c_vp * len(state))(*[t.data_ptr() for t in state])
        assign = (ctypes.c_int * nroles)()
        rep = (ctypes.c_double * 5)()
        _use_torch_stream()
        rc = load().tlab_dns_place_arrays(self._h, pool, parr, sarr, float(dtime), int(random_trials), int(seed), assign, rep)
        if rc != 0:      # the driver stays usable: the pool in order
            for i in range(nroles):
                assign[i] = i
        a = [cand[i] for i in assign]
        ns = self.nscal
        self.q, self.s = [t[: self.n] for t in a[0:3]], [t[: self.n] for t in a[3:3 + ns]]
        self.hq, self.hs = [t[: self.n] for t in a[3 + ns:6 + ns]], [t[: self.n] for t in a[6 + ns:6 + 2 * ns]]
        self.txc = a[6 + 2 * ns:]
        self._ptrs = None
        for t, r in zip(self.q + self.s, state):
            t.copy_(r)
        for t in self.hq + self.hs:
            t.zero_()
        del cand, state, a
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        check(rc, "tlab_dns_place_arrays")
        return {"ms_first": rep[0], "ms_best": rep[1], "ms_median": rep[2], "ms_worst": rep[3], "trials": int(rep[4]), "pool": pool,
                "seconds": time.perf_counter() - t0}

    # ---- sampling between two statistics steps: towers (dns_main.f90:300-303), phase averages (:282-298), saved planes (planes.f90) ----
    def set_towers(self, stride, nitera_save):
        """[SaveTowers] Stride: DNS_TOWER_INITIALIZE (tools/dns/dns_tower.f90:62).  The buffer (device, the reference's layout) holds nitera_save
        time steps; the host writes it (DNS_TOWER_WRITE on a copy) and calls tower_reset."""
        import torch
        from .operators import Tower
        if self.nscal < 1:
            raise TlabError("the towers take the first scalar (DNS_TOWER_ACCUMULATE(s, 2)): nscal must be at least 1")
        self.tower = Tower(self.nx, self.ny, self.nz, stride, nitera_save)
        self.tower_buf = torch.zeros(self.tower.bufsize, dtype=torch.float64, device=self.q[0].device)

    def tower_accumulate(self, itime=0, rtime=0.0):
        """DNS_TOWER_ACCUMULATE(q, 1) and (s, 2) after a time step (dns_main.f90:300-303); the pressure (index 4) was taken inside the last substep
        (TIME_RUNGEKUTTA with itime).  No synchronisation."""
        self.tower.accumulate(1, self.q, itime, rtime, self.tower_buf)
        self.tower.accumulate(2, self.s[:1], itime, rtime, self.tower_buf)

    def tower_buffer(self):
        """tower_buf (device) -- Tower.views names its parts"""
        return self.tower_buf

    def tower_reset(self):
        self.tower.reset()

    def set_phase_average(self, stride, nitera_first, nitera_save):
        """[Iteration] PhaseAvg: AvgPhaseInitializeMemory (statistics/avg_phase.f90:54-98) -- avg_planes = nitera_save / stride, and avg_flow, avg_scal,
        avg_p, avg_stress zeroed on the device, (fields, avg_planes + 1, ny, nx)"""
        import torch
        self.phase = {"stride": int(stride), "first": int(nitera_first), "save": int(nitera_save), "planes": int(nitera_save) // int(stride)}
        if self.phase["planes"] < 1:
            raise TlabError("nitera_save / stride must be at least 1")
        shape = (self.phase["planes"] + 1, self.ny, self.nx)
        z = lambda nf: torch.zeros((nf,) + shape, dtype=torch.float64, device=self.q[0].device)      # noqa: E731
        self.avg_flow, self.avg_scal, self.avg_p, self.avg_stress = z(3), z(max(self.nscal, 1)), z(1), z(6)

    def _phase_plane(self, itr):
        from .operators import avg_phase_plane_id
        return avg_phase_plane_id(itr, self.phase["first"], self.phase["save"] // self.phase["stride"])

    def phase_average(self, itime):
        """dns_main.f90:282-288 after time step itime: if mod(itime, stride) == 0, AvgPhaseSpace of q and s and AvgPhaseStress (u, v, w read once).
        True when the step was sampled.  The files and AvgPhaseResetVariable (phase_reset) stay with the caller."""
        from .operators import avg_phase_flow, avg_phase_space
        ph = self.phase
        if itime % ph["stride"] != 0:
            return False
        pid = self._phase_plane(itime // ph["stride"])
        avg_phase_flow(self.nx, self.ny, self.nz, self.q[0], self.q[1], self.q[2], ph["planes"], pid, self.avg_flow, self.avg_stress)
        if self.nscal:
            avg_phase_space(self.nx, self.ny, self.nz, self.s, ph["planes"], pid, self.avg_scal)
        return True

    def phase_buffers(self):
        return {"flow": self.avg_flow, "scal": self.avg_scal, "p": self.avg_p, "stress": self.avg_stress}

    def phase_reset(self):
        """AvgPhaseResetVariable (statistics/avg_phase.f90:453-470)"""
        for a in (self.avg_flow, self.avg_scal, self.avg_p, self.avg_stress):
            a.zero_()

    def _arm_pressure_sampling(self, itime, rtime):
        """rhs_global_incompressible_1.f90:292-305 for the last substep of step itime: the towers take the pressure at itime, the phase average
        at (itime + 1) / stride when mod(itime + 1, stride) == 0"""
        tower = getattr(self, "tower", None)
        ph = getattr(self, "phase", None)
        due = ph is not None and (itime + 1) % ph["stride"] == 0
        if tower is None and not due:
            return
        _use_torch_stream()
        check(load().tlab_dns_arm_pressure_sampling(
            self._h, tower._h if tower is not None else None, self.tower_buf.data_ptr() if tower is not None else None, int(itime),
            float(0.0 if rtime is None else rtime), self.avg_p.data_ptr() if due else None, ph["planes"] if due else 0,
            self._phase_plane((itime + 1) // ph["stride"]) if due else 0), "tlab_dns_arm_pressure_sampling")

    def PLANES_SAVE(self, iplanes=(), jplanes=(), kplanes=(), log=False, single=True):
        """PLANES_SAVE (tools/dns/planes.f90:213) without its files: (data_i, data_j, data_k) as device tensors (nz, size, ny), (nz, size, nx), (size,
        ny, nx), None for an empty list of nodes (1-based).  The variables run [u, v, w, scalars..., p, log10 enstrophy, log10 grad s...] (the last
        group with log, PLANES_LOG); p from FI_PRESSURE_BOUSSINESQ, the enstrophy from FI_VORTICITY.  single: float32 (IO_TYPE_SINGLE).  self.txc is
        the work space."""
        from .operators import fi_gradient, log10_small, planes_gather
        n = self.n
        p = self.FI_PRESSURE_BOUSSINESQ()                                  # self.txc[2]
        fields = self.q + self.s + [p[:n]]
        if log:
            if self.nscal > 5:
                raise TlabError("PLANES_SAVE(log=True) has work arrays for five scalars")
            fields.append(log10_small(self.FI_VORTICITY()[:n]))            # self.txc[0]; self.txc[3..8] are free again
            for i in range(self.nscal):
                fields.append(log10_small(fi_gradient(self, self.s[i], self.txc[3 + i], self.txc[8])[:n]))
        gather = lambda idir, nodes: planes_gather(self.nx, self.ny, self.nz, fields, idir, nodes, single=single) if len(nodes) else None      # noqa: E731
        return gather(1, iplanes), gather(2, jplanes), gather(3, kplanes)

    def TIME_RUNGEKUTTA(self, dtime, itime=None, rtime=None):
        """One time step: hq = hs = 0 (and l_hq = 0), then rkm_endstep substeps, each with the particle substep first when particles are set
        (time.f90:212-304).  itime (the iteration before the step, as TLab_Time holds it inside TIME_RUNGEKUTTA) and rtime: with towers or a phase
        average set, the last substep samples its pressure (rkm_substep == rkm_endstep, rhs_global_incompressible_1.f90:292-305).  Without itime
        nothing is sampled."""
        self.begin_step()
        for k in range(self.rkm_endstep):
            last = k == self.rkm_endstep - 1
            if self.l_q is not None:
                self.TIME_SUBSTEP_PARTICLE(dtime * self.kdt[k], 1.0 if last else self.kco[k], not last)
            if last and itime is not None:
                self._arm_pressure_sampling(itime, rtime)
            self.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dtime * self.kdt[k], 1.0 if last else self.kco[k], not last)

    def __del__(self):
        try:
            if self._h:
                load().tlab_dns_destroy(self._h)
        except Exception:
            pass
