"""numpy restatement of the groups of AVG_FLOW_XZ (statistics/avg_flow_xz.f90:673-699, :988-1248) and AVG_SCAL_XZ (statistics/avg_scal_xz.f90:451-453,
:607, :714-745) that work on derivative fields, incompressible branch, constant transport (no vis factor).  The derivatives are handed in.

Conventions of tests/averages_oracle.py: fields a3[k, j, i], a plane summed sequentially over i then k, ONE division; every term in the reference's
operation order, left to right as written there (numpy neither fuses nor reorders); an integer power is the product gfortran makes (a**2 = a*a), the
chains p = a*a; p = p*a; p = p*a stay chains.  A term is RAW: before any visc, diff, c23 or 2.0 the reference applies to the profile on the host;
finish_flow / finish_scal restate those host lines."""
import numpy as np

from averages_oracle import avg_ik_v, plane_sums, _fluct      # noqa: F401  (plane_sums: the bound of the GPU test)

C23 = 2.0 / 3.0
GRAD = ("dudx", "dudy", "dudz", "dvdx", "dvdy", "dvdz", "dwdx", "dwdy", "dwdz")
_CH = ("U_x", "V_y", "W_z", "U_y", "U_z", "V_x", "V_z", "W_x", "W_y")
FLOW1_NAMES = ("vortx", "vorty", "vortz", "Tau_yy", "Tau_xy", "Tau_yz")
FLOW2_NAMES = tuple("%s%d" % (n, k) for n in _CH for k in (2, 3, 4)) + ("U_ii2", "vortx2", "vorty2", "vortz2", "Phi", "Exx", "Eyy", "Ezz", "Exy", "Exz", "Eyz")
FLOW3_NAMES = ("Txxy_v", "Tyyy_v", "Tzzy_v", "Txyy_v", "Txzy_v", "Tyzy_v")
FLOW_GRAD_NAMES = FLOW1_NAMES + FLOW2_NAMES + FLOW3_NAMES
FLOW_GRAD_NAMES_P = ("PIxx", "PIyy", "PIzz", "PIxy", "PIxz", "PIyz")
SCAL1_NAMES = ("Fy", "Ess", "S_x2", "S_y2", "S_z2", "S_x3", "S_y3", "S_z3", "S_x4", "S_y4", "S_z4")
SCAL2_NAMES = ("Tssy2", "Tsuy2_d", "Tsvy2_d", "Tswy2_d")
SCAL_GRAD_NAMES = SCAL1_NAMES + SCAL2_NAMES
SCAL_GRAD_NAMES_P = ("PIsu", "PIsv", "PIsw")


def _chain(a):
    p2 = a * a
    p3 = p2 * a
    return p2, p3, p3 * a


def flow_terms1(g):
    """g: the nine derivatives in the order of GRAD.  vorticity (:991-1006) and the raw stresses (:1181-1197)"""
    dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz = g
    return {"vortx": dwdy - dvdz, "vorty": dudz - dwdx, "vortz": dvdx - dudy,
            "Tau_yy": dvdy * 2.0 - dudx - dwdz, "Tau_xy": dudy + dvdx, "Tau_yz": dvdz + dwdy}


def flow_terms2(g, rU_y, rV_y, rW_y, vortx, vorty, vortz):
    """:993-1176: the derivative moments, the dilatation fluctuation, the vorticity variances, Phi and the dissipation terms, raw"""
    dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz = g
    t = {}
    for name, a in zip(_CH, (dudx, _fluct(dvdy, rV_y), dwdz, _fluct(dudy, rU_y), dudz, dvdx, dvdz, dwdx, _fluct(dwdy, rW_y))):
        t[name + "2"], t[name + "3"], t[name + "4"] = _chain(a)
    d = dudx + dvdy + dwdz
    t["U_ii2"] = _fluct(d, rV_y) * _fluct(d, rV_y)
    for name, o, m in (("vortx2", dwdy - dvdz, vortx), ("vorty2", dudz - dwdx, vorty), ("vortz2", dvdx - dudy, vortz)):
        f = _fluct(o, m)
        t[name] = f * f
    sq = lambda a: a * a      # noqa: E731
    t["Phi"] = sq(dudx) + sq(dvdy) + sq(dwdz) + 0.5 * (sq(dudy + dvdx) + sq(dudz + dwdx) + sq(dvdz + dwdy)) - sq(dudx + dvdy + dwdz) / 3.0
    p = (dudx + dvdy + dwdz) * C23
    t["Exx"] = (dudx * 2.0 - p) * dudx + (dudy + dvdx) * dudy + (dudz + dwdx) * dudz
    t["Eyy"] = (dvdy * 2.0 - p) * dvdy + (dudy + dvdx) * dvdx + (dvdz + dwdy) * dvdz
    t["Ezz"] = (dwdz * 2.0 - p) * dwdz + (dwdy + dvdz) * dwdy + (dwdx + dudz) * dwdx
    t["Exy"] = ((dudx * 2.0 - p) * dvdx + (dudy + dvdx) * dvdy + (dudz + dwdx) * dvdz
                + (dvdy * 2.0 - p) * dudy + (dudy + dvdx) * dudx + (dvdz + dwdy) * dudz)
    t["Exz"] = ((dudx * 2.0 - p) * dwdx + (dudy + dvdx) * dwdy + (dudz + dwdx) * dwdz
                + (dwdz * 2.0 - p) * dudz + (dudz + dwdx) * dudx + (dvdz + dwdy) * dudy)
    t["Eyz"] = ((dvdy * 2.0 - p) * dwdy + (dudy + dvdx) * dwdx + (dvdz + dwdy) * dwdz
                + (dwdz * 2.0 - p) * dvdz + (dudz + dwdx) * dvdx + (dvdz + dwdy) * dvdy)
    assert tuple(t) == FLOW2_NAMES
    return t


def flow_terms3(g, u, v, w, p, Tau_yy, Tau_xy, Tau_yz, fU, fV, fW, rP):
    """:1185-1245 (Tau_* raw: the averages of flow_terms1) and with p the pressure strain (:681-699)"""
    dudx, dudy, dudz, dvdx, dvdy, dvdz, dwdx, dwdy, dwdz = g
    t22 = _fluct(dvdy * 2.0 - dudx - dwdz, Tau_yy) * C23
    t12 = _fluct(dudy + dvdx, Tau_xy)
    t23 = _fluct(dvdz + dwdy, Tau_yz)
    up, vp, wp = _fluct(u, fU), _fluct(v, fV), _fluct(w, fW)
    t = {"Txxy_v": t12 * up, "Tyyy_v": t22 * vp, "Tzzy_v": t23 * wp,
         "Txyy_v": t22 * up + t12 * vp, "Txzy_v": t23 * up + t12 * wp, "Tyzy_v": t23 * vp + t22 * wp}
    if p is not None:
        pp = _fluct(p, rP)
        t.update(PIxx=pp * dudx, PIyy=pp * dvdy, PIzz=pp * dwdz, PIxy=pp * (dudy + dvdx), PIxz=pp * (dudz + dwdx), PIyz=pp * (dvdz + dwdy))
    return t


def ugradp_term(u, v, w, dpdx, dpdy, dpdz):
    return u * dpdx + v * dpdy + w * dpdz                                  # :673


def flow_averages(g, u, v, w, p, fU, fV, fW, rP, rU_y, rV_y, rW_y, first=None):
    """the 50 (56) profiles of the three passes, a dict in column order.  first: the six profiles of the first pass to use as means in place of
    this restatement's own (a test hands the device's)"""
    a1 = {k: avg_ik_v(t) for k, t in flow_terms1(g).items()}
    m = a1 if first is None else dict(zip(FLOW1_NAMES, first))
    r = dict(a1)
    r.update({k: avg_ik_v(t) for k, t in flow_terms2(g, rU_y, rV_y, rW_y, m["vortx"], m["vorty"], m["vortz"]).items()})
    r.update({k: avg_ik_v(t) for k, t in flow_terms3(g, u, v, w, p, m["Tau_yy"], m["Tau_xy"], m["Tau_yz"], fU, fV, fW, rP).items()})
    return r


def scal_terms1(gs, rS_y):
    dsdx, dsdy, dsdz = gs
    t = {"Fy": dsdy, "Ess": dsdx * dsdx + dsdy * dsdy + dsdz * dsdz}           # avg_scal_xz.f90:738, :607
    cx, cy, cz = _chain(dsdx), _chain(_fluct(dsdy, rS_y)), _chain(dsdz)          # :711-730
    for k in range(3):
        t["S_x%d" % (k + 2)], t["S_y%d" % (k + 2)], t["S_z%d" % (k + 2)] = cx[k], cy[k], cz[k]
    assert tuple(t) == SCAL1_NAMES
    return t


def scal_terms2(gs, s, u, v, w, p, Fy, fS, fU, fV, fW, rP, fS_y):
    dsdx, dsdy, dsdz = gs
    f = _fluct(dsdy, Fy)
    t = {"Tssy2": f * _fluct(s, fS), "Tsuy2_d": f * _fluct(u, fU), "Tsvy2_d": f * _fluct(v, fV), "Tswy2_d": f * _fluct(w, fW)}      # :742-745
    if p is not None:
        pp = _fluct(p, rP)
        t.update(PIsu=pp * dsdx, PIsv=pp * _fluct(dsdy, fS_y), PIsw=pp * dsdz)                                                   # :451-453
    return t


def scal_averages(gs, s, u, v, w, p, fS, fU, fV, fW, rP, rS_y, fS_y, first=None):
    a1 = {k: avg_ik_v(t) for k, t in scal_terms1(gs, rS_y).items()}
    Fy = a1["Fy"] if first is None else first
    r = dict(a1)
    r.update({k: avg_ik_v(t) for k, t in scal_terms2(gs, s, u, v, w, p, Fy, fS, fU, fV, fW, rP, fS_y).items()})
    return r


def finish_flow(r, visc, rU_y, rV_y, rW_y):
    """the reference's host lines on the raw profiles (:1140, :1187-1203, :1263-1268, :687-689): a dict of the finished ones"""
    f = {"Phi": r["Phi"] * visc * 2.0, "Tau_yy": r["Tau_yy"] * visc * C23, "Tau_xy": r["Tau_xy"] * visc, "Tau_yz": r["Tau_yz"] * visc}
    f["Exx"] = (r["Exx"] * visc - f["Tau_xy"] * rU_y) * 2.0
    f["Eyy"] = (r["Eyy"] * visc - f["Tau_yy"] * rV_y) * 2.0
    f["Ezz"] = (r["Ezz"] * visc - f["Tau_yz"] * rW_y) * 2.0
    f["Exy"] = r["Exy"] * visc - f["Tau_xy"] * rV_y - f["Tau_yy"] * rU_y
    f["Exz"] = r["Exz"] * visc - f["Tau_xy"] * rW_y - f["Tau_yz"] * rU_y
    f["Eyz"] = r["Eyz"] * visc - f["Tau_yy"] * rW_y - f["Tau_yz"] * rV_y
    for k in ("PIxx", "PIyy", "PIzz"):
        if k in r:
            f[k] = r[k] * 2.0
    return f


def finish_scal(r, diff):
    return {"Ess": r["Ess"] * diff * 2.0}                                        # :610
