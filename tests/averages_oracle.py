"""numpy restatement of the plane statistics: AVG_IK_V and AVG1V2D_V of utils/averages.f90 (:301-327, :142-167) and the term fields of
AVG_FLOW_XZ (statistics/avg_flow_xz.f90:513-553, :597-654, incompressible branch) and AVG_SCAL_XZ (statistics/avg_scal_xz.f90:373-455).

Fields are numpy arrays a3[k, j, i] (x fastest, the reference's a(nx, ny, nz)).  A plane is summed in the reference's order: one running sum per
j, sequential over i, then over k (np.cumsum adds strictly left to right), then ONE division by real(nx*nz).  Terms are formed in the reference's
operation order, left to right as written there; numpy neither fuses nor reorders them."""
import math

import numpy as np

FLOW_NAMES = ("Rxx", "Ryy", "Rzz", "Rxy", "Rxz", "Ryz", "rU3", "rU4", "rV3", "rV4", "rW3", "rW4", "Txxy", "Tyyy", "Tzzy", "Txyy", "Txzy", "Tyzy")
FLOW_NAMES_P = ("rP2", "up", "vp", "wp")
SCAL_NAMES = ("rS2", "rS3", "rS4", "Rsu", "Rsv", "Rsw", "Tssy1", "Tsuy1", "Tsvy1", "Tswy1")
SCAL_NAMES_P = ("Tsvy3",)


def plane_sums(t3):
    """sum over (i, k) of every plane j, sequential over i then k"""
    nz, ny, nx = t3.shape
    rows = np.ascontiguousarray(np.transpose(t3, (1, 0, 2))).reshape(ny, nz * nx)
    return np.cumsum(rows, axis=1)[:, -1]


def avg_ik_v(a3):
    nz, ny, nx = a3.shape
    return plane_sums(a3) / float(nx * nz)


def power(a3, imom):
    """a**imom as gfortran expands an integer power"""
    a2 = a3 * a3
    return {1: a3, 2: a2, 3: a2 * a3, 4: a2 * a2}[imom]


def avg1v2d_v(a3, imom):
    return avg_ik_v(power(a3, imom))


def _fluct(a3, mean):
    return a3 - np.asarray(mean)[None, :, None]


def flow_terms(u, v, w, p, fU, fV, fW, rP):
    """the term fields of the FLOW program, a dict in output order (p = None: without the pressure terms)"""
    up, vp, wp = _fluct(u, fU), _fluct(v, fV), _fluct(w, fW)            # dwdx, dwdy, dwdz (:514-516)
    t = {"Rxx": up * up, "Ryy": vp * vp, "Rzz": wp * wp, "Rxy": up * vp, "Rxz": up * wp, "Ryz": vp * wp}
    t["rU3"] = up * up * up
    t["rU4"] = up * t["rU3"]
    t["rV3"] = vp * vp * vp
    t["rV4"] = vp * t["rV3"]
    t["rW3"] = wp * wp * wp
    t["rW4"] = wp * t["rW3"]
    t["Txxy"] = up * up * vp
    t["Tyyy"] = vp * vp * vp
    t["Tzzy"] = wp * wp * vp
    t["Txyy"] = up * vp * vp
    t["Txzy"] = up * vp * wp
    t["Tyzy"] = vp * vp * wp
    if p is not None:
        pp = _fluct(p, rP)                                             # dvdz (:640)
        t["rP2"] = pp * pp
        t["up"] = up * pp
        t["vp"] = vp * pp
        t["wp"] = wp * pp
    return t


def scal_terms(s, u, v, w, p, fS, fU, fV, fW, rP):
    """the term fields of the SCAL program, a dict in output order"""
    sp, up, vp, wp = _fluct(s, fS), _fluct(u, fU), _fluct(v, fV), _fluct(w, fW)
    t = {"rS2": sp * sp}
    t["rS3"] = sp * t["rS2"]
    t["rS4"] = sp * t["rS3"]
    t["Rsu"] = sp * up
    t["Rsv"] = sp * vp
    t["Rsw"] = sp * wp
    t["Tssy1"] = t["Rsv"] * sp
    t["Tsuy1"] = t["Rsu"] * vp
    t["Tsvy1"] = t["Rsv"] * vp
    t["Tswy1"] = t["Rsw"] * vp
    if p is not None:
        t["Tsvy3"] = _fluct(p, rP) * sp
    return t


def averages(terms):
    """dict of term fields -> array (len(terms), ny) of their plane averages, in the dict's order"""
    return np.stack([avg_ik_v(t) for t in terms.values()])


def exact_mean(a3):
    """the plane averages from correctly rounded sums"""
    nz, ny, nx = a3.shape
    return np.array([math.fsum(a3[:, j, :].ravel().tolist()) for j in range(ny)]) / float(nx * nz)
