"""numpy restatement of the reference's conditional statistics: the partition of FI_GATE (mappings/fi_gate.f90:65-90), AVG1V2D / AVG1V2D1G
(utils/averages.f90:114-137, :172-209) with AVG_N_XZ and RAW_TO_CENTRAL (statistics/avg_xz.f90:10-102), and the conditional averages of module PDFS
(the optional a, avg arguments of PDF1V2D, PDF1V2D1G, PDF2V2D, utils/pdfs.f90) with CAVG1V_N / CAVG2V (statistics/cavg.f90), without their files.
Fields are arrays (nz, ny, nx): plane j of the reference's a(nx, ny, nz) is a[:, j, :], the volume is every point; a gate is int8 in the same
layout.  tests/test_conditional_host.py holds every function here to what the reference's compiled routines gave (tests/golden/conditional_ref.npz).

Every sum is the reference's: one running sum that starts at 0.0 and takes the points in the order i fastest, then k (np.add.accumulate adds
strictly left to right).  a**m for a run-time integer m is the Fortran runtime's power, square and multiply from the low bit.  The bin of a point,
the intervals and the counts are those of pdfs_oracle.py."""
import numpy as np

import pdfs_oracle as P
from averages_oracle import plane_sums      # noqa: F401  (the ungated plane sum in the same order; the tests use it for the bounds)

U53 = 2.0 ** -53
NMOMS_MAX = 10


def seqsum(x):
    """0.0 + x[0] + x[1] + .. from left to right"""
    x = np.asarray(x, dtype=np.float64).ravel()
    return np.add.accumulate(np.concatenate(([0.0], x)))[-1]


def ipow(x, m):
    """x**m as the runtime's integer power forms it: r = 1; loop: if (b & 1) r *= x; b /= 2; if (!b) break; x *= x"""
    x = np.array(x, dtype=np.float64)
    r = np.ones_like(x)
    b = int(m)
    while True:
        if b & 1:
            r = r * x
        b >>= 1
        if not b:
            return r
        x = x * x


# ---- the partition ---------------------------------------------------------------------------------------------------------------------------
def gate_levels(a, thr):
    """fi_gate.f90:85-90: the first n in 1 .. len(thr) with a < thr[n - 1], else len(thr) + 1"""
    a = np.asarray(a, dtype=np.float64)
    lev = np.full(a.shape, len(thr) + 1, dtype=np.int8)
    done = np.zeros(a.shape, dtype=bool)
    for n, t in enumerate(thr, start=1):
        hit = ~done & (a < np.float64(t))
        lev[hit] = n
        done |= hit
    return lev


def gate_flux(a, v):
    """fi_gate.f90:65-71"""
    a, v = np.asarray(a, dtype=np.float64), np.asarray(v, dtype=np.float64)
    g = np.full(a.shape, 4, dtype=np.int8)
    g[(a < 0.0) & (v <= 0.0)] = 3
    g[(a <= 0.0) & (v > 0.0)] = 2
    g[(a > 0.0) & (v >= 0.0)] = 1
    return g


def relative_thresholds(thr, ind):
    """fi_gate.f90:74-76: gate_threshold*(umax - umin) of MINMAX of the indicator"""
    ind = np.asarray(ind, dtype=np.float64)
    return np.asarray(thr, dtype=np.float64) * (ind.max() - ind.min())


# ---- gated moments ---------------------------------------------------------------------------------------------------------------------------
def raw_moment(pts, m, mask=None):
    """(sum of pts**m over the points of the mask in their order, the number of them)"""
    pts = np.asarray(pts, dtype=np.float64).ravel()
    if mask is not None:
        pts = pts[np.asarray(mask).ravel()]
    return seqsum(ipow(pts, m)), pts.size


def avg1v2d(a, j, m):
    s, n = raw_moment(a[:, j, :], m)
    return s / np.float64(n)


def avg1v2d1g(a, j, igate, m, gate):
    s, n = raw_moment(a[:, j, :], m, gate[:, j, :] == igate)
    return s / np.float64(n) if n > 0 else s


def raw_to_central(moments):
    """RAW_TO_CENTRAL (avg_xz.f90:72-102), left to right as written there; a new array"""
    aux = np.array(moments, dtype=np.float64)
    out = aux.copy()
    nm = aux.size
    with np.errstate(all="ignore"):
        for im in range(2, nm + 1):
            acc = np.float64(0.0)
            for k in range(0, im):
                num = np.float64(1.0)
                for i in range(im, im - k, -1):
                    num = num * np.float64(i)
                den = np.float64(1.0)
                for i in range(k, 0, -1):
                    den = den * np.float64(i)
                acc = acc + num / den * aux[im - k - 1] * ipow(-aux[0], k)
            out[im - 1] = acc + ipow(-aux[0], im)
    return out


def avg_n_xz(fields, nm, np_=0, gate=None):
    """AVG_N_XZ for igate = 1 .. np_ (np_ = 0: ungated, one level): (avg, sums, nsample), avg and sums (L, nv, nm, ny), nsample (L, ny) int64"""
    nz, ny, nx = fields[0].shape
    L = max(np_, 1)
    sums, ns = np.zeros((L, len(fields), nm, ny)), np.zeros((L, ny), dtype=np.int64)
    for l in range(L):
        for v, a in enumerate(fields):
            for j in range(ny):
                mask = None if np_ == 0 else (gate[:, j, :] == l + 1)
                for m in range(1, nm + 1):
                    sums[l, v, m - 1, j], ns[l, j] = raw_moment(a[:, j, :], m, mask)
    return central_of(sums, ns), sums, ns


def central_of(sums, ns):
    """what AVG_N_XZ makes of the raw sums and the counts: the division where a count is positive, then RAW_TO_CENTRAL"""
    avg = np.zeros_like(sums)
    L, nv, nm, ny = sums.shape
    for l in range(L):
        for v in range(nv):
            for j in range(ny):
                mom = sums[l, v, :, j] / np.float64(ns[l, j]) if ns[l, j] > 0 else sums[l, v, :, j].copy()
                avg[l, v, :, j] = raw_to_central(mom) if nm > 1 else mom
    return avg


# ---- conditional averages ----------------------------------------------------------------------------------------------------------------------
def _bin_sums(a, ok, b, nbins):
    """per bin: (the running sum of a over its points in their order, their sum of |a| likewise)"""
    s, sa = np.zeros(nbins), np.zeros(nbins)
    idx = np.flatnonzero(ok)
    order = np.argsort(b[idx], kind="stable")                  # (stable: the points of a bin keep their order)
    vals, bs = a[idx][order], b[idx][order]
    starts = np.flatnonzero(np.diff(bs, prepend=-1))
    for lo, hi in zip(starts, list(starts[1:]) + [bs.size]):
        s[bs[lo]], sa[bs[lo]] = seqsum(vals[lo:hi]), seqsum(np.abs(vals[lo:hi]))
    return s, sa


def cavg1v2d(ilim, u, a, umin_ext, umax_ext, nbins, mask=None):
    """PDF1V2D with a, avg (mask: PDF1V2D1G with mask = (gate == igate)): (pdf(nbins + 2), sum(nbins), sum of |a| (nbins))"""
    pdf = P.pdf1v2d(ilim, u, umin_ext, umax_ext, nbins, mask)
    u, a = np.asarray(u, dtype=np.float64).ravel(), np.asarray(a, dtype=np.float64).ravel()
    umin, umax = (umin_ext, umax_ext) if ilim == 0 else P.minmax(u, mask)
    ustep, _, _ = P.step(umin, umax, nbins)
    if mask is not None:
        u, a = u[np.asarray(mask).ravel()], a[np.asarray(mask).ravel()]
    ok, b = P.bins(u, umin, ustep, nbins, ilim == 0)
    s, sa = _bin_sums(a, ok, b, nbins)
    return pdf, s, sa


def divide(s, cnt):
    """avg(up) = avg(up)/pdf(up) where pdf(up) > 0"""
    return np.divide(s, cnt, out=np.array(s, dtype=np.float64), where=cnt > 0)


def cavg1v_n(fields, a, nbins, ibc, umin=None, umax=None, gate=None, igate=0):
    """CAVG1V_N: (avg, sum, pdf, sum of |a|), each (nv, ny + 1, nbins + 2) with the two centres behind the bins (not in the last); the last plane
    is zero when ny == 1"""
    nz, ny, nx = fields[0].shape
    out = [np.zeros((len(fields), ny + 1, nbins + 2)) for _ in range(4)]
    masks = None if igate == 0 else P._planes(np.asarray(gate).reshape(nz, ny, nx) == igate)
    pa = P._planes(np.asarray(a, dtype=np.float64).reshape(nz, ny, nx))
    for v, f in enumerate(fields):
        for j, pts in enumerate(P._planes(np.asarray(f, dtype=np.float64).reshape(nz, ny, nx))):
            lo, hi = (umin[v], umax[v]) if ibc[v] == 0 else (0.0, 0.0)
            pdf, s, sa = cavg1v2d(ibc[v], pts, pa[j], lo, hi, nbins, None if masks is None else masks[j])
            out[0][v, j], out[1][v, j], out[2][v, j] = pdf, pdf, pdf
            out[0][v, j, :nbins], out[1][v, j, :nbins], out[3][v, j, :nbins] = divide(s, pdf[:nbins]), s, sa
    return out


def cavg2v2d(u, v, a, nbins):
    """PDF2V2D with a, avg: (pdf, sum(nb1*nb2), sum of |a|)"""
    pdf = P.pdf2v2d(u, v, nbins)
    u, v, a = (np.asarray(x, dtype=np.float64).ravel() for x in (u, v, a))
    nb1, nb2 = nbins
    nb = nb1 * nb2
    umin, umax = P.minmax(u)
    ustep, _, _ = P.step(umin, umax, nb1)
    ok, up = P.bins(u, umin, ustep, nb1, False)
    cell = np.zeros(u.size, dtype=np.int64)
    for b in range(nb1):
        sel = ok & (up == b)
        lo, hi = P.minmax(v, sel)
        vstep, _, _ = P.step(lo, hi, nb2)
        okv, vp = P.bins(v[sel], lo, vstep, nb2, False)
        cell[sel] = np.where(okv, vp * nb1 + b, -1)
    cell[~ok] = -1
    s, sa = _bin_sums(a, cell >= 0, cell, nb)
    return pdf, s, sa


def cavg2v(u, v, a, nbins):
    """CAVG2V: (avg, sum of |a|) in the layout of pdf2v, (ny + 1, nb1*nb2 + 2 + 2*nb1); counts: pdfs_oracle.pdf2v"""
    nz, ny, nx = u.shape
    nb = nbins[0] * nbins[1]
    avg, sa = np.zeros((ny + 1, nb + 2 + 2 * nbins[0])), np.zeros((ny + 1, nb))
    for j, (pu, pv, pa) in enumerate(zip(P._planes(u), P._planes(v), P._planes(a))):
        pdf, s, sa[j] = cavg2v2d(pu, pv, pa, nbins)
        avg[j] = pdf
        avg[j, :nb] = divide(s, pdf[:nb])
    return avg, sa


def within_bound(got, ref, sum_abs, n, what):
    """|got - ref| <= 2 (n - 1) u sum|.| / n + 2 u |ref| for every entry with n > 0 (the two-summation-orders bound); entries with n == 0 must be
    equal.  Prints and returns the largest fraction of the bound used."""
    got, ref, sum_abs, n = (np.asarray(x, dtype=np.float64) for x in (got, ref, sum_abs, n))
    nn = np.maximum(n, 1.0)
    bound = np.where(n > 0, 2.0 * (nn - 1.0) * U53 * sum_abs / nn + 2.0 * U53 * np.abs(ref), 0.0)
    err = np.abs(got - ref)
    frac = float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max()) if err.size else 0.0
    print("%s: largest error / bound = %.3f" % (what, frac))
    assert np.all(err <= bound), (what, frac, float(err.max()))
    return frac
