"""numpy restatement of the reference's module PDFS (utils/pdfs.f90: PDF1V2D, PDF1V2D1G, PDF2V2D, PDF_ANALIZE) and of PDF1V_N / PDF2V
(statistics/pdf.f90) without their files.  Fields are arrays (nz, ny, nx): plane j of the reference's u(nx, ny, nz) is a[:, j, :], the volume is
every point.  Histograms are counts in float64; a pdf holds nbins counts and the centres of the first and the last bin.

The bin of a point is up = int(q) + 1 with q = (u - umin)/ustep, one subtraction and one division in float64.  int() truncates toward zero, so
with an external interval a value slightly below umin (q in (-1, 0)) is counted in bin 1 and a value equal to umax (q = nbins) is dropped.
Where Fortran's int() is undefined the result is DEFINED (include/tlab_amd.h): an external interval counts a point iff -1 < q < nbins; a local
interval counts every finite q > -1 in bin min(trunc(q) + 1, nbins); NaN and infinite q are dropped."""
import numpy as np

BIG = np.float64(1.0e20)      # big_wp
HUGE = np.finfo(np.float64).max


def step(umin, umax, nbins):
    """utils/pdfs.f90:68-71: (ustep, first centre, last centre); the centres with the step before a zero step becomes 1"""
    with np.errstate(all="ignore"):
        umin, umax = np.float64(umin), np.float64(umax)
        ustep = (umax - umin) / np.float64(nbins)
        first = umin + np.float64(0.5) * ustep
        last = umax - np.float64(0.5) * ustep
        if ustep == 0.0:
            ustep = np.float64(1.0)
    return ustep, first, last


def bins(u, umin, ustep, nbins, ext):
    """(counted, 0-based bin) of every point of u"""
    with np.errstate(all="ignore"):
        q = (np.asarray(u, dtype=np.float64) - np.float64(umin)) / np.float64(ustep)
        inside = q < nbins
        ok = (q > -1.0) & (inside if ext else np.isfinite(q))
        b = np.where(ok & inside, np.trunc(np.where(ok & inside, q, 0.0)), nbins - 1).astype(np.int64)
    return ok, b


def minmax(u, mask=None):
    """:50-57 from the first point; gated (:144-153) from big_wp"""
    u = np.asarray(u, dtype=np.float64).ravel()
    if mask is None:
        return u.min(), u.max()
    g = u[np.asarray(mask).ravel()]
    return min(BIG, g.min()) if g.size else BIG, max(-BIG, g.max()) if g.size else -BIG


def pdf1v2d(ilim, u, umin_ext, umax_ext, nbins, mask=None):
    """PDF1V2D of the points u (mask: PDF1V2D1G with mask = (gate == igate)): pdf(nbins + 2)"""
    u = np.asarray(u, dtype=np.float64).ravel()
    umin, umax = (umin_ext, umax_ext) if ilim == 0 else minmax(u, mask)
    ustep, first, last = step(umin, umax, nbins)
    pts = u if mask is None else u[np.asarray(mask).ravel()]
    ok, b = bins(pts, umin, ustep, nbins, ilim == 0)
    pdf = np.zeros(nbins + 2)
    pdf[:nbins] = np.bincount(b[ok], minlength=nbins)[:nbins]
    pdf[nbins], pdf[nbins + 1] = first, last
    return pdf


def pdf_analize(ibc, nbins, pdf, plim):
    """PDF_ANALIZE (:329-379): (umin_ext, umax_ext, nplim); maxval of an empty range is -huge"""
    with np.errstate(all="ignore"):
        pdf = np.asarray(pdf, dtype=np.float64)
        half = np.float64(0.5)
        first = pdf[nbins]
        ustep = (pdf[nbins + 1] - pdf[nbins]) / np.float64(nbins - 1)
        upmin, upmax = 1, nbins
        if ibc in (1, 3):
            upmin += 1
        if ibc in (2, 3):
            upmax -= 1
        umin_ext = first - half * ustep + ustep * np.float64(upmin - 1)
        umax_ext = first - half * ustep + ustep * np.float64(upmax)
        rng = pdf[upmin - 1:upmax]
        threshold = np.float64(plim) * (rng.max() if rng.size else -HUGE)
        above = [up for up in range(upmin, upmax + 1) if pdf[up - 1] > threshold]
        if above:
            umin_ext = first - half * ustep + ustep * np.float64(above[0] - 1)
            umax_ext = first - half * ustep + ustep * np.float64(above[-1])
    return umin_ext, umax_ext, len(above)


def _planes(a):
    """the point sets PDF1V_N visits: every plane, then -- when ny > 1 -- the volume"""
    nz, ny, nx = a.shape
    return [a[:, j, :] for j in range(ny)] + ([a] if ny > 1 else [])


def pdf1v_n(fields, nbins, ibc, umin=None, umax=None, gate=None, igate=0, plim=1.0e-4):
    """PDF1V_N (statistics/pdf.f90:14-91): (nv, ny + 1, nbins + 2); the last plane is zero when ny == 1"""
    nz, ny, nx = fields[0].shape
    out = np.zeros((len(fields), ny + 1, nbins + 2))
    masks = None if igate == 0 else _planes(np.asarray(gate).reshape(nz, ny, nx) == igate)
    for v, a in enumerate(fields):
        for j, pts in enumerate(_planes(np.asarray(a, dtype=np.float64).reshape(nz, ny, nx))):
            m = None if masks is None else masks[j]
            lo, hi = (umin[v], umax[v]) if ibc[v] == 0 else (0.0, 0.0)
            pdf = pdf1v2d(ibc[v], pts, lo, hi, nbins, m)
            if ibc[v] > 1:
                lo, hi, _ = pdf_analize(ibc[v] - 2, nbins, pdf, plim)
                pdf = pdf1v2d(0, pts, lo, hi, nbins, m)
            out[v, j] = pdf
    return out


def pdf2v2d(u, v, nbins):
    """PDF2V2D (:215-322) of the points (u, v): pdf(nb1*nb2 + 2 + 2*nb1), bin (up, vp) at (vp-1)*nb1 + up"""
    u, v = np.asarray(u, dtype=np.float64).ravel(), np.asarray(v, dtype=np.float64).ravel()
    nb1, nb2 = nbins
    nb = nb1 * nb2
    pdf = np.zeros(nb + 2 + 2 * nb1)
    umin, umax = minmax(u)
    ustep, pdf[nb], pdf[nb + 1] = step(umin, umax, nb1)
    ok, up = bins(u, umin, ustep, nb1, False)
    vmin, vstep = np.zeros(nb1), np.zeros(nb1)
    for b in range(nb1):
        lo, hi = minmax(v, ok & (up == b))
        vmin[b] = lo
        vstep[b], pdf[nb + 2 + b], pdf[nb + 2 + nb1 + b] = step(lo, hi, nb2)
    for b in range(nb1):
        sel = ok & (up == b)
        okv, vp = bins(v[sel], vmin[b], vstep[b], nb2, False)
        pdf[b:nb:nb1] += np.bincount(vp[okv], minlength=nb2)[:nb2]
    return pdf


def pdf2v(u, v, nbins):
    """PDF2V (statistics/pdf.f90:123-159): (ny + 1, nb1*nb2 + 2 + 2*nb1); the last plane is zero when ny == 1"""
    nz, ny, nx = u.shape
    out = np.zeros((ny + 1, nbins[0] * nbins[1] + 2 + 2 * nbins[0]))
    for j, (pu, pv) in enumerate(zip(_planes(u), _planes(v))):
        out[j] = pdf2v2d(pu, pv, nbins)
    return out


def gate_threshold(a, thr):
    return (np.asarray(a) > thr).astype(np.int8)
