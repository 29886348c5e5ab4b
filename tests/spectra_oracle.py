"""numpy restatement of the plane spectra and correlations of the reference: the four routines of module SpectraMod
(tools/statistics/spectra_pool.f90), OPR_Fourier_CONVOLUTION_FXZ (operators/opr_fourier.f90:528-582) with the kz shuffle of
OPR_Fourier_Z_Forward / _Backward (:357-370, :407-420), and the loop body of tools/statistics/spectra.f90:620-659 for one pair.
tests/test_spectra_host.py holds it to the reference's own compiled routines (tests/golden/spectra_ref.npz).

Arrays are C-ordered numpy: a Fortran a(i, j, k) is a[k, j, i].  Where the order of a floating-point sum matters the loops run in the reference's
order; numpy only vectorises over elements that belong to DIFFERENT outputs (the planes y, or kx where kx is not summed over).  The routines are
dtype-generic: on int64 arrays with norm = 1 they are the integer evaluation that tests/golden/make_golden_spectra.py holds the exact-data
records to.  `sign` is the sign of the two subtractions of INTEGRATE_SPECTRUM (:105, :108); sign = +1 on |terms| lists every term of a sum once,
which is what the bound of two summation orders needs."""
import numpy as np


def shuffle(nz):
    """position ks of a shuffled array holds natural mode shuffle(nz)[ks] (opr_fourier.f90:358-366; with odd nz the loop leaves the last alone)"""
    h = nz // 2
    idx = np.arange(nz)
    idx[:h], idx[h:2 * h] = np.arange(h, 2 * h), np.arange(h)
    return idx


def fold(ks, nz):
    """INTEGRATE_SPECTRUM :84-88 for position ks (0-based): (kz_global 1-based with the Nyquist mode folded, flag)"""
    h, k1 = nz // 2, ks + 1
    kzg, flag = (h - k1 + 2, 1) if k1 <= h else (k1 - h, 0)
    if kzg == h + 1:
        kzg = max(h, 1)
    return kzg, flag


def ring(a, b):
    """int(sqrt(real(a**2 + b**2, wp))) (:99, :349, :394), 0-based ring"""
    return int(np.sqrt(np.float64(a * a + b * b)))


def reduce_spectrum(nx, ny, nz, nblock, power, out, variance):
    """REDUCE_SPECTRUM :226-274 without the phase: power[ks, y, kx] = real(c_in) for kx = 0 .. nx/2 (shuffled kz); out[ks, jb, kx] += ; variance[y]"""
    nkx, ny_loc = nx // 2, ny - ny % nblock
    variance[:] = 0
    for ks in range(nz):
        for y in range(ny_loc):
            out[ks, y // nblock, :] += power[ks, y, :nkx]
        for kx in range(nkx):                                       # variance(y, 1): kx inner, the Nyquist column after it (:239-268)
            variance[:ny_loc] += power[ks, :ny_loc, kx] * (1 if kx == 0 else 2)
        variance[:ny_loc] += power[ks, :ny_loc, nkx]


def integrate_spectrum(nkx, nyo, nz, kr_total, S, outx, outz, outr, sign=-1):
    """INTEGRATE_SPECTRUM :73-185 (single rank): S[ks, jb, kx]; outx[jb, kx], outz[jb, kz], outr[jb, kr] are accumulated into"""
    tmp_x = np.zeros((nyo, nkx), dtype=S.dtype)
    tmp_z = np.zeros((nz, nyo), dtype=S.dtype)
    for ks in range(nz):
        tmp_x += S[ks]
        kzg, flag = fold(ks, nz)
        for i in range(nkx):
            p = S[ks, :, i]
            tmp_z[ks] += p
            kr = ring(i, kzg - 1)
            if kr < kr_total:
                outr[:, kr] += p
            if i == 0 and flag == 1:
                tmp_z[ks] += sign * p
                if kr < kr_total:
                    outr[:, kr] += sign * p
            if kzg == 1 and i > 0:
                tmp_z[ks] += p
    outx += tmp_x
    wrk = np.zeros((nz, nyo), dtype=S.dtype)
    for ks in range(nz):
        wrk[fold(ks, nz)[0] - 1] += tmp_z[ks]
    outz += wrk[:nz // 2].T


def corr_norms(var1, var2):
    """:321-324"""
    n = np.sqrt(var1) * np.sqrt(var2)
    return np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 1.0)


def reduce_correlation(nx, ny, nz, nblock, nr_total, x, normj, out2d, outx, outz, outr, variance2, icalc_radial=1):
    """REDUCE_CORRELATION :313-358 on the scaled field x[k, j, i]; out2d[k, jb, i], outx[jb, i], outz[jb, k], outr[jb, r] are accumulated into"""
    ny_loc = ny - ny % nblock
    variance2[:] = 0
    for j in range(ny_loc):
        jb = j // nblock
        v = x[:, j, :] * normj[j]
        out2d[:, jb, :] += v
        outx[jb, :] += v[0, :]
        outz[jb, :] += v[:, 0]
        if icalc_radial == 1:
            for k in range(min(nz, nr_total)):
                for i in range(min(nx, nr_total)):
                    r = ring(k, i)
                    if r < nr_total:
                        outr[jb, r] += v[k, i]
        variance2[j] = x[0, j, 0]


def radial_samplesize(nx, nz, nr_total):
    """RADIAL_SAMPLESIZE :381-398 from zero"""
    s = np.zeros(nr_total)
    for k in range(min(nz, nr_total)):
        for i in range(min(nx, nr_total)):
            r = ring(k, i)
            if r < nr_total:
                s[r] += 1.0
    return s


def product(ah, bh=None):
    """Re(b^ conj(a^)) as the complex product of opr_fourier.f90:554, :563 evaluates it: two products and one sum"""
    bh = ah if bh is None else bh
    return bh.real * ah.real + bh.imag * ah.imag


def spectrum(nx, ny, nz, nblock, kr_total, ah, bh=None, norm=None, sign=-1):
    """tlab_spectrum_reduce: a^, b^ complex [kz natural, y, kx] -> dict(xz, x, z, r, variance) from zero.  norm = 1 with integer parts: exact"""
    nkx, nyo = nx // 2, ny // nblock
    if norm is None:
        power = (product(ah, bh) * (1.0 / (nx * nz))) * (1.0 / (nx * nz))       # spectra.f90:641
    else:
        power = product(ah, bh) * norm
    power = power[shuffle(nz)]
    dt = power.dtype
    S, var = np.zeros((nz, nyo, nkx), dtype=dt), np.zeros(ny, dtype=dt)
    reduce_spectrum(nx, ny, nz, nblock, power, S, var)
    o = {"xz": S, "x": np.zeros((nyo, nkx), dtype=dt), "z": np.zeros((nyo, nz // 2), dtype=dt), "r": np.zeros((nyo, kr_total), dtype=dt), "variance": var}
    integrate_spectrum(nkx, nyo, nz, kr_total, S, o["x"], o["z"], o["r"], sign)
    return o


def correlation(nx, ny, nz, nblock, nr_total, field, var1, var2, norm=None, normj=None):
    """tlab_correlation_reduce with icalc_radial = 1: field real [k, j, i] -> dict(xz, x, z, r, variance) from zero (variance: variance2)"""
    nyo = ny // nblock
    x = (field * (1.0 / (nx * nz))) * (1.0 / (nx * nz)) if norm is None else field * norm      # spectra.f90:653
    normj = corr_norms(np.asarray(var1), np.asarray(var2)) if normj is None else normj
    dt = x.dtype
    o = {"xz": np.zeros((nz, nyo, nx), dtype=dt), "x": np.zeros((nyo, nx), dtype=dt), "z": np.zeros((nyo, nz), dtype=dt),
         "r": np.zeros((nyo, nr_total), dtype=dt), "variance": np.zeros(ny, dtype=dt)}
    reduce_correlation(nx, ny, nz, nblock, nr_total, x, normj, o["xz"], o["x"], o["z"], o["r"], o["variance"])
    return o


# ---- the transforms ---------------------------------------------------------------------------------------------------------------------------------
def fft_numpy(a):
    """OPR_Fourier_X_Forward + the FFT of OPR_Fourier_Z_Forward: real [k, j, i] -> complex [kz natural, j, kx], unnormalised"""
    return np.fft.fft(np.fft.rfft(a, axis=2), axis=0)


def ifft_numpy(c, nx):
    """the FFTs of OPR_Fourier_Z_Backward + OPR_Fourier_X_Backward, unnormalised like FFTW"""
    nz = c.shape[0]
    return np.fft.irfft(np.fft.ifft(c, axis=0) * nz, n=nx, axis=2) * nx


def _twiddles(n, sign):
    """exp(sign 2 pi i k m / n) in long double, the angle reduced mod n before the multiplication"""
    k = np.arange(n)
    t = (np.outer(k, k) % n).astype(np.longdouble) * (2 * np.arctan2(np.longdouble(0), np.longdouble(-1)) / n)
    return np.cos(t) + (1j * sign) * np.sin(t)


def fft_direct(a):
    """fft_numpy as a direct DFT in np.longdouble (the yardstick of the FFT's own error; small shapes only)"""
    nz, _, nx = a.shape
    wx, wz = _twiddles(nx, -1)[:, :nx // 2 + 1], _twiddles(nz, -1)
    ax = np.einsum("kji,im->kjm", a.astype(np.longdouble), wx)
    return np.einsum("kjm,kn->njm", ax, wz)


def ifft_direct(c, nx):
    nz = c.shape[0]
    wz, wx = _twiddles(nz, +1), _twiddles(nx, +1)
    cz = np.einsum("kjm,kn->njm", c.astype(np.clongdouble), wz)
    full = np.zeros(c.shape[:2] + (nx,), dtype=np.clongdouble)      # the Hermitian completion a c2r transform implies
    full[:, :, :nx // 2 + 1] = cz
    full[:, :, nx // 2 + 1:] = np.conj(cz[:, :, 1:nx // 2][:, :, ::-1])
    full[:, :, 0] = full[:, :, 0].real
    full[:, :, nx // 2] = full[:, :, nx // 2].real
    return np.einsum("kjm,mi->kji", full, wx).real


def cov2v2d(a, b):
    """COV2V2D (utils/averages.f90:244-267) of every plane: k outer, i inner, then the division"""
    nz, ny, nx = a.shape
    acc = np.zeros(ny)
    for k in range(nz):
        for i in range(nx):
            acc = acc + a[k, :, i] * b[k, :, i]
    return acc / float(nx * nz)


def pair(mode, nblock, kr_total, a, b=None, fft=fft_numpy, ifft=ifft_numpy, var=None):
    """spectra.f90:620-659 for one pair of fluctuation fields a, b [k, j, i] (b None: auto): dict(xz, x, z, r, variance, cov[3, ny]).
    mode 1: spectra, 2: correlations.  The shuffles of the two z transforms of the correlation route cancel and are not carried out.
    var: (var1, var2) that normalise the correlations instead of cov[1], cov[2] -- COV2V2D's running sum of nx*nz terms is itself some ten
    units in the last place from the exact mean, and a correlation divides by it."""
    nz, ny, nx = a.shape
    bb = a if b is None else b
    cov = np.stack([cov2v2d(a, bb), cov2v2d(a, a), cov2v2d(bb, bb)])
    ah = fft(a)
    bh = None if b is None else fft(b)
    if mode == 1:
        o = spectrum(nx, ny, nz, nblock, kr_total, ah.astype(np.complex128), None if bh is None else bh.astype(np.complex128))
    else:
        bhh = ah if bh is None else bh
        c = bhh * np.conj(ah)
        o = correlation(nx, ny, nz, nblock, kr_total, np.asarray(ifft(c, nx), dtype=np.float64), *((cov[1], cov[2]) if var is None else var))
    o["cov"] = cov
    return o


def fluctuation(a):
    """FI_FLUCTUATION_INPLACE (mappings/fi_dissipation.f90:119-139) with AVG_IK's order (utils/averages.f90:273-295)"""
    nz, ny, nx = a.shape
    acc = np.zeros(ny)
    for k in range(nz):
        for i in range(nx):
            acc = acc + a[k, :, i]
    return a - (acc / float(nx * nz))[None, :, None]


def pairs(nscal, cross, with_p):
    """the pair list of spectra.f90:482-522 as (name, name): variables u v w (p) 1 2 .."""
    names = ["u", "v", "w"] + (["p"] if with_p else [])
    scal = [str(i + 1) for i in range(nscal)]
    if not cross:
        return [(n, n) for n in names + scal]
    return [("u", "v"), ("u", "w"), ("v", "w")] + [(n, s) for s in scal for n in "uvw"]
