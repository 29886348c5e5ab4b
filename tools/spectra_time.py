"""Cost of the plane spectra and correlations (csrc/spectra.hip): the single-domain driver at n^3 with one scalar on bench.py's initial field, in
one process on the same arrays (kernel times: in-library event timing, tlab_profile_*; wall times: a host clock around calls that end in a
synchronise).
  k_plane_partial<MEANS>   tlab_avg_ik_v of u, v, w, s in one launch: the streaming rate of this process, the yardstick of the rows below
  every new kernel         its time and TB/s on its algorithmic bytes, from one auto and one cross pair of each route
  a pair, end to end       tlab_spectra_pair, auto and cross, spectra and correlations: wall time, split into the transforms (the same
                           tlab_poisson_fft_x / _z calls on their own) and the rest (covariances, product, reductions, the copies of the profiles
                           and the synchronisations)
  Dns.spectra              the five auto pairs u, v, w, p, s with FI_PRESSURE_BOUSSINESQ first, and the pressure on its own
Algorithmic bytes (what a launch must move, caches aside), with C = 16 (n/2+1) n^2 the bytes of a transformed field, F = 8 n^3 those of a field
and S = 8 (n/2) (n/nblock) n those of the block-reduced spectrum:
  k_spectrum_reduce  C (2 C for a cross pair) read + S written     k_spectrum_x, _z, _r  S read each (x: 3 S with out2d)
  k_cross_product    2 C (3 C for a cross pair)                    k_fluctuation         2 F
  k_correlation_reduce  the row and the column alone without out2d, (nblock + 2) F with it
  k_plane_partial<COV2>  2 F
    python tools/spectra_time.py [--n 512] [--calls 5]
prints rows and one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per row")
    a = ap.parse_args()
    import tlab_amd as T
    import tlab_amd.operators as O
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load, check
    from bench import synthetic_fields
    T.init(0)
    L = load()
    n = a.n
    x = np.arange(n) / n
    y = np.arange(n) / (n - 1.0)
    d = Dns(x, y, x.copy(), nscal=1, visc=1.0 / 5000.0, schmidt=(1.0,), yuniform=True, hyper_bc1_ext=0.0)
    synthetic_fields(d.q + d.s, n, n, n, 0, n, 0)
    u, v, w = d.q
    s = d.s[0]
    kr = n // 2
    res = {"n": n, "calls_per_row": a.calls}

    def rows_of(fn):
        torch.cuda.synchronize()
        L.tlab_profile_reset(); L.tlab_profile_enable(1)
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        L.tlab_profile_enable(0)
        buf = ctypes.create_string_buffer(65536)
        L.tlab_profile_report(buf, len(buf))
        L.tlab_profile_reset()
        out = {}
        for r in buf.value.decode().splitlines():
            f = r.split("\t")
            if len(f) == 4:
                out[f[0]] = {"calls": int(f[1]), "ms": float(f[2]), "bytes": float(f[3])}
        return out

    def wall_of(fn, calls=None):
        calls = calls or a.calls
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    # the yardstick
    r = rows_of(lambda: O.avg_ik_v(n, n, n, [u, v, w, s]))["k_plane_partial<MEANS>"]
    yard = r["bytes"] / (r["ms"] * 1e-3) / 1e12
    res["plane_partial_TBps"] = yard
    print("%-24s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   (the yardstick)" % ("k_plane_partial<MEANS>", r["ms"] / r["calls"],
                                                                                        r["bytes"] / r["calls"] / 1e9, yard), flush=True)

    # two fluctuation fields in txc[0], txc[1]; work arrays txc[3..5]; accumulators
    mean = O.avg_ik_v(n, n, n, [u, s])
    fa, fb = d.txc[0][: d.n], d.txc[1][: d.n]
    tmp = d.txc[3:6]
    kernels = {}

    def note(rows):
        for tag, r in rows.items():
            if tag.startswith("k_spectrum") or tag.startswith("k_corr") or tag.startswith("k_cross") or tag.startswith("k_fluct") or "COV2" in tag:
                kernels.setdefault(tag, []).append(r)

    note(rows_of(lambda: (O.fluctuation(n, n, n, u, mean[0], fa), O.fluctuation(n, n, n, s, mean[1], fb))))
    plan = d.poisson

    def transforms(nfields, inverse):
        p = [t.data_ptr() for t in tmp]
        for f in (fa, fb)[:nfields]:
            check(L.tlab_poisson_fft_x(plan._h, 1, f.data_ptr(), p[0]), "fft_x")
            check(L.tlab_poisson_fft_z(plan._h, 1, p[0], p[1]), "fft_z")
        if inverse:
            check(L.tlab_poisson_fft_z(plan._h, -1, p[1], p[0]), "fft_z")
            check(L.tlab_poisson_fft_x(plan._h, -1, p[0], p[1]), "fft_x")

    for mode, mname in ((1, "spectra"), (2, "correlations")):
        for cross in (False, True):
            out = {}

            def pair():
                o = O.spectra_pair(plan, mode, 1, kr, fa, fb if cross else None, tmp=tmp, out=out or None)
                out.update({k: o[k] for k in ("x", "z", "r")})
            rows = rows_of(pair)
            note(rows)
            wall = wall_of(pair)
            tw = wall_of(lambda: transforms(2 if cross else 1, mode == 2))
            key = "%s_%s" % (mname, "cross" if cross else "auto")
            res[key + "_wall_ms"], res[key + "_transforms_ms"], res[key + "_rest_ms"] = wall, tw, wall - tw
            print("%-24s wall ms per pair %8.3f   transforms %8.3f   covariances, product, reductions, copies and synchronisations %8.3f"
                  % (key, wall, tw, wall - tw), flush=True)
    # the correlation reduce with its 2-D output, on its own
    note(rows_of(lambda: O.correlation_reduce(n, n, n, 1, kr, fa, np.ones(n), np.ones(n), out2d=True)))

    for tag in sorted(kernels):
        for i, r in enumerate(kernels[tag]):
            ms, by = r["ms"] / r["calls"], r["bytes"] / r["calls"]
            rate = by / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            res.setdefault("kernels", []).append({"tag": tag, "kernel_ms": ms, "bytes": by, "TBps": rate, "over_yardstick": rate / yard})
            print("%-24s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   = %.2f of k_plane_partial" % (tag, ms, by / 1e9, rate, rate / yard), flush=True)

    # what a pair of the driver call adds to tlab_spectra_pair, each a call that ends in a synchronise
    pf = d.txc[2][: d.n]
    for name, fn in (("avg_ik_v, 5 fields", lambda: O.avg_ik_v(n, n, n, [u, v, w, pf, s])), ("fluctuation, 1 field", lambda: O.fluctuation(n, n, n, u, mean[0], fa)),
                     ("avg_cov2v, 1 pair", lambda: O.avg_cov2v(n, n, n, fa, fb))):
        t = wall_of(fn)
        res[name.split(",")[0] + "_wall_ms"] = t
        print("%-24s wall ms per call %8.3f" % (name, t), flush=True)
    # the driver call: five auto pairs with p, the four without, and the pressure alone
    tp = wall_of(lambda: d.FI_PRESSURE_BOUSSINESQ(), 3)
    t4 = wall_of(lambda: d.spectra("spectra", False, 1), 3)
    res["dns_spectra_4_auto_pairs_wall_ms"] = t4
    print("Dns.spectra(spectra     ) four auto pairs without p: wall ms %.2f; per pair %.2f" % (t4, t4 / 4.0), flush=True)
    for mname in ("spectra", "correlations"):
        t5 = wall_of(lambda: d.spectra(mname, False, 1, p=True), 3)
        res["dns_%s_5_auto_pairs_with_p_wall_ms" % mname] = t5
        print("Dns.spectra(%-12s) five auto pairs with p: wall ms %.2f, of which FI_PRESSURE_BOUSSINESQ %.2f; per pair %.2f"
              % (mname, t5, tp, (t5 - tp) / 5.0), flush=True)
    res["pressure_wall_ms"] = tp
    print(json.dumps(res))


if __name__ == "__main__":
    main()
