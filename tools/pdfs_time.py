"""Cost of the plane PDFs (csrc/pdfs.hip) at n^3, fp64: 5 fields with ibc = 2 and 32 bins, what DNS_STATISTICS asks for with one scalar, on three
data sets, in one process (in-library event timing, tlab_profile_*):
  uniform    independent uniform(-1, 1) values: the bins of neighbouring lanes are spread
  smooth     products of a few sines and cosines per field: neighbouring lanes share a bin -- the realistic case
  constant   one value: every atomic of a workgroup lands on one bin (reported, not a criterion)
Rows per data set: the min/max pass (k_pdf_minmax), the histogram pass (k_pdf_hist, each point binned into its plane's and the volume's table),
both also with a gate, and the two passes of the joint PDF of two of the fields (32 x 32 bins); then the wall time of the whole tlab_pdf1v_n call
(three passes, their final kernels, the copies and three synchronisations) and of tlab_pdf2v.
Algorithmic bytes: 8 n^3 per field per pass, plus n^3 for a gate.  The budget of a pass: 2 x those bytes / the rate k_final_update reaches in the
same run.  Per launch the kernel time, its TB/s and the fraction of the budget it takes.
    python tools/pdfs_time.py [--n 512] [--calls 10] [--bins 32]
prints rows and one JSON line."""
import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402

NV = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per row")
    ap.add_argument("--bins", type=int, default=32)
    a = ap.parse_args()
    import tlab_amd as T
    import tlab_amd.operators as O
    from tlab_amd.lib import load
    T.init(0)
    L = load()
    n, nb = a.n, a.bins
    npts = n ** 3
    f = [torch.empty(npts, dtype=torch.float64, device="cuda") for _ in range(NV)]
    h = torch.zeros(npts, dtype=torch.float64, device="cuda")

    def rows_of(fn, calls):
        torch.cuda.synchronize()
        L.tlab_profile_reset(); L.tlab_profile_enable(1)
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        L.tlab_profile_enable(0)
        buf = ctypes.create_string_buffer(65536)
        L.tlab_profile_report(buf, len(buf))
        L.tlab_profile_reset()
        out = {}
        for r in buf.value.decode().splitlines():
            c = r.split("\t")
            if len(c) == 4:
                out[c[0]] = {"calls": int(c[1]), "ms": float(c[2]), "bytes": float(c[3])}
        return out

    def wall_of(fn, calls):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    def fill(kind):
        g = torch.Generator(device="cuda").manual_seed(7)
        ax = torch.arange(n, dtype=torch.float64, device="cuda") * (2.0 * math.pi / n)
        for i, t in enumerate(f):
            if kind == "uniform":
                t.copy_(torch.rand(npts, dtype=torch.float64, device="cuda", generator=g) * 2.0 - 1.0)
            elif kind == "smooth":
                X, Y, Z = torch.sin((1 + i) * ax)[None, None, :], torch.cos(2.0 * ax + i)[None, :, None], torch.sin(3.0 * ax + 0.5 * i)[:, None, None]
                t.copy_((X * Y + 0.5 * Z * X + 0.1 * (i + 1) * Y).reshape(-1))
            else:
                t.fill_(0.75)
        torch.cuda.synchronize()

    res = {"n": n, "fields": NV, "nbins": nb, "calls_per_row": a.calls}
    fu = rows_of(lambda: L.tlab_pw_final_update(f[0].data_ptr(), h.data_ptr(), None, None, None, 0.0, 1.0, 0, n, n, n), a.calls)["k_final_update"]
    rate = fu["bytes"] / (fu["ms"] * 1e-3)      # dte = 0: the field keeps its values
    res["final_update_TBps"] = rate / 1e12
    print("%-26s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   (the yardstick)"
          % ("k_final_update", fu["ms"] / fu["calls"], fu["bytes"] / fu["calls"] / 1e9, rate / 1e12), flush=True)

    for kind in ("uniform", "smooth", "constant"):
        fill(kind)
        gate = O.gate_threshold(f[0], 0.0 if kind != "constant" else 0.5)
        lo, hi = O.pdf_minmax_planes(n, n, n, f)
        glo, ghi = O.pdf_minmax_planes(n, n, n, f, gate, 1)
        calls = [("minmax", lambda: O.pdf_minmax_planes(n, n, n, f), "k_pdf_minmax"),
                 ("hist", lambda: O.pdf_histogram_planes(n, n, n, f, nb, 1, lo, hi), "k_pdf_hist"),
                 ("minmax gated", lambda: O.pdf_minmax_planes(n, n, n, f, gate, 1), "k_pdf_minmax"),
                 ("hist gated", lambda: O.pdf_histogram_planes(n, n, n, f, nb, 1, glo, ghi, gate, 1), "k_pdf_hist"),
                 ("pdf2v range", lambda: O.pdf2v(n, n, n, (32, 32), f[0], f[1]), "k_pdf2v_range"),
                 ("pdf2v hist", lambda: O.pdf2v(n, n, n, (32, 32), f[0], f[1]), "k_pdf2v_hist")]
        cache = {}
        for name, fn, tag in calls:
            key = name.split()[0] + ("g" if "gated" in name else "")
            if key not in cache:
                cache[key] = rows_of(fn, a.calls)
            r = cache[key][tag]
            ms, by = r["ms"] / r["calls"], r["bytes"] / r["calls"]
            budget = 2.0 * by / rate * 1e3
            k = "%s_%s" % (kind, name.replace(" ", "_"))
            res[k + "_kernel_ms"], res[k + "_bytes"], res[k + "_TBps"] = ms, by, by / (ms * 1e-3) / 1e12
            res[k + "_budget_ms"], res[k + "_over_budget"] = budget, ms / budget
            print("%-9s %-16s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   budget ms %8.4f   kernel / budget %.3f"
                  % (kind, name, ms, by / 1e9, res[k + "_TBps"], budget, ms / budget), flush=True)
        whole = lambda: O.pdf1v_n(n, n, n, f, nb, 2)      # noqa: E731
        rows = rows_of(whole, a.calls)
        res[kind + "_pdf1v_n_wall_ms"] = wall_of(whole, a.calls)
        res[kind + "_pdf1v_n_kernels"] = {k: r["ms"] / a.calls for k, r in sorted(rows.items())}
        res[kind + "_pdf2v_wall_ms"] = wall_of(calls[4][1], a.calls)
        print("%-9s tlab_pdf1v_n, %d fields, ibc 2: wall ms per call %8.4f; kernel ms per call: %s"
              % (kind, NV, res[kind + "_pdf1v_n_wall_ms"], ", ".join("%s %.4f (%g launches)" % (k, r["ms"] / a.calls, r["calls"] / a.calls)
                                                                   for k, r in sorted(rows.items()))), flush=True)
        print("%-9s tlab_pdf2v, 32 x 32 bins: wall ms per call %8.4f" % (kind, res[kind + "_pdf2v_wall_ms"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
