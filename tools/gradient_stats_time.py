"""Cost of the gradient statistics (the GRAD_* programs of k_plane_partial, csrc/averages.hip): the single-domain driver at n^3 with one scalar on
bench.py's initial field, in one process on the same arrays (in-library event timing, tlab_profile_*):
  GRAD_FLOW1, GRAD_FLOW2, GRAD_FLOW3, GRAD_FLOW3+p   the passes of tlab_avg_gradients_flow over the nine gradients (, u v w, p)
  UGRADP                                              tlab_avg_ugradp
  GRAD_SCAL1, GRAD_SCAL2, GRAD_SCAL2+p                the passes of tlab_avg_gradients_scal
  k_final_update                                      on one field, for the rate of the budget
Algorithmic bytes: 8 n^3 per field read, once.  The budget: 2 x those bytes / the rate k_final_update reaches in the same run.  Per launch the
kernel time, its TB/s and the fraction of the budget it takes.  Then the whole tlab_dns_avg_gradients_flow call with p (Dns.flow_gradient_stats
without its means): wall time, and the kernel time split into the twelve derivative launches and the plane passes.
    python tools/gradient_stats_time.py [--n 512] [--calls 10]
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
    ap.add_argument("--calls", type=int, default=10, help="timed calls per row")
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
    p = d.hq[0][: d.n]                                                   # (the tendencies are free here: no substep runs)
    p.copy_(0.5 * u * u + 0.25 * s)
    grad = [t[: d.n] for t in d.txc]

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
            f = r.split("\t")
            if len(f) == 4:
                out[f[0]] = {"calls": int(f[1]), "ms": float(f[2]), "bytes": float(f[3])}
        return out

    def wall_of(fn, calls):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e3

    fU, fV, fW, fS, rP = O.avg_ik_v(n, n, n, [u, v, w, s, p])
    z = np.zeros(n)
    stats = d.flow_gradient_stats(p)                                     # fills txc with the nine gradients; its means for the driver call below
    rU_y, rV_y, rW_y = stats["rU_y"], stats["rV_y"], stats["rW_y"]
    res = {"n": n, "calls_per_row": a.calls}
    fu = rows_of(lambda: L.tlab_pw_final_update(s.data_ptr(), d.hs[0].data_ptr(), None, None, None, 0.0, 1.0, 0, n, n, n), a.calls)["k_final_update"]
    rate = fu["bytes"] / (fu["ms"] * 1e-3)      # dte = 0: the field keeps its values; the scratch tendency is spent
    res["final_update_TBps"] = rate / 1e12
    print("%-14s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   (the yardstick)" % ("k_final_update", fu["ms"] / fu["calls"],
                                                                                          fu["bytes"] / fu["calls"] / 1e9, rate / 1e12), flush=True)
    flow = lambda: O.avg_gradients_flow(n, n, n, grad, u, v, w, fU, fV, fW, rU_y, rV_y, rW_y)                # noqa: E731
    flow_p = lambda: O.avg_gradients_flow(n, n, n, grad, u, v, w, fU, fV, fW, rU_y, rV_y, rW_y, p, rP)       # noqa: E731
    scal = lambda: O.avg_gradients_scal(n, n, n, grad[:3], s, u, v, w, fS, fU, fV, fW, z)                     # noqa: E731
    scal_p = lambda: O.avg_gradients_scal(n, n, n, grad[:3], s, u, v, w, fS, fU, fV, fW, z, p, rP, z)         # noqa: E731
    ugradp = lambda: O.avg_ugradp(n, n, n, u, v, w, grad[6], grad[7], grad[8])                                # noqa: E731
    launches = [("GRAD_FLOW1", flow, "k_plane_partial<GRAD_FLOW1>"), ("GRAD_FLOW2", flow, "k_plane_partial<GRAD_FLOW2>"),
                ("GRAD_FLOW3", flow, "k_plane_partial<GRAD_FLOW3>"), ("GRAD_FLOW3+p", flow_p, "k_plane_partial<GRAD_FLOW3>"),
                ("UGRADP", ugradp, "k_plane_partial<UGRADP>"), ("GRAD_SCAL1", scal, "k_plane_partial<GRAD_SCAL1>"),
                ("GRAD_SCAL2", scal, "k_plane_partial<GRAD_SCAL2>"), ("GRAD_SCAL2+p", scal_p, "k_plane_partial<GRAD_SCAL2>")]
    cache = {}
    for name, fn, tag in launches:
        if fn not in cache:
            cache[fn] = rows_of(fn, a.calls)
        r = cache[fn][tag]
        ms, by = r["ms"] / r["calls"], r["bytes"] / r["calls"]
        budget = 2.0 * by / rate * 1e3
        key = name.replace("+", "_")
        res[key + "_kernel_ms"], res[key + "_bytes"] = ms, by
        res[key + "_TBps"], res[key + "_budget_ms"], res[key + "_over_budget"] = by / (ms * 1e-3) / 1e12, budget, ms / budget
        print("%-14s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   budget ms %8.4f   kernel / budget %.3f"
              % (name, ms, by / 1e9, res[key + "_TBps"], budget, ms / budget), flush=True)
    for name, fn in (("flow", flow), ("flow+p", flow_p), ("scal", scal), ("scal+p", scal_p), ("ugradp", ugradp)):
        res[name.replace("+", "_") + "_wall_ms"] = wall_of(fn, a.calls)
        print("%-14s wall ms per call %8.4f (all its launches, the copies of the profiles, the synchronisations)" % (name, res[name.replace("+", "_") + "_wall_ms"]),
              flush=True)

    q, _, _, _, txc = d._arrays()
    out = np.zeros((57, n))
    prof = lambda t: t.ctypes.data_as(ctypes.c_void_p)      # noqa: E731

    def driver_call():
        check(L.tlab_dns_avg_gradients_flow(d._h, q, p.data_ptr(), txc, prof(fU), prof(fV), prof(fW), prof(rP), prof(rU_y), prof(rV_y), prof(rW_y),
                                            prof(out), n), "tlab_dns_avg_gradients_flow")
    calls = max(1, a.calls // 2)
    rows = rows_of(driver_call, calls)
    plane = sum(r["ms"] for k, r in rows.items() if k.startswith("k_plane_partial")) / calls
    der = sum(r["ms"] for k, r in rows.items() if not k.startswith("k_plane_")) / calls
    nder = sum(r["calls"] for k, r in rows.items() if not k.startswith("k_plane_")) / calls
    res["driver_wall_ms"] = wall_of(driver_call, calls)
    res["driver_derivative_kernel_ms"], res["driver_derivative_launches"], res["driver_plane_kernel_ms"] = der, nder, plane
    res["driver_kernels"] = {k: r["ms"] / calls for k, r in sorted(rows.items())}
    print("tlab_dns_avg_gradients_flow with p: wall ms %.3f; kernel ms: %.3f in %g derivative launches, %.3f in the 4 k_plane_partial launches"
          " (k_plane_final, ny x nout threads, is not timed)" % (res["driver_wall_ms"], der, nder, plane), flush=True)
    for k, r in sorted(rows.items()):
        print("    %-34s launches per call %4g   ms per call %8.4f" % (k, r["calls"] / calls, r["ms"] / calls), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
