"""Cost of the plane statistics (k_plane_partial of csrc/averages.hip): the single-domain driver at n^3 with one scalar on bench.py's initial
field, in one process on the same arrays (in-library event timing, tlab_profile_*):
  MEANS           tlab_avg_ik_v of u, v, w, s in one launch
  FLOW, FLOW+p    tlab_avg_moments_flow without / with a pressure field (18 / 22 outputs)
  SCAL, SCAL+p    tlab_avg_moments_scal without / with a pressure field (10 / 11 outputs)
  k_final_update  on one field, for the rate of the budget
Algorithmic bytes: 8 n^3 per field, read once.  The budget: 2 x those bytes / the rate k_final_update reaches in the same run.  Per program the
kernel time, its TB/s and the fraction of the budget it takes, and the wall time of a whole call (both launches, the copy of the profile, the
synchronisation).
The literal device route for FLOW, as the reference's statements read: three fluctuation fields (one pass each: read one field, write one), then
per output one product pass into a temporary (read two fields, write one) and one tlab_avg_ik_v of the temporary.  The library has no pointwise
product; tlab_pw_scale (in place) and tlab_pw_sum3 stand in for the two passes with the same traffic.  Its wall time over that of the FLOW call is
reported, not judged.
    python tools/averages_time.py [--n 512] [--calls 10]
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
    p = d.txc[0][: d.n]
    p.copy_(0.5 * u * u + 0.25 * s)
    tmp = [t[: d.n] for t in d.txc[1:5]]

    def rows_of(fn):
        torch.cuda.synchronize()
        L.tlab_profile_reset(); L.tlab_profile_enable(1)
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        L.tlab_profile_enable(0)
        buf = ctypes.create_string_buffer(32768)
        L.tlab_profile_report(buf, len(buf))
        L.tlab_profile_reset()
        out = {}
        for r in buf.value.decode().splitlines():
            f = r.split("\t")
            if len(f) == 4:
                out[f[0]] = {"calls": int(f[1]), "ms": float(f[2]), "bytes": float(f[3])}
        return out

    def wall_of(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.calls * 1e3

    m = O.avg_ik_v(n, n, n, [u, v, w, s, p])
    fU, fV, fW, fS, rP = m
    programs = [
        ("MEANS nf 4", "k_plane_partial<MEANS>", lambda: O.avg_ik_v(n, n, n, [u, v, w, s])),
        ("FLOW", "k_plane_partial<FLOW>", lambda: O.avg_moments_flow(n, n, n, u, v, w, fU, fV, fW)),
        ("FLOW+p", "k_plane_partial<FLOW>", lambda: O.avg_moments_flow(n, n, n, u, v, w, fU, fV, fW, p, rP)),
        ("SCAL", "k_plane_partial<SCAL>", lambda: O.avg_moments_scal(n, n, n, s, u, v, w, fS, fU, fV, fW)),
        ("SCAL+p", "k_plane_partial<SCAL>", lambda: O.avg_moments_scal(n, n, n, s, u, v, w, fS, fU, fV, fW, p, rP)),
    ]
    res = {"n": n, "calls_per_row": a.calls}
    fu = rows_of(lambda: L.tlab_pw_final_update(s.data_ptr(), d.txc[5].data_ptr(), None, None, None, 0.0, 1.0, 0, n, n, n))["k_final_update"]
    rate = fu["bytes"] / (fu["ms"] * 1e-3)      # dte = 0: the field keeps its values; the scratch tendency is spent
    res["final_update_TBps"] = rate / 1e12
    print("%-12s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   (the yardstick)" % ("k_final_update", fu["ms"] / fu["calls"],
                                                                                        fu["bytes"] / fu["calls"] / 1e9, rate / 1e12), flush=True)
    for name, tag, fn in programs:
        r = rows_of(fn)[tag]
        ms, by = r["ms"] / r["calls"], r["bytes"] / r["calls"]
        wall = wall_of(fn)
        budget = 2.0 * by / rate * 1e3
        key = name.replace(" nf 4", "").replace("+", "_")
        res[key + "_kernel_ms"], res[key + "_wall_ms"], res[key + "_bytes"] = ms, wall, by
        res[key + "_TBps"], res[key + "_budget_ms"], res[key + "_over_budget"] = by / (ms * 1e-3) / 1e12, budget, ms / budget
        print("%-12s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   budget ms %8.4f   kernel / budget %.3f   wall ms per call %8.4f"
              % (name, ms, by / 1e9, res[key + "_TBps"], budget, ms / budget, wall), flush=True)

    def literal_flow():
        for t in tmp[:3]:                                                # dwdx, dwdy, dwdz
            check(L.tlab_pw_scale(t.data_ptr(), 1.0, d.n), "tlab_pw_scale")
        for _ in range(18):                                              # dvdx = dwdx*dwdy; call AVG_IK_V(.., dvdx, ..)
            check(L.tlab_pw_sum3(tmp[3].data_ptr(), tmp[0].data_ptr(), tmp[1].data_ptr(), d.n), "tlab_pw_sum3")
            O.avg_ik_v(n, n, n, [tmp[3]])
    for t, f in zip(tmp, (u, v, w, u)):
        t.copy_(f)
    res["FLOW_literal_wall_ms"] = wall_of(literal_flow)
    res["FLOW_literal_over_fused_wall"] = res["FLOW_literal_wall_ms"] / res["FLOW_wall_ms"]
    print("FLOW, the literal route (3 + 18 pointwise passes, 18 single-field averages): wall ms %.3f = %.1f x the FLOW call"
          % (res["FLOW_literal_wall_ms"], res["FLOW_literal_over_fused_wall"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
