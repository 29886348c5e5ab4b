"""Cost of the Lagrangian particles beside the device substep: the single-domain driver at n^3 with one scalar and tracers at uniformly random
positions, np = 2^24 and np = n^3 / 2.  Per particle count, in one process on the same arrays (in-library event timing, tlab_profile_*):
  unsorted          k_particle_substep on the random order
  sorted            the same right after tlab_dns_particle_sort
  sorted + 10/100   the same after 10 and after 100 further steps of the flow of bench.py's initial field (particles advected with it): how fast the
                    order decays
  sort              tlab_dns_particle_sort itself (keys, radix sort, one gather per array), on the random order and on the decayed one
  k_final_update    on one field, for the rate of the budget
The timed substeps use dte = 0 (positions, nodes and order keep their values; same loads, stores and arithmetic).
The budget: the sorted kernel within 2 x its algorithmic bytes / the rate k_final_update reaches in the same run; algorithmic bytes =
np (2 x 8 x 2 x inb_part + 8) for l_q, l_hq and nodes read and written + 3 x 8 x n^3 for one pass over the velocities.
    python tools/particles_time.py [--n 512] [--calls 5] [--np 16777216 67108864]       (prints rows and one JSON line per particle count)"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--calls", type=int, default=5, help="timed launches per row")
    ap.add_argument("--np", type=int, nargs="*", default=None, help="particle counts (default 2^24 and n^3 / 2)")
    ap.add_argument("--decay", type=int, nargs="*", default=[10, 100], help="cumulative flow steps after the sort at which the substep is timed again")
    a = ap.parse_args()
    import tlab_amd as T
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    from bench import synthetic_fields
    T.init(0)
    L = load()
    n = a.n
    counts = a.np or [1 << 24, n ** 3 // 2]
    x = np.arange(n) / n
    y = np.arange(n) / (n - 1.0)
    d = Dns(x, y, x.copy(), nscal=1, visc=1.0 / 5000.0, schmidt=(1.0,), yuniform=True, hyper_bc1_ext=0.0)
    dt = 1e-3
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)

    def rows_of(fn):
        torch.cuda.synchronize()
        L.tlab_profile_reset(); L.tlab_profile_enable(1)
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

    def substeps():
        for _ in range(a.calls):
            d.TIME_SUBSTEP_PARTICLE(0.0)

    def show(np_, name, r):
        ms, gb = r["ms"] / r["calls"], r["bytes"] / r["calls"] / 1e9
        print("np %-9d %-22s calls %3d   ms/call %8.4f   algorithmic GB/call %7.4f   TB/s %.3f" % (np_, name, r["calls"], ms, gb, gb / ms))
        return ms

    for np_ in counts:
        synthetic_fields(d.q + d.s, n, n, n, 0, n, 0)
        d.set_particles("tracer", np_)
        for i, t in enumerate(d.l_q):      # uniformly random in the box (y between the walls)
            t.copy_(torch.rand(np_, dtype=torch.float64, device="cuda", generator=gen))
        d.locate_particles()
        d.TIME_SUBSTEP_PARTICLE(0.0)       # first touch
        res = {"n": n, "np": np_, "inb_part": 3, "calls_per_row": a.calls}
        res["ms_unsorted"] = show(np_, "substep unsorted", rows_of(substeps)["k_particle_substep"])
        res["ms_sort_random_order"] = show(np_, "sort (random order)", rows_of(d.sort_particles)["particle_sort"])
        r = rows_of(substeps)["k_particle_substep"]
        res["ms_sorted"] = show(np_, "substep sorted", r)
        res["bytes_per_substep"] = r["bytes"] / r["calls"]
        done = 0
        for steps in a.decay:
            for _ in range(steps - done):
                d.TIME_RUNGEKUTTA(dt)
            done = steps
            res["ms_sorted_plus_%d_steps" % steps] = show(np_, "substep sorted + %d" % steps, rows_of(substeps)["k_particle_substep"])
        res["ms_sort_decayed_order"] = show(np_, "sort (decayed order)", rows_of(d.sort_particles)["particle_sort"])
        res["ms_sorted_again"] = show(np_, "substep sorted again", rows_of(substeps)["k_particle_substep"])

        def final_updates():      # dte = 0: the field keeps its values; the scratch tendency is spent
            for _ in range(3):
                L.tlab_pw_final_update(d.s[0].data_ptr(), d.txc[0].data_ptr(), None, None, None, 0.0, 1.0, 0, n, n, n)
        fu = rows_of(final_updates)["k_final_update"]
        show(np_, "k_final_update", fu)
        rate = fu["bytes"] / (fu["ms"] * 1e-3)
        res["final_update_TBps"] = rate / 1e12
        res["budget_ms"] = 2.0 * res["bytes_per_substep"] / rate * 1e3
        res["sorted_over_budget"] = res["ms_sorted"] / res["budget_ms"]
        res["within_budget"] = bool(res["ms_sorted"] <= res["budget_ms"])
        res["fields_finite"] = all(bool(torch.isfinite(t).all()) for t in d.q + d.s + d.l_q)
        print(json.dumps(res))
        d.set_particles("none")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
