"""Cost of the head of DNS_STATISTICS_TEMPORAL (dns_statistics.f90:93-117) on the device at n^3, fp64, one scalar, in one process (wall times end in
a device synchronise; kernel times are the library's own event timing, tlab_profile_*):
  pressure      one tlab_dns_pressure call, DCMP_TOTAL with a Coriolis term and a linear buoyancy: wall time, the per-kernel table, and the wall
                time of a full Runge-Kutta substep of the SAME driver as the yardstick -- the call makes the substep's Burgers, forcing and solve
                launches without the scalar equation, the gradient and the update, so it must not take longer; the ratio is printed.
  intermittency k_vorticity_magnitude (7 field passes: 56 n^3 bytes) and k_gate_count (n^3 bytes) against the project's budget, 2 x bytes at the
                rate k_final_update reaches in the same run: kernel time, TB/s, share of the budget; then the wall time of Dns.intermittency().
    python tools/statistics_head_time.py [--n 512] [--calls 10]
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

FORCES = dict(coriolis={"type": "explicit", "vector": (0.0, 1.5, 0.0)}, buoyancy={"type": "linear", "vector": (0.0, -2.0, 0.0), "parameters": (1.0, 0.1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per row")
    a = ap.parse_args()
    import tlab_amd as T
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    T.init(0)
    L = load()
    n = a.n
    x = np.arange(n) / n * 2.0
    z = np.arange(n) / n
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(n) / (n - 1) - 1)) / np.tanh(1.5))
    d = Dns(x, y, z, nscal=1, visc=1.0 / 800.0, schmidt=(0.7,), yuniform=False)
    d.set_body_forces(FORCES["coriolis"], FORCES["buoyancy"])
    ax = torch.arange(n, dtype=torch.float64, device="cuda") * (2.0 * math.pi / n)
    wall = torch.sin(math.pi * torch.as_tensor(y, device="cuda"))[None, :, None]
    g = torch.Generator(device="cuda").manual_seed(7)
    for i, t in enumerate(d.q + d.s):      # smooth fields that vanish on the walls, with a little noise
        X, Z = torch.sin((1 + i) * ax + 0.3 * i)[None, None, :], torch.cos(2.0 * ax + i)[:, None, None]
        t.copy_(((X * Z + 0.1 * (torch.rand((n, n, n), dtype=torch.float64, device="cuda", generator=g) * 2.0 - 1.0)) * wall).reshape(-1))
    torch.cuda.synchronize()

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

    res = {"n": n, "calls_per_row": a.calls}
    fu = rows_of(lambda: L.tlab_pw_final_update(d.txc[7].data_ptr(), d.txc[8].data_ptr(), None, None, None, 0.0, 1.0, 0, n, n, n), a.calls)["k_final_update"]
    rate = fu["bytes"] / (fu["ms"] * 1e-3)
    res["final_update_TBps"] = rate / 1e12
    print("%-26s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   (the yardstick)"
          % ("k_final_update", fu["ms"] / fu["calls"], fu["bytes"] / fu["calls"] / 1e9, rate / 1e12), flush=True)

    # ---- the pressure against a substep of the same driver ----
    pressure = lambda: d.FI_PRESSURE_BOUSSINESQ()      # noqa: E731

    def substep():      # the first substep of a step: fresh tendencies, as the pressure call counts its sums
        d.begin_step()
        d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(1e-5, -5.0 / 9.0, True)
    walls = {"pressure": [], "substep": []}
    for _ in range(3):      # alternated, all kept
        walls["pressure"].append(wall_of(pressure, a.calls))
        walls["substep"].append(wall_of(substep, a.calls))
    res["pressure_wall_ms"], res["substep_wall_ms"] = walls["pressure"], walls["substep"]
    mp, ms_ = sum(walls["pressure"]) / 3, sum(walls["substep"]) / 3
    res["pressure_over_substep"] = mp / ms_
    print("tlab_dns_pressure, total: wall ms per call %s (mean %.4f); substep of the same driver: %s (mean %.4f); pressure / substep %.3f"
          % (", ".join("%.4f" % v for v in walls["pressure"]), mp, ", ".join("%.4f" % v for v in walls["substep"]), ms_, mp / ms_), flush=True)
    for name, fn in (("pressure", pressure), ("substep", substep)):
        rows = rows_of(fn, a.calls)
        res[name + "_kernels"] = {k: {"ms": r["ms"] / a.calls, "launches": r["calls"] / a.calls} for k, r in sorted(rows.items())}
        print("%-9s kernel ms per call (launches): %s; sum %.4f"
              % (name, ", ".join("%s %.4f (%g)" % (k, r["ms"] / a.calls, r["calls"] / a.calls) for k, r in sorted(rows.items())),
                 sum(r["ms"] for r in rows.values()) / a.calls), flush=True)

    # ---- intermittency ----
    rows = rows_of(lambda: d.FI_VORTICITY(), a.calls)
    gate = T.gate_threshold(d.txc[0][: d.n], 1e-6)
    rows.update(rows_of(lambda: T.inter_n_xz(n, n, n, 1, gate), a.calls))
    for tag in ("k_vorticity_magnitude", "k_gate_count"):
        r = rows[tag]
        ms, by = r["ms"] / r["calls"], r["bytes"] / r["calls"]
        budget = 2.0 * by / rate * 1e3
        res[tag + "_kernel_ms"], res[tag + "_bytes"], res[tag + "_TBps"], res[tag + "_over_budget"] = ms, by, by / (ms * 1e-3) / 1e12, ms / budget
        print("%-26s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   budget ms %8.4f   kernel / budget %.3f"
              % (tag, ms, by / 1e9, res[tag + "_TBps"], budget, ms / budget), flush=True)
    res["intermittency_wall_ms"] = wall_of(lambda: d.intermittency(), a.calls)
    print("Dns.intermittency(): wall ms per call %8.4f (six derivatives, the pass, MINMAX, the gate, the counts, two synchronisations)"
          % res["intermittency_wall_ms"], flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
