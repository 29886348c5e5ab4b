"""Cost of the cloud-top physics in the device substep: the single-domain driver at n^3 with two scalars, AirWaterLinear mixture; the infrared source
off / on interleaved in one process on the same arrays (events around whole substeps, median per substep), then the kernel table of one step with the
source on: the rows of k_infrared_y, k_airwater_linear and of k_final_update, run on one field for the rate.  Two variants:
  downward   flux_bottom = 0: l twice, the intermediate written and read, hs read and written (6 field passes)
  both       both fluxes: the stored transmission written and read and l once more (9 passes)
The budget: the launch within 2 x its algorithmic bytes / the rate k_final_update reaches in the same run (the margin is for the two dependent
sweeps and the exp).  Also printed: the substep with nothing set (no mixture), for the comparison with the parent commit.
    python tools/infrared_time.py [--n 512] [--rounds 5] [--steps 4]       (prints the kernel rows and one JSON line per variant)"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4, help="RK3 steps per round and variant")
    a = ap.parse_args()
    import tlab_amd as T
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    T.init(0)
    n = a.n
    x = np.arange(n) / n
    y = np.arange(n) / (n - 1.0)
    d = Dns(x, y, x.copy(), nscal=2, visc=1.0 / 5000.0, schmidt=(1.0, 1.0), yuniform=True, hyper_bc1_ext=0.0)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    wall = torch.sin(np.pi * torch.linspace(0, 1, n, dtype=torch.float64, device="cuda")).view(1, n, 1)

    def fill():
        for t in d.q:
            t.copy_(((2 * torch.rand(n, n, n, dtype=torch.float64, device="cuda", generator=g) - 1) * wall).reshape(-1))
        for t in d.s:
            t.copy_(torch.rand(n ** 3, dtype=torch.float64, device="cuda", generator=g))
        if d.liquid is not None:
            d.FI_DIAGNOSTIC()
    dt = 1e-3
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    variants = {"downward": (1, 2, 2.0, -1.0, 0.0), "both": (1, 2, 2.0, -1.0, 0.5)}

    def timed_steps(ir):
        if d.liquid is not None:
            d.set_infrared(*(ir or (0, 0, 0.0, 0.0, 0.0)))
        ms = []
        for _ in range(a.steps):
            d.begin_step()
            for k in range(3):
                ev[0].record()
                d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(dt * d.kdt[k], d.kco[k] if k < 2 else 1.0, k < 2)
                ev[1].record()
                ev[1].synchronize()
                ms.append(ev[0].elapsed_time(ev[1]))
        return ms
    med = lambda v: float(np.median(v))      # noqa: E731
    fill()
    timed_steps(None)
    plain = []
    for _ in range(a.rounds):
        plain += timed_steps(None)                 # nothing set: the kernels of a driver without the feature
    print(json.dumps({"variant": "nothing set", "n": n, "nscal": 2, "substeps": len(plain), "ms_substep": med(plain),
                      "ms_substep_p10_p90": [float(np.percentile(plain, 10)), float(np.percentile(plain, 90))]}))
    d.set_mixture("airwaterlinear", (-1.0, 0.5, 0.0))
    fill()
    timed_steps(None)
    for v in variants.values():
        timed_steps(v)                             # warm-up of every route
    off, on = [], {k: [] for k in variants}
    for _ in range(a.rounds):
        off += timed_steps(None)
        for k, v in variants.items():
            on[k] += timed_steps(v)
    L = load()
    spread = [float(np.percentile(off, 10)), float(np.percentile(off, 90))]
    for name, v in variants.items():
        d.set_infrared(*v)
        L.tlab_profile_reset(); L.tlab_profile_enable(1)
        d.TIME_RUNGEKUTTA(dt)
        # the yardstick of the budget: k_final_update on one field of this run (dte = 0: the field keeps its values; the scratch tendency is spent)
        for _ in range(3):
            L.tlab_pw_final_update(d.s[0].data_ptr(), d.txc[0].data_ptr(), None, None, None, 0.0, 1.0, 0, n, n, n)
        torch.cuda.synchronize()
        L.tlab_profile_enable(0)
        buf = ctypes.create_string_buffer(32768)
        L.tlab_profile_report(buf, len(buf))
        rows = {}
        for r in buf.value.decode().splitlines():
            f = r.split("\t")
            if len(f) == 4:
                rows[f[0]] = {"calls": int(f[1]), "ms": float(f[2]), "bytes": float(f[3])}
        for k in ("k_infrared_y", "k_airwater_linear", "k_final_update"):
            r = rows[k]
            print("%-10s %-18s calls %3d   ms/call %.4f   algorithmic GB/call %.4f   TB/s %.2f" % (name, k, r["calls"], r["ms"] / r["calls"],
                                                                                                 r["bytes"] / r["calls"] / 1e9, r["bytes"] / r["ms"] / 1e9))
        fu, ir, aw = rows["k_final_update"], rows["k_infrared_y"], rows["k_airwater_linear"]
        rate = fu["bytes"] / (fu["ms"] * 1e-3)                                       # B/s of k_final_update in this run
        new_bytes = ir["bytes"] / ir["calls"]                                        # algorithmic bytes of the new launch per substep
        launch_ms = ir["ms"] / ir["calls"]
        print(json.dumps({"variant": name, "n": n, "nscal": 2, "substeps_per_variant": len(off), "ms_substep_nothing_set": med(plain),
                          "ms_substep_mixture_source_off": med(off), "ms_substep_source_off_p10_p90": spread, "ms_substep_source_on": med(on[name]),
                          "ms_added_by_source": med(on[name]) - med(off), "ms_added_by_liquid_refresh": med(off) - med(plain),
                          "infrared_bytes_per_substep": new_bytes, "infrared_ms_per_launch": launch_ms, "infrared_TBps": new_bytes / launch_ms / 1e9,
                          "airwater_ms_per_launch": aw["ms"] / aw["calls"], "final_update_TBps": rate / 1e12, "budget_ms": 2.0 * new_bytes / rate * 1e3,
                          "within_budget": bool(launch_ms <= 2.0 * new_bytes / rate * 1e3)}))


if __name__ == "__main__":
    main()
