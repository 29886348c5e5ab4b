"""Cost of the relaxation buffer zones ([BufferZone] Type = relaxation) in the device substep: the single-domain driver at n^3 with one scalar and
a zone of 20 planes at Jmax for the flow and the scalar (ParametersU = ParametersS = 1.57, 2.0), zones off / on interleaved in one process on the
same arrays (events around whole substeps, median per substep), then the kernel table of one step with zones on: the rows of the zone kernel and
of k_final_update, run on one field for the rate.  The budget: added time <= 2 x the algorithmic bytes of the new kernels (plus the scalar's
separate update pass on the routes that need one; the Dirichlet route here does not) / the rate k_final_update reaches in the same run.
    python tools/buffer_time.py [--n 512] [--points 20] [--rounds 5] [--steps 4]       (prints the kernel rows and one JSON line)"""
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
    ap.add_argument("--points", type=int, default=20)
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
    d = Dns(x, y, x.copy(), nscal=1, visc=1.0 / 5000.0, schmidt=(1.0,), yuniform=True, hyper_bc1_ext=0.0)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    wall = torch.sin(np.pi * torch.linspace(0, 1, n, dtype=torch.float64, device="cuda")).view(1, n, 1)
    for t in d.q:
        t.copy_(((2 * torch.rand(n, n, n, dtype=torch.float64, device="cuda", generator=g) - 1) * wall).reshape(-1))
    d.s[0].copy_(torch.rand(n ** 3, dtype=torch.float64, device="cuda", generator=g))
    dt = 1e-3
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    zones = lambda on: d.set_buffer_zones(0, a.points if on else 0, (1.57, 2.0), (1.57, 2.0))      # noqa: E731

    def timed_steps(on):
        zones(on)
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
    timed_steps(False); timed_steps(True)          # warm-up of both routes
    off, on = [], []
    for _ in range(a.rounds):
        off += timed_steps(False)
        on += timed_steps(True)
    L = load()
    zones(True)
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
    new = [k for k in rows if k.startswith("k_buffer_relax")]
    for name in new + ["k_rk_update", "k_final_update"]:
        if name in rows:
            r = rows[name]
            print("%-28s calls %3d   ms/call %.4f   algorithmic GB/call %.4f   TB/s %.2f" % (name, r["calls"], r["ms"] / r["calls"], r["bytes"] / r["calls"] / 1e9,
                                                                                            r["bytes"] / r["ms"] / 1e9))
    med = lambda v: float(np.median(v))      # noqa: E731
    out = {"n": n, "nscal": 1, "points_jmax": a.points, "substeps_per_variant": len(off), "ms_substep_zones_off": med(off), "ms_substep_zones_on": med(on),
           "ms_added": med(on) - med(off)}
    fu = rows["k_final_update"]
    rate = fu["bytes"] / (fu["ms"] * 1e-3)                                       # B/s of k_final_update in this run
    zone_bytes = sum(rows[k]["bytes"] for k in new) / 3.0                        # algorithmic bytes of the new kernels per substep
    extra = rows["k_rk_update"]["bytes"] / 3.0 if "k_rk_update" in rows else 0.0  # a separate update pass of the scalar, on the routes that need one
    out.update({"zone_bytes_per_substep": zone_bytes, "scalar_pass_bytes_per_substep": extra, "final_update_TBps": rate / 1e12,
                "zone_kernels_ms_per_substep": sum(rows[k]["ms"] for k in new) / 3.0,
                "budget_ms": 2.0 * (zone_bytes + extra) / rate * 1e3, "within_budget": bool(med(on) - med(off) <= 2.0 * (zone_bytes + extra) / rate * 1e3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
