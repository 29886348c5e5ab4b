"""Cost of the sampling between two statistics steps on the device at n^3, fp64, one scalar, in one process (wall times end in a device synchronise
and are medians of --rounds rounds of --calls calls after a warm-up call; kernel times are the library's own event timing, tlab_profile_*):
  phase       k_phase_space in its fused flow form (u, v, w read once: 24 n^3 bytes, 9 fp64 divisions per point and plane): kernel time and
              algorithmic bytes over time, next to what k_plane_partial<MEANS> reaches on the same three fields in the same process -- the
              yardstick -- and tools/phase_divide_probe (the same loop with and without the division) as a child process; then
              tlab_avg_phase_space for one field and for the scalars.
  towers      one time step's tower work, the three calls 4, 1, 2 with Stride = 16, 1, 16, against a time step of the same driver
  planes      Dns.PLANES_SAVE of two j-, two k- and two i-planes, with and without log
  armed       the last substep armed (towers and phase average) against unarmed, alternated
    python tools/sampling_time.py [--n 512] [--calls 5] [--rounds 5]
prints rows and one JSON line.  The clock state is whatever the shared box gives: the yardstick row of the same process is the comparison."""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--calls", type=int, default=5, help="timed calls per round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds per row (the median is reported, min and max beside it)")
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
    ax = torch.arange(n, dtype=torch.float64, device="cuda") * (2.0 * math.pi / n)
    wall = torch.sin(math.pi * torch.as_tensor(y, device="cuda"))[None, :, None]
    g = torch.Generator(device="cuda").manual_seed(7)
    for i, t in enumerate(d.q + d.s):      # smooth fields that vanish on the walls, with a little noise
        X, Z = torch.sin((1 + i) * ax + 0.3 * i)[None, None, :], torch.cos(2.0 * ax + i)[:, None, None]
        t.copy_(((X * Z + 0.1 * (torch.rand((n, n, n), dtype=torch.float64, device="cuda", generator=g) * 2.0 - 1.0)) * wall).reshape(-1))
    torch.cuda.synchronize()
    state = [t.clone() for t in d.q + d.s]

    def restore():
        for t, r in zip(d.q + d.s, state):
            t.copy_(r)

    def rows_of(fn, calls):
        fn()
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

    def wall_of(fn):
        """[median, min, max] of the rounds, ms per call"""
        fn()
        torch.cuda.synchronize()
        v = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t0) / a.calls * 1e3)
        return [statistics.median(v), min(v), max(v)]

    res = {"n": n, "calls": a.calls, "rounds": a.rounds}

    def kernel_row(tag, rows, note=""):
        r = rows[tag]
        ms, by = r["ms"] / r["calls"], r["bytes"] / r["calls"]
        res[tag] = {"kernel_ms": ms, "bytes": by, "TBps": by / (ms * 1e-3) / 1e12}
        print("%-28s kernel ms %8.4f   algorithmic GB %7.3f   TB/s %.3f   %s" % (tag, ms, by / 1e9, res[tag]["TBps"], note), flush=True)
        return res[tag]

    # ---- phase averages ----
    planes = 4
    avg_flow = torch.zeros((3, planes + 1, n, n), dtype=torch.float64, device="cuda")
    avg_stress = torch.zeros((6, planes + 1, n, n), dtype=torch.float64, device="cuda")
    avg_one = torch.zeros((1, planes + 1, n, n), dtype=torch.float64, device="cuda")
    calls = a.calls * a.rounds
    yard = kernel_row("k_plane_partial<MEANS>", rows_of(lambda: T.avg_ik_v(n, n, n, d.q), calls), "(the yardstick: three fields, one pass)")
    flow = kernel_row("k_phase_space<flow>", rows_of(lambda: T.avg_phase_flow(n, n, n, d.q[0], d.q[1], d.q[2], planes, 2, avg_flow, avg_stress), calls))
    res["phase_flow_over_yardstick"] = flow["TBps"] / yard["TBps"]
    print("k_phase_space<flow> reaches %.3f of the yardstick's bandwidth" % res["phase_flow_over_yardstick"], flush=True)
    one = kernel_row("k_phase_space", rows_of(lambda: T.avg_phase_space(n, n, n, d.s, planes, 2, avg_one), calls), "(one field: the scalars, or p)")
    res["avg_phase_space_one_field_wall_ms"] = wall_of(lambda: T.avg_phase_space(n, n, n, d.s, planes, 2, avg_one))
    res["avg_phase_flow_wall_ms"] = wall_of(lambda: T.avg_phase_flow(n, n, n, d.q[0], d.q[1], d.q[2], planes, 2, avg_flow, avg_stress))
    print("wall ms per call [median, min, max]: avg_phase_space(one field) %s; avg_phase_flow %s"
          % (res["avg_phase_space_one_field_wall_ms"], res["avg_phase_flow_wall_ms"]), flush=True)
    del avg_flow, avg_stress, avg_one, one
    probe = os.path.join(ROOT, "tools", "phase_divide_probe")
    if os.path.exists(probe):
        torch.cuda.synchronize()
        r = subprocess.run([probe, str(n), "15"], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            res["divide_probe"] = json.loads(r.stdout.strip().splitlines()[-1])
            print("phase_divide_probe: %s" % r.stdout.strip(), flush=True)
        else:
            print("phase_divide_probe failed (%d): %s" % (r.returncode, r.stderr.strip()), flush=True)
    else:
        print("phase_divide_probe is not built: division against multiplication not measured", flush=True)

    # ---- towers against a time step ----
    d.set_towers((16, 1, 16), 64)
    p = d.txc[2][: d.n]
    p.copy_(state[0])

    def towers():
        d.tower_reset()
        d.tower.accumulate(4, [p], 1, 0.1, d.tower_buf)
        d.tower_accumulate(1, 0.1)

    def step():
        d.TIME_RUNGEKUTTA(1e-5)
    res["tower_step_wall_ms"] = wall_of(towers)
    res["time_step_wall_ms"] = wall_of(step)
    restore()
    res["tower_share_of_step"] = res["tower_step_wall_ms"][0] / res["time_step_wall_ms"][0]
    print("towers, one time step (calls 4, 1, 2; Stride 16,1,16; %d x %d x %d towers): wall ms [median, min, max] %s; a time step of the same driver %s; "
          "share %.4f" % (d.tower.imax, d.tower.jmax, d.tower.kmax, res["tower_step_wall_ms"], res["time_step_wall_ms"], res["tower_share_of_step"]), flush=True)
    rows = rows_of(towers, a.calls)
    res["tower_kernels"] = {k: {"ms": r["ms"] / a.calls, "launches": r["calls"] / a.calls} for k, r in sorted(rows.items())}
    print("towers kernel ms per step (launches): %s" % ", ".join("%s %.4f (%g)" % (k, v["ms"], v["launches"]) for k, v in res["tower_kernels"].items()), flush=True)

    # ---- armed against unarmed last substep ----
    d.set_phase_average(1, 0, 4)
    kdt, last = d.kdt[-1], d.rkm_endstep - 1

    def substep(armed):
        def run():
            d.tower_reset()
            if armed:
                d._arm_pressure_sampling(0, 0.1)
            d.TIME_SUBSTEP_INCOMPRESSIBLE_EXPLICIT(1e-5 * kdt, 1.0, False)
        return run
    un, ar = [], []
    for _ in range(3):      # alternated
        un.append(wall_of(substep(False))[0])
        ar.append(wall_of(substep(True))[0])
    restore()
    res["last_substep_unarmed_wall_ms"], res["last_substep_armed_wall_ms"] = un, ar
    print("last substep (%d of %d), wall ms, medians of three alternated runs: unarmed %s, armed %s; difference of the medians %.4f ms"
          % (last + 1, d.rkm_endstep, un, ar, statistics.median(ar) - statistics.median(un)), flush=True)

    # ---- PLANES_SAVE ----
    nodes = dict(iplanes=(1, n // 2), jplanes=(1, n // 2), kplanes=(1, n // 2))
    for log in (False, True):
        key = "planes_save_log_wall_ms" if log else "planes_save_wall_ms"
        res[key] = wall_of(lambda: d.PLANES_SAVE(log=log, **nodes))
        print("Dns.PLANES_SAVE(two i-, two j-, two k-planes, log=%s, single): wall ms [median, min, max] %s" % (log, res[key]), flush=True)
    rows = rows_of(lambda: d.PLANES_SAVE(log=True, **nodes), a.calls)
    for tag in ("k_planes_gather", "k_gradient_magnitude", "k_log10_small"):
        if tag in rows:
            r = rows[tag]
            print("%-28s kernel ms per launch %8.4f (%g launches a call)   TB/s %.3f" % (tag, r["ms"] / r["calls"], r["calls"] / a.calls,
                                                                                         r["bytes"] / (r["ms"] * 1e-3) / 1e12), flush=True)
            res[tag] = {"kernel_ms": r["ms"] / r["calls"], "TBps": r["bytes"] / (r["ms"] * 1e-3) / 1e12}
    # the worst distance of the device's log10 from numpy's, in ulp of the result (tests/test_gpu_sampling.py bounds it by 4)
    rng = np.random.default_rng(7)
    h = np.concatenate([10.0 ** rng.uniform(-25, 12, 1 << 20), rng.uniform(0.5, 2.0, 1 << 20)])
    got = T.log10_small(torch.from_numpy(h).cuda()).cpu().numpy()
    want = np.log10(h + 1.0e-20)
    res["log10_small_worst_ulp"] = float((np.abs(got - want) / np.spacing(np.abs(want))).max())
    print("log10_small: worst distance to numpy over %d values %.2f ulp" % (h.size, res["log10_small_worst_ulp"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
