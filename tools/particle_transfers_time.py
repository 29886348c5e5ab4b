"""Cost of the transfers between particles and fields (k_particle_sample, k_particle_trajectories, k_particle_deposit): the single-domain driver at
n^3 with one scalar and tracers at uniformly random positions, np = 2^24 and 2^26, and the deposit also at np = n^3 (one particle per cell on
average).  Per particle count, in one process on the same arrays (in-library event timing, tlab_profile_*), unsorted and right after
tlab_dns_particle_sort:
  sample          tlab_dns_field_to_particle of q and s (nvar = 4)
  trajectories    tlab_dns_trajectories_accumulate with q and s behind the positions, ntraj = 2^10 and 2^16 (the default tag list)
  deposit         tlab_dns_particle_to_field of the number density, periodic
  k_final_update  on one field, for the rate of the budget
The budget of the sample and the trajectories: 2 x their algorithmic bytes (from the shapes, as the kernels report them) / the rate k_final_update
reaches in the same run.  The deposit is reported against a yardstick of its own, because nobody has published the fp64 atomic rate of this chip:
tools/atomic_yardstick (consecutive lanes add to consecutive doubles of a 1-GiB array), run as a child process at the end; atomic bytes = np x 64.
    python tools/particle_transfers_time.py [--n 512] [--calls 5] [--np 16777216 67108864] [--np-deposit 134217728]
prints rows and one JSON line per particle count."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--calls", type=int, default=5, help="timed launches per row")
    ap.add_argument("--np", type=int, nargs="*", default=None, help="particle counts of the full table (default 2^24 and 2^26)")
    ap.add_argument("--np-deposit", type=int, nargs="*", default=None, help="particle counts at which only the sorted deposit is timed (default n^3)")
    ap.add_argument("--ntraj", type=int, nargs="*", default=[1 << 10, 1 << 16])
    a = ap.parse_args()
    import tlab_amd as T
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    from bench import synthetic_fields
    T.init(0)
    L = load()
    n = a.n
    full = a.np if a.np is not None else [1 << 24, 1 << 26]
    only_deposit = a.np_deposit if a.np_deposit is not None else [n ** 3]
    x = np.arange(n) / n
    y = np.arange(n) / (n - 1.0)
    d = Dns(x, y, x.copy(), nscal=1, visc=1.0 / 5000.0, schmidt=(1.0,), yuniform=True, hyper_bc1_ext=0.0)
    synthetic_fields(d.q + d.s, n, n, n, 0, n, 0)
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)

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

    def show(np_, name, r):
        ms, gb = r["ms"] / r["calls"], r["bytes"] / r["calls"] / 1e9
        print("np %-9d %-34s calls %3d   ms/call %9.4f   algorithmic GB/call %8.4f   TB/s %.3f" % (np_, name, r["calls"], ms, gb, gb / ms), flush=True)
        return ms, r["bytes"] / r["calls"]

    def final_update_rate():      # dte = 0: the field keeps its values; the scratch tendency is spent
        fu = rows_of(lambda: L.tlab_pw_final_update(d.s[0].data_ptr(), d.txc[0].data_ptr(), None, None, None, 0.0, 1.0, 0, n, n, n))["k_final_update"]
        show(0, "k_final_update", fu)
        return fu["bytes"] / (fu["ms"] * 1e-3)

    results = []
    for np_ in full + only_deposit:
        everything = np_ in full
        d.set_particles("tracer", np_)
        for t in d.l_q:      # uniformly random in the box (y between the walls)
            t.copy_(torch.rand(np_, dtype=torch.float64, device="cuda", generator=gen))
        d.locate_particles()
        res = {"n": n, "np": np_, "calls_per_row": a.calls}
        fields = d.q + d.s
        field = torch.empty(d.n, dtype=torch.float64, device="cuda")
        out = [torch.zeros(np_, dtype=torch.float64, device="cuda") for _ in fields] if everything else None
        for order in (("unsorted", "sorted") if everything else ("sorted",)):
            if order == "sorted":
                d.sort_particles()
            d.PARTICLE_TO_FIELD(out=field)      # first touch
            if everything:
                ms, by = show(np_, "sample nvar 4 %s" % order, rows_of(lambda: d.FIELD_TO_PARTICLE(fields, out))["k_particle_sample"])
                res["sample_ms_" + order], res["sample_bytes"] = ms, by
                for nt in a.ntraj:
                    d.set_trajectories(number=nt, nsave=1, fields=fields)

                    def accumulate():
                        d.traj_counter = 0
                        d.ParticleTrajectories_Accumulate(0.5)
                    ms, by = show(np_, "trajectories ntraj %d %s" % (nt, order), rows_of(accumulate)["k_particle_trajectories"])
                    res["traj%d_ms_%s" % (nt, order)], res["traj%d_bytes" % nt] = ms, by
                    d.set_trajectories(number=0)
            ms, _ = show(np_, "deposit %s" % order, rows_of(lambda: d.PARTICLE_TO_FIELD(out=field))["k_particle_deposit"])
            res["deposit_ms_" + order] = ms
            res["deposit_sum_over_np_" + order] = float(field.sum()) / np_      # 1 up to rounding: nothing was lost
        rate = final_update_rate()
        res["final_update_TBps"] = rate / 1e12
        if everything:
            res["sample_budget_ms"] = 2.0 * res["sample_bytes"] / rate * 1e3
            res["sample_sorted_over_budget"] = res["sample_ms_sorted"] / res["sample_budget_ms"]
            for nt in a.ntraj:
                res["traj%d_budget_ms" % nt] = 2.0 * res["traj%d_bytes" % nt] / rate * 1e3
                res["traj%d_sorted_over_budget" % nt] = res["traj%d_ms_sorted" % nt] / res["traj%d_budget_ms" % nt]
        results.append(res)
        d.set_particles("none")
        del field, out
        torch.cuda.empty_cache()

    # the deposit's yardstick, in a process of its own once this one's arrays are gone
    del d
    torch.cuda.empty_cache()
    yard = subprocess.run([os.path.join(ROOT, "tools", "atomic_yardstick")], capture_output=True, text=True, timeout=300)
    print(yard.stdout.strip(), yard.stderr.strip(), flush=True)
    rate = json.loads(yard.stdout.strip().splitlines()[-1])["TBps_added"] if yard.returncode == 0 else None
    for res in results:
        if rate:
            res["atomic_yardstick_TBps"] = rate
            for order in ("unsorted", "sorted"):
                if "deposit_ms_" + order in res:
                    tb = res["np"] * 64.0 / (res["deposit_ms_" + order] * 1e-3) / 1e12
                    res["deposit_TBps_" + order], res["deposit_fraction_of_yardstick_" + order] = tb, tb / rate
        print(json.dumps(res))


if __name__ == "__main__":
    main()
