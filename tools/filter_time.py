"""Cost of DNS_FILTER on the device at n^3, fp64, u, v, w and one scalar, in one process: the streaming in-place kernels of
csrc/filter_stream.hip (Dns.DNS_FILTER -> tlab_dns_filter, four fields a launch) against the route a host had to take before them, tlab_opr_filter
on the same four fields one after the other with one tmp (k_filter1d: out of place, a device copy after every application, two transposes along x).
Per filter type (compact, explicit6, explicit4, compactcutoff), periodic along x and z and biased along y: each direction alone, then x, y, z.
  wall      ms per call of the whole route, ending in a device synchronise: medians of --rounds rounds of --calls calls after a warm-up call, the
            two routes alternated round by round
  kernel    the library's own event timing (tlab_profile_*) of k_filter_stream_x / _y / _z: ms per launch, algorithmic bytes (sweeps x 16 B per
            point and field), their ratio as a share of 8 TB/s
The coefficient tables are those of the 64-point fixtures (tests/golden/filters.npz) stretched to n rows -- the first and the last 32 rows kept,
the middle row repeated -- which times the kernels on tables of the right shape; the results are compared between the two routes, word for word,
not with a reference.
    python tools/filter_time.py [--n 512] [--calls 3] [--rounds 3]
prints rows and one JSON line.  The clock state is whatever the shared box gives: the old route's row of the same process is the comparison."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402

TYPES = {1: "compact", 2: "explicit6", 3: "explicit4", 9: "compactcutoff"}
SWEEPS = {(1, 0): 2, (1, 1): 2, (2, 0): 1, (2, 1): 1, (3, 0): 1, (3, 1): 1, (9, 0): 2, (9, 1): 3}      # (type, periodic) -> sweeps over a line
PEAK = 8.0e12


def stretch(c, n):
    """a table of n rows from one of 64: both ends kept, the middle row repeated"""
    if c.shape[1] == 0:
        return None
    h = c.shape[0] // 2
    return np.concatenate([c[:h], np.repeat(c[h:h + 1], n - 2 * h, axis=0), c[-h:]], axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--calls", type=int, default=3, help="timed calls per round")
    ap.add_argument("--rounds", type=int, default=3, help="rounds per row (the median is reported, min and max beside it)")
    a = ap.parse_args()
    import tlab_amd as T
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    T.init(0)
    L = load()
    n = a.n
    G = np.load(os.path.join(ROOT, "tests", "golden", "filters.npz"))
    x = np.arange(n) / n * 2.0
    z = np.arange(n) / n
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(n) / (n - 1) - 1)) / np.tanh(1.5))
    d = Dns(x, y, z, nscal=1, visc=1.0 / 800.0, schmidt=(0.7,), yuniform=False)
    g = torch.Generator(device="cuda").manual_seed(7)
    for t in d.q + d.s:
        t.copy_(torch.rand(n ** 3, dtype=torch.float64, device="cuda", generator=g) * 2.0 - 1.0)
    state = [t.clone() for t in d.q + d.s]
    tmp = torch.empty_like(d.q[0])
    fields = d.q + d.s

    def restore():
        for t, r in zip(fields, state):
            t.copy_(r)

    def wall_pair(new, old):
        """[median, min, max] ms per call of each route, the rounds alternated"""
        for fn in (new, old):
            fn()
        torch.cuda.synchronize()
        v = {0: [], 1: []}
        for _ in range(a.rounds):
            for k, fn in enumerate((new, old)):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                torch.cuda.synchronize()
                v[k].append((time.perf_counter() - t0) / a.calls * 1e3)
        return [[statistics.median(w), min(w), max(w)] for w in (v[0], v[1])]

    def kernel_rows(fn):
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
            c = r.split("\t")
            if len(c) == 4:
                out[c[0]] = {"calls": int(c[1]), "ms": float(c[2]), "bytes": float(c[3])}
        return out

    res = {"n": n, "calls": a.calls, "rounds": a.rounds, "cases": {}}
    slower = []
    print("n = %d, four fields (u, v, w, one scalar); wall ms per call [median, min, max]" % n, flush=True)
    for t, name in TYPES.items():
        c_per = stretch(G["n64_t%d_p1_b00_coeffs" % t], n)
        c_bia = stretch(G["n64_t%d_p0_b11_coeffs" % t], n)
        fper = T.Filter(t, n, True, c_per)
        fbia = T.Filter(t, n, False, c_bia, 1, 1)
        for label, fl in (("x", (fper, None, None)), ("y", (None, fbia, None)), ("z", (None, None, fper)), ("xyz", (fper, fbia, fper))):
            d.set_filter(*fl)

            def new():
                d.DNS_FILTER()

            def old():
                for f in fields:
                    T.OPR_FILTER(n, n, n, fl[0], fl[1], fl[2], f, tmp)
            # the two routes on the same input: equal word for word
            restore(); new(); got = [f.clone() for f in fields]
            restore(); old()
            differing = sum(int((gf.view(torch.int64) != f.view(torch.int64)).sum().item()) for gf, f in zip(got, fields))
            finite = all(bool(torch.isfinite(gf).all().item()) for gf in got)
            del got
            restore()
            w_new, w_old = wall_pair(new, old)
            restore()
            rows = kernel_rows(new)
            restore()
            case = {"wall_new_ms": w_new, "wall_old_ms": w_old, "old_over_new": w_old[0] / w_new[0], "words_differing": differing, "finite": finite,
                    "kernels": {}}
            print("%-13s %-3s  new %8.3f [%8.3f, %8.3f]   old %8.3f [%8.3f, %8.3f]   old / new %6.2f   words differing between the routes %d%s"
                  % (name, label, *w_new, *w_old, case["old_over_new"], differing, "" if finite else "   NOT FINITE"), flush=True)
            for tag, r in sorted(rows.items()):
                if not tag.startswith("k_filter_stream"):
                    continue
                ms, by = r["ms"] / r["calls"], r["bytes"] / r["calls"]
                per = 0 if tag.endswith("_y") else 1
                budget_ms = by / PEAK * 1e3
                case["kernels"][tag] = {"ms": ms, "bytes": by, "sweeps": SWEEPS[(t, per)], "share_of_8TBps": by / (ms * 1e-3) / PEAK,
                                        "time_over_byte_budget": ms / budget_ms}
                print("    %-18s kernel ms %8.3f   sweeps %d   algorithmic GB %7.3f   share of 8 TB/s %.3f   time / byte budget %.2f"
                      % (tag, ms, SWEEPS[(t, per)], by / 1e9, case["kernels"][tag]["share_of_8TBps"], ms / budget_ms), flush=True)
            res["cases"]["%s_%s" % (name, label)] = case
            if not w_new[0] < w_old[0] or differing or not finite:
                slower.append("%s_%s" % (name, label))
        d.set_filter(None, None, None)
        del fper, fbia
    res["not_faster_or_not_equal"] = slower
    print("cases in which the new route is not faster than the old one, or differs from it: %s" % (slower or "none"), flush=True)
    print(json.dumps(res))
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
