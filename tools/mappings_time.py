"""Cost of the field mappings on the device at n^3, fp64, one scalar, in one process (kernel times are the library's own event timing,
tlab_profile_*; wall times end in a device synchronise):
  the pass      k_gradient_maps for P + Q + R (12 arrays: 96 B/point), for the enstrophy set VORTICITY + VORTICITY_PRODUCTION + P, and for all
                maps (12 inputs, 22 outputs): kernel ms and TB/s on the algorithmic bytes, beside k_vorticity_magnitude (7 arrays) timed in the
                same process, and the ratio of the two rates.
  end to end    Dns.invariants() and Dns.enstrophy_equation() against the reference's literal call sequence on the same device: every
                OPR_Partial the reference makes, through the public operators, with torch for the pointwise lines (tests/mappings_oracle.py run
                on device tensors: FI_INVARIANT_R, _Q, _P -- 23 calls; FI_VORTICITY_PRODUCTION, FI_VORTICITY_DIFFUSION, FI_VORTICITY,
                FI_INVARIANT_P with the scalings -- 39 calls, and with FI_CURL, whose only use is the Baroclinic entry that is left out, 45).
    python tools/mappings_time.py [--n 512] [--calls 10] [--out FILE]
prints rows and one JSON line; --out also writes them to FILE."""
import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per row")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mappings_oracle as M
    import tlab_amd as T
    from tlab_amd.dns import Dns
    from tlab_amd.lib import load
    T.init(0)
    L = load()
    n = a.n
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

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
    N = d.n

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

    # ---- the pass beside k_vorticity_magnitude ----
    new = lambda k: [torch.empty(N, dtype=torch.float64, device="cuda") for _ in range(k)]      # noqa: E731
    ds3 = new(3)
    T.velocity_gradients(d, d.q, d.txc[:9])
    T.scalar_gradient(d, d.s[0], ds3)
    du9 = [t[:N] for t in d.txc[:9]]
    vout = new(1)[0]
    sets = (("P + Q + R", ["P", "Q", "R"]), ("VORTICITY + VORTICITY_PRODUCTION + P", ["VORTICITY", "VORTICITY_PRODUCTION", "P"]), ("all maps", list(M.MAPS)))
    outs = {name: new(sum(M.NOUT[m] for m in maps)) for name, maps in sets}
    rates = {name: [] for name, _ in sets}
    yard = []
    for _ in range(3):      # alternated, all kept
        r = rows_of(lambda: T.vorticity_from_gradients(du9[3], du9[1], du9[2], du9[6], du9[7], du9[5], result=vout), a.calls)["k_vorticity_magnitude"]
        yard.append((r["ms"] / r["calls"], r["bytes"] / (r["ms"] * 1e-3) / 1e12))
        for name, maps in sets:
            r = rows_of(lambda: T.gradient_maps(du9, ds3, maps, out=outs[name]), a.calls)["k_gradient_maps"]
            rates[name].append((r["ms"] / r["calls"], r["bytes"] / r["calls"], r["bytes"] / (r["ms"] * 1e-3) / 1e12))
    ymean = sum(v[1] for v in yard) / 3
    res["k_vorticity_magnitude_ms"], res["k_vorticity_magnitude_TBps"] = [v[0] for v in yard], [v[1] for v in yard]
    say("%-40s kernel ms %s   algorithmic GB %7.3f   TB/s %s (mean %.3f)   (7 arrays; the yardstick)"
        % ("k_vorticity_magnitude", ", ".join("%.4f" % v[0] for v in yard), 56.0 * N / 1e9, ", ".join("%.3f" % v[1] for v in yard), ymean))
    for name, maps in sets:
        v = rates[name]
        mean = sum(t[2] for t in v) / 3
        res["pass " + name] = {"ms": [t[0] for t in v], "bytes": v[0][1], "TBps": [t[2] for t in v], "rate_over_vorticity_magnitude": mean / ymean}
        say("%-40s kernel ms %s   algorithmic GB %7.3f   TB/s %s (mean %.3f)   %d arrays, %d B/point; rate / k_vorticity_magnitude %.3f"
            % ("k_gradient_maps: " + name, ", ".join("%.4f" % t[0] for t in v), v[0][1] / 1e9, ", ".join("%.3f" % t[2] for t in v), mean,
               round(v[0][1] / N / 8), round(v[0][1] / N), mean / ymean))
    del outs, vout

    # ---- end to end against the reference's literal call sequence on the public operators ----
    P = (T.OPR_Partial_X, T.OPR_Partial_Y, T.OPR_Partial_Z)
    calls = [0]

    def p1(dd, f):
        r = torch.empty(N, dtype=torch.float64, device="cuda")
        P[dd - 1](T.OPR_P1, n, n, n, 0, d.g[dd - 1], f, r)
        calls[0] += 1
        return r

    def p2(dd, f):
        r, w = torch.empty(N, dtype=torch.float64, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda")
        P[dd - 1](T.OPR_P2, n, n, n, 0, d.g[dd - 1], f, r, w)
        calls[0] += 1
        return r
    u, v, w = d.q

    def literal_invariants():
        return {"InvariantR": M.fi_invariant_r(p1, u, v, w), "InvariantQ": M.fi_invariant_q(p1, u, v, w), "InvariantP": M.fi_invariant_p(p1, u, v, w)}

    def literal_enstrophy(curl=False):
        if curl:
            M.fi_curl(p1, u, v, w)
        prod = M.fi_vorticity_production(p1, u, v, w)
        dif = d.visc * M.fi_vorticity_diffusion(p1, p2, u, v, w)
        ens = M.fi_vorticity(p1, u, v, w)
        dil = M.fi_invariant_p(p1, u, v, w) * ens
        return {"EnstrophyW_iW_i": ens, "LnEnstrophyW_iW_i": torch.log(ens), "ProductionW_iW_jS_ij": prod, "DiffusionNuW_iLapW_i": dif,
                "DilatationMsW_iW_iDivU": dil, "RateAN_iN_jS_ij": prod / ens}

    def same(got, want):      # the new calls compute what the literal sequence computes: equal bits for the first-derivative entries
        return {k: bool(torch.equal(got[k], want[k])) for k in want}
    for name, new_fn, lit_fn, variants in (("Dns.invariants()", d.invariants, literal_invariants, ()),
                                           ("Dns.enstrophy_equation()", d.enstrophy_equation, literal_enstrophy, (("with FI_CURL", lambda: literal_enstrophy(True)),))):
        calls[0] = 0
        want = lit_fn()
        ncalls = calls[0]
        eq = same(new_fn(), want)
        del want
        wn, wl = [], []
        for _ in range(3):      # alternated, all kept
            wn.append(wall_of(new_fn, a.calls))
            wl.append(wall_of(lit_fn, a.calls))
        mn, ml = sum(wn) / 3, sum(wl) / 3
        res[name] = {"new_ms": wn, "literal_ms": wl, "literal_opr_partial_calls": ncalls, "literal_over_new": ml / mn, "equal_bits": eq}
        say("%-26s wall ms per call %s (mean %.3f); the literal sequence of %d OPR_Partial calls: %s (mean %.3f); literal / new %.2f; entries with equal bits: %s"
            % (name, ", ".join("%.3f" % t for t in wn), mn, ncalls, ", ".join("%.3f" % t for t in wl), ml, ml / mn,
               ", ".join(k for k, e in eq.items() if e) or "none"))
        for tag, fn in variants:
            calls[0] = 0
            fn()
            nc = calls[0]
            t = wall_of(fn, a.calls)
            res[name][tag] = {"literal_ms": t, "literal_opr_partial_calls": nc}
            say("%-26s %s: %d OPR_Partial calls, wall ms per call %.3f; literal / new %.2f" % ("", tag, nc, t, t / mn))
    say(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
