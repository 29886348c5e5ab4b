"""Cost of scalar bounds limiting ([Control] ScalLimit) in the device substep: the single-domain driver at n^3 with one scalar, bounds off / on
interleaved in one process on the same arrays (events around whole substeps, median per substep), and the deferred tail replaying time.f90's
sequence with the clips of DNS_BOUNDS_LIMIT (every substep must be fused: tlab_deferred_stats / tlab_deferred_clip_stats).
    python tools/bounds_time.py [--n 512] [--rounds 5] [--steps 4]       (prints one JSON line)"""
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
    from tlab_amd.lib import load, check, c_vp
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
    lo, hi, dt = 0.1, 0.9, 1e-3
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def timed_steps(bounds):
        d.set_scalar_bounds(*bounds) if bounds else d.set_scalar_bounds(None)
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
    timed_steps(None); timed_steps(([lo], [hi]))          # warm-up of both instantiations
    off, on = [], []
    for _ in range(a.rounds):
        off += timed_steps(None)
        on += timed_steps(([lo], [hi]))
    d.set_scalar_bounds(None)
    # the deferred tail: time.f90's calls with the clip of DNS_BOUNDS_LIMIT between the DAXPYs and the DSCALs
    L = load()
    mk = lambda ts: (c_vp * max(1, len(ts)))(*[t.data_ptr() for t in ts])      # noqa: E731
    q, s, hq, hs, txc = mk(d.q), mk(d.s), mk(d.hq), mk(d.hs), mk(d.txc)
    st0, cs0 = (ctypes.c_longlong * 6)(), (ctypes.c_longlong * 2)()
    check(L.tlab_deferred_stats(st0), "stats"); check(L.tlab_deferred_clip_stats(cs0), "clip stats")
    N = d.n
    deferred = []
    check(L.tlab_deferred_enable(1), "enable")
    try:
        for _ in range(a.steps):
            for t in d.hq + d.hs:
                check(L.tlab_deferred_zero(t.data_ptr(), N), "zero")
            for k in range(3):
                dte = dt * d.kdt[k]
                ev[2].record()
                check(L.tlab_deferred_rhs(d._h, dte, q, s, hq, hs, txc), "rhs")
                for h, u in zip(d.hq + d.hs, d.q + d.s):
                    check(L.tlab_deferred_axpy(N, dte, h.data_ptr(), u.data_ptr()), "axpy")
                check(L.tlab_deferred_clip(N, lo, hi, d.s[0].data_ptr()), "clip")
                if k < 2:
                    for h in d.hq + d.hs:
                        check(L.tlab_deferred_scal(N, d.kco[k], h.data_ptr()), "scal")
                else:
                    check(L.tlab_deferred_flush(), "flush")
                ev[3].record()
                ev[3].synchronize()
                deferred.append(ev[2].elapsed_time(ev[3]))
    finally:
        check(L.tlab_deferred_enable(0), "disable")
    st1, cs1 = (ctypes.c_longlong * 6)(), (ctypes.c_longlong * 2)()
    check(L.tlab_deferred_stats(st1), "stats"); check(L.tlab_deferred_clip_stats(cs1), "clip stats")
    dst = [b - c for b, c in zip(st1, st0)]
    dcs = [b - c for b, c in zip(cs1, cs0)]
    s0 = d.s[0]
    med = lambda v: float(np.median(v))      # noqa: E731
    print(json.dumps({"n": n, "nscal": 1, "substeps_per_variant": len(off), "ms_substep_bounds_off": med(off), "ms_substep_bounds_on": med(on),
                      "ratio_on_off": med(on) / med(off), "ms_substep_deferred_with_clips": med(deferred),
                      "deferred_fused": dst[0], "deferred_literal": dst[1], "deferred_fused_with_clips": dcs[0], "clips_on_their_own": dcs[1],
                      "s_min": float(s0.min()), "s_max": float(s0.max())}))


if __name__ == "__main__":
    main()
