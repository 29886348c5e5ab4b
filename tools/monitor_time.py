"""Cost of the per-iteration monitors on the device (TIME_COURANT, DNS_BOUNDS_CONTROL's dilatation check): at n^3 on one GPU,
  - the Courant pass (k_courant_partial through a one-rank pencil driver: the kernel alone by the library's event timing, and the whole call with its
    final pass, copy and synchronisation) next to the single-domain tlab_time_courant of before;
  - the dilatation monitor: tlab_dns_dilatation_extremes (three accumulated P1 derivatives + one reduction with the locations) against the 7-launch
    FI_INVARIANT_P + MINMAX path of Dns.dilatation_bounds, interleaved;
  - both on loopback npro_i x npro_k pencils (every rank on this GPU).
Each entry is the median wall time of whole calls (each ends in a synchronisation of the stream).
    python tools/monitor_time.py [--n 512] [--reps 20] [--pencils 2x4]       (prints one JSON line)"""
import argparse
import ctypes
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms))


def kernel_ms(L, tag, fn, reps):
    """mean duration of the launches named tag inside fn, by the library's own event timing"""
    from tlab_amd.lib import check
    check(L.tlab_profile_filter(tag.encode()), "filter")
    check(L.tlab_profile_enable(1), "profile")
    check(L.tlab_profile_reset(), "reset")
    try:
        for _ in range(reps):
            fn()
        buf = ctypes.create_string_buffer(1 << 14)
        if L.tlab_profile_report(buf, len(buf)) < 0:
            return None
    finally:
        check(L.tlab_profile_enable(0), "profile off")
        check(L.tlab_profile_filter(b""), "filter")
    for line in buf.value.decode().splitlines():
        f = line.split("\t")
        if f[0] == tag:
            return float(f[2]) / int(f[1])
    return None


def fill(tensors, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    for t in tensors:
        t.copy_((2 * torch.rand(t.numel(), dtype=torch.float64, device="cuda", generator=g) - 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pencils", default="2x4")
    a = ap.parse_args()
    import tlab_amd as T
    from tlab_amd.dns import Dns
    from tlab_amd.pencil import NativePencilDns
    from tlab_amd.lib import load
    T.init(0)
    L = load()
    n = a.n
    x = np.arange(n) / n * 2 * np.pi
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(n) / (n - 1) - 1)) / np.tanh(1.5))
    kw = dict(nscal=1, visc=1.0 / 5000.0, schmidt=(1.0,), yuniform=False)
    out = {"n": n, "reps": a.reps, "field_GB": n ** 3 * 8 / 1e9}

    d = Dns(x, y, x.copy(), **kw)
    fill(d.q, 1)
    out["ms_courant_single_before"] = timed(lambda: d.TIME_COURANT(1.0, 0.2), a.reps)
    out["ms_dilatation_7_launch"], out["ms_dilatation_new"] = [], []
    for _ in range(3):            # interleaved rounds
        out["ms_dilatation_7_launch"].append(timed(d.dilatation_bounds, a.reps))
        out["ms_dilatation_new"].append(timed(lambda: d.dilatation_extremes(), a.reps))
    out["ms_dilatation_7_launch"] = float(np.median(out["ms_dilatation_7_launch"]))
    out["ms_dilatation_new"] = float(np.median(out["ms_dilatation_new"]))
    out["ms_kernel_extremes_partial"] = kernel_ms(L, "k_extremes_partial", lambda: d.dilatation_extremes(), a.reps)
    del d
    gc.collect()
    torch.cuda.empty_cache()

    p = NativePencilDns("loopback", 1, 1, x, y, x.copy(), **kw)
    fill(p.st[0]["q"], 1)
    out["ms_courant_call"] = timed(lambda: p.TIME_COURANT(1.0, 0.2), a.reps)
    kms = kernel_ms(L, "k_courant_partial", lambda: p.TIME_COURANT(1.0, 0.2), a.reps)
    out["ms_kernel_courant_partial"] = kms
    out["courant_TBps"] = 3 * n ** 3 * 8 / (kms * 1e-3) / 1e12 if kms else None
    p.close()
    del p
    gc.collect()
    torch.cuda.empty_cache()

    npi, npk = (int(v) for v in a.pencils.split("x"))
    p = NativePencilDns("loopback", npi, npk, x, y, x.copy(), **kw)
    for r in p.local_ranks:
        fill(p.st[r]["q"], 10 + r)
    out["pencils"] = a.pencils
    out["ms_pencil_courant"] = timed(lambda: p.TIME_COURANT(1.0, 0.2), a.reps)
    out["ms_pencil_dilatation"] = timed(p.dilatation_bounds, a.reps)
    out["ms_pencil_dilatation_extremes"] = timed(lambda: p.dilatation_extremes(), a.reps)
    p.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
