"""Cost of the conditional statistics (csrc/conditional.hip) on a box of 512 x 256 x 512 points, fp64, uniform random fields and a gate with the
levels 0 .. 3, in one process: the wall time of a whole call -- kernels, their final kernels, copies and synchronisations -- as the median of 5
after one warm-up (the gate calls only enqueue: they are followed by a device synchronisation here).  Rows: the partition (4 and 127 levels, the
quadrants), tlab_avg_n_xz for several numbers of fields, moments and levels (4 levels a launch), tlab_cavg1v_n of four fields for the bin counts
at which k_cavg_sum has 64, 16, 4 and 1 columns and splits its tables, tlab_pdf1v_n with ibc = 1 beside it (the counts alone), tlab_cavg2v.
The rate is field and gate bytes read per pass / wall time, the min/max pass of a local interval included.
    python tools/conditional_time.py"""
import statistics
import sys
import time

import numpy as np
import torch

import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tlab_amd as T                 # noqa: E402
import tlab_amd.operators as O       # noqa: E402

T.init(0)
nx, ny, nz = 512, 256, 512
n = nx * ny * nz
g = torch.Generator(device="cuda"); g.manual_seed(1)
f = [torch.rand(n, dtype=torch.float64, device="cuda", generator=g) * 2 - 1 for _ in range(5)]
gate = torch.randint(0, 4, (n,), dtype=torch.int8, device="cuda", generator=g)


def timed(what, nbytes, fn):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    t = statistics.median(ts)
    print("%-58s %8.3f ms  %7.1f GB/s of field and gate bytes" % (what, 1e3 * t, nbytes / t / 1e9), flush=True)


print("box %d x %d x %d, %d points" % (nx, ny, nz, n))
out = torch.empty(n, dtype=torch.int8, device="cuda")
timed("gate_levels, 4 levels", 9 * n, lambda: O.gate_levels(f[0], [-0.5, 0.0, 0.5], out))
timed("gate_levels, 127 levels", 9 * n, lambda: O.gate_levels(f[0], list(np.linspace(-1, 1, 126)), out))
timed("gate_flux", 17 * n, lambda: O.gate_flux(f[0], f[1], out))
for nv, nm, np_ in ((4, 4, 0), (4, 4, 3), (4, 10, 3), (4, 4, 8), (1, 4, 127)):
    launches = (max(np_, 1) + 3) // 4
    timed("avg_n_xz nv=%d nm=%d np=%d (%d launches)" % (nv, nm, np_, launches), launches * nv * (8 + (1 if np_ else 0)) * n,
          lambda: O.avg_n_xz(nx, ny, nz, f[:nv], nm, np_, gate if np_ else None))
for nb in (8, 32, 100, 512, 1024):
    timed("cavg1v_n nv=4 nbins=%d local" % nb, (4 * 8 + 4 * 16) * n, lambda: O.cavg1v_n(nx, ny, nz, f[:4], f[4], nb, 1))
timed("cavg1v_n nv=4 nbins=32 external, gated", 4 * 17 * n, lambda: O.cavg1v_n(nx, ny, nz, f[:4], f[4], 32, 0, -1.0, 1.0, gate, 2))
timed("pdf1v_n nv=4 nbins=32 ibc=1 (the counts alone)", (4 * 8 + 4 * 8) * n, lambda: O.pdf1v_n(nx, ny, nz, f[:4], 32, 1))
for nb2 in ((8, 8), (32, 32)):
    timed("cavg2v nbins=%dx%d" % nb2, (8 + 16 + 16 + 24) * n, lambda: O.cavg2v(nx, ny, nz, nb2, f[0], f[1], f[4]))
