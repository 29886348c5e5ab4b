"""What tests/test_gpu_penta_lines.py shares with the child processes it starts, and the child itself.  TEST INFRASTRUCTURE.

TLAB_PENTA_TILE, TLAB_PENTA_TILE_X and TLAB_PENTA_PLX are read once per process (function-local statics of csrc/pentatile.hip), so a form behind
one of them runs in a process started with it in the environment:  python penta_lines_child.py OUT.npz  runs CHILD_CASES through the public C ABI
-- tlab_opr_partial(OPR_P1) and tlab_opr_burgers(U_IN), results between guard zones -- and writes to OUT.npz, per case and operator, the result,
the kernel names launched (tlab_profile_*) and whether the guard zones survived.  The parent compares with the oracle; nothing is judged here."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

PENTA = (5, 7)
NU = (1.0 / 500.0, 1.0 / 350.0, 1.0 / 900.0)
_FIELD, _OPLAN = {}, {}


def field(nx, ny, nz, seed):
    """a smooth product of sines + 0.1 uniform(-1, 1), flat x-fastest, read-only: neighbouring rows and lines differ everywhere"""
    key = (nx, ny, nz, seed)
    if key not in _FIELD:
        rng = np.random.default_rng([nx, ny, nz, seed, 57])
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        u = np.sin(2.0 * np.pi * (1 + seed % 3) * i / nx + 0.3 * seed) * np.cos(0.61 * j + 0.2) * np.sin(2.0 * np.pi * (1 + seed % 2) * k / nz + 0.1 * seed + 0.5)
        u = (u + 0.1 * rng.uniform(-1, 1, u.shape)).ravel()
        u.setflags(write=False)
        _FIELD[key] = u
    return _FIELD[key]


def stretched(n):
    """tanh-stretched nodes on [0, 1], one-sided: x = tanh(2 (1/4 + 3/4 s)), s = i / (n - 1), shifted and scaled to [0, 1].  The spacing falls
    monotonically (by 11 over the line) and nowhere slowly: by 3 tanh(1/2) / (n - 1) = 1.4 / (n - 1) per row and more, 8 % per 32 rows at 512
    points -- a symmetric stretching is flat at its centre, where the table rows of neighbouring chunks would agree to 2e-4."""
    t = np.tanh(2.0 * (0.25 + 0.75 * np.arange(n) / (n - 1)))
    return (t - t[0]) / (t[-1] - t[0])


def oracle_plan(n, kind):
    """the oracle's plan of a line of n points: kind in periodic_tables.KINDS (periodic, scheme (5, 7)) or "stretched" (non-periodic); shared, never modified"""
    import periodic_tables as PT
    from oracle import tlab_oracle as O
    if kind != "stretched":
        return PT.oracle_plan(n, kind, PENTA)
    if n not in _OPLAN:
        _OPLAN[n] = O.FdmPlan(stretched(n), False, False, *PENTA)
    return _OPLAN[n]


def device_plan(T, n, kind):
    import periodic_tables as PT
    return PT.device_plan(T, oracle_plan(n, kind)) if kind != "stretched" else T.FdmPlan(stretched(n), False, False, *PENTA)


def profiled(L, fn):
    """fn() with every launch timed by the library; returns the set of kernel names it launched"""
    import torch
    L.tlab_profile_filter(None); L.tlab_profile_reset(); L.tlab_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.tlab_profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 14)
    L.tlab_profile_report(buf, len(buf))
    L.tlab_profile_reset()
    return {ln.split("\t")[0] for ln in buf.value.decode().split("\n") if ln}


def guard_size(nx, ny):
    return max(2 * nx * ny, 64)                  # two planes, at least one tile of 64 lines; even: 16-byte accesses stay aligned


# (direction, (nx, ny, nz), kind, ibc): `varying` periodic tables and the stretched grid with ibc 0 and 3; 35 x lines = 2 x 16 + 3 = 4 x 8 + 3 =
# 32 + 3, 72 x lines (64 and more: the x lines go through the transposes when the x form is off; 72 = 2 x 32 + 8), 200 z lines = 6 x 32 + 8
CHILD_CASES = [(d, box, kind, ibc)
               for n in (96, 256, 512)
               for d, box in ((1, (n, 5, 7)), (1, (n, 8, 9)), (3, (40, 5, n)))
               for kind, ibc in (("varying", 0), ("stretched", 0), ("stretched", 3))]


def case_key(d, box, kind, ibc):
    return "d%d_%dx%dx%d_%s_%d" % ((d,) + tuple(box) + (kind, ibc))


def run_cases(T, cases=None):
    """{case_key + "_p1" / "_burgers": array, + "_names": "a,b", + "_guards": bool} for every case"""
    import torch
    from guarded import Guarded
    from tlab_amd.lib import load, check, c_vp
    L = load()
    check(L.tlab_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "tlab_set_stream")
    out, plans = {}, {}
    for d, box, kind, ibc in (CHILD_CASES if cases is None else cases):
        nx, ny, nz = box
        n = box[d - 1]
        if (n, kind) not in plans:
            plans[(n, kind)] = device_plan(T, n, kind)
        g = plans[(n, kind)]._h
        u, v = (torch.from_numpy(np.array(field(nx, ny, nz, s))).cuda() for s in (0, 1))
        for op in ("p1", "burgers"):
            res, tmp = (Guarded(nx * ny * nz, guard_size(nx, ny), float("nan")) for _ in range(2))
            if op == "p1":
                call = lambda: check(L.tlab_opr_partial(d, g, T.OPR_P1, nx, ny, nz, ibc, c_vp(u.data_ptr()), res.ptr(), tmp.ptr()), "tlab_opr_partial")      # noqa: E731
            else:
                call = lambda: check(L.tlab_opr_burgers(d, g, T.OPR_B_U_IN, nx, ny, nz, ibc, NU[0], c_vp(u.data_ptr()), c_vp(v.data_ptr()), res.ptr(), tmp.ptr(), 0),      # noqa: E731
                                     "tlab_opr_burgers")
            names = profiled(L, call)
            key = case_key(d, box, kind, ibc) + "_" + op
            out[key] = res.host()
            out[key + "_names"] = ",".join(sorted(names))
            out[key + "_guards"] = bool(res.guards_intact() and tmp.guards_intact())
    return out


if __name__ == "__main__":
    import torch
    import tlab_amd as T
    assert torch.cuda.is_available(), "the child needs the GPU"
    T.init(0)
    np.savez(sys.argv[1], **run_cases(T))
