"""GPU parity tests of the pentadiagonal first derivative (SpaceOrder1 = CompactJacobian6Penta, scheme (5, 7)) line by line: k_pentatile<x> along x,
k_pentatile along y / z (csrc/pentatile.hip) and k_penta1 (csrc/kernels.hip) for every length the tile kernels do not take, through the public C
ABI only -- tlab_fdm_plan_create(_from_arrays), tlab_opr_partial, tlab_opr_burgers, tlab_opr_partial_add, tlab_opr_burgers_add_n -- against the
numpy oracle working from the same arrays.  Tolerance: fp64 relative error <= 1e-12 (BASELINE.json north_star); the oracle's own rounding on these
tables is 4e-16 .. 1.4e-15 (tests/test_periodic_tables_host.py).

What tests/test_gpu_derivs.py::test_penta_first_derivative leaves open, and what is here:
 - periodic lines on tables whose rows DIFFER (tests/periodic_tables.py, `varying`): on a uniform grid a kernel that reads the table rows of
   another chunk of the far interior computes the same numbers (tests/test_periodic_tables_host.py); non-periodic lines on a tanh-stretched grid,
   whose factor rows differ from chunk to chunk (asserted below), with ibc 0 .. 3;
 - every chunk count at both ends and three odd ones: n = 64, 96, 160, 256, 480, 512 -> C = 2, 3, 5, 8, 15, 16 (odd C: workgroups of 96, 160, 480
   threads, no whole number of waves).  A wrong block of the 2 x 2 products one or two chunks away shows at 1e-1 / 1e-8; three chunks away it is
   multiplied by 1e-16 and no fp64 test can see it -- nor does it matter;
 - partial tiles: 15 and 35 x lines (16-line tiles: one short workgroup; 2 x 16 + 3), 200 z lines (6 x 32 + 8), 40 lines per z-plane along y
   (the second tile of every plane is 8 lines short), and whole tiles (96 per plane) beside them;
 - the x form on non-periodic lines, k_penta1 along x (directly: fewer than 64 lines; behind two k_transpose: 64 lines) and at 40, 80, 130 and
   1024 points;
 - every result, tmp1, tmp2 and accumulated tendency between guard zones (two planes, at least one tile of 64 lines); after every call the guards
   are intact, overwritten outputs (NaN before) hold no NaN, every operand equals its snapshot to the bit;
 - the accumulating entry points called directly (they fall back to k_axpy1 / k_add1 around the plain operator on this scheme);
 - the kernel names every call launched (tlab_profile_*), against an expectation written down from the dispatch rules (operators.cpp run_generic,
   pentatile.hip pentatile_ok / pentatile_x_ok), not read off the run;
 - the forms behind TLAB_PENTA_TILE, TLAB_PENTA_TILE_X, TLAB_PENTA_PLX, each in a fresh child process (tests/penta_lines_child.py).

Operands whose base address is 8 but not 16 bytes aligned are NOT covered: the x form reads them as double2."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import rel_err
from guarded import Guarded
import periodic_tables as PT
import penta_lines_child as PC
from penta_lines_child import NU, field, profiled

pytestmark = pytest.mark.gpu
TOL = 1e-12
SCALE = 0.75
TILE_N = (64, 96, 160, 256, 480, 512)            # C = 2, 3, 5, 8, 15, 16
ENDS = (64, 256, 512)                            # where `equal` and `wander` tables run too

PENTA_NAMES = ("k_pentatile<x>", "k_pentatile", "k_penta1", "k_transpose")
OTHER_FAMILIES = ("k_xline", "k_rtile", "k_htile", "k_ptile", "k_zslab")


def _cases():
    c = []
    # x, k_pentatile<x>: 15 lines (one short workgroup), 35 lines (2 x 16 + 3)
    for n in TILE_N:
        for box in ((n, 5, 3), (n, 5, 7)):
            c += [(1, box, k) for k in PT.KINDS if k == "varying" or n in ENDS] + [(1, box, "stretched")]
    # z, k_pentatile: 200 lines = 6 x 32 + 8
    for n in TILE_N:
        c += [(3, (40, 5, n), k) for k in PT.KINDS if k == "varying" or n in ENDS]
        if n in (64, 160, 512):
            c.append((3, (40, 5, n), "stretched"))
    # y, k_pentatile: 40 lines per z-plane (32 + 8, three planes); 96 per plane (whole tiles)
    for n in TILE_N:
        c += [(2, (40, n, 3), "stretched"), (2, (96, n, 2), "stretched")]
    # x, k_penta1: 15 lines directly; 8 x 8 = 64 lines behind two k_transpose
    for box_of in (lambda n: (n, 5, 3), lambda n: (n, 8, 8)):
        c += [(1, box_of(n), "varying") for n in (40, 80, 1024)] + [(1, box_of(80), "stretched")]
    # y / z, k_penta1
    c += [(3, (40, 5, n), "varying") for n in (40, 80)]
    c += [(2, box, "stretched") for n in (40, 80, 130) for box in ((40, n, 3), (96, n, 2))]
    return c


CASES = _cases()


def _id(c):
    return "%s-%dx%dx%d-%s" % (("x", "y", "z")[c[0] - 1], c[1][0], c[1][1], c[1][2], c[2])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# what the dispatch rules say
# ---------------------------------------------------------------------------------------------------------------------------------------------
def first_derivative_kernels(d, box, tile=True, tile_x=True):
    """Kernel names of one pentadiagonal first derivative along d (operators.cpp run_generic).  k_pentatile takes lines of 32 C points, C = 2 .. 16
    (pentatile_ok; TLAB_PENTA_TILE=0: never); along x the form with the LDS tile does (pentatile_x_ok: the same lengths -- its LDS need, (32 C +
    68) x 16 + 64 doubles = 70 KB at 512 points, is below the 160 KB limit at all of them; TLAB_PENTA_TILE_X=0: never), else 64 and more x lines go
    through two transposes around the y / z form or k_penta1, fewer straight to k_penta1 (row stride 1 is not for k_pentatile)."""
    n = box[d - 1]
    lines = box[0] * box[1] * box[2] // n
    chunks_ok = n % 32 == 0 and 2 <= n // 32 <= 16
    if d != 1:
        return {"k_pentatile"} if (chunks_ok and tile) else {"k_penta1"}
    if chunks_ok and tile_x:
        return {"k_pentatile<x>"}
    if lines >= 64:
        return {"k_transpose", "k_pentatile" if (chunks_ok and tile) else "k_penta1"}
    return {"k_penta1"}


def expected_kernels(op, d, box, periodic, **switches):
    """... of a public operator: everything but OPR_P2 on a uniform grid needs the first derivative (a stretched grid: the Jacobian correction of
    the second one, opr_partial.f90:96); the second derivative, the Burgers epilogue, k_axpy1 and k_add1 are of no family named here."""
    return set() if (op == "p2" and periodic) else first_derivative_kernels(d, box, **switches)


def check_names(names, must, tag):
    """the launches include `must`; no pentadiagonal kernel or transpose that `must` does not name, and no tridiagonal fast kernel at all"""
    assert must <= names, (tag, "expected", sorted(must), "launched", sorted(names))
    stray = {k for k in names if (k in PENTA_NAMES and k not in must) or k.startswith(OTHER_FAMILIES)}
    assert not stray, (tag, "expected", sorted(must), "also launched", sorted(stray))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# fixtures, references (made once per key, shared, read-only)
# ---------------------------------------------------------------------------------------------------------------------------------------------
_REF, _DEV, WORST, ROWS = {}, {}, {}, []


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    from tlab_amd.lib import load, check
    T.init(0)
    check(load().tlab_set_stream(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "tlab_set_stream")
    yield T
    _DEV.clear()
    print("\nworst relative error per kernel form:")
    for form, (err, tag) in sorted(WORST.items()):
        print("  %-28s %.3e  (%s)" % (form, err, tag))


def stretched_plan(n):
    """The oracle's plan of the stretched grid; its factor rows differ from chunk to chunk (the Jacobian form scales every row by its spacing):
    in every interior row (8 rows off either wall) some factor differs from the same factor 32 rows further on by more than 1e-3 of itself, for
    every ibc (0.09 .. 0.69 measured: the pivot and the two upper factors carry the spacing; the two multipliers are ratios and barely move)."""
    og = PC.oracle_plan(n, "stretched")
    for ibc in range(4):
        lu = og.der1.lu[8:n - 8, 5 * ibc:5 * ibc + 5]
        if lu.shape[0] > 32:
            diff = (np.abs(lu[32:] - lu[:-32]) / np.abs(lu[:-32])).max(axis=1)
            assert diff.min() > 1e-3, (n, ibc, diff.min())
    return og


def references(d, box, kind, ibc):
    from oracle import tlab_oracle as O
    key = (d, box, kind, ibc)
    if key not in _REF:
        nx, ny, nz = box
        og = stretched_plan(box[d - 1]) if kind == "stretched" else PC.oracle_plan(box[d - 1], kind)
        f = [field(nx, ny, nz, s) for s in range(7)]
        p2, p1 = O.opr_partial(d, O.OPR_P2_P1, nx, ny, nz, ibc, og, f[0])
        r = {"p1": p1, "p2": p2,
             "b_self": O.opr_burgers(d, nx, ny, nz, ibc, og, NU[0], f[0], f[0])[0],
             "p_add": f[4] + O.opr_partial(d, O.OPR_P1, nx, ny, nz, ibc, og, f[0] + SCALE * f[2])[0],
             "b_n": [O.opr_burgers(d, nx, ny, nz, ibc, og, NU[i], f[i], f[1])[0] for i in range(3)]}
        r["b_uin"] = r["b_n"][0]                 # field 0 advected by field 1 with NU[0]
        for a in [r["p1"], r["p2"], r["b_self"], r["p_add"]] + r["b_n"]:
            a.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def device_plan(T, n, kind):
    if (n, kind) not in _DEV:
        _DEV[(n, kind)] = PC.device_plan(T, n, kind)
    return _DEV[(n, kind)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# one case: every operator, guarded
# ---------------------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, T, d, box, kind):
        import torch
        from tlab_amd.lib import load
        nx, ny, nz = box
        self.T, self.L, self.d, self.box, self.kind = T, load(), d, box, kind
        self.n, self.N = box[d - 1], nx * ny * nz
        self.periodic = kind != "stretched"
        self.guard = PC.guard_size(nx, ny)
        self.g = device_plan(T, self.n, kind)
        self.f = [field(nx, ny, nz, s) for s in range(7)]
        self.dev = [torch.from_numpy(np.array(a)).cuda() for a in self.f]
        self.snap = [t.clone() for t in self.dev]
        self.where = "%s %dx%dx%d" % (("x", "y", "z")[d - 1], nx, ny, nz)

    def new(self, fill):
        return Guarded(self.N, self.guard, fill)

    def call(self, tag, op, fn, arrays, written):
        """fn() -> return code; then: guards of all `arrays` intact, `written` without NaN, operands untouched, kernel names as the dispatch rules say"""
        import torch
        from tlab_amd.lib import check
        names = profiled(self.L, lambda: check(fn(), tag))
        for k, a in enumerate(arrays):
            assert a.guards_intact(), (self.where, tag, "guard zone of array %d written" % k)
        for k, a in enumerate(written):
            assert not np.isnan(a.host()).any(), (self.where, tag, "output %d left unwritten in places" % k)
        for k, (t, s) in enumerate(zip(self.dev, self.snap)):
            assert torch.equal(t, s), (self.where, tag, "operand %d modified" % k)
        assert self.L.tlab_last_kernel_path() == 1, (self.where, tag, "kernel path", self.L.tlab_last_kernel_path())
        check_names(names, expected_kernels(op, self.d, self.box, self.periodic), (self.where, tag))
        return sorted(k for k in names if k in PENTA_NAMES)

    def close_to(self, tag, names, got, ref):
        err = rel_err(got.host(), ref)
        form = "+".join(names) if names else "(none)"
        row = "%-14s %-14s %-44s %-26s %.3e" % (self.where, tag[0], tag[1], form, err)
        print(row)
        ROWS.append(row)
        if err > WORST.get(form, (-1.0, ""))[0]:
            WORST[form] = (err, "%s %s %s" % (self.where, tag[0], tag[1]))
        assert err <= TOL, (self.where, tag, err)

    def run(self, ibc):
        L, d, g = self.L, self.d, self.g._h
        nx, ny, nz = self.box
        from tlab_amd.lib import c_vp
        ref = references(d, self.box, self.kind, ibc)
        lab = self.kind if self.periodic else "ibc %d" % ibc
        nan = float("nan")
        p = lambda t: c_vp(t.data_ptr())       # noqa: E731
        u, v, ub = self.dev[0], self.dev[1], self.dev[2]
        for typ, op, key in ((1, "p1", "p1"), (2, "p2", "p2"), (3, "p2_p1", "p2")):
            res, tmp = self.new(nan), self.new(nan)
            what = "tlab_opr_partial OPR_%s" % op.upper()
            names = self.call(what, op, lambda: L.tlab_opr_partial(d, g, typ, nx, ny, nz, ibc, p(u), res.ptr(), tmp.ptr()), [res, tmp], [res, tmp] if typ == 3 else [res])
            self.close_to((lab, what), names, res, ref[key])
            if typ == 3:
                self.close_to((lab, what + " tmp1"), names, tmp, ref["p1"])
        for ivel, vel, key in ((self.T.OPR_B_U_IN, v, "b_uin"), (self.T.OPR_B_SELF, u, "b_self")):
            res, tmp = self.new(nan), self.new(nan)
            what = "tlab_opr_burgers " + ("U_IN" if key == "b_uin" else "SELF")
            names = self.call(what, "burgers", lambda: L.tlab_opr_burgers(d, g, ivel, nx, ny, nz, ibc, NU[0], p(u), p(vel), res.ptr(), tmp.ptr(), 0), [res, tmp], [res])
            self.close_to((lab, what), names, res, ref[key])
        # result += d (u + SCALE ub)
        res, t1, t2 = self.new(self.f[4]), self.new(nan), self.new(nan)
        names = self.call("tlab_opr_partial_add", "p_add", lambda: L.tlab_opr_partial_add(d, g, nx, ny, nz, ibc, p(u), p(ub), SCALE, res.ptr(), 1, t1.ptr(), t2.ptr()),
                          [res, t1, t2], [res])
        self.close_to((lab, "tlab_opr_partial_add"), names, res, ref["p_add"])
        # three fields advected by the second of them: accumulating, then overwriting NaN
        nu = (ctypes.c_double * 3)(*NU)
        sp = (c_vp * 3)(*[self.dev[i].data_ptr() for i in range(3)])
        for overwrite in (0, 1):
            out = [self.new(nan if overwrite else self.f[4 + i]) for i in range(3)]
            t1, t2 = self.new(nan), self.new(nan)
            hp = (c_vp * 3)(*[o.ptr().value for o in out])
            what = "tlab_opr_burgers_add_n overwrite=%d" % overwrite
            names = self.call(what, "b_n", lambda: L.tlab_opr_burgers_add_n(d, g, nx, ny, nz, ibc, 3, nu, sp, p(v), hp, t1.ptr(), t2.ptr(), overwrite), out + [t1, t2], out)
            for i in range(3):
                self.close_to((lab, "%s field %d" % (what, i)), names, out[i], ref["b_n"][i] if overwrite else self.f[4 + i] + ref["b_n"][i])


@pytest.mark.parametrize("d,box,kind", CASES, ids=[_id(c) for c in CASES])
def test_penta_lines(T, d, box, kind):
    """One box: every operator; a stretched (non-periodic) grid with ibc 0 .. 3.  Rows printed: direction and box, kind or ibc, operator, the
    pentadiagonal kernels and transposes launched, relative error."""
    c = Case(T, d, box, kind)
    for ibc in ((0,) if c.periodic else (0, 1, 2, 3)):
        c.run(ibc)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the forms behind switches that are read once per process
# ---------------------------------------------------------------------------------------------------------------------------------------------
SWITCHES = [{"TLAB_PENTA_TILE_X": "0"},                                  # x lines: two transposes around k_pentatile (64 lines and more), else k_penta1
            {"TLAB_PENTA_TILE": "0", "TLAB_PENTA_TILE_X": "0"},          # everything on k_penta1
            {"TLAB_PENTA_PLX": "8"},                                     # 8 x lines per workgroup
            {"TLAB_PENTA_PLX": "32"}]                                    # 32 up to 256 points; 512 points stay on 16
_DEFAULT = {}


@pytest.mark.parametrize("env", SWITCHES, ids=["+".join("%s=%s" % kv for kv in sorted(e.items())) for e in SWITCHES])
def test_forms_behind_process_wide_switches(T, env, tmp_path):
    """A fresh child process per setting (tests/penta_lines_child.py: `varying` periodic tables and the stretched grid with ibc 0 and 3; 96, 256,
    512 points; 35 and 72 x lines, 200 z lines; OPR_P1 and Burgers U_IN); this process compares with the oracle at 1e-12 and asserts the kernel
    names the child reports against the dispatch rules under that setting.  TLAB_PENTA_PLX changes the tile of k_pentatile<x>, not its name; with
    32, lines of 512 points keep the 16-line tile and must be right all the same.  Printed, not asserted: how many words differ from what the
    default form computes in this process."""
    from oracle import tlab_oracle as O
    for k in ("TLAB_PENTA_TILE", "TLAB_PENTA_TILE_X", "TLAB_PENTA_PLX"):
        assert k not in os.environ, "the parent process must run the default forms"
    if not _DEFAULT:
        _DEFAULT.update(PC.run_cases(T))
    out = str(tmp_path / "child.npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(PC.HERE, "penta_lines_child.py"), out]
    r = subprocess.run(cmd, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (env, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got = np.load(out)
    tile, tile_x = env.get("TLAB_PENTA_TILE") != "0", env.get("TLAB_PENTA_TILE_X") != "0"
    label = " ".join("%s=%s" % kv for kv in sorted(env.items()))
    for d, box, kind, ibc in PC.CHILD_CASES:
        nx, ny, nz = box
        og = stretched_plan(box[d - 1]) if kind == "stretched" else PC.oracle_plan(box[d - 1], kind)
        refs = {"p1": lambda: O.opr_partial(d, O.OPR_P1, nx, ny, nz, ibc, og, field(nx, ny, nz, 0))[0],
                "burgers": lambda: O.opr_burgers(d, nx, ny, nz, ibc, og, NU[0], field(nx, ny, nz, 0), field(nx, ny, nz, 1))[0]}
        for op in ("p1", "burgers"):
            key = PC.case_key(d, box, kind, ibc) + "_" + op
            if key not in _REF:
                _REF[key] = refs[op]()
            names = set(str(got[key + "_names"]).split(","))
            where = "%s %dx%dx%d" % (("x", "y", "z")[d - 1], nx, ny, nz)
            tag = (label, where, kind, ibc, op)
            assert bool(got[key + "_guards"]), (tag, "guard zone written")
            check_names(names, expected_kernels(op, d, box, kind != "stretched", tile=tile, tile_x=tile_x), tag)
            err, err0 = rel_err(got[key], _REF[key]), rel_err(_DEFAULT[key], _REF[key])
            words = int(np.count_nonzero(got[key].view(np.int64) != _DEFAULT[key].view(np.int64)))
            form = "+".join(sorted(k for k in names if k in PENTA_NAMES))
            row = "%-14s %-14s %-44s %-26s %.3e  (default form %.3e; %d of %d words differ)" % (
                where, kind if kind != "stretched" else "ibc %d" % ibc, "%s [%s]" % (op, label), form, err, err0, words, got[key].size)
            print(row)
            ROWS.append(row)
            wkey = "%s [%s]" % (form, label)
            if err > WORST.get(wkey, (-1.0, ""))[0]:
                WORST[wkey] = (err, "%s %s %s" % (where, kind, op))
            assert err <= TOL, (tag, err)
            assert err0 <= TOL, (tag, "default form", err0)
