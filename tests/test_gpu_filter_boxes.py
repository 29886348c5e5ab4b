"""The 1-D filters of tlab_amd/csrc/filter.hip on whole boxes: every route of tlab_opr_filter_1d (x strided below 64 lines, x through the two
transposes and the scratch f->ws from 64 lines on, y with several planes, z), OPR_FILTER (tlab_opr_filter: x, y, z in that order, Repeat, in place
through tmp) and the dealiasing branch of OPR_Burgers off the cube.

The expected value is the numpy oracle (oracle/tlab_oracle_filter.py), which tests/test_oracle_filter.py pins to the bit against the reference's
own filter modules at every line length used here: 24, 64 (tests/golden/filters.npz) and 8, 37, 130 (filter_boxes.npz).  The fields are
rng.uniform(-1, 1), so no two lines are equal and no two extents of a box are: an exchange of n and nlines, of a stride or of a line index
cannot cancel.  Results are written into NaN with 8 guard doubles behind them; the operands are compared as 64-bit words afterwards.

Bound: bit equality.  The kernel repeats the reference's operations in the reference's order with FP contraction off, and on the MI355X not one
64-bit word of any result here differs from the oracle's (profiles/r20/filter_boxes.txt: counts and relative errors per route and filter type,
OPR_FILTER_1D and OPR_FILTER), so the project's bound for this operator, rel_err <= 1e-14, was tightened to equality of the words.  Run with -s
for the per-call figures and the summary the record was made from."""
import re
import numpy as np
import pytest
from conftest import rel_err
from test_oracle_filter import G, GB, filter_of, fixture_of

pytestmark = pytest.mark.gpu
REF_HYPER = 0.1
TOL = 1e-14           # the project's bound for this operator (tests/test_gpu_filter.py); asserted first, for the message of a gross failure
GUARD = 8
TYPE_NAME = {1: "compact", 2: "explicit6", 3: "explicit4", 9: "compactcutoff"}

# route -> (dir, box at line length n)
ROUTES = {
    "x_strided_63": (1, lambda n: (n, 7, 9)),             # 63 lines: the last shape below the switch to the transposed route
    "x_transposed_72": (1, lambda n: (n, 9, 8)),          # 72 lines: nlines != n, partial workgroup
    "x_transposed_272": (1, lambda n: (n, 17, 16)),       # 272 lines: two workgroups, the second almost empty
    "y_333": (2, lambda n: (37, n, 9)),                   # odd nx, nine planes (outer_stride), 333 lines: two workgroups
    "z_273": (3, lambda n: (13, 21, n)),                  # lines_inner = nx * ny = 273: two workgroups
}
KEYS = [str(k) for k in G["cases"]] + [str(k) for k in GB["cases"]]
STATS = {}            # (operator, route, filter type) -> [calls, differing words, words, worst rel_err]


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    yield T
    if STATS:
        print("\nsummary: operator, route, filter type, calls, differing 64-bit words / words compared, worst rel_err")
        for (op, route, t), (calls, bad, words, worst) in sorted(STATS.items()):
            print("SUMMARY %-14s %-22s %-14s calls %3d   words differing %d / %d   worst rel_err %.3e" % (op, route, t, calls, bad, words, worst))


def parse(key):
    return tuple(int(v) for v in re.match(r"n(\d+)_t(\d+)_p(\d)_b(\d)(\d)", key).groups())


_DEV = {}


def device_filter(T, key):
    """one device Filter per case for the whole module: the x routes of a case share its scratch, which grows from box to box"""
    if key not in _DEV:
        n, t, per, b0, b1 = parse(key)
        c = fixture_of(key)[key + "_coeffs"]
        _DEV[key] = T.Filter(t, n, bool(per), c if c.shape[1] else None, b0, b1)
    return _DEV[key]


def words(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def field(seed, n):
    return np.random.default_rng(seed).uniform(-1, 1, n)


def expected_1d(key, d, nx, ny, nz, u):
    from oracle import tlab_oracle as O
    from oracle import tlab_oracle_filter as F
    return O._from_lines(F.opr_filter_1d(filter_of(key)[0], O._to_lines(u, nx, ny, nz, d)), nx, ny, nz, d)


def guarded_result(torch, n):
    """n doubles of NaN to be written and GUARD more behind them that must stay NaN"""
    buf = torch.full((n + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    return buf, buf[:n]


def judge(op, route, ftype, what, buf, want, operands=()):
    """buf: result + guards (device).  operands: (device tensor, host array) pairs that the call must not have changed."""
    n = want.size
    host = buf.cpu().numpy()
    got, guard = host[:n], host[n:]
    assert np.isnan(guard).all(), (what, "wrote behind the result")
    assert not np.isnan(got).any(), (what, "%d points left unwritten" % int(np.isnan(got).sum()))
    for dev, orig in operands:
        assert np.array_equal(words(dev.cpu().numpy()), words(orig)), (what, "an operand was changed")
    err = rel_err(got, want)
    bad = int(np.count_nonzero(words(got) != words(want)))
    print("%s %s %s: words differing %d / %d, rel_err %.3e" % (op, route, what, bad, n, err))
    s = STATS.setdefault((op, route, TYPE_NAME.get(ftype, str(ftype))), [0, 0, 0, 0.0])
    s[0] += 1; s[1] += bad; s[2] += n; s[3] = max(s[3], err)
    assert err <= TOL, (what, err)
    assert bad == 0, (what, "%d of %d words differ from the oracle" % (bad, n), err)
    return got


# ---------------------------------------------------------------------------------------------------------------------------------------------
# OPR_FILTER_1D, every case of both fixtures on every route
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("key", KEYS)
def test_filter_1d_on_boxes(T, key, route):
    import torch
    n, t = parse(key)[:2]
    d, box = ROUTES[route]
    nx, ny, nz = box(n)
    assert (nx, ny, nz)[d - 1] == n
    u = field([n, nx, ny, nz], nx * ny * nz)
    du = torch.from_numpy(u).cuda()
    buf, res = guarded_result(torch, u.size)
    T.OPR_FILTER_1D(d, device_filter(T, key), nx, ny, nz, du, res)
    judge("OPR_FILTER_1D", route, t, "%s box %dx%dx%d" % (key, nx, ny, nz), buf, expected_1d(key, d, nx, ny, nz, u), [(du, u)])


def test_one_handle_serves_boxes_of_different_sizes(T):
    """the scratch f->ws of the transposed x route grows with the second box and is larger than needed for the third"""
    import torch
    key = "n37_t1_p1_b00"
    n, t, per = parse(key)[:3]
    c = GB[key + "_coeffs"]
    f = T.Filter(t, n, bool(per), c)           # a handle of its own: its scratch starts empty
    boxes = [(37, 9, 8), (37, 17, 16), (37, 9, 8)]
    ins = [field([5, 1], 37 * 72), field([5, 2], 37 * 272), field([5, 3], 37 * 72)]
    got = []
    for (nx, ny, nz), u in zip(boxes, ins):
        du = torch.from_numpy(u).cuda()
        buf, res = guarded_result(torch, u.size)
        T.OPR_FILTER_1D(1, f, nx, ny, nz, du, res)
        got.append(judge("OPR_FILTER_1D", "x_one_handle", t, "%s box %dx%dx%d" % (key, nx, ny, nz), buf, expected_1d(key, 1, nx, ny, nz, u), [(du, u)]))
    du = torch.from_numpy(ins[0]).cuda()       # the first input again, after the scratch has grown
    buf, res = guarded_result(torch, ins[0].size)
    T.OPR_FILTER_1D(1, f, 37, 9, 8, du, res)
    again = judge("OPR_FILTER_1D", "x_one_handle", t, key + " first input again", buf, expected_1d(key, 1, 37, 9, 8, ins[0]), [(du, ins[0])])
    assert np.array_equal(words(again), words(got[0])), "the same input gives another result once the scratch is larger than the box"


# ---------------------------------------------------------------------------------------------------------------------------------------------
# OPR_FILTER through the ABI
# ---------------------------------------------------------------------------------------------------------------------------------------------
BOX = (37, 24, 130)                                               # all three extents differ, every direction has more than 64 lines
KX, KY, KZ, KY66 = "n37_t9_p1_b00", "n24_t1_p0_b11", "n130_t3_p1_b00", "n24_t1_p0_b66"
OPR_FILTER_CASES = {
    "xyz_repeat_213": ((KX, KY, KZ), (2, 1, 3)),
    "x_alone": ((KX, None, None), (1, 1, 1)),
    "y_alone": ((None, KY, None), (1, 1, 1)),
    "z_alone": ((None, None, KZ), (1, 1, 1)),
    "xyz_repeat_none": ((KX, KY, KZ), None),
    "y_b66_repeat_121": ((None, KY66, None), (1, 2, 1)),          # the pressure filter's form
}


def oracle_filters(keys, repeat):
    out = []
    for d, k in enumerate(keys):
        f = None if k is None else filter_of(k)[0]
        if f is not None and repeat is not None:
            f.repeat = repeat[d]
        out.append(f)
    return out


@pytest.mark.parametrize("case", list(OPR_FILTER_CASES))
def test_opr_filter_vs_oracle(T, case):
    import torch
    from oracle import tlab_oracle_filter as F
    keys, repeat = OPR_FILTER_CASES[case]
    nx, ny, nz = BOX
    u = field([11, list(OPR_FILTER_CASES).index(case)], nx * ny * nz)
    want = F.opr_filter(nx, ny, nz, oracle_filters(keys, repeat), u)
    assert rel_err(want, u) > 1e-3                                  # (the filters do something)
    buf, du = guarded_result(torch, u.size)
    du.copy_(torch.from_numpy(u))
    tbuf, tmp = guarded_result(torch, u.size)
    T.OPR_FILTER(nx, ny, nz, *(None if k is None else device_filter(T, k) for k in keys), du, tmp, repeat)
    types = "+".join(TYPE_NAME[parse(k)[1]] for k in keys if k is not None)
    judge("OPR_FILTER", case, types, "box %dx%dx%d repeat %s" % (nx, ny, nz, repeat), buf, want)
    assert np.isnan(tbuf.cpu().numpy()[u.size:]).all(), "wrote behind tmp"


def refused(T, call, text):
    """the call returns non-zero and leaves an error string that says why"""
    with pytest.raises(T.TlabError) as e:
        call()
    m = re.search(r"failed \((-?\d+)\): (.*)", str(e.value), re.S)
    assert m and int(m.group(1)) != 0 and text in m.group(2), str(e.value)


def test_refusals(T):
    import torch
    nx, ny, nz = BOX
    fx, fy, fz = (device_filter(T, k) for k in (KX, KY, KZ))
    f64 = device_filter(T, "n64_t1_p0_b11")
    u = field([13], nx * ny * nz)
    du = torch.from_numpy(u).cuda()
    tmp = torch.full_like(du, float("nan"))

    def untouched():
        return np.array_equal(words(du.cpu().numpy()), words(u))
    refused(T, lambda: T.OPR_FILTER(nx, ny, nz, fx, fy, fz, du, du), "bad arguments")                       # u == tmp
    assert untouched()
    refused(T, lambda: T.OPR_FILTER(nx, ny, nz, fx, fy, fz, du, tmp, (1, 0, 1)), "Repeat must be positive")
    assert untouched(), "u was filtered along x before the Repeat of y was refused"
    refused(T, lambda: T.OPR_FILTER(nx, ny, nz, fx, fy, fz, du, tmp, (-1, 1, 1)), "Repeat must be positive")
    assert untouched()
    refused(T, lambda: T.OPR_FILTER(nx, ny, nz, fx, f64, fz, du, tmp), "filter size does not match")        # y filter of 64 on ny = 24
    assert untouched(), "u was filtered along x before the size of the y filter was refused"
    refused(T, lambda: T.OPR_FILTER(nx, ny, nz, fx, fy, fx, du, tmp, (2, 1, 1)), "filter size does not match")   # z filter of 37 on nz = 130
    assert untouched(), "u was filtered along x and y before the size of the z filter was refused"
    refused(T, lambda: T.OPR_FILTER(nx, ny, nz, fy, None, None, du, tmp), "filter size does not match")
    assert untouched()
    res = torch.full_like(du, float("nan"))
    refused(T, lambda: T.OPR_FILTER_1D(1, fx, nx, ny, nz, du, du), "out of place")                          # in place
    for d in (0, 4, -1):
        refused(T, lambda: T.OPR_FILTER_1D(d, fx, nx, ny, nz, du, res), "bad sizes")
    refused(T, lambda: T.OPR_FILTER_1D(2, fx, nx, ny, nz, du, res), "filter size does not match")
    assert untouched() and bool(torch.isnan(res).all())
    # and the handles still work
    T.OPR_FILTER_1D(1, fx, nx, ny, nz, du, res)
    assert np.array_equal(words(res.cpu().numpy()), words(expected_1d(KX, 1, nx, ny, nz, u)))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# [Dealiasing] in OPR_Burgers off the cube
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_dealiased_burgers_off_the_cube(T):
    """the operator-level half of test_gpu_filter.py::test_dealiased_burgers_and_substep_vs_oracle on 37 x 24 x 130: filter(u) and filter(ds/dx)
    of opr_burgers.f90:478-500 on lines of three different lengths, none of them the number of lines"""
    import torch
    from oracle import tlab_oracle as O
    nx, ny, nz = BOX
    x, z = np.arange(nx) / nx * 2.0, np.arange(nz) / nz * 2.0
    y = 0.5 * (1 + np.tanh(1.5 * (2 * np.arange(ny) / (ny - 1) - 1)) / np.tanh(1.5))
    assert np.array_equal(x, GB["n37_x"]) and np.array_equal(y, G["n24_y"]) and np.array_equal(z, GB["n130_x"])    # the tables belong to these nodes
    keys = {1: KX, 2: KY, 3: KZ}
    dev = {d: device_filter(T, k) for d, k in keys.items()}
    orc = {d: filter_of(k)[0] for d, k in keys.items()}
    s0, v0 = field([17, 1], nx * ny * nz), field([17, 2], nx * ny * nz)
    visc = 1.0 / 500.0
    try:
        for d in (1, 2, 3):
            T.set_dealiasing(d, dev[d])
        s_, v_ = torch.from_numpy(s0).cuda(), torch.from_numpy(v0).cuda()
        tmp = torch.empty_like(s_)
        for d, (nodes, per) in {1: (x, True), 2: (y, False), 3: (z, True)}.items():
            gp, go = T.FdmPlan(nodes, per, per, hyper_bc1_ext=REF_HYPER), O.FdmPlan(nodes, per, per)
            buf, res = guarded_result(torch, s0.size)
            (T.OPR_Burgers_X, T.OPR_Burgers_Y, T.OPR_Burgers_Z)[d - 1](T.OPR_B_U_IN, visc, nx, ny, nz, 0, gp, s_, v_, res, tmp)
            ref = O.opr_burgers(d, nx, ny, nz, 0, go, visc, s0, v0, dealiasing=orc[d])[0]
            plain = O.opr_burgers(d, nx, ny, nz, 0, go, visc, s0, v0)[0]
            host = buf.cpu().numpy()
            assert np.isnan(host[s0.size:]).all() and not np.isnan(host[:s0.size]).any(), d
            e = rel_err(host[:s0.size], ref)
            print("dealiased OPR_Burgers dir %d on %dx%dx%d: rel_err %.3e, against the plain operator %.3e" % (d, nx, ny, nz, e, rel_err(host[:s0.size], plain)))
            assert e <= 1e-12, (d, e)
            assert rel_err(ref, plain) > 1e-6 and rel_err(host[:s0.size], plain) > 1e-6, d                     # (the filters do something)
            assert np.array_equal(words(s_.cpu().numpy()), words(s0)) and np.array_equal(words(v_.cpu().numpy()), words(v0)), d
    finally:
        for d in (1, 2, 3):
            T.set_dealiasing(d, None)
