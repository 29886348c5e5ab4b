"""The streaming in-place filter kernels of tlab_amd/csrc/filter_stream.hip behind tlab_opr_filter_fields (OPR_FILTER_FIELDS): every case of both
filter fixtures along x, y and z, several fields a launch, OPR_FILTER with Repeat, the old route as a second yardstick, and the refusals.

Cases and expected values are those of tests/test_gpu_filter_boxes.py: filter_of, fixture_of, G, GB from tests/test_oracle_filter.py, the expected
result oracle.tlab_oracle_filter.opr_filter (pinned to the bit against the reference's filter modules at the line lengths 8, 24, 37, 64, 130), the
fields rng.uniform(-1, 1), 8 NaN guard doubles behind every field, results compared as 64-bit words.

Bound: equality of every word.  The kernels keep k_filter1d's expression trees and its order of operations, and k_filter1d equals the oracle word
for word (test_gpu_filter_boxes.py), so there is nothing to tolerate.

Boxes: x (n, 7, 9) -- 63 lines, one partial workgroup -- and (n, 17, 16) -- 272 lines, five workgroups, the last with 16 lines; y (37, n, 9): odd
nx, a workgroup's 64 lines span two planes; z (13, 21, n): 273 lines.  n = 8 is the shortest legal line: the periodic end points, the near-wall
rows and the interior overlap, and the whole line is less than one tile.  The tile is 32 points along x and 16 along y and z: 8 is below it, 24
between the two, 37 one tile and a part, 64 whole tiles, 130 several and a part.  The one switch of the implementation is the number of fields a
launch takes (8): every case runs 3 fields in one call, test_more_fields_than_a_launch_takes runs 9."""
import numpy as np
import pytest
from test_oracle_filter import G, GB, filter_of, fixture_of                       # noqa: F401  (the cases and their expected values)
from test_gpu_filter_boxes import (BOX, GUARD, KX, KY, KZ, OPR_FILTER_CASES, device_filter, field, oracle_filters, parse, refused, words)

pytestmark = pytest.mark.gpu

BOXES = {
    "x_63": (1, lambda n: (n, 7, 9)),
    "x_272": (1, lambda n: (n, 17, 16)),
    "y_333": (2, lambda n: (37, n, 9)),
    "z_273": (3, lambda n: (13, 21, n)),
}
KEYS = [str(k) for k in G["cases"]] + [str(k) for k in GB["cases"]]


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import tlab_amd as T
    T.init(0)
    return T


def guarded_fields(torch, hosts):
    """every host field on the device with GUARD doubles of NaN behind it: (buffers, the views the filter gets)"""
    bufs = []
    for u in hosts:
        b = torch.full((u.size + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        b[:u.size].copy_(torch.from_numpy(u))
        bufs.append(b)
    return bufs, [b[:u.size] for b, u in zip(bufs, hosts)]


def judge(what, bufs, wants):
    for k, (b, want) in enumerate(zip(bufs, wants)):
        host = b.cpu().numpy()
        got, guard = host[:want.size], host[want.size:]
        assert np.isnan(guard).all(), (what, k, "wrote behind the field")
        bad = int(np.count_nonzero(words(got) != words(want)))
        print("%s field %d: words differing %d / %d" % (what, k, bad, want.size))
        assert bad == 0, (what, "field %d: %d of %d words differ from the oracle" % (k, bad, want.size))


def expected(nx, ny, nz, keys, repeat, u):
    from oracle import tlab_oracle_filter as F
    return F.opr_filter(nx, ny, nz, oracle_filters(keys, repeat), u)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# every case of both fixtures alone, along x (two boxes), y and z, three different fields in one call
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("key", KEYS)
def test_one_filter_on_boxes(T, key, box):
    import torch
    n = parse(key)[0]
    d, shape = BOXES[box]
    nx, ny, nz = shape(n)
    assert (nx, ny, nz)[d - 1] == n
    keys = tuple(key if i == d - 1 else None for i in range(3))
    hosts = [field([n, nx, ny, nz, k], nx * ny * nz) for k in range(3)]
    wants = [expected(nx, ny, nz, keys, None, u) for u in hosts]
    bufs, dev = guarded_fields(torch, hosts)
    T.OPR_FILTER_FIELDS(nx, ny, nz, *(None if k is None else device_filter(T, k) for k in keys), dev)
    judge("%s box %dx%dx%d" % (key, nx, ny, nz), bufs, wants)


def test_more_fields_than_a_launch_takes(T):
    """9 fields: a launch of 8 and a launch of 1 per direction"""
    import torch
    nx, ny, nz = 37, 24, 13
    keys = (KX, KY, None)
    hosts = [field([23, k], nx * ny * nz) for k in range(9)]
    wants = [expected(nx, ny, nz, keys, (1, 2, 1), u) for u in hosts]
    bufs, dev = guarded_fields(torch, hosts)
    T.OPR_FILTER_FIELDS(nx, ny, nz, device_filter(T, KX), device_filter(T, KY), None, dev, (1, 2, 1))
    judge("9 fields", bufs, wants)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# OPR_FILTER: x, y, z with Repeat, against the oracle and against the old route on the device
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(OPR_FILTER_CASES))
def test_opr_filter_fields_vs_oracle_and_old_route(T, case):
    import torch
    keys, repeat = OPR_FILTER_CASES[case]
    nx, ny, nz = BOX
    u = field([11, list(OPR_FILTER_CASES).index(case)], nx * ny * nz)
    want = expected(nx, ny, nz, keys, repeat, u)
    assert np.abs(want - u).max() > 1e-3                             # (the filters do something)
    filters = [None if k is None else device_filter(T, k) for k in keys]
    bufs, dev = guarded_fields(torch, [u])
    T.OPR_FILTER_FIELDS(nx, ny, nz, *filters, dev, repeat)
    judge("%s box %dx%dx%d repeat %s" % (case, nx, ny, nz, repeat), bufs, [want])
    old = torch.from_numpy(u).cuda()
    T.OPR_FILTER(nx, ny, nz, *filters, old, torch.empty_like(old), repeat)
    bad = int(np.count_nonzero(words(bufs[0].cpu().numpy()[:u.size]) != words(old.cpu().numpy())))
    assert bad == 0, (case, "%d words differ from OPR_FILTER's on the device" % bad)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the refusals of test_gpu_filter_boxes.py::test_refusals at the new entry
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(T):
    import torch
    nx, ny, nz = BOX
    fx, fy, fz = (device_filter(T, k) for k in (KX, KY, KZ))
    f64 = device_filter(T, "n64_t1_p0_b11")
    hosts = [field([13, k], nx * ny * nz) for k in range(2)]
    dev = [torch.from_numpy(u).cuda() for u in hosts]

    def untouched():
        return all(np.array_equal(words(d.cpu().numpy()), words(u)) for d, u in zip(dev, hosts))
    refused(T, lambda: T.OPR_FILTER_FIELDS(nx, ny, nz, fx, fy, fz, [dev[0], dev[0]]), "bad arguments")          # one field twice in a launch
    assert untouched()
    refused(T, lambda: T.OPR_FILTER_FIELDS(nx, ny, nz, fx, fy, fz, dev, (1, 0, 1)), "Repeat must be positive")
    assert untouched(), "the fields were filtered along x before the Repeat of y was refused"
    refused(T, lambda: T.OPR_FILTER_FIELDS(nx, ny, nz, fx, fy, fz, dev, (-1, 1, 1)), "Repeat must be positive")
    assert untouched()
    refused(T, lambda: T.OPR_FILTER_FIELDS(nx, ny, nz, fx, f64, fz, dev), "filter size does not match")        # y filter of 64 on ny = 24
    assert untouched(), "the fields were filtered along x before the size of the y filter was refused"
    refused(T, lambda: T.OPR_FILTER_FIELDS(nx, ny, nz, fx, fy, fx, dev, (2, 1, 1)), "filter size does not match")   # z filter of 37 on nz = 130
    assert untouched(), "the fields were filtered along x and y before the size of the z filter was refused"
    refused(T, lambda: T.OPR_FILTER_FIELDS(nx, ny, nz, fy, None, None, dev), "filter size does not match")
    assert untouched()
    # a null field, through the ABI (OPR_FILTER_FIELDS itself refuses what is no tensor)
    from tlab_amd.lib import load, c_vp
    u = (c_vp * 2)(dev[0].data_ptr(), None)
    rc = load().tlab_opr_filter_fields(nx, ny, nz, fx._h, fy._h, fz._h, None, 2, u)
    assert rc != 0 and b"bad arguments" in load().tlab_last_error()
    rc = load().tlab_opr_filter_fields(nx, ny, nz, fx._h, fy._h, fz._h, None, 2, None)
    assert rc != 0
    torch.cuda.synchronize()
    assert untouched()
    # and the handles still work
    T.OPR_FILTER_FIELDS(nx, ny, nz, fx, None, None, dev[:1])
    assert np.array_equal(words(dev[0].cpu().numpy()), words(expected(nx, ny, nz, (KX, None, None), None, hosts[0])))
