"""The cases of the sampling entry points that run on host arrays (tests/test_sampling_host.py) and on device arrays (tests/test_gpu_sampling.py)
alike: `put` makes an array of the kind under test from a numpy array, `get` brings one back.  Every comparison is against tests/sampling_oracle.py."""
import ctypes

import numpy as np

import sampling_oracle as S

PHASE_BOXES = [(20, 12, 8), (7, 5, 3), (6, 4, 1), (130, 6, 19)]      # (130, 6, 19): several workgroups, a k-unroll with a remainder
TOWER_CASES = [((16, 12, 8), (4, 1, 2)), ((7, 5, 3), (1, 1, 1))]
EINVAL = -1
vp = ctypes.c_void_p


def fields(shape, n, seed):
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.uniform(-1, 1, (nz, ny, nx)) + 0.3 * (i + 1)) for i in range(n)]


def dyadic_fields(shape, n, seed):
    """integers times 2^-10: every partial sum of a plane is exact, whatever its order"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.integers(-1000, 1000, (nz, ny, nx)) * 2.0 ** -10) for _ in range(n)]


def check_phase(T, shape, put, get):
    """means, fused flow and stresses, bitwise: nz_total = nz and 2 nz, avg_planes 1 and 3, every plane_id in turn, so that the running mean
    accumulates over (up to) three successive planes"""
    nx, ny, nz = shape
    for nz_total in (nz, 2 * nz):
        for avg_planes in (1, 3):
            ref_s, ref_f, ref_t = (np.zeros((n, avg_planes + 1, ny, nx)) for n in (4, 3, 6))
            got_s, got_f, got_t, got_f1 = put(ref_s), put(ref_f), put(ref_t), put(ref_f)
            for plane_id in range(1, avg_planes + 1):
                h = fields(shape, 4, 10 * plane_id + avg_planes)
                d = [put(a) for a in h]
                S.avg_phase_space(h, nz_total, avg_planes, plane_id, ref_s)          # four fields: two launches on the device
                S.avg_phase_space(h[:3], nz_total, avg_planes, plane_id, ref_f)
                S.avg_phase_stress(h[0], h[1], h[2], nz_total, avg_planes, plane_id, ref_t)
                T.avg_phase_space(nx, ny, nz, d, avg_planes, plane_id, got_s, nz_total=nz_total)
                T.avg_phase_space(nx, ny, nz, d[:3], avg_planes, plane_id, got_f1, nz_total=nz_total)
                T.avg_phase_flow(nx, ny, nz, d[0], d[1], d[2], avg_planes, plane_id, got_f, got_t, nz_total=nz_total)
                what = (shape, nz_total, avg_planes, plane_id)
                assert np.array_equal(get(got_s), ref_s), ("space", what)
                assert np.array_equal(get(got_f1), ref_f), ("space, three fields", what)
                assert np.array_equal(get(got_f), ref_f), ("flow", what)
                assert np.array_equal(get(got_t), ref_t), ("stress", what)
            # the ids: uv is plane 2 of the stresses (not the comment's order), vw plane 5
            uv = np.zeros((1, avg_planes + 1, ny, nx))
            S.avg_phase_space([h[0] * h[1]], nz_total, avg_planes, avg_planes, uv)
            assert np.array_equal(get(got_t)[1, avg_planes - 1], uv[0, avg_planes - 1])
            vw = np.zeros((1, avg_planes + 1, ny, nx))
            S.avg_phase_space([h[1] * h[2]], nz_total, avg_planes, avg_planes, vw)
            assert np.array_equal(get(got_t)[4, avg_planes - 1], vw[0, avg_planes - 1])


def check_phase_refusals(L, put, get, ptr):
    nx, ny, nz = 6, 4, 3
    a = put(fields((nx, ny, nz), 1, 1)[0])
    one = (vp * 1)(ptr(a))
    for avg_planes, plane_id in ((0, 1), (3, 0), (3, 4)):
        avg = put(np.full((9, max(avg_planes, 1) + 1, ny, nx), -7.0))
        assert L.tlab_avg_phase_space(nx, ny, nz, nz, 1, one, avg_planes, plane_id, vp(ptr(avg))) == EINVAL, (avg_planes, plane_id)
        assert b"tlab_avg_phase_space" in L.tlab_last_error()
        assert L.tlab_avg_phase_flow(nx, ny, nz, nz, vp(ptr(a)), vp(ptr(a)), vp(ptr(a)), avg_planes, plane_id, vp(ptr(avg)), vp(ptr(avg))) == EINVAL
        assert np.all(get(avg) == -7.0)
    avg = put(np.zeros((1, 2, ny, nx)))
    assert L.tlab_avg_phase_space(nx, ny, nz, nz, 1, one, 1, 1, vp(ptr(avg))) == 0
    assert L.tlab_avg_phase_space(nx, ny, 0, nz, 1, one, 1, 1, vp(ptr(avg))) == EINVAL
    assert L.tlab_avg_phase_space(nx, ny, nz, 0, 1, one, 1, 1, vp(ptr(avg))) == EINVAL
    assert L.tlab_avg_phase_space(nx, ny, nz, nz, 0, one, 1, 1, vp(ptr(avg))) == EINVAL
    assert L.tlab_avg_phase_space(nx, ny, nz, nz, 1, one, 1, 1, None) == EINVAL


def check_towers(T, shape, stride, put, get, exact):
    """two full steps in the order 4, 1, 2 into a buffer of three; exact: data whose plane sums are exact (the means bitwise), else the means
    within the summation bound of AVG_IK_V and everything else bitwise"""
    nx, ny, nz = shape
    ref = S.Tower(nx, ny, nz, stride, 3)
    assert ref.consistent
    t = T.Tower(nx, ny, nz, stride, 3)
    assert (t.imax, t.jmax, t.kmax, t.isize_acc_field, t.isize_acc_mean, t.bufsize) == (ref.imax, ref.jmax, ref.kmax, ref.acc_field, ref.acc_mean,
                                                                                         ref.bufsize)
    assert np.array_equal(t.ipos, ref.ipos) and np.array_equal(t.jpos, ref.jpos) and np.array_equal(t.kpos, ref.kpos)
    buf = put(np.zeros(t.bufsize))
    make = dyadic_fields if exact else fields
    kept = []
    for step in range(2):
        u, v, w, p, s = make(shape, 5, 20 + step)
        kept.append((u, v, w, p, s))
        for index, fl in ((4, [p]), (1, [u, v, w]), (2, [s])):
            assert (t.accumulation, t.mode_check) == (ref.accumulation, ref.mode_check) == (step + 1, {4: 0, 1: 4, 2: 5}[index])
            ref.accumulate(index, fl, 100 + step, 0.25 * (step + 1))
            t.accumulate(index, [put(a) for a in fl], 100 + step, 0.25 * (step + 1), buf)
    assert (t.accumulation, t.mode_check) == (3, 0)      # advanced only on the sum 7
    got = get(buf)
    gv, rv = t.views(got), t.views(ref.buf)
    for name in ("u", "v", "w", "p", "s", "t", "it"):
        assert np.array_equal(gv[name], rv[name]), name
    assert np.array_equal(gv["it"][:2], [100.0, 101.0]) and np.array_equal(gv["t"][:2], [0.25, 0.5])
    assert gv["u"][0, 1 % t.kmax, 0, 2] == kept[0][0][t.kpos[1 % t.kmax] - 1, t.jpos[2] - 1, t.ipos[0] - 1]      # (kk, ii, j) as the reference runs them
    worst = 0.0
    for fi, name in enumerate(("um", "vm", "wm", "pm", "sm")):
        if exact:
            assert np.array_equal(gv[name], rv[name]), name
            continue
        for step in range(2):
            bound = S.summation_bound(kept[step][fi], t.jpos, rv[name][step])
            err = np.abs(gv[name][step] - rv[name][step])
            print("tower mean %s step %d: largest error / bound = %.3f" % (name, step, float((err / bound).max())))
            assert np.all(err <= bound), (name, step)
            worst = max(worst, float((err / bound).max()))
        assert np.all(gv[name][2] == 0.0)
    return t, buf, worst


def check_tower_refusals(T, L, put, get):
    from tlab_amd.lib import TlabError
    import pytest
    with pytest.raises(TlabError):
        T.Tower(9, 12, 8, (4, 1, 2), 3)                  # (9 - 1) mod 4 = 0: the reference writes past tower_ipos
    assert not S.Tower(9, 12, 8, (4, 1, 2), 3).consistent
    with pytest.raises(TlabError):
        T.Tower(16, 12, 8, (4, 1, 2), 0)
    shape = (16, 12, 8)
    nx, ny, nz = shape
    t = T.Tower(nx, ny, nz, (4, 1, 2), 1)
    buf = put(np.full(t.bufsize, -7.0))
    u, v, w, p, s = (put(a) for a in fields(shape, 5, 3))
    with pytest.raises(TlabError):
        t.accumulate(3, [p], 1, 0.1, buf)                # no such index
    t.accumulate(4, [p], 1, 0.1, buf)
    before = get(buf).copy()
    with pytest.raises(TlabError, match="greater than 7"):
        t.accumulate(4, [p], 1, 0.1, buf)                # 4 + 4 > 7
    t.accumulate(1, [u, v, w], 1, 0.1, buf)
    t.accumulate(2, [s], 1, 0.1, buf)
    assert (t.accumulation, t.mode_check) == (2, 0)
    before = get(buf).copy()
    with pytest.raises(TlabError, match="full"):
        t.accumulate(4, [p], 2, 0.2, buf)                # past nitera_save
    assert np.array_equal(get(buf), before) and (t.accumulation, t.mode_check) == (2, 0)
    t.reset()
    assert (t.accumulation, t.mode_check) == (1, 0)
    t.accumulate(4, [p], 2, 0.2, buf)


def check_planes(T, L, shape, put, get, ptr):
    nx, ny, nz = shape
    h = fields(shape, 3, 5)
    d = [put(a) for a in h]
    for idir, n in ((1, nx), (2, ny), (3, nz)):
        nodes = [1, n, 1] if n > 1 else [1, 1]           # the first and the last plane, one of them twice
        ref = S.planes_gather(h, idir, nodes)
        got = get(T.planes_gather(nx, ny, nz, d, idir, nodes))
        assert got.dtype == np.float64 and got.shape == ref.shape and np.array_equal(got, ref), idir
        got = get(T.planes_gather(nx, ny, nz, d, idir, nodes, single=True))
        assert got.dtype == np.float32 and np.array_equal(got, ref.astype(np.float32)), idir
        out = put(np.full(ref.shape, -7.0))
        ptrs = (vp * 3)(*[ptr(a) for a in d])
        for bad in (0, n + 1):
            assert L.tlab_planes_gather(nx, ny, nz, 3, ptrs, idir, 2, (ctypes.c_int * 2)(1, bad), vp(ptr(out)), 0) == EINVAL, (idir, bad)
        assert L.tlab_planes_gather(nx, ny, nz, 3, ptrs, 4, 1, (ctypes.c_int * 1)(1), vp(ptr(out)), 0) == EINVAL
        assert L.tlab_planes_gather(nx, ny, nz, 17, ptrs, idir, 1, (ctypes.c_int * 1)(1), vp(ptr(out)), 0) == EINVAL
        assert np.all(get(out) == -7.0)
