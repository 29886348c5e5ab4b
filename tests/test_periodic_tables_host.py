"""CPU checks of the tables of tests/periodic_tables.py themselves: the conditions under which the GPU tests that use them (tests/
test_gpu_periodic_tables.py, the `varying` cases of tests/test_gpu_zslab_operators.py) are able to fail.  They hold for the oracle alone.

 - the oracle's TRIDPFS + TRIDPSS on `varying` tables is the solution of the cyclic system: equal to a dense solve to <= 1e-13 relative;
 - a kernel that read its left-hand-side rows 1, 16 or 32 rows off would be wrong by >= 1e-3 relative on `varying` tables ...
 - ... and by < 1e-12 on `wander` tables (rows that differ by 1e-13): that kind alone cannot catch an indexing error under the 1e-12 tolerance;
 - slab 0's rows exchanged with slab 1's (the z-slab plans built for the wrong koffset) move the result by >= 1e-3."""
import numpy as np
import pytest
from conftest import rel_err
import periodic_tables as PT

SIZES = [64, 256, 512]
ROLLS = [1, 16, 32]
LINES = 7


def lines(n, seed=0):
    rng = np.random.default_rng(100 + n + seed)
    i = np.arange(n)[:, None]
    return np.sin(2.0 * np.pi * (1 + np.arange(LINES)[None, :] % 3) * i / n + 0.3 * np.arange(LINES)[None, :]) + 0.1 * rng.uniform(-1, 1, (n, LINES))


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_oracle_equals_a_dense_solve_of_the_cyclic_system(n, which):
    og = PT.oracle_plan(n, "varying")
    u = lines(n)
    lhs = (og.der1 if which == 1 else og.der2).lhs
    A = PT.cyclic_matrix(lhs)
    cond = np.linalg.cond(A)
    dense = np.linalg.solve(A, PT.right_hand_side(og, which, u))
    err = rel_err(PT.solve(og, which, u), dense)
    print("n=%d der%d: condition number %.2f, oracle against dense solve %.2e" % (n, which, cond, err))
    # well conditioned: the uniform second-derivative system has off-diagonal / diagonal = 4 / 11 per side, 0.402 at most after (1.05 / 0.95), so
    # that the row-scaled matrix has a condition number of at most (1 + 0.804) / (1 - 0.804) = 9.2 (Gershgorin; the first derivative, 1 / 3: 6.6);
    # 5.3 and 7.0 measured
    assert cond <= 10.0, cond
    assert err <= 1e-13, err                   # 7e-16 measured


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_rolled_rows_show_on_varying_tables_and_not_on_wandering_ones(n, which):
    u = lines(n, 1)
    for kind, visible in (("varying", True), ("wander", False)):
        ref = PT.solve(PT.oracle_plan(n, kind), which, u)
        for roll in ROLLS:
            err = rel_err(PT.solve(PT.make_plan(n, kind, roll=roll), which, u), ref)
            print("n=%d der%d %s rows rolled by %d: %.2e" % (n, which, kind, roll, err))
            if visible:
                assert err >= 1e-3, (kind, roll, err)       # 0.09 and more measured
            else:
                assert err < 1e-12, (kind, roll, err)       # 0.75e-13 .. 1.7e-13 measured: the wrong kernel would pass


def test_equal_rows_are_bit_identical_and_wander_rows_are_not():
    for n in SIZES:
        for kind in PT.KINDS:
            og = PT.oracle_plan(n, kind)
            for dp in (og.der1, og.der2):
                assert np.all(dp.rhs == dp.rhs[0]), (n, kind, "the right-hand side must be constants")
                assert bool(np.all(dp.lhs == dp.lhs[0])) == (kind == "equal"), (n, kind)
                if kind == "varying":      # every row differs from its neighbour and from the row one chunk (16, 32 rows) and one slab (64) away
                    for step in (s for s in (1, 8, 16, 32, 64) if s < n):
                        assert np.all(np.any(dp.lhs != np.roll(dp.lhs, step, axis=0), axis=1)), (n, step)


@pytest.mark.parametrize("kmax,P", [(64, 3), (96, 2), (128, 2), (256, 2)])
def test_exchanged_slab_rows_show(kmax, P):
    """The negative control of the z-slab cases: the oracle with the rows of slab 0 exchanged with those of slab 1 (what plans built for each
    other's koffset would solve) against the oracle on the tables as they are."""
    n = kmax * P
    u = lines(n, 2)
    for which in (1, 2):
        err = rel_err(PT.solve(PT.make_plan(n, "varying", swap=(0, kmax, kmax)), which, u), PT.solve(PT.oracle_plan(n, "varying"), which, u))
        print("kmax=%d P=%d der%d slab 0 <-> slab 1: %.2e" % (kmax, P, which, err))
        assert err >= 1e-3, (which, err)
