"""CPU checks of the tables of tests/periodic_tables.py themselves: the conditions under which the GPU tests that use them (tests/
test_gpu_periodic_tables.py, the `varying` cases of tests/test_gpu_zslab_operators.py) are able to fail.  They hold for the oracle alone.

 - the oracle's TRIDPFS + TRIDPSS on `varying` tables is the solution of the cyclic system: equal to a dense solve to <= 1e-13 relative;
 - a kernel that read its left-hand-side rows 1, 16 or 32 rows off would be wrong by >= 1e-3 relative on `varying` tables ...
 - ... and by < 1e-12 on `wander` tables (rows that differ by 1e-13): that kind alone cannot catch an indexing error under the 1e-12 tolerance;
 - slab 0's rows exchanged with slab 1's (the z-slab plans built for the wrong koffset) move the result by >= 1e-3.

The same for the pentadiagonal first derivative of scheme (5, 7) (tests/test_gpu_penta_lines.py: k_pentatile, k_penta1), second half of the file:
the tables are well conditioned, the oracle's PENTADPSS on them is exact to rounding, and two controls -- the left-hand rows rolled by one chunk
of 32 rows, and a numpy restatement of the chunked superposition whose chunks read the table rows of the chunk before them -- show on `varying`
tables and, away from the ends of the line, not on `equal` ones."""
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


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scheme (5, 7): five left-hand diagonals, PENTADPFS / PENTADPSS
# ---------------------------------------------------------------------------------------------------------------------------------------------
PENTA = (5, 7)
PM = 32                                          # rows per chunk of k_pentatile
PENTA_TILE = [64, 96, 160, 256, 480, 512]        # lengths of tests/test_gpu_penta_lines.py on k_pentatile: 2, 3, 5, 8, 15, 16 chunks
PENTA_LINE = [40, 80, 1024]                      # ... and on k_penta1 (1024 = 32 chunks: the restatement below runs there too)


def chunked_pentadpss(lu, frc, shifted=()):
    """PENTADPSS (linear5.f90:352-411) on the factors lu (n, 7) by chunks of PM rows, written from the reference's recurrences: each chunk runs
    G(i) = F(i) - G(i+1) D(i) - G(i+2) E(i) downwards and G(i) = (G(i) - G(i-1) B(i) - G(i-2) A(i)) / C(i) upwards with zero inflow, together with
    the two unit-inflow responses of its rows, and adds the responses times the two values that enter it; then the rank-two correction.  A chunk
    named in `shifted` takes every table row (factors, hence responses, and the correction vectors) from the chunk before it."""
    n, C = lu.shape[0], lu.shape[0] // PM
    a, b, c, d, e, F, G = (lu[:, k] for k in range(7))
    A, B, D, E = a.copy(), b.copy(), d.copy(), e.copy()
    D[n - 1] = E[n - 1] = E[n - 2] = 0.0         # rows without predecessors: G(n-1) = F(n-1) - G(n) D(n-1); G(1) = G(1) / C(1), G(2) = (G(2) - G(1) B(2)) / C(2)
    A[0] = B[0] = A[1] = 0.0
    f = frc.copy()
    table = lambda k: (k - 1 if k in shifted else k) * PM      # noqa: E731
    unit = np.eye(2)[:, :, None]                 # the two unit inflows, as lines of their own
    for down in (True, False):
        in1 = in2 = np.zeros(f.shape[1])         # what enters the chunk: the nearest and the second-nearest value of the chunk before it along the sweep
        for k in (range(C - 1, -1, -1) if down else range(C)):
            r0, t0 = k * PM, table(k)
            g1 = g2 = np.zeros(f.shape[1])
            h1, h2 = unit[0], unit[1]            # (2, 1): response 1 starts from (1, 0), response 2 from (0, 1)
            for p in (range(PM - 1, -1, -1) if down else range(PM)):
                c1, c2, piv = (D[t0 + p], E[t0 + p], 1.0) if down else (B[t0 + p], A[t0 + p], c[t0 + p])
                v = (f[r0 + p] - g1 * c1 - g2 * c2) / piv
                r = (-h1 * c1 - h2 * c2) / piv
                f[r0 + p] = v + r[0] * in1 + r[1] * in2
                g1, g2, h1, h2 = v, g1, r, h1
            first, second = (r0, r0 + 1) if down else (r0 + PM - 1, r0 + PM - 2)
            in1, in2 = f[first].copy(), f[second].copy()
    m1 = e[n - 1] * F[0] + a[0] * F[n - 2] + b[0] * F[n - 1] + 1.0
    m2 = e[n - 1] * G[0] + a[0] * G[n - 2] + b[0] * G[n - 1]
    m3 = d[n - 1] * F[0] + e[n - 1] * F[1] + a[0] * F[n - 1]
    m4 = d[n - 1] * G[0] + e[n - 1] * G[1] + a[0] * G[n - 1] + 1.0
    di = 1 / (m1 * m4 - m2 * m3)
    d1 = di * ((m4 * e[n - 1] - m2 * d[n - 1]) * f[0] + (m4 * b[0] - m2 * a[0]) * f[n - 1] + m4 * a[0] * f[n - 2] - m2 * e[n - 1] * f[1])
    d2 = di * ((m1 * d[n - 1] - m3 * e[n - 1]) * f[0] + (m1 * a[0] - m3 * b[0]) * f[n - 1] - m3 * a[0] * f[n - 2] + m1 * e[n - 1] * f[1])
    for k in range(C):
        r0, t0 = k * PM, table(k)
        f[r0:r0 + PM] -= d1[None, :] * F[t0:t0 + PM, None] + d2[None, :] * G[t0:t0 + PM, None]
    return f


@pytest.mark.parametrize("kind", PT.KINDS)
@pytest.mark.parametrize("n", PENTA_TILE + PENTA_LINE)
def test_penta_tables_are_well_conditioned_and_the_oracle_is_exact_to_rounding(n, kind):
    """Condition number of the cyclic pentadiagonal matrix <= 75 (37.5 on the uniform grid; 72.4 at most measured with amplitude 0.05), and the
    oracle's PENTADPSS in fp64 against the same recurrences on the same factors in np.longdouble <= 1e-14 (3.4e-16 .. 1.4e-15 measured): the
    GPU tests' 1e-12 is 700 times the reference's own rounding.  NOT asserted: agreement with a dense solve of the cyclic matrix -- PENTADPFS
    effectively solves a matrix that differs from it in the entries (1, n-1) and (n-2, 0), which no uniform grid shows
    (2e-15 on `equal`) and `varying` tables do (2e-3 .. 2e-2, printed).  The kernels restate the reference's algorithm on the same factors."""
    from oracle import tlab_oracle as O
    og = PT.oracle_plan(n, kind, PENTA)
    assert og.der1.nb_diag == (5, 7) and og.der1.lu.shape == (n, 7) and og.der2.nb_diag[0] == 3
    u = lines(n)
    rhs = PT.right_hand_side(og, 1, u)
    ref = PT.solve(og, 1, u)
    A = PT.cyclic_matrix(og.der1.lhs, 5)
    cond = np.linalg.cond(A)
    wide = rhs.astype(np.longdouble)
    lu = og.der1.lu.astype(np.longdouble)
    O.pentadpss(*(lu[:, k] for k in range(7)), wide)
    err = rel_err(ref, wide.astype(np.float64))
    # response of the descending recurrence to unit inflow after one chunk: what a wrong block one chunk further away is multiplied by
    g1, g2 = 1.0, 0.0
    for p in range(n - 8, n - 8 - PM, -1):
        g1, g2 = -g1 * og.der1.lu[p, 3] - g2 * og.der1.lu[p, 4], g1
    print("n=%d %s: condition number %.1f, fp64 against long double %.2e, against a dense solve %.2e, unit inflow after %d rows %.1e"
          % (n, kind, cond, err, rel_err(ref, np.linalg.solve(A, rhs)), PM, abs(g1)))
    assert cond <= 75.0, cond
    assert err <= 1e-14, err


@pytest.mark.parametrize("n", PENTA_TILE + PENTA_LINE)
def test_penta_rows_rolled_by_a_chunk_show_on_varying_tables_and_not_on_equal_ones(n):
    """First control: the left-hand rows rolled by one chunk (32 rows) and factorized again.  >= 1e-3 on `varying` tables (0.25 .. 0.71
    measured); exactly 0 on `equal` ones: why the uniform grids of tests/test_gpu_derivs.py::test_penta_first_derivative were not enough."""
    u = lines(n, 1)
    for kind in ("varying", "equal"):
        ref = PT.solve(PT.oracle_plan(n, kind, PENTA), 1, u)
        err = rel_err(PT.solve(PT.make_plan(n, kind, PENTA, roll=PM), 1, u), ref)
        print("n=%d %s rows rolled by %d: %.2e" % (n, kind, PM, err))
        if kind == "varying":
            assert err >= 1e-3, (n, err)
        else:
            assert err <= 1e-12, (n, err)


@pytest.mark.parametrize("n", PENTA_TILE + [1024])
def test_penta_chunks_reading_the_rows_of_the_chunk_before_them(n):
    """Second control: chunked_pentadpss -- first shown to BE the oracle's PENTADPSS (<= 1e-14 on every kind), then with chunks reading the
    table rows of the chunk before them.
      every chunk c >= 1 shifted (what a kernel with `row0 - 32` does): >= 1e-3 on `varying` tables at every length (0.9 .. 5.7 measured).
      On `equal` tables that shift shows as well (0.9 .. 4.4, printed): the factors of rows 1, 2 and of the last thirty-odd rows are not those
      of the interior (the factorization starts at row n and converges by 0.49 per row), so the uniform grids did see a wrong FIRST or LAST chunk.
      What they could not see is a wrong chunk in the far interior: chunks 3 <= c <= C - 3 (64 rows and more from either end, where the
      factors have converged to 0.49^64 = 1e-20 and the correction vectors have decayed as far) shifted: <= 1e-12 on `equal` tables
      (5e-16 .. 8e-16 measured, the restatement's own rounding), >= 1e-3 on `varying` ones (0.31 .. 0.47).  Such chunks exist from 6 chunks on (256, 480, 512, 1024 points); with chunks 2 and
      C - 2 included the `equal` figure is 1e-8 (the correction vectors 32 rows from the end are 1e-9), still far above 1e-12."""
    C = n // PM
    u = lines(n, 2)
    every, far = tuple(range(1, C)), tuple(range(3, C - 2))
    for kind in PT.KINDS:
        og = PT.oracle_plan(n, kind, PENTA)
        rhs, ref = PT.right_hand_side(og, 1, u), PT.solve(og, 1, u)
        same = rel_err(chunked_pentadpss(og.der1.lu, rhs), ref)
        e_every = rel_err(chunked_pentadpss(og.der1.lu, rhs, every), ref)
        e_far = rel_err(chunked_pentadpss(og.der1.lu, rhs, far), ref) if far else None
        print("n=%d %s: chunked restatement %.2e; chunks >= 1 shifted %.2e; chunks 3 .. C - 3 shifted %s" % (n, kind, same, e_every, "%.2e" % e_far if far else "(none)"))
        assert same <= 1e-14, (n, kind, same)
        if kind == "varying":
            assert e_every >= 1e-3, (n, e_every)
            assert e_far is None or e_far >= 1e-3, (n, e_far)
        elif kind == "equal":
            assert e_far is None or e_far <= 1e-12, (n, e_far)
