"""Tables of a PERIODIC direction whose rows differ, for the tests of the chunked compact-scheme kernels (k_xline, k_rtile / k_htile / k_ptile along z,
k_zslab).  With the tables of a uniform grid the cyclic tridiagonal system is circulant: a kernel that reads the rows of the wrong chunk, swaps a
slab's separator row with its neighbour's, builds a z-slab plan for the wrong koffset, transposes the dense separator inverse or reverses the lane
order of its per-lane tables computes the same numbers.  TEST INFRASTRUCTURE (uses oracle/ only; tests/test_periodic_tables_host.py holds the
conditions under which the tables can tell such a kernel from a right one).

Every kind starts from the oracle's plan of a uniform periodic grid, O.FdmPlan(nodes, True, True, m1, m2).  For both derivatives the right-hand side
becomes its middle row in every row, bit-identical (the periodic kernels take the right-hand side as constants), the left-hand side becomes

  equal    the middle row in every row;
  wander   the middle row x (1 + 1e-13 u_i), one factor per row: what the reference's own tables of a "uniform" grid look like;
  varying  each of the three coefficients of each row x (1 + AMPLITUDE u), independent u in [-1, 1], fixed seed.  AMPLITUDE = 0.05: the worst row
           ratio off-diagonal / diagonal is then 0.37 (first derivative) and 0.40 (second), a separator decay of less than 0.5 per row, which
           keeps slabs of 64 planes under the 1e-19 coupling limit of tlab_zslab_plan_create (the same quantity worked out in numpy from these
           tables: 2.5e-27 and 8.4e-24 for three slabs of 64 planes, far less for thicker ones); the systems stay well conditioned (condition
           number 7.0 at most, tests/test_periodic_tables_host.py),

and is factorized again with the oracle's TRIDPFS into lu.  device_plan hands the very same arrays to tlab_fdm_plan_create_from_arrays.

Scheme m = (5, 7) (CompactJacobian6Penta; tests/test_gpu_penta_lines.py: k_pentatile, k_penta1): the first derivative has five left-hand
diagonals and seven right-hand ones.  The same three kinds act on its five coefficients per row (`varying`: five independent factors), the
right-hand side is its middle row in every row, lu comes from the oracle's PENTADPFS (7 columns: five factors and the two vectors of the
rank-two correction), and the library factorizes the lhs it is given itself; the second derivative stays tridiagonal and is treated as above.
With AMPLITUDE = 0.05 the condition number of the cyclic matrix is 72.4 at most (37.5 uniform) and the response to unit inflow after a chunk
of 32 rows 6e-10 .. 5e-8.  PENTADPFS inverts a matrix that differs from the cyclic one in two corner entries as soon as rows differ (DESIGN.md
section 2, defect 15): the oracle, never a dense solve, is the reference on these tables."""
import numpy as np

KINDS = ("equal", "wander", "varying")
AMPLITUDE = 0.05
WANDER = 1e-13

_PLANS = {}


def nodes(n):
    return np.arange(n) / n * 2.0


def refactor(dp):
    """dp.lu from dp.lhs: TRIDPFS on copies of the three diagonals (5 columns), PENTADPFS on copies of the five (7 columns)"""
    from oracle import tlab_oracle as O
    n, ndl = dp.lhs.shape[0], dp.nb_diag[0]
    assert ndl in (3, 5), "tridiagonal and pentadiagonal left-hand sides only"
    cols = [dp.lhs[:, k].copy() if k < ndl else np.zeros(n) for k in range(ndl + 2)]
    (O.tridpfs if ndl == 3 else O.pentadpfs)(*cols)
    dp.lu = np.stack(cols, axis=1)


def make_plan(n, kind, m=(6, 7), amplitude=AMPLITUDE, roll=0, swap=None):
    """A fresh oracle plan of n periodic points with tables of `kind`.  roll: the left-hand-side rows moved by that many rows (np.roll), swap = (a, b,
    rows): the rows a .. a + rows - 1 exchanged with b .. b + rows - 1 -- the negative controls of the host tests; the right-hand side never moves."""
    from oracle import tlab_oracle as O
    assert kind in KINDS, kind
    og = O.FdmPlan(nodes(n), True, True, *m)
    mid = n // 2
    for which, dp in ((1, og.der1), (2, og.der2)):
        rng = np.random.default_rng([n, which, KINDS.index(kind), m[0], m[1]])
        ndl = dp.nb_diag[0]                      # 3; 5 for the first derivative of scheme (5, 7)
        row = dp.lhs[mid, :ndl].copy()
        if kind == "equal":
            f = np.ones((n, ndl))
        elif kind == "wander":
            f = np.repeat(1.0 + WANDER * rng.uniform(-1, 1, (n, 1)), ndl, axis=1)
        else:
            f = 1.0 + amplitude * rng.uniform(-1, 1, (n, ndl))
        lhs = np.zeros_like(dp.lhs)
        lhs[:, :ndl] = row[None, :] * f
        if roll:
            lhs = np.roll(lhs, roll, axis=0)
        if swap is not None:
            a, b, rows = swap
            lhs[a:a + rows], lhs[b:b + rows] = lhs[b:b + rows].copy(), lhs[a:a + rows].copy()
        dp.lhs = lhs
        dp.rhs = np.tile(dp.rhs[mid], (n, 1))
        refactor(dp)
    og.table_kind = kind
    return og


def oracle_plan(n, kind, m=(6, 7), amplitude=AMPLITUDE):
    """make_plan, made once per key and shared: never modified by a test"""
    key = (n, kind, tuple(m), amplitude)
    if key not in _PLANS:
        _PLANS[key] = make_plan(n, kind, m, amplitude)
    return _PLANS[key]


def host_tables(og):
    """what tlab_fdm_plan_create_from_arrays takes: lhs1, rhs1 [:, :ndr1], lhs2, rhs2 [:, :ndr2 + 3]"""
    return og.der1.lhs, og.der1.rhs[:, :og.der1.nb_diag[1]], og.der2.lhs, og.der2.rhs[:, :og.der2.nb_diag[1] + 3]


def device_plan(T, og):
    """tlab_amd.FdmPlan from the oracle plan's arrays (operators only: no wavenumbers).  A pentadiagonal lhs1 is factorized by the library itself
    (tlab_fdm_plan_create_from_arrays: the reference's PENTADPFS restated in C++)."""
    return T.FdmPlan.from_arrays(og.size, True, 0, *host_tables(og), ndl1=og.der1.nb_diag[0])


def device_plan_for_driver(T, og):
    """... with what the Poisson solver and the monitors take from a plan besides: the uniform plan's modified wavenumbers, Jacobian and nodes"""
    assert og.der1.nb_diag[0] == 3, "the drivers take tridiagonal first derivatives only"
    lhs1, rhs1, lhs2, rhs2 = host_tables(og)
    tab = {"ndr1": og.der1.nb_diag[1], "ndr2": og.der2.nb_diag[1], "need_1der": 0, "lhs1": lhs1, "rhs1": rhs1, "lhs2": lhs2, "rhs2": rhs2,
           "mwn1": og.der1.mwn, "mwn2": og.der2.mwn, "jac": og.jac, "nodes": og.nodes}
    return T.FdmPlan.from_tables(tab, periodic=True, scheme1=og.der1.mode_fdm, scheme2=og.der2.mode_fdm)


def cyclic_matrix(lhs, ndl=3):
    """dense matrix of the cyclic system with ndl = 3 or 5 diagonals: row i holds lhs[i, k] at column i + k - ndl // 2 (mod n)"""
    n = lhs.shape[0]
    A = np.zeros((n, n))
    i = np.arange(n)
    for k in range(ndl):
        A[i, (i + k - ndl // 2) % n] = lhs[:, k]
    return A


def right_hand_side(og, which, u):
    """B u of derivative `which` by the oracle's own MatMul routines, u: (n, lines)"""
    from oracle import tlab_oracle as O
    f = np.empty_like(u)
    if which == 1:
        O.der1_matmul(og.der1, u, f, O.BCS_PERIODIC)
    elif og.der2.nb_diag[1] == 5:
        O.matmul_5d_sym(og.der2.rhs, u, f, O.BCS_PERIODIC)
    else:
        O.matmul_7d_sym(og.der2.rhs, u, f, O.BCS_PERIODIC)
    return f


def solve(og, which, u):
    """derivative `which` of the lines u (n, lines) by the oracle: right-hand side + TRIDPSS (PENTADPSS for five diagonals) on og's lu"""
    from oracle import tlab_oracle as O
    if which == 1:
        return O.der1_solve(og.der1, 0, u)
    return O.der2_solve(og.der2, og.der2.lu, u, np.zeros_like(u))
