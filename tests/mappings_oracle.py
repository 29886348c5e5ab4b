"""numpy restatement of the reference's mappings/ routines, statement by statement: fi_vectorcalculus.f90 (FI_CURL, FI_INVARIANT_P/Q/R),
fi_strain.f90, fi_vorticity.f90 and fi_gradient.f90.  A plain module: neither a conftest nor a test.

Every numpy operation on float64 arrays is one IEEE operation per element, and Python evaluates a*b*c as (a*b)*c like Fortran, so each
statement below rounds where the Fortran statement rounds (no fused multiply-add, no reassociation).  The derivative operators come in as
callables p1(dir, f) and p2(dir, f) (dir = 1, 2, 3; OPR_Partial_X/Y/Z with OPR_P1 and OPR_P2, bcs = 0), so the same code runs on the
oracle's opr_partial, on the periodic differences of the golden fixture, and -- with from_gradients() -- on gradients that exist already,
which is what the pass k_gradient_maps and the host loop of tlab_gradient_maps are held to, bit for bit."""
import numpy as np


# ---- fi_vectorcalculus.f90 ------------------------------------------------------------------------------------------------------------------------
def fi_curl(p1, u, v, w):
    """:20-60 -> wx, wy, wz, tmp"""
    wz = p1(1, v)
    tmp = p1(2, u)
    wz = wz - tmp
    wy = p1(3, u)
    tmp = p1(1, w)
    wy = wy - tmp
    wx = p1(2, w)
    tmp = p1(3, v)
    wx = wx - tmp
    tmp = wx * wx + wy * wy + wz * wz
    return wx, wy, wz, tmp


def fi_invariant_p(p1, u, v, w):
    """:111-141"""
    result = p1(1, u)
    tmp1 = p1(2, v)
    result = result + tmp1
    tmp1 = p1(3, w)
    return -(result + tmp1)


def fi_invariant_q(p1, u, v, w):
    """:184-223"""
    tmp1, tmp2, tmp3 = p1(1, u), p1(2, v), p1(3, w)
    result = tmp1 * tmp2 + tmp2 * tmp3 + tmp3 * tmp1
    tmp1, tmp2 = p1(1, v), p1(2, u)
    result = result - tmp1 * tmp2
    tmp1, tmp2 = p1(1, w), p1(3, u)
    result = result - tmp1 * tmp2
    tmp1, tmp2 = p1(2, w), p1(3, v)
    result = result - tmp1 * tmp2
    return result


def fi_invariant_r(p1, u, v, w):
    """:229-270"""
    tmp1, tmp2, tmp3, tmp4, tmp5 = p1(3, w), p1(2, w), p1(2, v), p1(3, v), p1(1, u)
    result = tmp5 * (tmp1 * tmp3 - tmp2 * tmp4)
    tmp3, tmp4, tmp5 = p1(3, u), p1(2, u), p1(1, v)
    result = result + tmp5 * (tmp2 * tmp3 - tmp1 * tmp4)
    tmp1, tmp2, tmp5 = p1(3, v), p1(2, v), p1(1, w)
    result = result + tmp5 * (tmp1 * tmp4 - tmp2 * tmp3)
    return -result


# ---- fi_strain.f90 --------------------------------------------------------------------------------------------------------------------------------
def fi_strain_tensor(p1, u, v, w):
    """:29-63 -> Sxx, Syy, Szz, Sxy, Sxz, Syz"""
    tmp1, tmp4 = p1(1, v), p1(2, u)
    tmp4 = 0.5 * (tmp4 + tmp1)
    tmp1, tmp5 = p1(1, w), p1(3, u)
    tmp5 = 0.5 * (tmp5 + tmp1)
    tmp1, tmp6 = p1(2, w), p1(3, v)
    tmp6 = 0.5 * (tmp6 + tmp1)
    return p1(1, u), p1(2, v), p1(3, w), tmp4, tmp5, tmp6


def fi_strain(p1, u, v, w):
    """:68-99"""
    tmp1, tmp2 = p1(1, u), p1(2, v)
    result = tmp1 * tmp1 + tmp2 * tmp2
    tmp2 = p1(3, w)
    result = result + tmp2 * tmp2
    tmp1, tmp2 = p1(1, v), p1(2, u)
    result = result + 0.5 * (tmp1 + tmp2) * (tmp1 + tmp2)
    tmp1, tmp2 = p1(1, w), p1(3, u)
    result = result + 0.5 * (tmp1 + tmp2) * (tmp1 + tmp2)
    tmp1, tmp2 = p1(2, w), p1(3, v)
    result = result + 0.5 * (tmp1 + tmp2) * (tmp1 + tmp2)
    return result


def fi_strain_production(p1, u, v, w):
    """:113-163"""
    result = fi_vorticity_production(p1, u, v, w)
    result = 0.25 * result
    tmp1, tmp2 = p1(1, v), p1(2, u)
    s_12 = 0.5 * (tmp1 + tmp2)
    tmp1, tmp2 = p1(1, w), p1(3, u)
    s_13 = 0.5 * (tmp1 + tmp2)
    tmp1, tmp2 = p1(2, w), p1(3, v)
    s_23 = 0.5 * (tmp1 + tmp2)
    result = result + 2.0 * s_12 * s_13 * s_23
    tmp1 = p1(1, u)
    result = result + tmp1 * (tmp1 * tmp1 + 3.0 * (s_12 * s_12 + s_13 * s_13))
    tmp1 = p1(2, v)
    result = result + tmp1 * (tmp1 * tmp1 + 3.0 * (s_12 * s_12 + s_23 * s_23))
    tmp1 = p1(3, w)
    result = result + tmp1 * (tmp1 * tmp1 + 3.0 * (s_13 * s_13 + s_23 * s_23))
    return -result


def _laplacian_term(p2, f):
    """strain*(tmp1 + tmp2 + tmp3) without the factor: the three OPR_P2 in the reference's order z, y, x"""
    tmp3, tmp2, tmp1 = p2(3, f), p2(2, f), p2(1, f)
    return tmp1 + tmp2 + tmp3


def fi_strain_diffusion(p1, p2, u, v, w):
    """:169-249"""
    strain = p1(1, u)
    result = strain * _laplacian_term(p2, strain)
    strain = p1(2, v)
    result = result + strain * _laplacian_term(p2, strain)
    strain = p1(3, w)
    result = result + strain * _laplacian_term(p2, strain)
    strain = p1(1, v) + p1(2, u)
    result = result + 0.5 * strain * _laplacian_term(p2, strain)
    strain = p1(3, u) + p1(1, w)
    result = result + 0.5 * strain * _laplacian_term(p2, strain)
    strain = p1(2, w) + p1(3, v)
    result = result + 0.5 * strain * _laplacian_term(p2, strain)
    return result


def fi_strain_pressure(p1, p2, u, v, w, p):
    """:254-304"""
    tmp1, tmp2 = p1(1, u), p2(1, p)
    result = tmp1 * tmp2
    tmp1, tmp2 = p1(2, v), p2(2, p)
    result = result + tmp1 * tmp2
    tmp1, tmp2 = p1(3, w), p2(3, p)
    result = result + tmp1 * tmp2
    tmp1 = p1(2, p1(1, p))
    tmp2, tmp3 = p1(1, v), p1(2, u)
    result = result + tmp1 * (tmp2 + tmp3)
    tmp1 = p1(3, p1(1, p))
    tmp2, tmp3 = p1(1, w), p1(3, u)
    result = result + tmp1 * (tmp2 + tmp3)
    tmp1 = p1(3, p1(2, p))
    tmp2, tmp3 = p1(2, w), p1(3, v)
    result = result + tmp1 * (tmp2 + tmp3)
    return -result


def fi_strain_a(p1, a, u, v, w):
    """:310-362 -> strain1, strain2, tmp1 (= grad(a).grad(a)); normal1..3 are the gradient of a"""
    normal1, normal2, normal3 = p1(1, a), p1(2, a), p1(3, a)
    strain1 = normal1 * p1(1, u) * normal1
    strain1 = strain1 + normal2 * p1(2, u) * normal1
    strain1 = strain1 + normal3 * p1(3, u) * normal1
    strain1 = strain1 + normal1 * p1(1, v) * normal2
    strain1 = strain1 + normal2 * p1(2, v) * normal2
    strain1 = strain1 + normal3 * p1(3, v) * normal2
    strain1 = strain1 + normal1 * p1(1, w) * normal3
    strain1 = strain1 + normal2 * p1(2, w) * normal3
    strain1 = strain1 + normal3 * p1(3, w) * normal3
    tmp1 = normal1 * normal1 + normal2 * normal2 + normal3 * normal3      # normal1**2: the compiler's x*x
    strain2 = strain1.copy()
    pos = tmp1 > 0.0
    strain2[pos] = strain1[pos] / tmp1[pos]
    return strain1, strain2, tmp1


# ---- fi_vorticity.f90 -----------------------------------------------------------------------------------------------------------------------------
def fi_vorticity(p1, u, v, w):
    """:28-59"""
    tmp1, tmp2 = p1(1, v), p1(2, u)
    result = (tmp1 - tmp2) * (tmp1 - tmp2)
    tmp1, tmp2 = p1(3, u), p1(1, w)
    result = result + (tmp1 - tmp2) * (tmp1 - tmp2)
    tmp1, tmp2 = p1(2, w), p1(3, v)
    result = result + (tmp1 - tmp2) * (tmp1 - tmp2)
    return result


def fi_vorticity_production(p1, u, v, w):
    """:64-116"""
    vort_z = p1(1, v) - p1(2, u)
    vort_y = p1(3, u) - p1(1, w)
    vort_x = p1(2, w) - p1(3, v)
    tmp1, tmp2 = p1(1, u), p1(2, v)
    result = tmp1 * vort_x * vort_x + tmp2 * vort_y * vort_y
    tmp2 = p1(3, w)
    result = result + tmp2 * vort_z * vort_z
    tmp1, tmp2 = p1(1, v), p1(2, u)
    result = result + (tmp1 + tmp2) * vort_x * vort_y
    tmp1, tmp2 = p1(1, w), p1(3, u)
    result = result + (tmp1 + tmp2) * vort_x * vort_z
    tmp1, tmp2 = p1(2, w), p1(3, v)
    result = result + (tmp1 + tmp2) * vort_y * vort_z
    return result


def fi_vorticity_diffusion(p1, p2, u, v, w):
    """:122-167"""
    vort = p1(1, v) - p1(2, u)
    result = vort * _laplacian_term(p2, vort)
    vort = p1(3, u) - p1(1, w)
    result = result + vort * _laplacian_term(p2, vort)
    vort = p1(2, w) - p1(3, v)
    result = result + vort * _laplacian_term(p2, vort)
    return result


# ---- fi_gradient.f90 ------------------------------------------------------------------------------------------------------------------------------
def fi_gradient(p1, s):
    """:26-48"""
    result, tmp1 = p1(1, s), p1(2, s)
    result = result * result + tmp1 * tmp1
    tmp1 = p1(3, s)
    return result + tmp1 * tmp1


def fi_gradient_production(p1, s, u, v, w):
    """:53-94"""
    grad_x, grad_y, grad_z = p1(1, s), p1(2, s), p1(3, s)
    tmp1, tmp2 = p1(1, u), p1(2, v)
    result = tmp1 * grad_x * grad_x + tmp2 * grad_y * grad_y
    tmp2 = p1(3, w)
    result = result + tmp2 * grad_z * grad_z
    tmp1, tmp2 = p1(1, v), p1(2, u)
    result = result + (tmp1 + tmp2) * grad_x * grad_y
    tmp1, tmp2 = p1(1, w), p1(3, u)
    result = result + (tmp1 + tmp2) * grad_x * grad_z
    tmp1, tmp2 = p1(2, w), p1(3, v)
    return -(result + (tmp1 + tmp2) * grad_y * grad_z)


def fi_gradient_diffusion(p1, p2, s):
    """:100-133"""
    grad = p1(1, s)
    result = grad * _laplacian_term(p2, grad)
    grad = p1(2, s)
    result = result + grad * _laplacian_term(p2, grad)
    grad = p1(3, s)
    result = result + grad * _laplacian_term(p2, grad)
    return result


# ---- the maps of tlab_gradient_maps ---------------------------------------------------------------------------------------------------------------
MAPS = ("P", "Q", "R", "STRAIN", "STRAIN_TENSOR", "CURL", "VORTICITY", "VORTICITY_PRODUCTION", "STRAIN_PRODUCTION", "GRADIENT",
        "GRADIENT_PRODUCTION", "STRAIN_A")
SCALAR_MAPS = ("GRADIENT", "GRADIENT_PRODUCTION", "STRAIN_A")
NOUT = dict(zip(MAPS, (1, 1, 1, 1, 6, 4, 1, 1, 1, 1, 1, 3)))


def fi_map(name, p1, u, v, w, s=None):
    """the outputs of map `name` as a tuple of arrays, in the order of tlab_amd_mappings.h"""
    if name == "P":
        return (fi_invariant_p(p1, u, v, w),)
    if name == "Q":
        return (fi_invariant_q(p1, u, v, w),)
    if name == "R":
        return (fi_invariant_r(p1, u, v, w),)
    if name == "STRAIN":
        return (fi_strain(p1, u, v, w),)
    if name == "STRAIN_TENSOR":
        return fi_strain_tensor(p1, u, v, w)
    if name == "CURL":
        return fi_curl(p1, u, v, w)
    if name == "VORTICITY":
        return (fi_vorticity(p1, u, v, w),)
    if name == "VORTICITY_PRODUCTION":
        return (fi_vorticity_production(p1, u, v, w),)
    if name == "STRAIN_PRODUCTION":
        return (fi_strain_production(p1, u, v, w),)
    if name == "GRADIENT":
        return (fi_gradient(p1, s),)
    if name == "GRADIENT_PRODUCTION":
        return (fi_gradient_production(p1, s, u, v, w),)
    if name == "STRAIN_A":
        return fi_strain_a(p1, s, u, v, w)
    raise KeyError(name)


def from_gradients(du9, ds3=None):
    """(p1, u, v, w, s) for the routines above when the derivatives exist: the fields are the names "u", "v", "w", "s" and p1 looks the
    gradient up in du9 = [u,x u,y u,z v,x v,y v,z w,x w,y w,z], ds3 = [s,x s,y s,z].  A copy is handed out: no routine changes its input."""
    table = {("uvw"[c], d + 1): du9[3 * c + d] for c in range(3) for d in range(3)}
    if ds3 is not None:
        table.update({("s", d + 1): ds3[d] for d in range(3)})
    return (lambda d, f: np.array(table[(f, d)], dtype=np.float64)), "u", "v", "w", "s"


def gradient_maps(du9, ds3, maps):
    """what tlab_gradient_maps must give: a dict name -> tuple of arrays"""
    p1, u, v, w, s = from_gradients(du9, ds3)
    return {m: fi_map(m, p1, u, v, w, s) for m in maps}


FI_DIFFUSION = {
    "VORTICITY_DIFFUSION": lambda p1, p2, q, f: fi_vorticity_diffusion(p1, p2, *q),
    "STRAIN_DIFFUSION": lambda p1, p2, q, f: fi_strain_diffusion(p1, p2, *q),
    "GRADIENT_DIFFUSION": lambda p1, p2, q, f: fi_gradient_diffusion(p1, p2, f),
    "STRAIN_PRESSURE": lambda p1, p2, q, f: fi_strain_pressure(p1, p2, *q, f),
}


# ---- the stand-in operators of the golden fixture (tests/golden/make_golden_mappings.py) -----------------------------------------------------------
def standin_operators(nx, ny, nz):
    """p1, p2 on flat fields of a box (nx, ny, nz), x fastest: the periodic one-point difference f(i+1) - f(i) along the direction, and its
    second difference p1(p1(f)).  One rounding per result, so numpy and the compiled stand-in agree in every bit."""
    ax = {1: 2, 2: 1, 3: 0}

    def p1(d, f):
        a = np.asarray(f, dtype=np.float64).reshape(nz, ny, nx)
        return (np.roll(a, -1, axis=ax[d]) - a).reshape(-1)

    def p2(d, f):
        return p1(d, p1(d, f))

    return p1, p2
