"""Restatement of the head of DNS_STATISTICS_TEMPORAL (tools/dns/dns_statistics.f90:93-117) in the reference's statement order:

  fi_pressure_boussinesq   FI_PRESSURE_BOUSSINESQ (physics/fi_pressure_boussinesq.f90:8-280), all six decompositions, written on the operator
                           methods of oracle.tlab_oracle_rhs.DnsOracle (burgers, p1, pint, weight, solve_poisson) -- so it runs as well on
                           oracle.tlab_ref_rhs.RefComposedDns, whose methods are the reference's compiled routines.  The body forces are those
                           of tests/sources_oracle.py.
  fi_vorticity             FI_VORTICITY (mappings/fi_vorticity.f90:28-59)
  inter_n_xz               INTER_N_XZ over INTER1V2D (statistics/avg_xz.f90:134-139, utils/averages.f90:214-239)
  intermittency            the block stats_intermittency itself (dns_statistics.f90:99-117)

The advecting velocity of a Burgers term is the argument the routine PASSES (u, v, w; tmp9 = 0 in the diffusion block, :117-141).  The reference's
OPR_Burgers as compiled does not honour that argument everywhere (OPR_B_SELF advects with the field itself, OPR_B_U_IN along x -- and along y when
nz > 1 -- with the transposed velocity the call before left in tmp1; physics/opr_burgers.f90:236-240, :323-331), so its DCMP_DIFFUSION and
DCMP_ADVECTION are not a diffusion and an advection pressure; DESIGN.md section 2 records the defect and this file, like the device, states what
the calls say.  TEST INFRASTRUCTURE (numpy only)."""
import numpy as np

from oracle import tlab_oracle as O
from sources_oracle import EQNS_BOD_NONE, EQNS_COR_NONE, buoyancy, coriolis, sources_flow

DCMP_TOTAL, DCMP_RESOLVED, DCMP_ADVECTION, DCMP_ADVDIFF, DCMP_DIFFUSION, DCMP_CORIOLIS, DCMP_BUOYANCY = range(7)      # include/dns_const.h:30-36
DECOMPOSITIONS = {"total": DCMP_TOTAL, "advection": DCMP_ADVECTION, "advdiff": DCMP_ADVDIFF, "diffusion": DCMP_DIFFUSION, "coriolis": DCMP_CORIOLIS,
                  "buoyancy": DCMP_BUOYANCY}


# ---- the cases of tests/golden/pressure_ref.npz (made by tests/golden/make_golden_pressure.py, read by tests/test_pressure_host.py): inputs come
# from seeds, the file holds results only ----
GOLDEN_BOXES = {"a": (16, 12, 8, True), "b": (24, 14, 10, False)}      # nx, ny, nz, stretched y
GOLDEN_CASES = ("total", "advdiff", "advection", "diffusion")
GOLDEN_STRIDE = 5                                                      # the file holds every fifth point of a field (coprime with nx: every column is met)
GOLDEN_VISC, GOLDEN_SC = 1.0 / 800.0, (0.7,)
GOLDEN_COR = (4, (0.0, 1.5, 0.0), ())                                  # [Rotation] explicit
GOLDEN_BOD = (6, (0.0, -2.0, 0.0), 1, (1.0, 0.1), 1, None)             # [BodyForce] linear in one scalar


def golden_case(box):
    """dict(x, y, z, yuniform, q, s, gate) of box "a" or "b": the fields of tests/cases.py, and a gate with the levels 0..3 and an empty plane"""
    import cases as C
    nx, ny, nz, stretch = GOLDEN_BOXES[box]
    x, y, z = C.grids(nx, ny, nz, stretch)
    q, s = C.init_fields(nx, ny, nz, x, y, z, 40 + nx)
    gate = np.random.default_rng(nx).integers(0, 4, (nz, ny, nx)).astype(np.int8)
    gate[:, 1, :] = 0
    return dict(x=x, y=y, z=z, yuniform=not stretch, q=q, s=s, gate=gate)


def golden_oracle(case, cls=None):
    """a DnsOracle (or cls, with its interface) of the case, fields loaded"""
    from oracle.tlab_oracle_rhs import DnsOracle
    o = (cls or DnsOracle)(case["x"], case["y"], case["z"], nscal=1, visc=GOLDEN_VISC, schmidt=GOLDEN_SC, yuniform=case["yuniform"])
    o.q = [a.copy() for a in case["q"]]
    o.s = [a.copy() for a in case["s"]]
    return o


def _burgers_block(o, fields, vel, sums):
    """the nine calls of :93-112 (or :120-141) in their order: sums[i] = sums[i] + p after every call"""
    u, v, w = fields
    nu = o.visc
    for d, order in ((1, (0, 1, 2)), (2, (1, 0, 2)), (3, (2, 1, 0))):      # X: u v w; Y: v u w; Z: w v u
        for i in order:
            sums[i] = sums[i] + o.burgers(d, nu, (u, v, w)[i], vel[d - 1])


def fi_pressure_boussinesq(o, decomposition=DCMP_TOTAL, cor=None, bod=None):
    """p of the fields o.q, o.s of a DnsOracle (or a class with its operator methods).  cor, bod: the tuples of sources_oracle.sources_flow."""
    nx, ny, nz, n = o.nx, o.ny, o.nz, o.n
    dc = DECOMPOSITIONS[decomposition] if isinstance(decomposition, str) else int(decomposition)
    if dc not in DECOMPOSITIONS.values():
        raise ValueError("not a case of FI_PRESSURE_BOUSSINESQ: %r" % (decomposition,))
    q, s = o.q, o.s
    tmp = [np.zeros(n) for _ in range(3)]                                                                   # :58-59
    sources_flow(cor, bod, q, s, tmp, nx, ny, nz)                                                           # :68
    if dc != DCMP_TOTAL:                                                                                    # :74-86
        tmp = [np.zeros(n) for _ in range(3)]
    dif = [np.zeros(n) for _ in range(3)]                                                                   # tmp6, tmp7, tmp8
    if dc in (DCMP_ADVDIFF, DCMP_TOTAL, DCMP_ADVECTION):                                                    # :91-114
        _burgers_block(o, q, q, tmp)
    if dc in (DCMP_ADVECTION, DCMP_DIFFUSION):                                                              # :116-143
        zero = np.zeros(n)                                                                                  # tmp9
        _burgers_block(o, q, (zero, zero, zero), dif)
    if dc == DCMP_ADVECTION:                                                                                # :145-148
        tmp = [a - b for a, b in zip(tmp, dif)]
    elif dc == DCMP_DIFFUSION:                                                                              # :150-153
        tmp = [b.copy() for b in dif]
    if dc == DCMP_CORIOLIS and cor is not None and cor[0] != EQNS_COR_NONE:                                 # :158-163
        coriolis(cor[0], cor[1], cor[2], q, tmp)
    if dc == DCMP_BUOYANCY and bod is not None and bod[0] != EQNS_BOD_NONE:                                 # :166-196
        btype, vector, nscalars, parameters, inb, ref = bod
        ref = np.zeros(ny) if ref is None else np.asarray(ref, dtype=np.float64)
        for iq in range(3):
            if abs(float(vector[iq])) > 0.0:                                                                # buoyancy%active(iq)
                b = buoyancy(btype, nscalars, parameters, inb, s, ref if iq == 1 else np.zeros(ny), nx, ny, nz)      # :172-177
                tmp[iq] = tmp[iq] + float(vector[iq]) * b
    tmp3, tmp4, tmp5 = tmp
    VP0, VP1, PV0 = O.OPR_P0_INT_VP, O.OPR_P1_INT_VP, O.OPR_P0_INT_PV
    anel = getattr(o, "anelastic", None)
    stag = getattr(o, "stagger", False)
    p = np.zeros(n)                                                                                         # :202
    if anel is not None:                                                                                    # :212-214
        tmp3 = o.weight(anel[0], tmp3)
    p = p + (o.pint(3, VP0, o.pint(1, VP1, tmp3)) if stag else o.p1(1, tmp3))                               # :215-221
    if anel is not None:                                                                                    # :224-226
        tmp4 = o.weight(anel[0], tmp4)
    p = p + (o.pint(3, VP0, o.p1(2, o.pint(1, VP0, tmp4))) if stag else o.p1(2, tmp4))                      # :227-234
    if anel is not None:                                                                                    # :237-239
        tmp5 = o.weight(anel[0], tmp5)
    p = p + (o.pint(3, VP1, o.pint(1, VP0, tmp5)) if stag else o.p1(3, tmp5))                               # :240-246
    if stag:                                                                                                # :255-259
        tmp4 = o.pint(3, VP0, o.pint(1, VP0, tmp4))
    h2 = tmp4.reshape(nz, ny, nx)                                                                           # (weighted already: no second weight)
    hb, ht = h2[:, 0, :].copy(), h2[:, ny - 1, :].copy()                                                    # :260-262
    p = o.solve_poisson(p, hb, ht)[0]                                                                       # :264
    if any(f is not None for f in getattr(o, "pressure_filter", [None])):                                   # :267-269
        from oracle.tlab_oracle_filter import opr_filter
        p = opr_filter(nx, ny, nz, o.pressure_filter, p)
    if stag:                                                                                                # :272-275
        p = o.pint(1, PV0, o.pint(3, PV0, p))
    return p


def vorticity_from_gradients(vx, uy, uz, wx, wy, vz):
    """:41, :46, :51 -- three statements, one rounding per operation"""
    r = (vx - uy) * (vx - uy)
    r = r + (uz - wx) * (uz - wx)
    return r + (wy - vz) * (wy - vz)


def fi_vorticity(o):
    """(result, [v,x  u,y  u,z  w,x  w,y  v,z]) of the velocities o.q"""
    u, v, w = o.q
    six = [o.p1(1, v), o.p1(2, u), o.p1(3, u), o.p1(1, w), o.p1(2, w), o.p1(3, v)]
    return vorticity_from_gradients(*six), six


def inter_n_xz(gate, np_):
    """inter (np_, ny): row ip - 1 is column ip of the reference's inter(ny, np).  gate: int8 (nz, ny, nx).  The reference sums 1.0_wp over the
    plane -- exact below 2^53 -- and divides once by real(nx*nz)."""
    g = np.asarray(gate)
    nz, ny, nx = g.shape
    out = np.zeros((np_, ny))
    for ip in range(1, np_ + 1):
        for j in range(ny):
            out[ip - 1, j] = np.float64(np.count_nonzero(g[:, j, :] == ip)) / np.float64(nx * nz)
    return out


def intermittency(vort, nx, ny, nz):
    """dns_statistics.f90:104-114 from the vorticity magnitude: {"Vorticity": (ny,)} and the gate"""
    amax = np.float64(vort.max())
    amin = np.float64(1.0e-3) * np.float64(1.0e-3) * amax                # :105 (its comment says 0.1 %; the code is 1e-6)
    gate = (vort > amin).astype(np.int8).reshape(nz, ny, nx)
    return {"Vorticity": inter_n_xz(gate, 1)[0]}, gate
