// C ABI of include/tlab_amd.h: the finite-difference plan -- matrices, stencils, cached device systems -- and its entry points.
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "errors.hpp"
#include "internal.hpp"
#include "kernels.hpp"
#include "plan.hpp"

using namespace tlab;

// ------------------------------------------------------------------------------------------------
// plan: matrices, stencils, cached device systems
// ------------------------------------------------------------------------------------------------
namespace {

// FDM_Bcs_Neumann on a copy of the first derivative's tridiagonal LHS (only if `reduce`): the reduced LHS and the boundary rows of the RHS
struct NeumannReduced {
    std::vector<double> lhs;
    double rb[4 * 8] = {0}, rt[5 * 7] = {0};
    NeumannReduced(const DerTables &d, int ibc, bool reduce) {
        if (!reduce) return;
        lhs.assign(d.lhs.begin(), d.lhs.begin() + (size_t)3 * d.n);
        fdm_bcs_neumann(ibc, d.n, 3, lhs.data(), d.ndr, d.rhs.data(), rb, rt);
    }
    double RB(int j, int c) const { return rb[(j - 1) + 4 * c]; }
    double RT(int rr, int c) const { return rt[rr + 5 * (c - 1)]; }
};

#define RI(i, k) r[((i)-1) + (size_t)nx * ((k)-1)]
// the three rows at each wall of a pentadiagonal RHS r(nx, 5) as the reference's loops read them (MatMul_5d fdm_matmul.f90:291-318, MatMul_5d_antisym :382-415)
void penta_rows_bottom(StencilDev &s, const double *r, int nx) {
    s.bb[0][0] = RI(1, 3); s.bb[0][1] = RI(1, 4); s.bb[0][2] = RI(1, 5); s.bb[0][3] = RI(1, 1);
    s.bb[1][0] = RI(2, 2); s.bb[1][1] = RI(2, 3); s.bb[1][2] = RI(2, 4); s.bb[1][3] = RI(2, 5);
    for (int k = 0; k < 5; ++k) s.bb[2][k] = RI(3, 1 + k);
}
void penta_rows_top(StencilDev &s, const double *r, int nx) {
    for (int k = 0; k < 5; ++k) s.bt[0][1 + k] = RI(nx - 2, 1 + k);
    for (int k = 0; k < 4; ++k) s.bt[1][2 + k] = RI(nx - 1, 1 + k);
    s.bt[2][2] = RI(nx, 5); s.bt[2][3] = RI(nx, 1); s.bt[2][4] = RI(nx, 2); s.bt[2][5] = RI(nx, 3);
}
// [nx][5] = r1..r5 of every row of a direct scheme (StencilDev::rowc)
std::vector<double> penta_rowc(const double *r, int nx) {
    std::vector<double> rc((size_t)5 * nx, 0.0);
    for (int i = 1; i <= nx; ++i)
        for (int k = 1; k <= 5; ++k) rc[(size_t)(i - 1) * 5 + (k - 1)] = RI(i, k);
    for (int i = 5; i <= nx - 4; ++i) rc[(size_t)(i - 1) * 5 + 3] = 1.0;       // the interior loop has no r4 factor (:303-305)
    return rc;
}

}  // namespace

TriDiag tlab_fdm_plan::tridiag(int which, int ibc) const {
    const DerTables &d = (which == 1) ? t.der1 : t.der2;
    const int n = d.n;
    if (d.ndl != 3) throw Fail(TLAB_EUNSUPPORTED, "only tridiagonal LHS schemes are built (CompactJacobian6Penta is not)");
    const bool reduce = which == 1 && !d.periodic && ibc != BCS_DD;
    const NeumannReduced nr(d, ibc, reduce);
    const double *lhs = reduce ? nr.lhs.data() : d.lhs.data();
    TriDiag T;
    T.n = n;
    T.periodic = d.periodic;
    T.a.assign(lhs, lhs + n);
    T.b.assign(lhs + n, lhs + 2 * n);
    T.c.assign(lhs + 2 * n, lhs + 3 * n);
    if (which == 1 && !d.periodic) {
        if (ibc == BCS_ND || ibc == BCS_NN) {  // wall value forced to zero (fdm_derivative.f90:239-241): identity row
            T.a[0] = 0; T.b[0] = 1; T.c[0] = 0; T.a[1] = 0;
        }
        if (ibc == BCS_DN || ibc == BCS_NN) {
            T.a[n - 1] = 0; T.b[n - 1] = 1; T.c[n - 1] = 0; T.c[n - 2] = 0;
        }
    }
    return T;
}

StencilDev tlab_fdm_plan::stencil(int which, int ibc) {
    const DerTables &d = (which == 1) ? t.der1 : t.der2;
    const int nx = d.n;
    StencilDev s;
    std::memset(&s, 0, sizeof(s));
    s.sym = (which == 2);
    s.periodic = d.periodic ? 1 : 0;
    const double *r = d.rhs.data();
    const bool nb = (ibc == BCS_ND || ibc == BCS_NN), ntp = (ibc == BCS_DN || ibc == BCS_NN);
#define RB(j, c) nr.RB(j, c)
#define RT(rr, c) nr.RT(rr, c)
    if (which == 1 && d.direct) {   // MatMul_3d / MatMul_5d (fdm_matmul.f90:70-121, 265-319) with the Neumann-reduced rows of the variant
        if ((d.ndr != 3 && d.ndr != 5) || d.periodic) throw Fail(TLAB_EUNSUPPORTED, "direct first derivative: 3 or 5 RHS diagonals in a non-periodic direction");
        const NeumannReduced nr(d, ibc, nb || ntp);
        std::vector<double> rc;
        if (d.ndr == 5) {
            rc = penta_rowc(r, nx);
            if (nb) {       // f(1) carries the boundary value, 0 (fdm_derivative.f90:240): its terms are dropped
                s.bb[1][1] = RB(2, 3); s.bb[1][2] = RB(2, 4); s.bb[1][3] = RB(2, 5);
                s.bb[2][1] = RB(3, 2); s.bb[2][2] = RB(3, 3); s.bb[2][3] = RB(3, 4); s.bb[2][4] = RB(3, 5);
                for (int k = 1; k <= 5; ++k) rc[(size_t)3 * 5 + (k - 1)] = RB(4, k);
            } else {
                penta_rows_bottom(s, r, nx);
            }
            if (ntp) {
                for (int k = 1; k <= 5; ++k) rc[(size_t)(nx - 4) * 5 + (k - 1)] = RT(0, k);
                s.bt[0][1] = RT(1, 1); s.bt[0][2] = RT(1, 2); s.bt[0][3] = RT(1, 3); s.bt[0][4] = RT(1, 4);
                s.bt[1][2] = RT(2, 1); s.bt[1][3] = RT(2, 2); s.bt[1][4] = RT(2, 3);
            } else {
                penta_rows_top(s, r, nx);
            }
        } else {
            rc.assign((size_t)5 * nx, 0.0);
            for (int i = 1; i <= nx; ++i) {       // (0, r1, r2, 1, 0): the interior loop has no r3 factor (:103-105)
                rc[(size_t)(i - 1) * 5 + 1] = RI(i, 1); rc[(size_t)(i - 1) * 5 + 2] = RI(i, 2); rc[(size_t)(i - 1) * 5 + 3] = 1.0;
            }
            if (nb) {
                s.bb[1][1] = RB(2, 2); s.bb[1][2] = RB(2, 3);
                s.bb[2][1] = RB(3, 1); s.bb[2][2] = RB(3, 2); s.bb[2][3] = RB(3, 3);
            } else {
                s.bb[0][0] = RI(1, 2); s.bb[0][1] = RI(1, 3); s.bb[0][2] = RI(1, 1);
                s.bb[1][0] = RI(2, 1); s.bb[1][1] = RI(2, 2); s.bb[1][2] = RI(2, 3);
                s.bb[2][1] = RI(3, 1); s.bb[2][2] = RI(3, 2); s.bb[2][3] = RI(3, 3);
            }
            if (ntp) {
                s.bt[0][2] = RT(0, 1); s.bt[0][3] = RT(0, 2); s.bt[0][4] = RT(0, 3);
                s.bt[1][3] = RT(1, 1); s.bt[1][4] = RT(1, 2);
            } else {
                s.bt[0][2] = RI(nx - 2, 1); s.bt[0][3] = RI(nx - 2, 2); s.bt[0][4] = RI(nx - 2, 3);
                s.bt[1][3] = RI(nx - 1, 1); s.bt[1][4] = RI(nx - 1, 2); s.bt[1][5] = RI(nx - 1, 3);
                s.bt[2][3] = RI(nx, 3); s.bt[2][4] = RI(nx, 1); s.bt[2][5] = RI(nx, 2);
            }
        }
        auto &slot = rowc1[ibc & 3];
        if (!slot) {
            slot = std::make_unique<DeviceArray>();
            slot->upload(rc);
        }
        s.rowc = slot->p;
    } else if (which == 1) {
        if (d.ndr != 3 && d.ndr != 5) throw Fail(TLAB_EUNSUPPORTED, "first-derivative RHS must have 3 or 5 diagonals");
        s.c2 = (d.ndr == 5) ? RI(4, 5) : 0.0;  // r5_loc, fdm_matmul.f90:373
        if (!d.periodic) {
            const NeumannReduced nr(d, ibc, nb || ntp);
            if (d.ndr == 5) {  // MatMul_5d_antisym :382-391, :406-415
                if (nb) {
                    s.bb[1][1] = RB(2, 3); s.bb[1][2] = RB(2, 4); s.bb[1][3] = RB(2, 5);
                    s.bb[2][1] = RB(3, 2); s.bb[2][2] = RB(3, 3); s.bb[2][3] = RB(3, 4); s.bb[2][4] = RB(3, 5);
                } else {
                    penta_rows_bottom(s, r, nx);
                }
                if (ntp) {
                    s.bt[0][1] = RT(1, 1); s.bt[0][2] = RT(1, 2); s.bt[0][3] = RT(1, 3); s.bt[0][4] = RT(1, 4);
                    s.bt[1][2] = RT(2, 1); s.bt[1][3] = RT(2, 2); s.bt[1][4] = RT(2, 3);
                } else {
                    penta_rows_top(s, r, nx);
                }
            } else {  // MatMul_3d_antisym :177-186, :200-209 ; third row from each wall is an interior row
                s.bb[2][1] = -1.0; s.bb[2][3] = 1.0;
                s.bt[0][2] = -1.0; s.bt[0][4] = 1.0;
                if (nb) {
                    s.bb[1][1] = RB(2, 2); s.bb[1][2] = RB(2, 3);
                } else {
                    s.bb[0][0] = RI(1, 2); s.bb[0][1] = RI(1, 3); s.bb[0][2] = RI(1, 1);
                    s.bb[1][0] = RI(2, 1); s.bb[1][1] = RI(2, 2); s.bb[1][2] = RI(2, 3);
                }
                if (ntp) {
                    s.bt[1][3] = RT(1, 1); s.bt[1][4] = RT(1, 2);
                } else {
                    s.bt[1][3] = RI(nx - 1, 1); s.bt[1][4] = RI(nx - 1, 2); s.bt[1][5] = RI(nx - 1, 3);
                    s.bt[2][3] = RI(nx, 3); s.bt[2][4] = RI(nx, 1); s.bt[2][5] = RI(nx, 2);
                }
            }
        }
    } else if (d.direct) {   // MatMul_5d, fdm_matmul.f90:291-318 (no boundary data: FDM_Der2_Solve passes BCS_DD)
        if (d.ndr != 5 || d.periodic) throw Fail(TLAB_EUNSUPPORTED, "direct schemes: pentadiagonal RHS in a non-periodic direction only");
        penta_rows_bottom(s, r, nx);
        penta_rows_top(s, r, nx);
        if (!rowc2) {
            rowc2 = std::make_unique<DeviceArray>();
            rowc2->upload(penta_rowc(r, nx));
        }
        s.rowc = rowc2->p;
    } else {
        if (d.ndr == 7) {  // MatMul_7d_sym :578-580, :596-601, :628-635
            s.c0 = RI(4, 4); s.c2 = RI(4, 6); s.c3 = RI(4, 7);
            if (!d.periodic) {
                s.bb[0][0] = RI(1, 4); s.bb[0][1] = RI(1, 5); s.bb[0][2] = RI(1, 6); s.bb[0][3] = RI(1, 7); s.bb[0][4] = RI(1, 1);
                s.bb[1][0] = RI(2, 3); s.bb[1][1] = RI(2, 4); s.bb[1][2] = RI(2, 5); s.bb[1][3] = RI(2, 6); s.bb[1][4] = RI(2, 7);
                for (int k = 0; k < 6; ++k) s.bb[2][k] = RI(3, 2 + k);
                for (int k = 0; k < 6; ++k) s.bt[0][k] = RI(nx - 2, 1 + k);
                for (int k = 0; k < 5; ++k) s.bt[1][1 + k] = RI(nx - 1, 1 + k);
                s.bt[2][1] = RI(nx, 7); s.bt[2][2] = RI(nx, 1); s.bt[2][3] = RI(nx, 2); s.bt[2][4] = RI(nx, 3); s.bt[2][5] = RI(nx, 4);
            }
        } else if (d.ndr == 5) {  // MatMul_5d_sym :438-439, :450-453, :474-478
            s.c0 = RI(3, 3); s.c2 = RI(3, 5); s.c3 = 0.0;
            if (!d.periodic) {
                s.bb[0][0] = RI(1, 3); s.bb[0][1] = RI(1, 4); s.bb[0][2] = RI(1, 5); s.bb[0][3] = RI(1, 1);
                s.bb[1][0] = RI(2, 2); s.bb[1][1] = RI(2, 3); s.bb[1][2] = RI(2, 4); s.bb[1][3] = RI(2, 5);
                s.bb[2][0] = s.c2; s.bb[2][1] = 1.0; s.bb[2][2] = s.c0; s.bb[2][3] = 1.0; s.bb[2][4] = s.c2;
                s.bt[0][1] = s.c2; s.bt[0][2] = 1.0; s.bt[0][3] = s.c0; s.bt[0][4] = 1.0; s.bt[0][5] = s.c2;
                s.bt[1][2] = RI(nx - 1, 1); s.bt[1][3] = RI(nx - 1, 2); s.bt[1][4] = RI(nx - 1, 3); s.bt[1][5] = RI(nx - 1, 4);
                s.bt[2][2] = RI(nx, 5); s.bt[2][3] = RI(nx, 1); s.bt[2][4] = RI(nx, 2); s.bt[2][5] = RI(nx, 3);
            }
        } else {
            throw Fail(TLAB_EUNSUPPORTED, "second-derivative RHS must have 5 or 7 diagonals");
        }
    }
#undef RB
#undef RT
    return s;
}

SystemEntry &tlab_fdm_plan::system(int which, int ibc, int P) {
    if (which == 2 || t.der1.periodic) ibc = 0;
    auto key = std::make_tuple(which, ibc, P);
    auto it = systems.find(key);
    if (it != systems.end()) return *it->second;
    auto e = std::make_unique<SystemEntry>();
    TriDiag T = tridiag(which, ibc);
    build_chunked(T, P, e->host);
    const ChunkedTables &h = e->host;
    const int n = h.n, m = h.m;
    std::vector<double> rowtab((size_t)5 * n);
    std::copy(h.Lm.begin(), h.Lm.end(), rowtab.begin());
    std::copy(h.Dinv.begin(), h.Dinv.end(), rowtab.begin() + n);
    std::copy(h.Cm.begin(), h.Cm.end(), rowtab.begin() + 2 * n);
    std::copy(h.V.begin(), h.V.end(), rowtab.begin() + 3 * n);
    std::copy(h.W.begin(), h.W.end(), rowtab.begin() + 4 * n);
    e->rowtab.upload(rowtab);
    // lane-invariant: all chunks carry bitwise identical tables (circulant matrix with exactly uniform coefficients), so that the
    // kernel can use wave-uniform scalar loads.  NOTE: plans made by FDM_CreatePlan are NOT invariant: the reference derives the
    // "uniform" spacing numerically (fdm.f90:194-201) and its a,b,c wander by ~eps*n (2e-13 at n = 512).  Replacing them by chunk 0's
    // values would cost that much parity, so only exact equality qualifies; otherwise the per-lane tables are staged through LDS.
    auto close = [](double a, double b) { return a == b; };
    bool inv = h.periodic;
    for (int tab = 0; tab < 5 && inv; ++tab)
        for (int j = 1; j < P && inv; ++j)
            for (int p = 0; p < m; ++p)
                if (!close(rowtab[(size_t)tab * n + j * m + p], rowtab[(size_t)tab * n + p])) { inv = false; break; }
    if (P == 64) {      // wave-per-line kernel: parallel cyclic reduction over the 64 lanes
        if (h.pcr_steps != 6) throw Fail(TLAB_EINVAL, "internal: PCR schedule missing");
        std::vector<double> red((size_t)13 * 64);
        std::copy(h.pcr_k1.begin(), h.pcr_k1.end(), red.begin());
        std::copy(h.pcr_k2.begin(), h.pcr_k2.end(), red.begin() + 6 * 64);
        std::copy(h.pcr_dinv.begin(), h.pcr_dinv.end(), red.begin() + 12 * 64);
        for (int q = 0; q < 13 && inv; ++q)
            for (int j = 1; j < 64; ++j)
                if (!close(red[(size_t)q * 64 + j], red[(size_t)q * 64])) { inv = false; break; }
        e->red.upload(red);
    } else if (P == 128 || P == 256) {      // several waves per line: two-level reduction tables [21][P] (chunked.hpp), per-lane by construction
        if (h.tl_waves * 64 != P) throw Fail(TLAB_EINVAL, "two-level separator tables unavailable for this system");      // (inv: the row tables only)
        e->red.upload(h.tl);
    } else {
        e->red.upload(h.ginv);
    }
    e->lane_invariant = inv;
    {   // interior chunks equal to chunk 1 to the bit (the first and the last chunk carry the wall rows of a non-periodic system)
        bool ci = P >= 3;
        long long worst = 0;
        for (int tab = 0; tab < 5; ++tab)
            for (int j = 2; j < P - 1; ++j)
                for (int p = 0; p < m; ++p) {
                    const double u = rowtab[(size_t)tab * n + j * m + p], v = rowtab[(size_t)tab * n + m + p];
                    if (u != v) {
                        ci = false;
                        long long iu, iv;
                        std::memcpy(&iu, &u, 8);
                        std::memcpy(&iv, &v, 8);
                        worst = std::max(worst, std::llabs(iu - iv));
                    }
                }
        e->chunk_invariant = ci;
        bool band = P >= 8 && P <= 32 && (P & (P - 1)) == 0 && h.ginv.size() == (size_t)P * P;
        if (band) {
            double dmax = 0.0, omax = 0.0;
            std::vector<double> gb((size_t)P * 5, 0.0);
            for (int c = 0; c < P; ++c)
                for (int q = 0; q < P; ++q) {
                    int d = q - c;
                    if (d > P / 2) d -= P;
                    if (d < -P / 2) d += P;
                    const double v = h.ginv[(size_t)c * P + q];
                    if (d >= -2 && d <= 2) { gb[(size_t)c * 5 + d + 2] = v; if (d == 0) dmax = std::max(dmax, std::fabs(v)); }
                    else omax = std::max(omax, std::fabs(v));
                }
            band = omax <= 1e-30 * dmax;
            if (band) e->band.upload(gb);
        }
        e->band_ok = band;
        if (getenv("TLAB_DEBUG_TABLES")) fprintf(stderr, "system n=%d P=%d periodic=%d: lane_invariant %d chunk_invariant %d (largest interior difference %lld ulp) banded inverse %d\n", n, P, (int)h.periodic, (int)inv, (int)ci, worst, (int)band);
    }
    SystemEntry &ref = *e;
    systems[key] = std::move(e);
    return ref;
}

JacCorrDev tlab_fdm_plan::jaccorr() {
    if (!t.der2.need_1der) return JacCorrDev{nullptr};
    if (!jc) {
        jc = std::make_unique<DeviceArray>();
        const int n = t.n, ndr = t.der2.ndr;
        std::vector<double> j(t.der2.rhs.begin() + (size_t)n * ndr, t.der2.rhs.begin() + (size_t)n * (ndr + 3));
        jc->upload(j);
    }
    return JacCorrDev{jc->p};
}

// coefficients of BOUNDARY_BCS_NEUMANN_Y (boundary_bcs.f90:368-473): wall value = (u(2) cb0 + u(3) cb1) + u(4) cb2 + cb3 du(2), likewise at the top
void tlab_internal_neumann_y_coefficients(tlab_fdm_plan_t g, int ibc, int ny, double (&cb)[4], double (&ct)[4]) {
    const DerTables &d = g->t.der1;
    if (d.ndl != 3 || (d.ndr != 3 && d.ndr != 5)) throw Fail(TLAB_EUNSUPPORTED, "BOUNDARY_BCS_NEUMANN_Y: tridiagonal first-derivative schemes only");
    if (ny < 8) throw Fail(TLAB_EINVAL, "BOUNDARY_BCS_NEUMANN_Y: ny too small");
    const NeumannReduced nr(d, ibc, true);
    for (int q = 0; q < 4; ++q) cb[q] = ct[q] = 0.0;
    if (d.ndr == 5) {   // MatMul_5d_antisym, fdm_matmul.f90:384,410
        cb[0] = nr.RB(1, 4); cb[1] = nr.RB(1, 5); cb[2] = nr.RB(1, 1);
        ct[0] = nr.RT(3, 5); ct[1] = nr.RT(3, 1); ct[2] = nr.RT(3, 2);
    } else {            // MatMul_3d_antisym, fdm_matmul.f90:179,203
        cb[0] = nr.RB(1, 3); cb[1] = nr.RB(1, 1);
        ct[1] = nr.RT(2, 3); ct[2] = nr.RT(2, 1);
    }
    cb[3] = nr.lhs[0 + (size_t)ny * 2];          // lu(1, ip+idl+1): first row of the reduced LHS is not touched by TRIDFS
    ct[3] = nr.lhs[(ny - 1) + (size_t)ny * 0];   // lu(ny, ip+idl-1)
}
#undef RI

extern "C" {

int tlab_fdm_plan_create(tlab_fdm_plan_t *out, int n, const double *nodes, int periodic, int uniform, int scheme1,
                         int scheme2, double hyper_bc1_ext) {
    return catch_fail([&] {
        if (!out || !nodes || n < 1) throw Fail(TLAB_EINVAL, "tlab_fdm_plan_create: bad arguments");
        if (periodic && !uniform) throw Fail(TLAB_EINVAL, "grid must be uniform in a periodic direction (fdm.f90:117-120)");
        if (n > 1 && n < 8) throw Fail(TLAB_EINVAL, "tlab_fdm_plan_create: a direction needs 1 or >= 8 points");
        auto p = std::make_unique<tlab_fdm_plan>();
        try {
            fdm_create_plan(p->t, n, nodes, periodic != 0, uniform != 0, scheme1, scheme2, hyper_bc1_ext);
        } catch (const std::runtime_error &e) {
            throw Fail(TLAB_EUNSUPPORTED, e.what());
        }
        *out = p.release();
    }, TLAB_EINVAL);
}

int tlab_fdm_plan_create_from_arrays(tlab_fdm_plan_t *out, int n, int periodic, int need_1der, int ndl1, int ndr1,
                                     const double *lhs1, const double *rhs1, int ndl2, int ndr2, const double *lhs2,
                                     const double *rhs2) {
    return catch_fail([&] {
        if (!out || n < 8 || !lhs1 || !rhs1 || !lhs2 || !rhs2) throw Fail(TLAB_EINVAL, "tlab_fdm_plan_create_from_arrays: bad arguments");
        const bool penta = (ndl1 == 5 && ndr1 == 7);      // CompactJacobian6Penta first derivative (k_pentatile on lines of 64 .. 512 points in 32-row chunks, else k_penta1 in the reference's operation order)
        if ((ndl1 != 3 && !penta) || ndl2 != 3) throw Fail(TLAB_EUNSUPPORTED, "LHS: 3 diagonals (first derivative: or 5 with 7 RHS diagonals, CompactJacobian6Penta)");
        if ((!penta && ndr1 != 3 && ndr1 != 5) || (ndr2 != 5 && ndr2 != 7)) throw Fail(TLAB_EUNSUPPORTED, "unsupported number of RHS diagonals");
        auto p = std::make_unique<tlab_fdm_plan>();
        FdmTables &t = p->t;
        t.n = n; t.periodic = periodic != 0; t.uniform = !need_1der;
        for (DerTables *d : {&t.der1, &t.der2}) { d->n = n; d->periodic = t.periodic; d->lhs.assign((size_t)n * 5, 0.0); d->mwn.assign(n, 0.0); }
        t.der1.ndl = ndl1; t.der1.ndr = ndr1; t.der1.rhs_cols = 7; t.der1.rhs.assign((size_t)n * 7, 0.0);
        t.der2.ndl = 3; t.der2.ndr = ndr2; t.der2.rhs_cols = 12; t.der2.rhs.assign((size_t)n * 12, 0.0);
        t.der2.need_1der = need_1der != 0;
        std::copy(lhs1, lhs1 + (size_t)n * ndl1, t.der1.lhs.begin());
        std::copy(rhs1, rhs1 + (size_t)n * ndr1, t.der1.rhs.begin());
        std::copy(lhs2, lhs2 + (size_t)n * 3, t.der2.lhs.begin());
        std::copy(rhs2, rhs2 + (size_t)n * (ndr2 + 3), t.der2.rhs.begin());
        if (penta) {      // the kernel follows the reference's PENTADSS2 / PENTADPSS: factorize the host's lhs the reference's way (fdm_derivative.f90:78-119)
            t.der1.mode_fdm = FDM_COM6_JACOBIAN_PENTA;
            const int all[4] = {BCS_DD, BCS_ND, BCS_DN, BCS_NN};
            try { der1_factorize(t.der1, all, 4); } catch (const std::runtime_error &e) { throw Fail(TLAB_EUNSUPPORTED, e.what()); }
        }
        *out = p.release();
    }, TLAB_EINVAL);
}

// what else the Poisson solver and the monitors take from type(fdm_dt): modified wavenumbers (fdm_derivative.f90:193-211, periodic
// directions; opr_elliptic.f90:199-203), Jacobian (fdm.f90:194-224; time.f90:148-152), node positions
int tlab_fdm_plan_set_aux(tlab_fdm_plan_t p, const double *mwn1, const double *mwn2, const double *jac, const double *nodes) {
    return catch_fail([&] {
        if (!p) throw Fail(TLAB_EINVAL, "tlab_fdm_plan_set_aux: null plan");
        const int n = p->t.n;
        if (mwn1) p->t.der1.mwn.assign(mwn1, mwn1 + n);
        if (mwn2) p->t.der2.mwn.assign(mwn2, mwn2 + n);
        if (jac) p->t.jac.assign(jac, jac + (size_t)3 * n);
        if (nodes) p->t.nodes.assign(nodes, nodes + n);
    }, TLAB_EINVAL);
}

// mode_fdm of the two derivatives of a host-built plan (FDM_COM6_DIRECT = 16, FDM_COM4_DIRECT = 17 change how rhs is read)
int tlab_fdm_plan_set_scheme(tlab_fdm_plan_t p, int mode1, int mode2) {
    return flushed([&] {      // the recorded substep runs with the state of before
        if (!p) throw Fail(TLAB_EINVAL, "tlab_fdm_plan_set_scheme: null plan");
        auto direct = [](int m) { return m == FDM_COM6_DIRECT || m == FDM_COM4_DIRECT; };
        if (direct(mode1) && (p->t.periodic || p->t.der1.ndl != 3 || (p->t.der1.ndr != 3 && p->t.der1.ndr != 5)))
            throw Fail(TLAB_EINVAL, "direct first derivative: non-periodic direction, tridiagonal LHS, 3 or 5 RHS diagonals (FDM_C1N4_Direct / FDM_C1N6_Direct)");
        if (direct(mode2) && (p->t.periodic || p->t.der2.ndr != 5)) throw Fail(TLAB_EINVAL, "direct second derivative: non-periodic direction with 5 RHS diagonals");
        p->t.der1.mode_fdm = mode1; p->t.der2.mode_fdm = mode2;
        p->t.der1.direct = direct(mode1);
        p->t.der2.direct = direct(mode2);
        if (p->t.der2.direct) p->t.der2.need_1der = false;                 // fdm_derivative.f90:379,383
        p->systems.clear();
        p->rowc2.reset();
        for (auto &r : p->rowc1) r.reset();
    });
}

// [Staggering] StaggerHorizontalPressure (TLab_WorkFlow::stagger_on): what FDM_CreatePlan adds for a periodic direction (fdm.f90:236-248)
int tlab_fdm_plan_set_stagger(tlab_fdm_plan_t p, int mode) {
    return flushed([&] {      // the recorded substep runs with the state of before
        if (!p) throw Fail(TLAB_EINVAL, "tlab_fdm_plan_set_stagger: null plan");
        if (mode < 0 || mode > 2) throw Fail(TLAB_EINVAL, "tlab_fdm_plan_set_stagger: mode 0 off, 1 tables + interpolatory wavenumbers, 2 tables only");
        for (auto &f : p->interp)
            if (f) { tlab_filter_destroy(f); f = nullptr; }
        if (mode == 0) { p->t.stagger = false; return; }
        if (p->t.jac.size() < (size_t)p->t.n) throw Fail(TLAB_EINVAL, "tlab_fdm_plan_set_stagger: the plan has no Jacobian (tlab_fdm_plan_set_aux)");
        try { interpol_initialize(p->t, mode == 1); } catch (const std::runtime_error &e) { throw Fail(TLAB_EUNSUPPORTED, e.what()); }
    });
}

int tlab_fdm_plan_destroy(tlab_fdm_plan_t p) {
    (void)tlab_internal_deferred_flush();      // (a recorded substep may still need the plan)
    if (p)
        for (auto &f : p->interp)
            if (f) tlab_filter_destroy(f);
    delete p;
    return TLAB_OK;
}

int tlab_fdm_plan_info(tlab_fdm_plan_t p, int what) {
    if (!p) return TLAB_EINVAL;
    if (what == 8 || what == 9) {      // the x-line kernel's view of the plan (builds the chunked tables on first use: needs tlab_init)
        int r = 0;
        const int rc = catch_fail([&] {
            const int P = xline_chunks(p->t.n, p);
            if (what == 8 || P == 0) r = P;
            else r = (p->system(1, 0, P).lane_invariant && p->system(2, 0, P).lane_invariant) ? 1 : 0;
        }, TLAB_EINVAL);
        return rc == TLAB_OK ? r : TLAB_EINVAL;      // (whatever kept the tables from being built)
    }
    switch (what) {
    case 0: return p->t.n;
    case 1: return p->t.der1.ndl;
    case 2: return p->t.der1.ndr;
    case 3: return p->t.der2.ndl;
    case 4: return p->t.der2.ndr;
    case 5: return p->t.der2.need_1der ? 1 : 0;
    case 6: return p->t.periodic ? 1 : 0;
    case 7: return p->t.stagger ? 1 : 0;
    }
    return TLAB_EINVAL;
}

int tlab_fdm_plan_get(tlab_fdm_plan_t p, int which, double *buf, int nbuf) {
    if (!p || !buf) return TLAB_EINVAL;
    const FdmTables &t = p->t;
    const double *src = nullptr;
    size_t m = 0;
    switch (which) {
    case 1: src = t.der1.lhs.data(); m = t.der1.lhs.size(); break;
    case 2: src = t.der1.rhs.data(); m = t.der1.rhs.size(); break;
    case 3: src = t.der1.lu.data(); m = t.der1.lu.size(); break;
    case 4: src = t.der1.rhs_b; m = 32; break;
    case 5: src = t.der1.rhs_t; m = 35; break;
    case 6: src = t.der1.mwn.data(); m = t.der1.mwn.size(); break;
    case 7: src = t.der2.lhs.data(); m = t.der2.lhs.size(); break;
    case 8: src = t.der2.rhs.data(); m = t.der2.rhs.size(); break;
    case 9: src = t.der2.lu.data(); m = t.der2.lu.size(); break;
    case 10: src = t.der2.mwn.data(); m = t.der2.mwn.size(); break;
    case 11: src = t.jac.data(); m = t.jac.size(); break;
    case 12: src = t.lu0i.data(); m = t.lu0i.size(); break;
    case 13: src = t.lu1i.data(); m = t.lu1i.size(); break;
    default: return TLAB_EINVAL;
    }
    if ((size_t)nbuf < m) return TLAB_EINVAL;
    std::copy(src, src + m, buf);
    return (int)m;
}

int tlab_debug_host_chunked_solve(tlab_fdm_plan_t p, int which, int ibc, int chunks, double *f) {
    return catch_fail([&] {
        if (!p || !f || (which != 1 && which != 2)) throw Fail(TLAB_EINVAL, "bad arguments");
        TriDiag T = p->tridiag(which, (which == 2 || p->t.der1.periodic) ? 0 : ibc);
        ChunkedTables t;
        build_chunked(T, chunks, t);
        chunked_solve_host(t, f, chunks >= 64);
    }, TLAB_EINVAL);
}

}  // extern "C"
