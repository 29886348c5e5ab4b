// The line algorithms of the streaming filter kernels (filter_stream.hip), apart from how a line's points reach the thread: G gives
//   g.u(i)                       the stored value of point i (1-based) of the thread's line, read before the first sweep
//   g.sweep<S, LAG>(step)        one sweep, S = +1 upwards from point 1, -1 downwards from point n: step(i, x) is called for i = 1 - LAG .. n
//                                (S = -1: n + LAG .. 1) with x = the stored value of point i + S LAG where that is a point of the line (anything
//                                otherwise) and returns the new value of point i (ignored where i is no point of the line)
// The arithmetic is k_filter1d's (filter.hip:56-164): the same expression trees in the same order, FP contraction off, true fp64 divisions, the
// recursions in the reference's order.  The end rows of the non-periodic forms and the points a periodic form needs from the far end are taken into
// registers before the first sweep and handed out in the order the sweep meets them (plain moves: a choice by index would put them in scratch).
// Plain C++ apart from the function attributes, so that a host program can run the same text on one line.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define TLAB_FLT_HD __host__ __device__ __forceinline__
#else
#define TLAB_FLT_HD inline
#endif

namespace tlab {

constexpr int FLT_COMPACT = 1, FLT_6E = 2, FLT_4E = 3, FLT_CUTOFF = 9;       // opr_filter.f90:56-65
constexpr int FBCS_ZERO = 6;                                                   // filters/flt_base.f90:11

// c: coeffs, column-major [ncols][n] (f%coeffs)
template <int TYPE, bool PER, class G>
TLAB_FLT_HD void filter_line(G &g, const double *c, int n, int bcsmin, int bcsmax) {
#pragma clang fp contract(off)
#define U(i) g.u(i)
#define C(i, k) c[((i)-1) + (size_t)n * ((k)-1)]
    if constexpr (TYPE == FLT_COMPACT || TYPE == FLT_4E) {
        // ---- FLT_C4_RHS (flt_compact.f90:225-296) / FLT_E4 (flt_explitic.f90:17-62): the end rows, or the wrap of the periodic form ----
        double e1 = 0.0, e2 = 0.0, en1 = 0.0, en = 0.0, w1 = 0.0, w2 = 0.0;
        double um2 = 0.0, um1 = 0.0, u0 = 0.0, up1 = 0.0;      // u(i-2) .. u(i+1)
        if constexpr (PER) {
            u0 = U(n - 1); up1 = U(n); w1 = U(1); w2 = U(2);
        } else {
            const double u1 = U(1), u2 = U(2), u3 = U(3), u4 = U(4), u5 = U(5), v0 = U(n), v1 = U(n - 1), v2 = U(n - 2), v3 = U(n - 3), v4 = U(n - 4);
            if constexpr (TYPE == FLT_COMPACT) {
                e1 = C(1, 1) * u1 + C(1, 2) * u2 + C(1, 3) * u3 + C(1, 4) * u4 + C(1, 5) * u5;
                e2 = C(2, 1) * u1 + C(2, 2) * u2 + C(2, 3) * u3 + C(2, 4) * u4 + C(2, 5) * u5;
                en1 = C(n - 1, 5) * v0 + C(n - 1, 4) * v1 + C(n - 1, 3) * v2 + C(n - 1, 2) * v3 + C(n - 1, 1) * v4;
                en = C(n, 5) * v0 + C(n, 4) * v1 + C(n, 3) * v2 + C(n, 2) * v3 + C(n, 1) * v4;
                if (bcsmin == FBCS_ZERO) e1 = u1;
                if (bcsmax == FBCS_ZERO) en = v0;
            } else {
                e1 = u1;
                e2 = C(2, 2) * u1 + C(2, 3) * u2 + C(2, 4) * u3 + C(2, 5) * u4 + C(2, 1) * u5;
                en1 = C(n - 1, 1) * v3 + C(n - 1, 2) * v2 + C(n - 1, 3) * v1 + C(n - 1, 4) * v0 + C(n - 1, 5) * v4;
                en = v0;
            }
        }
        double fp = 0.0, wrk = 0.0, rhsn = 0.0;
        // the right-hand side, and with it the forward sweep of TRIDSS (linear3.f90:56-150) / TRIDPSS (:321-442) with coeffs(:, 6:10)
        g.template sweep<1, 2>([&](int i, double x) __attribute__((always_inline)) {
            double e = x, v = 0.0;
            if constexpr (PER) {
                if (i + 2 > n) { e = w1; w1 = w2; }      // u(n+1) = u(1), u(n+2) = u(2)
            }
            if (i >= 1) {
                double rhs;
                if (!PER && i <= 2) { rhs = e1; e1 = e2; }      // the end rows, in the order the sweep meets them
                else if (!PER && i >= n - 1) { rhs = en1; en1 = en; }
                else rhs = C(i, 1) * um2 + C(i, 2) * um1 + C(i, 3) * u0 + C(i, 4) * up1 + C(i, 5) * e;
                if constexpr (TYPE == FLT_4E) {
                    v = rhs;
                } else if constexpr (PER) {
                    if (i == n) {
                        rhsn = rhs; v = rhs;
                    } else {
                        v = i == 1 ? rhs * C(1, 7) : rhs * C(i, 7) + C(i, 6) * fp;
                        wrk = wrk + C(i, 9) * v;
                        fp = v;
                    }
                } else {
                    v = i == 1 ? rhs : rhs + C(i, 6) * fp;
                    fp = v;
                }
            }
            um2 = um1; um1 = u0; u0 = up1; up1 = e;
            return v;
        });
        if constexpr (TYPE == FLT_COMPACT) {
            double fn = 0.0, flast = 0.0, fn1 = 0.0;
            if constexpr (PER) {
                flast = (rhsn - wrk) * C(n, 7);
                fn1 = C(n - 1, 10) * flast + fp;
            }
            g.template sweep<-1, 0>([&](int i, double x) __attribute__((always_inline)) {
                double v;
                if constexpr (PER) {
                    if (i == n) v = flast;
                    else if (i == n - 1) v = fn1;
                    else v = x + C(i, 8) * fn + C(i, 10) * flast;
                } else {
                    if (i == n) v = x * C(n, 7);
                    else v = (x + C(i, 8) * fn) * C(i, 7);
                }
                fn = v;
                return v;
            });
        }
    } else if constexpr (TYPE == FLT_6E) {      // FLT_E6 flt_explitic.f90:179-362
        const double b0 = 11.0 / 16.0, b1 = 15.0 / 64.0, b2 = -3.0 / 32.0, b3 = 1.0 / 64.0;
        const double bb[7] = {1.0 / 16.0, 3.0 / 4.0, 3.0 / 8.0, -1.0 / 4.0, 1.0 / 16.0, 0.0, 0.0};
        const double bc[7] = {-1.0 / 32.0, 5.0 / 32.0, 11.0 / 16.0, 5.0 / 16.0, -5.0 / 32.0, 1.0 / 32.0, 0.0};
        double e1 = 0.0, e2 = 0.0, e3 = 0.0, en2 = 0.0, en1 = 0.0, en = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0;
        double m3 = 0.0, m2 = 0.0, m1 = 0.0, c0 = 0.0, p1 = 0.0, p2 = 0.0;      // u(i-3) .. u(i+2)
        if constexpr (PER) {
            c0 = U(n - 2); p1 = U(n - 1); p2 = U(n); w1 = U(1); w2 = U(2); w3 = U(3);
        } else {
            e1 = U(1);
            if (bcsmin == 1) {
                e2 = bb[0] * U(1) + bb[1] * U(2) + bb[2] * U(3) + bb[3] * U(4) + bb[4] * U(5) + bb[5] * U(6) + bb[6] * U(7);
                e3 = bc[0] * U(1) + bc[1] * U(2) + bc[2] * U(3) + bc[3] * U(4) + bc[4] * U(5) + bc[5] * U(6) + bc[6] * U(7);
            } else {
                e2 = U(2); e3 = U(3);
            }
            en = U(n);
            if (bcsmax == 1) {
                en1 = bb[0] * U(n) + bb[1] * U(n - 1) + bb[2] * U(n - 2) + bb[3] * U(n - 3) + bb[4] * U(n - 4) + bb[5] * U(n - 5) + bb[6] * U(n - 6);
                en2 = bc[0] * U(n) + bc[1] * U(n - 1) + bc[2] * U(n - 2) + bc[3] * U(n - 3) + bc[4] * U(n - 4) + bc[5] * U(n - 5) + bc[6] * U(n - 6);
            } else {
                en2 = U(n - 2); en1 = U(n - 1);
            }
        }
        g.template sweep<1, 3>([&](int i, double x) __attribute__((always_inline)) {
            double e = x, v = 0.0;
            if constexpr (PER) {
                if (i + 3 > n) { e = w1; w1 = w2; w2 = w3; }
            }
            if (i >= 1) {
                if (!PER && i <= 3) { v = e1; e1 = e2; e2 = e3; }
                else if (!PER && i >= n - 2) { v = en2; en2 = en1; en1 = en; }
                else v = b3 * (m3 + e) + b2 * (m2 + p2) + b1 * (m1 + p1) + b0 * c0;
            }
            m3 = m2; m2 = m1; m1 = c0; c0 = p1; p1 = p2; p2 = e;
            return v;
        });
    } else {      // FLT_CUTOFF
        const double BD2 = 0.66059, CD2 = 0.1666774, DD2 = 0.679925e-3, CA = 0.9891856;      // flt_compact.f90:11-16
        double e1 = 0.0, e2 = 0.0, e3 = 0.0, en2 = 0.0, en1 = 0.0, en = 0.0, wl0 = 0.0, wl1 = 0.0, wl2 = 0.0;
        double p3 = 0.0, p2 = 0.0, p1 = 0.0, c0 = 0.0, m1 = 0.0, m2 = 0.0;      // u(i+3) .. u(i-2)
        if constexpr (PER) {      // FLT_C4P_CUTOFF_RHS :327-349
            c0 = U(3); m1 = U(2); m2 = U(1); wl0 = U(n); wl1 = U(n - 1); wl2 = U(n - 2);
        } else {                  // FLT_C4_CUTOFF_RHS :351-375
            e1 = (15.0 * U(1) + 4.0 * U(2) - 6.0 * U(3) + 4.0 * U(4) - U(5)) / 16.0;
            e2 = (12.0 * U(2) + U(1) + 6.0 * U(3) - 4.0 * U(4) + U(5)) / 16.0;
            e3 = (10.0 * U(3) - U(1) + 4.0 * U(2) + 4.0 * U(4) - U(5)) / 16.0;
            en2 = (10.0 * U(n - 2) - U(n) + 4.0 * U(n - 1) + 4.0 * U(n - 3) - U(n - 4)) / 16.0;
            en1 = (12.0 * U(n - 1) + U(n) + 6.0 * U(n - 2) - 4.0 * U(n - 3) + U(n - 4)) / 16.0;
            en = (15.0 * U(n) + 4.0 * U(n - 1) - 6.0 * U(n - 2) + 4.0 * U(n - 3) - U(n - 4)) / 16.0;
        }
        // PENTADSS2 (linear5.f90:207-268) with (a .. e) = coeffs(:, 1:5); periodic: PENTADPSS (:352-411) with f, g = coeffs(:, 6:7)
        const double *A = c, *Bv = c + (size_t)n, *Cc = c + (size_t)2 * n, *D = c + (size_t)3 * n, *E = c + (size_t)4 * n;
        double f1 = 0.0, f2 = 0.0;      // F(i+1), F(i+2)
        g.template sweep<-1, 3>([&](int i, double x) __attribute__((always_inline)) {
            double e = x, v = 0.0;
            if constexpr (PER) {
                if (i - 3 < 1) { e = wl0; wl0 = wl1; wl1 = wl2; }      // u(0) = u(n), u(-1) = u(n-1), u(-2) = u(n-2)
            }
            if (i <= n) {
                double rhs;
                if (!PER && i >= n - 2) { rhs = en; en = en1; en1 = en2; }      // downwards: n, n-1, n-2 ... 3, 2, 1
                else if (!PER && i <= 3) { rhs = e3; e3 = e2; e2 = e1; }
                else rhs = BD2 * (p1 + m1) + CD2 * (p2 + m2) + DD2 * (p3 + e) + CA * c0;
                if (i == n) v = rhs;
                else if (i == n - 1) v = rhs - f1 * D[n - 2];
                else v = rhs - f1 * D[i - 1] - f2 * E[i - 1];
                f2 = f1; f1 = v;
            }
            p3 = p2; p2 = p1; p1 = c0; c0 = m1; m1 = m2; m2 = e;
            return v;
        });
        double g1 = 0.0, g2 = 0.0, F1 = 0.0, F2 = 0.0;      // F(i-1), F(i-2); F(1), F(2)
        g.template sweep<1, 0>([&](int i, double x) __attribute__((always_inline)) {
            double v;
            if (i == 1) { v = x / Cc[0]; F1 = v; }
            else if (i == 2) { v = (x - g1 * Bv[1]) / Cc[1]; F2 = v; }
            else v = (x - g1 * Bv[i - 1] - g2 * A[i - 1]) / Cc[i - 1];
            g2 = g1; g1 = v;
            return v;
        });
        if constexpr (PER) {
            const double *Fv = c + (size_t)5 * n, *Gv = c + (size_t)6 * n;
            const double m1_ = E[n - 1] * Fv[0] + A[0] * Fv[n - 2] + Bv[0] * Fv[n - 1] + 1.0;
            const double m2_ = E[n - 1] * Gv[0] + A[0] * Gv[n - 2] + Bv[0] * Gv[n - 1];
            const double m3_ = D[n - 1] * Fv[0] + E[n - 1] * Fv[1] + A[0] * Fv[n - 1];
            const double m4_ = D[n - 1] * Gv[0] + E[n - 1] * Gv[1] + A[0] * Gv[n - 1] + 1.0;
            const double di = 1 / (m1_ * m4_ - m2_ * m3_);
            const double d11 = di * (m4_ * E[n - 1] - m2_ * D[n - 1]), d12 = di * (m4_ * Bv[0] - m2_ * A[0]), d13 = di * m4_ * A[0], d14 = di * m2_ * E[n - 1];
            const double d21 = di * (m1_ * D[n - 1] - m3_ * E[n - 1]), d22 = di * (m1_ * A[0] - m3_ * Bv[0]), d23 = di * m3_ * A[0], d24 = di * m1_ * E[n - 1];
            const double Fn = g1, Fn1 = g2;
            const double dummy1 = d11 * F1 + d12 * Fn + d13 * Fn1 - d14 * F2;
            const double dummy2 = d21 * F1 + d22 * Fn - d23 * Fn1 + d24 * F2;
            g.template sweep<-1, 0>([&](int i, double x) __attribute__((always_inline)) { return x - dummy1 * Fv[i - 1] - dummy2 * Gv[i - 1]; });
        }
    }
#undef U
#undef C
}

}  // namespace tlab
