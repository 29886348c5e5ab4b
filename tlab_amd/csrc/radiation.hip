// Radiation_Infrared_Y, TYPE_IR_GRAY_LIQUID (src/physics/radiation.f90:265-283) with IR_RTE1_OnlyLiquid (:401-444): the radiative heating of a
// gray liquid-water field, per (i, k) column of a physical-space field (nx, ny, nz), x fastest:
//     a = kappa l;   tau = FDM_Int1_Solve(fdm_Int0(BCS_MAX)) of a with tau(ny) = 0   (minus the optical depth from the top, fdm_integral.f90:219-314);
//     f = exp(tau);  source = a f flux_top                                           (downward only, flux_bottom = 0)
//                    source = a (f flux_top + f(1) / f flux_bottom)                  (both fluxes)
// and hs = hs + source (TLab_Sources_Scal, tlab_sources.f90:152-168).  The reference's operation order, no fused multiply-adds.
//
// The integral system is the pentadiagonal one of CompactJacobian6 with lambda = 0: the SAME coefficients for every column.  They are built once per
// plan on the host (int1_build_tables, the reduction of the opposite boundary and PENTADFS, where FDM_Int1_Initialize does them) and read through
// addresses that are uniform across the wave.  One thread per column, consecutive lanes on consecutive i: every row access of a wave is one
// contiguous line.  The Poisson solver's marching kernels (poisson_int1.hip) solve the same operator per spectral mode with per-mode factors.
//   sweep A, up the column:   the three-point right-hand side (MatMul_3d, BCS_BOTH) from a rolling window of a, the forward substitution of PENTADSS;
//                             the intermediate goes to scratch
//   sweep B, down the column: the back substitution, exp, and -- downward only -- the source into hs; row 1 (closed from rows 2..4) comes last
//   sweep C (both fluxes):    the upward term needs f(1), which exists only after sweep B: B stores f, C forms the source from it
// The row loads do not depend on the recurrences: they are issued U rows ahead.  Algorithmic traffic, downward only: l twice, the intermediate
// written and read, hs read and written -- six field passes; both fluxes: f written and read and l once more, nine.
// A 2-D run (nz = 1) has nx columns, a handful of waves: slow, correct.
#include <hip/hip_runtime.h>

#include <cmath>
#include <stdexcept>

#include "kernels.hpp"
#include "poisson_host.hpp"
#include "profile.hpp"

namespace tlab {

namespace {

constexpr int IR_U = 8;        // rows per block of loads: with one wave per 64 columns a 512^2 plane gives four waves per SIMD, so the bytes in flight that
                               // hide the memory latency must come from each wave -- 8 rows of 1 to 3 streams

template <bool UP>
__global__ void __launch_bounds__(64) k_infrared_y(const double *__restrict__ l, double *__restrict__ hs, double *__restrict__ yscr,
                                                   double *__restrict__ fscr, const double *__restrict__ tab, InfraredCoef C, double kappa,
                                                   double ft, double fb, int nx, int ny, long long ncol) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncol) return;
    const int n = ny;
    const long long base = (t % nx) + (long long)nx * ny * (t / nx);
    auto at = [&](int j) { return base + (long long)nx * j; };
    auto A = [&](int j) { return kappa * l[at(j)]; };
    const int nmax = n - 2;
    // ---- sweep A: right-hand side and forward substitution of rows 2 .. n-1 (0-based 1 .. n-2) ----
    const double res0 = A(0), resN = 0.0;      // result(:, 1) = f(:, 1) (fdm_integral.f90:244); tau(ny) = 0
    double fm = 0.0, fc = A(1), fp = A(2);
    const double bcs_b = res0 * C.rb[0][2] + fc * C.rb[0][3] + fp * C.rb[0][1];
    double y1 = 0.0, y2 = 0.0;
    for (int jb = 1; jb <= nmax; jb += IR_U) {
        double fq[IR_U], T[IR_U][4];
#pragma unroll
        for (int u = 0; u < IR_U; ++u) {
            const int jr = jb + u + 2;
            fq[u] = jr <= n - 1 ? A(jr) : 0.0;
            const int jc = jb + u <= nmax ? jb + u : nmax;
#pragma unroll
            for (int c = 0; c < 4; ++c) T[u][c] = tab[jc * 8 + c];
        }
#pragma unroll
        for (int u = 0; u < IR_U; ++u) {
            const int j = jb + u;
            if (j <= nmax) {
                double rhs;
                if (j == 1) rhs = res0 * C.rb[1][1] + fc * C.rb[1][2] + fp * C.rb[1][3];
                else if (j == 2) rhs = res0 * C.rb[2][0] + fm * C.rb[2][1] + fc * C.rb[2][2] + fp * C.rb[2][3];
                else if (j == n - 3) rhs = fm * C.rt[0][0] + fc * C.rt[0][1] + fp * C.rt[0][2] + resN * C.rt[0][3];
                else if (j == n - 2) rhs = fm * C.rt[1][0] + fc * C.rt[1][1] + resN * C.rt[1][2];
                else rhs = fm * T[u][0] + fc * T[u][1] + fp;
                const double y = rhs + y1 * T[u][3] + y2 * T[u][2];      // PENTADSS: f(n) + f(n-1) b(n) + f(n-2) a(n), factors negated by PENTADFS
                yscr[at(j)] = y;
                y2 = y1; y1 = y;
                fm = fc; fc = fp; fp = fq[u];
            }
        }
    }
    // ---- sweep B: back substitution, f = exp(tau); downward only: the source ----
    double x1 = 0.0, x2 = 0.0, xs1 = 0.0, xs2 = 0.0, xs3 = 0.0;
    {
        const double f = exp(resN);                 // row n
        if (UP) fscr[at(n - 1)] = f;
        else hs[at(n - 1)] = hs[at(n - 1)] + A(n - 1) * f * ft;
    }
    for (int jb = nmax; jb >= 1; jb -= IR_U) {
        double yb[IR_U], lb[IR_U], hb[IR_U], T[IR_U][3];
#pragma unroll
        for (int u = 0; u < IR_U; ++u) {
            const int jr = jb - u >= 1 ? jb - u : 1;
            yb[u] = yscr[at(jr)];
            if (!UP) { lb[u] = l[at(jr)]; hb[u] = hs[at(jr)]; }
#pragma unroll
            for (int c = 0; c < 3; ++c) T[u][c] = tab[jr * 8 + 4 + c];
        }
#pragma unroll
        for (int u = 0; u < IR_U; ++u) {
            const int j = jb - u;
            if (j >= 1) {
                const double x = (yb[u] + x1 * T[u][1] + x2 * T[u][2]) * T[u][0];
                x2 = x1; x1 = x;
                if (j == 1) xs1 = x;
                if (j == 2) xs2 = x;
                if (j == 3) xs3 = x;
                const double f = exp(x);
                if (UP) fscr[at(j)] = f;
                else hs[at(j)] = hb[u] + kappa * lb[u] * f * ft;
            }
        }
    }
    const double tau0 = bcs_b + C.l0[0] * xs1 + C.l0[1] * xs2 + C.l0[2] * xs3;      // row 1 from rows 2..4 (fdm_integral.f90:265-270)
    const double f0 = exp(tau0);
    if (!UP) {
        hs[at(0)] = hs[at(0)] + res0 * f0 * ft;
        return;
    }
    // ---- sweep C: a (f flux_top + f(1) / f flux_bottom) from the stored f; every value this thread wrote itself ----
    fscr[at(0)] = f0;
    for (int jb = 0; jb < n; jb += IR_U) {
        double fv[IR_U], lb[IR_U], hb[IR_U];
#pragma unroll
        for (int u = 0; u < IR_U; ++u) {
            const int jr = jb + u < n ? jb + u : n - 1;
            fv[u] = fscr[at(jr)]; lb[u] = l[at(jr)]; hb[u] = hs[at(jr)];
        }
#pragma unroll
        for (int u = 0; u < IR_U; ++u) {
            const int j = jb + u;
            if (j < n) hs[at(j)] = hb[u] + kappa * lb[u] * (fv[u] * ft + f0 / fv[u] * fb);
        }
    }
}

}  // namespace

// FDM_Int1_Initialize(x, g, lambda = 0, BCS_MAX) (fdm_integral.f90:58-87) on the host: the lambda-independent tables, the reduction of the bottom
// boundary (FDM_Bcs_Reduce(BCS_MIN), :209-210 -- the operations k_int1 does per mode, here once) and PENTADFS (utils/linear5.f90:30-71) of rows
// 2 .. n-1.  tab: [n][8] = rhs(j, 1), rhs(j, 2), a, b (forward factors), c, d, e (backward factors) as PENTADSS reads them, 0; entries PENTADSS never
// reads are zero, so that one expression serves every row.
void infrared_build_tables(const DerTables &g, std::vector<double> &tab, InfraredCoef &C) {
    Int1Tables T;
    int1_build_tables(g, 2, T);
    const int n = T.n;
    const double lam = 0.0;
    std::vector<double> L((size_t)n * 5);
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < 5; ++k) L[(size_t)j * 5 + k] = (T.L0[(size_t)j * 5 + k] + lam * T.L1[(size_t)j * 5 + k]) * T.L0[(size_t)n * 5 + j];
    double *l0 = &L[0], *l1 = &L[5], *l2 = &L[10];
    const double d = 1.0 / l0[2];
    for (int k = 0; k < 5; ++k) l0[k] = -l0[k] * d;
    l0[2] = 1.0;
    l1[2] = l1[2] + l1[1] * l0[3]; l1[3] = l1[3] + l1[1] * l0[4]; l1[4] = l1[4] + l1[1] * l0[0];
    l2[1] = l2[1] + l2[0] * l0[3]; l2[2] = l2[2] + l2[0] * l0[4]; l2[3] = l2[3] + l2[0] * l0[0];
    double rb[3][4];
    for (int c = 0; c < 3; ++c) {
        rb[0][c + 1] = T.R[0 * 3 + c] * d;
        rb[1][c + 1] = T.R[1 * 3 + c];
        rb[2][c + 1] = T.R[2 * 3 + c];
    }
    rb[0][0] = rb[1][0] = rb[2][0] = 0.0;
    rb[1][1] = rb[1][1] - l1[1] * rb[0][2]; rb[1][2] = rb[1][2] - l1[1] * rb[0][3]; rb[1][3] = rb[1][3] - l1[1] * rb[0][1];
    rb[2][0] = rb[2][0] - l2[0] * rb[0][2]; rb[2][1] = rb[2][1] - l2[0] * rb[0][3]; rb[2][2] = rb[2][2] - l2[0] * rb[0][1];
    for (int j = 0; j < 3; ++j)
        for (int c = 0; c < 4; ++c) C.rb[j][c] = rb[j][c];
    for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 4; ++c) C.rt[r][c] = T.rt[r][c];
    C.l0[0] = l0[3]; C.l0[1] = l0[4]; C.l0[2] = l0[0];
    // PENTADFS on rows 2 .. n-1: sub-row m <-> row j = m + 1 (0-based)
    const int nmax = n - 2;
    auto a = [&](int m) -> double & { return L[(size_t)(m + 1) * 5 + 0]; };
    auto b = [&](int m) -> double & { return L[(size_t)(m + 1) * 5 + 1]; };
    auto c = [&](int m) -> double & { return L[(size_t)(m + 1) * 5 + 2]; };
    auto dd = [&](int m) -> double & { return L[(size_t)(m + 1) * 5 + 3]; };
    auto e = [&](int m) -> double & { return L[(size_t)(m + 1) * 5 + 4]; };
    b(1) = b(1) / c(0);
    c(1) = c(1) - b(1) * dd(0);
    dd(1) = dd(1) - b(1) * e(0);
    for (int m = 2; m < nmax; ++m) {
        a(m) = a(m) / c(m - 2);
        b(m) = (b(m) - a(m) * dd(m - 2)) / c(m - 1);
        c(m) = c(m) - b(m) * dd(m - 1) - a(m) * e(m - 2);
        if (m < nmax - 1) dd(m) = dd(m) - b(m) * e(m - 1);
    }
    tab.assign((size_t)n * 8, 0.0);
    for (int j = 0; j < n; ++j) {
        tab[(size_t)j * 8 + 0] = T.R[(size_t)j * 3 + 0];
        tab[(size_t)j * 8 + 1] = T.R[(size_t)j * 3 + 1];
    }
    for (int m = 0; m < nmax; ++m) {
        double *r = &tab[(size_t)(m + 1) * 8];
        r[2] = m >= 2 ? -a(m) : 0.0;
        r[3] = m >= 1 ? -b(m) : 0.0;
        r[4] = 1.0 / c(m);
        r[5] = m <= nmax - 2 ? -dd(m) : 0.0;
        r[6] = m <= nmax - 3 ? -e(m) : 0.0;
    }
    for (double v : tab)
        if (!std::isfinite(v)) throw std::runtime_error("infrared: the first-order integral system of this y plan does not factorize");
}

hipError_t launch_infrared_y(const double *l, double *hs, double *scr1, double *scr2, const double *tab, const InfraredCoef &C, double kappa,
                             double flux_top, double flux_bottom, int nx, int ny, int nz, hipStream_t st) {
    if (nx < 1 || ny < 8 || nz < 1 || !l || !hs || !scr1 || !tab) return hipErrorInvalidValue;
    const bool up = std::fabs(flux_bottom) > 0.0;
    if (up && !scr2) return hipErrorInvalidValue;
    const long long ncol = (long long)nx * nz, n = ncol * ny;
    const long long grid = (ncol + 63) / 64;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    ProfScope ps("k_infrared_y", st, 8.0 * (double)n * (up ? 9 : 6));
    if (up) hipLaunchKernelGGL((k_infrared_y<true>), dim3((unsigned)grid), dim3(64), 0, st, l, hs, scr1, scr2, tab, C, kappa, flux_top, flux_bottom, nx, ny, ncol);
    else hipLaunchKernelGGL((k_infrared_y<false>), dim3((unsigned)grid), dim3(64), 0, st, l, hs, scr1, scr2, tab, C, kappa, flux_top, flux_bottom, nx, ny, ncol);
    return hipGetLastError();
}

}  // namespace tlab
