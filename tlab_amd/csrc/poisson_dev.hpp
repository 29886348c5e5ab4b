// Device code of the Poisson kernel files (poisson_int1.hip, poisson_ode.hip, poisson_direct.hip) that is not one file's own: the non-fused arithmetic and
// the matrix rows of the first-order integral systems (marching and chunked solvers), the PENTADFS step and the scan over the chunks (chunked solvers).
#pragma once
#include "poisson_plan.hpp"

namespace tlab {

// Non-fused arithmetic for everything that builds or factorizes the per-mode matrices: the reference's CPU build rounds every product and
// every sum, and the solution of these boundary-value problems is sensitive to the last bit of the matrix and of its LU factors (a table
// of the form L0 + lambda L1 with the row normalisation folded in, evaluated and eliminated with fused multiply-adds, sits 7-10x above the
// floor that one ulp of forcing noise sets: 4e-12 in p and 2e-11 in dp/dy on the 512-point lines of a projection step, measured).
__device__ __forceinline__ double nf_madd(double a, double b, double c) {   // a + b * c, two roundings
#pragma clang fp contract(off)
    const double t = b * c;
    return a + t;
}
__device__ __forceinline__ double nf_msub(double a, double b, double c) {   // a - b * c, two roundings
#pragma clang fp contract(off)
    const double t = b * c;
    return a - t;
}

// row j of lhs = (B + lambda A) * normalisation, in the operation order of FDM_Int1_CreateSystem (fdm_integral.f90:150-201); the
// normalisation of row j is stored behind the [n][5] block of L0
__device__ __forceinline__ void lhs_row(const Int1Dev &T, int j, double lam, double (&r)[5]) {
    const double sj = T.L0[5 * T.n + j];
#pragma unroll
    for (int k = 0; k < 5; ++k) r[k] = nf_madd(T.L0[j * 5 + k], lam, T.L1[j * 5 + k]) * sj;
}

template <class TT>
__device__ __forceinline__ void lhs_row_t(const TT &T, int j, double lam, double (&r)[5]) {
    const double sj = T.L0[(unsigned)(5 * T.n + j)];
#pragma unroll
    for (int k = 0; k < 5; ++k) r[k] = nf_madd(T.L0[(unsigned)(j * 5 + k)], lam, T.L1[(unsigned)(j * 5 + k)]) * sj;
}

// one PENTADFS step (linear5.f90:30-71) for row j; st = (c1, d1, e1, c2, d2, e2) of rows j-1, j-2
__device__ __forceinline__ void ode_factor_step(int j, const double (&r)[5], double (&st)[6], double &am, double &bm, double &cinv, double &nd,
                                                double &ne) {
    double cm = r[2], dm = r[3];
    const double em = r[4];
    am = 0.0; bm = 0.0;
    if (j == 2) {
        bm = r[1] / st[0];
        cm = nf_msub(r[2], bm, st[1]);
        dm = nf_msub(r[3], bm, st[2]);
    } else if (j >= 3) {
        am = r[0] / st[3];
        bm = nf_msub(r[1], am, st[4]) / st[0];
        cm = nf_msub(nf_msub(r[2], bm, st[1]), am, st[5]);
        dm = nf_msub(r[3], bm, st[2]);
    }
    cinv = 1.0 / cm; nd = -dm; ne = -em;
    st[3] = st[0]; st[4] = st[1]; st[5] = st[2];
    st[0] = cm; st[1] = dm; st[2] = em;
}

// Inflow of every chunk from the chunks before it (DIR = +1: c-1, c-2, ... ; DIR = -1: c+1, c+2, ...), i.e. the exclusive prefix of the
// affine maps in -> Phi in + e of the chunks, composed in the direction of the sweep.  Lanes hold (mode m, chunk c) with m fastest, so a
// wave owns 64/NM consecutive chunks of NM modes: Hillis-Steele with lane shuffles inside the wave, the wave totals through LDS.
//   phi = {p00, p01, p10, p11}, e[l] = {e1, e2} per line; returns in[l] = {in1, in2}.     s_w: [nwaves][4 + 2 NL][NM] doubles
template <int NM, int DIR, int NL = 2>
__device__ __forceinline__ void ode_chain(double (&phi)[4], double (&e)[NL][2], int c, int C, int m, double *s_w, double (&in)[NL][2]) {
    constexpr int SW = 4 + 2 * NL;                     // doubles per wave total: phi, then (e1, e2) of every line
    constexpr int CPW = 64 / NM;                       // chunks per wave
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int cw = lane / NM;                          // chunk index inside the wave
    // position along the sweep inside the wave: DIR = +1 -> cw, DIR = -1 -> reversed
#pragma unroll
    for (int d = 1; d < CPW; d <<= 1) {
        double q[4], f[NL][2];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = (DIR > 0) ? __shfl_up(phi[k], d * NM) : __shfl_down(phi[k], d * NM);
#pragma unroll
        for (int l = 0; l < NL; ++l)
#pragma unroll
            for (int k = 0; k < 2; ++k) f[l][k] = (DIR > 0) ? __shfl_up(e[l][k], d * NM) : __shfl_down(e[l][k], d * NM);
        const bool has = (DIR > 0) ? (cw >= d) : (cw + d < CPW && c + d < C);
        if (has) {      // (phi, e) <- (phi * q, phi * f + e): the partner's chunks come first in the sweep
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double n1 = phi[0] * f[l][0] + phi[1] * f[l][1] + e[l][0];
                const double n2 = phi[2] * f[l][0] + phi[3] * f[l][1] + e[l][1];
                e[l][0] = n1; e[l][1] = n2;
            }
            const double r00 = phi[0] * q[0] + phi[1] * q[2], r01 = phi[0] * q[1] + phi[1] * q[3];
            const double r10 = phi[2] * q[0] + phi[3] * q[2], r11 = phi[2] * q[1] + phi[3] * q[3];
            phi[0] = r00; phi[1] = r01; phi[2] = r10; phi[3] = r11;
        }
    }
    // wave totals = the inclusive value of the last chunk of the wave along the sweep
    const bool last_in_wave = (DIR > 0) ? (cw == CPW - 1 || c == C - 1) : (cw == 0);
    if (last_in_wave) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_w[(w * SW + k) * NM + m] = phi[k];
#pragma unroll
        for (int l = 0; l < NL; ++l) { s_w[(w * SW + 4 + 2 * l) * NM + m] = e[l][0]; s_w[(w * SW + 5 + 2 * l) * NM + m] = e[l][1]; }
    }
    __syncthreads();
    // what enters my wave: the waves before it along the sweep, composed in order
    const int nw = (blockDim.x + 63) >> 6;
    double pe[NL][2];
#pragma unroll
    for (int l = 0; l < NL; ++l) pe[l][0] = pe[l][1] = 0.0;
    if (DIR > 0) {
        for (int v = 0; v < w; ++v) {
            const double a0 = s_w[(v * SW + 0) * NM + m], a1 = s_w[(v * SW + 1) * NM + m], a2 = s_w[(v * SW + 2) * NM + m], a3 = s_w[(v * SW + 3) * NM + m];
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double n1 = a0 * pe[l][0] + a1 * pe[l][1] + s_w[(v * SW + 4 + 2 * l) * NM + m];
                const double n2 = a2 * pe[l][0] + a3 * pe[l][1] + s_w[(v * SW + 5 + 2 * l) * NM + m];
                pe[l][0] = n1; pe[l][1] = n2;
            }
        }
    } else {
        for (int v = nw - 1; v > w; --v) {
            const double a0 = s_w[(v * SW + 0) * NM + m], a1 = s_w[(v * SW + 1) * NM + m], a2 = s_w[(v * SW + 2) * NM + m], a3 = s_w[(v * SW + 3) * NM + m];
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double n1 = a0 * pe[l][0] + a1 * pe[l][1] + s_w[(v * SW + 4 + 2 * l) * NM + m];
                const double n2 = a2 * pe[l][0] + a3 * pe[l][1] + s_w[(v * SW + 5 + 2 * l) * NM + m];
                pe[l][0] = n1; pe[l][1] = n2;
            }
        }
    }
    // inclusive value of my chunk over the whole line, then the previous chunk's along the sweep = my inflow
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const double f1 = phi[0] * pe[l][0] + phi[1] * pe[l][1] + e[l][0];
        const double f2 = phi[2] * pe[l][0] + phi[3] * pe[l][1] + e[l][1];
        const double g1 = (DIR > 0) ? __shfl_up(f1, NM) : __shfl_down(f1, NM);
        const double g2 = (DIR > 0) ? __shfl_up(f2, NM) : __shfl_down(f2, NM);
        const bool first_in_wave = (DIR > 0) ? (cw == 0) : (cw == CPW - 1 || c == C - 1);
        in[l][0] = first_in_wave ? pe[l][0] : g1;
        in[l][1] = first_in_wave ? pe[l][1] : g2;
    }
    __syncthreads();      // s_w is reused by the next scan
}

}  // namespace tlab
