// The chunked per-mode solver of the Poisson solver (poisson.hip): k_ode_nn, k_ode_sing, their plan-time tables and launchers.
#include "poisson_dev.hpp"

namespace tlab {

// ================================================================================================
// k_ode_nn : OPR_ODE2_Factorize_NN for a group of modes with the y-line cut into chunks of 8 rows that live in registers.
//
// k_int1 marches one thread per mode along the whole line: 512 dependent steps, twice, with every intermediate of the
// pentadiagonal solve (5 doubles per row) written to and read back from HBM -- latency-bound on small slabs, traffic-bound
// (22 GB per Poisson solve at 512^3) on large ones.  Here a workgroup owns NM modes x all rows, thread (m, c) owns rows
// [8c, 8c+8) of mode m:
//   * the LU factors of its rows are regenerated from a CHECKPOINT of the PENTADFS recurrence (pivots of the two rows before
//     the chunk, 6 doubles per chunk and mode, written once at plan creation by k_ode_checkpoint): the same numbers the serial
//     elimination produces (the system B + lambda A is not diagonally dominant -- partitioned eliminations with their own
//     local pivots lose up to 6 digits for small lambda, measured -- so the serial pivot sequence is kept);
//   * forward and backward substitution are two-term linear recurrences: every chunk computes its particular end values and its
//     2x2 transfer matrix, a parallel scan over the chunks (lane shuffles inside a wave, wave totals through LDS) gives every
//     chunk its inflow, and the chunk repeats its 8 rows with it;
//   * v0, u0 stay in registers until the three constants of the 3x3 constraint system are known, and the superposition with the
//     homogeneous solutions of the mode (5 arrays computed at plan creation, opr_odes.f90:350-367) is the epilogue of the same kernel.
//     (Running the pair of solves a second time with the final boundary values instead of reading them was measured: the kernel is
//     bound by dependent fp64 latency at 8 waves per CU, not by HBM, and the second pass doubled its time.)
// HBM traffic per mode and row: f^ 16 B, p^ + dp^/dy 32 B, homogeneous solutions 40 B, checkpoints 12 B; no scratch.
// ================================================================================================
struct OdeArgs {
    OdeSys T1, T2;               // BCS_MIN (+lambda) and BCS_MAX (-lambda) tables
    const double *lam;           // [nm]
    const unsigned char *skip;   // [nm] singular modes: computed elsewhere
    const double *chk1, *chk2;   // [C][6][nm] PENTADFS state before the first row of each chunk
    const double *cst;           // [9][nm] LU of the constraint matrix (k_nn_constants)
    const double *hom;           // [5][n][nm] homogeneous solutions v1, em, u1, sp, ep (build_homogeneous)
    const int *band;             // [2][nm] (may be NULL): rows (jb, jt) exclusive where all five homogeneous solutions of the mode are negligible
    int pair_xcd;                // see k_ode_nn
    const double *f_hat;
    double *p_hat, *dp_hat;
    double fscale;
    int n, nxh, ny, C;
    long long nm;
};

// boundary rows of the system of one mode (the prologue of k_int1)
struct OdeRows {
    double l0[5], l1[5], l2[5], lN[5], lN1[5], lN2[5], rb[3][4], rt[3][4];
};

// lhs_row_t and R(j, 1:3) of row j from the packed table (OdeSys::pk): the same numbers by the same operations
__device__ __forceinline__ void ode_row_pk(const OdeSys &T, int j, double lam, double (&r)[5], double (&R)[3]) {
    const double2 *pk = reinterpret_cast<const double2 *>(T.pk) + (unsigned)(j * 8);
    const double2 q0 = pk[0], q1 = pk[1], q2 = pk[2], q3 = pk[3], q4 = pk[4], q5 = pk[5], q6 = pk[6];
    const double sj = q5.x;
    r[0] = nf_madd(q0.x, lam, q2.y) * sj; r[1] = nf_madd(q0.y, lam, q3.x) * sj; r[2] = nf_madd(q1.x, lam, q3.y) * sj;
    r[3] = nf_madd(q1.y, lam, q4.x) * sj; r[4] = nf_madd(q2.x, lam, q4.y) * sj;
    R[0] = q5.y; R[1] = q6.x; R[2] = q6.y;
}

// (the two ends are independent of each other: a caller that stores one end only -- ode_solve -- pays for that end only)
template <int BC>
__device__ __forceinline__ void ode_boundary_rows(const OdeSys &T, double lam, OdeRows &k) {
    const int n = T.n;
    double R0[3], R1[3], R2[3], RN[3], RN1[3], RN2[3];
    ode_row_pk(T, 0, lam, k.l0, R0); ode_row_pk(T, 1, lam, k.l1, R1); ode_row_pk(T, 2, lam, k.l2, R2);
    ode_row_pk(T, n - 1, lam, k.lN, RN); ode_row_pk(T, n - 2, lam, k.lN1, RN1); ode_row_pk(T, n - 3, lam, k.lN2, RN2);
    if (BC == 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) k.rb[j][c] = T.bt[j * 4 + c];
        const double d = 1.0 / k.lN[2];
#pragma unroll
        for (int q = 0; q < 5; ++q) k.lN[q] = -k.lN[q] * d;
        k.lN[2] = 1.0;
        k.lN1[0] = nf_madd(k.lN1[0], k.lN1[3], k.lN[4]); k.lN1[1] = nf_madd(k.lN1[1], k.lN1[3], k.lN[0]); k.lN1[2] = nf_madd(k.lN1[2], k.lN1[3], k.lN[1]);
        k.lN2[1] = nf_madd(k.lN2[1], k.lN2[4], k.lN[4]); k.lN2[2] = nf_madd(k.lN2[2], k.lN2[4], k.lN[0]); k.lN2[3] = nf_madd(k.lN2[3], k.lN2[4], k.lN[1]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            k.rt[2][c] = RN[c] * d;
            k.rt[1][c] = RN1[c];
            k.rt[0][c] = RN2[c];
        }
        k.rt[0][3] = k.rt[1][3] = k.rt[2][3] = 0.0;
        k.rt[1][0] = nf_msub(k.rt[1][0], k.lN1[3], k.rt[2][2]); k.rt[1][1] = nf_msub(k.rt[1][1], k.lN1[3], k.rt[2][0]); k.rt[1][2] = nf_msub(k.rt[1][2], k.lN1[3], k.rt[2][1]);
        k.rt[0][1] = nf_msub(k.rt[0][1], k.lN2[4], k.rt[2][2]); k.rt[0][2] = nf_msub(k.rt[0][2], k.lN2[4], k.rt[2][0]); k.rt[0][3] = nf_msub(k.rt[0][3], k.lN2[4], k.rt[2][1]);
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) k.rt[j][c] = T.bt[j * 4 + c];
        const double d = 1.0 / k.l0[2];
#pragma unroll
        for (int q = 0; q < 5; ++q) k.l0[q] = -k.l0[q] * d;
        k.l0[2] = 1.0;
        k.l1[2] = nf_madd(k.l1[2], k.l1[1], k.l0[3]); k.l1[3] = nf_madd(k.l1[3], k.l1[1], k.l0[4]); k.l1[4] = nf_madd(k.l1[4], k.l1[1], k.l0[0]);
        k.l2[1] = nf_madd(k.l2[1], k.l2[0], k.l0[3]); k.l2[2] = nf_madd(k.l2[2], k.l2[0], k.l0[4]); k.l2[3] = nf_madd(k.l2[3], k.l2[0], k.l0[0]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            k.rb[0][c + 1] = R0[c] * d;
            k.rb[1][c + 1] = R1[c];
            k.rb[2][c + 1] = R2[c];
        }
        k.rb[0][0] = k.rb[1][0] = k.rb[2][0] = 0.0;
        k.rb[1][1] = nf_msub(k.rb[1][1], k.l1[1], k.rb[0][2]); k.rb[1][2] = nf_msub(k.rb[1][2], k.l1[1], k.rb[0][3]); k.rb[1][3] = nf_msub(k.rb[1][3], k.l1[1], k.rb[0][1]);
        k.rb[2][0] = nf_msub(k.rb[2][0], k.l2[0], k.rb[0][2]); k.rb[2][1] = nf_msub(k.rb[2][1], k.l2[0], k.rb[0][3]); k.rb[2][2] = nf_msub(k.rb[2][2], k.l2[0], k.rb[0][1]);
    }
}

// matrix row j of the reduced system of one mode
__device__ __forceinline__ void ode_row(const OdeSys &T, const OdeRows &k, int j, double lam, double (&r)[5]) {
    const int n = T.n;
    if (j == 1) { for (int q = 0; q < 5; ++q) r[q] = k.l1[q]; }
    else if (j == 2) { for (int q = 0; q < 5; ++q) r[q] = k.l2[q]; }
    else if (j == n - 3) { for (int q = 0; q < 5; ++q) r[q] = k.lN2[q]; }
    else if (j == n - 2) { for (int q = 0; q < 5; ++q) r[q] = k.lN1[q]; }
    else lhs_row_t(T, j, lam, r);
}

// The boundary rows depend on the mode only: one thread per mode computes them into LDS (54 doubles per mode), the two chunks that
// touch a boundary read what they need from there, and no thread keeps them in registers.  Layout: [field][NM], fields:
//   0-4 l0, 5-9 l1, 10-14 l2, 15-19 lN, 20-24 lN1, 25-29 lN2, 30-41 rb[3][4], 42-53 rt[3][4]
constexpr int OK_L0 = 0, OK_L1 = 5, OK_L2 = 10, OK_LN = 15, OK_LN1 = 20, OK_LN2 = 25, OK_RB = 30, OK_RT = 42, OK_FS = 54, OK_CST = 58, OK_BAND = 67, OK_SIZE = 70;      // OK_FS: one f row per line, parked by the chunk that needs it after the solve; OK_CST, OK_BAND: the mode's constants and band (k_ode_nn: fetched at the start)
template <int NM, int END = 0>      // END = 1 / 2: the rows of the bottom / the top only
__device__ __forceinline__ void ode_rows_to_lds(const OdeRows &k, double *s_k, int m) {
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        if (END != 2) { s_k[(OK_L0 + q) * NM + m] = k.l0[q]; s_k[(OK_L1 + q) * NM + m] = k.l1[q]; s_k[(OK_L2 + q) * NM + m] = k.l2[q]; }
        if (END != 1) { s_k[(OK_LN + q) * NM + m] = k.lN[q]; s_k[(OK_LN1 + q) * NM + m] = k.lN1[q]; s_k[(OK_LN2 + q) * NM + m] = k.lN2[q]; }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (END != 2) s_k[(OK_RB + j * 4 + c) * NM + m] = k.rb[j][c];
            if (END != 1) s_k[(OK_RT + j * 4 + c) * NM + m] = k.rt[j][c];
        }
}
template <int NM>
__device__ __forceinline__ void ode_row_lds(const OdeSys &T, const double *s_k, int m, int j, double lam, double (&r)[5]) {
    const int n = T.n;
    const int off = (j == 1) ? OK_L1 : (j == 2) ? OK_L2 : (j == n - 3) ? OK_LN2 : (j == n - 2) ? OK_LN1 : -1;
    if (off >= 0) {
#pragma unroll
        for (int q = 0; q < 5; ++q) r[q] = s_k[(off + q) * NM + m];
    } else {
        lhs_row_t(T, j, lam, r);
    }
}

// checkpoints of the factor recurrence: state before rows 8, 16, ... (chunk 0 starts from zeros)
template <int BC>
// Layout of everything k_ode_nn reads per mode: blocked by the NM modes of a workgroup, [block][...][NM], so that a workgroup's reads are
// one contiguous stream (mode-minor [..][nm] rows would be 64-B pieces of 128-B lines at NM = 8: measured 2x over-fetch).
__global__ void __launch_bounds__(256) k_ode_checkpoint(OdeSys T, const double *__restrict__ lamv, double lam_sign, double *__restrict__ chk,
                                                        long long nm, int NM, int C, int om) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nm) return;
    const int n = T.n;
    const double lam = lam_sign * lamv[t];
    OdeRows k;
    ode_boundary_rows<BC>(T, lam, k);
    double st[6] = {0, 0, 0, 0, 0, 0};
    for (int j = 1; j <= n - 2; ++j) {
        if ((j % om) == 0) {
            const int c = j / om;
#pragma unroll
            for (int q = 0; q < 6; ++q) chk[(((t / NM) * C + c) * 6 + q) * NM + (t % NM)] = st[q];
        }
        double r[5], am, bm, cinv, nd, ne;
        ode_row(T, k, j, lam, r);
        ode_factor_step(j, r, st, am, bm, cinv, nd, ne);
    }
}

// Per mode: the rows between which all five homogeneous solutions are below 1e-40 of their own maximum, found from the middle of the line
// outwards (band[t] = last significant row of the lower half, band[nm + t] = first one of the upper half).  hom: [5][n][nm].
__global__ void __launch_bounds__(256) k_ode_hom_band(const double *__restrict__ hom, int n, long long nm, int *__restrict__ band, double rel) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nm) return;
    double thr[5];
    for (int a = 0; a < 5; ++a) {
        double mx = 0.0;
        for (int j = 0; j < n; ++j) mx = fmax(mx, fabs(hom[((size_t)a * n + j) * nm + t]));
        thr[a] = mx * rel;
    }
    const int mid = n / 2;
    int jb = -1, jt = n;
    for (int j = 0; j < n; ++j) {
        bool sig = false;
        for (int a = 0; a < 5; ++a) sig = sig || !(fabs(hom[((size_t)a * n + j) * nm + t]) <= thr[a]);      // NaN counts as significant
        if (sig && j < mid) jb = j;
        if (sig && j >= mid && j < jt) jt = j;
    }
    band[t] = jb;
    band[nm + t] = jt;
}

// src[a][j][nm] -> dst[blk][a][j][NM]
// (the five solutions of a mode and row side by side, [blk][j][NM][6] with three 16-B loads per row in k_ode_nn, was measured: 3 % slower)
__global__ void __launch_bounds__(256) k_ode_block_layout(const double *__restrict__ src, double *__restrict__ dst, int A, int n, long long nm, int NM) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)A * n * nm) return;
    const long long t = i % nm, aj = i / nm;          // aj = a * n + j
    dst[((t / NM) * A * n + aj) * NM + (t % NM)] = src[i];
}

// One FDM_Int1_Solve of BOTH lines (Re, Im) for the rows of this thread.
//   fl[p][l], p = 0..9: f rows j0-1 .. j0+8 (the halo rows are only read where they exist)
//   res0 / resN: the boundary values as MatMul_3d sees them (fdm_integral.f90:240-245)
//   x[p][l]: solution rows j0..j0+7 (boundary rows included after the reconstruction)
//   ext[l]: derivative at the given end: BC == 1 at the bottom (valid in chunk 0), BC == 2 at the top (valid in the last chunk)
// LDS: s_w [nwaves][4 + 2 NL][NM] (scan), s_k [OK_SIZE][NM] (boundary rows), s_fac [threads][3 OM + 1] (backward factors)
// OM rows per thread (8, or 4 with the line cut into twice as many chunks), NL lines sharing the factors (2 = Re, Im of one mode; 4 = of two
// modes with the same lambda)
template <int BC, int NM, int OM = 8, int NL = 2>
__device__ __forceinline__ void ode_solve(const OdeSys &T, double lam, const double *__restrict__ chk, int nm, int t, int c, int C, int m,
                                          const double (&fl)[OM + 2][NL], const double (&res0)[NL], const double (&resN)[NL],
                                          double (&x)[OM][NL], double (&ext)[NL], double *s_w, double *s_k, double *s_fac) {
    static_assert(OM == 4 || OM == 8, "rows per thread");
    const int n = T.n, j0 = c * OM;
    // the boundary rows of the mode: the bottom ones by the thread of chunk 1, the top ones by that of chunk 2 (every other thread of the workgroup waits
    // for them at the barrier below: two threads side by side halve that wait; what a thread does not store is not computed)
    if (C >= 3) {
        if (c == 1) {
            OdeRows k;
            ode_boundary_rows<BC>(T, lam, k);
            ode_rows_to_lds<NM, 1>(k, s_k, m);
        }
        if (c == 2) {
            OdeRows k;
            ode_boundary_rows<BC>(T, lam, k);
            ode_rows_to_lds<NM, 2>(k, s_k, m);
        }
    } else if (c == 1) {       // C >= 2; chunk 1 never touches a boundary row itself
        OdeRows k;
        ode_boundary_rows<BC>(T, lam, k);
        ode_rows_to_lds<NM>(k, s_k, m);
    }
    __syncthreads();
#define KK(field, q) s_k[((field) + (q)) * NM + m]
#define KRB(j, cc) s_k[(OK_RB + (j) * 4 + (cc)) * NM + m]
#define KRT(j, cc) s_k[(OK_RT + (j) * 4 + (cc)) * NM + m]
    // ---- factors of my rows, from the checkpoint ----
    double st[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) st[q] = (c == 0) ? 0.0 : chk[(unsigned)((((t / NM) * C + c) * 6 + q) * NM + m)];      // 32-bit indices: checked on the host
    double am[OM], bm[OM];             // forward multipliers in registers; the backward factors (1/c, -d, -e) wait in LDS
    double *my_fac = s_fac + threadIdx.x * (3 * OM + 1);      // thread-major with an odd stride: constant offsets, no bank conflicts
#define FAC(p, q) my_fac[(p) * 3 + (q)]
    double (&rhs)[OM][NL] = x;          // right-hand side -> y -> x in place
    double bcs_b[NL], bcs_t[NL];
    static_assert(NL <= OK_CST - OK_FS, "parking rows (the mode constants start at OK_CST)");
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        // the only use of fl after the right-hand side: f(n-2) of the last chunk (BCS_MAX) / f(1) of the first one (BCS_MIN), for du -- parked in
        // LDS by the thread that reads it back (8 VGPRs less through both sweeps)
        if (BC == 2 && c == C - 1) s_k[(OK_FS + l) * NM + m] = fl[OM - 1][l];
        if (BC == 1 && c == 0) s_k[(OK_FS + l) * NM + m] = fl[2][l];
        bcs_b[l] = bcs_t[l] = 0.0;
    }
    // The special rows sit at fixed positions of the first and the last chunk (requires n = 8 C): row 0 / n-1 are not part of the
    // system, rows 1, 2 / n-3, n-2 carry the reduced boundary closures.  Conditions are written on the unrolled p so that they fold away
    // everywhere else, and the special cases are selections of coefficients, not branches.
    const bool lo = (c == 0), hi = (c == C - 1);
#pragma unroll
    for (int p = 0; p < OM; ++p) {
        const int j = j0 + p;
        const bool off = (p == 0 && lo) || (p == OM - 1 && hi);         // boundary rows
        double r[5], c0, c1, c2 = 1.0, cb = 0.0, ct = 0.0;     // rhs = c0 f(j-1) + c1 f(j) + c2 f(j+1) + cb res0 + ct resN
        {   // lhs_row_t and R(j, 1:2) from the packed row (same numbers, same operations)
            const double2 *pk = reinterpret_cast<const double2 *>(T.pk) + (unsigned)(j * 8);
            const double2 q0 = pk[0], q1 = pk[1], q2 = pk[2], q3 = pk[3], q4 = pk[4], q5 = pk[5], q6 = pk[6];
            const double sj = q5.x;
            r[0] = nf_madd(q0.x, lam, q2.y) * sj; r[1] = nf_madd(q0.y, lam, q3.x) * sj; r[2] = nf_madd(q1.x, lam, q3.y) * sj;
            r[3] = nf_madd(q1.y, lam, q4.x) * sj; r[4] = nf_madd(q2.x, lam, q4.y) * sj;
            c0 = q5.y; c1 = q6.x;
        }
        if (p == 1 && lo) {
#pragma unroll
            for (int q = 0; q < 5; ++q) r[q] = KK(OK_L1, q);
            c0 = 0.0; c1 = KRB(1, 2); c2 = KRB(1, 3); cb = KRB(1, 1);
        }
        if (p == 2 && lo) {
#pragma unroll
            for (int q = 0; q < 5; ++q) r[q] = KK(OK_L2, q);
            c0 = KRB(2, 1); c1 = KRB(2, 2); c2 = KRB(2, 3); cb = KRB(2, 0);
        }
        if (p == OM - 3 && hi) {
#pragma unroll
            for (int q = 0; q < 5; ++q) r[q] = KK(OK_LN2, q);
            c0 = KRT(0, 0); c1 = KRT(0, 1); c2 = KRT(0, 2); ct = KRT(0, 3);
        }
        if (p == OM - 2 && hi) {
#pragma unroll
            for (int q = 0; q < 5; ++q) r[q] = KK(OK_LN1, q);
            c0 = KRT(1, 0); c1 = KRT(1, 1); c2 = 0.0; ct = KRT(1, 2);
        }
        // PENTADFS step (linear5.f90:30-71): row 1 starts the elimination, row 2 has one sub-diagonal, the rest two
        double a_m = 0.0, b_m = 0.0, cm = r[2], dm = r[3];
        const double em = r[4];
        if (p >= 3 || !lo) {
            a_m = r[0] / st[3];
            b_m = nf_msub(r[1], a_m, st[4]) / st[0];
            cm = nf_msub(nf_msub(r[2], b_m, st[1]), a_m, st[5]);
            dm = nf_msub(r[3], b_m, st[2]);
        } else if (p == 2) {
            b_m = r[1] / st[0];
            cm = nf_msub(r[2], b_m, st[1]);
            dm = nf_msub(r[3], b_m, st[2]);
        }
        if (off) { a_m = 0.0; b_m = 0.0; }
        am[p] = a_m; bm[p] = b_m;
        FAC(p, 0) = off ? 1.0 : 1.0 / cm; FAC(p, 1) = off ? 0.0 : -dm; FAC(p, 2) = off ? 0.0 : -em;
        if (!off) {
            st[3] = st[0]; st[4] = st[1]; st[5] = st[2];
            st[0] = cm; st[1] = dm; st[2] = em;
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const double fm = fl[p][l], fc = fl[p + 1][l], fp = fl[p + 2][l];
            double v = fm * c0 + fc * c1 + fp * c2;
            if ((p == 1 || p == 2) && lo) v = res0[l] * cb + v;          // (order of the reference: boundary term first, fdm_matmul.f90:93-94)
            if ((p == OM - 3 || p == OM - 2) && hi) v = v + resN[l] * ct;
            rhs[p][l] = off ? 0.0 : v;
            if (p == 1 && lo) bcs_b[l] = res0[l] * KRB(0, 2) + fc * KRB(0, 3) + fp * KRB(0, 1);
            if (p == OM - 2 && hi) bcs_t[l] = fm * KRT(2, 2) + fc * KRT(2, 0) + resN[l] * KRT(2, 1);
        }
        if (p & 1) __builtin_amdgcn_sched_barrier(0);      // table loads of two rows in flight, not of all eight (96 doubles)
    }
    // ---- forward substitution: particular end values + transfer matrix, scan, repeat with the inflow ----
    double inflow[NL][2];
    {
        double y1[NL], y2[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) y1[l] = y2[l] = 0.0;
        double h1a = 1.0, h2a = 0.0, h1b = 0.0, h2b = 1.0;     // responses to unit inflows (y[j0-1], y[j0-2]) = (1,0), (0,1)
#pragma unroll
        for (int p = 0; p < OM; ++p) {
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double y = rhs[p][l] - y1[l] * bm[p] - y2[l] * am[p];
                y2[l] = y1[l]; y1[l] = y;
            }
            const double ha = -h1a * bm[p] - h2a * am[p]; h2a = h1a; h1a = ha;
            const double hb = -h1b * bm[p] - h2b * am[p]; h2b = h1b; h1b = hb;
        }
        // out = (y[j0+7], y[j0+6]) = Phi (in1, in2) + end
        double phi[4] = {h1a, h1b, h2a, h2b}, ee[NL][2];
#pragma unroll
        for (int l = 0; l < NL; ++l) { ee[l][0] = y1[l]; ee[l][1] = y2[l]; }
        ode_chain<NM, +1, NL>(phi, ee, c, C, m, s_w, inflow);
    }
    double (&y)[OM][NL] = x;
    {
        double y1[NL], y2[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) { y1[l] = inflow[l][0]; y2[l] = inflow[l][1]; }
#pragma unroll
        for (int p = 0; p < OM; ++p)
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double v = rhs[p][l] - y1[l] * bm[p] - y2[l] * am[p];
                y[p][l] = v; y2[l] = y1[l]; y1[l] = v;
            }
    }
    __syncthreads();
    // ---- backward substitution, same scheme downwards: in = (x[j0+8], x[j0+9]), out = (x[j0], x[j0+1]) ----
    {
        double x1[NL], x2[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) x1[l] = x2[l] = 0.0;
        double h1a = 1.0, h2a = 0.0, h1b = 0.0, h2b = 1.0;
#pragma unroll
        for (int p = OM - 1; p >= 0; --p) {
            const double cinv_p = FAC(p, 0), nd_p = FAC(p, 1), ne_p = FAC(p, 2);
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double v = (y[p][l] + x1[l] * nd_p + x2[l] * ne_p) * cinv_p;
                x2[l] = x1[l]; x1[l] = v;
            }
            const double ha = (h1a * nd_p + h2a * ne_p) * cinv_p; h2a = h1a; h1a = ha;
            const double hb = (h1b * nd_p + h2b * ne_p) * cinv_p; h2b = h1b; h1b = hb;
        }
        double phi[4] = {h1a, h1b, h2a, h2b}, ee[NL][2];
#pragma unroll
        for (int l = 0; l < NL; ++l) { ee[l][0] = x1[l]; ee[l][1] = x2[l]; }
        ode_chain<NM, -1, NL>(phi, ee, c, C, m, s_w, inflow);
    }
    {
        double x1[NL], x2[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) { x1[l] = inflow[l][0]; x2[l] = inflow[l][1]; }
#pragma unroll
        for (int p = OM - 1; p >= 0; --p) {
            const double cinv_p = FAC(p, 0), nd_p = FAC(p, 1), ne_p = FAC(p, 2);
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double v = (y[p][l] + x1[l] * nd_p + x2[l] * ne_p) * cinv_p;
                x[p][l] = v; x2[l] = x1[l]; x1[l] = v;
            }
        }
    }
    __syncthreads();
    // ---- boundary value at the free end, derivative at the given end (fdm_integral.f90:265-311) ----
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        ext[l] = 0.0;
        if (BC == 2) {
            if (c == 0) x[0][l] = bcs_b[l] + KK(OK_L0, 3) * x[1][l] + KK(OK_L0, 4) * x[2][l] + KK(OK_L0, 0) * x[3][l];
            if (c == C - 1) {
                x[OM - 1][l] = resN[l];
                // rows n-2, n-3, n-4 = p 6, 5, 4 ; f[n-2] = fl[7]
                ext[l] = KK(OK_LN, 2) * resN[l] + KK(OK_LN, 1) * x[OM - 2][l] + KK(OK_LN, 0) * x[OM - 3][l] + KK(OK_LN, 4) * x[OM - 4][l] +
                         T.R[(n - 1) * 3 + 0] * s_k[(OK_FS + l) * NM + m];
            }
        } else {
            if (c == C - 1) x[OM - 1][l] = bcs_t[l] + KK(OK_LN, 1) * x[OM - 2][l] + KK(OK_LN, 0) * x[OM - 3][l] + KK(OK_LN, 4) * x[OM - 4][l];
            if (c == 0) {
                x[0][l] = res0[l];
                ext[l] = KK(OK_L0, 2) * res0[l] + KK(OK_L0, 3) * x[1][l] + KK(OK_L0, 4) * x[2][l] + KK(OK_L0, 0) * x[3][l] + T.R[0 * 3 + 2] * s_k[(OK_FS + l) * NM + m];
            }
        }
    }
    __syncthreads();       // s_k is rewritten by the next solve
#undef KK
#undef KRB
#undef KRT
#undef FAC
}

// DD: OPR_ODE2_Factorize_DD (opr_odes.f90:391-478) instead of _NN: the same two solves with the top value of u GIVEN (bcs(:,2)), two constants
// instead of three (a.cst = [5][nm]: aa, bb, 1 / (aa sp(1) - bb u1(1)), sp(1), u1(1) from k_dd_constants), no e^(+) term in the superposition.
// NL = 4: MIRROR PAIRS.  lambda(kx, kz) = lambda(kx, nz - kz) to the bit (the modified wavenumbers of +-omega, fdm_derivative.f90:198-204), so the
// pivots, the checkpoints, the constants and the homogeneous solutions of the two modes are the same numbers: one thread carries the four lines
// (Re, Im of both modes) through one regeneration of the factors and one read of the tables.  Workgroup = NM values of kx x one kz <= nz/2 (and its
// mirror plane); kz = 0 and nz/2 are their own partners (the second store is dropped).  The plan checks the symmetry of lambda and of the skip
// flags on the host before it picks this form.  OMR = 4 rows per thread there: the same 16 values per thread as 8 rows x 2 lines.
template <int NM, bool DD = false, int OMR = 8, int NL = 2>
__global__ void __launch_bounds__(512) k_ode_nn(OdeArgs a) {
    constexpr int NQ = NL / 2;                                                                    // modes per thread
    extern __shared__ double lds[];
    const int C = a.C, n = a.n;
    const int m = threadIdx.x % NM, c = threadIdx.x / NM;
    double *s_w = lds, *s_x = lds + 8 * (4 + 2 * NL) * NM;                                       // s_w: [8 waves][4 + 2 NL][NM]; s_x: [C][NL lines][2][NM]
    double *s_sc = s_x + (size_t)C * 2 * NL * NM;                                                // [5][NL][NM]
    double *s_k = s_sc + 5 * NL * NM;                                                            // [OK_SIZE][NM]
    double *s_fac = s_k + OK_SIZE * NM;                                                          // [threads][3 OMR + 1]
#define SC(q, l) s_sc[((q) * NL + (l)) * NM + m]
    // 32-bit index arithmetic throughout (the host checks that every array has < 2^31 elements): 64-bit address pairs for the ~50
    // distinct rows this thread touches would otherwise be precomputed and kept in registers
    const int nm = (int)a.nm;
    // NM = 4: a workgroup's row of f^ / p^ / dp^ is 64 B, half a 128-B line.  Workgroups go round-robin over the 8 XCDs (each with its own L2), so
    // the neighbour that owns the other half would sit on another XCD and the line would cross the fabric twice (PMC: 9.3 GB per launch, 8.3 with the pairing, against
    // 6.7 algorithmic).  Pair them: of every 16 consecutive workgroups, XCD x gets the adjacent blocks 2x and 2x + 1.
    unsigned blk = blockIdx.x;
    // pair_xcd = G (16, 32, 64, ...): of every G consecutive workgroups XCD x gets the G/8 ADJACENT blocks x G/8 .. -- the rows of f^ / p^ / dp^ are
    // nxh = nx/2 + 1 complex numbers long, an ODD number of 16-B elements, so the 128-B lines are not aligned with any fixed window of kx: a line is
    // shared by neighbouring blocks in every row but one of eight, and only neighbours on the same XCD (same L2) share it for free.  Counters at 512^3
    // (profiles/r06/poisson_requests.txt): G = 16 read 4.06 GB per launch in 128-B requests where f^ + checkpoints + homogeneous solutions are 1.75.
    if (a.pair_xcd >= 16) {
        const unsigned G = (unsigned)a.pair_xcd;
        if ((blk | (G - 1u)) < gridDim.x) blk = (blk & ~(G - 1u)) + (blk & 7u) * (G >> 3) + ((blk & (G - 1u)) >> 3);
    }
    int t = (int)blk * NM + m;                        // the mode whose tables are read (NL = 4: kz <= nz/2, so the pair index is the mode index)
    const int nlive = (NL == 4) ? a.nxh * (nm / a.nxh / 2 + 1) : nm;
    const bool live = t < nlive;
    if (!live) t = nlive - 1;
    const double lam = a.lam[t];
    unsigned fidx0[NQ];
    bool store[NQ];                                   // modes solved elsewhere (singular, low) are left alone, each of a pair on its own
    fidx0[0] = (unsigned)((t % a.nxh) + a.nxh * a.ny * (t / a.nxh));
    store[0] = live && !a.skip[t];
    if (NL == 4) {
        const int nz = nm / a.nxh, kz = t / a.nxh, kz2 = (nz - kz) % nz;
        fidx0[NQ - 1] = (unsigned)((t % a.nxh) + a.nxh * a.ny * kz2);
        store[NQ - 1] = live && kz2 != kz && !a.skip[(t % a.nxh) + a.nxh * kz2];      // kz = 0, nz/2: their own mirror, stored once
    }
    const int j0 = c * OMR;
    const double2 *F = reinterpret_cast<const double2 *>(a.f_hat);
    double2 *P = reinterpret_cast<double2 *>(a.p_hat), *D = reinterpret_cast<double2 *>(a.dp_hat);
    // the constants of the mode and its band of negligible homogeneous solutions are needed after the two solves, by every chunk: one thread per mode
    // fetches them now (their trip to HBM was exposed in front of the epilogue, and 64 chunks issued the same nine loads)
    if (c == (C > 3 ? 3 : 0)) {
#pragma unroll
        for (int k = 0; k < (DD ? 5 : 9); ++k) s_k[(OK_CST + k) * NM + m] = a.cst[(unsigned)(k * nm + t)];
        s_k[(OK_BAND + 0) * NM + m] = a.band != nullptr ? (double)a.band[t] : (double)n;
        s_k[(OK_BAND + 1) * NM + m] = a.band != nullptr ? (double)a.band[nm + t] : 0.0;
    }

    double u[OMR][NL], ext[NL];
    double v_1[NL], u_n[NL], fn[NL];      // (the Neumann data bb = SC(0, l), bt = SC(1, l) stay in LDS until the constants are formed)
#pragma unroll
    for (int l = 0; l < NL; ++l) v_1[l] = u_n[l] = fn[l] = 0.0;
    double vh[OMR + 2][NL];      // rows j0-1 .. j0+OMR of the u-solve's right-hand side v; vh[1..OMR] is where the v-solve puts v
    {
        // ---- f rows j0-1 .. j0+OMR (normalised).  f(n) itself is never read by the solves: the callers' f(n) = 0 enters as resN (opr_odes.f90:303)
        double fl[OMR + 2][NL];
#pragma unroll
        for (int p = 0; p < OMR + 2; ++p) {
            const int j = j0 - 1 + p;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                double2 w = make_double2(0.0, 0.0);
                if (j >= 0 && j <= n - 1) w = F[fidx0[q] + (unsigned)(j * a.nxh)];
                fl[p][2 * q] = w.x * a.fscale; fl[p][2 * q + 1] = w.y * a.fscale;
            }
        }
        // Neumann data travel in the boundary rows of the forcing (opr_elliptic.f90:310-311)
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (c == 0) SC(0, l) = fl[1][l];
            if (c == C - 1) SC(1, l) = fl[OMR][l];
        }
        // ---- v0' + lambda v0 = f, v0(1) = 0 ; f(n) = 0 ----
        ode_solve<1, NM, OMR, NL>(a.T1, lam, a.chk1, nm, t, c, C, m, fl, v_1, fn, reinterpret_cast<double (&)[OMR][NL]>(vh[1]), ext, s_w, s_k, s_fac);
    }
    // halo rows of v0 for the right-hand side of the u-solve
#pragma unroll
    for (int l = 0; l < NL; ++l) { s_x[((c * NL + l) * 2 + 0) * NM + m] = vh[1][l]; s_x[((c * NL + l) * 2 + 1) * NM + m] = vh[OMR][l]; }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        vh[0][l] = (c > 0) ? s_x[(((c - 1) * NL + l) * 2 + 1) * NM + m] : 0.0;
        vh[OMR + 1][l] = (c < C - 1) ? s_x[(((c + 1) * NL + l) * 2 + 0) * NM + m] : 0.0;
    }
    if (c == C - 1) {     // v0(n)
#pragma unroll
        for (int l = 0; l < NL; ++l) SC(3, l) = vh[OMR][l];
    }
    // ---- u0' - lambda u0 = v0, u0(n) = 0 ; the "opposite boundary value" is v0(1) = 0 (res(1) = f(1), fdm_integral.f90:243) ----
    if (DD) {      // u(:, nx) = bcs(:, 2)  (:440)
#pragma unroll
        for (int l = 0; l < NL; ++l) u_n[l] = SC(1, l);
    }
    ode_solve<2, NM, OMR, NL>(a.T2, -lam, a.chk2, nm, t, c, C, m, vh, v_1, u_n, u, ext, s_w, s_k, s_fac);
    // ---- u0(1), v0(n), du0(n) -> the three constants (opr_odes.f90:350-356 with the LU of k_nn_constants) ----
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        if (c == 0) SC(2, l) = u[0][l];
        if (c == C - 1) SC(4, l) = ext[l];
    }
    __syncthreads();
    if (DD) {      // :452-456
        const double aa = s_k[(OK_CST + 0) * NM + m], bc = s_k[(OK_CST + 1) * NM + m], dummy = s_k[(OK_CST + 2) * NM + m];
        const double sp1 = s_k[(OK_CST + 3) * NM + m], u11 = s_k[(OK_CST + 4) * NM + m];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const double u0_1 = SC(2, l), v0_n = SC(3, l), du0n = SC(4, l), bbl = SC(0, l), btl = SC(1, l);
            const double w = lam * btl - du0n + v0_n;
            v_1[l] = (aa * (bbl - u0_1) - u11 * w) * dummy;
            fn[l] = (sp1 * w - bc * (bbl - u0_1)) * dummy;
        }
    } else {
        const double a11 = s_k[(OK_CST + 0) * NM + m], a21 = s_k[(OK_CST + 1) * NM + m], a31 = s_k[(OK_CST + 2) * NM + m];
        const double a12 = s_k[(OK_CST + 3) * NM + m], a22 = s_k[(OK_CST + 4) * NM + m], a32 = s_k[(OK_CST + 5) * NM + m];
        const double a13 = s_k[(OK_CST + 6) * NM + m], a23 = s_k[(OK_CST + 7) * NM + m], a33 = s_k[(OK_CST + 8) * NM + m];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const double u0_1 = SC(2, l), v0_n = SC(3, l), du0n = SC(4, l), bbl = SC(0, l), btl = SC(1, l);
            v_1[l] = (bbl - lam * u0_1) / a11;
            u_n[l] = (btl - v0_n - a21 * v_1[l]) / a22;
            fn[l] = (btl - du0n - a31 * v_1[l] - a32 * u_n[l]) / a33;
            u_n[l] = u_n[l] - a23 * fn[l];
            v_1[l] = v_1[l] - a12 * u_n[l] - a13 * fn[l];
        }
    }
    // ---- superposition with the stored homogeneous solutions (opr_odes.f90:358-367); p^ = u, dp^/dy = v ----
    if (!store[0] && !store[NQ - 1]) return;
    // The homogeneous solutions decay like exp(-sqrt(lambda) distance from their wall): for all but the lowest modes they are below 1e-40 of
    // their maximum a few tens of rows away from the walls, where adding them changes no bit of the sum.  The plan records that band per
    // mode (k_ode_hom_band); chunks inside it skip the five loads (40 of the 100 B per mode and row this kernel would otherwise move).
    const bool need = (j0 <= (int)s_k[(OK_BAND + 0) * NM + m]) || (j0 + OMR - 1 >= (int)s_k[(OK_BAND + 1) * NM + m]);
#pragma unroll
    for (int p = 0; p < OMR; ++p) {
        const int j = j0 + p;
        const unsigned h = (unsigned)(((t / NM) * 5 * n + j) * NM + m), hs = (unsigned)(n * NM);       // hom_blocked[blk][5][n][NM]
        double hv1 = 0.0, hem = 0.0, hu1 = 0.0, hsp = 0.0, hep = 0.0;
        if (need) { hv1 = a.hom[h]; hem = a.hom[h + hs]; hu1 = a.hom[h + 2 * hs]; hsp = a.hom[h + 3 * hs]; if (!DD) hep = a.hom[h + 4 * hs]; }
        double uu[NL], vv[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const double u0 = u[p][l], v0 = vh[p + 1][l];
            if (DD) {           // :459-465: rows nx .. 2 by the general formula (u0(nx) = bcs(:,2), u1(nx) = sp(nx) = 0), row 1 = the bottom value
                if (j == 0) {
                    uu[l] = SC(0, l);
                    vv[l] = v_1[l] + lam * uu[l];
                } else {
                    uu[l] = u0 + fn[l] * hu1 + v_1[l] * hsp;
                    vv[l] = v0 + fn[l] * hv1 + v_1[l] * hem + lam * uu[l];
                }
            } else if (j == n - 1) {
                uu[l] = u_n[l];
                vv[l] = v0 + fn[l] * hv1 + v_1[l] * hem + lam * uu[l];
            } else if (j == 0) {
                uu[l] = u0 + fn[l] * hu1 + v_1[l] * hsp + u_n[l] * hep;
                vv[l] = v_1[l] + lam * uu[l];
            } else {
                uu[l] = u0 + fn[l] * hu1 + v_1[l] * hsp + u_n[l] * hep;
                vv[l] = v0 + fn[l] * hv1 + v_1[l] * hem + lam * uu[l];
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (!store[q]) continue;
            const unsigned idx = fidx0[q] + (unsigned)(j * a.nxh);
            P[idx] = make_double2(uu[2 * q], uu[2 * q + 1]);
            D[idx] = make_double2(vv[2 * q], vv[2 * q + 1]);
        }
    }
#undef SC
}

// The <= 4 singular modes (lambda = 0): OPR_ODE2_Factorize_NN_Sing -> _DN_Sing (opr_odes.f90:165-183, 37-96) with the same chunked
// solves, one workgroup: v0' = f (f(1) = 0), v0(n) = bcs_t ; u0' = v0, u0(1) = 0 ; u = u0 + c u1, v = v0 + c v1 with
// c = (v0(1) - du0(1)) / (du1(1) - v1(1)); u1, v1, du1 depend on the mode only (plan creation).
struct OdeSingArgs {
    OdeSys T1, T2;
    const double *chk1, *chk2;          // checkpoints of the ns singular modes, blocked [0][C][6][NM]
    const int *modes;                   // [ns] flat mode indices
    const double *v1, *u1, *du1;        // [n][ns] (line 0 of the stored pairs), [ns]
    const double *f_hat;
    double *p_hat, *dp_hat;
    double fscale;
    int n, nxh, ny, C, ns;
};

template <int NM>
__global__ void __launch_bounds__(512) k_ode_sing(OdeSingArgs a) {
    extern __shared__ double lds[];
    const int C = a.C, n = a.n;
    const int m = threadIdx.x % NM, c = threadIdx.x / NM;
    double *s_w = lds, *s_x = lds + 8 * 8 * NM;
    double *s_sc = s_x + (size_t)C * 4 * NM;
    double *s_k = s_sc + 10 * NM;
    double *s_fac = s_k + OK_SIZE * NM;
    const bool live = m < a.ns;
    const int t = a.modes[live ? m : 0];
    const unsigned fidx0 = (unsigned)((t % a.nxh) + a.nxh * a.ny * (t / a.nxh));
    const int j0 = c * OM;
    const double2 *F = reinterpret_cast<const double2 *>(a.f_hat);
    double vh[OM + 2][2], u[OM][2], ext[2];
    double zero[2] = {0, 0}, bct[2];
    {
        double fl[OM + 2][2];
#pragma unroll
        for (int p = 0; p < OM + 2; ++p) {
            const int j = j0 - 1 + p;
            double2 w = make_double2(0.0, 0.0);
            if (j >= 0 && j <= n - 1) w = F[fidx0 + (unsigned)(j * a.nxh)];
            fl[p][0] = w.x * a.fscale; fl[p][1] = w.y * a.fscale;
        }
        if (c == C - 1) { s_sc[2 * NM + m] = fl[OM][0]; s_sc[3 * NM + m] = fl[OM][1]; }      // Neumann datum at the top (opr_elliptic.f90:310-311)
        if (c == 0) { fl[1][0] = 0.0; fl[1][1] = 0.0; }                                     // f(1) = 0 (opr_odes.f90:59 via :179)
        __syncthreads();
        bct[0] = s_sc[2 * NM + m]; bct[1] = s_sc[3 * NM + m];
        ode_solve<2, NM>(a.T2, 0.0, a.chk2, 0, m, c, C, m, fl, zero, bct, reinterpret_cast<double (&)[OM][2]>(vh[1]), ext, s_w, s_k, s_fac);
    }
#pragma unroll
    for (int l = 0; l < 2; ++l) { s_x[((c * 2 + l) * 2 + 0) * NM + m] = vh[1][l]; s_x[((c * 2 + l) * 2 + 1) * NM + m] = vh[OM][l]; }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        vh[0][l] = (c > 0) ? s_x[(((c - 1) * 2 + l) * 2 + 1) * NM + m] : 0.0;
        vh[OM + 1][l] = (c < C - 1) ? s_x[(((c + 1) * 2 + l) * 2 + 0) * NM + m] : 0.0;
    }
    if (c == 0) { s_sc[4 * NM + m] = vh[1][0]; s_sc[5 * NM + m] = vh[1][1]; }                 // v0(1)
    ode_solve<1, NM>(a.T1, 0.0, a.chk1, 0, m, c, C, m, vh, zero, bct, u, ext, s_w, s_k, s_fac);
    if (c == 0) { s_sc[6 * NM + m] = ext[0]; s_sc[7 * NM + m] = ext[1]; }                   // du0 at the bottom
    __syncthreads();
    if (!live) return;
    const int ns = a.ns;
    const double f1 = 1.0 / (a.du1[m] - a.v1[(0 * n + 0) * ns + m]);
    double cc[2];
#pragma unroll
    for (int l = 0; l < 2; ++l) cc[l] = (s_sc[(4 + l) * NM + m] - s_sc[(6 + l) * NM + m]) * f1;
    double2 *P = reinterpret_cast<double2 *>(a.p_hat), *D = reinterpret_cast<double2 *>(a.dp_hat);
#pragma unroll
    for (int p = 0; p < OM; ++p) {
        const int j = j0 + p;
        const double hu = a.u1[j * ns + m], hv = a.v1[j * ns + m];
        const unsigned idx = fidx0 + (unsigned)(j * a.nxh);
        P[idx] = make_double2(u[p][0] + cc[0] * hu, u[p][1] + cc[1] * hu);
        D[idx] = make_double2(vh[p + 1][0] + cc[0] * hv, vh[p + 1][1] + cc[1] * hv);
    }
}

// ================================================================================================
// host side: geometry, checkpoints, launches
// ================================================================================================
int ode_modes_per_wg(int C) {
    // 256 threads per workgroup where the line allows it: two workgroups then share a CU (the kernel needs ~230 VGPRs, i.e. 8 waves per CU
    // either way) and one runs while the other waits at one of its ~40 barriers: 2.85 -> 2.55 ms at 512^3 against one 512-thread workgroup
    int nmw = 64;
    while (nmw > 4 && nmw * C > 256) nmw >>= 1;
    const int v = env_int("TLAB_ODE_NM", 0);      // experiments
    if ((v == 4 || v == 8 || v == 16 || v == 32 || v == 64) && v * C <= 512) nmw = v;
    return (nmw * C <= 512) ? nmw : 0;
}
size_t ode_lds_bytes(int C, int NM, int om, int NL) {
    return ((size_t)(8 * (4 + 2 * NL) + 2 * NL * C + 5 * NL + OK_SIZE) * NM + (size_t)(3 * om + 1) * NM * C) * sizeof(double);
}

template <int NM, bool DD, int NL>
static void launch_ode_nm(const OdeArgs &a, size_t lds, hipStream_t st) {
    allow_max_lds<&k_ode_nn<NM, DD, OM, NL>>();
    const long long nlive = NL == 4 ? (long long)a.nxh * (a.nm / a.nxh / 2 + 1) : a.nm;
    const unsigned grid = (unsigned)((nlive + NM - 1) / NM);
    hipLaunchKernelGGL((k_ode_nn<NM, DD, OM, NL>), dim3(grid), dim3(NM * a.C), lds, st, a);
}

void launch_ode(tlab_poisson_plan &P, double *f_hat, double *p_hat, double *dp_hat, hipStream_t st, bool dd) {
    OdeArgs a{};
    a.T1 = P.sys(0); a.T2 = P.sys(1);
    a.lam = P.lam.p; a.skip = P.d_skip; a.chk1 = P.chk[0].p; a.chk2 = P.chk[1].p; a.cst = dd ? P.cst_dd.p : P.cst.p; a.hom = P.homb.p; a.band = P.d_hom_band;
    a.f_hat = f_hat; a.p_hat = p_hat; a.dp_hat = dp_hat; a.fscale = P.norm;
    a.n = P.ny; a.nxh = P.nxh; a.ny = P.ny; a.C = P.ny / P.ode_om; a.nm = P.nm;
    // TLAB_ODE_PAIR_XCD = 0 (blocks in dispatch order) or the group size G, a power of two >= 16 (1 = 16, the round-5 pairing)
    static const int pair = [] {
        int v = env_int("TLAB_ODE_PAIR_XCD", 128);      // 128: XCD x takes 16 adjacent blocks of every 128 (HBM reads of the launch 4.07 -> 3.15 GB, requests 3.18e7 -> 2.46e7 at 512^3)
        if (v == 1) v = 16;
        if (v != 0 && (v < 16 || (v & (v - 1)) != 0)) v = 16;
        return v;
    }();
    a.pair_xcd = pair;
    const size_t lds = ode_lds_bytes(a.C, P.ode_nm_per_wg, P.ode_om, P.ode_pair ? 4 : 2);
    ProfScope ps(dd ? "k_ode_nn<DD>" : "k_ode_nn", st, (double)P.nm * P.ny * 48.0);      // algorithmic bytes: f^ in, p^ and dp^/dy out (its own tables -- checkpoints 12 B, the band of the homogeneous solutions -- come on top)
    // The pair form: 8 rows x 4 lines per thread (256 VGPRs, ~20 of them spilled) beats 4 rows x 4 lines in twice as many chunks (217 VGPRs, but 512-thread
    // workgroups that do not share a CU and a scan twice as long): 1.86 against 2.83 ms at 512^3, one mode per thread 2.30 (profiles/r03)
    if (P.ode_pair && P.ode_om != OM) throw Fail(TLAB_EHIP, "k_ode_nn: no pair form for this geometry");
    dispatch_nm(P.ode_nm_per_wg, [&](auto nm_c) {
        constexpr int NM = decltype(nm_c)::value;
        if (P.ode_pair) dd ? launch_ode_nm<NM, true, 4>(a, lds, st) : launch_ode_nm<NM, false, 4>(a, lds, st);
        else dd ? launch_ode_nm<NM, true, 2>(a, lds, st) : launch_ode_nm<NM, false, 2>(a, lds, st);
    });
    hipc(hipGetLastError(), "k_ode_nn");
}

void build_checkpoints(tlab_poisson_plan &P, hipStream_t st) {
    const int C = P.ny / P.ode_om, NM = P.ode_nm_per_wg;
    const long long nblk = (P.nm + NM - 1) / NM;
    for (int w = 0; w < 2; ++w) {
        const Int1Tables &T = w == 0 ? P.tmin : P.tmax;
        std::vector<double> bt(12);
        for (int j = 0; j < 3; ++j)
            for (int c = 0; c < 4; ++c) bt[j * 4 + c] = (w == 0) ? T.rb[j][c] : T.rt[j][c];
        P.d_bt[w].upload(bt);
        P.chk[w].alloc((size_t)C * 6 * nblk * NM);
    }
    const int grid = (int)((P.nm + 255) / 256);
    hipLaunchKernelGGL((k_ode_checkpoint<1>), dim3(grid), dim3(256), 0, st, P.sys(0), P.lam.p, 1.0, P.chk[0].p, P.nm, NM, C, P.ode_om);
    hipLaunchKernelGGL((k_ode_checkpoint<2>), dim3(grid), dim3(256), 0, st, P.sys(1), P.lam.p, -1.0, P.chk[1].p, P.nm, NM, C, P.ode_om);
    hipc(hipGetLastError(), "k_ode_checkpoint");
    P.homb.alloc((size_t)5 * P.ny * nblk * NM);
    const long long tot = (long long)5 * P.ny * P.nm;
    hipLaunchKernelGGL(k_ode_block_layout, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, P.hom.p, P.homb.p, 5, P.ny, P.nm, NM);
    hipc(hipGetLastError(), "k_ode_block_layout");
    static const bool band_on = env_int("TLAB_ODE_HOM_BAND", 1) != 0;
    if (band_on) {
        hipc(hipMalloc((void **)&P.d_hom_band, (size_t)2 * P.nm * sizeof(int)), "hipMalloc");
        static const double rel = [] { const char *e = getenv("TLAB_ODE_HOM_THR"); return e ? atof(e) : 1.0e-40; }();
        hipLaunchKernelGGL(k_ode_hom_band, dim3(grid), dim3(256), 0, st, P.hom.p, P.ny, P.nm, P.d_hom_band, rel);
        hipc(hipGetLastError(), "k_ode_hom_band");
    }
}

// k_ode_sing: 8 lanes per chunk (<= 4 modes in use), 4 when the line has more than 64 chunks (512 threads at most) -- ode_sing_nm.
// 256 threads from 512 rows on: the one workgroup then fits the slot any retiring workgroup of k_ode_nn (256 threads, ~250 VGPRs: two per CU)
// leaves; with 512 threads it needs a whole CU and waited for the tail of k_ode_nn (measured: 1.84 ms in the queue beside the pair form)
void build_singular_checkpoints(tlab_poisson_plan &P, hipStream_t st) {
    const int ns = (int)P.sing_modes.size();
    if (ns == 0) return;
    const int C = P.ny / OM, NM = ode_sing_nm(C);
    for (int w = 0; w < 2; ++w) P.chk_s[w].alloc((size_t)C * 6 * NM);
    hipLaunchKernelGGL((k_ode_checkpoint<1>), dim3(1), dim3(256), 0, st, P.sys(0), P.s_lam.p, 1.0, P.chk_s[0].p, (long long)ns, NM, C, OM);
    hipLaunchKernelGGL((k_ode_checkpoint<2>), dim3(1), dim3(256), 0, st, P.sys(1), P.s_lam.p, -1.0, P.chk_s[1].p, (long long)ns, NM, C, OM);
    hipc(hipGetLastError(), "k_ode_checkpoint (singular)");
}

void launch_ode_sing(tlab_poisson_plan &P, double *f_hat, double *p_hat, double *dp_hat, hipStream_t st) {
    OdeSingArgs a{};
    a.T1 = P.sys(0); a.T2 = P.sys(1);
    a.chk1 = P.chk_s[0].p; a.chk2 = P.chk_s[1].p; a.modes = P.d_sing;
    a.v1 = P.s_v1.p; a.u1 = P.s_u1.p; a.du1 = P.s_du1.p;
    a.f_hat = f_hat; a.p_hat = p_hat; a.dp_hat = dp_hat; a.fscale = P.norm;
    a.n = P.ny; a.nxh = P.nxh; a.ny = P.ny; a.C = P.ny / OM; a.ns = (int)P.sing_modes.size();
    ProfScope ps("k_ode_sing", st, (double)a.ns * P.ny * 48.0);
    dispatch_nm(ode_sing_nm(a.C), [&](auto nm_c) {
        constexpr int NM = decltype(nm_c)::value;
        if constexpr (NM <= 8) {      // (ode_sing_nm gives 4 or 8: no wider forms of the kernel are built)
            allow_max_lds<&k_ode_sing<NM>>();
            hipLaunchKernelGGL((k_ode_sing<NM>), dim3(1), dim3(NM * a.C), ode_lds_bytes(a.C, NM), st, a);
        }
    });
    hipc(hipGetLastError(), "k_ode_sing");
}

}  // namespace tlab
