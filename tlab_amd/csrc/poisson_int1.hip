// The marching first-order integral solves of the Poisson solver (poisson.hip): k_int1, k_int1g and their launcher.
#include "poisson_dev.hpp"

namespace tlab {

template <int NL, int FS>
__device__ __forceinline__ void load_f(const Int1Args &a, int j, long long t, long long fidx0, double (&f)[NL]) {
    if (FS == FS_FIELD) {
        if (NL == 1 && a.fpart) {       // (SPLIT launch: the imaginary part alone)
            f[0] = reinterpret_cast<const double *>(a.fsrc)[2 * (fidx0 + (long long)j * a.nxh) + 1] * a.fscale;
            return;
        }
        const double2 v = reinterpret_cast<const double2 *>(a.fsrc)[fidx0 + (long long)j * a.nxh];
        f[0] = v.x * a.fscale;
        if (NL > 1) f[1] = v.y * a.fscale;
    } else if (FS == FS_LINEAR) {
#pragma unroll
        for (int l = 0; l < NL; ++l) f[l] = (l < a.nlf) ? a.fsrc[((long long)l * a.T.n + j) * a.nm + t] : 0.0;
    } else {
#pragma unroll
        for (int l = 0; l < NL; ++l) f[l] = (l == 0 && j == a.unit_row) ? 1.0 : 0.0;
    }
}

// One FDM_Int1_Solve per thread (mode).  BC = 1: value given at the bottom (BCS_MIN), BC = 2: at the top (BCS_MAX).
// SPLIT (with NL = 1): the two lines of a mode (real and imaginary part) on two threads, thread gid -> (mode gid % nm, line gid / nm).  The few
// modes of the low-mode sub-plan are a latency chain of n dependent rows bound by the instructions per row: half of them per thread.
// LDSV (with SPLIT): the few lines of the low-mode sub-plan are a chain of 2 n dependent rows whose every block of U rows waited for a round trip to
// memory -- 0.7 + 0.3 ms per substep at 512 rows beside a k_ode_nn that keeps the memory system busy, and on z-slabs / kx-pencils the critical path of
// the ranks that own the low kx.  Here a workgroup stages what its LV1 = 4 (2 from 1024 rows on) lines read in a sweep (source and forward factors, then
// the backward factors; the two right-hand-side coefficients) in LDS with all its threads, four lanes run the same recurrences on LDS operands (same
// expressions, same order: the results are the marching kernel's to the bit), and the intermediate of the forward sweep stays in LDS.
template <int BC, int NL, int FS, int U, bool STORED, bool SPLIT = false, bool LDSV = false, int LV1 = 4>
__global__ void __launch_bounds__(256) k_int1(Int1Args a) {
#pragma clang fp contract(off)
    static_assert(!SPLIT || (NL == 1 && STORED), "SPLIT: one line per thread, stored factors");
    static_assert(!LDSV || (SPLIT && FS != FS_UNIT), "LDSV: the low-mode form");
    extern __shared__ double s_i1[];
    const int n = a.T.n;
    const long long nm = a.nm;
    // LDS per line: four rows of n doubles -- forward sweep: source, a, b (forward factors), intermediate out; backward sweep: 1/c, -d, -e, intermediate
    // (16 KiB per line at 512 rows: a workgroup of four lines fits beside ONE workgroup of k_ode_nn on a CU, so it is scheduled while that kernel runs)
    double *s_b = s_i1, *s_R = s_b + LV1 * 4 * n;      // [LV1][4][n], [n][2]
    auto stage = [&](bool forward) {
        for (int idx = threadIdx.x; idx < LV1 * n; idx += blockDim.x) {
            const int k = idx / n, j = idx - k * n;
            const long long g = (long long)blockIdx.x * LV1 + k;
            if (g >= 2 * nm) continue;
            const long long tk = g % nm;
            const int pk = (int)(g / nm);
            if (forward) {
                double fv;
                if (FS == FS_FIELD) {
                    const long long f0 = (tk % a.nxh) + (long long)a.nxh * a.ny * (tk / a.nxh);
                    fv = a.fsrc[2 * (f0 + (long long)j * a.nxh) + pk];
                } else {
                    fv = (pk < a.nlf) ? a.fsrc[((long long)pk * n + j) * nm + tk] : 0.0;      // (line pk of the stored lines; lines >= nlf are zero)
                }
                s_b[(k * 4 + 0) * n + j] = fv;
                s_b[(k * 4 + 1) * n + j] = a.fac[((long long)0 * n + j) * nm + tk];
                s_b[(k * 4 + 2) * n + j] = a.fac[((long long)1 * n + j) * nm + tk];
            } else {
#pragma unroll
                for (int q = 0; q < 3; ++q) s_b[(k * 4 + q) * n + j] = a.fac[((long long)(2 + q) * n + j) * nm + tk];
            }
        }
    };
    bool active = true;      // LDSV: lanes beyond the workgroup's lines (and beyond the last line) repeat the work of its first line and store nothing: every
                             // thread reaches the barriers between the sweeps
    if constexpr (LDSV) {
        stage(true);
        for (int idx = threadIdx.x; idx < n; idx += blockDim.x) { s_R[idx * 2] = a.T.R[idx * 3]; s_R[idx * 2 + 1] = a.T.R[idx * 3 + 1]; }
        __syncthreads();
        active = threadIdx.x < LV1 && (long long)blockIdx.x * LV1 + threadIdx.x < 2 * nm;
    }
    const int myk = (LDSV && active) ? (int)threadIdx.x : 0;
    const long long gid = LDSV ? (long long)blockIdx.x * LV1 + myk : (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (!LDSV && gid >= (SPLIT ? 2 : 1) * a.nm) return;
    const long long t = SPLIT ? gid % a.nm : gid;
    const int part = SPLIT ? (int)(gid / a.nm) : 0;
    if (SPLIT && part) {      // line 1 of every array becomes this thread's line 0
        a.scratch += (long long)n * nm;
        a.dst += (long long)n * nm;
        if (a.du) a.du += nm;
        if (a.bv_ptr) a.bv_ptr += nm;
        a.bv[0] = a.bv[1];
        if (FS == FS_LINEAR) { a.fsrc += (long long)n * nm; a.nlf -= 1; }
        a.fpart = 1;
    }
    const double lam = a.lam_sign * a.lam[t];
    const long long fidx0 = (FS == FS_FIELD) ? (t % a.nxh) + (long long)a.nxh * a.ny * (t / a.nxh) : 0;
    auto ldf = [&](int j, double (&f)[NL]) {      // row j of the source: from LDS (LDSV: the staged raw value, scaled / masked as load_f does) or from memory
        if constexpr (LDSV) {
            if (FS == FS_FIELD) f[0] = s_b[(myk * 4 + 0) * n + j] * a.fscale;
            else f[0] = (0 < a.nlf) ? s_b[(myk * 4 + 0) * n + j] : 0.0;
        } else {
            load_f<NL, FS>(a, j, t, fidx0, f);
        }
    };

    // ---- boundary rows of the system of this mode (fdm_integral.f90:203-211 -> FDM_Bcs_Reduce at the opposite end) ----
    double l0[5], l1[5], l2[5], lN[5], lN1[5], lN2[5], rb[3][4], rt[3][4];
    lhs_row(a.T, 0, lam, l0); lhs_row(a.T, 1, lam, l1); lhs_row(a.T, 2, lam, l2);
    lhs_row(a.T, n - 1, lam, lN); lhs_row(a.T, n - 2, lam, lN1); lhs_row(a.T, n - 3, lam, lN2);
    if (BC == 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) rb[j][c] = a.T.rb[j][c];
        const double d = 1.0 / lN[2];
#pragma unroll
        for (int k = 0; k < 5; ++k) lN[k] = -lN[k] * d;
        lN[2] = 1.0;
        lN1[0] = nf_madd(lN1[0], lN1[3], lN[4]); lN1[1] = nf_madd(lN1[1], lN1[3], lN[0]); lN1[2] = nf_madd(lN1[2], lN1[3], lN[1]);
        lN2[1] = nf_madd(lN2[1], lN2[4], lN[4]); lN2[2] = nf_madd(lN2[2], lN2[4], lN[0]); lN2[3] = nf_madd(lN2[3], lN2[4], lN[1]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            rt[2][c] = a.T.R[(n - 1) * 3 + c] * d;
            rt[1][c] = a.T.R[(n - 2) * 3 + c];
            rt[0][c] = a.T.R[(n - 3) * 3 + c];
        }
        rt[0][3] = rt[1][3] = rt[2][3] = 0.0;
        rt[1][0] = nf_msub(rt[1][0], lN1[3], rt[2][2]); rt[1][1] = nf_msub(rt[1][1], lN1[3], rt[2][0]); rt[1][2] = nf_msub(rt[1][2], lN1[3], rt[2][1]);
        rt[0][1] = nf_msub(rt[0][1], lN2[4], rt[2][2]); rt[0][2] = nf_msub(rt[0][2], lN2[4], rt[2][0]); rt[0][3] = nf_msub(rt[0][3], lN2[4], rt[2][1]);
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) rt[j][c] = a.T.rt[j][c];
        const double d = 1.0 / l0[2];
#pragma unroll
        for (int k = 0; k < 5; ++k) l0[k] = -l0[k] * d;
        l0[2] = 1.0;
        l1[2] = nf_madd(l1[2], l1[1], l0[3]); l1[3] = nf_madd(l1[3], l1[1], l0[4]); l1[4] = nf_madd(l1[4], l1[1], l0[0]);
        l2[1] = nf_madd(l2[1], l2[0], l0[3]); l2[2] = nf_madd(l2[2], l2[0], l0[4]); l2[3] = nf_madd(l2[3], l2[0], l0[0]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            rb[0][c + 1] = a.T.R[0 * 3 + c] * d;
            rb[1][c + 1] = a.T.R[1 * 3 + c];
            rb[2][c + 1] = a.T.R[2 * 3 + c];
        }
        rb[0][0] = rb[1][0] = rb[2][0] = 0.0;
        rb[1][1] = nf_msub(rb[1][1], l1[1], rb[0][2]); rb[1][2] = nf_msub(rb[1][2], l1[1], rb[0][3]); rb[1][3] = nf_msub(rb[1][3], l1[1], rb[0][1]);
        rb[2][0] = nf_msub(rb[2][0], l2[0], rb[0][2]); rb[2][1] = nf_msub(rb[2][1], l2[0], rb[0][3]); rb[2][2] = nf_msub(rb[2][2], l2[0], rb[0][1]);
    }

    // ---- boundary values: res0 (row 0) and resN (row n-1) as MatMul_3d sees them (fdm_integral.f90:240-245) ----
    double fb0[NL], fbN[NL], res0[NL], resN[NL];
    ldf(0, fb0);
    ldf(n - 1, fbN);
    if (FS == FS_FIELD && a.bcs_save != nullptr) {  // Neumann data travel in the forcing planes (opr_elliptic.f90:285-286,310-311)
        if (SPLIT) {
            if (active) {
                a.bcs_save[(long long)part * nm + t] = fb0[0];
                a.bcs_save[(long long)(2 + part) * nm + t] = fbN[0];
            }
        } else {
            a.bcs_save[0 * nm + t] = fb0[0]; a.bcs_save[1 * nm + t] = fb0[NL > 1 ? 1 : 0];
            a.bcs_save[2 * nm + t] = fbN[0]; a.bcs_save[3 * nm + t] = fbN[NL > 1 ? 1 : 0];
        }
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        const double given = a.bv_ptr ? a.bv_ptr[(long long)l * nm + t] : a.bv[l];
        if (BC == 1) { res0[l] = given; resN[l] = a.zero_bsave ? 0.0 : fbN[l]; }
        else { resN[l] = given; res0[l] = a.zero_bsave ? 0.0 : fb0[l]; }
    }

    // ---- forward: right-hand side (MatMul_3d, BCS_BOTH), LU on the fly (PENTADFS), forward substitution (PENTADSS) ----
    double fm[NL], fc[NL], fp[NL];           // f[j-1], f[j], f[j+1]
    ldf(1, fc);
    ldf(2, fp);
    double f1[NL], fn2[NL];                   // f[1] and f[n-2] are needed again for du
    double bcs_b[NL], bcs_t[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        f1[l] = fc[l];
        bcs_b[l] = res0[l] * rb[0][2] + fc[l] * rb[0][3] + fp[l] * rb[0][1];
        fm[l] = 0.0;
    }
    double c1 = 0.0, c2 = 0.0, d1 = 0.0, d2 = 0.0, e1 = 0.0, e2 = 0.0;  // pivots of rows m-1, m-2
    double y1[NL], y2[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) y1[l] = y2[l] = 0.0;
    const int nmax = n - 2;
    // U = rows per block: the loads of a block are issued together so that only one memory latency is exposed per U rows.  Large U
    // pays on small slabs (few modes -> few waves -> latency-bound), small U keeps the registers down when the grid fills the chip.
    constexpr bool stored = STORED;          // a.fac != nullptr (launch_int1): the factors of every row are read instead of regenerated
    for (int jb = 1; jb <= nmax; jb += U) {
        double fqb[U][NL], fab[U][2];         // f[jb+2 .. jb+U+1]; stored forward factors of rows jb .. jb+U-1
        double Rb[U][2];                      // right-hand-side coefficients of the rows of the block: requested with the rest, BEFORE the first store
        //                                       of the block (the output arrays may alias the tables as far as the compiler knows: left inside the row loop,
        //                                       every row waited for its own scalar load -- 7 us per block of 8 rows with few modes in flight)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jc = (jb + u <= nmax) ? jb + u : nmax;
            if constexpr (LDSV) { Rb[u][0] = s_R[jc * 2 + 0]; Rb[u][1] = s_R[jc * 2 + 1]; }
            else { Rb[u][0] = a.T.R[jc * 3 + 0]; Rb[u][1] = a.T.R[jc * 3 + 1]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jr = jb + u + 2;
            if (jr <= n - 1) ldf(jr, fqb[u]);
            else {
#pragma unroll
                for (int l = 0; l < NL; ++l) fqb[u][l] = 0.0;
            }
            fab[u][0] = fab[u][1] = 0.0;
            if (stored) {
                const int jf = (jb + u <= nmax) ? jb + u : nmax;
                if constexpr (LDSV) { fab[u][0] = s_b[(myk * 4 + 1) * n + jf]; fab[u][1] = s_b[(myk * 4 + 2) * n + jf]; }
                else {
                    fab[u][0] = a.fac[((long long)0 * n + jf) * nm + t];
                    fab[u][1] = a.fac[((long long)1 * n + jf) * nm + t];
                }
            }
        }
        // A block without one of the boundary rows 1, 2, n-3, n-2 (all but the first and the last one or two) takes the plain form of every
        // expression: with few modes in flight (the low-mode sub-plan: 2 waves) the kernel is bound by the instructions per row, and the
        // row-number selects of the general form are most of them.
        const bool edge_blk = jb < 3 || jb + U - 1 > n - 4;
        auto fwd_row = [&](auto edge_c, int u) {
            constexpr bool EDGE = decltype(edge_c)::value;
            const int j = jb + u;
            if (EDGE && j > nmax) return;
            double r[5] = {0.0, 0.0, 1.0, 0.0, 0.0};
            if (!stored) {
                if (EDGE && j == 1) { for (int k = 0; k < 5; ++k) r[k] = l1[k]; }
                else if (EDGE && j == 2) { for (int k = 0; k < 5; ++k) r[k] = l2[k]; }
                else if (EDGE && j == n - 3) { for (int k = 0; k < 5; ++k) r[k] = lN2[k]; }
                else if (EDGE && j == n - 2) { for (int k = 0; k < 5; ++k) r[k] = lN1[k]; }
                else lhs_row(a.T, j, lam, r);
            }
            // right-hand side of row j
            double rhs[NL];
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                if (EDGE && j == 1) rhs[l] = res0[l] * rb[1][1] + fc[l] * rb[1][2] + fp[l] * rb[1][3];
                else if (EDGE && j == 2) rhs[l] = res0[l] * rb[2][0] + fm[l] * rb[2][1] + fc[l] * rb[2][2] + fp[l] * rb[2][3];
                else if (EDGE && j == n - 3) rhs[l] = fm[l] * rt[0][0] + fc[l] * rt[0][1] + fp[l] * rt[0][2] + resN[l] * rt[0][3];
                else if (EDGE && j == n - 2) rhs[l] = fm[l] * rt[1][0] + fc[l] * rt[1][1] + resN[l] * rt[1][2];
                else rhs[l] = fm[l] * Rb[u][0] + fc[l] * Rb[u][1] + fp[l];
            }
            if (EDGE && j == n - 2) {
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    fn2[l] = fc[l];
                    bcs_t[l] = fm[l] * rt[2][2] + fc[l] * rt[2][0] + resN[l] * rt[2][1];
                }
            }
            // PENTADFS row m = j
            double am = 0.0, bm = 0.0, cm = r[2], dm = r[3], em = r[4], cinv = 1.0;
            if (stored) {
                am = fab[u][0]; bm = fab[u][1];
            } else {
                if (EDGE && j == 2) {
                    bm = r[1] / c1;
                    cm = nf_msub(r[2], bm, d1);
                    dm = nf_msub(r[3], bm, e1);
                } else if (!EDGE || j >= 3) {
                    am = r[0] / c2;
                    bm = nf_msub(r[1], am, d2) / c1;
                    cm = nf_msub(nf_msub(r[2], bm, d1), am, e2);
                    dm = nf_msub(r[3], bm, e1);
                }
                cinv = 1.0 / cm;
            }
            // PENTADSS forward: f(n) = f(n) + f(n-1)*b(n) + f(n-2)*a(n) with a, b negated
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double y = rhs[l] - y1[l] * bm - y2[l] * am;
                if constexpr (LDSV) s_b[(myk * 4 + 3) * n + j] = y;      // (the lanes that repeat line 0 write the same value)
                else a.scratch[((long long)l * n + j) * nm + t] = y;
                y2[l] = y1[l];
                y1[l] = y;
            }
            if (!stored) {
                a.scratch[((long long)(NL + 0) * n + j) * nm + t] = cinv;
                a.scratch[((long long)(NL + 1) * n + j) * nm + t] = -dm;
                a.scratch[((long long)(NL + 2) * n + j) * nm + t] = -em;
                if (a.fac_out) {
                    a.fac_out[((long long)0 * n + j) * nm + t] = am; a.fac_out[((long long)1 * n + j) * nm + t] = bm;
                    a.fac_out[((long long)2 * n + j) * nm + t] = cinv; a.fac_out[((long long)3 * n + j) * nm + t] = -dm;
                    a.fac_out[((long long)4 * n + j) * nm + t] = -em;
                }
            }
            c2 = c1; d2 = d1; e2 = e1;
            c1 = cm; d1 = dm; e1 = em;
#pragma unroll
            for (int l = 0; l < NL; ++l) { fm[l] = fc[l]; fc[l] = fp[l]; fp[l] = fqb[u][l]; }
        };
        if (edge_blk) {
#pragma unroll
            for (int u = 0; u < U; ++u) fwd_row(std::true_type{}, u);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) fwd_row(std::false_type{}, u);
        }
    }

    if constexpr (LDSV) {      // the backward factors take the place of the source and the forward factors
        __syncthreads();
        stage(false);
        __syncthreads();
    }
    // ---- backward substitution ----
    double x1[NL], x2[NL];                    // x[j+1], x[j+2]
    double xs1[NL], xs2[NL], xs3[NL];         // x[1], x[2], x[3]
    double xe2[NL], xe3[NL], xe4[NL];         // x[n-2], x[n-3], x[n-4]
#pragma unroll
    for (int l = 0; l < NL; ++l) x1[l] = x2[l] = xs1[l] = xs2[l] = xs3[l] = xe2[l] = xe3[l] = xe4[l] = 0.0;
    const double *fsrc = stored ? a.fac + (long long)2 * n * nm : a.scratch + (long long)NL * n * nm;      // 1/c, -d, -e of every row
    for (int jb = nmax; jb >= 1; jb -= U) {
        double yb[U][NL], cb[U], db[U], eb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = jb - u;
            const int jr = j >= 1 ? j : 1;
            if constexpr (LDSV) {
                cb[u] = s_b[(myk * 4 + 0) * n + jr]; db[u] = s_b[(myk * 4 + 1) * n + jr]; eb[u] = s_b[(myk * 4 + 2) * n + jr];
                yb[u][0] = s_b[(myk * 4 + 3) * n + jr];
            } else {
                cb[u] = fsrc[((long long)0 * n + jr) * nm + t];
                db[u] = fsrc[((long long)1 * n + jr) * nm + t];
                eb[u] = fsrc[((long long)2 * n + jr) * nm + t];
#pragma unroll
                for (int l = 0; l < NL; ++l) yb[u][l] = a.scratch[((long long)l * n + jr) * nm + t];
            }
        }
        const bool edge_blk = jb > n - 5 || jb - U + 1 < 4;       // holds one of the rows 1, 2, 3, n-4, n-3, n-2 (kept for the boundary formulas), or runs past row 1
        auto bwd_row = [&](auto edge_c, int u) {
            constexpr bool EDGE = decltype(edge_c)::value;
            const int j = jb - u;
            if (EDGE && j < 1) return;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const double x = (yb[u][l] + x1[l] * db[u] + x2[l] * eb[u]) * cb[u];
                if (active) a.dst[((long long)l * n + j) * nm + t] = x;
                x2[l] = x1[l];
                x1[l] = x;
                if (EDGE) {
                    if (j == 1) xs1[l] = x;
                    if (j == 2) xs2[l] = x;
                    if (j == 3) xs3[l] = x;
                    if (j == n - 2) xe2[l] = x;
                    if (j == n - 3) xe3[l] = x;
                    if (j == n - 4) xe4[l] = x;
                }
            }
        };
        if (edge_blk) {
#pragma unroll
            for (int u = 0; u < U; ++u) bwd_row(std::true_type{}, u);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) bwd_row(std::false_type{}, u);
        }
    }

    // ---- boundary value at the free end and derivative at the given end (fdm_integral.f90:265-311) ----
    if (!active) return;
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        if (BC == 2) {
            const double r0 = bcs_b[l] + l0[3] * xs1[l] + l0[4] * xs2[l] + l0[0] * xs3[l];
            a.dst[((long long)l * n + 0) * nm + t] = r0;
            a.dst[((long long)l * n + (n - 1)) * nm + t] = resN[l];
            if (a.du) a.du[(long long)l * nm + t] = lN[2] * resN[l] + lN[1] * xe2[l] + lN[0] * xe3[l] + lN[4] * xe4[l] + a.T.R[(n - 1) * 3 + 0] * fn2[l];
        } else {
            const double rN = bcs_t[l] + lN[1] * xe2[l] + lN[0] * xe3[l] + lN[4] * xe4[l];
            a.dst[((long long)l * n + (n - 1)) * nm + t] = rN;
            a.dst[((long long)l * n + 0) * nm + t] = res0[l];
            if (a.du) a.du[(long long)l * nm + t] = l0[2] * res0[l] + l0[3] * xs1[l] + l0[4] * xs2[l] + l0[0] * xs3[l] + a.T.R[0 * 3 + 2] * f1[l];
        }
    }
}

// ================================================================================================
// k_int1g : FDM_Int1_Solve (fdm/fdm_integral.f90:219-314) for the 3- and 7-diagonal integral systems of SpaceOrder1 = CompactJacobian4 /
// CompactDirect4 / CompactJacobian6Penta, factorized on the host (int1_generic.cpp).  One thread per mode, the reference's operations in the
// reference's order, no fused multiply-adds: right-hand side (MatMul_3d / MatMul_5d with BCS_BOTH, fdm_matmul.f90:70-121 / :267-320), substitution
// (TRIDSS utils/linear3.f90:56-150 / HEPTADSS utils/linear7.f90:98-142), value at the free end and derivative at the given one (:265-311).
// Nobody selects these schemes with the factorized solver: correctness first, every operand re-read where it is used.
// Compiled at -O3 like everything else since round 4.  Rounds 2-3 carried __attribute__((optnone)) here because "-O3 gave O(1) errors that vanished when a
// printf was added".  Root cause (tools/repro/int1g_O3.hip, a stand-alone reduction: the same function body on host and device): hipcc 7.2's loop
// unroller mis-transforms the two substitution loops below -- loops whose first three / last three iterations take other branches and whose
// iterations communicate through memory -- at -O2 and -O3; -O1, -O0 and -fno-unroll-loops give the host's bits, the host replay is clean under
// AddressSanitizer and UBSan (no undefined behaviour in the source), fences and volatile accesses change nothing.  `#pragma clang loop
// unroll(disable)` on those two loops is the whole work-around; every instantiation in use is bitwise equal to the oracle at -O3
// (tests/test_gpu_poisson.py, tlab_debug_int1_solve variants 0-2).
template <int BC, int NL, int FS, int NDI>
__global__ void __launch_bounds__(256) k_int1g(Int1Args a) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.nm) return;
    constexpr int ndi = NDI, nri = NDI == 3 ? 3 : 5, idl = ndi / 2 + 1, idr = nri / 2 + 1;      // (3, 3): CompactJacobian4 / Direct4; (7, 5): CompactJacobian6Penta
    const int n = a.T.n;
    const long long nm = a.nm;
    const long long fidx0 = (FS == FS_FIELD) ? (t % a.nxh) + (long long)a.nxh * a.ny * (t / a.nxh) : 0;
    auto F = [&](int k, int j) { return a.g_fac[((long long)k * n + j) * nm + t]; };                 // diagonal k (0-based) of row j (0-based)
    auto RB = [&](int j1, int c) { return a.g_rb[(long long)((j1 - 1) + 5 * c) * nm + t]; };          // rhs_b(j1, c)
    auto RT = [&](int r, int c1) { return a.g_rt[(long long)(r + 5 * (c1 - 1)) * nm + t]; };          // rhs_t(r, c1)
    auto Rr = [&](int j, int k1) { return a.g_R[j * nri + (k1 - 1)]; };                               // rhs(j+1, k1)
    auto fv = [&](int j, int l) -> double {                                                            // f(l, j+1): one value, no private array
        if (FS == FS_FIELD) return reinterpret_cast<const double *>(a.fsrc)[2 * (fidx0 + (long long)j * a.nxh) + l] * a.fscale;
        if (FS == FS_LINEAR) return (l < a.nlf) ? a.fsrc[((long long)l * n + j) * nm + t] : 0.0;
        return (l == 0 && j == a.unit_row) ? 1.0 : 0.0;
    };
    double res0[NL], resN[NL];
    {
        double fb0[NL], fbN[NL];
        load_f<NL, FS>(a, 0, t, fidx0, fb0);
        load_f<NL, FS>(a, n - 1, t, fidx0, fbN);
        if (FS == FS_FIELD && a.bcs_save != nullptr) {
            a.bcs_save[0 * nm + t] = fb0[0]; a.bcs_save[1 * nm + t] = fb0[NL > 1 ? 1 : 0];
            a.bcs_save[2 * nm + t] = fbN[0]; a.bcs_save[3 * nm + t] = fbN[NL > 1 ? 1 : 0];
        }
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const double given = a.bv_ptr ? a.bv_ptr[(long long)l * nm + t] : a.bv[l];
            if (BC == 1) { res0[l] = given; resN[l] = a.zero_bsave ? 0.0 : fbN[l]; }
            else { resN[l] = given; res0[l] = a.zero_bsave ? 0.0 : fb0[l]; }
        }
    }
    const int nmax = n - 2;                       // the systems are those of rows 2 .. n-1; sub-row m <-> row j = m + 1 (0-based)
#pragma unroll
    for (int l = 0; l < NL; ++l) {
        // ---- right-hand side of row j (0-based) ----
        auto rhs_row = [&](int j) -> double {
            if (nri == 3) {
                if (j == 1) return res0[l] * RB(2, 1) + fv(1, l) * RB(2, 2) + fv(2, l) * RB(2, 3);
                if (j == 2) return res0[l] * RB(3, 0) + fv(1, l) * RB(3, 1) + fv(2, l) * RB(3, 2) + fv(3, l) * RB(3, 3);
                if (j == n - 3) return fv(n - 4, l) * RT(0, 1) + fv(n - 3, l) * RT(0, 2) + fv(n - 2, l) * RT(0, 3) + resN[l] * RT(0, 4);
                if (j == n - 2) return fv(n - 3, l) * RT(1, 1) + fv(n - 2, l) * RT(1, 2) + resN[l] * RT(1, 3);
                return fv(j - 1, l) * Rr(j, 1) + fv(j, l) * Rr(j, 2) + fv(j + 1, l);
            }
            if (j == 1) return res0[l] * RB(2, 2) + fv(1, l) * RB(2, 3) + fv(2, l) * RB(2, 4) + fv(3, l) * RB(2, 5);
            if (j == 2) return res0[l] * RB(3, 1) + fv(1, l) * RB(3, 2) + fv(2, l) * RB(3, 3) + fv(3, l) * RB(3, 4) + fv(4, l) * RB(3, 5);
            if (j == 3) return res0[l] * RB(4, 0) + fv(1, l) * RB(4, 1) + fv(2, l) * RB(4, 2) + fv(3, l) * RB(4, 3) + fv(4, l) * RB(4, 4) + fv(5, l) * RB(4, 5);
            if (j == n - 4)
                return fv(n - 6, l) * RT(0, 1) + fv(n - 5, l) * RT(0, 2) + fv(n - 4, l) * RT(0, 3) + fv(n - 3, l) * RT(0, 4) + fv(n - 2, l) * RT(0, 5) +
                       resN[l] * RT(0, 6);
            if (j == n - 3) return fv(n - 5, l) * RT(1, 1) + fv(n - 4, l) * RT(1, 2) + fv(n - 3, l) * RT(1, 3) + fv(n - 2, l) * RT(1, 4) + resN[l] * RT(1, 5);
            if (j == n - 2) return fv(n - 4, l) * RT(2, 1) + fv(n - 3, l) * RT(2, 2) + fv(n - 2, l) * RT(2, 3) + resN[l] * RT(2, 4);
            return fv(j - 2, l) * Rr(j, 1) + fv(j - 1, l) * Rr(j, 2) + fv(j, l) * Rr(j, 3) + fv(j + 1, l) + fv(j + 2, l) * Rr(j, 5);
        };
        double bcs_b, bcs_t;
        if (nri == 3) {
            bcs_b = res0[l] * RB(1, 2) + fv(1, l) * RB(1, 3) + fv(2, l) * RB(1, 1);
            bcs_t = fv(n - 3, l) * RT(2, 3) + fv(n - 2, l) * RT(2, 1) + resN[l] * RT(2, 2);
        } else {
            bcs_b = res0[l] * RB(1, 3) + fv(1, l) * RB(1, 4) + fv(2, l) * RB(1, 5) + fv(3, l) * RB(1, 1);
            bcs_t = fv(n - 4, l) * RT(3, 5) + fv(n - 3, l) * RT(3, 1) + fv(n - 2, l) * RT(3, 2) + resN[l] * RT(3, 3);
        }
        double *y = a.scratch + (long long)l * n * nm + t;                   // y(j) at y[j * nm]
        double *x = a.dst + (long long)l * n * nm + t;
        // ---- forward substitution (the rows before come back from memory: same thread, program order) ----
        auto Y = [&](int j) { return y[(long long)j * nm]; };
#pragma clang loop unroll(disable)      // hipcc 7.2 miscompiles these two loops when its loop unroller peels them: tools/repro/int1g_O3.hip
        for (int m = 0; m < nmax; ++m) {
            const int j = m + 1;
            const double r = rhs_row(j);
            double v;
            if constexpr (NDI == 3) {
                v = m == 0 ? r : r + F(0, j) * Y(j - 1);                      // f(n) = f(n) + a(n) f(n-1)
            } else {
                if (m == 0) v = r * F(2, j);                                  // normalise the first equation (c(1) = 1 / d(1), HEPTADFS)
                else if (m == 1) v = r - Y(j - 1) * F(2, j);
                else if (m == 2) v = r - Y(j - 1) * F(2, j) - Y(j - 2) * F(1, j);
                else v = r - Y(j - 1) * F(2, j) - Y(j - 2) * F(1, j) - Y(j - 3) * F(0, j);
            }
            y[(long long)j * nm] = v;
        }
        // ---- backward substitution ----
        auto XX = [&](int j) { return x[(long long)j * nm]; };
#pragma clang loop unroll(disable)
        for (int m = nmax - 1; m >= 0; --m) {
            const int j = m + 1;
            const double yv = Y(j);
            double v;
            if constexpr (NDI == 3) {
                v = m == nmax - 1 ? yv * F(1, j) : (yv + F(2, j) * XX(j + 1)) * F(1, j);
            } else {
                if (m == nmax - 1) v = yv / F(3, j);
                else if (m == nmax - 2) v = (yv - XX(j + 1) * F(4, j)) / F(3, j);
                else if (m == nmax - 3) v = (yv - XX(j + 1) * F(4, j) - XX(j + 2) * F(5, j)) / F(3, j);
                else v = (yv - XX(j + 1) * F(4, j) - XX(j + 2) * F(5, j) - XX(j + 3) * F(6, j)) / F(3, j);
            }
            x[(long long)j * nm] = v;
        }
        // ---- value at the free end, derivative at the given end (fdm_integral.f90:265-311); idl: centre of the integral system ----
        auto X = [&](int j) { return x[(long long)j * nm]; };
        if (BC == 2) {
            double r0 = bcs_b;
            for (int ic = 1; ic <= idl - 1; ++ic) r0 = r0 + F(idl + ic - 1, 0) * X(ic);
            r0 = r0 + F(0, 0) * X(idl);
            x[0] = r0;
            x[(long long)(n - 1) * nm] = resN[l];
            if (a.du) {
                double du = F(idl - 1, n - 1) * resN[l];
                for (int ic = 1; ic <= idl - 1; ++ic) du = du + F(idl - ic - 1, n - 1) * X(n - 1 - ic);
                du = du + F(ndi - 1, n - 1) * X(n - 1 - idl);
                for (int ic = 1; ic <= idr - 1; ++ic) du = du + Rr(n - 1, idr - ic) * fv(n - 1 - ic, l);
                a.du[(long long)l * nm + t] = du;
            }
        } else {
            double rN = bcs_t;
            for (int ic = 1; ic <= idl - 1; ++ic) rN = rN + F(idl - ic - 1, n - 1) * X(n - 1 - ic);
            rN = rN + F(ndi - 1, n - 1) * X(n - 1 - idl);
            x[(long long)(n - 1) * nm] = rN;
            x[0] = res0[l];
            if (a.du) {
                double du = F(idl - 1, 0) * res0[l];
                for (int ic = 1; ic <= idl - 1; ++ic) du = du + F(idl + ic - 1, 0) * X(ic);
                du = du + F(0, 0) * X(idl);
                for (int ic = 1; ic <= idr - 1; ++ic) du = du + Rr(0, idr + ic) * fv(ic, l);
                a.du[(long long)l * nm + t] = du;
            }
        }
    }
}

template <int BC, int NL, int FS>
void launch_int1(const Int1Args &a, hipStream_t st) {
    const int grid = (int)((a.nm + 255) / 256);
    // operand traffic of one integral solve: read NL lines, write NL lines (scratch traffic is overhead, not algorithmic)
    const bool few = a.nm <= 8;   // the <= 4 singular modes, solved beside the regular ones on the side stream
    ProfScope ps(few ? "k_int1<singular modes>" : (FS == FS_FIELD ? "k_int1<field>" : (FS == FS_LINEAR ? "k_int1<linear>" : "k_int1<unit>")), st,
                 (double)a.nm * a.T.n * 16.0 * NL);
    if (a.g_fac) {
        if (a.g_ndi == 3) hipLaunchKernelGGL((k_int1g<BC, NL, FS, 3>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_int1g<BC, NL, FS, 7>), dim3(grid), dim3(256), 0, st, a);
    } else if (a.fac && NL == 2 && a.nm <= 2048) {      // the low-mode sub-plan: one line per thread
        // four rows per line (source / factors of the sweep, intermediate) + the rhs coefficients; at most what is left of a CU beside one workgroup of k_ode_nn
        auto lds_of = [&](int lv) { return ((size_t)lv * 4 * a.T.n + (size_t)2 * a.T.n) * sizeof(double); };
        if constexpr (FS != FS_UNIT) {
            auto go = [&](auto lv_c) {
                constexpr int LV = decltype(lv_c)::value;
                allow_max_lds<&k_int1<BC, 1, FS, 8, true, true, true, LV>>();
                hipLaunchKernelGGL((k_int1<BC, 1, FS, 8, true, true, true, LV>), dim3((unsigned)((2 * a.nm + LV - 1) / LV)), dim3(256), lds_of(LV), st, a);
                hipc(hipGetLastError(), "k_int1 (LDS)");
            };
            if (lds_of(4) <= (size_t)84 * 1024) { go(std::integral_constant<int, 4>{}); return; }
            if (lds_of(2) <= (size_t)84 * 1024) { go(std::integral_constant<int, 2>{}); return; }
        }
        hipLaunchKernelGGL((k_int1<BC, 1, FS, 8, true, true>), dim3((unsigned)((2 * a.nm + 127) / 128)), dim3(128), 0, st, a);      // FS_UNIT, or lines too long for the LDS form
    } else if (a.fac) {
        if (a.nm < 65536) hipLaunchKernelGGL((k_int1<BC, NL, FS, 8, true>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_int1<BC, NL, FS, 2, true>), dim3(grid), dim3(256), 0, st, a);
    } else {
        if (a.nm < 65536) hipLaunchKernelGGL((k_int1<BC, NL, FS, 8, false>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_int1<BC, NL, FS, 2, false>), dim3(grid), dim3(256), 0, st, a);
    }
    hipc(hipGetLastError(), "k_int1");
}

// the combinations the solver uses (poisson_plan.hpp declares the template for the other files)
template void launch_int1<1, 2, FS_FIELD>(const Int1Args &, hipStream_t);
template void launch_int1<1, 2, FS_LINEAR>(const Int1Args &, hipStream_t);
template void launch_int1<2, 2, FS_LINEAR>(const Int1Args &, hipStream_t);
template void launch_int1<2, 3, FS_LINEAR>(const Int1Args &, hipStream_t);
template void launch_int1<1, 2, FS_UNIT>(const Int1Args &, hipStream_t);
template void launch_int1<2, 2, FS_UNIT>(const Int1Args &, hipStream_t);

}  // namespace tlab
