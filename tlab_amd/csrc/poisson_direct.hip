// The DIRECT elliptic solver of the Poisson plan (poisson.hip): k_int2 (marching), k_int2c (chunked) and the stage that launches them.
#include "poisson_dev.hpp"

namespace tlab {

// ================================================================================================
// k_int2 : FDM_Int2_Solve of the DIRECT elliptic solver (EllipticOrder = CompactDirect6; OPR_Poisson_FourierXZ_Direct,
// opr_elliptic.f90:368-455): ONE pentadiagonal solve per Fourier mode, (B - lambda2 A) p^ = A f^ with both boundary data in the wall
// planes of f^.  Same marching scheme as k_int1 (thread = mode, LU of the mode regenerated on the fly, forward-substituted line and U
// factors through a scratch array), and the solution goes straight into the spectral field p^ (no superposition stage).  The Neumann
// problem amplifies last-bit differences of the matrix entries and of the elimination to 1e-12 .. 5e-12 in p (measured with an affine
// table and fused multiply-adds), so this kernel repeats the reference's operations in the reference's order with FP contraction OFF:
// given the same f^ it returns the same bits as FDM_Int2_Initialize + FDM_Int2_Solve on the CPU.
// ================================================================================================
struct Int2Args {
    Int2Dev T;
    const double *lam;      // [nm] lambda2 = mwn2_x + mwn2_z of each mode
    double alpha;           // Helmholtz: the system constant is lambda2 - alpha (opr_elliptic.f90:604); 0 for Poisson
    long long nm;           // modes of the spectral box
    long long first, count; // threads cover modes [first, first + count)
    long long skip;         // mode left out (the singular one, solved by its own launch with the BCS_DN tables), or -1
    const double *fsrc;     // complex field (nxh, ny, nz)
    double *dst;            // complex field (nxh, ny, nz); may alias fsrc (a thread reads its whole column before it writes it)
    double fscale;          // 1/(nx*nz) (opr_elliptic.f90:402)
    int nxh, ny;
    int zero_bottom;        // compatibility constraint of the singular mode: p = 0 at the bottom (opr_elliptic.f90:420-421)
    int neumann_b, neumann_t;
    double *scratch;        // SoA [(k*n + j)*nm + t], k < 5
};

template <int U>
__global__ void __launch_bounds__(256) k_int2(Int2Args a) {
#pragma clang fp contract(off)
    const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.count) return;
    const long long t = a.first + q;
    if (t == a.skip) return;
    const int n = a.T.n;
    const long long nm = a.nm;
    const double lam = a.lam[t] - a.alpha;
    const long long fidx0 = (t % a.nxh) + (long long)a.nxh * a.ny * (t / a.nxh);
    const double2 *__restrict__ fs = reinterpret_cast<const double2 *>(a.fsrc);
    auto loadf = [&](int j, double (&f)[2]) {
        const double2 v = fs[fidx0 + (long long)j * a.nxh];
        f[0] = v.x * a.fscale; f[1] = v.y * a.fscale;
    };
    // rows 1 and n of the Neumann system (fdm_integral.f90:446-452, 485-491)
    double l1[3] = {a.T.c1[0], a.T.c1[1], a.T.c1[2]}, lN[3] = {a.T.cn[0], a.T.cn[1], a.T.cn[2]};
    l1[0] = l1[0] + lam * a.T.e1;
    lN[2] = lN[2] + lam * a.T.en;
    double res0[2], resN[2], fm[2] = {0.0, 0.0}, fc[2], fp[2];
    loadf(0, res0); loadf(n - 1, resN);                       // u(1:2) = f(1:2), u(2ny-1:2ny) = f(...) (opr_elliptic.f90:416-417)
    if (a.zero_bottom) res0[0] = res0[1] = 0.0;
    loadf(1, fc); loadf(2, fp);
    double bcs_b[2], bcs_t[2] = {0.0, 0.0};
#pragma unroll
    for (int l = 0; l < 2; ++l) bcs_b[l] = res0[l] * a.T.rb[0][2] + fc[l] * a.T.rb[0][3] + fp[l] * a.T.rb[0][1];   // MatMul_3d, BCS_BOTH

    // ---- forward: right-hand side (MatMul_3d), LU on the fly (PENTADFS), forward substitution (PENTADSS) ----
    double c1 = 0.0, c2 = 0.0, d1 = 0.0, d2 = 0.0, e1 = 0.0, e2 = 0.0;
    double y1[2] = {0.0, 0.0}, y2[2] = {0.0, 0.0};
    const int nmax = n - 2;
    for (int jb = 1; jb <= nmax; jb += U) {
        double fqb[U][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int jr = jb + u + 2;
            if (jr <= n - 1) loadf(jr, fqb[u]);
            else fqb[u][0] = fqb[u][1] = 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = jb + u;
            if (j > nmax) break;
            double r[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) r[k] = a.T.Bt[j * 5 + k] - lam * a.T.A5[j * 5 + k];      // :412-432
            if (a.neumann_b && (j == 1 || j == 2)) {       // rows 2, 3: lhs(1+ir, idr-ir+1 : idr-ir+3) -= rhs_b(1+ir, idl-ir) * lhs(1, 1:3)  (:462-464)
                const int k0 = 3 - j;
#pragma unroll
                for (int qq = 0; qq < 3; ++qq) r[k0 + qq] = r[k0 + qq] - a.T.nb[j - 1] * l1[qq];
            }
            if (a.neumann_t && (j == n - 2 || j == n - 3)) {   // rows n-1, n-2: lhs(nx-ir, ir : ir+2) -= rhs_t(idl-ir, idl+ir) * lhs(nx, ndr-2:ndr)  (:501-503)
                const int ir = n - 1 - j;
#pragma unroll
                for (int qq = 0; qq < 3; ++qq) r[ir - 1 + qq] = r[ir - 1 + qq] - a.T.nt[ir - 1] * lN[qq];
            }
            {
                const double sj = a.T.s[j];                  // :518-540
#pragma unroll
                for (int k = 0; k < 5; ++k) r[k] = r[k] * sj;
            }
            double rhs[2];
#pragma unroll
            for (int l = 0; l < 2; ++l) {
                if (j == 1) rhs[l] = res0[l] * a.T.rb[1][1] + fc[l] * a.T.rb[1][2] + fp[l] * a.T.rb[1][3];
                else if (j == 2) rhs[l] = res0[l] * a.T.rb[2][0] + fm[l] * a.T.rb[2][1] + fc[l] * a.T.rb[2][2] + fp[l] * a.T.rb[2][3];
                else if (j == n - 3) rhs[l] = fm[l] * a.T.rt[0][0] + fc[l] * a.T.rt[0][1] + fp[l] * a.T.rt[0][2] + resN[l] * a.T.rt[0][3];
                else if (j == n - 2) rhs[l] = fm[l] * a.T.rt[1][0] + fc[l] * a.T.rt[1][1] + resN[l] * a.T.rt[1][2];
                else rhs[l] = fm[l] * a.T.R[j * 3 + 0] + fc[l] * a.T.R[j * 3 + 1] + fp[l];
            }
            if (j == n - 2) {
#pragma unroll
                for (int l = 0; l < 2; ++l) bcs_t[l] = fm[l] * a.T.rt[2][2] + fc[l] * a.T.rt[2][0] + resN[l] * a.T.rt[2][1];
            }
            double am = 0.0, bm = 0.0, cm = r[2], dm = r[3], em = r[4];
            if (j == 2) {
                bm = r[1] / c1;
                cm = r[2] - bm * d1;
                dm = r[3] - bm * e1;
            } else if (j >= 3) {
                am = r[0] / c2;
                bm = (r[1] - am * d2) / c1;
                cm = r[2] - bm * d1 - am * e2;
                dm = r[3] - bm * e1;
            }
            const double cinv = 1.0 / cm;
#pragma unroll
            for (int l = 0; l < 2; ++l) {
                const double y = rhs[l] - y1[l] * bm - y2[l] * am;
                a.scratch[((long long)l * n + j) * nm + t] = y;
                y2[l] = y1[l];
                y1[l] = y;
            }
            a.scratch[((long long)2 * n + j) * nm + t] = cinv;
            a.scratch[((long long)3 * n + j) * nm + t] = -dm;
            a.scratch[((long long)4 * n + j) * nm + t] = -em;
            c2 = c1; d2 = d1; e2 = e1;
            c1 = cm; d1 = dm; e1 = em;
#pragma unroll
            for (int l = 0; l < 2; ++l) { fm[l] = fc[l]; fc[l] = fp[l]; fp[l] = fqb[u][l]; }
        }
    }

    // ---- backward substitution, straight into the spectral field ----
    double2 *__restrict__ ds = reinterpret_cast<double2 *>(a.dst);
    double x1[2] = {0.0, 0.0}, x2[2] = {0.0, 0.0};
    double xs[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};     // x[1..3]
    double xe[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};     // x[n-2], x[n-3], x[n-4]
    for (int jb = nmax; jb >= 1; jb -= U) {
        double yb[U][2], cb[U], db[U], eb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = jb - u;
            const int jr = j >= 1 ? j : 1;
            cb[u] = a.scratch[((long long)2 * n + jr) * nm + t];
            db[u] = a.scratch[((long long)3 * n + jr) * nm + t];
            eb[u] = a.scratch[((long long)4 * n + jr) * nm + t];
            yb[u][0] = a.scratch[((long long)0 * n + jr) * nm + t];
            yb[u][1] = a.scratch[((long long)1 * n + jr) * nm + t];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = jb - u;
            if (j < 1) break;
            double x[2];
#pragma unroll
            for (int l = 0; l < 2; ++l) {
                x[l] = (yb[u][l] + x1[l] * db[u] + x2[l] * eb[u]) * cb[u];
                x2[l] = x1[l];
                x1[l] = x[l];
                if (j <= 3) xs[j - 1][l] = x[l];
                if (j >= n - 4) xe[n - 2 - j][l] = x[l];
            }
            ds[fidx0 + (long long)j * a.nxh] = make_double2(x[0], x[1]);
        }
    }

    // ---- end values: given (Dirichlet) or from the biased first-derivative formula (Neumann), fdm_integral.f90:659-668 ----
    double r0[2], rN[2];
#pragma unroll
    for (int l = 0; l < 2; ++l) { r0[l] = res0[l]; rN[l] = resN[l]; }
    if (a.neumann_b) {
#pragma unroll
        for (int l = 0; l < 2; ++l) r0[l] = bcs_b[l] + l1[0] * xs[0][l] + l1[1] * xs[1][l] + l1[2] * xs[2][l];
    }
    if (a.neumann_t) {
#pragma unroll
        for (int l = 0; l < 2; ++l) rN[l] = bcs_t[l] + lN[2] * xe[0][l] + lN[1] * xe[1][l] + lN[0] * xe[2][l];
    }
    ds[fidx0] = make_double2(r0[0], r0[1]);
    ds[fidx0 + (long long)(n - 1) * a.nxh] = make_double2(rN[0], rN[1]);
}

// ================================================================================================
// k_int2c : FDM_Int2_Solve (the DIRECT elliptic solver, k_int2 above) on the chunked scheme of k_ode_nn: ONE pentadiagonal system per mode,
// thread (mode m, chunk c) owns 8 rows, the PENTADFS pivots of its rows regenerated from a checkpoint of the serial recurrence, forward and
// backward substitution as particular end values + 2 x 2 transfer matrix, parallel scan over the chunks (ode_chain), repeat with the inflow.
// Rows and right-hand sides are built exactly as k_int2 builds them (same operations, no contraction); what differs from the marching kernel is
// the association of the substitution sums.  No scratch: f^ 16 B in, p^ 16 B out, checkpoints 6 B per mode and row.
// ================================================================================================
struct Int2cArgs {
    Int2Dev T;
    const double *lam;
    double alpha;
    long long nm, skip;
    const double *chk;          // [blk][C][6][NM] PENTADFS state before the first row of each chunk
    const double *fsrc;
    double *dst;
    double fscale;
    int nxh, ny, C, neumann_b, neumann_t;
};

__device__ __forceinline__ void int2_row(const Int2Dev &T, int j, double lam, const double (&l1)[3], const double (&lN)[3], int nb_on, int nt_on,
                                         double (&r)[5]) {
#pragma clang fp contract(off)
    const int n = T.n;
#pragma unroll
    for (int k = 0; k < 5; ++k) r[k] = T.Bt[(unsigned)(j * 5 + k)] - lam * T.A5[(unsigned)(j * 5 + k)];      // fdm_integral.f90:412-432
    if (nb_on && (j == 1 || j == 2)) {       // :462-464
        const int k0 = 3 - j;
#pragma unroll
        for (int q = 0; q < 3; ++q) r[k0 + q] = r[k0 + q] - T.nb[j - 1] * l1[q];
    }
    if (nt_on && (j == n - 2 || j == n - 3)) {   // :501-503
        const int ir = n - 1 - j;
#pragma unroll
        for (int q = 0; q < 3; ++q) r[ir - 1 + q] = r[ir - 1 + q] - T.nt[ir - 1] * lN[q];
    }
    const double sj = T.s[j];                    // :518-540
#pragma unroll
    for (int k = 0; k < 5; ++k) r[k] = r[k] * sj;
}

// checkpoints of the factor recurrence of every mode: state before rows 8, 16, ...
__global__ void __launch_bounds__(256) k_int2_checkpoint(Int2Dev T, const double *__restrict__ lamv, double alpha, int nb_on, int nt_on,
                                                         double *__restrict__ chk, long long nm, int NM, int C) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nm) return;
    const int n = T.n;
    const double lam = lamv[t] - alpha;
    double l1[3] = {T.c1[0], T.c1[1], T.c1[2]}, lN[3] = {T.cn[0], T.cn[1], T.cn[2]};
    l1[0] = l1[0] + lam * T.e1;
    lN[2] = lN[2] + lam * T.en;
    double st[6] = {0, 0, 0, 0, 0, 0};
    for (int j = 1; j <= n - 2; ++j) {
        if ((j % OM) == 0) {
            const int c = j / OM;
#pragma unroll
            for (int q = 0; q < 6; ++q) chk[(((t / NM) * C + c) * 6 + q) * NM + (t % NM)] = st[q];
        }
        double r[5], am, bm, cinv, nd, ne;
        int2_row(T, j, lam, l1, lN, nb_on, nt_on, r);
        ode_factor_step(j, r, st, am, bm, cinv, nd, ne);
    }
}

template <int NM>
__global__ void __launch_bounds__(512) k_int2c(Int2cArgs a) {
    extern __shared__ double lds[];
    const int C = a.C, n = a.T.n;
    const int m = threadIdx.x % NM, c = threadIdx.x / NM;
    double *s_w = lds, *s_fac = lds + 8 * 8 * NM;
    const int nm = (int)a.nm;
    int t = (int)blockIdx.x * NM + m;
    const bool live = t < nm;
    if (!live) t = nm - 1;
    const bool store = live && ((long long)t != a.skip);
    const double lam = a.lam[t] - a.alpha;
    const unsigned fidx0 = (unsigned)((t % a.nxh) + a.nxh * a.ny * (t / a.nxh));
    const int j0 = c * OM;
    const bool lo = (c == 0), hi = (c == C - 1);
    const double2 *F = reinterpret_cast<const double2 *>(a.fsrc);
    double fl[OM + 2][2];        // f rows j0-1 .. j0+8 (normalised)
#pragma unroll
    for (int p = 0; p < OM + 2; ++p) {
        const int j = j0 - 1 + p;
        double2 w = make_double2(0.0, 0.0);
        if (j >= 0 && j <= n - 1) w = F[fidx0 + (unsigned)(j * a.nxh)];
        fl[p][0] = w.x * a.fscale; fl[p][1] = w.y * a.fscale;
    }
    const double res0[2] = {fl[1][0], fl[1][1]}, resN[2] = {fl[OM][0], fl[OM][1]};      // rows 0 / n-1: meaningful in the first / last chunk only
    double l1[3] = {a.T.c1[0], a.T.c1[1], a.T.c1[2]}, lN[3] = {a.T.cn[0], a.T.cn[1], a.T.cn[2]};
    l1[0] = nf_madd(l1[0], lam, a.T.e1);
    lN[2] = nf_madd(lN[2], lam, a.T.en);
    double bcs_b[2] = {0, 0}, bcs_t[2] = {0, 0};
    // ---- factors of my rows from the checkpoint, right-hand side ----
    double st[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) st[q] = (c == 0) ? 0.0 : a.chk[(unsigned)((((t / NM) * C + c) * 6 + q) * NM + m)];
    double am[OM], bm[OM], x[OM][2];
    double *my_fac = s_fac + threadIdx.x * (3 * OM + 1);
#define FAC(p, q) my_fac[(p) * 3 + (q)]
#pragma unroll
    for (int p = 0; p < OM; ++p) {
        const int j = j0 + p;
        const bool off = (p == 0 && lo) || (p == OM - 1 && hi);
        double r[5];
        int2_row(a.T, j, lam, l1, lN, a.neumann_b, a.neumann_t, r);
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
        for (int l = 0; l < 2; ++l) {
#pragma clang fp contract(off)
            const double fm = fl[p][l], fc = fl[p + 1][l], fp = fl[p + 2][l];
            double v = fm * a.T.R[(unsigned)(j * 3 + 0)] + fc * a.T.R[(unsigned)(j * 3 + 1)] + fp;      // MatMul_3d interior row
            if (p == 1 && lo) v = res0[l] * a.T.rb[1][1] + fc * a.T.rb[1][2] + fp * a.T.rb[1][3];
            if (p == 2 && lo) v = res0[l] * a.T.rb[2][0] + fm * a.T.rb[2][1] + fc * a.T.rb[2][2] + fp * a.T.rb[2][3];
            if (p == OM - 3 && hi) v = fm * a.T.rt[0][0] + fc * a.T.rt[0][1] + fp * a.T.rt[0][2] + resN[l] * a.T.rt[0][3];
            if (p == OM - 2 && hi) v = fm * a.T.rt[1][0] + fc * a.T.rt[1][1] + resN[l] * a.T.rt[1][2];
            x[p][l] = off ? 0.0 : v;
            if (p == 1 && lo) bcs_b[l] = res0[l] * a.T.rb[0][2] + fc * a.T.rb[0][3] + fp * a.T.rb[0][1];
            if (p == OM - 2 && hi) bcs_t[l] = fm * a.T.rt[2][2] + fc * a.T.rt[2][0] + resN[l] * a.T.rt[2][1];
        }
        if (p & 1) __builtin_amdgcn_sched_barrier(0);
    }
    // ---- forward substitution ----
    double inflow[2][2];
    {
        double y1[2] = {0, 0}, y2[2] = {0, 0};
        double h1a = 1.0, h2a = 0.0, h1b = 0.0, h2b = 1.0;
#pragma unroll
        for (int p = 0; p < OM; ++p) {
#pragma unroll
            for (int l = 0; l < 2; ++l) {
                const double y = x[p][l] - y1[l] * bm[p] - y2[l] * am[p];
                y2[l] = y1[l]; y1[l] = y;
            }
            const double ha = -h1a * bm[p] - h2a * am[p]; h2a = h1a; h1a = ha;
            const double hb = -h1b * bm[p] - h2b * am[p]; h2b = h1b; h1b = hb;
        }
        double phi[4] = {h1a, h1b, h2a, h2b}, ee[2][2] = {{y1[0], y2[0]}, {y1[1], y2[1]}};
        ode_chain<NM, +1>(phi, ee, c, C, m, s_w, inflow);
    }
    {
        double y1[2] = {inflow[0][0], inflow[1][0]}, y2[2] = {inflow[0][1], inflow[1][1]};
#pragma unroll
        for (int p = 0; p < OM; ++p)
#pragma unroll
            for (int l = 0; l < 2; ++l) {
                const double v = x[p][l] - y1[l] * bm[p] - y2[l] * am[p];
                x[p][l] = v; y2[l] = y1[l]; y1[l] = v;
            }
    }
    __syncthreads();
    // ---- backward substitution ----
    {
        double x1[2] = {0, 0}, x2[2] = {0, 0};
        double h1a = 1.0, h2a = 0.0, h1b = 0.0, h2b = 1.0;
#pragma unroll
        for (int p = OM - 1; p >= 0; --p) {
            const double cinv_p = FAC(p, 0), nd_p = FAC(p, 1), ne_p = FAC(p, 2);
#pragma unroll
            for (int l = 0; l < 2; ++l) {
                const double v = (x[p][l] + x1[l] * nd_p + x2[l] * ne_p) * cinv_p;
                x2[l] = x1[l]; x1[l] = v;
            }
            const double ha = (h1a * nd_p + h2a * ne_p) * cinv_p; h2a = h1a; h1a = ha;
            const double hb = (h1b * nd_p + h2b * ne_p) * cinv_p; h2b = h1b; h1b = hb;
        }
        double phi[4] = {h1a, h1b, h2a, h2b}, ee[2][2] = {{x1[0], x2[0]}, {x1[1], x2[1]}};
        ode_chain<NM, -1>(phi, ee, c, C, m, s_w, inflow);
    }
    {
        double x1[2] = {inflow[0][0], inflow[1][0]}, x2[2] = {inflow[0][1], inflow[1][1]};
#pragma unroll
        for (int p = OM - 1; p >= 0; --p) {
            const double cinv_p = FAC(p, 0), nd_p = FAC(p, 1), ne_p = FAC(p, 2);
#pragma unroll
            for (int l = 0; l < 2; ++l) {
                const double v = (x[p][l] + x1[l] * nd_p + x2[l] * ne_p) * cinv_p;
                x[p][l] = v; x2[l] = x1[l]; x1[l] = v;
            }
        }
    }
#undef FAC
    // ---- end values: given (Dirichlet) or from the biased first-derivative formula (Neumann), fdm_integral.f90:659-668 ----
#pragma unroll
    for (int l = 0; l < 2; ++l) {
#pragma clang fp contract(off)
        if (lo) x[0][l] = a.neumann_b ? bcs_b[l] + l1[0] * x[1][l] + l1[1] * x[2][l] + l1[2] * x[3][l] : res0[l];
        if (hi) x[OM - 1][l] = a.neumann_t ? bcs_t[l] + lN[2] * x[OM - 2][l] + lN[1] * x[OM - 3][l] + lN[0] * x[OM - 4][l] : resN[l];
    }
    if (!store) return;
    double2 *D = reinterpret_cast<double2 *>(a.dst);
#pragma unroll
    for (int p = 0; p < OM; ++p) D[fidx0 + (unsigned)((j0 + p) * a.nxh)] = make_double2(x[p][0], x[p][1]);
}

// FDM_Int2_Solve of every local mode (opr_elliptic.f90:413-434)
// helmholtz: OPR_Helmholtz_FourierXZ_Direct (:562-628): system constant lambda2 - alpha for every mode, no singular-mode treatment
void poisson_direct_stage(tlab_poisson_plan_t P, int ibc, double *f_hat, double *p_hat, hipStream_t st, bool helmholtz, double alpha) {
    Int2Args a{};
    a.T = P->dev2(ibc);
    a.lam = P->lam.p; a.nm = P->nm; a.first = 0; a.count = P->nm;
    a.alpha = helmholtz ? alpha : 0.0;
    a.skip = (ibc == TLAB_BCS_NN && !helmholtz) ? P->sing_direct : -1;   // singular mode: BCS_DN system with p = 0 at the bottom (:236-240, :420-424)
    a.fsrc = f_hat; a.dst = p_hat; a.fscale = P->norm; a.nxh = P->nxh; a.ny = P->ny;
    a.zero_bottom = 0;
    a.neumann_b = (ibc == TLAB_BCS_ND || ibc == TLAB_BCS_NN) ? 1 : 0;
    a.neumann_t = (ibc == TLAB_BCS_DN || ibc == TLAB_BCS_NN) ? 1 : 0;
    a.scratch = P->scratch.p;
    // chunked kernel (k_int2c) where the line splits into 8-row chunks and 32-bit indices suffice; TLAB_INT2_CHUNKED=0 (read per call) or
    // tlab_poisson_set_exact(1) keep the marching kernel, which repeats the reference's operation order
    const int C = P->ny / OM, NM = (P->ny % OM == 0 && P->ny >= 2 * OM) ? ode_modes_per_wg(C) : 0;
    const bool chunked = NM > 0 && env_int("TLAB_INT2_CHUNKED", 1) != 0 && !P->exact_mode && (double)P->nm * P->ny * 2.0 < 2.0e9;
    if (chunked) {
        auto &E = *P->int2[ibc];
        const long long nblk = (P->nm + NM - 1) / NM;
        if (!E.chk_ok || E.chk_alpha != a.alpha) {
            if (E.chk.n != (size_t)C * 6 * nblk * NM) E.chk.alloc((size_t)C * 6 * nblk * NM);
            hipLaunchKernelGGL(k_int2_checkpoint, dim3((unsigned)((P->nm + 255) / 256)), dim3(256), 0, st, a.T, P->lam.p, a.alpha, a.neumann_b, a.neumann_t,
                               E.chk.p, P->nm, NM, C);
            hipc(hipGetLastError(), "k_int2_checkpoint");
            E.chk_alpha = a.alpha; E.chk_ok = true;
        }
        Int2cArgs k{};
        k.T = a.T; k.lam = a.lam; k.alpha = a.alpha; k.nm = P->nm; k.skip = a.skip; k.chk = E.chk.p; k.fsrc = f_hat; k.dst = p_hat; k.fscale = a.fscale;
        k.nxh = a.nxh; k.ny = a.ny; k.C = C; k.neumann_b = a.neumann_b; k.neumann_t = a.neumann_t;
        const size_t lds = ((size_t)64 * NM + (size_t)(3 * OM + 1) * NM * C) * sizeof(double);
        ProfScope ps("k_int2c", st, (double)P->nm * P->ny * 32.0);
        dispatch_nm(NM, [&](auto nm_c) {
            constexpr int N = decltype(nm_c)::value;
            allow_max_lds<&k_int2c<N>>();
            hipLaunchKernelGGL((k_int2c<N>), dim3((unsigned)((k.nm + N - 1) / N)), dim3(N * k.C), lds, st, k);
        });
    } else {
        ProfScope ps("k_int2", st, (double)P->nm * P->ny * 32.0);
        hipLaunchKernelGGL((k_int2<4>), dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, st, a);
    }
    if (a.skip >= 0) {
        Int2Args b = a;
        b.T = P->dev2(TLAB_BCS_DN);
        b.first = a.skip; b.count = 1; b.skip = -1; b.zero_bottom = 1; b.neumann_b = 0; b.neumann_t = 1;
        hipLaunchKernelGGL((k_int2<4>), dim3(1), dim3(64), 0, st, b);
    }
    hipc(hipGetLastError(), "k_int2");
}

}  // namespace tlab
