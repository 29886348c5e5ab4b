// OPR_Poisson_FourierXZ_Factorize (operators/opr_elliptic.f90:263-364) on the MI355X.
//
//   p  --rocFFT r2c (x)-->  --rocFFT c2c (z)-->  f^(kx, j, kz)            (OPR_Fourier_X/Z_Forward, opr_fourier.f90:219,333)
//   per Fourier mode: (d/dy + l)(d/dy - l) p^ = f^,  l = sqrt(kx'^2 + kz'^2)  (OPR_ODE2_Factorize_NN, opr_odes.f90:265-386)
//   p^, dp^/dy --c2c (z)--> --c2r (x)--> p, dpdy                          (OPR_Fourier_Z/X_Backward)
//
// The reference transposes the spectral array so that each mode's y-line is contiguous and loops over modes on one
// core.  Here a mode is a THREAD: modes (kx fastest) lie across the lanes, y is the slow index, so every access is a
// coalesced 16-B-per-lane row and no transpose is needed.  Each first-order integral solve (FDM_Int1_Solve,
// fdm_integral.f90:219-314: tridiagonal matmul + pentadiagonal solve whose matrix B + l A depends on the mode) is one
// kernel: the pentadiagonal LU (PENTADFS, linear5.f90:30-71) is recomputed on the fly per mode instead of being
// stored (the reference stores 2 LUs per mode = 5.4 GB at 512^3), the forward-substituted lines and the three U
// factors per row go through a scratch array, the backward sweep reads them back.  The three homogeneous solutions
// the reference recomputes on every call (opr_odes.f90:308-324) depend only on the mode and are computed once at plan
// creation.
//
// Files: this one holds plan creation, the rocFFT plans, the small gather / scatter / combine / constants kernels with the marching-route stages that
// launch them, and the C entry points; poisson_int1.hip the marching integral solves (k_int1, k_int1g), poisson_ode.hip the chunked solver (k_ode_nn,
// k_ode_sing), poisson_direct.hip the direct solver (k_int2, k_int2c); poisson_plan.hpp / poisson_dev.hpp what they share on the host / the device.
#include "poisson_plan.hpp"

namespace tlab {

// ------------------------------------------------------------------------------------------------
// per-mode constants of OPR_ODE2_Factorize_NN: LU of the 3x3 constraint matrix (opr_odes.f90:329-348)
// hom: SoA [(c*n + j)*nm + t], c = 0 v1, 1 em, 2 u1, 3 sp, 4 ep ; der: [(c*nm + t)], c = 0 du1_n, 1 dsp_n, 2 dep_n
// cst: [(c*nm + t)], c = 0..8 = a11 a21 a31 a12 a22 a32 a13 a23 a33 (after the LU)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_nn_constants(const double *__restrict__ hom, const double *__restrict__ der,
                                                      const double *__restrict__ lamv, double *__restrict__ cst, int n, long long nm) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nm) return;
    const double lam = lamv[t];
    auto H = [&](int c, int j) { return hom[((long long)c * n + j) * nm + t]; };
    double a11 = 1.0 + lam * H(3, 0), a21 = H(1, n - 1), a31 = der[1 * nm + t];
    double a12 = lam * H(4, 0), a22 = lam, a32 = der[2 * nm + t];
    double a13 = lam * H(2, 0), a23 = H(0, n - 1), a33 = der[0 * nm + t];
    a12 = a12 / a11;
    a22 = a22 - a21 * a12;
    a32 = a32 - a31 * a12;
    a13 = a13 / a11;
    a23 = (a23 - a21 * a13) / a22;
    a33 = a33 - a31 * a13 - a32 * a23;
    cst[0 * nm + t] = a11; cst[1 * nm + t] = a21; cst[2 * nm + t] = a31;
    cst[3 * nm + t] = a12; cst[4 * nm + t] = a22; cst[5 * nm + t] = a32;
    cst[6 * nm + t] = a13; cst[7 * nm + t] = a23; cst[8 * nm + t] = a33;
}

// ------------------------------------------------------------------------------------------------
// superposition (opr_odes.f90:350-367): writes p^ and dp^/dy in the spectral field layout.
// u0, v0: SoA [(l*n + j)*nm + t] (l = Re, Im); du0: [(l*nm + t)]; bcs: [(c*nm + t)] c = ReB, ImB, ReT, ImT
// ------------------------------------------------------------------------------------------------
struct CombineArgs {
    const double *u0, *v0, *du0, *bcs, *hom, *cst, *lam;
    const unsigned char *skip;   // [nm]: 1 for the singular modes (handled separately)
    double *p_hat, *dp_hat;      // complex fields (nxh, ny, nz)
    int n, nxh, ny;
    long long nm;
};

__global__ void __launch_bounds__(256) k_nn_combine(CombineArgs a) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.nm) return;
    if (a.skip[t]) return;
    const int n = a.n;
    const long long nm = a.nm;
    const double lam = a.lam[t];
    const long long fidx0 = (t % a.nxh) + (long long)a.nxh * a.ny * (t / a.nxh);
    const double a11 = a.cst[0 * nm + t], a21 = a.cst[1 * nm + t], a31 = a.cst[2 * nm + t];
    const double a12 = a.cst[3 * nm + t], a22 = a.cst[4 * nm + t], a32 = a.cst[5 * nm + t];
    const double a13 = a.cst[6 * nm + t], a23 = a.cst[7 * nm + t], a33 = a.cst[8 * nm + t];
    double v_1[2], u_n[2], fn[2];
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        const double bb = a.bcs[(long long)l * nm + t], bt = a.bcs[(long long)(2 + l) * nm + t];
        const double u0_1 = a.u0[((long long)l * n + 0) * nm + t];
        const double v0_n = a.v0[((long long)l * n + (n - 1)) * nm + t];
        const double du0n = a.du0[(long long)l * nm + t];
        v_1[l] = (bb - lam * u0_1) / a11;
        u_n[l] = (bt - v0_n - a21 * v_1[l]) / a22;
        fn[l] = (bt - du0n - a31 * v_1[l] - a32 * u_n[l]) / a33;
        u_n[l] = u_n[l] - a23 * fn[l];
        v_1[l] = v_1[l] - a12 * u_n[l] - a13 * fn[l];
    }
    double2 *P = reinterpret_cast<double2 *>(a.p_hat), *D = reinterpret_cast<double2 *>(a.dp_hat);
    // rows [jlo, jhi) of this thread: gridDim.y row blocks (few modes: the rows are the parallelism; many modes: one block does them all)
    const int rows = (n + (int)gridDim.y - 1) / (int)gridDim.y;
    const int jlo = (int)blockIdx.y * rows, jhi = (jlo + rows < n) ? jlo + rows : n;
    for (int j = jlo; j < jhi; ++j) {
        const double hv1 = a.hom[((long long)0 * n + j) * nm + t], hem = a.hom[((long long)1 * n + j) * nm + t];
        const double hu1 = a.hom[((long long)2 * n + j) * nm + t], hsp = a.hom[((long long)3 * n + j) * nm + t];
        const double hep = a.hom[((long long)4 * n + j) * nm + t];
        double u[2], v[2];
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            const double u0 = a.u0[((long long)l * n + j) * nm + t], v0 = a.v0[((long long)l * n + j) * nm + t];
            if (j == n - 1) {
                u[l] = u_n[l];
                v[l] = v0 + fn[l] * hv1 + v_1[l] * hem + lam * u[l];
            } else if (j == 0) {
                u[l] = u0 + fn[l] * hu1 + v_1[l] * hsp + u_n[l] * hep;
                v[l] = v_1[l] + lam * u[l];
            } else {
                u[l] = u0 + fn[l] * hu1 + v_1[l] * hsp + u_n[l] * hep;
                v[l] = v0 + fn[l] * hv1 + v_1[l] * hem + lam * u[l];
            }
        }
        const long long idx = fidx0 + (long long)j * a.nxh;
        P[idx] = make_double2(u[0], u[1]);
        D[idx] = make_double2(v[0], v[1]);
    }
}

// ------------------------------------------------------------------------------------------------
// singular modes (lambda = 0: OPR_ODE2_Factorize_NN_Sing -> _DN_Sing, opr_odes.f90:165-183, 37-96): <= 4 modes
// ------------------------------------------------------------------------------------------------
// gather f^ * norm of the singular modes into SoA [(l*n + j)*ns + s], with row 0 zeroed (f(:,1) = 0), and the top BC
__global__ void k_sing_gather(const double *__restrict__ f_hat, const int *__restrict__ modes, int ns, int n, int nxh, int ny,
                              double scale, double *__restrict__ fs, double *__restrict__ bct) {
    const int s = blockIdx.x, j = threadIdx.x + blockIdx.y * blockDim.x;
    if (s >= ns || j >= n) return;
    const long long t = modes[s];
    const long long idx = (t % nxh) + (long long)nxh * ny * (t / nxh) + (long long)j * nxh;
    const double2 v = reinterpret_cast<const double2 *>(f_hat)[idx];
    fs[((long long)0 * n + j) * ns + s] = (j == 0) ? 0.0 : v.x * scale;
    fs[((long long)1 * n + j) * ns + s] = (j == 0) ? 0.0 : v.y * scale;
    if (j == n - 1) { bct[0 * ns + s] = v.x * scale; bct[1 * ns + s] = v.y * scale; }
}

// columns of a list of modes between the spectral field layout (nxh, ny, nz) and a compact (ns, ny, 1) field (low-mode sub-plan)
__global__ void k_modes_gather(const double2 *__restrict__ f_hat, const int *__restrict__ modes, int ns, int n, int nxh, int ny,
                               double2 *__restrict__ out) {
    const int s = threadIdx.x + blockIdx.x * blockDim.x, j = blockIdx.y;
    if (s >= ns || j >= n) return;
    const long long t = modes[s];
    out[(long long)j * ns + s] = f_hat[(t % nxh) + (long long)nxh * ny * (t / nxh) + (long long)j * nxh];
}
__global__ void k_modes_scatter(const double2 *__restrict__ p_low, const double2 *__restrict__ dp_low, const int *__restrict__ modes, int ns,
                                int n, int nxh, int ny, double2 *__restrict__ p_hat, double2 *__restrict__ dp_hat) {
    const int s = threadIdx.x + blockIdx.x * blockDim.x, j = blockIdx.y;
    if (s >= ns || j >= n) return;
    const long long t = modes[s];
    const long long idx = (t % nxh) + (long long)nxh * ny * (t / nxh) + (long long)j * nxh;
    p_hat[idx] = p_low[(long long)j * ns + s];
    dp_hat[idx] = dp_low[(long long)j * ns + s];
}

// u = u0 + c u1, v = v0 + c v1, c = (v0(1) - du0_n) / (du1_n - v1(1)); scatter into the spectral fields
__global__ void k_sing_combine(const double *__restrict__ u0, const double *__restrict__ v0, const double *__restrict__ u1,
                               const double *__restrict__ v1, const double *__restrict__ du0, const double *__restrict__ du1,
                               const int *__restrict__ modes, int ns, int n, int nxh, int ny, double *__restrict__ p_hat,
                               double *__restrict__ dp_hat) {
    const int s = blockIdx.x, j = threadIdx.x + blockIdx.y * blockDim.x;
    if (s >= ns || j >= n) return;
    const long long t = modes[s];
    const long long idx = (t % nxh) + (long long)nxh * ny * (t / nxh) + (long long)j * nxh;
    const double f1 = 1.0 / (du1[0 * ns + s] - v1[((long long)0 * n + 0) * ns + s]);
    double u[2], v[2];
    for (int l = 0; l < 2; ++l) {
        const double c = (v0[((long long)l * n + 0) * ns + s] - du0[l * ns + s]) * f1;
        u[l] = u0[((long long)l * n + j) * ns + s] + c * u1[((long long)0 * n + j) * ns + s];
        v[l] = v0[((long long)l * n + j) * ns + s] + c * v1[((long long)0 * n + j) * ns + s];
    }
    reinterpret_cast<double2 *>(p_hat)[idx] = make_double2(u[0], u[1]);
    reinterpret_cast<double2 *>(dp_hat)[idx] = make_double2(v[0], v[1]);
}

// ------------------------------------------------------------------------------------------------
// ibc = BCS_DD of the factorized solver: OPR_ODE2_Factorize_DD (opr_odes.f90:391-478) and _DD_Sing (:188-260).  Marching kernels only
// (the chunked kernel is the BCS_NN solver of the RHS); same two integral solves as BCS_NN with the top value of u given, other constants.
// ------------------------------------------------------------------------------------------------
struct DDCombineArgs {
    const double *u0, *v0, *du0, *bcs, *hom, *der, *lam;
    const int *sing;             // singular modes (handled separately)
    int ns;
    int hom_nm_block;            // 0: hom is SoA [(c*n + j)*nm + t]; NM > 0: blocked [blk][5][n][NM] (k_ode_block_layout)
    double *p_hat, *dp_hat;
    int n, nxh, ny;
    long long nm;
};

// constants of OPR_ODE2_Factorize_DD that depend on the mode only (opr_odes.f90:452-454), for the chunked kernel: cst[5][nm]
__global__ void __launch_bounds__(256) k_dd_constants(const double *__restrict__ hom, int hom_nm_block, const double *__restrict__ der,
                                                      double *__restrict__ cst, int n, long long nm) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nm) return;
    auto H = [&](int c, int j) {
        if (hom_nm_block > 0) {
            const int NM = hom_nm_block;
            return hom[(((t / NM) * 5 + c) * n + j) * NM + (t % NM)];
        }
        return hom[((long long)c * n + j) * nm + t];
    };
    const double aa = der[0 * nm + t] - H(0, n - 1);
    const double bb = der[1 * nm + t] - H(1, n - 1);
    cst[0 * nm + t] = aa;
    cst[1 * nm + t] = bb;
    cst[2 * nm + t] = 1.0 / (aa * H(3, 0) - bb * H(2, 0));
    cst[3 * nm + t] = H(3, 0);
    cst[4 * nm + t] = H(2, 0);
}

__global__ void __launch_bounds__(256) k_dd_combine(DDCombineArgs a) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.nm) return;
    for (int s = 0; s < a.ns; ++s)
        if (a.sing[s] == t) return;
    const int n = a.n;
    const long long nm = a.nm;
    const double lam = a.lam[t];
    const long long fidx0 = (t % a.nxh) + (long long)a.nxh * a.ny * (t / a.nxh);
    auto H = [&](int c, int j) {
        if (a.hom_nm_block > 0) {
            const int NM = a.hom_nm_block;
            return a.hom[(((t / NM) * 5 + c) * n + j) * NM + (t % NM)];
        }
        return a.hom[((long long)c * n + j) * nm + t];
    };
    // c = 0 v1, 1 em, 2 u1, 3 sp ; der: 0 du1_n, 1 dsp_n
    const double aa = a.der[0 * nm + t] - H(0, n - 1);
    const double bb = a.der[1 * nm + t] - H(1, n - 1);
    const double dummy = 1.0 / (aa * H(3, 0) - bb * H(2, 0));
    double q1[2], fn[2], bb_[2];
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        const double bcb = a.bcs[(long long)l * nm + t], bct = a.bcs[(long long)(2 + l) * nm + t];
        const double u0_1 = a.u0[((long long)l * n + 0) * nm + t];
        const double v0_n = a.v0[((long long)l * n + (n - 1)) * nm + t];
        const double w = lam * bct - a.du0[(long long)l * nm + t] + v0_n;
        q1[l] = (aa * (bcb - u0_1) - H(2, 0) * w) * dummy;
        fn[l] = (H(3, 0) * w - bb * (bcb - u0_1)) * dummy;
        bb_[l] = bcb;
    }
    double2 *P = reinterpret_cast<double2 *>(a.p_hat), *D = reinterpret_cast<double2 *>(a.dp_hat);
    const int rows = (n + (int)gridDim.y - 1) / (int)gridDim.y;      // row blocks as in k_nn_combine
    const int jlo = (int)blockIdx.y * rows, jhi = (jlo + rows < n) ? jlo + rows : n;
    for (int j = jhi - 1; j >= (jlo > 1 ? jlo : 1); --j) {
        const double hv1 = H(0, j), hem = H(1, j), hu1 = H(2, j), hsp = H(3, j);
        double u[2], v[2];
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            u[l] = a.u0[((long long)l * n + j) * nm + t] + fn[l] * hu1 + q1[l] * hsp;
            v[l] = a.v0[((long long)l * n + j) * nm + t] + fn[l] * hv1 + q1[l] * hem + lam * u[l];
        }
        P[fidx0 + (long long)j * a.nxh] = make_double2(u[0], u[1]);
        D[fidx0 + (long long)j * a.nxh] = make_double2(v[0], v[1]);
    }
    if (jlo == 0) {
        P[fidx0] = make_double2(bb_[0], bb_[1]);
        D[fidx0] = make_double2(q1[0] + lam * bb_[0], q1[1] + lam * bb_[1]);
    }
}

// singular modes: f^ * norm into SoA [(l*n + j)*ns + s] (all rows), bottom / top values into bcb / bct [l*ns + s]
__global__ void k_sing_gather_dd(const double *__restrict__ f_hat, const int *__restrict__ modes, int ns, int n, int nxh, int ny, double scale,
                                 double *__restrict__ fs, double *__restrict__ bcb, double *__restrict__ bct) {
    const int s = blockIdx.x, j = threadIdx.x + blockIdx.y * blockDim.x;
    if (s >= ns || j >= n) return;
    const long long t = modes[s];
    const double2 v = reinterpret_cast<const double2 *>(f_hat)[(t % nxh) + (long long)nxh * ny * (t / nxh) + (long long)j * nxh];
    fs[((long long)0 * n + j) * ns + s] = v.x * scale;
    fs[((long long)1 * n + j) * ns + s] = v.y * scale;
    if (j == 0) { bcb[0 * ns + s] = v.x * scale; bcb[1 * ns + s] = v.y * scale; }
    if (j == n - 1) { bct[0 * ns + s] = v.x * scale; bct[1 * ns + s] = v.y * scale; }
}
__global__ void k_fill_ones(double *__restrict__ a, long long m) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) a[i] = 1.0;
}
// opr_odes.f90:238-251
__global__ void k_sing_combine_dd(const double *__restrict__ u0, const double *__restrict__ v0, const double *__restrict__ u1,
                                  const double *__restrict__ v1, const double *__restrict__ sp, const double *__restrict__ du0,
                                  const double *__restrict__ du1, const double *__restrict__ bcb, const int *__restrict__ modes, int ns, int n,
                                  int nxh, int ny, double *__restrict__ p_hat, double *__restrict__ dp_hat) {
#pragma clang fp contract(off)
    const int s = blockIdx.x, j = threadIdx.x + blockIdx.y * blockDim.x;
    if (s >= ns || j >= n) return;
    const long long t = modes[s];
    const long long idx = (t % nxh) + (long long)nxh * ny * (t / nxh) + (long long)j * nxh;
    const double fn = 1.0 / (du1[0 * ns + s] - v1[((long long)0 * n + (n - 1)) * ns + s]);
    const double dummy = 1.0 / sp[((long long)0 * n + 0) * ns + s];
    double u[2], v[2];
    for (int l = 0; l < 2; ++l) {
        const double c = (v0[((long long)l * n + (n - 1)) * ns + s] - du0[l * ns + s]) * fn;
        const double q = (bcb[l * ns + s] - (u0[((long long)l * n + 0) * ns + s] + c * u1[((long long)0 * n + 0) * ns + s])) * dummy;
        if (j == 0) {
            u[l] = bcb[l * ns + s];
            v[l] = q;
        } else {
            u[l] = u0[((long long)l * n + j) * ns + s] + c * u1[((long long)0 * n + j) * ns + s] + q * sp[((long long)0 * n + j) * ns + s];
            v[l] = v0[((long long)l * n + j) * ns + s] + c * v1[((long long)0 * n + j) * ns + s] + q;
        }
    }
    reinterpret_cast<double2 *>(p_hat)[idx] = make_double2(u[0], u[1]);
    reinterpret_cast<double2 *>(dp_hat)[idx] = make_double2(v[0], v[1]);
}

// p(:,1,:) = bcs_hb, p(:,ny,:) = bcs_ht  (opr_elliptic.f90:285-286)
__global__ void __launch_bounds__(256) k_set_wall_planes(double *__restrict__ p, const double *__restrict__ hb,
                                                          const double *__restrict__ ht, int nx, int ny, int nz) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nx * nz) return;
    const int ix = (int)(i % nx);
    const long long k = i / nx;
    p[ix + (long long)nx * (0 + (long long)ny * k)] = hb[i];
    p[ix + (long long)nx * ((ny - 1) + (long long)ny * k)] = ht[i];
}

}  // namespace tlab

// ================================================================================================
// host side: plan, rocFFT, orchestration
// ================================================================================================
namespace {

bool g_rocfft_up = false;
bool g_poisson_exact = env_int("TLAB_POISSON_EXACT", 0) != 0;

void wall_planes(tlab_poisson_plan_t P, double *p, const double *hb, const double *ht, int nz, hipStream_t st) {
    hipLaunchKernelGGL(k_set_wall_planes, dim3((unsigned)(((long long)P->nx * nz + 255) / 256)), dim3(256), 0, st, p, hb, ht, P->nx, P->ny, nz);
}

Int1Args base_args(const tlab_poisson_plan &P, int which, const double *lam, long long nm, double *scratch) {
    Int1Args a{};
    a.T = P.dev(which);
    a.lam = lam;
    a.lam_sign = which == 0 ? 1.0 : -1.0;
    a.nm = nm;
    a.fscale = 1.0;
    a.nxh = P.nxh;
    a.ny = P.ny;
    a.scratch = scratch;
    if (P.generic) {
        const tlab_poisson_plan::GenSet &G = P.gen_set(which, lam, nm);
        a.g_fac = G.fac.p; a.g_rb = G.rb.p; a.g_rt = G.rt.p; a.g_R = G.R.p; a.g_ndi = G.ndi; a.g_nri = G.nri;
    }
    return a;
}

// v1, u1, du1 of the singular modes depend on the mode only (opr_odes.f90:64-73): once per plan
void build_singular_homogeneous(tlab_poisson_plan &P, hipStream_t st) {
    const int ns = (int)P.sing_modes.size();
    if (ns == 0) return;
    Int1Args s2 = base_args(P, 1, P.s_lam.p, ns, P.s_scr.p);   // v1' = delta_1, v1(n) = 0
    s2.unit_row = 0; s2.zero_bsave = 0; s2.dst = P.s_v1.p;
    launch_int1<2, 2, FS_UNIT>(s2, st);
    Int1Args s4 = base_args(P, 0, P.s_lam.p, ns, P.s_scr.p);   // u1' = v1, u1(1) = 0
    s4.fsrc = P.s_v1.p; s4.nlf = 2; s4.zero_bsave = 0; s4.dst = P.s_u1.p; s4.du = P.s_du1.p;
    launch_int1<1, 2, FS_LINEAR>(s4, st);
}

// the streams of the singular / low modes.  NOT high-priority ones: the presence of a high-priority stream in the process slowed every kernel of
// the normal streams on this stack (measured A/B on one box: substep 17.7 -> 21.9 ms, k_fftz 0.53 -> 0.66 ms; 8 loopback slabs 30.6 -> 62.9 ms)
void create_side_stream(hipStream_t *s) { hipc(hipStreamCreateWithFlags(s, hipStreamNonBlocking), "stream"); }

void build_fft(tlab_poisson_plan &P) {
    if (!g_rocfft_up) {
        fftc(rocfft_setup(), "setup");
        g_rocfft_up = true;
    }
    const size_t nx = P.nx, ny = P.ny, nxh = P.fx_nxh;
    size_t nz = P.fx_nz;
    {   // x: real -> complex, batch ny*nz (dfftw_plan_many_dft_r2c, opr_fourier.f90:163-166)
        rocfft_plan_description d = nullptr;
        fftc(rocfft_plan_description_create(&d), "desc");
        size_t is[1] = {1}, os[1] = {1};
        fftc(rocfft_plan_description_set_data_layout(d, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved, nullptr, nullptr,
                                                     1, is, nx, 1, os, nxh), "layout r2c");
        size_t len[1] = {nx};
        fftc(rocfft_plan_create(&P.fx_r2c.plan, rocfft_placement_notinplace, rocfft_transform_type_real_forward, rocfft_precision_double,
                                1, len, ny * nz, d), "plan r2c");
        rocfft_plan_description_destroy(d);
        P.fx_r2c.finish();
        // TLAB_FFTX=0 keeps rocFFT for the forward x-transform
        if (env_int("TLAB_FFTX", 1) != 0 && FftxPlan::supported((int)nx) && nxh == nx / 2 + 1) P.fx_own = std::make_unique<FftxPlan>((int)nx, (long long)(ny * nz));
    }
    {   // x: complex -> real (dfftw_plan_many_dft_c2r, :167-170)
        rocfft_plan_description d = nullptr;
        fftc(rocfft_plan_description_create(&d), "desc");
        size_t is[1] = {1}, os[1] = {1};
        fftc(rocfft_plan_description_set_data_layout(d, rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, nullptr, nullptr,
                                                     1, is, nxh, 1, os, nx), "layout c2r");
        size_t len[1] = {nx};
        fftc(rocfft_plan_create(&P.fx_c2r.plan, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, rocfft_precision_double,
                                1, len, ny * nz, d), "plan c2r");
        rocfft_plan_description_destroy(d);
        P.fx_c2r.finish();
    }
    if (P.nzt > 1) {  // z: complex <-> complex, stride = batch = nlines with distance 1 (dfftw_plan_many_dft, :111-119);
        // nlines = (imax/2+1)*jmax, or tmpi_plan_fftz%nlines = that / npro_k after the K-transposition (opr_fourier.f90:85-98)
        nz = P.nz;
        const size_t nlines = (size_t)P.nxh * ny * nz / (size_t)P.nzt;
        // TLAB_FFTZ=0 keeps rocFFT for the z-transform
        if (env_int("TLAB_FFTZ", 1) != 0 && FftzPlan::supported(P.nzt)) P.fz_own = std::make_unique<FftzPlan>(P.nzt, (long long)nlines);
        for (int dir = 0; dir < 2; ++dir) {
            rocfft_plan_description d = nullptr;
            fftc(rocfft_plan_description_create(&d), "desc");
            size_t st[1] = {nlines};
            fftc(rocfft_plan_description_set_data_layout(d, rocfft_array_type_complex_interleaved, rocfft_array_type_complex_interleaved,
                                                         nullptr, nullptr, 1, st, 1, 1, st, 1), "layout c2c");
            size_t len[1] = {(size_t)P.nzt};
            FftPlan &F = dir == 0 ? P.fz_f : P.fz_b;
            fftc(rocfft_plan_create(&F.plan, rocfft_placement_notinplace,
                                    dir == 0 ? rocfft_transform_type_complex_forward : rocfft_transform_type_complex_inverse,
                                    rocfft_precision_double, 1, len, nlines, d), "plan c2c");
            rocfft_plan_description_destroy(d);
            F.finish();
        }
    }
}

// fused 2-D transforms over (x, z), one per y plane: same arithmetic as r2c(x) followed by c2c(z)
void build_fft_2d(tlab_poisson_plan &P) {
    const size_t nx = P.nx, ny = P.ny, nz = P.nz, nxh = P.nxh;
    for (int dir = 0; dir < 2; ++dir) {
        rocfft_plan_description d = nullptr;
        fftc(rocfft_plan_description_create(&d), "desc");
        size_t rs[2] = {1, nx * ny}, cs[2] = {1, nxh * ny};
        if (dir == 0)
            fftc(rocfft_plan_description_set_data_layout(d, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved, nullptr, nullptr,
                                                         2, rs, nx, 2, cs, nxh), "layout 2d fwd");
        else
            fftc(rocfft_plan_description_set_data_layout(d, rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, nullptr, nullptr,
                                                         2, cs, nxh, 2, rs, nx), "layout 2d bwd");
        size_t len[2] = {nx, nz};
        FftPlan &F = dir == 0 ? P.f2_fwd : P.f2_bwd;
        fftc(rocfft_plan_create(&F.plan, rocfft_placement_notinplace,
                                dir == 0 ? rocfft_transform_type_real_forward : rocfft_transform_type_real_inverse,
                                rocfft_precision_double, 2, len, ny, d), "plan 2d");
        rocfft_plan_description_destroy(d);
        F.finish();
    }
}

// homogeneous solutions and constraint LU of every mode (opr_odes.f90:308-348), once per plan
void build_homogeneous(tlab_poisson_plan &P, hipStream_t st) {
    const long long nm = P.nm;
    const int n = P.ny;
    // v^(1), e^(-): v' + l v = (delta_n, 0), v(1) = (0, 1)   [third line of the reference is identically zero]
    Int1Args a = base_args(P, 0, P.lam.p, nm, P.scratch.p);
    a.unit_row = n - 1;
    a.zero_bsave = 0;
    a.bv[0] = 0.0; a.bv[1] = 1.0; a.bv[2] = 0.0;
    a.dst = P.hom.p;                                   // lines 0,1 -> v1, em
    launch_int1<1, 2, FS_UNIT>(a, st);
    // u^(1), s^(+), e^(+): u' - l u = (v1, em, 0), u(n) = (0, 0, 1)
    Int1Args b = base_args(P, 1, P.lam.p, nm, P.scratch.p);
    b.fsrc = P.hom.p;
    b.nlf = 2;
    b.zero_bsave = 0;
    b.bv[0] = 0.0; b.bv[1] = 0.0; b.bv[2] = 1.0;
    b.dst = P.hom.p + (size_t)2 * n * nm;              // lines 2,3,4 -> u1, sp, ep
    b.du = P.der.p;
    launch_int1<2, 3, FS_LINEAR>(b, st);
    const int grid = (int)((nm + 255) / 256);
    hipLaunchKernelGGL(k_nn_constants, dim3(grid), dim3(256), 0, st, P.hom.p, P.der.p, P.lam.p, P.cst.p, n, nm);
    hipc(hipGetLastError(), "k_nn_constants");
}

// The difference between k_ode_nn and the reference's serial sweeps lives in the few modes with lambda h^2 << 1: the
// substitution recurrences of B +- lambda A are neutral there and the rounding of the chunk transfers adds up.  Those modes -- sqrt(lambda) *
// mean(h) <= 0.06, at most 128 per box, i.e. the energy-carrying ones of a smooth field -- are taken out of k_ode_nn (skip flag) and solved by a
// marching sub-plan (the reference's operations one by one) on the side stream, beside the regular modes: 4.5e-12 -> 7.6e-13 in p on the
// projection forcing of tests/test_gpu_poisson.py, i.e. the FFT-noise floor.  TLAB_POISSON_LOW_MODES=0 disables it.
void build_low_modes(tlab_poisson_plan &P, const std::vector<double> &nodes, const std::vector<double> &lam, std::vector<unsigned char> &skip,
                     hipStream_t st) {
    // Cost: the sub-plan's chain of latency-bound launches (2.6 ms beside k_ode_nn's 2.4 ms at 512^3) sticks out by ~0.3 ms on a single device
    // (1.4 % of the substep).  Decomposed plans (z-slabs, kx-pencils) take it too: parity with the single domain at <= 1e-12 comes first, and
    // with the staged pencil exchange the low modes sit in the first kx half of rank 0, whose solve runs under the transfer of the second half.
    // Every plan applies the same threshold to its own modes, so the union over the ranks is the single-domain set (below the cap of 128).
    if (env_int("TLAB_POISSON_LOW_MODES", 1) == 0) return;
    const int ny = P.ny;
    if ((int)nodes.size() != ny || ny < 2) return;               // host-built plans without nodes: feature off
    const double hbar = (nodes[ny - 1] - nodes[0]) / (ny - 1.0);
    std::vector<int> cand;
    for (long long t = 0; t < P.nm; ++t)
        if (!skip[t] && lam[t] * hbar <= 0.06) cand.push_back((int)t);
    if (cand.empty()) return;
    std::sort(cand.begin(), cand.end(), [&](int a, int b) { return lam[a] < lam[b] || (lam[a] == lam[b] && a < b); });
    if (cand.size() > 128) cand.resize(128);
    const int ns = (int)cand.size();
    auto L = std::make_unique<tlab_poisson_plan>();
    L->nx = 2; L->ny = ny; L->nz = 1; L->nxh = ns; L->nzt = 1; L->nproc = 1; L->fx_nxh = ns; L->fx_nz = 1;
    L->nm = ns; L->norm = P.norm;
    L->tmin = P.tmin; L->tmax = P.tmax;
    L->d_L0[0].upload(L->tmin.L0); L->d_L1[0].upload(L->tmin.L1); L->d_R[0].upload(L->tmin.R);
    L->d_L0[1].upload(L->tmax.L0); L->d_L1[1].upload(L->tmax.L1); L->d_R[1].upload(L->tmax.R);
    std::vector<double> sub(ns);
    for (int s = 0; s < ns; ++s) { sub[s] = lam[cand[s]]; skip[cand[s]] = 1; }
    L->lam.upload(sub);
    hipc(hipMalloc((void **)&L->d_skip, (size_t)ns), "hipMalloc");
    hipc(hipMemset(L->d_skip, 0, (size_t)ns), "hipMemset");
    hipc(hipMalloc((void **)&L->d_sing, sizeof(int)), "hipMalloc");
    const size_t n = ny;
    L->hom.alloc(5 * n * ns); L->der.alloc(3 * (size_t)ns); L->cst.alloc(9 * (size_t)ns);
    L->scratch.alloc(6 * n * ns);
    L->v0.alloc(2 * n * ns); L->u0.alloc(2 * n * ns); L->du0.alloc(2 * (size_t)ns); L->bcs.alloc(4 * (size_t)ns);
    create_side_stream(&L->side);
    hipc(hipEventCreateWithFlags(&L->ev_fork, hipEventDisableTiming), "event");
    hipc(hipEventCreateWithFlags(&L->ev_join, hipEventDisableTiming), "event");
    build_homogeneous(*L, st);
    {   // LU factors of both systems, stored once: the per-call solves of these few threads then only substitute
        L->fac[0].alloc(5 * n * ns); L->fac[1].alloc(5 * n * ns);
        Int1Args a = base_args(*L, 0, L->lam.p, ns, L->scratch.p);
        a.unit_row = 1; a.dst = L->v0.p; a.fac_out = L->fac[0].p;
        launch_int1<1, 2, FS_UNIT>(a, st);
        Int1Args b = base_args(*L, 1, L->lam.p, ns, L->scratch.p);
        b.unit_row = 1; b.dst = L->u0.p; b.fac_out = L->fac[1].p;
        launch_int1<2, 2, FS_UNIT>(b, st);
    }
    hipc(hipMalloc((void **)&P.d_low_modes, ns * sizeof(int)), "hipMalloc");
    hipc(hipMemcpy(P.d_low_modes, cand.data(), ns * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy");
    hipc(hipMemcpy(P.d_skip, skip.data(), (size_t)P.nm, hipMemcpyHostToDevice), "hipMemcpy");      // k_ode_nn leaves these columns alone
    P.n_low = ns;
    P.low_f.alloc(2 * n * ns); P.low_p.alloc(2 * n * ns); P.low_dp.alloc(2 * n * ns);
    P.low = std::move(L);
    create_side_stream(&P.side_low);
    hipc(hipEventCreateWithFlags(&P.ev_join_low, hipEventDisableTiming), "event");
}

}  // namespace

// forward transforms field -> tmp2 -> tmp1 (opr_elliptic.f90:288-293); the scaling by norm (:295) is folded into the loads of the ODE stage
void tlab_poisson_plan::forward_xz(double *field, double *tmp1, double *tmp2, hipStream_t st) {
    if (use_2d) {
        f2_fwd.exec(field, tmp1, st);
    } else if (nz > 1) {
        x_forward(field, tmp2, st);
        z_exec(1, tmp2, tmp1, st);
    } else {
        x_forward(field, tmp1, st);
    }
}
// backward transforms hat -> (cwork ->) out (:341-356); vf: hat is dp^/dy and the inverse x-transform honours the request (x_backward_dpdy)
void tlab_poisson_plan::backward_xz(double *hat, double *out, hipStream_t st, const VFinal *vf) {
    if (use_2d) {
        f2_bwd.exec(hat, out, st);
        return;
    }
    double *src = hat;
    if (nz > 1) {
        z_exec(-1, hat, cwork.p, st);
        src = cwork.p;
    }
    if (vf) x_backward_dpdy(src, out, st, *vf);
    else x_backward_p(src, out, st);
}

bool tlab_internal_poisson_has_own_x(tlab_poisson_plan_t P) { return P && P->fx_own; }
bool tlab_internal_poisson_box(tlab_poisson_plan_t P, int *n) {
    if (!P || P->nproc != 1 || P->nzt != P->nz || P->koff != 0 || P->ioff != 0 || P->nxh != P->nx / 2 + 1 || P->fx_nxh != P->nxh || P->fx_nz != P->nz) return false;
    n[0] = P->nx; n[1] = P->ny; n[2] = P->nz;
    return true;
}

extern "C" {

// nz: planes of the local spectral box; [ioff, ioff+nxl) its kx range (nxl = 0: all nx/2+1); fx_nz: planes of the local PHYSICAL box
static int poisson_plan_create_impl(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz, int nx, int ny,
                                    int nz, int nzt, int koff, int nproc, int ioff = 0, int nxl = 0, int fx_nz = 0,
                                    tlab_fdm_plan_t gy_ell = nullptr, bool helmholtz = false, double alpha = 0.0) {
    return catch_fail([&]() -> int {
        if (!out || !gx || !gy || !gz) throw Fail(TLAB_EINVAL, "tlab_poisson_plan_create: null argument");
        if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called (no CPU fallback exists)");
        if (gx->t.n != nx || gy->t.n != ny || gz->t.n != nzt) throw Fail(TLAB_EINVAL, "plan sizes do not match nx, ny, nz");
        if (!gx->t.periodic || (nzt > 1 && !gz->t.periodic) || gy->t.periodic)
            throw Fail(TLAB_EINVAL, "OPR_Poisson_FourierXZ needs periodic x, z and non-periodic y");
        if (nx % 2 != 0) throw Fail(TLAB_EINVAL, "Imax must be a multiple of 2 for the FFT operations (opr_fourier.f90:72-75)");
        {   // host-built plans (tlab_fdm_plan_create_from_arrays) carry the modified wavenumbers only after tlab_fdm_plan_set_aux
            auto no_mwn = [](const tlab::DerTables &d) {
                for (double v : d.mwn) if (v != 0.0) return false;
                return true;
            };
            if (!gy_ell && (no_mwn(gx->t.der1) || (nzt > 1 && no_mwn(gz->t.der1))))
                throw Fail(TLAB_EINVAL, "the x / z plans carry no modified wavenumbers (der1%mwn): call tlab_fdm_plan_set_aux");
            if (gy_ell && (no_mwn(gx->t.der2) || (nzt > 1 && no_mwn(gz->t.der2))))
                throw Fail(TLAB_EINVAL, "the x / z plans carry no second-derivative modified wavenumbers (der2%mwn): call tlab_fdm_plan_set_aux");
            if (gy_ell && (gy_ell->t.n != ny || gy_ell->t.periodic || !gy_ell->t.der2.direct || gy_ell->t.der2.ndl != 3 || gy_ell->t.der2.ndr != 5 ||
                           (int)gy_ell->t.nodes.size() != ny))
                throw Fail(TLAB_EINVAL, "direct elliptic solver: the elliptic y plan must hold a CompactDirect6 second derivative (3/5 diagonals) and its nodes");
        }
        if (nproc < 1 || nz * nproc != nzt || koff < 0 || koff + nz > nzt) throw Fail(TLAB_EINVAL, "bad z-slab decomposition");
        if (((long long)(nx / 2 + 1) * ny) % nproc != 0) throw Fail(TLAB_EINVAL, "(imax/2+1)*jmax must be divisible by the number of z slabs (tlab_mpi_transpose.f90:292)");
        auto P = std::make_unique<tlab_poisson_plan>();
        if (nxl < 0 || ioff < 0 || ioff + nxl > nx / 2 + 1) throw Fail(TLAB_EINVAL, "bad kx range");
        P->nx = nx; P->ny = ny; P->nz = nz; P->nxh = nxl > 0 ? nxl : nx / 2 + 1;
        P->ioff = nxl > 0 ? ioff : 0;
        P->fx_nxh = nx / 2 + 1; P->fx_nz = fx_nz > 0 ? fx_nz : nz;
        P->nzt = nzt; P->koff = koff; P->nproc = nproc;
        P->nm = (long long)P->nxh * nz;
        P->norm = 1.0 / ((double)nx * (double)nzt);                     // opr_elliptic.f90:130
        if (gy_ell) {   // TYPE_DIRECT (opr_elliptic.f90:152-163, 228-245)
            P->direct = true;
            P->exact_mode = g_poisson_exact;
            P->gy_der = gy;
            P->ell_der2 = gy_ell->t.der2;
            P->ell_nodes = gy_ell->t.nodes;
            const long long nm = P->nm;
            std::vector<double> lam((size_t)nm);
            for (int k = 0; k < nz; ++k)
                for (int i = 0; i < P->nxh; ++i) {
                    double l2 = gx->t.der2.mwn[P->ioff + i];                       // lambda = mwn2_x + mwn2_z (:230-234)
                    if (nzt > 1) l2 += gz->t.der2.mwn[koff + k];
                    lam[(size_t)i + (size_t)P->nxh * k] = l2;
                }
            if (P->ioff == 0 && koff == 0) P->sing_direct = 0;                      // i_sing = k_sing = [1, 1] (:160-161)
            P->lam.upload(lam);
            (void)P->dev2(TLAB_BCS_NN);
            if (P->sing_direct >= 0) (void)P->dev2(TLAB_BCS_DN);
            P->scratch.alloc((size_t)5 * ny * nm);
            P->cwork.alloc((size_t)2 * P->nxh * ny * nz);
            build_fft(*P);
            *out = P.release();
            return TLAB_OK;
        }
        if (int1_generic_applies(gy->t.der1)) {      // (3, 3) / (5, 7) diagonals: TRIDFS / HEPTADFS systems, factorized on the host (int1_generic.cpp)
            if (gy->t.periodic) throw Fail(TLAB_EINVAL, "Poisson: the wall-normal direction must not be periodic");
            P->generic = true;
            P->gder = gy->t.der1;
        } else {
            int1_build_tables(gy->t.der1, 1, P->tmin);
            int1_build_tables(gy->t.der1, 2, P->tmax);
            P->d_L0[0].upload(P->tmin.L0); P->d_L1[0].upload(P->tmin.L1); P->d_R[0].upload(P->tmin.R);
            P->d_L0[1].upload(P->tmax.L0); P->d_L1[1].upload(P->tmax.L1); P->d_R[1].upload(P->tmax.R);
            for (int w = 0; w < 2; ++w) {
                const Int1Tables &T = w == 0 ? P->tmin : P->tmax;
                if (T.L0.size() < (size_t)6 * ny || T.L1.size() < (size_t)5 * ny || T.R.size() < (size_t)3 * ny) continue;      // (generic tables: k_int1g)
                std::vector<double> pk((size_t)16 * ny, 0.0);
                for (int j = 0; j < ny; ++j) {
                    for (int k = 0; k < 5; ++k) { pk[(size_t)16 * j + k] = T.L0[(size_t)5 * j + k]; pk[(size_t)16 * j + 5 + k] = T.L1[(size_t)5 * j + k]; }
                    pk[(size_t)16 * j + 10] = T.L0[(size_t)5 * ny + j];
                    pk[(size_t)16 * j + 11] = T.R[(size_t)3 * j + 0];
                    pk[(size_t)16 * j + 12] = T.R[(size_t)3 * j + 1];
                    pk[(size_t)16 * j + 13] = T.R[(size_t)3 * j + 2];
                }
                P->d_pk[w].upload(pk);
            }
        }
        // lambda(k,i) = mwn_x(i)^2 + mwn_z(k)^2 (opr_elliptic.f90:199-203), stored as sqrt (:205-209)
        const long long nm = P->nm;
        std::vector<double> lam((size_t)nm);
        std::vector<unsigned char> skip((size_t)nm, 0);
        for (int k = 0; k < nz; ++k)
            for (int i = 0; i < P->nxh; ++i) {
                double l2 = std::pow(gx->t.der1.mwn[P->ioff + i], 2.0);
                if (nzt > 1) l2 += std::pow(gz->t.der1.mwn[koff + k], 2.0);   // kglobal = k + ims_offset_k (:191)
                if (helmholtz) {                                             // sqrt(lambda(k,i) - alpha) (:518-522)
                    if (!(l2 - alpha > 0.0)) throw Fail(TLAB_EINVAL, "OPR_Helmholtz (factorized): lambda - alpha must be positive for every mode");
                    l2 = l2 - alpha;
                }
                lam[(size_t)i + (size_t)P->nxh * k] = std::sqrt(l2);
            }
        // i_sing, k_sing (:148-149), 0-based, global; with the staggered pressure grid only (1, 1) is singular: the interpolatory modified
        // wavenumbers do not vanish at the Nyquist modes (:144-146)
        const bool stag = gx->t.stagger || (nzt > 1 && gz->t.stagger);
        const int isg[2] = {0, stag ? 0 : nx / 2}, ksg[2] = {0, (nzt > 1 && !stag) ? nzt / 2 : 0};
        for (int a = 0; a < 2 && !helmholtz; ++a)                           // Helmholtz: every mode is a regular one (:512-531)
            for (int b = 0; b < 2; ++b) {
                const int kl = ksg[b] - koff;                               // task-local index (:177-178)
                const int il = isg[a] - P->ioff;
                if (kl < 0 || kl >= nz || il < 0 || il >= P->nxh) continue;
                const int t = il + P->nxh * kl;
                if (!skip[t]) { skip[t] = 1; P->sing_modes.push_back(t); }
            }
        P->lam.upload(lam);
        hipc(hipMalloc((void **)&P->d_skip, (size_t)nm), "hipMalloc");
        hipc(hipMemcpy(P->d_skip, skip.data(), (size_t)nm, hipMemcpyHostToDevice), "hipMemcpy");
        const int ns = (int)P->sing_modes.size();
        hipc(hipMalloc((void **)&P->d_sing, (ns + 1) * sizeof(int)), "hipMalloc");
        if (ns) hipc(hipMemcpy(P->d_sing, P->sing_modes.data(), ns * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy");
        std::vector<double> slam(ns);
        for (int s = 0; s < ns; ++s) slam[s] = lam[P->sing_modes[s]];
        P->s_lam.upload(slam);
        const size_t n = ny;
        P->hom.alloc(5 * n * nm); P->der.alloc(3 * nm); P->cst.alloc(9 * nm);
        P->scratch.alloc(6 * n * nm);      // NL + 3 components, NL <= 3
        P->v0.alloc(2 * n * nm); P->u0.alloc(2 * n * nm); P->du0.alloc(2 * nm); P->bcs.alloc(4 * nm);
        P->helmholtz = helmholtz;
        if (!helmholtz) P->cwork.alloc((size_t)2 * P->nxh * ny * nz);
        if (nproc == 1 && nxl == 0) { P->g3[0] = gx; P->g3[1] = gy; P->g3[2] = gz; }
        P->s_f.alloc(2 * n * ns); P->s_bct.alloc(2 * ns); P->s_v0.alloc(2 * n * ns); P->s_v1.alloc(2 * n * ns);
        P->s_u0.alloc(2 * n * ns); P->s_u1.alloc(2 * n * ns); P->s_du0.alloc(2 * ns); P->s_du1.alloc(2 * ns); P->s_scr.alloc(5 * n * ns);
        if (!helmholtz) build_fft(*P);
        {   // fused 2-D (x,z) transforms are ~2x faster than r2c(x) + strided c2c(z) at 512^3, but rocFFT does not build them
            // for every layout: fall back to the two 1-D plans when plan creation fails (TLAB_FFT2D=0 forces the 1-D path)
            // ... and slower than r2c(x) + the own strided z-transform (fftz.hip: 0.49 + 0.53 ms against 1.14 ms at 512^3), so they are only
            // built where that kernel does not apply (TLAB_FFTZ=0 or a length that is not 8^a * {1,2,4})
            if (!helmholtz && nzt > 1 && nproc == 1 && nxl == 0 && !P->fz_own && env_int("TLAB_FFT2D", 1) != 0) {
                try {
                    build_fft_2d(*P);
                    P->use_2d = true;
                } catch (const std::exception &) {
                    P->use_2d = false;
                }
            }
        }
        create_side_stream(&P->side);
        hipc(hipEventCreateWithFlags(&P->ev_fork, hipEventDisableTiming), "event");
        hipc(hipEventCreateWithFlags(&P->ev_join, hipEventDisableTiming), "event");
        hipStream_t st = tlab_current_stream();
        build_homogeneous(*P, st);
        build_singular_homogeneous(*P, st);
        {   // chunked ODE kernel (k_ode_nn) when the line splits into 8-row chunks and 32-bit indices suffice; tlab_poisson_set_exact(1)
            // (or TLAB_ODE_CHUNKED=0) keeps the marching kernels, which repeat the reference's operations one by one
            const bool want = !g_poisson_exact && env_int("TLAB_ODE_CHUNKED", 1) != 0;
            const int C = ny / OM;
            const long long big = std::max<long long>((long long)5 * ny * (nm + 64), std::max<long long>(9 * nm, (long long)P->nxh * ny * nz));
            if (!P->generic && want && ny % OM == 0 && C >= 2 && ode_modes_per_wg(C) > 0 && big < (1LL << 31) &&
                ode_lds_bytes(C, ode_modes_per_wg(C)) <= (size_t)160 * 1024) {
                P->ode_nm_per_wg = ode_modes_per_wg(C);
                {   // mirror pairs (see k_ode_nn): TLAB_ODE_PAIR=0 keeps one mode per thread
                    const int om = OM;
                    const int nzm = (int)(nm / P->nxh);
                    bool sym = env_int("TLAB_ODE_PAIR", 1) != 0 && nzm >= 4 && (om == 4 || om == 8) && ny % om == 0;
                    for (int kz = 1; sym && kz < nzm; ++kz)
                        for (long long i = 0; i < P->nxh; ++i) sym = sym && lam[i + P->nxh * kz] == lam[i + P->nxh * (nzm - kz)];
                    const int Cp = ny / om, NMp = sym ? ode_modes_per_wg(Cp) : 0;
                    if (sym && NMp > 0 && ode_lds_bytes(Cp, NMp, om, 4) <= (size_t)160 * 1024) {
                        P->ode_pair = true; P->ode_om = om; P->ode_nm_per_wg = NMp;
                    }
                }
                build_checkpoints(*P, st);
                P->use_chunked = true;
                if (ode_sing_nm(C) * C <= 512 && (int)P->sing_modes.size() <= ode_sing_nm(C) && ode_lds_bytes(C, ode_sing_nm(C)) <= (size_t)160 * 1024)
                    build_singular_checkpoints(*P, st);
                else P->use_chunked = false;
            }
        }
        if (P->use_chunked) build_low_modes(*P, gy->t.nodes, lam, skip, st);
        hipc(hipStreamSynchronize(st), "sync");
        if (P->use_chunked) {   // the scratch of the marching kernels is not needed any more
            P->scratch.alloc(0); P->v0.alloc(0); P->u0.alloc(0); P->hom.alloc(0);      // hom lives on in its blocked copy
        }
        *out = P.release();
        return TLAB_OK;
    }, TLAB_EHIP);
}

int tlab_poisson_plan_create(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz, int nx, int ny,
                             int nz) {
    return poisson_plan_create_impl(out, gx, gy, gz, nx, ny, nz, nz, 0, 1);
}

int tlab_poisson_set_exact(int on) {
    g_poisson_exact = on != 0;
    return TLAB_OK;
}

int tlab_poisson_plan_create_direct(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz, int nx, int ny,
                                    int nz, tlab_fdm_plan_t gy_elliptic) {
    if (!gy_elliptic) {
        tlab_set_error("tlab_poisson_plan_create_direct: null elliptic plan");
        return TLAB_EINVAL;
    }
    return poisson_plan_create_impl(out, gx, gy, gz, nx, ny, nz, nz, 0, 1, 0, 0, 0, gy_elliptic);
}

int tlab_poisson_plan_create_slab(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz, int nx, int ny,
                                  int kmax, int nz_total, int koffset, int nproc_k) {
    return poisson_plan_create_impl(out, gx, gy, gz, nx, ny, kmax, nz_total, koffset, nproc_k);
}

int tlab_poisson_plan_create_pencil(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz, int nx, int ny,
                                    int kmax, int nz_total, int ioffset, int nxl) {
    if (nxl <= 0 || kmax <= 0 || nz_total % kmax != 0) {
        tlab_set_error("tlab_poisson_plan_create_pencil: bad decomposition");
        return TLAB_EINVAL;
    }
    return poisson_plan_create_impl(out, gx, gy, gz, nx, ny, nz_total, nz_total, 0, 1, ioffset, nxl, kmax);
}

// decomposed variants of a direct plan (EllipticOrder = CompactDirect6): mode = 0 z-slab (K-transposes), 1 kx-pencil; a, b as in the
// factorized creators: (koffset, nproc_k) or (ioffset, nxl)
int tlab_poisson_plan_create_direct_decomposed(tlab_poisson_plan_t *out, tlab_fdm_plan_t gx, tlab_fdm_plan_t gy, tlab_fdm_plan_t gz, int nx,
                                               int ny, int kmax, int nz_total, int mode, int a, int b, tlab_fdm_plan_t gy_elliptic) {
    if (!gy_elliptic || kmax <= 0 || nz_total % kmax != 0 || (mode != 0 && mode != 1) || (mode == 1 && b <= 0)) {
        tlab_set_error("tlab_poisson_plan_create_direct_decomposed: bad arguments");
        return TLAB_EINVAL;
    }
    if (mode == 0) return poisson_plan_create_impl(out, gx, gy, gz, nx, ny, kmax, nz_total, a, b, 0, 0, 0, gy_elliptic);
    return poisson_plan_create_impl(out, gx, gy, gz, nx, ny, nz_total, nz_total, 0, 1, a, b, kmax, gy_elliptic);
}

int tlab_poisson_plan_destroy(tlab_poisson_plan_t p) {
    (void)tlab_internal_deferred_flush();      // (a recorded substep may still solve with it)
    delete p;
    return TLAB_OK;
}

// The lowest-lambda modes of a chunked plan: gathered into a compact field, solved by `stage` on the marching sub-plan, scattered back -- all on st,
// beside the regular modes of k_ode_nn, which leaves their columns alone
static void low_modes_stage(tlab_poisson_plan_t P, void (*stage)(tlab_poisson_plan_t, double *, double *, double *, hipStream_t), double *f_hat,
                            double *p_hat, double *dp_hat, hipStream_t st) {
    const int nl = P->n_low, n = P->ny;
    const dim3 g((nl + 63) / 64, n), blk(64);
    hipLaunchKernelGGL(k_modes_gather, g, blk, 0, st, reinterpret_cast<const double2 *>(f_hat), P->d_low_modes, nl, n, P->nxh, P->ny,
                       reinterpret_cast<double2 *>(P->low_f.p));
    stage(P->low.get(), P->low_f.p, P->low_p.p, P->low_dp.p, st);
    hipLaunchKernelGGL(k_modes_scatter, g, blk, 0, st, reinterpret_cast<const double2 *>(P->low_p.p), reinterpret_cast<const double2 *>(P->low_dp.p),
                       P->d_low_modes, nl, n, P->nxh, P->ny, reinterpret_cast<double2 *>(p_hat), reinterpret_cast<double2 *>(dp_hat));
}

// ibc = BCS_DD on a factorized plan (opr_elliptic.f90:322-329).  Chunked plans: the regular modes in k_ode_nn<DD> (the BCS_NN kernel with the
// top value given and the two constants of OPR_ODE2_Factorize_DD), the <= 4 singular modes (_DD_Sing) and the lowest-lambda modes (marching
// sub-plan) beside it on the side stream, as for BCS_NN; other plans: marching kernels for every mode.  TLAB_ODE_DD_CHUNKED=0 keeps the marching route.
static void poisson_dd_stage(tlab_poisson_plan_t P, double *f_hat, double *p_hat, double *dp_hat, hipStream_t st) {
    const long long nm = P->nm;
    const int n = P->ny, nxh = P->nxh, ny = P->ny;
    const int ns = (int)P->sing_modes.size();
    const bool chunked = P->use_chunked && env_int("TLAB_ODE_DD_CHUNKED", 1) != 0;      // read per call: the tests switch between the two routes of one plan
    hipStream_t main_st = st;
    if (chunked) {
        if (P->cst_dd.n == 0) {
            P->cst_dd.alloc((size_t)5 * nm);
            hipLaunchKernelGGL(k_dd_constants, dim3((unsigned)((nm + 255) / 256)), dim3(256), 0, st, P->homb.p, P->ode_nm_per_wg, P->der.p, P->cst_dd.p, n, nm);
            hipc(hipGetLastError(), "k_dd_constants");
        }
        hipc(hipEventRecord(P->ev_fork, st), "event record");
        hipc(hipStreamWaitEvent(P->side, P->ev_fork, 0), "stream wait");
        st = P->side;            // the singular and the low modes run beside k_ode_nn<DD>, which leaves their columns alone
    } else if (P->scratch.n == 0) {     // a chunked plan released the work arrays of the marching kernels: they come back
        P->scratch.alloc((size_t)6 * n * nm); P->v0.alloc((size_t)2 * n * nm); P->u0.alloc((size_t)2 * n * nm);
    }
    // ---- singular modes first (they read f^ before the regular combine may overwrite it when p_hat aliases f_hat) ----
    if (ns > 0) {
        if (!P->dd_ready) {      // v^(1): v' = delta_n, v(1) = 0 ; u^(1): u' = v1, u(n) = 0 ; s^(+): u' = 1, u(n) = 0   (opr_odes.f90:216-236)
            P->dd_v1.alloc((size_t)2 * n * ns); P->dd_u1.alloc((size_t)2 * n * ns); P->dd_du1.alloc((size_t)2 * ns);
            P->dd_sp.alloc((size_t)2 * n * ns); P->dd_ones.alloc((size_t)n * ns); P->dd_bcb.alloc((size_t)2 * ns);
            hipLaunchKernelGGL(k_fill_ones, dim3((unsigned)(((long long)n * ns + 255) / 256)), dim3(256), 0, st, P->dd_ones.p, (long long)n * ns);
            Int1Args h1 = base_args(*P, 0, P->s_lam.p, ns, P->s_scr.p);
            h1.unit_row = n - 1; h1.zero_bsave = 0; h1.dst = P->dd_v1.p;
            launch_int1<1, 2, FS_UNIT>(h1, st);
            Int1Args h2 = base_args(*P, 1, P->s_lam.p, ns, P->s_scr.p);
            h2.fsrc = P->dd_v1.p; h2.nlf = 1; h2.zero_bsave = 0; h2.dst = P->dd_u1.p; h2.du = P->dd_du1.p;
            launch_int1<2, 2, FS_LINEAR>(h2, st);
            Int1Args h3 = base_args(*P, 1, P->s_lam.p, ns, P->s_scr.p);
            h3.fsrc = P->dd_ones.p; h3.nlf = 1; h3.zero_bsave = 0; h3.dst = P->dd_sp.p;
            launch_int1<2, 2, FS_LINEAR>(h3, st);
            P->dd_ready = true;
        }
        dim3 g(ns, (n + 63) / 64), blk(64);
        hipLaunchKernelGGL(k_sing_gather_dd, g, blk, 0, st, f_hat, P->d_sing, ns, n, nxh, ny, P->norm, P->s_f.p, P->dd_bcb.p, P->s_bct.p);
        Int1Args s1 = base_args(*P, 0, P->s_lam.p, ns, P->s_scr.p);        // v' = f (f(n) = 0), v(1) = 0
        s1.fsrc = P->s_f.p; s1.nlf = 2; s1.zero_bsave = 1; s1.dst = P->s_v0.p;
        launch_int1<1, 2, FS_LINEAR>(s1, st);
        Int1Args s2 = base_args(*P, 1, P->s_lam.p, ns, P->s_scr.p);        // u' = v, u(n) = bcs_t
        s2.fsrc = P->s_v0.p; s2.nlf = 2; s2.zero_bsave = 0; s2.bv_ptr = P->s_bct.p; s2.dst = P->s_u0.p; s2.du = P->s_du0.p;
        launch_int1<2, 2, FS_LINEAR>(s2, st);
    }
    if (!chunked) {      // ---- regular modes, marching ----
        Int1Args a = base_args(*P, 0, P->lam.p, nm, P->scratch.p);             // v' + l v = f, v(1) = 0
        a.fsrc = f_hat; a.fscale = P->norm; a.zero_bsave = 1; a.bcs_save = P->bcs.p; a.dst = P->v0.p;
        launch_int1<1, 2, FS_FIELD>(a, st);
        Int1Args b = base_args(*P, 1, P->lam.p, nm, P->scratch.p);             // u' - l u = v, u(n) = bcs_t
        b.fsrc = P->v0.p; b.nlf = 2; b.zero_bsave = 0; b.bv_ptr = P->bcs.p + (size_t)2 * nm; b.dst = P->u0.p; b.du = P->du0.p;
        launch_int1<2, 2, FS_LINEAR>(b, st);
        DDCombineArgs c{};
        c.u0 = P->u0.p; c.v0 = P->v0.p; c.du0 = P->du0.p; c.bcs = P->bcs.p; c.der = P->der.p; c.lam = P->lam.p;
        c.hom = P->use_chunked ? P->homb.p : P->hom.p;
        c.hom_nm_block = P->use_chunked ? P->ode_nm_per_wg : 0;
        c.sing = P->d_sing; c.ns = ns;
        c.p_hat = p_hat; c.dp_hat = dp_hat; c.n = n; c.nxh = nxh; c.ny = ny; c.nm = nm;
        hipLaunchKernelGGL(k_dd_combine, dim3((unsigned)((nm + 255) / 256), nm <= 4096 ? (unsigned)((n + 15) / 16) : 1u), dim3(256), 0, st, c);
    }
    if (ns > 0) {
        dim3 g(ns, (n + 63) / 64), blk(64);
        hipLaunchKernelGGL(k_sing_combine_dd, g, blk, 0, st, P->s_u0.p, P->s_v0.p, P->dd_u1.p, P->dd_v1.p, P->dd_sp.p, P->s_du0.p, P->dd_du1.p,
                           P->dd_bcb.p, P->d_sing, ns, n, nxh, ny, p_hat, dp_hat);
    }
    if (chunked) {
        if (P->low) low_modes_stage(P, poisson_dd_stage, f_hat, p_hat, dp_hat, st);      // (poisson_ode_stage does the same for BCS_NN)
        launch_ode(*P, f_hat, p_hat, dp_hat, main_st, true);
        hipc(hipEventRecord(P->ev_join, st), "event record");
        hipc(hipStreamWaitEvent(main_st, P->ev_join, 0), "stream wait");
    }
    hipc(hipGetLastError(), "BCS_DD kernels");
}

// ODE stage on the local modes: f_hat (complex (nxh, ny, kmax), unnormalised FFT output) -> p_hat, dp_hat.
// p_hat may alias f_hat (the reference also overwrites); dp_hat must be a different array.
static void poisson_ode_stage(tlab_poisson_plan_t P, double *f_hat, double *p_hat, double *dp_hat, hipStream_t st) {
    if (P->direct) throw Fail(TLAB_EINVAL, "direct elliptic plan: use tlab_poisson_direct_ode (there is no dp^/dy; dp/dy is OPR_Partial_Y of p)");
    const long long nm = P->nm;
    const int n = P->ny, nxh = P->nxh, ny = P->ny;
    hipc(hipEventRecord(P->ev_fork, st), "event record");
    hipc(hipStreamWaitEvent(P->side, P->ev_fork, 0), "stream wait");
    // ---- regular modes: OPR_ODE2_Factorize_NN (opr_odes.f90:302-318) ----
    if (!P->use_chunked) {
        Int1Args a = base_args(*P, 0, P->lam.p, nm, P->scratch.p);   // v' + l v = f, v(1) = 0
        a.fsrc = f_hat; a.fscale = P->norm; a.zero_bsave = 1; a.bcs_save = P->bcs.p; a.dst = P->v0.p;
        if (P->fac[0].n) a.fac = P->fac[0].p;
        launch_int1<1, 2, FS_FIELD>(a, st);
        Int1Args b = base_args(*P, 1, P->lam.p, nm, P->scratch.p);   // u' - l u = v, u(n) = 0
        b.fsrc = P->v0.p; b.nlf = 2; b.zero_bsave = 0; b.dst = P->u0.p; b.du = P->du0.p;
        if (P->fac[1].n) b.fac = P->fac[1].p;
        launch_int1<2, 2, FS_LINEAR>(b, st);
    }
    // ---- singular modes: OPR_ODE2_Factorize_NN_Sing -> _DN_Sing (opr_odes.f90:165-183, 37-96) ----
    const int ns = (int)P->sing_modes.size();
    hipStream_t ss = P->side;   // independent of the regular modes until the scatter below
    if (ns > 0 && P->use_chunked) launch_ode_sing(*P, f_hat, p_hat, dp_hat, ss);      // one workgroup beside the regular modes; writes only the singular entries
    if (P->use_chunked && P->low) {                         // the lowest-lambda modes: marching sub-plan, also beside the regular ones
        hipc(hipStreamWaitEvent(P->side_low, P->ev_fork, 0), "stream wait");
        low_modes_stage(P, poisson_ode_stage, f_hat, p_hat, dp_hat, P->side_low);
        hipc(hipEventRecord(P->ev_join_low, P->side_low), "event record");
    }
    if (ns > 0 && !P->use_chunked) {
        dim3 g(ns, (n + 63) / 64), blk(64);
        hipLaunchKernelGGL(k_sing_gather, g, blk, 0, ss, f_hat, P->d_sing, ns, n, nxh, ny, P->norm, P->s_f.p, P->s_bct.p);
        Int1Args s1 = base_args(*P, 1, P->s_lam.p, ns, P->s_scr.p);   // v' = f (f(1)=0), v(n) = bcs_t
        s1.fsrc = P->s_f.p; s1.nlf = 2; s1.zero_bsave = 0; s1.bv_ptr = P->s_bct.p; s1.dst = P->s_v0.p;
        launch_int1<2, 2, FS_LINEAR>(s1, ss);
        Int1Args s3 = base_args(*P, 0, P->s_lam.p, ns, P->s_scr.p);   // u' = v, u(1) = bcs_b = 0
        s3.fsrc = P->s_v0.p; s3.nlf = 2; s3.zero_bsave = 0; s3.dst = P->s_u0.p; s3.du = P->s_du0.p;
        launch_int1<1, 2, FS_LINEAR>(s3, ss);
    }
    // ---- superposition ----
    if (!P->use_chunked) {
        CombineArgs c{};
        c.u0 = P->u0.p; c.v0 = P->v0.p; c.du0 = P->du0.p; c.bcs = P->bcs.p; c.hom = P->hom.p; c.cst = P->cst.p; c.lam = P->lam.p;
        c.skip = P->d_skip; c.p_hat = p_hat; c.dp_hat = dp_hat; c.n = n; c.nxh = nxh; c.ny = ny; c.nm = nm;
        ProfScope ps("k_nn_combine", st, (double)nm * n * (9 + 4) * 8.0);
        hipLaunchKernelGGL(k_nn_combine, dim3((unsigned)((nm + 255) / 256), nm <= 4096 ? (unsigned)((n + 15) / 16) : 1u), dim3(256), 0, st, c);
    } else {
        launch_ode(*P, f_hat, p_hat, dp_hat, st);      // both solves, the constants and the final pass in one kernel
    }
    // the singular modes write other entries than k_nn_combine (which skips them), but f^ must have been consumed by the regular
    // v-solve first when p_hat aliases it: order the scatter after it through the main stream
    hipc(hipEventRecord(P->ev_join, ss), "event record");
    hipc(hipStreamWaitEvent(st, P->ev_join, 0), "stream wait");
    if (P->use_chunked && P->low) hipc(hipStreamWaitEvent(st, P->ev_join_low, 0), "stream wait");
    if (ns > 0 && !P->use_chunked) {
        dim3 g(ns, (n + 63) / 64), blk(64);
        hipLaunchKernelGGL(k_sing_combine, g, blk, 0, st, P->s_u0.p, P->s_v0.p, P->s_u1.p, P->s_v1.p, P->s_du0.p, P->s_du1.p,
                           P->d_sing, ns, n, nxh, ny, p_hat, dp_hat);
    }
    hipc(hipGetLastError(), "poisson kernels");
}

int tlab_opr_poisson(tlab_poisson_plan_t P, int nx, int ny, int nz, int ibc, double *p, double *tmp1, double *tmp2,
                     const double *bcs_hb, const double *bcs_ht, double *dpdy) {
    return catch_fail([&]() -> int {
        if (!P || !p || !tmp1 || !tmp2 || !bcs_hb || !bcs_ht) throw Fail(TLAB_EINVAL, "tlab_opr_poisson: null argument");
        const tlab_poisson_plan::VFinal vf = P->vfinal;      // the request holds for THIS call only, whatever its outcome
        P->vfinal.armed = false;
        if (vf.armed && (!dpdy || !tlab_internal_poisson_can_v_final(P))) throw Fail(TLAB_EINVAL, "tlab_opr_poisson: internal: the fused v update was requested from a plan that cannot do it");
        if (nx != P->nx || ny != P->ny || nz != P->nz) throw Fail(TLAB_EINVAL, "tlab_opr_poisson: sizes do not match the plan");
        if (P->nproc != 1 || P->nxh != P->fx_nxh || P->fx_nz != P->nz)
            throw Fail(TLAB_EINVAL, "tlab_opr_poisson: plan is a z-slab / kx-pencil plan; drive its stages with the transposes in between");
        if (ibc != TLAB_BCS_NN && ibc != TLAB_BCS_DD && !P->direct) {
            tlab_set_error("OPR_Poisson (factorized): BCS_NN and BCS_DD only, like the reference (opr_elliptic.f90:312-331)");
            return TLAB_EUNSUPPORTED;
        }
        if (ibc < TLAB_BCS_DD || ibc > TLAB_BCS_NN) throw Fail(TLAB_EINVAL, "tlab_opr_poisson: bad ibc");
        if (p == tmp1 || p == tmp2 || tmp1 == tmp2 || dpdy == p || dpdy == tmp1 || dpdy == tmp2) throw Fail(TLAB_EINVAL, "arrays must be distinct");
        hipStream_t st = tlab_current_stream();
        wall_planes(P, p, bcs_hb, bcs_ht, nz, st);      // BC planes into the forcing (opr_elliptic.f90:285-286)
        P->forward_xz(p, tmp1, tmp2, st);
        if (P->direct) {    // OPR_Poisson_FourierXZ_Direct (opr_elliptic.f90:368-455)
            poisson_direct_stage(P, ibc, tmp1, tmp1, st);
            P->backward_xz(tmp1, p, st);
            if (dpdy) {     // :447-449, with the y plan of the derivatives
                const int rc = tlab_opr_partial(2, P->gy_der, TLAB_OPR_P1, nx, ny, nz, 0, p, dpdy, tmp1);
                if (rc != TLAB_OK) return rc;
            }
            return TLAB_OK;
        }
        if (ibc == TLAB_BCS_DD) poisson_dd_stage(P, tmp1, tmp1, tmp2, st);
        else poisson_ode_stage(P, tmp1, tmp1, tmp2, st);      // p^ -> tmp1 (over f^), dp^/dy -> tmp2
        P->backward_xz(tmp1, p, st);
        if (dpdy) P->backward_xz(tmp2, dpdy, st, &vf);
        return TLAB_OK;
    }, TLAB_EHIP);
}

// ---- stages, for the z-slab (multi-GPU) driver: the K-transposes of OPR_Fourier_Z_* (opr_fourier.f90:343-376) happen between them ----
int tlab_poisson_set_wall_planes(tlab_poisson_plan_t P, double *p, const double *bcs_hb, const double *bcs_ht) {
    return catch_fail([&]() -> int {
        if (!P || !p || !bcs_hb || !bcs_ht) throw Fail(TLAB_EINVAL, "null argument");
        wall_planes(P, p, bcs_hb, bcs_ht, P->fx_nz, tlab_current_stream());
        return TLAB_OK;
    }, TLAB_EHIP);
}
// dir = +1: real (nx,ny,kmax) -> complex (nx/2+1,ny,kmax)  [OPR_Fourier_X_Forward]; dir = -1: the inverse [OPR_Fourier_X_Backward]
// dir = -2: the inverse by the library's own kernel (k_fftx_c2r; the solver itself uses rocFFT's, which already runs at the copy rate) -- tests
int tlab_poisson_fft_x(tlab_poisson_plan_t P, int dir, double *in, double *out) {
    return catch_fail([&]() -> int {
        if (!P || !in || !out || in == out) throw Fail(TLAB_EINVAL, "tlab_poisson_fft_x: bad arguments");
        if (dir > 0) P->x_forward(in, out, tlab_current_stream());
        else if (dir == -2) {
            if (!P->fx_own) throw Fail(TLAB_EINVAL, "tlab_poisson_fft_x: no own transform for this length");
            P->fx_own->exec_inverse(in, out, tlab_current_stream());
        } else P->fx_c2r.exec(in, out, tlab_current_stream());
        return TLAB_OK;
    }, TLAB_EHIP);
}
// The x-transforms with the complex side in the pack layout of tlab_pencil_repack_blocks (the repack pass folded into the transform):
// dir = +1: real in (nx,ny,kmax) -> pack buffer out; dir = -1: pack buffer in -> real out.  Own kernels only.
static void packed_check(tlab_poisson_plan_t P, const void *a, const void *b, int nblocks, const int *start, const long long *base, const char *who) {
    if (!P || !a || !b || !start || !base || nblocks < 1 || nblocks > 16 || start[0] != 0) throw Fail(TLAB_EINVAL, std::string(who) + ": bad arguments");
    for (int p = 0; p + 1 < nblocks; ++p)
        if (start[p + 1] < start[p] || start[p + 1] > P->fx_nxh) throw Fail(TLAB_EINVAL, std::string(who) + ": block starts must increase within [0, nx/2+1]");
}
#define PACKED_NEEDS_OWN(P, who) if ((P) && !(P)->fx_own) { tlab_set_error(who ": no own transform for this length"); return TLAB_EUNSUPPORTED; }
int tlab_poisson_fft_x_packed(tlab_poisson_plan_t P, int dir, double *in, double *out, int nblocks, const int *start, const long long *base) {
    PACKED_NEEDS_OWN(P, "tlab_poisson_fft_x_packed")
    return catch_fail([&]() -> int {
        packed_check(P, in, out, nblocks, start, base, "tlab_poisson_fft_x_packed");
        if (in == out) throw Fail(TLAB_EINVAL, "tlab_poisson_fft_x_packed: out of place only");
        const auto &m = P->kx_map(nblocks, start, base);
        if (dir > 0) P->fx_own->exec(in, out, tlab_current_stream(), m.off, m.w);
        else P->fx_own->exec_inverse(in, out, tlab_current_stream(), m.off, m.w);
        return TLAB_OK;
    }, TLAB_EHIP);
}
// ... and the inverse of dp^/dy finishing the v equation (h = h - dp/dy, wall planes zeroed, q += dte h, h *= kco when scale) in its epilogue
int tlab_poisson_fft_x_packed_final(tlab_poisson_plan_t P, double *in, double *q, double *h, double dte, double kco, int scale, int nblocks,
                                    const int *start, const long long *base) {
    PACKED_NEEDS_OWN(P, "tlab_poisson_fft_x_packed_final")
    return catch_fail([&]() -> int {
        packed_check(P, in, q, nblocks, start, base, "tlab_poisson_fft_x_packed_final");
        if (!h) throw Fail(TLAB_EINVAL, "tlab_poisson_fft_x_packed_final: bad arguments");
        const auto &m = P->kx_map(nblocks, start, base);
        P->fx_own->exec_inverse_final(in, q, h, dte, kco, scale, (int)P->ny, tlab_current_stream(), m.off, m.w);
        return TLAB_OK;
    }, TLAB_EHIP);
}
// complex (nlines, nz_total) lines-fastest (the K-transposed layout; nlines = (nx/2+1)*ny/nproc_k), out of place; in == out with the own transform only
int tlab_poisson_fft_z(tlab_poisson_plan_t P, int dir, double *in, double *out) {
    return catch_fail([&]() -> int {
        if (!P || !in || !out || (in == out && !P->fz_own)) throw Fail(TLAB_EINVAL, "tlab_poisson_fft_z: bad arguments");
        if (P->nzt <= 1) throw Fail(TLAB_EINVAL, "tlab_poisson_fft_z: no z direction");
        P->z_exec(dir, in, out, tlab_current_stream());
        return TLAB_OK;
    }, TLAB_EHIP);
}
// per-mode ODE solves on the local (kx, kz) modes: f_hat -> p_hat (may alias f_hat), dp_hat
int tlab_poisson_ode(tlab_poisson_plan_t P, double *f_hat, double *p_hat, double *dp_hat) {
    return catch_fail([&]() -> int {
        if (!P || !f_hat || !p_hat || !dp_hat || dp_hat == f_hat || dp_hat == p_hat) throw Fail(TLAB_EINVAL, "tlab_poisson_ode: bad arguments");
        poisson_ode_stage(P, f_hat, p_hat, dp_hat, tlab_current_stream());
        return TLAB_OK;
    }, TLAB_EHIP);
}

// OPR_Helmholtz(nx, ny, nz, ibc, alpha, a, tmp1, tmp2, bcs_hb, bcs_ht): OPR_Helmholtz_FourierXZ_Direct (operators/opr_elliptic.f90:562-628) on a
// direct plan, OPR_Helmholtz_FourierXZ_Factorize (:466-557) on a factorized one
int tlab_opr_helmholtz(tlab_poisson_plan_t P, int nx, int ny, int nz, int ibc, double alpha, double *a, double *tmp1, double *tmp2,
                       const double *bcs_hb, const double *bcs_ht) {
    return catch_fail([&]() -> int {
        if (!P || !a || !tmp1 || !tmp2 || !bcs_hb || !bcs_ht) throw Fail(TLAB_EINVAL, "tlab_opr_helmholtz: null argument");
        if (nx != P->nx || ny != P->ny || nz != P->nz) throw Fail(TLAB_EINVAL, "tlab_opr_helmholtz: sizes do not match the plan");
        if (ibc < TLAB_BCS_DD || ibc > TLAB_BCS_NN) throw Fail(TLAB_EINVAL, "tlab_opr_helmholtz: bad ibc");
        if (a == tmp1 || a == tmp2 || tmp1 == tmp2) throw Fail(TLAB_EINVAL, "arrays must be distinct");
        tlab_poisson_plan *H = nullptr;
        if (!P->direct) {
            if (ibc != TLAB_BCS_NN && ibc != TLAB_BCS_DD) {
                tlab_set_error("OPR_Helmholtz (factorized): BCS_NN and BCS_DD only, like the reference (opr_elliptic.f90:524-532)");
                return TLAB_EUNSUPPORTED;
            }
            if (!P->g3[0] || P->helmholtz) throw Fail(TLAB_EINVAL, "tlab_opr_helmholtz: needs a single-device plan of tlab_poisson_plan_create");
            for (size_t i = 0; i < P->helm.size(); ++i)
                if (P->helm[i].first == alpha) {      // most recently used last
                    std::rotate(P->helm.begin() + i, P->helm.begin() + i + 1, P->helm.end());
                    H = P->helm.back().second.get();
                    break;
                }
            if (!H) {
                tlab_poisson_plan_t h = nullptr;
                const int rc = poisson_plan_create_impl(&h, P->g3[0], P->g3[1], P->g3[2], nx, ny, nz, nz, 0, 1, 0, 0, 0, nullptr, true, alpha);
                if (rc != TLAB_OK) return rc;
                if (P->helm.size() >= 4) P->helm.erase(P->helm.begin());
                P->helm.emplace_back(alpha, std::unique_ptr<tlab_poisson_plan>(h));
                H = h;
            }
        }
        hipStream_t st = tlab_current_stream();
        wall_planes(P, a, bcs_hb, bcs_ht, nz, st);
        P->forward_xz(a, tmp1, tmp2, st);
        if (P->direct) poisson_direct_stage(P, ibc, tmp1, tmp1, st, true, alpha);
        else if (ibc == TLAB_BCS_DD) poisson_dd_stage(H, tmp1, tmp1, tmp2, st);      // u over f^; v = u' + sqrt(lambda - alpha) u (not returned) in tmp2
        else poisson_ode_stage(H, tmp1, tmp1, tmp2, st);
        P->backward_xz(tmp1, a, st);
        return TLAB_OK;
    }, TLAB_EHIP);
}

// direct plans: FDM_Int2_Solve of the local modes, f_hat -> p_hat (may alias)
int tlab_poisson_direct_ode(tlab_poisson_plan_t P, int ibc, double *f_hat, double *p_hat) {
    return catch_fail([&]() -> int {
        if (!P || !f_hat || !p_hat) throw Fail(TLAB_EINVAL, "tlab_poisson_direct_ode: bad arguments");
        if (!P->direct) throw Fail(TLAB_EINVAL, "tlab_poisson_direct_ode: not a direct plan");
        if (ibc < TLAB_BCS_DD || ibc > TLAB_BCS_NN) throw Fail(TLAB_EINVAL, "tlab_poisson_direct_ode: bad ibc");
        poisson_direct_stage(P, ibc, f_hat, p_hat, tlab_current_stream());
        return TLAB_OK;
    }, TLAB_EHIP);
}


// include/tlab_amd.h: debug aid -- one FDM_Int1_Solve of the 3- / 7-diagonal path on the device (k_int1g), two lines per mode, for tests
int tlab_debug_int1_solve(tlab_fdm_plan_t gy, int ibc, int variant, int nm, const double *lam, const double *f, const double *bv, double *res, double *du) {
    return catch_fail([&]() -> int {
        if (!gy || !lam || !f || !bv || !res || !du || nm < 1 || (ibc != 1 && ibc != 2)) throw Fail(TLAB_EINVAL, "tlab_debug_int1_solve: bad arguments");
        if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called");
        const int n = gy->t.n;
        Int1Gen G;
        int1_generic_build(gy->t.der1, ibc, lam, nm, 1.0, G);
        DBuf fac, rb, rt, R, df, dbv, dres, ddu, scr;
        fac.upload(G.fac); rb.upload(G.rb); rt.upload(G.rt); R.upload(G.R);
        df.upload(std::vector<double>(f, f + (size_t)2 * n * nm));
        dbv.upload(std::vector<double>(bv, bv + (size_t)2 * nm));
        dres.alloc((size_t)2 * n * nm); ddu.alloc((size_t)2 * nm); scr.alloc((size_t)5 * n * nm);
        Int1Args a{};
        a.T.n = n; a.nm = nm; a.fscale = 1.0; a.fsrc = df.p; a.nlf = 2; a.bv_ptr = dbv.p; a.dst = dres.p; a.du = ddu.p; a.scratch = scr.p;
        a.g_fac = fac.p; a.g_rb = rb.p; a.g_rt = rt.p; a.g_R = R.p; a.g_ndi = G.ndi; a.g_nri = G.nri;
        hipStream_t st = tlab_current_stream();
        if (variant == 1) {                 // FS_UNIT variants of build_homogeneous / build_singular_homogeneous
            a.bv_ptr = nullptr; a.bv[0] = 0.0; a.bv[1] = 1.0; a.bv[2] = 0.0;
            if (ibc == 1) { a.unit_row = n - 1; launch_int1<1, 2, FS_UNIT>(a, st); }
            else { a.unit_row = 0; launch_int1<2, 2, FS_UNIT>(a, st); }
        } else if (variant == 2) {          // three lines, two stored (build_homogeneous, u-solve); ibc = 2
            DBuf d3, u3;
            d3.alloc((size_t)3 * n * nm); u3.alloc((size_t)3 * nm);
            a.bv_ptr = nullptr; a.bv[0] = 0.0; a.bv[1] = 0.0; a.bv[2] = 1.0;
            a.dst = d3.p; a.du = u3.p;
            launch_int1<2, 3, FS_LINEAR>(a, st);
            hipc(hipStreamSynchronize(st), "sync");
            hipc(hipMemcpy(dres.p, d3.p + (size_t)n * nm, (size_t)2 * n * nm * sizeof(double), hipMemcpyDeviceToDevice), "copy");      // lines 1, 2
            hipc(hipMemcpy(ddu.p, u3.p + (size_t)nm, (size_t)2 * nm * sizeof(double), hipMemcpyDeviceToDevice), "copy");
        } else if (ibc == 1) launch_int1<1, 2, FS_LINEAR>(a, st);
        else launch_int1<2, 2, FS_LINEAR>(a, st);
        hipc(hipStreamSynchronize(st), "sync");
        hipc(hipMemcpy(res, dres.p, (size_t)2 * n * nm * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
        hipc(hipMemcpy(du, ddu.p, (size_t)2 * nm * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy");
        return TLAB_OK;
    }, TLAB_EHIP);
}

}  // extern "C"

// ---- hooks of the RHS driver (rhs.cpp) ----
// The v equation needs dp/dy only as the operand of its final update: when the plan has the own x-transform and takes the 1-D transform route, the
// driver arms the NEXT tlab_opr_poisson call with (q, h, dte, kco, scale) and that call's last inverse transform finishes v instead of storing dp/dy.
bool tlab_internal_poisson_can_v_final(tlab_poisson_plan_t P) {
    static const bool on = env_int("TLAB_V_FINAL", 1) != 0;
    return on && P && P->fx_own && !P->use_2d && !P->direct && !P->helmholtz && P->nproc == 1;
}
void tlab_internal_poisson_arm_v_final(tlab_poisson_plan_t P, double *q, double *h, double dte, double kco, int scale) {
    P->vfinal.q = q; P->vfinal.h = h; P->vfinal.dte = dte; P->vfinal.kco = kco; P->vfinal.scale = scale; P->vfinal.armed = true;
}
